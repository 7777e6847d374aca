"""TEST-ONLY helpers of tests/test_jpeg_{cpu,gpu}.py: a numpy restatement of the JPEG contract of include/zr_jpeg.h, written from the contract's text and
not from the header -- a marker / Huffman reader in plain Python, dequantisation, the 13-bit integer IDCT, the triangle-filter upsampling, the
fixed-point colour conversion -- an expansion of the coefficient record, the fixture, and the Cornell glTF rewritten with JPEG images."""
import gzip
import json
import os
import shutil

import numpy as np

from zetaray_amd import wire

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF_GLTF = os.path.join(ROOT, "tests", "golden", "cornell_gltf")
FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")

# natural position of zigzag position k: walk the anti-diagonals
ZZ = []
for _s in range(15):
    _d = [(r, _s - r) for r in range(8) if 0 <= _s - r < 8]
    ZZ += [r * 8 + c for r, c in (_d if _s % 2 else _d[::-1])]
ZZ = np.array(ZZ)


def load_fixture():
    """[(name, file bytes, Pillow's decode as (h, w, 3) uint8 or None)] of tests/golden/jpeg_cases.npz (tools/make_jpeg_goldens.py)"""
    z = np.load(FIXTURE)
    out = []
    for i, name in enumerate(z["names"]):
        key = "d_%d" % i
        out.append((str(name), z["f_%d" % i].tobytes(), z[key] if key in z.files else None))
    return out


# ---------------------------------------------------------------------------------------------------- the sequential part
class _Bits:
    def __init__(self, data, pos):
        self.d, self.pos, self.buf, self.cnt = data, pos, 0, 0

    def bit(self):
        if self.cnt == 0:
            b = self.d[self.pos]
            self.pos += 1
            if b == 0xFF:
                assert self.d[self.pos] == 0, "a marker inside the entropy-coded data"
                self.pos += 1
            self.buf, self.cnt = b, 8
        self.cnt -= 1
        return (self.buf >> self.cnt) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def restart(self, k):
        self.cnt = 0
        assert self.d[self.pos] == 0xFF and self.d[self.pos + 1] == 0xD0 + (k & 7), "restart marker"
        self.pos += 2


def _huff(counts, symbols):
    """{(length, code): symbol} of a DHT table"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table


def _decode(bits, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | bits.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise AssertionError("no such Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def parse(data):
    """A baseline JPEG file -> dict(w, h, comps=[dict(hs, vs, q (64, zigzag order), blocks (bh, bw, 64) quantised, zigzag order)]); blocks padded to
    whole MCUs as the scan holds them"""
    d = bytes(data)
    assert d[:2] == b"\xff\xd8"
    at, qt, dc, ac, restart, frame = 2, {}, {}, {}, 0, None
    while True:
        assert d[at] == 0xFF
        m = d[at + 1]
        n = (d[at + 2] << 8) | d[at + 3]
        seg = d[at + 4:at + 2 + n]
        if m in (0xC0, 0xC1):
            assert seg[0] == 8
            frame = dict(h=(seg[1] << 8) | seg[2], w=(seg[3] << 8) | seg[4],
                         comps=[dict(id=seg[6 + 3 * c], hs=seg[7 + 3 * c] >> 4, vs=seg[7 + 3 * c] & 15, tq=seg[8 + 3 * c]) for c in range(seg[5])])
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                counts = list(seg[p + 1:p + 17])
                (ac if seg[p] >> 4 else dc)[seg[p] & 15] = _huff(counts, seg[p + 17:p + 17 + sum(counts)])
                p += 17 + sum(counts)
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    qt[seg[p] & 15] = np.frombuffer(seg[p + 1:p + 129], ">u2").astype(np.int64)
                    p += 129
                else:
                    qt[seg[p] & 15] = np.frombuffer(seg[p + 1:p + 65], np.uint8).astype(np.int64)
                    p += 65
        elif m == 0xDD:
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            break
        else:
            assert m not in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not a sequential Huffman file"
        at += 2 + n
    comps = frame["comps"]
    assert seg[0] == len(comps)
    if len(comps) == 1:
        comps[0]["hs"] = comps[0]["vs"] = 1
    hmax, vmax = max(c["hs"] for c in comps), max(c["vs"] for c in comps)
    mx, my = -(-frame["w"] // (8 * hmax)), -(-frame["h"] // (8 * vmax))
    for k, c in enumerate(comps):
        c["td"], c["ta"] = dc[seg[2 + 2 * k] >> 4], ac[seg[2 + 2 * k] & 15]
        c["q"] = qt[c["tq"]]
        c["blocks"] = np.zeros((my * c["vs"], mx * c["hs"], 64), np.int64)
        c["pred"] = 0
    bits = _Bits(d, at + 2 + n)
    count = 0
    for y in range(my):
        for x in range(mx):
            if restart and count and count % restart == 0:
                bits.restart(count // restart - 1)
                for c in comps:
                    c["pred"] = 0
            count += 1
            for c in comps:
                for v in range(c["vs"]):
                    for h in range(c["hs"]):
                        blk = c["blocks"][y * c["vs"] + v, x * c["hs"] + h]
                        s = _decode(bits, c["td"])
                        c["pred"] += _extend(bits.bits(s), s)
                        blk[0] = c["pred"]
                        k = 1
                        while k < 64:
                            rs = _decode(bits, c["ta"])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[k] = _extend(bits.bits(s), s)
                            k += 1
    return dict(w=frame["w"], h=frame["h"], comps=[dict(hs=c["hs"], vs=c["vs"], q=c["q"], blocks=c["blocks"]) for c in comps])


# ---------------------------------------------------------------------------------------------------- the arithmetic of the contract
def _i32(x):
    return np.asarray(x).astype(np.int64).astype(np.int32)      # wrap to 32 bits


def _pass(v, n):
    """one IDCT pass along the last axis of an int32 array (.., 8), descaled by n bits; every sum and product wraps in 32 bits"""
    with np.errstate(over="ignore"):
        i = [v[..., k].astype(np.int32) for k in range(8)]
        c = np.int32
        z1 = (i[2] + i[6]) * c(4433)
        t2 = z1 - i[6] * c(15137)
        t3 = z1 + i[2] * c(6270)
        t0 = (i[0] + i[4]) << c(13)
        t1 = (i[0] - i[4]) << c(13)
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
        z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
        z5 = (z3 + z4) * c(9633)
        a0, a1, a2, a3 = a0 * c(2446), a1 * c(16819), a2 * c(25172), a3 * c(12299)
        z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069), z4 * c(-3196)
        z3, z4 = z3 + z5, z4 + z5
        a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
        outs = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
        return np.stack([(o + c(1 << (n - 1))) >> c(n) for o in outs], axis=-1)


def idct(coef):
    """(.., 8, 8) dequantised coefficients in natural order (row, column) -> (.., 8, 8) samples, uint8: columns then rows, + 128, clamped"""
    v = _i32(coef)
    v = np.swapaxes(_pass(np.swapaxes(v, -1, -2), 11), -1, -2)      # columns: along the row index
    v = _pass(v, 18)
    return np.clip(v.astype(np.int64) + 128, 0, 255).astype(np.uint8)


def component_plane(q, blocks):
    """quantised blocks (bh, bw, 64) in zigzag order and their table -> the sample plane (8 bh, 8 bw)"""
    bh, bw, _ = blocks.shape
    with np.errstate(over="ignore"):
        deq = _i32(blocks) * _i32(q)
    nat = np.zeros((bh, bw, 64), np.int32)
    nat[..., ZZ] = deq
    s = idct(nat.reshape(bh, bw, 8, 8))
    return s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _up_h2v1(s, w):
    """s: (rows, n) real samples -> (rows, w)"""
    s = s.astype(np.int64)
    n = s.shape[1]
    if n <= 2:      # (libjpeg filters only components wider than 2 samples)
        return np.repeat(s, 2, axis=1)[:, :w]
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    o = np.zeros((s.shape[0], 2 * n), np.int64)
    o[:, 0::2] = (3 * s + left + 1) >> 2
    o[:, 1::2] = (3 * s + right + 2) >> 2
    o[:, 0], o[:, -1] = s[:, 0], s[:, -1]
    return o[:, :w]


def _up_h2v2(s, w, h):
    """s: (rows, n) real samples -> (h, w)"""
    s = s.astype(np.int64)
    rows, n = s.shape
    if n <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)[:h, :w]
    above = np.concatenate([s[:1], s[:-1]], axis=0)
    below = np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.zeros((2 * rows, 2 * n), np.int64)
    for k, other in ((0, above), (1, below)):
        cs = 3 * s + other
        left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        o = np.zeros((rows, 2 * n), np.int64)
        o[:, 0::2] = (3 * cs + left + 8) >> 4
        o[:, 1::2] = (3 * cs + right + 7) >> 4
        o[:, 0], o[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        out[k::2] = o
    return out[:h, :w]


def assemble(w, h, comps, planes):
    """sample planes -> (h, w, 4) uint8 RGBA"""
    y = planes[0][:h, :w].astype(np.int64)
    if len(comps) == 1:
        return np.stack([y, y, y, np.full_like(y, 255)], axis=2).astype(np.uint8)
    hs, vs = comps[0]["hs"], comps[0]["vs"]
    n, rows = -(-w // hs), -(-h // vs)      # the real samples of a chroma component
    ch = []
    for p in planes[1:]:
        s = p[:rows, :n]
        ch.append(s.astype(np.int64) if hs == 1 else (_up_h2v1(s, w) if vs == 1 else _up_h2v2(s, w, h)))
    cb, cr = ch[0] - 128, ch[1] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.stack([np.clip(r, 0, 255), np.clip(g, 0, 255), np.clip(b, 0, 255), np.full_like(y, 255)], axis=2).astype(np.uint8)


def decode(data):
    """the whole contract: a JPEG file -> (h, w, 4) uint8 RGBA"""
    p = parse(data)
    return assemble(p["w"], p["h"], p["comps"], [component_plane(c["q"], c["blocks"]) for c in p["comps"]])


def apply_map(rgba, channel_map):
    if channel_map == wire.JPEG_MAP_RGBA:
        return rgba
    return np.ascontiguousarray(rgba[..., [0, 1]] if channel_map == wire.JPEG_MAP_RG else rgba[..., [2, 1]])


# ---------------------------------------------------------------------------------------------------- the record
HEADER = np.dtype([("magic", "<u4"), ("pad0", "<u4"), ("bytes", "<u8"), ("w", "<u4"), ("h", "<u4"), ("ncomp", "<u4"), ("map", "<u4"), ("num_blocks", "<u4"),
                   ("pad1", "<u4"), ("comp", [("hs", "<u4"), ("vs", "<u4"), ("bw", "<u4"), ("bh", "<u4"), ("first_block", "<u4"), ("pad", "<u4"), ("q", "<u2", 64)], 3)])
MAGIC = 0x47504A5A
assert HEADER.itemsize == 496


def record_header(record):
    return np.frombuffer(np.ascontiguousarray(record, np.uint8)[:496].tobytes(), HEADER)[0]


def expand_record(record):
    """a record of scene_io.pack_jpeg -> the texels of its channel map, through the numpy contract above (not through the header)"""
    rec = np.ascontiguousarray(record, np.uint8)
    h = record_header(rec)
    assert int(h["magic"]) == MAGIC and int(h["bytes"]) <= len(rec)
    B = int(h["num_blocks"])
    begin = np.frombuffer(rec[496:496 + 4 * (B + 1)].tobytes(), "<u4").astype(np.int64)
    coef = np.frombuffer(rec[496 + 4 * (B + 1):496 + 4 * (B + 1) + 2 * int(begin[-1])].tobytes(), "<i2")
    assert begin[0] == 0 and (np.diff(begin) >= 1).all() and (np.diff(begin) <= 64).all()
    comps, planes = [], []
    for c in h["comp"][:int(h["ncomp"])]:
        bw, bh, first = int(c["bw"]), int(c["bh"]), int(c["first_block"])
        blocks = np.zeros((bh * bw, 64), np.int64)
        for b in range(bh * bw):
            run = coef[begin[first + b]:begin[first + b + 1]]
            blocks[b, :len(run)] = run
        comps.append(dict(hs=int(c["hs"]), vs=int(c["vs"])))
        planes.append(component_plane(c["q"].astype(np.int64), blocks.reshape(bh, bw, 64)))
    return apply_map(assemble(int(h["w"]), int(h["h"]), comps, planes), int(h["map"]))


# ---------------------------------------------------------------------------------------------------- the Cornell glTF with JPEG images
def cornell_jpeg_gltf(tmp_path, files=None):
    """tests/golden/cornell_gltf/cornell_emissive.gltf copied into tmp_path with its textured material given JPEG maps from the fixture -- a 33 x 17 4:2:0
    base colour map, a 16 x 16 4:4:4 normal map, a 7 x 5 4:2:2 metallic-roughness map -- and another material given the fixture's own .dds as its base
    colour map, so the file mixes .dds and .jpg.  Returns (path, {"base" / "normal" / "mr": the file bytes})."""
    fx = {name: data for name, data, _ in load_fixture()}
    files = files or {"base": fx["33x17_420_q90_noise"], "normal": fx["16x16_444_q100_smooth"], "mr": fx["7x5_422_q90_noise"]}
    shutil.copy(os.path.join(REF_GLTF, "cornell.bin"), tmp_path / "cornell.bin")
    (tmp_path / "compressed").mkdir(exist_ok=True)
    with gzip.open(os.path.join(REF_GLTF, "compressed", "checkerboard.dds.gz"), "rb") as src:
        (tmp_path / "compressed" / "checkerboard.dds").write_bytes(src.read())
    g = json.load(open(os.path.join(REF_GLTF, "cornell_emissive.gltf")))
    ext = {"base": ".jpg", "normal": ".jpeg", "mr": ".JPG"}
    for name, data in files.items():
        (tmp_path / (name + ext[name])).write_bytes(data)
    assert len(g["images"]) == 1 and len(g["textures"]) == 1
    g["images"] += [{"uri": name + ext[name], "mimeType": "image/jpeg"} for name in files]
    g["textures"] += [{"source": k, "sampler": 0} for k in (1, 2, 3)]
    textured = [m for m in g["materials"] if "baseColorTexture" in m.get("pbrMetallicRoughness", {})]
    assert len(textured) == 1
    m = textured[0]
    m["pbrMetallicRoughness"]["baseColorTexture"] = {"index": 1}
    m["pbrMetallicRoughness"]["metallicRoughnessTexture"] = {"index": 3}
    m["normalTexture"] = {"index": 2}
    other = next(x for x in g["materials"] if x is not m)
    other["pbrMetallicRoughness"]["baseColorTexture"] = {"index": 0}
    path = str(tmp_path / "cornell_jpeg.gltf")
    json.dump(g, open(path, "w"))
    return path, files


# ---------------------------------------------------------------------------------------------------- records and files made by the tests
def make_gray_record(blocks, bw, bh, q=None, w=None, h=None, channel_map=wire.JPEG_MAP_RGBA):
    """blocks: (bh * bw, 64) integer coefficients in NATURAL order, already quantised -> the record of a one-component image of bw x bh blocks"""
    blocks = np.asarray(blocks, np.int64).reshape(bh * bw, 64)
    zz = blocks[:, ZZ]
    n = np.maximum(1, 64 - np.argmax(zz[:, ::-1] != 0, axis=1))
    n[~(zz != 0).any(axis=1)] = 1
    begin = np.concatenate([[0], np.cumsum(n)]).astype("<u4")
    coef = zz[np.arange(64)[None, :] < n[:, None]].astype("<i2")
    hdr = np.zeros(1, HEADER)
    hdr["magic"], hdr["w"], hdr["h"], hdr["ncomp"], hdr["map"], hdr["num_blocks"] = MAGIC, w or 8 * bw, h or 8 * bh, 1, channel_map, bw * bh
    c = hdr["comp"][0][0]
    c["hs"], c["vs"], c["bw"], c["bh"], c["first_block"] = 1, 1, bw, bh, 0
    c["q"] = np.ones(64, np.uint16) if q is None else q
    hdr["bytes"] = 496 + begin.nbytes + coef.nbytes
    raw = hdr.tobytes() + begin.tobytes() + coef.tobytes()
    return np.frombuffer(raw + bytes(-len(raw) % 16), np.uint8).copy()


def segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def tiny_gray_jpeg(scan, w=8, h=8, dc=((1,), (0,)), ac=((1,), (0xF1,)), extra=b""):
    """a one-component file put together by hand: DHT tables given as (counts of lengths 1 .., symbols), one scan with the bytes `scan`"""
    def dht(cls, t):
        counts = list(t[0]) + [0] * (16 - len(t[0]))
        return segment(0xC4, bytes([cls << 4]) + bytes(counts) + bytes(t[1]))
    sof = segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([1, 1, 0x11, 0]))
    return b"\xff\xd8" + extra + segment(0xDB, bytes([0]) + bytes([1] * 64)) + sof + dht(0, dc) + dht(1, ac) + segment(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + bytes(scan) + b"\xff\xd9"


def five_encoding_box(rng):
    """The untextured Cornell box with a map of every source encoding, at sizes on the seams: a 5 x 3 RG8 RAW_MIP0 map, a 37 x 21 sRGB RAW map with its
    stored chain, a 4 x 4 BC7 map of 3 mips, a 33 x 17 4:2:0 JPEG as an sRGB map and a grey 17 x 23 JPEG as an RG8 map of 2 mips (level 0 from the record,
    the rest generated), and a 5 x 3 BC5 map.  The chains are then moved: they lie in the heap in another order than the textures, 8 bytes of padding in
    front, 4 .. 44 bytes between them and 24 behind the last.  Returns (scene, the order of the chains in the heap)."""
    from tests.bcnmath import zbc
    from tests.mipmath import zmg
    from zetaray_amd import scene_io
    fx = {name: data for name, data, _ in load_fixture()}
    sc = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))

    def blocks(w, h, mips):
        return rng.integers(0, 256, 16 * sum(zbc.mip_blocks(max(1, w >> m), max(1, h >> m)) for m in range(mips)), dtype=np.uint8)

    sc.add_texture_blocks(rng.integers(0, 256, 5 * 3 * 2, dtype=np.uint8), 5, 3, zmg.full_mips(5, 3), wire.TEX_RG8, wire.TEX_SRC_RAW_MIP0)
    mips = zmg.full_mips(37, 21)
    sc.add_texture_blocks(rng.integers(0, 256, zmg.chain_bytes(37, 21, mips, wire.TEX_RGBA8_SRGB), dtype=np.uint8), 37, 21, mips, wire.TEX_RGBA8_SRGB, wire.TEX_SRC_RAW)
    sc.add_texture_blocks(blocks(4, 4, 3), 4, 4, 3, wire.TEX_RGBA8, wire.TEX_SRC_BC7)
    sc.add_texture_blocks(scene_io.pack_jpeg(fx["33x17_420_q90_noise"], "a.jpg"), 33, 17, zmg.full_mips(33, 17), wire.TEX_RGBA8_SRGB, wire.TEX_SRC_JPEG_COEF)
    sc.add_texture_blocks(scene_io.pack_jpeg(fx["17x23_gray_restart_rows"], "b.jpg", wire.JPEG_MAP_RG), 17, 23, 2, wire.TEX_RG8, wire.TEX_SRC_JPEG_COEF)
    sc.add_texture_blocks(blocks(5, 3, 3), 5, 3, 3, wire.TEX_RG8, wire.TEX_SRC_BC5)
    order, at = [3, 0, 5, 2, 4, 1], 8
    for k, i in enumerate(order):
        t = sc.textures[i]
        sc.textures["offset"][i] = at
        at += zmg.chain_bytes(int(t["width"]), int(t["height"]), int(t["num_mips"]), int(t["format"]))
        at = (at + 3) // 4 * 4 + (4 + 8 * k if k + 1 < len(order) else 24)
    sc.texel_heap_bytes = at
    return sc, order
