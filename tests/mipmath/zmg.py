"""TEST-ONLY helpers of tests/test_mipgen_{cpu,gpu}.py: a numpy restatement of include/zr_mipgen.h (written from the contract's text, not from the header),
the header on the host through zrh_mip_generate, a PNG writer (zlib + struct) that forces a row filter, a compression level and a strategy, and the Cornell
glTF rewritten with PNG images."""
import gzip
import json
import os
import shutil
import struct
import zlib

import numpy as np

from zetaray_amd import scene_io, wire

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF_GLTF = os.path.join(ROOT, "tests", "golden", "cornell_gltf")
FORMATS = {"rgba8_srgb": wire.TEX_RGBA8_SRGB, "rgba8": wire.TEX_RGBA8, "rg8": wire.TEX_RG8}


def channels(fmt):
    return 2 if fmt == wire.TEX_RG8 else 4


def full_mips(w, h):
    return 1 + int(np.floor(np.log2(max(w, h))))


def srgb_to_linear(c):
    c = np.asarray(c, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def linear_to_srgb(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.0031308, v * 12.92, 1.055 * np.power(np.maximum(v, 1e-30), 1 / 2.4) - 0.055)


# L[c] = round(65535 srgb_to_linear(c)), from the IEC formula in double
L16 = np.round(65535.0 * srgb_to_linear(np.arange(256))).astype(np.int64)


def taps(n, x):
    """the contract's table: (source indices, weights, denominator) of destination texel x of a source extent n"""
    m = max(1, n >> 1)
    if n == 1:
        return [0], [1], 1
    if n % 2 == 0:
        return [2 * x, 2 * x + 1], [1, 1], 2
    return [2 * x, 2 * x + 1, 2 * x + 2], [m - x, m, x + 1], n


def weights_matrix(n):
    """(max(1, n >> 1), n) integer matrix of the 1-D weights, and the denominator"""
    m = max(1, n >> 1)
    W = np.zeros((m, n), np.int64)
    den = 1
    for x in range(m):
        idx, w, den = taps(n, x)
        W[x, idx] = w
    return W, den


def sums(level, fmt):
    """S (per destination texel and channel, exact int64; sRGB channels in L16 units) and D of the level below `level` ((h, w, C) uint8)"""
    h, w, C = level.shape
    v = level.astype(np.int64)
    if fmt == wire.TEX_RGBA8_SRGB:
        v = np.concatenate([L16[level[..., :3]], v[..., 3:]], axis=2)
    Wy, dy = weights_matrix(h)
    Wx, dx = weights_matrix(w)
    return np.einsum("yj,xi,jic->yxc", Wy, Wx, v), dx * dy


def np_level(level, fmt):
    """the level below `level`, by the contract in numpy"""
    S, D = sums(level, fmt)
    out = (2 * S + D) // (2 * D)
    if fmt == wire.TEX_RGBA8_SRGB:
        T = (L16[:-1] + L16[1:]) * D      # code c is reached when 2 S >= (L[c - 1] + L[c]) D
        out[..., :3] = np.searchsorted(T, 2 * S[..., :3].reshape(-1), side="right").reshape(S[..., :3].shape)
    return out.astype(np.uint8)


def np_chain(level0, fmt, mips=None):
    h, w, _ = level0.shape
    out = [np.ascontiguousarray(level0, np.uint8)]
    for _ in range(1, full_mips(w, h) if mips is None else mips):
        out.append(np_level(out[-1], fmt))
    return out


def descs(rows):
    """rows of (offset, w, h, mips, fmt) -> wire.TEXTURE_DESC"""
    d = np.zeros(len(rows), wire.TEXTURE_DESC)
    for i, (off, w, h, mips, fmt) in enumerate(rows):
        d["offset"][i], d["width"][i], d["height"][i], d["num_mips"][i], d["format"][i] = off, w, h, mips, fmt
    return d


def chain_bytes(w, h, mips, fmt):
    return sum(max(1, w >> m) * max(1, h >> m) for m in range(mips)) * channels(fmt)


def header_chain(level0, fmt, mips=None):
    """include/zr_mipgen.h on the host (zrh_mip_generate) into an exact-size buffer: the levels as arrays"""
    h, w, C = level0.shape
    mips = full_mips(w, h) if mips is None else mips
    heap = np.zeros(chain_bytes(w, h, mips, fmt), np.uint8)
    heap[:level0.size] = level0.reshape(-1)
    scene_io.mip_generate(descs([(0, w, h, mips, fmt)]), heap)
    out, at = [], 0
    for m in range(mips):
        mw, mh = max(1, w >> m), max(1, h >> m)
        out.append(heap[at:at + mw * mh * C].reshape(mh, mw, C).copy())
        at += mw * mh * C
    return out


# ---------------------------------------------------------------------------------------------------- PNG files
def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def _filter_rows(raw, bpp, flt):
    """raw: (h, stride) uint8 -> the filtered rows, filter `flt` forced on every row (PNG specification, section 9)"""
    h, stride = raw.shape
    x = raw.astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if stride > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp] if stride > bpp else 0
    if flt == 0:
        pred = 0
    elif flt == 1:
        pred = a
    elif flt == 2:
        pred = b
    elif flt == 3:
        pred = (a + b) >> 1
    else:
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    body = ((x - pred) & 0xFF).astype(np.uint8)
    return np.concatenate([np.full((h, 1), flt, np.uint8), body], axis=1)


def png_bytes(samples, ctype, depth=8, flt=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, palette=None, trns=None, interlace=0, idat_split=None):
    """samples: (h, w, channels) of uint8 (depth 8) or uint16 (depth 16; written big endian); ctype 3: (h, w, 1) palette indices"""
    h, w, ch = samples.shape
    raw = (samples.astype(">u2") if depth == 16 else samples.astype(np.uint8)).tobytes()
    bpp = ch * (depth // 8) if depth >= 8 else 1
    raw = np.frombuffer(raw, np.uint8).reshape(h, -1)
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    z = co.compress(_filter_rows(raw, bpp, flt).tobytes()) + co.flush()
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if palette is not None:
        out += _chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += _chunk(b"tRNS", bytes(trns))
    out += _chunk(b"tEXt", b"Comment\0written by the test")
    parts = [z] if not idat_split else [z[i:i + idat_split] for i in range(0, len(z), idat_split)]
    for p in parts:
        out += _chunk(b"IDAT", p)
    return out + _chunk(b"IEND", b"")


def write_rgba_png(path, rgba):
    with open(path, "wb") as f:
        f.write(png_bytes(np.ascontiguousarray(rgba, np.uint8), 6, flt=4, level=9))


# ---------------------------------------------------------------------------------------------------- the Cornell glTF with PNG images
def cornell_png_gltf(tmp_path, rng):
    """tests/golden/cornell_gltf/cornell_emissive.gltf copied into tmp_path with its textured material given PNG maps -- a 37 x 21 base colour map
    (odd sizes), a 16 x 16 normal map, a 5 x 3 metallic-roughness map (an RG8 chain of 30 + 4 + 2 bytes) -- and another material given the fixture's own
    .dds as its base colour map, so the file mixes .dds and .png.  Returns (path, {"base" / "normal" / "mr": the (h, w, 4) RGBA arrays of the files})."""
    for f in ("cornell.bin",):
        shutil.copy(os.path.join(REF_GLTF, f), tmp_path / f)
    (tmp_path / "compressed").mkdir(exist_ok=True)
    with gzip.open(os.path.join(REF_GLTF, "compressed", "checkerboard.dds.gz"), "rb") as src:
        (tmp_path / "compressed" / "checkerboard.dds").write_bytes(src.read())
    g = json.load(open(os.path.join(REF_GLTF, "cornell_emissive.gltf")))
    files = {"base": rng.integers(0, 256, (21, 37, 4), dtype=np.uint8), "normal": rng.integers(0, 256, (16, 16, 4), dtype=np.uint8),
             "mr": rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)}
    for name, img in files.items():
        write_rgba_png(tmp_path / (name + ".png"), img)
    assert len(g["images"]) == 1 and len(g["textures"]) == 1
    g["images"] += [{"uri": name + ".png", "mimeType": "image/png"} for name in files]
    g["textures"] += [{"source": k, "sampler": 0} for k in (1, 2, 3)]
    textured = [m for m in g["materials"] if "baseColorTexture" in m.get("pbrMetallicRoughness", {})]
    assert len(textured) == 1
    m = textured[0]
    m["pbrMetallicRoughness"]["baseColorTexture"] = {"index": 1}
    m["pbrMetallicRoughness"]["metallicRoughnessTexture"] = {"index": 3}
    m["normalTexture"] = {"index": 2}
    other = next(x for x in g["materials"] if x is not m)
    other["pbrMetallicRoughness"]["baseColorTexture"] = {"index": 0}
    path = str(tmp_path / "cornell_png.gltf")
    json.dump(g, open(path, "w"))
    return path, files
