"""JPEG loading on the host: include/zr_jpeg.h (through zrh_jpeg_decode / zrh_jpeg_pack / zrh_jpeg_expand) against a numpy restatement of its contract
(tests/jpegmath/zjp.py), against Pillow's decode of files Pillow wrote (tests/golden/jpeg_cases.npz, tools/make_jpeg_goldens.py) and against a float64 IDCT;
every refusal; load_gltf_native on a glTF with JPEG images in both texture modes.  No GPU."""
import io
import json

import numpy as np
import pytest

from tests.jpegmath import zjp
from tests.mipmath import zmg
from zetaray_amd import scene_io, wire

FIXTURE = zjp.load_fixture()
GOOD = [(n, d, w) for n, d, w in FIXTURE if w is not None]
FILES = {n: d for n, d, _ in FIXTURE}


def test_constants_and_fixture():
    assert wire.TEX_SRC_JPEG_COEF == 16 and scene_io.LOAD_JPEG == 2 and scene_io.LOAD_KEEP_COMPRESSED == 1
    assert (wire.JPEG_MAP_RGBA, wire.JPEG_MAP_RG, wire.JPEG_MAP_BG) == (0, 1, 2)
    names = [n for n, _, _ in FIXTURE]
    sizes = {n.split("_")[0] for n in names}
    assert {"1x1", "7x5", "8x8", "9x9", "16x16", "17x23", "33x17", "2x40"} <= sizes
    for tag in ("gray", "444", "422", "420", "q30", "q90", "q100", "optimize", "restart_blocks", "restart_rows", "qtables", "progressive", "cmyk"):
        assert any(tag in n for n in names), tag
    assert len(GOOD) >= 40


# ---- 1. header == numpy contract == Pillow's bytes, on every file
@pytest.mark.parametrize("case", GOOD, ids=[c[0] for c in GOOD])
def test_header_equals_the_contract_and_pillow(case):
    name, data, want = case
    got = scene_io.decode_jpeg(data, name + ".jpg")
    assert got.shape == want.shape[:2] + (4,) and (got[..., 3] == 255).all()
    assert np.array_equal(got[..., :3], want), ("the fixture (Pillow's decode)", int(np.abs(got[..., :3].astype(int) - want).max()))
    assert np.array_equal(got, zjp.decode(data)), "the numpy contract"
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        live = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert np.array_equal(got[..., :3], live), "Pillow, live"
    # the entropy decode alone, expanded by the numpy contract and by the header, in the three channel maps
    for cmap in (wire.JPEG_MAP_RGBA, wire.JPEG_MAP_RG, wire.JPEG_MAP_BG):
        rec = scene_io.pack_jpeg(data, name + ".jpg", cmap)
        assert len(rec) % 16 == 0
        h = zjp.record_header(rec)
        assert int(h["magic"]) == zjp.MAGIC and int(h["map"]) == cmap and (int(h["w"]), int(h["h"])) == (want.shape[1], want.shape[0])
        assert len(rec) - 15 <= int(h["bytes"]) <= len(rec)
        expect = zjp.apply_map(got, cmap)
        assert np.array_equal(zjp.expand_record(rec), expect), ("pack + numpy expansion", cmap)
        assert np.array_equal(scene_io.jpeg_expand(rec), expect), ("pack + header expansion", cmap)


def test_record_stores_leading_coefficients_only():
    data = FILES["33x17_420_q90_noise"]
    rec = scene_io.pack_jpeg(data)
    h = zjp.record_header(rec)
    p = zjp.parse(data)
    B = int(h["num_blocks"])
    assert B == sum(c["blocks"].shape[0] * c["blocks"].shape[1] for c in p["comps"]) == 3 * 2 * (4 + 1 + 1)
    begin = np.frombuffer(rec[496:496 + 4 * (B + 1)].tobytes(), "<u4").astype(np.int64)
    coef = np.frombuffer(rec[496 + 4 * (B + 1):496 + 4 * (B + 1) + 2 * int(begin[-1])].tobytes(), "<i2")
    b = 0
    for c, hc in zip(p["comps"], h["comp"]):
        assert np.array_equal(hc["q"], c["q"]) and int(hc["first_block"]) == b and (int(hc["bh"]), int(hc["bw"])) == c["blocks"].shape[:2]
        for blk in c["blocks"].reshape(-1, 64):
            nz = np.nonzero(blk)[0]
            n = int(nz[-1]) + 1 if len(nz) else 1
            assert begin[b + 1] - begin[b] == n and np.array_equal(coef[begin[b]:begin[b + 1]], blk[:n])
            b += 1
    smooth = scene_io.pack_jpeg(FILES["64x64_420_q90_bench"])
    blocks = int(zjp.record_header(smooth)["num_blocks"])
    assert (len(smooth) - 496 - 4 * (blocks + 1)) / blocks < 64, "a typical block is a few dozen bytes, not 128"


# ---- 2. the IDCT alone against float64, by the IEEE 1180-1990 procedure
def _dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    c = np.cos((2 * n + 1) * k * np.pi / 16) * 0.5
    c[0] /= np.sqrt(2.0)
    return c


@pytest.mark.parametrize("lo,hi", [(-256, 255), (-5, 5), (-300, 300)])
@pytest.mark.parametrize("sign", [1, -1])
def test_idct_accuracy_ieee_1180(lo, hi, sign):
    """10 000 random blocks: forward DCT in float64, rounded and clipped to 12 bits; the header's IDCT (a one-component record with a unit table,
    expanded by zrh_jpeg_expand) against the float64 IDCT of the same integers, rounded.  The header's output is an 8-bit sample (+ 128, clamped), so
    both sides are compared after that clamp."""
    rng = np.random.default_rng(1180 + hi)
    C = _dct_matrix()
    x = sign * rng.integers(lo, hi + 1, (10000, 8, 8)).astype(np.float64)
    coef = np.clip(np.floor(C @ x @ C.T + 0.5), -2048, 2047)
    ref = np.clip(np.floor(C.T @ coef @ C + 0.5) + 128, 0, 255)
    rec = zjp.make_gray_record(coef.reshape(-1, 64), 100, 100)
    got = scene_io.jpeg_expand(rec)[..., 0].reshape(100, 8, 100, 8).transpose(0, 2, 1, 3).reshape(10000, 8, 8).astype(np.float64)
    err = got - ref
    figures = dict(peak=np.abs(err).max(), pmse=(err ** 2).mean(axis=0).max(), omse=(err ** 2).mean(), pme=np.abs(err.mean(axis=0)).max(), ome=abs(err.mean()))
    print(lo, hi, sign, figures)
    assert figures["peak"] <= 1 and figures["pmse"] <= 0.06 and figures["omse"] <= 0.02 and figures["pme"] <= 0.015 and figures["ome"] <= 0.0015, figures


def test_idct_of_zero_is_128():
    out = scene_io.jpeg_expand(zjp.make_gray_record(np.zeros((6, 64)), 3, 2))
    assert out.shape == (16, 24, 4) and (out[..., :3] == 128).all() and (out[..., 3] == 255).all()


def test_idct_wraps_in_32_bits_like_the_contract():
    """coefficients and tables no conforming file holds: defined all the same, and the numpy contract (int32 wrap-around) gives the same samples"""
    rng = np.random.default_rng(5)
    blocks = rng.integers(-32768, 32768, (12, 64))
    q = rng.integers(1, 65536, 64).astype(np.uint16)
    rec = zjp.make_gray_record(blocks, 4, 3, q=q, w=29, h=19)
    assert np.array_equal(scene_io.jpeg_expand(rec), zjp.expand_record(rec))


# ---- 3. refusals: each names the file and the reason
def _refused(data, *words, name="some/dir/photo.jpg"):
    for call in (scene_io.decode_jpeg, scene_io.pack_jpeg):
        with pytest.raises(RuntimeError) as e:
            call(data, name)
        msg = str(e.value)
        assert name in msg and all(w in msg for w in words), msg


def _patched(data, marker, offset, value):
    """byte `offset` of the body of the first segment with `marker` replaced"""
    at = data.index(bytes([0xFF, marker]))
    b = bytearray(data)
    b[at + 4 + offset] = value
    return bytes(b)


def test_jpeg_refusals():
    colour, gray = FILES["16x16_444_q100_smooth"], FILES["17x23_gray_restart_rows"]
    scene_io.decode_jpeg(colour)
    _refused(FILES["16x16_progressive"], "progressive")
    _refused(FILES["16x16_cmyk"], "4-component")
    sof = colour.index(b"\xff\xc0")
    for marker, word in ((0xC9, "arithmetic"), (0xCA, "arithmetic"), (0xC3, "lossless"), (0xC5, "hierarchical"), (0xC2, "progressive")):
        _refused(colour[:sof + 1] + bytes([marker]) + colour[sof + 2:], word)
    _refused(_patched(colour, 0xC0, 0, 12), "12-bit")
    _refused(_patched(colour, 0xC0, 7, 0x41), "sampling")      # 4:1:1
    _refused(_patched(colour, 0xC0, 7, 0x12), "sampling")      # 4:4:0
    _refused(_patched(_patched(colour, 0xC0, 1, 0), 0xC0, 2, 0), "dimensions", "[1, 65535]")
    _refused(_patched(_patched(colour, 0xC0, 3, 0), 0xC0, 4, 0), "dimensions", "[1, 65535]")
    # a header that promises more blocks than the bytes can hold: 65535 x 65535 in a file of a few hundred bytes
    big = colour
    for off in (1, 2, 3, 4):
        big = _patched(big, 0xC0, off, 0xFF)
    _refused(big, "truncated", "more blocks")
    # an Adobe APP14 segment with transform 0: RGB, not YCbCr
    _refused(colour[:2] + zjp.segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00") + colour[2:], "RGB")
    assert scene_io.decode_jpeg(colour[:2] + zjp.segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01") + zjp.segment(0xFE, b"a comment") + colour[2:]).shape == (16, 16, 4)
    # a scan that holds one of the three components
    sos = colour.index(b"\xff\xda")
    _refused(colour[:sos] + zjp.segment(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + colour[sos + 14:], "several scans")
    # data that ends early; a file cut inside its headers
    scan = sos + 14
    for cut in (scan + 1, scan + (len(colour) - scan) // 2):
        _refused(colour[:cut], "truncated")
    for cut in (sos + 5, sof + 6, 4):
        _refused(colour[:cut], "truncated")
    _refused(colour[:3], "not a JPEG")
    _refused(b"\x89PNG\r\n\x1a\n" + colour[8:], "not a JPEG")
    # a Huffman code that is not in the table: sixteen 1-bits
    _refused(colour[:scan] + b"\xff\x00" * 40 + b"\xff\xd9", "not in the table")
    # a coefficient index past 63: DC size 0, then four (run 15, size 1) codes
    assert scene_io.decode_jpeg(zjp.tiny_gray_jpeg(b"\x3f", ac=((1, 1), (0x00, 0xF1)))).shape == (8, 8, 4)
    _refused(zjp.tiny_gray_jpeg(b"\x2a\x00"), "index past 63")
    # a restart marker with the wrong number, and one that is missing
    rst = gray.index(b"\xff\xd0", gray.index(b"\xff\xda"))
    _refused(gray[:rst + 1] + b"\xd3" + gray[rst + 2:], "restart marker")
    _refused(gray[:rst] + gray[rst + 2:], "restart marker")


# ---- 4. the loader
def _level0(sc, i):
    t = sc.textures[i]
    n = int(t["width"]) * int(t["height"]) * zmg.channels(int(t["format"]))
    return sc.texels[int(t["offset"]):int(t["offset"]) + n].reshape(int(t["height"]), int(t["width"]), -1)


def test_loader_both_modes(tmp_path):
    path, files = zjp.cornell_jpeg_gltf(tmp_path)
    dec, offs = scene_io.load_gltf_native(path, jpeg=True)
    cmp_, offs2 = scene_io.load_gltf_native(path, textures="compressed", jpeg=True)
    assert offs == offs2 and len(dec.textures) == 4 and np.array_equal(dec.textures, cmp_.textures)
    assert len(cmp_.texels) == 0 and cmp_.texel_heap_bytes == len(dec.texels)
    assert [int(offs[k]) for k in ("base_color", "normal", "metallic_roughness", "emissive")] == [0, 2, 3, 4]
    enc = [int(e) for e in cmp_.texture_sources["encoding"]]
    assert sorted(enc[:2]) == [wire.TEX_SRC_BC7, wire.TEX_SRC_JPEG_COEF] and enc[2:] == [wire.TEX_SRC_JPEG_COEF] * 2
    base = enc.index(wire.TEX_SRC_JPEG_COEF)
    rgba = {k: zjp.decode(v) for k, v in files.items()}
    for i, name, fmt in ((base, "base", wire.TEX_RGBA8_SRGB), (2, "normal", wire.TEX_RG8), (3, "mr", wire.TEX_RG8)):
        t = dec.textures[i]
        h, w, _ = rgba[name].shape
        assert (int(t["width"]), int(t["height"]), int(t["format"])) == (w, h, fmt)
        assert int(t["num_mips"]) == 1 + int(np.floor(np.log2(max(w, h)))), name
    assert np.array_equal(_level0(dec, base), rgba["base"])
    assert np.array_equal(_level0(dec, 2), rgba["normal"][..., [0, 1]]), "a normal map keeps the file's (R, G)"
    assert np.array_equal(_level0(dec, 3), rgba["mr"][..., [2, 1]]), "a metallic-roughness map keeps the file's (B, G)"
    for i, fmt in ((base, wire.TEX_RGBA8_SRGB), (2, wire.TEX_RG8), (3, wire.TEX_RG8)):
        t = dec.textures[i]
        want = np.concatenate([m.reshape(-1) for m in zmg.np_chain(_level0(dec, i), fmt)])
        assert np.array_equal(dec.texels[int(t["offset"]):int(t["offset"]) + len(want)], want), i
    # the records name their slots' channel maps, and the payload rebuilds the default mode's heap
    maps = [int(zjp.record_header(cmp_.texture_payload[int(s["offset"]):])["map"]) for s in cmp_.texture_sources if int(s["encoding"]) == wire.TEX_SRC_JPEG_COEF]
    assert maps == [wire.JPEG_MAP_RGBA, wire.JPEG_MAP_RG, wire.JPEG_MAP_BG]
    cmp_.decode_textures()
    assert np.array_equal(cmp_.texels, dec.texels)
    assert len(cmp_.texture_payload) < len(dec.texels)


def test_without_the_flag_jpeg_is_refused_with_the_same_words(tmp_path):
    path, _ = zjp.cornell_jpeg_gltf(tmp_path)
    for kw in ({}, {"textures": "compressed"}, {"jpeg": False}):
        with pytest.raises(RuntimeError) as e:
            scene_io.load_gltf_native(path, **kw)
        assert str(e.value) == "glTF: image 'base.jpg': JPEG images are not supported (.dds and .png are)", str(e.value)
    # with it, a file the decoder refuses names its path and the reason
    g = json.load(open(path))
    (tmp_path / "prog.jpg").write_bytes(FILES["16x16_progressive"])
    g["images"][1]["uri"] = "prog.jpg"
    p = str(tmp_path / "prog.gltf")
    json.dump(g, open(p, "w"))
    for kw in ({}, {"textures": "compressed"}):
        with pytest.raises(RuntimeError) as e:
            scene_io.load_gltf_native(p, jpeg=True, **kw)
        assert "prog.jpg" in str(e.value) and "progressive" in str(e.value)
    g["images"][1]["uri"] = "image.webp"
    json.dump(g, open(p, "w"))
    with pytest.raises(RuntimeError) as e:
        scene_io.load_gltf_native(p, jpeg=True)
    assert "image.webp" in str(e.value)


def test_add_texture_blocks_takes_a_record():
    sc = scene_io.Scene()
    data = FILES["17x23_422_q100_noise" if "17x23_422_q100_noise" in FILES else "33x17_420_q90_noise"]
    rgba = zjp.decode(data)
    h, w, _ = rgba.shape
    i = sc.add_texture_blocks(scene_io.pack_jpeg(data, "a.jpg", wire.JPEG_MAP_BG), w, h, zmg.full_mips(w, h), wire.TEX_RG8, wire.TEX_SRC_JPEG_COEF)
    j = sc.add_texture_blocks(scene_io.pack_jpeg(data, "a.jpg"), w, h, 1, wire.TEX_RGBA8, wire.TEX_SRC_JPEG_COEF)
    assert (i, j) == (0, 1)
    sc.decode_textures()
    want = np.concatenate([m.reshape(-1) for m in zmg.np_chain(rgba[..., [2, 1]], wire.TEX_RG8)])
    assert np.array_equal(sc.texels[:len(want)], want)
    o = int(sc.textures["offset"][1])
    assert np.array_equal(sc.texels[o:o + rgba.size], rgba.reshape(-1))
    bad = scene_io.Scene()
    bad.add_texture_blocks(scene_io.pack_jpeg(data, "a.jpg"), w + 1, h, 1, wire.TEX_RGBA8, wire.TEX_SRC_JPEG_COEF)
    with pytest.raises(ValueError):
        bad.decode_textures()
