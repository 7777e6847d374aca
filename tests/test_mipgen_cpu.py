"""Mip generation and PNG loading on the host: include/zr_mipgen.h (through zrh_mip_generate) against a numpy restatement of its contract and against
float64, zrh_png_decode against arrays, and load_gltf_native on a glTF with PNG images in both texture modes.  No GPU."""
import gzip
import os
import re
import shutil
import zlib

import numpy as np
import pytest

from tests.mipmath import zmg
from zetaray_amd import scene_io, wire

ROOT = zmg.ROOT
SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (5, 3), (1, 7), (7, 1), (4, 6), (9, 7), (16, 16), (17, 5)]      # (w, h)


def _inputs(rng, w, h, C):
    return {"random": rng.integers(0, 256, (h, w, C), dtype=np.uint8), "dark": rng.integers(0, 24, (h, w, C), dtype=np.uint8),
            "constant": np.broadcast_to(rng.integers(0, 256, C, dtype=np.uint8), (h, w, C)).copy()}


# ---- 1. the header against the contract restated in numpy
def test_the_table_is_the_formula():
    txt = open(os.path.join(ROOT, "include", "zr_srgb16_table.h")).read()
    vals = [int(v) for v in re.findall(r"\d+", txt[txt.index("{") + 1:txt.index("}")])]
    assert vals == [int(v) for v in zmg.L16]
    assert vals[:4] == [0, 20, 40, 60] and vals[255] == 65535 and all(b > a for a, b in zip(vals, vals[1:]))
    assert wire.TEX_SRC_RAW_MIP0 == 8


@pytest.mark.parametrize("fmt", list(zmg.FORMATS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_header_equals_the_numpy_contract(fmt, size):
    w, h = size
    f = zmg.FORMATS[fmt]
    rng = np.random.default_rng(1000 * w + h)
    for kind, img in _inputs(rng, w, h, zmg.channels(f)).items():
        got, want = zmg.header_chain(img, f), zmg.np_chain(img, f)
        assert len(got) == len(want) == zmg.full_mips(w, h)
        assert np.array_equal(got[0], img)
        for m, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and np.array_equal(a, b), (kind, "level", m, a.reshape(-1)[:8], b.reshape(-1)[:8])
        if kind == "constant":
            for m, a in enumerate(got):
                assert (a == img[0, 0]).all(), ("a constant image must stay constant", m)


def test_one_level_chains_generate_nothing():
    img = np.random.default_rng(4).integers(0, 256, (5, 9, 4), dtype=np.uint8)
    heap = np.full(img.size + 16, 0xA5, np.uint8)
    heap[:img.size] = img.reshape(-1)
    before = heap.copy()
    scene_io.mip_generate(zmg.descs([(0, 9, 5, 1, wire.TEX_RGBA8_SRGB)]), heap)
    assert np.array_equal(heap, before)


# ---- 2. against float64
def _footprints(rng, n, hi, taps):
    """n footprints of `taps` values below `hi`, half of them near-equal neighbours (+-3 around the first)"""
    v = rng.integers(0, hi, (n, taps))
    v[:n // 2] = np.clip(v[:n // 2, :1] + rng.integers(-3, 4, (n // 2, taps)), 0, 255)
    return v.astype(np.uint8)


def _reduce_footprints(v, side, fmt):
    """one generated texel per footprint (n, side * side, C): every footprint is a side x side texture of its own with a 2-level chain"""
    n, _, C = v.shape
    per = side * side * C + C
    per_pad = (per + 3) // 4 * 4
    heap = np.zeros(n * per_pad, np.uint8)
    view = heap.reshape(n, per_pad)
    view[:, :side * side * C] = v.reshape(n, -1)
    d = np.zeros(n, wire.TEXTURE_DESC)
    d["offset"], d["width"], d["height"], d["num_mips"], d["format"] = np.arange(n) * per_pad, side, side, 2, fmt
    scene_io.mip_generate(d, heap)
    return view[:, side * side * C:per].copy()


@pytest.mark.parametrize("kind", ["full 2x2", "dark 2x2", "uniform 3x3"])
def test_against_float64(kind):
    rng = np.random.default_rng(2)
    n = 400_000 // 4 + 1      # x 4 channels: 400 000 footprints per format
    side, hi = (3, 256) if kind == "uniform 3x3" else (2, 32 if kind.startswith("dark") else 256)
    v = np.stack([_footprints(rng, n, hi, side * side) for _ in range(4)], axis=2)      # (n, taps, 4)
    # UNORM channels: floor(mean + 0.5); a 3 x 3 texture's one texel weighs its nine texels equally (weights {1, 1, 1} on both axes)
    for fmt, C in ((wire.TEX_RGBA8, 4), (wire.TEX_RG8, 2)):
        got = _reduce_footprints(np.ascontiguousarray(v[:, :, :C]), side, fmt)
        want = np.floor(v[:, :, :C].astype(np.float64).sum(axis=1) / (side * side) + 0.5)
        assert np.array_equal(got, want.astype(np.uint8)), fmt
    got = _reduce_footprints(v, side, wire.TEX_RGBA8_SRGB)
    assert np.array_equal(got[:, 3], np.floor(v[:, :, 3].astype(np.float64).sum(axis=1) / (side * side) + 0.5).astype(np.uint8)), "alpha is UNORM"
    ref = 255.0 * zmg.linear_to_srgb(zmg.srgb_to_linear(v[:, :, :3]).mean(axis=1))
    err = np.abs(got[:, :3].astype(np.float64) - ref)
    differs = (got[:, :3] != np.round(ref)).mean()
    print("%s: worst |code - 255 encode(mean)| = %.4f, differs from round() in %.3f %% of %d channels" % (kind, err.max(), 100 * differs, ref.size))
    assert err.max() <= 0.6, err.max()      # (a)
    # (b) on the uniform-random half of the input (the other half are near-equal neighbours)
    half = n // 2
    differs_uniform = (got[half:, :3] != np.round(ref[half:])).mean()
    assert differs_uniform <= 0.05, differs_uniform


# ---- 3. the PNG decoder
PNG_SIZES = [(1, 1), (3, 5), (64, 64), (257, 3)]      # (w, h)
COMPRESSION = {"stored": (0, zlib.Z_DEFAULT_STRATEGY), "dynamic": (9, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED)}
# (name, colour type, depth, channels, tRNS?)
KINDS = [("grey8", 0, 8, 1, False), ("grey16", 0, 16, 1, False), ("grey8+tRNS", 0, 8, 1, True), ("grey16+tRNS", 0, 16, 1, True),
         ("rgb8", 2, 8, 3, False), ("rgb16", 2, 16, 3, False), ("rgb8+tRNS", 2, 8, 3, True), ("rgb16+tRNS", 2, 16, 3, True),
         ("palette", 3, 8, 1, False), ("palette+tRNS", 3, 8, 1, True), ("grey-alpha8", 4, 8, 2, False), ("grey-alpha16", 4, 16, 2, False),
         ("rgba8", 6, 8, 4, False), ("rgba16", 6, 16, 4, False)]


def _png_case(rng, w, h, ctype, depth, ch, with_trns):
    """(samples, expected RGBA, palette, tRNS body)"""
    palette = trns = None
    if ctype == 3:
        npal = 37
        palette = rng.integers(0, 256, (npal, 3), dtype=np.uint8)
        samples = rng.integers(0, npal, (h, w, 1), dtype=np.uint8)
        alpha = np.full(npal, 255, np.uint8)
        if with_trns:
            trns = rng.integers(0, 256, 20, dtype=np.uint8)      # (fewer entries than the palette: the rest are opaque)
            alpha[:20] = trns
            trns = trns.tobytes()
        want = np.concatenate([palette[samples[..., 0]], alpha[samples[..., 0]][..., None]], axis=2)
        return samples, want, palette, trns
    # few distinct values, so that the key colour occurs and rows repeat (which the filters and the match finder see)
    samples = rng.integers(0, 4, (h, w, ch)).astype(np.uint16 if depth == 16 else np.uint8)
    if depth == 16:
        samples = (samples * 0x3A17 + rng.integers(0, 2, (h, w, ch)) * 0x0101).astype(np.uint16)
    else:
        samples = (samples * 61).astype(np.uint8)
    hi = (samples >> 8).astype(np.uint8) if depth == 16 else samples
    if ctype in (0, 4):
        rgb = np.repeat(hi[..., :1], 3, axis=2)
    else:
        rgb = hi[..., :3]
    if ctype in (4, 6):
        a = hi[..., -1:]
    else:
        a = np.full((h, w, 1), 255, np.uint8)
        if with_trns:
            key = samples[h // 2, w // 2, :].astype(np.uint16)      # the full sample is compared, both bytes of a 16-bit one
            trns = key.astype(">u2").tobytes()
            a[(samples == key).all(axis=2)] = 0
    return samples, np.concatenate([rgb, a], axis=2), palette, trns


@pytest.mark.parametrize("comp", list(COMPRESSION))
@pytest.mark.parametrize("flt", range(5))
def test_png_decode(flt, comp):
    level, strategy = COMPRESSION[comp]
    rng = np.random.default_rng(10 * flt + len(comp))
    for w, h in PNG_SIZES:
        for name, ctype, depth, ch, with_trns in KINDS:
            samples, want, palette, trns = _png_case(rng, w, h, ctype, depth, ch, with_trns)
            data = zmg.png_bytes(samples, ctype, depth, flt, level, strategy, palette, trns, idat_split=97 if (w, h) == (64, 64) else None)
            got = scene_io.png_decode(data, name)
            assert got.shape == want.shape and np.array_equal(got, want), (name, w, h, int((got != want).sum()))
            if with_trns and ctype != 3:
                assert (want[..., 3] == 0).any() and ((want[..., 3] == 255).any() or w * h == 1)


def test_png_decode_of_incompressible_data():
    """random samples: long literal runs, and at level 0 a stored block of more than 65535 bytes split in two"""
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (150, 150, 4), dtype=np.uint8)
    for level in (0, 1, 9):
        for flt in (0, 4):
            assert np.array_equal(scene_io.png_decode(zmg.png_bytes(img, 6, flt=flt, level=level)), img), (level, flt)


def test_png_decode_of_pillow_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(8)
    for mode, shape in (("RGBA", (21, 37, 4)), ("RGB", (64, 64, 3)), ("L", (3, 257)), ("LA", (5, 3, 2)), ("P", (16, 16))):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        im = Image.fromarray(a, mode) if mode != "P" else Image.fromarray(a, "P")
        if mode == "P":
            im.putpalette(list(rng.integers(0, 256, 768, dtype=np.uint8)))
        for kw in ({}, {"optimize": True}, {"compress_level": 0}):
            p = tmp_path / ("%s.png" % mode)
            im.save(p, **kw)
            want = np.asarray(Image.open(p).convert("RGBA"))
            assert np.array_equal(scene_io.png_decode(p.read_bytes(), str(p)), want), (mode, kw)
    a16 = rng.integers(0, 65536, (9, 7), dtype=np.uint16)
    p = tmp_path / "grey16.png"
    Image.fromarray(a16).save(p)
    got = scene_io.png_decode(p.read_bytes())
    assert np.array_equal(got[..., 0], (a16 >> 8).astype(np.uint8)) and (got[..., 3] == 255).all()


def _refused(data, *words, name="some/file.png"):
    with pytest.raises(RuntimeError) as e:
        scene_io.png_decode(data, name)
    msg = str(e.value)
    assert name in msg and all(w in msg for w in words), msg


def test_png_refusals():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)
    good = zmg.png_bytes(img, 6, flt=1, level=6)
    assert np.array_equal(scene_io.png_decode(good), img)
    _refused(zmg.png_bytes(img, 6, interlace=1), "interlaced")
    for depth in (1, 2, 4):
        _refused(zmg.png_bytes(img[..., :1] & 1, 0, depth=depth), "bit depths below 8")
    # a flipped byte inside the IDAT body: the chunk CRC; with the CRC mended, the Adler-32 (or the deflate stream itself)
    at = good.index(b"IDAT") + 4
    n = int.from_bytes(good[at - 8:at - 4], "big")
    bad = bytearray(good)
    bad[at + n - 6] ^= 0x40
    _refused(bytes(bad), "CRC")
    mended = bytes(bad[:at + n]) + (zlib.crc32(bytes(bad[at - 4:at + n])) & 0xFFFFFFFF).to_bytes(4, "big") + bytes(bad[at + n + 4:])
    with pytest.raises(RuntimeError):
        scene_io.png_decode(mended)
    # the Adler-32 alone: the last four bytes of the zlib stream
    bad = bytearray(good)
    bad[at + n - 1] ^= 0x01
    mended = bytes(bad[:at + n]) + (zlib.crc32(bytes(bad[at - 4:at + n])) & 0xFFFFFFFF).to_bytes(4, "big") + bytes(bad[at + n + 4:])
    _refused(mended, "Adler-32")
    bad = bytearray(good)
    bad[20] ^= 0xFF      # IHDR: its CRC
    _refused(bytes(bad), "CRC")
    for cut in (len(good) - 1, len(good) - 12, at + n // 2, at, 40, 20, 8, 3):
        _refused(good[:cut], "truncated" if cut >= 8 else "PNG")
    # image data that ends early inside a well-formed file: rows missing
    short = zmg.png_bytes(img[:5], 6)
    z = short[short.index(b"IDAT") + 4:][:int.from_bytes(short[short.index(b"IDAT") - 4:short.index(b"IDAT")], "big")]
    _refused(good[:at - 8] + zmg._chunk(b"IDAT", z) + zmg._chunk(b"IEND", b""), "truncated")
    import struct
    for w, h in ((0, 8), (8, 0), (65536, 1), (1, 65536), (1 << 31, 1 << 31)):
        hdr = zmg._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
        _refused(good[:8] + hdr + good[8 + 25:], "dimensions", "[1, 65535]")
    # 65535 x 65535 promised by a tiny file: refused before anything of that size is allocated
    hdr = zmg._chunk(b"IHDR", struct.pack(">IIBBBBB", 65535, 65535, 16, 6, 0, 0, 0))
    _refused(good[:8] + hdr + good[8 + 25:], "truncated")


# ---- 4. the loader
def _plain_dds_gltf(tmp_path):
    d = tmp_path / "dds"
    d.mkdir()
    for f in ("cornell_emissive.gltf", "cornell.bin"):
        shutil.copy(os.path.join(zmg.REF_GLTF, f), d / f)
    (d / "compressed").mkdir()
    with gzip.open(os.path.join(zmg.REF_GLTF, "compressed", "checkerboard.dds.gz"), "rb") as src:
        (d / "compressed" / "checkerboard.dds").write_bytes(src.read())
    return str(d / "cornell_emissive.gltf")


def _level0(sc, i):
    t = sc.textures[i]
    n = int(t["width"]) * int(t["height"]) * zmg.channels(int(t["format"]))
    return sc.texels[int(t["offset"]):int(t["offset"]) + n].reshape(int(t["height"]), int(t["width"]), -1)


def test_loader_both_modes(tmp_path):
    rng = np.random.default_rng(11)
    path, files = zmg.cornell_png_gltf(tmp_path, rng)
    dec, offs = scene_io.load_gltf_native(path)
    cmp_, offs2 = scene_io.load_gltf_native(path, textures="compressed")
    assert offs == offs2 and len(dec.textures) == 4 and np.array_equal(dec.textures, cmp_.textures)
    assert len(cmp_.texels) == 0 and cmp_.texel_heap_bytes == len(dec.texels)
    # heap order: base colour maps (the .png of the textured material, then the .dds), the normal map, the metallic-roughness map
    kinds = [int(offs["base_color"]), int(offs["normal"]), int(offs["metallic_roughness"]), int(offs["emissive"])]
    assert kinds == [0, 2, 3, 4]
    enc = [int(e) for e in cmp_.texture_sources["encoding"]]
    assert sorted(enc[:2]) == [wire.TEX_SRC_BC7, wire.TEX_SRC_RAW_MIP0] and enc[2:] == [wire.TEX_SRC_RAW_MIP0] * 2
    png_base = enc.index(wire.TEX_SRC_RAW_MIP0)
    for i, name, fmt in ((png_base, "base", wire.TEX_RGBA8_SRGB), (2, "normal", wire.TEX_RG8), (3, "mr", wire.TEX_RG8)):
        t = dec.textures[i]
        h, w, _ = files[name].shape
        assert (int(t["width"]), int(t["height"]), int(t["format"])) == (w, h, fmt)
        assert int(t["num_mips"]) == 1 + int(np.floor(np.log2(max(w, h)))), name
    assert np.array_equal(_level0(dec, png_base), files["base"])
    assert np.array_equal(_level0(dec, 2), files["normal"][..., [0, 1]]), "a normal map keeps the file's (R, G)"
    assert np.array_equal(_level0(dec, 3), files["mr"][..., [2, 1]]), "a metallic-roughness map keeps the file's (B, G)"
    # the chains are the contract's, and the compressed-mode payload rebuilds the same heap
    for i, fmt in ((png_base, wire.TEX_RGBA8_SRGB), (2, wire.TEX_RG8), (3, wire.TEX_RG8)):
        t = dec.textures[i]
        want = np.concatenate([m.reshape(-1) for m in zmg.np_chain(_level0(dec, i), fmt)])
        assert np.array_equal(dec.texels[int(t["offset"]):int(t["offset"]) + len(want)], want), i
    cmp_.decode_textures()
    assert np.array_equal(cmp_.texels, dec.texels)
    # level 0 alone travels: the payload is smaller than the heap
    assert len(cmp_.texture_payload) < len(dec.texels)


def test_dds_fixture_loads_to_the_same_bytes(tmp_path):
    """the untouched .dds glTF: the .dds texture of the mixed file above decodes to the bytes it has here, in both modes"""
    plain = _plain_dds_gltf(tmp_path)
    a, offs = scene_io.load_gltf_native(plain)
    b, _ = scene_io.load_gltf_native(plain, textures="compressed")
    b.decode_textures()
    assert len(a.textures) == 1 and np.array_equal(a.texels, b.texels) and int(b.texture_sources["encoding"][0]) == wire.TEX_SRC_BC7
    path, _ = zmg.cornell_png_gltf(tmp_path, np.random.default_rng(11))
    mixed, _ = scene_io.load_gltf_native(path)
    i = [k for k in range(2) if int(mixed.textures["width"][k]) == int(a.textures["width"][0])][0]
    o = int(mixed.textures["offset"][i])
    assert np.array_equal(mixed.texels[o:o + len(a.texels)], a.texels)
    z = np.load(os.path.join(ROOT, "tests", "golden", "cornell_emissive.npz"))
    if "texels" in z.files:
        assert np.array_equal(z["texels"], a.texels)


def test_jpeg_and_unknown_images_are_refused_by_name(tmp_path):
    import json
    path, _ = zmg.cornell_png_gltf(tmp_path, np.random.default_rng(12))
    g = json.load(open(path))
    for uri, words in (("photo.jpg", ("JPEG", "not supported")), ("photo.JPEG", ("JPEG", "not supported")), ("image.webp", ("image.webp",))):
        g["images"][1]["uri"] = uri
        p = str(tmp_path / "refused.gltf")
        json.dump(g, open(p, "w"))
        with pytest.raises(RuntimeError) as e:
            scene_io.load_gltf_native(p)
        assert uri in str(e.value) and all(w in str(e.value) for w in words) and "only .dds images" not in str(e.value), str(e.value)
    # a corrupted .png names its file
    g["images"][1]["uri"] = "base.png"
    data = bytearray((tmp_path / "base.png").read_bytes())
    data[40] ^= 0x10
    (tmp_path / "base.png").write_bytes(bytes(data))
    p = str(tmp_path / "corrupt.gltf")
    json.dump(g, open(p, "w"))
    with pytest.raises(RuntimeError) as e:
        scene_io.load_gltf_native(p)
    assert "base.png" in str(e.value)


def test_add_texture_blocks_takes_level_0(tmp_path):
    rng = np.random.default_rng(13)
    sc = scene_io.Scene()
    img = rng.integers(0, 256, (7, 9, 2), dtype=np.uint8)
    i = sc.add_texture_blocks(img, 9, 7, zmg.full_mips(9, 7), wire.TEX_RG8, wire.TEX_SRC_RAW_MIP0)
    j = sc.add_texture_blocks(rng.integers(0, 256, (4, 4, 4), dtype=np.uint8), 4, 4, 1, wire.TEX_RGBA8, wire.TEX_SRC_RAW_MIP0)
    assert (i, j) == (0, 1) and sc.texel_heap_bytes == int(sc.textures["offset"][1]) + 64
    with pytest.raises(ValueError):
        sc.add_texture_blocks(np.zeros(10, np.uint8), 9, 7, 4, wire.TEX_RG8, wire.TEX_SRC_RAW_MIP0)
    sc.decode_textures()
    want = np.concatenate([m.reshape(-1) for m in zmg.np_chain(img, wire.TEX_RG8)])
    assert np.array_equal(sc.texels[:len(want)], want)
