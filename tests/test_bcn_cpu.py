"""include/zr_bcn.h on the host: the lane form the decode kernel compiles (tests/bcnmath/libzbc.so) and the loader's decoder (zrh_bc7_decode /
zrh_bc5_decode) against the block fixture and Pillow; the compressed mode of the glTF loader and of the host scene."""
import ctypes as C
import gzip
import io
import json
import os
import shutil
import struct

import numpy as np
import pytest

from tests.bcnmath import zbc
from zetaray_amd import scene_io, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_GLTF = os.path.join(ROOT, "tests", "golden", "cornell_gltf")


@pytest.fixture(scope="module")
def fixture_blocks():
    z = np.load(os.path.join(ROOT, "tests", "golden", "bcn_blocks.npz"))
    return {k: np.ascontiguousarray(z[k]) for k in z.files}


def _loader_decode(enc, blocks, w, h):
    L = scene_io._sceneio_lib()
    f = L.zrh_bc7_decode if enc == zbc.BC7 else L.zrh_bc5_decode
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1)
    out = np.zeros((h, w, 4 if enc == zbc.BC7 else 2), np.uint8)
    f(blocks.ctypes.data, w, h, out.ctypes.data)
    return out


def _as_blocks(img, n):
    return img.reshape(4, n, 4, -1).transpose(1, 0, 2, 3).reshape(n, 16, -1)


@pytest.mark.parametrize("name,enc", [("bc7", zbc.BC7), ("bc5", zbc.BC5)])
def test_header_equals_the_fixture(fixture_blocks, name, enc):
    blocks, want = fixture_blocks[name], fixture_blocks[name + "_texels"]
    assert len(blocks) == (2112 if enc == zbc.BC7 else 1040)
    assert np.array_equal(zbc.decode_blocks(enc, blocks), want)                              # the lane form
    assert np.array_equal(_as_blocks(_loader_decode(enc, blocks, 4 * len(blocks), 4), len(blocks)), want)      # the loader's decoder, moved into the header
    if enc == zbc.BC7:
        reserved = blocks[:, 0] == 0
        assert reserved.sum() == 64 and not want[reserved].any()


def _dds(payload, w, h, fmt):
    hdr = bytearray(148)
    hdr[0:4] = b"DDS "
    struct.pack_into("<7I", hdr, 4, 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, h, w, len(payload), 0, 1)
    struct.pack_into("<2I", hdr, 76, 32, 0x4)
    hdr[84:88] = b"DX10"
    struct.pack_into("<I", hdr, 108, 0x1000)
    struct.pack_into("<5I", hdr, 128, fmt, 3, 0, 1, 0)
    return bytes(hdr) + bytes(payload)


def test_header_equals_pillow(fixture_blocks):
    """(the reserved mode is left out: it is this project's to define, (0, 0, 0, 0), and opaque black in Pillow)"""
    Image = pytest.importorskip("PIL.Image")
    b7 = fixture_blocks["bc7"]
    b7 = b7[b7[:, 0] != 0]
    ref = np.array(Image.open(io.BytesIO(_dds(b7.tobytes(), 4 * len(b7), 4, 98))).convert("RGBA"))
    assert np.array_equal(zbc.decode_mip(zbc.BC7, b7, 4 * len(b7), 4), ref)
    b5 = fixture_blocks["bc5"]
    ref5 = np.array(Image.open(io.BytesIO(_dds(b5.tobytes(), 4 * len(b5), 4, 83))))
    assert np.array_equal(zbc.decode_mip(zbc.BC5, b5, 4 * len(b5), 4), ref5[..., :2])


@pytest.mark.parametrize("enc", [zbc.BC7, zbc.BC5])
def test_partial_blocks_lane_form_equals_the_loader(enc):
    """every size from 1 x 1 to 9 x 7: what lies beyond w / h is dropped, rows are w texels apart"""
    rng = np.random.default_rng(11)
    for w in range(1, 10):
        for h in range(1, 8):
            b = rng.integers(0, 256, (zbc.mip_blocks(w, h), 16), dtype=np.uint8)
            assert np.array_equal(zbc.decode_mip(enc, b, w, h), _loader_decode(enc, b, w, h)), (w, h)


def _cornell_gltf(tmp_path, name):
    for f in (name + ".gltf", "cornell.bin"):
        shutil.copy(os.path.join(REF_GLTF, f), tmp_path / f)
    (tmp_path / "compressed").mkdir()
    with gzip.open(os.path.join(REF_GLTF, "compressed", "checkerboard.dds.gz"), "rb") as src:
        (tmp_path / "compressed" / "checkerboard.dds").write_bytes(src.read())
    return str(tmp_path / (name + ".gltf"))


def test_compressed_load_of_the_cornell_gltf(tmp_path):
    path = _cornell_gltf(tmp_path, "cornell")
    dec, offs = scene_io.load_gltf_native(path)
    cmp_, offs2 = scene_io.load_gltf_native(path, textures="compressed")
    assert offs == offs2
    assert len(dec.texture_payload) == 0 and len(dec.texture_sources) == 0
    assert cmp_.textures.tobytes() == dec.textures.tobytes() and len(cmp_.textures) == 1
    assert len(cmp_.texels) == 0 and cmp_.texel_heap_bytes == len(dec.texels)
    assert (cmp_.texture_sources["offset"] % 16 == 0).all() and list(cmp_.texture_sources["encoding"]) == [zbc.BC7]
    # 1024^2 BC7 with 11 mips: 1 byte per texel of mips 0 - 8, one block each for 4^2, 2^2 and 1^2
    assert len(cmp_.texture_payload) == sum(zbc.mip_blocks(max(1, 1024 >> m), max(1, 1024 >> m)) * 16 for m in range(11))
    for f in ("vertices", "indices", "instances", "materials", "instance_to_world"):
        assert getattr(cmp_, f).tobytes() == getattr(dec, f).tobytes(), f
    d = cmp_.desc()
    assert not d.texels and d.texel_bytes == len(dec.texels)
    cmp_.decode_textures()
    assert np.array_equal(cmp_.texels, dec.texels)
    with pytest.raises(ValueError):
        scene_io.load_gltf_native(path, textures="zip")


def test_a_gltf_without_textures_has_no_blocks(tmp_path):
    """zrh_scene_data_texture_blocks is null for it in the compressed mode too, and its desc is the default mode's: zr_scene_create takes it"""
    path = _cornell_gltf(tmp_path, "cornell")
    g = json.load(open(path))
    for k in ("images", "textures", "samplers"):
        g.pop(k, None)
    for m in g.get("materials", []):
        m.get("pbrMetallicRoughness", {}).pop("baseColorTexture", None)
    plain = str(tmp_path / "plain.gltf")
    json.dump(g, open(plain, "w"))
    L = scene_io._sceneio_lib()
    rho, rho_dim = scene_io.load_rho_default()
    rho = np.ascontiguousarray(rho, np.uint16)
    dims = (C.c_uint32 * 3)(*rho_dim)
    for p, want_blocks in ((plain, False), (path, True)):
        h = C.c_void_p()
        assert L.zrh_gltf_load_ex(os.fsencode(p), rho.ctypes.data, dims, scene_io.LOAD_KEEP_COMPRESSED, C.byref(h)) == 0, L.zrh_scene_io_last_error()
        b, d = L.zrh_scene_data_texture_blocks(h), L.zrh_scene_data_desc(h).contents
        assert bool(b) == want_blocks and (d.num_textures > 0) == want_blocks and not d.texels
        if want_blocks:
            assert b.contents.sources and b.contents.payload and b.contents.payload_bytes and d.texel_bytes
        else:
            assert d.texel_bytes == 0 and not d.textures
        L.zrh_scene_data_destroy(h)
    sc, _ = scene_io.load_gltf_native(plain, textures="compressed")
    assert len(sc.texture_payload) == 0 and len(sc.texture_sources) == 0 and sc.texel_heap_bytes == 0 and sc.texture_blocks() is None


def test_add_texture_blocks_round_trips():
    rng = np.random.default_rng(4)
    sc = scene_io.Scene()
    want = []
    for enc, fmt, w, h, mips in ((zbc.BC7, wire.TEX_RGBA8_SRGB, 12, 20, 5), (zbc.BC5, wire.TEX_RG8, 5, 3, 3), (zbc.RAW, wire.TEX_RG8, 3, 3, 2), (zbc.BC7, wire.TEX_RGBA8, 4, 4, 1)):
        chain, texels = [], []
        for m in range(mips):
            mw, mh = max(1, w >> m), max(1, h >> m)
            if enc == zbc.RAW:
                t = rng.integers(0, 256, mw * mh * 2, dtype=np.uint8)
                chain.append(t)
            else:
                b = rng.integers(0, 256, (zbc.mip_blocks(mw, mh), 16), dtype=np.uint8)
                chain.append(b.reshape(-1))
                t = zbc.decode_mip(enc, b, mw, mh).reshape(-1)
            texels.append(t)
        idx = sc.add_texture_blocks(np.concatenate(chain), w, h, mips, fmt, enc)
        assert idx == len(want)
        want.append(np.concatenate(texels))
    assert (sc.textures["offset"] % 4 == 0).all() and (sc.texture_sources["offset"] % 16 == 0).all()
    assert len(sc.texels) == 0
    sc.decode_textures()
    assert len(sc.texels) == sc.texel_heap_bytes
    covered = np.zeros(len(sc.texels), bool)
    for i, t in enumerate(want):
        off = int(sc.textures["offset"][i])
        assert np.array_equal(sc.texels[off:off + len(t)], t), i
        covered[off:off + len(t)] = True
    assert not sc.texels[~covered].any()
    with pytest.raises(ValueError):
        sc.add_texture_blocks(np.zeros(16, np.uint8), 4, 4, 1, wire.TEX_RG8, zbc.BC7)      # BC7 decodes to RGBA8
    with pytest.raises(ValueError):
        sc.add_texture_blocks(np.zeros(15, np.uint8), 4, 4, 1, wire.TEX_RGBA8, zbc.BC7)    # a short chain
    # a heap is all sources or all texels, in either order; a fixture holds texels
    with pytest.raises(ValueError):
        sc.add_texture(np.zeros((4, 4, 4), np.uint8))
    n = len(sc.textures)
    plain = scene_io.Scene()
    plain.add_texture(np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(ValueError):
        plain.add_texture_blocks(np.zeros(16, np.uint8), 4, 4, 1, wire.TEX_RGBA8, zbc.BC7)
    assert len(sc.textures) == n == len(sc.texture_sources) and len(plain.textures) == 1


def test_save_npz_refuses_undecoded_sources(tmp_path):
    base = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))
    base.add_texture_blocks(np.arange(16, dtype=np.uint8) + 64, 4, 4, 1, wire.TEX_RGBA8, zbc.BC7)
    with pytest.raises(ValueError, match="decode_textures"):
        scene_io.save_npz(base, str(tmp_path / "a.npz"))
    base.decode_textures()
    scene_io.save_npz(base, str(tmp_path / "a.npz"))
    back = scene_io.load_npz(str(tmp_path / "a.npz"))
    assert np.array_equal(back.texels, base.texels) and back.textures.tobytes() == base.textures.tobytes()
