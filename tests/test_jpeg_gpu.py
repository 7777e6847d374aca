"""The JPEG decode on the GPU (zr_tu_jpeg.hip) against include/zr_jpeg.h on the host (zrh_jpeg_expand / zrh_jpeg_decode), byte for byte: on caller
buffers (zr_jpeg_decode_device) and through the scene path (zr_scene_create_compressed with ZR_TEX_SRC_JPEG_COEF sources).  Expected bytes never come
from the kernel."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.bcnmath import zbc
from tests.jpegmath import zjp
from tests.mipmath import zmg
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
ROOT = zjp.ROOT
FAST_LIB = os.path.join(ROOT, "zetaray_amd", "libzetaray_amd_fast.so")
FILL = 0xA5
FIXTURE = zjp.load_fixture()
GOOD = [(n, d) for n, d, w in FIXTURE if w is not None]
FILES = {n: d for n, d, _ in FIXTURE}
MAPS = ((wire.JPEG_MAP_RGBA, wire.TEX_RGBA8_SRGB), (wire.JPEG_MAP_RG, wire.TEX_RG8), (wire.JPEG_MAP_BG, wire.TEX_RG8))
INVALID = 1      # ZR_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


@pytest.fixture(scope="module")
def stream(api):
    import torch
    return torch.cuda.Stream()


def _call(items, first=12):
    """items: [(file bytes, channel map, format)] -> (descs, sources, payload, heap bytes, [(offset, expected level 0 from the header on the host)]);
    one-level chains with a few bytes of padding between them"""
    descs, sources = np.zeros(len(items), wire.TEXTURE_DESC), np.zeros(len(items), wire.TEXTURE_SOURCE)
    payload, want, at = np.zeros(0, np.uint8), [], first
    for i, (data, cmap, fmt) in enumerate(items):
        rec = scene_io.pack_jpeg(data, "file%d.jpg" % i, cmap)
        px = scene_io.jpeg_expand(rec)
        payload = np.concatenate([payload, np.zeros(-len(payload) % 16, np.uint8)])
        sources["offset"][i], sources["encoding"][i] = len(payload), wire.TEX_SRC_JPEG_COEF
        payload = np.concatenate([payload, rec])
        at = (at + 3) // 4 * 4
        descs["offset"][i], descs["width"][i], descs["height"][i], descs["num_mips"][i], descs["format"][i] = at, px.shape[1], px.shape[0], 1, fmt
        want.append((at, px.reshape(-1)))
        at += px.size + 5
    return descs, sources, payload, at + 59, want


# ---- 1. every fixture file through the kernels, in the three channel maps, on a non-null stream
@pytest.mark.parametrize("case", GOOD, ids=[c[0] for c in GOOD])
def test_kernel_equals_the_header(api, stream, case):
    name, data = case
    descs, sources, payload, nbytes, want = _call([(data, cmap, fmt) for cmap, fmt in MAPS])
    got = api.jpeg_decode_device(descs, sources, payload, nbytes, fill=FILL, stream=stream)
    expect = np.full(nbytes, FILL, np.uint8)
    for off, px in want:
        expect[off:off + len(px)] = px
    bad = np.nonzero(got != expect)[0]
    assert len(bad) == 0, (name, len(bad), bad[:8], got[bad[:8]], expect[bad[:8]])
    rgba = scene_io.decode_jpeg(data, name)
    assert np.array_equal(want[0][1], rgba.reshape(-1)) and np.array_equal(want[2][1], rgba[..., [2, 1]].reshape(-1))


def test_rg8_rows_on_two_byte_boundaries(api, stream):
    """A chain starts on a multiple of 4 (zr_scene_create refuses any other desc), so level 0 itself cannot start at 2 mod 4; its rows and texels can:
    a 7 x 5 RG8 level 0 has rows of 14 bytes, every second one at 2 mod 4, and here the level sits at 4 mod 8 behind a 33 x 17 one of 1122 bytes."""
    items = [(FILES["33x17_420_q90_noise"], wire.JPEG_MAP_BG, wire.TEX_RG8), (FILES["7x5_422_q90_noise"], wire.JPEG_MAP_RG, wire.TEX_RG8)]
    descs, sources, payload, nbytes, want = _call(items, first=4)
    assert (33 * 17 * 2) % 4 == 2 and int(descs["offset"][1]) % 8 == 4
    got = api.jpeg_decode_device(descs, sources, payload, nbytes, fill=FILL, stream=stream)
    expect = np.full(nbytes, FILL, np.uint8)
    for off, px in want:
        expect[off:off + len(px)] = px
    assert np.array_equal(got, expect)


# ---- 2. the scene path
def _mixed_box(rng):
    """the untextured Cornell box with five maps in its heap: a 4:2:0 JPEG as an sRGB map and a grey JPEG as an RG8 map (level 0 from the record, the rest
    generated), a BC7 map and a RAW map with their stored chains, and a RAW_MIP0 RG8 map"""
    sc = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))
    sc.add_texture_blocks(scene_io.pack_jpeg(FILES["33x17_420_q90_noise"], "a.jpg"), 33, 17, zmg.full_mips(33, 17), wire.TEX_RGBA8_SRGB, wire.TEX_SRC_JPEG_COEF)
    mips = zmg.full_mips(8, 8)
    blocks = np.concatenate([rng.integers(0, 256, zbc.mip_blocks(max(1, 8 >> m), max(1, 8 >> m)) * 16, dtype=np.uint8) for m in range(mips)])
    sc.add_texture_blocks(blocks, 8, 8, mips, wire.TEX_RGBA8_SRGB, wire.TEX_SRC_BC7)
    sc.add_texture_blocks(scene_io.pack_jpeg(FILES["17x23_gray_restart_rows"], "b.jpg", wire.JPEG_MAP_RG), 17, 23, 2, wire.TEX_RG8, wire.TEX_SRC_JPEG_COEF)      # (782 + 176 bytes: the next chain starts 2 bytes further)
    sc.add_texture_blocks(rng.integers(0, 256, 2 * 2 * 4 + 4, dtype=np.uint8), 2, 2, 2, wire.TEX_RGBA8, wire.TEX_SRC_RAW)
    sc.add_texture_blocks(rng.integers(0, 256, 9 * 7 * 2, dtype=np.uint8), 9, 7, zmg.full_mips(9, 7), wire.TEX_RG8, wire.TEX_SRC_RAW_MIP0)
    sc.texel_heap_bytes += 24      # (and padding behind the last chain)
    return sc


def test_scene_with_mixed_sources(api):
    sc = _mixed_box(np.random.default_rng(5))
    host = _mixed_box(np.random.default_rng(5))
    host.decode_textures()
    got = api.Scene(sc).get_texels()
    assert len(got) == sc.texel_heap_bytes == len(host.texels)
    assert np.array_equal(got, host.texels), np.nonzero(got != host.texels)[0][:8]
    inside = np.zeros(len(got), bool)
    for t in sc.textures:
        inside[int(t["offset"]):int(t["offset"]) + zmg.chain_bytes(int(t["width"]), int(t["height"]), int(t["num_mips"]), int(t["format"]))] = True
    assert (~inside).sum() == 2 + 24 and (got[~inside] == 0).all(), "every byte outside the chains is zero"
    # level 0 of the JPEG maps is the decoder's, their chains the mipgen contract's
    rgba = scene_io.decode_jpeg(FILES["33x17_420_q90_noise"])
    want = np.concatenate([m.reshape(-1) for m in zmg.np_chain(rgba, wire.TEX_RGBA8_SRGB)])
    o = int(sc.textures["offset"][0])
    assert np.array_equal(got[o:o + len(want)], want)


def test_scene_path_on_the_jpeg_cornell(api, tmp_path):
    path, _ = zjp.cornell_jpeg_gltf(tmp_path)
    dec, offs = scene_io.load_gltf_native(path, jpeg=True)
    cmp_, offs2 = scene_io.load_gltf_native(path, textures="compressed", jpeg=True)
    assert offs == offs2 and len(cmp_.texture_payload) and len(cmp_.texels) == 0 and len(dec.texels)
    assert (cmp_.texture_sources["encoding"] == wire.TEX_SRC_JPEG_COEF).sum() == 3
    w, h = 96, 54
    prm = wire.default_params()
    ra = api.Renderer(dec, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    rb = api.Renderer(cmp_, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    heap = rb.scene.get_texels()
    assert len(heap) == len(dec.texels) and np.array_equal(heap, dec.texels)
    assert np.array_equal(ra.scene.get_texels(), dec.texels)
    for f in (1, 2):
        cb = scene_io.make_frame_constants(w, h, frame_num=f, num_emissives=len(dec.emissives))
        scene_io.set_texture_heap_offsets(cb, offs)
        for r in (ra, rb):
            r.render_frame(cb)
        ga, gb = ra.gbuffer.download()[0], rb.gbuffer.download()[0]
        for k, (pa, pb) in enumerate(zip(ga, gb)):
            assert np.array_equal(np.asarray(pa).view(np.uint8), np.asarray(pb).view(np.uint8)), ("G-buffer plane", k, "frame", f)
        assert np.array_equal(ra.final().view(np.uint32), rb.final().view(np.uint32)), ("FINAL", f)
        ca, cb_ = ra.p_indirect.read_counters(), rb.p_indirect.read_counters()
        assert ca == cb_ and ca[0] > 0, (ca, cb_)


# ---- 3. refusals: zr::BuildTexturePlan (zr_tex_plan.h) validates the whole record before anything is enqueued
def _u32(payload, at, value):
    payload[at:at + 4] = np.frombuffer(np.uint32(value).tobytes(), np.uint8)


def test_refusals_leave_nothing_behind(api):
    import torch
    L = api.lib()
    sc = _mixed_box(np.random.default_rng(5))
    SENTINEL = 0x5A5A5A5A
    r0, r2 = int(sc.texture_sources["offset"][0]), int(sc.texture_sources["offset"][2])
    h0 = zjp.record_header(sc.texture_payload[r0:])
    B0 = int(h0["num_blocks"])
    assert int(h0["ncomp"]) == 3 and B0 == 36

    def variant(edit):
        descs, sources, payload = sc.textures.copy(), sc.texture_sources.copy(), sc.texture_payload.copy()
        desc, blocks = sc.desc(), sc.texture_blocks()
        desc.texels, desc.texel_bytes = None, sc.texel_heap_bytes
        desc.textures, blocks.sources, blocks.payload = descs.ctypes.data, sources.ctypes.data, payload.ctypes.data
        edit(descs, sources, desc, blocks, payload)
        h = C.c_void_p(SENTINEL)
        code = L.zr_scene_create_compressed(0, C.addressof(desc), C.addressof(blocks), C.byref(h))
        if code == 0:
            L.zr_scene_destroy(h)
        else:
            assert h.value == SENTINEL, "*out was written"
        return code

    assert variant(lambda d, s, desc, b, p: None) == 0, L.zr_last_error()
    comp0 = r0 + 40      # the first component's entry of the record's header: hs, vs, bw, bh, first_block
    begin = r0 + 496
    last_source = int(np.argmax(sc.texture_sources["offset"]))
    assert int(sc.texture_sources["encoding"][last_source]) == wire.TEX_SRC_RAW_MIP0
    edits = {
        "wrong magic": lambda d, s, desc, b, p: _u32(p, r0, 0x12345678),
        "the record ends beyond the payload": lambda d, s, desc, b, p: (p.__setitem__(slice(r0 + 8, r0 + 16), np.frombuffer(np.uint64(len(p) - r0 + 1).tobytes(), np.uint8))),
        "a header cut by the payload's end": lambda d, s, desc, b, p: (s["offset"].__setitem__(2, (len(p) - 100) // 16 * 16)),
        "the record starts beyond the payload": lambda d, s, desc, b, p: s["offset"].__setitem__(0, 1 << 40),
        "offset not a multiple of 16": lambda d, s, desc, b, p: s["offset"].__setitem__(0, r0 + 8),
        "w differs from the desc": lambda d, s, desc, b, p: d["width"].__setitem__(0, 34),
        "h differs from the desc": lambda d, s, desc, b, p: d["height"].__setitem__(2, 24),
        "an RGBA map on RG8": lambda d, s, desc, b, p: _u32(p, r2 + 28, wire.JPEG_MAP_RGBA),
        "an RG map on RGBA8": lambda d, s, desc, b, p: _u32(p, r0 + 28, wire.JPEG_MAP_BG),
        "unknown map": lambda d, s, desc, b, p: _u32(p, r0 + 28, 3),
        "4:1:1 sampling": lambda d, s, desc, b, p: _u32(p, comp0, 4),
        "4:4:0 sampling": lambda d, s, desc, b, p: (_u32(p, comp0, 1), _u32(p, comp0 + 4, 2)),
        "two components": lambda d, s, desc, b, p: _u32(p, r0 + 24, 2),
        "a block row more than the size gives": lambda d, s, desc, b, p: _u32(p, comp0 + 12, 5),
        "a block count that does not follow": lambda d, s, desc, b, p: _u32(p, r0 + 32, B0 + 1),
        "coef_begin does not start at 0": lambda d, s, desc, b, p: _u32(p, begin, 1),
        "coef_begin stands still": lambda d, s, desc, b, p: _u32(p, begin + 4 * 5, int(np.frombuffer(p[begin + 16:begin + 20].tobytes(), "<u4")[0])),
        "coef_begin steps by more than 64": lambda d, s, desc, b, p: [_u32(p, begin + 4 * k, int(np.frombuffer(p[begin + 4 * k:begin + 4 * k + 4].tobytes(), "<u4")[0]) + 64) for k in range(3, B0 + 1)],
        "coef_begin decreases": lambda d, s, desc, b, p: _u32(p, begin + 4 * 7, 2),
        "the coefficients end beyond the record": lambda d, s, desc, b, p: (p.__setitem__(slice(r0 + 8, r0 + 16), np.frombuffer(np.uint64(int(h0["bytes"]) - 2).tobytes(), np.uint8))),
        "encoding 3 is still unknown": lambda d, s, desc, b, p: s["encoding"].__setitem__(0, 3),
        "encoding 9 is still unknown": lambda d, s, desc, b, p: s["encoding"].__setitem__(0, 9),
        "encoding 17": lambda d, s, desc, b, p: s["encoding"].__setitem__(0, 17),
    }
    for name, edit in edits.items():
        assert variant(edit) == INVALID, name

    # zr_jpeg_decode_device refuses the same, and a refused call writes nothing
    descs, sources, payload, nbytes, want = _call([(FILES["33x17_420_q90_noise"], wire.JPEG_MAP_RGBA, wire.TEX_RGBA8)])
    d_payload = torch.from_numpy(np.concatenate([payload, np.zeros(16, np.uint8)])).cuda()
    d_heap = torch.full((nbytes + 4,), FILL, dtype=torch.uint8, device="cuda:0")

    def run(descs=descs, sources=sources, n=1, pp=None, pb=len(payload), tp=None, tb=nbytes, dptr=True):
        return L.zr_jpeg_decode_device(0, None, descs.ctypes.data if dptr else None, sources.ctypes.data, n, d_payload.data_ptr() if pp is None else pp, pb,
                                       d_heap.data_ptr() if tp is None else tp, tb)

    assert run(dptr=False) == INVALID and run(n=0) == INVALID and run(pp=0) == INVALID and run(tp=0) == INVALID
    assert run(pp=d_payload.data_ptr() + 8) == INVALID and run(tp=d_heap.data_ptr() + 2) == INVALID
    assert run(pb=len(payload) - 17) == INVALID, "a record that ends beyond payload_bytes"
    assert run(tb=int(descs["offset"][0]) + 33 * 17 * 4 - 1) == INVALID, "a level 0 that ends beyond texel_bytes"
    d2 = descs.copy()
    d2["format"] = wire.TEX_RG8
    assert run(descs=d2) == INVALID
    torch.cuda.synchronize()
    assert (d_heap.cpu().numpy() == FILL).all(), "a refused call wrote"
    # more than 2^32 - 1 texels in one call: 1025 textures of 2048 x 2048 that name the same (all-grey) record and the same place
    big = zjp.make_gray_record(np.zeros((256 * 256, 64)), 256, 256)
    n = 1025
    many_d, many_s = np.zeros(n, wire.TEXTURE_DESC), np.zeros(n, wire.TEXTURE_SOURCE)
    many_d["width"], many_d["height"], many_d["num_mips"], many_d["format"] = 2048, 2048, 1, wire.TEX_RGBA8
    many_s["encoding"] = wire.TEX_SRC_JPEG_COEF
    d_big, d_big_px = torch.from_numpy(big).cuda(), torch.zeros(2048 * 2048 * 4, dtype=torch.uint8, device="cuda:0")
    assert L.zr_jpeg_decode_device(0, None, many_d.ctypes.data, many_s.ctypes.data, n, d_big.data_ptr(), len(big), d_big_px.data_ptr(), 2048 * 2048 * 4) == INVALID
    assert b"2^32 - 1" in L.zr_last_error()
    # three textures that name one record and one place are fine
    rec = scene_io.pack_jpeg(FILES["64x64_gray_q90_bench"])
    many_d["width"], many_d["height"] = 64, 64
    d_rec = torch.from_numpy(rec).cuda()
    d_px = torch.full((64 * 64 * 4,), FILL, dtype=torch.uint8, device="cuda:0")
    assert L.zr_jpeg_decode_device(0, None, many_d.ctypes.data, many_s.ctypes.data, 3, d_rec.data_ptr(), len(rec), d_px.data_ptr(), 64 * 64 * 4) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_px.cpu().numpy(), scene_io.jpeg_expand(rec).reshape(-1))
    assert (d_heap.cpu().numpy() == FILL).all()
    # zr_jpeg_decode_device leaves the other encodings alone, and zr_bcn_decode_device leaves JPEG records to it
    src = np.zeros(1, wire.TEXTURE_SOURCE)
    got = api.jpeg_decode_device(zmg.descs([(0, 4, 4, 1, wire.TEX_RGBA8)]), src, np.arange(64, dtype=np.uint8), 64, fill=FILL)
    assert (got == FILL).all()
    src["encoding"] = wire.TEX_SRC_JPEG_COEF
    with pytest.raises(api.ZetaRayError):
        api.bcn_decode_device(zmg.descs([(0, 64, 64, 1, wire.TEX_RGBA8)]), src, rec, 64 * 64 * 4)


# ---- 4. the tolerance-mode library decodes to the same bytes
def test_fast_library_decodes_the_same_bytes():
    assert os.path.exists(FAST_LIB), "libzetaray_amd_fast.so is missing: __graft_entry__.build() builds it"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "jpegmath", "fast_check.py")], env=dict(os.environ, ZETARAY_AMD_LIB=FAST_LIB),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep == {"lib": "libzetaray_amd_fast.so", "bytes": 33 * 17 * 4 + 33 * 17 * 2 + 16 * 16 * 2 + 17 * 23 * 4, "bad": 0}
