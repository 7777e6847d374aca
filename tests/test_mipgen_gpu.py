"""The mip generation on the GPU (zr_tu_mipgen.hip) against include/zr_mipgen.h on the host (zrh_mip_generate), byte for byte: on caller buffers
(zr_mipgen_device) and through the scene path (zr_scene_create_compressed with ZR_TEX_SRC_RAW_MIP0 sources).  Expected bytes never come from the kernel."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.bcnmath import zbc
from tests.mipmath import zmg
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
ROOT = zmg.ROOT
FAST_LIB = os.path.join(ROOT, "zetaray_amd", "libzetaray_amd_fast.so")
FILL = 0xA5
SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 3), (1, 7), (7, 1), (9, 7), (17, 5), (64, 64), (65, 33), (129, 127), (258, 6), (256, 256)]      # (w, h)


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


@pytest.fixture(scope="module")
def stream(api):
    import torch
    return torch.cuda.Stream()


def _heap_with(rng, rows, tail=64):
    """rows of (offset, w, h, mips, fmt): a heap filled with FILL, random level 0s in place; returns (heap, expected heap from the header on the host)"""
    end = max(off + zmg.chain_bytes(w, h, mips, fmt) for off, w, h, mips, fmt in rows)
    heap = np.full(end + tail, FILL, np.uint8)
    for off, w, h, mips, fmt in rows:
        n = w * h * zmg.channels(fmt)
        heap[off:off + n] = rng.integers(0, 256, n, dtype=np.uint8)
    want = scene_io.mip_generate(zmg.descs(rows), heap.copy())
    return heap, want


# ---- 1. one chain per call: odd sizes, one-texel sides, more than one block, levels that start on a byte that is 2 mod 4
@pytest.mark.parametrize("fmt", list(zmg.FORMATS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_header(api, stream, fmt, size):
    w, h = size
    f = zmg.FORMATS[fmt]
    rng = np.random.default_rng(1000 * w + h)
    mips = zmg.full_mips(w, h)
    for off in (0, 12):
        rows = [(off, w, h, mips, f)]
        heap, want = _heap_with(rng, rows)
        got = api.mipgen_device(zmg.descs(rows), heap, stream=stream)
        n0 = w * h * zmg.channels(f)
        assert np.array_equal(got[:off + n0], heap[:off + n0]), "level 0 or the bytes before it changed"
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (off, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
        end = off + zmg.chain_bytes(w, h, mips, f)
        assert (got[end:] == FILL).all() and len(got) - end == 64


def test_rg8_levels_on_two_byte_boundaries(api, stream):
    """Heap offsets are multiples of 4, so a chain cannot start on a byte that is 2 mod 4, but an RG8 level of odd area is 2 mod 4 bytes long and every
    level behind it starts there: 9 x 7 (126 bytes) -> 4 x 3 -> 2 x 1 -> 1 x 1 reads and writes levels at 2 mod 4, 65 x 33 (4290 bytes) does so with
    more than one wave.  The sizes are in SIZES too; here the alignment is asserted, and the chain sits at an offset of 4 mod 8"""
    rng = np.random.default_rng(22)
    for w, h in ((9, 7), (65, 33), (5, 3)):
        assert (w * h * 2) % 4 == 2
        rows = [(4, w, h, zmg.full_mips(w, h), wire.TEX_RG8)]
        heap, want = _heap_with(rng, rows)
        got = api.mipgen_device(zmg.descs(rows), heap, stream=stream)
        assert np.array_equal(got, want), (w, h)


# ---- 2. five textures of mixed formats with padding in one call, partial chains among them
def test_mixed_textures_in_one_call(api, stream):
    rng = np.random.default_rng(3)
    spec = [(wire.TEX_RGBA8_SRGB, 37, 21, None), (wire.TEX_RG8, 64, 64, None), (wire.TEX_RGBA8, 8, 8, 1), (wire.TEX_RG8, 5, 3, None), (wire.TEX_RGBA8_SRGB, 129, 2, 3)]
    rows, at = [], 12
    for fmt, w, h, mips in spec:
        mips = zmg.full_mips(w, h) if mips is None else mips
        at = (at + 3) // 4 * 4
        rows.append((at, w, h, mips, fmt))
        at += zmg.chain_bytes(w, h, mips, fmt) + int(rng.integers(1, 40))
    heap, want = _heap_with(rng, rows)
    got = api.mipgen_device(zmg.descs(rows), heap, stream=stream)
    generated = np.zeros(len(heap), bool)
    for off, w, h, mips, fmt in rows:
        generated[off + w * h * zmg.channels(fmt):off + zmg.chain_bytes(w, h, mips, fmt)] = True
    assert np.array_equal(got[~generated], heap[~generated]), "level 0 or padding changed"
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert (got[generated] != FILL).any() and (~generated).sum() > 64


# ---- 3. the scene path
def _mixed_box(rng):
    """the untextured Cornell box with four maps in its heap: a BC7 sRGB 8 x 8 map and a RAW RGBA8 2 x 2 one with their stored chains, and two maps
    that carry level 0 alone, a 37 x 21 sRGB one and a 9 x 7 RG8 one"""
    sc = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))
    mips = zmg.full_mips(8, 8)
    blocks = np.concatenate([rng.integers(0, 256, zbc.mip_blocks(max(1, 8 >> m), max(1, 8 >> m)) * 16, dtype=np.uint8) for m in range(mips)])
    sc.add_texture_blocks(blocks, 8, 8, mips, wire.TEX_RGBA8_SRGB, wire.TEX_SRC_BC7)
    sc.add_texture_blocks(rng.integers(0, 256, 37 * 21 * 4, dtype=np.uint8), 37, 21, zmg.full_mips(37, 21), wire.TEX_RGBA8_SRGB, wire.TEX_SRC_RAW_MIP0)
    sc.add_texture_blocks(rng.integers(0, 256, 2 * 2 * 4 + 4, dtype=np.uint8), 2, 2, 2, wire.TEX_RGBA8, wire.TEX_SRC_RAW)
    sc.add_texture_blocks(rng.integers(0, 256, 9 * 7 * 2, dtype=np.uint8), 9, 7, zmg.full_mips(9, 7), wire.TEX_RG8, wire.TEX_SRC_RAW_MIP0)
    sc.add_texture_blocks(rng.integers(0, 256, 4 * 4 * 4, dtype=np.uint8), 4, 4, 1, wire.TEX_RGBA8, wire.TEX_SRC_RAW_MIP0)      # one level: nothing generated
    return sc


def test_scene_with_mixed_sources(api):
    sc = _mixed_box(np.random.default_rng(5))
    host = _mixed_box(np.random.default_rng(5))
    host.decode_textures()
    s = api.Scene(sc)
    got = s.get_texels()
    assert len(got) == sc.texel_heap_bytes == len(host.texels)
    assert np.array_equal(got, host.texels), np.nonzero(got != host.texels)[0][:8]
    # the heap zr_scene_create holds when handed the host's texels
    host.texture_payload = np.zeros(0, np.uint8)
    assert np.array_equal(api.Scene(host).get_texels(), host.texels)


def test_scene_path_on_the_png_cornell(api, tmp_path):
    path, _ = zmg.cornell_png_gltf(tmp_path, np.random.default_rng(11))
    dec, offs = scene_io.load_gltf_native(path)
    cmp_, offs2 = scene_io.load_gltf_native(path, textures="compressed")
    assert offs == offs2 and len(cmp_.texture_payload) and len(cmp_.texels) == 0 and len(dec.texels)
    assert (cmp_.texture_sources["encoding"] == wire.TEX_SRC_RAW_MIP0).sum() == 3
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


# ---- 4. refusals
def test_refusals_leave_nothing_behind(api):
    import torch
    L = api.lib()
    INVALID = 1      # ZR_ERR_INVALID_ARG
    sc = _mixed_box(np.random.default_rng(5))
    SENTINEL = 0x5A5A5A5A

    def variant(edit):
        descs, sources = sc.textures.copy(), sc.texture_sources.copy()
        desc, blocks = sc.desc(), sc.texture_blocks()
        desc.texels, desc.texel_bytes = None, sc.texel_heap_bytes
        desc.textures, blocks.sources = descs.ctypes.data, sources.ctypes.data
        edit(descs, sources, desc, blocks)
        h = C.c_void_p(SENTINEL)
        code = L.zr_scene_create_compressed(0, C.addressof(desc), C.addressof(blocks), C.byref(h))
        if code == 0:
            L.zr_scene_destroy(h)
        else:
            assert h.value == SENTINEL, "*out was written"
        return code

    assert variant(lambda d, s, desc, b: None) == 0, L.zr_last_error()
    payload_end = len(sc.texture_payload)
    assert int(sc.texture_sources["encoding"][4]) == wire.TEX_SRC_RAW_MIP0 and int(sc.texture_sources["offset"][4]) + 64 == payload_end
    edits = {
        "encoding 3 is still unknown": lambda d, s, desc, b: s["encoding"].__setitem__(1, 3),
        "encoding 9": lambda d, s, desc, b: s["encoding"].__setitem__(1, 9),
        "RAW_MIP0 offset not a multiple of 4": lambda d, s, desc, b: s["offset"].__setitem__(3, int(s["offset"][3]) + 2),
        "level 0 ends beyond the payload": lambda d, s, desc, b: setattr(b, "payload_bytes", payload_end - 1),
        "level 0 starts beyond the payload": lambda d, s, desc, b: s["offset"].__setitem__(1, 1 << 40),
        "desc: zero height": lambda d, s, desc, b: d["height"].__setitem__(1, 0),
        "desc: unknown format": lambda d, s, desc, b: d["format"].__setitem__(3, 3),
        "desc: outside the heap": lambda d, s, desc, b: setattr(desc, "texel_bytes", int(d["offset"][4]) + 63),
        "RAW needs the whole chain in the payload": lambda d, s, desc, b: (s["encoding"].__setitem__(4, wire.TEX_SRC_RAW), d["num_mips"].__setitem__(4, 2)),
    }
    for name, edit in edits.items():
        assert variant(edit) == INVALID, name
    # the level-0 size is what the chain-end check uses: the last source may end exactly with the payload although its chain is longer
    assert variant(lambda d, s, desc, b: setattr(b, "payload_bytes", payload_end)) == 0

    # zr_mipgen_device
    rows = [(0, 9, 7, 4, wire.TEX_RG8), (256, 8, 8, 4, wire.TEX_RGBA8_SRGB)]
    d_heap = torch.zeros(1024, dtype=torch.uint8, device="cuda:0")
    before = d_heap.cpu().numpy().copy()

    def run(rows, ptr=None, bytes_=1024, descs_ptr=True, n=None):
        d = zmg.descs(rows)
        return L.zr_mipgen_device(0, None, d.ctypes.data if descs_ptr else None, len(d) if n is None else n, d_heap.data_ptr() if ptr is None else ptr, bytes_)

    assert run(rows, descs_ptr=False) == INVALID and run(rows, ptr=0) == INVALID
    assert run(rows, descs_ptr=False, ptr=0, n=0) == 0, "n == 0 asks for nothing"
    assert run([(0, 9, 7, 4, 3)]) == INVALID, "unknown format"
    assert run([(0, 0, 7, 1, wire.TEX_RG8)]) == INVALID and run([(0, 9, 0, 1, wire.TEX_RG8)]) == INVALID, "zero dimensions"
    assert run([(0, 9, 7, 0, wire.TEX_RG8)]) == INVALID and run([(2, 9, 7, 4, wire.TEX_RG8)]) == INVALID
    assert run(rows, bytes_=256 + zmg.chain_bytes(8, 8, 4, wire.TEX_RGBA8_SRGB) - 1) == INVALID, "a chain that ends beyond texel_bytes"
    assert run(rows, ptr=d_heap.data_ptr() + 2) == INVALID
    torch.cuda.synchronize()
    assert np.array_equal(d_heap.cpu().numpy(), before), "a refused call wrote"
    assert run(rows, bytes_=256 + zmg.chain_bytes(8, 8, 4, wire.TEX_RGBA8_SRGB)) == 0
    torch.cuda.synchronize()
    # zr_bcn_decode_device leaves RAW_MIP0 to zr_mipgen_device
    src = np.zeros(1, wire.TEXTURE_SOURCE)
    src["encoding"] = wire.TEX_SRC_RAW_MIP0
    with pytest.raises(api.ZetaRayError):
        api.bcn_decode_device(zmg.descs([(0, 4, 4, 1, wire.TEX_RGBA8)]), src, np.zeros(64, np.uint8), 64)


# ---- 5. the tolerance-mode library generates the same bytes
def test_fast_library_generates_the_same_bytes():
    assert os.path.exists(FAST_LIB), "libzetaray_amd_fast.so is missing: __graft_entry__.build() builds it"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mipmath", "fast_check.py")], env=dict(os.environ, ZETARAY_AMD_LIB=FAST_LIB),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    n = zmg.chain_bytes(65, 33, 7, wire.TEX_RGBA8) - 65 * 33 * 4
    assert rep == {"lib": "libzetaray_amd_fast.so", "rgba8_srgb": n, "rgba8_srgb_bad": 0, "rgba8": n, "rgba8_bad": 0, "rg8": n // 2, "rg8_bad": 0}
