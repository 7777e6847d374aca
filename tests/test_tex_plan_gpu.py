"""The texture path as a whole (zr_tex_plan.h plans it, RunTexturePlan of zr_api.hip enqueues it): every source encoding in one scene with its chains out
of order in the heap, and calls enqueued back to back on one stream, whose job tables live in stream-ordered allocations that are freed behind the
kernels.  Expected bytes come from the host (scene_io.decode_textures, scene_io.mip_generate, scene_io.jpeg_expand), never from a kernel."""
import ctypes as C

import numpy as np
import pytest

from tests.bcnmath import zbc
from tests.jpegmath import zjp
from tests.mipmath import zmg
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
FILL = 0xA5
FILES = {n: d for n, d, _ in zjp.load_fixture()}


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


def test_scene_with_all_five_encodings(api):
    sc, order = zjp.five_encoding_box(np.random.default_rng(17))
    host, _ = zjp.five_encoding_box(np.random.default_rng(17))
    host.decode_textures()
    assert sorted(set(int(e) for e in sc.texture_sources["encoding"])) == [wire.TEX_SRC_RAW, wire.TEX_SRC_BC7, wire.TEX_SRC_BC5, wire.TEX_SRC_RAW_MIP0, wire.TEX_SRC_JPEG_COEF]
    assert order != sorted(order) and list(np.argsort(sc.textures["offset"])) == order, "the chains are not in texture order"
    got = api.Scene(sc).get_texels()
    assert len(got) == sc.texel_heap_bytes == len(host.texels)
    assert np.array_equal(got, host.texels), np.nonzero(got != host.texels)[0][:8]
    inside = np.zeros(len(got), bool)
    for t in sc.textures:
        inside[int(t["offset"]):int(t["offset"]) + zmg.chain_bytes(int(t["width"]), int(t["height"]), int(t["num_mips"]), int(t["format"]))] = True
    assert inside[:8].sum() == 0 and inside[-24:].sum() == 0 and (~inside).sum() >= 8 + 24 + sum(4 + 8 * k for k in range(5))
    assert (got[~inside] == 0).all(), "every byte outside the chains is zero"
    assert (got[inside] != 0).any()


def _bc7_call(rng):
    """one 8 x 8 BC7 chain of 2 mips at offset 12 -> (descs, sources, payload, heap bytes, expected heap)"""
    blocks, texels = [], []
    for w in (8, 4):
        b = rng.integers(0, 256, (zbc.mip_blocks(w, w), 16), dtype=np.uint8)
        blocks.append(b.reshape(-1))
        texels.append(zbc.decode_mip(zbc.BC7, b, w, w).reshape(-1))
    want = np.full(12 + 8 * 8 * 4 + 4 * 4 * 4 + 36, FILL, np.uint8)
    want[12:12 + 320] = np.concatenate(texels)
    src = np.zeros(1, wire.TEXTURE_SOURCE)
    src["encoding"] = wire.TEX_SRC_BC7
    return zmg.descs([(12, 8, 8, 2, wire.TEX_RGBA8)]), src, np.concatenate(blocks), len(want), want


def _jpeg_call(cmap, fmt):
    """the 33 x 17 4:2:0 file as one level 0 at offset 20"""
    rec = scene_io.pack_jpeg(FILES["33x17_420_q90_noise"], "a.jpg", cmap)
    px = scene_io.jpeg_expand(rec).reshape(-1)
    want = np.full(20 + len(px) + 50, FILL, np.uint8)
    want[20:20 + len(px)] = px
    src = np.zeros(1, wire.TEXTURE_SOURCE)
    src["encoding"] = wire.TEX_SRC_JPEG_COEF
    return zmg.descs([(20, 33, 17, 1, fmt)]), src, rec, len(want), want


def _mip_call(rng):
    """one 5 x 3 RG8 chain at offset 4: the heap with a random level 0, and what the host generates in it"""
    rows = [(4, 5, 3, zmg.full_mips(5, 3), wire.TEX_RG8)]
    heap = np.full(4 + zmg.chain_bytes(5, 3, rows[0][3], wire.TEX_RG8) + 30, FILL, np.uint8)
    heap[4:4 + 30] = rng.integers(0, 256, 30, dtype=np.uint8)
    return zmg.descs(rows), heap, scene_io.mip_generate(zmg.descs(rows), heap.copy())


def test_back_to_back_calls_on_one_stream(api):
    """Two calls of each entry point into different heaps on one non-null stream, no synchronize between them: the second call's tables are allocated
    while the first call's frees are pending.  One synchronize, then both heaps are right byte for byte and the fill outside the chains untouched."""
    import torch
    L = api.lib()
    rng = np.random.default_rng(23)
    st = torch.cuda.Stream()
    bc = [_bc7_call(rng) for _ in range(2)]
    jp = [_jpeg_call(wire.JPEG_MAP_RGBA, wire.TEX_RGBA8_SRGB), _jpeg_call(wire.JPEG_MAP_BG, wire.TEX_RG8)]
    mg = [_mip_call(rng) for _ in range(2)]
    assert not np.array_equal(bc[0][4], bc[1][4]) and len(jp[0][4]) != len(jp[1][4]) and not np.array_equal(mg[0][2], mg[1][2])
    d_payload = [torch.from_numpy(c[2].copy()).cuda() for c in bc + jp]
    d_heap = [torch.full((c[3],), FILL, dtype=torch.uint8, device="cuda:0") for c in bc + jp] + [torch.from_numpy(m[1].copy()).cuda() for m in mg]
    torch.cuda.synchronize()
    for k, (descs, src, payload, nbytes, _) in enumerate(bc):
        api._check(L.zr_bcn_decode_device(0, st.cuda_stream, descs.ctypes.data, src.ctypes.data, 1, d_payload[k].data_ptr(), len(payload), d_heap[k].data_ptr(), nbytes))
    for k, (descs, src, payload, nbytes, _) in enumerate(jp):
        api._check(L.zr_jpeg_decode_device(0, st.cuda_stream, descs.ctypes.data, src.ctypes.data, 1, d_payload[2 + k].data_ptr(), len(payload), d_heap[2 + k].data_ptr(), nbytes))
    for k, (descs, heap, _) in enumerate(mg):
        api._check(L.zr_mipgen_device(0, st.cuda_stream, descs.ctypes.data, 1, d_heap[4 + k].data_ptr(), len(heap)))
    st.synchronize()
    want = [c[4] for c in bc + jp] + [m[2] for m in mg]
    for k, (d, w) in enumerate(zip(d_heap, want)):
        got = d.cpu().numpy()
        assert np.array_equal(got, w), (k, np.nonzero(got != w)[0][:8])
    assert all((w == FILL).sum() >= 30 and (w != FILL).any() for w in want)
