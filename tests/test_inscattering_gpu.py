"""Inscattering voxel grid of the sky pass (RP/Sky/Inscattering.hlsl) and its compositing term (Compositing.hlsl:74-97) on the GPU, through the
C ABI: bit for bit against the test-side restatement (tests/inscatter), the passes around it unchanged, the error paths, the Renderer."""
import ctypes as C
import os

import numpy as np
import pytest

from zetaray_amd import scene_io, wire
from tests.inscatter import zis

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_B = dict(cam_pos=(1.3, 2.1, -3.2), view_dir=(-0.35, -0.25, 1.0))


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


def _cornell():
    return scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))


def _grid_gpu(api, sc, cb, sky=None, **kw):
    p = sky or api.Pass(api.PASS_SKY, 256, 128)
    if kw or sky is None:
        p.set_inscattering(True, **kw)
    p.render(cb, sc, None)
    return p.download_plane("inscattering")


def _assert_same(got, want, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} texels differ"


@pytest.mark.parametrize("pose,frame,kw", [
    ({}, 0, {}),
    (POSE_B, 5, {}),
    ({}, 1, dict(voxels=(160, 90), depth_map_exp=3.0, near_z=0.2, far_z=12.0)),
])
def test_grid_bit_exact(api, pose, frame, kw):
    host = _cornell()
    cb = scene_io.make_frame_constants(1920, 1080, frame_num=frame, **pose)
    got = _grid_gpu(api, api.Scene(host), cb, **kw)
    args = {k: v for k, v in kw.items()}
    want, _, vis = zis.grid(zis.Scene(host), cb, args.pop("voxels", (192, 108)), with_ls=True, **args)
    assert 0.02 < float((vis == 0).mean()) < 0.98
    _assert_same(got, want, "grid")


def test_grid_moved_instance_and_non_opaque(api):
    """visibility rays see the refitted tree after an instance moved, and skip ZR_INSTANCE_NON_OPAQUE instances (RAY_FLAG_CULL_NON_OPAQUE)"""
    host = _cornell()
    cb = scene_io.make_frame_constants(1920, 1080, frame_num=2)
    sc, osc = api.Scene(host), zis.Scene(host)
    sky = api.Pass(api.PASS_SKY, 256, 128)
    sky.set_inscattering(True)
    xform_of = {}
    inst, xf = scene_io.move_instance(host, 3, translation=host.instances["translation"][3] + np.float32([0.3, 0.25, -0.2]), xform_of=xform_of)
    sc.update_instances(inst, xf)
    osc.update_instances(inst, xf)
    moved = _grid_gpu(api, sc, cb, sky=sky)
    want, _, vis_moved = zis.grid(osc, cb, with_ls=True)
    _assert_same(moved, want, "moved instance")
    # the instance that shadows the most voxels becomes non-opaque: its shadow disappears
    small = (24, 14)
    base_lit = int(zis.grid(zis.Scene(host), cb, small, with_ls=True)[2].sum())
    gains = []
    for k in range(len(host.instances)):
        h2 = _cornell()
        h2.instance_mask[k] |= wire_non_opaque()
        gains.append(int(zis.grid(zis.Scene(h2), cb, small, with_ls=True)[2].sum()) - base_lit)
    k = int(np.argmax(gains))
    assert gains[k] > 0
    h2 = _cornell()
    h2.instance_mask[k] |= wire_non_opaque()
    got = _grid_gpu(api, api.Scene(h2), cb)
    want2, _, vis2 = zis.grid(zis.Scene(h2), cb, with_ls=True)
    _assert_same(got, want2, "non-opaque instance")
    _, _, vis_opaque = zis.grid(zis.Scene(_cornell()), cb, with_ls=True)
    assert int(vis2.sum()) > int(vis_opaque.sum())


def wire_non_opaque():
    return np.uint8(0x80)      # ZR_INSTANCE_NON_OPAQUE (zr_wire.h)


def _sun_sky_frame(api, host, w, h, cb):
    r = api.Renderer(host, w, h, params=wire.default_params())
    r.enable_sky_direct()
    r.enable_compositing()
    r.render_frame(cb)
    return r


@pytest.mark.parametrize("accumulate", [False, True])
def test_compositing_bit_exact_1080p(api, accumulate):
    host = _cornell()
    w, h = 1920, 1080
    kw = dict(accumulate=1, camera_static=1, num_frames_static=3) if accumulate else {}
    cb = scene_io.make_frame_constants(w, h, frame_num=3, **kw)
    r = _sun_sky_frame(api, host, w, h, cb)
    base = r.p_composit.download()
    # never-bound compositing, and one bound then unbound, leave the image as it was
    comp = api.Pass(api.PASS_COMPOSITING, w, h)
    for which, plane in ((api.IN_INDIRECT, r.p_indirect), (api.IN_SKY_DI, r.p_sky_direct)):
        comp.set_input(which, plane.output_ptr()[0])
    comp.bind_inscattering(r.p_sky)
    with pytest.raises(RuntimeError):
        comp.render(cb, r.scene, r.gbuffer)              # the sky pass's grid is disabled
    r.p_sky.set_inscattering(True)
    comp.bind_inscattering(None)
    comp.render(cb, r.scene, r.gbuffer)
    assert np.array_equal(comp.download().view(np.uint32), base.view(np.uint32))
    # the LUT does not move when the grid is on
    lut0 = r.p_sky.download_plane("sky_lut").copy()
    r.p_sky.render(cb, r.scene, None)
    assert np.array_equal(r.p_sky.download_plane("sky_lut"), lut0)
    grid = r.p_sky.download_plane("inscattering")
    _assert_same(grid, zis.grid(zis.Scene(host), cb), "grid")
    comp.bind_inscattering(r.p_sky)
    comp.render(cb, r.scene, r.gbuffer)
    got = comp.download()
    arrays, _ = r.gbuffer.download()
    mr, depth = arrays[wire.GB_PLANE_NAMES.index("metallic_roughness")], arrays[wire.GB_PLANE_NAMES.index("depth")]
    want = zis.composite(cb, mr.reshape(h, w), depth.reshape(h, w), base, grid)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{bad} floats differ"
    changed = (got != base).any(-1)
    assert changed.mean() > 0.3
    invalid = (mr.reshape(h, w).astype(np.uint32) & 0xff & 4) != 0      # GBuffer::Flags::invalid (ZR_GBUF_INVALID)
    if not accumulate:
        assert invalid.any() and not changed[invalid].any(), "sky pixels must stay as they were"
    # re-enabled with other voxel counts: the binding follows the new grid
    r.p_sky.set_inscattering(True, voxels=(160, 90), depth_map_exp=1.5, near_z=0.1, far_z=20.0)
    r.p_sky.render(cb, r.scene, None)
    comp.render(cb, r.scene, r.gbuffer)
    grid2 = r.p_sky.download_plane("inscattering")
    _assert_same(grid2, zis.grid(zis.Scene(host), cb, (160, 90), 1.5, 0.1, 20.0), "re-enabled grid")
    want2 = zis.composite(cb, mr.reshape(h, w), depth.reshape(h, w), base, grid2, 1.5, 0.1, 20.0)
    assert np.array_equal(comp.download().view(np.uint32), want2.view(np.uint32))


def test_error_paths(api):
    L = api.lib()
    host = _cornell()
    sky = api.Pass(api.PASS_SKY, 256, 128)
    comp = api.Pass(api.PASS_COMPOSITING, 64, 64)
    INVALID = 1
    for args in ((1, 0, 0, 0.5, 0.5, 30.0), (1, 0, 0, 6.0, 0.5, 30.0), (1, 0, 0, 2.0, 30.0, 30.0), (1, 0, 0, 2.0, -1.0, 30.0),
                 (1, 0, 108, 2.0, 0.5, 30.0), (1, 5000, 10, 2.0, 0.5, 30.0)):
        assert L.zr_pass_set_inscattering(sky.h, *args) == INVALID, args
    assert L.zr_pass_set_inscattering(comp.h, 1, 0, 0, 2.0, 0.5, 30.0) == INVALID
    assert L.zr_pass_bind_inscattering(sky.h, sky.h) == INVALID
    assert L.zr_pass_bind_inscattering(comp.h, comp.h) == INVALID
    with pytest.raises(RuntimeError):
        sky.output_ptr(wire.OUT_INSCATTERING)          # disabled: no grid
    sky.set_inscattering(True)
    _, gw, gh, bpp = sky.output_ptr(wire.OUT_INSCATTERING)
    assert (gw, gh, bpp) == (192, 108 * 128, 4)
    # compositing with the grid on a tile of the split screen is refused
    sc = api.Scene(host)
    gb = api.GBuffer(64, 64)
    gb.set_tile_origin(32, 32)
    comp.bind_inscattering(sky)
    cb = scene_io.make_frame_constants(128, 128)
    with pytest.raises(RuntimeError, match="tile"):
        comp.render(cb, sc, gb)
    comp.bind_inscattering(None)
    sky.set_inscattering(False)
    with pytest.raises(RuntimeError):
        sky.output_ptr(wire.OUT_INSCATTERING)


def test_renderer_enable_inscattering_end_to_end(api):
    host = _cornell()
    w, h = 320, 180
    r = api.Renderer(host, w, h, params=wire.default_params())
    r.enable_sky_direct()
    r.enable_inscattering()
    ref = api.Renderer(host, w, h, params=wire.default_params())
    ref.enable_sky_direct()
    ref.enable_compositing()
    sky = api.Pass(api.PASS_SKY, 256, 128)
    sky.set_inscattering(True)
    comp = api.Pass(api.PASS_COMPOSITING, w, h)
    comp.bind_inscattering(sky)
    for f in range(4):
        cb = scene_io.make_frame_constants(w, h, frame_num=f + 1, cam_pos=(0.1 * f, 1.2, -4.043))
        r.render_frame(cb)
        ref.render_frame(cb)
        sky.render(cb, ref.scene, None)
        comp.set_input(api.IN_INDIRECT, ref.p_indirect.output_ptr()[0])
        comp.set_input(api.IN_SKY_DI, ref.p_sky_direct.output_ptr()[0])
        comp.render(cb, ref.scene, ref.gbuffer)
        assert np.array_equal(r.p_sky.download_plane("inscattering"), sky.download_plane("inscattering")), f"frame {f}"
        assert np.array_equal(r.p_composit.download().view(np.uint32), comp.download().view(np.uint32)), f"frame {f}"
    r.p_sky.enable_timing(True)
    r.render_frame(cb)
    assert "inscattering" in r.p_sky.timings()


def test_cpp_mirror_renders_inscattering_like_the_python_renderer(api):
    """the C++ mirror (Sky::SetInscatteringEnablement, Compositing's INSCATTERING descriptor + voxel-grid parameters, scheduled by the RenderGraph)
    gives the composited bytes and the grid of Renderer.enable_inscattering() over the same frames"""
    host = _cornell()
    w, h, n = 160, 96, 3
    cbs = np.ascontiguousarray(np.stack([scene_io.make_frame_constants(w, h, frame_num=f + 1) for f in range(n)]))
    L = C.CDLL(os.path.join(ROOT, "zetaray_amd", "libzetaray_host.so"))
    L.zrh_render_sequence_sky_inscattering.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    comp = np.zeros((h, w, 4), np.float32)
    grid = np.zeros((zis.SLICES, 90, 160), np.uint32)
    desc = host.desc()
    assert L.zrh_render_sequence_sky_inscattering(C.addressof(desc), cbs.ctypes.data, n, w, h, api.INTEGRATOR_RESTIR_PT, 160, 90,
                                                  comp.ctypes.data, grid.ctypes.data) == 0
    r = api.Renderer(host, w, h, integrator=api.INTEGRATOR_RESTIR_PT)
    r.enable_sky_direct()
    r.enable_inscattering(voxels=(160, 90))
    for f in range(n):
        r.render_frame(cbs[f])
    assert np.array_equal(r.p_sky.download_plane("inscattering"), grid)
    assert np.array_equal(r.p_composit.download().view(np.uint32), comp.view(np.uint32))
    assert (comp[..., :3] > 0).any()
