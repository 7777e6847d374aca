"""ReSTIR GI's spatial reuse stage (k_rgi_spatial, zr_pass_set_rgi_spatial) on the GPU, through the C ABI.  The stage has no reference counterpart:
the kernel is held bit for bit to the same stage function run on the host (tests/rgispatial) over the GPU's own downloaded G-buffer and reservoir
planes, to its own staged / tiled / switched-off forms, and -- as an estimator -- to the K9 path tracer.  Run on the GPU box with -m gpu."""
import numpy as np
import pytest

from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


def _frames(sc, w, h, n, cam, offs=None, first=1, **kw):
    """frame constants 1..n; cam(f) = camera position; the previous frame's view is carried over"""
    prev = None
    for f in range(first, first + n):
        cb = scene_io.make_frame_constants(w, h, frame_num=f, num_emissives=len(sc.emissives), cam_pos=cam(f), **kw)
        if offs is not None:
            scene_io.set_texture_heap_offsets(cb, offs)
        if prev is not None:
            cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
        prev = cb.copy()
        yield f, cb


def _planes(p):
    return {k: p.download_plane("gi_" + k) for k in "ABC"}


def _spatial_counters(p):
    c = p.kernel_counters()
    p.read_counters(reset=True)
    return c.get("rgi_spatial", (0, 0))


CORNELL_CAM = lambda f: (0.05 * max(0, f - 2), 1.2, -4.043)      # noqa: E731


@pytest.mark.parametrize("num_samples", [1, 2])
@pytest.mark.parametrize("case", ["cornell_moving", "materials_presampled", "textured"])
def test_rgi_spatial_bit_exact_vs_host_executor(api, cornell_emissive, case, num_samples):
    """FINAL and the kernel's ray counters == rgi::SpatialResample run serially on the host over the GPU's own G-buffer and GI planes, 5 frames"""
    from tests.hostexec import zhx
    from tests.rgispatial import zrs
    w, h, offs = 96, 64, None
    prm = wire.default_params()
    if case == "cornell_moving":
        sc, cam = cornell_emissive, CORNELL_CAM
    else:
        sc = scene_io.make_synthetic_scene(num_tris=3000, num_emissive=1500, seed=11)
        prm.max_non_tr_bounces, prm.max_glossy_tr_bounces = 5, 7
        if case == "materials_presampled":
            prm.presampling, prm.num_sample_sets, prm.sample_set_size = 1, 16, 64
            cam = lambda f: (0.03 * max(0, f - 2), 0, -3.5)      # noqa: E731
        else:
            offs = scene_io.add_test_textures(sc)
            cam = lambda f: (0.3 + 0.05 * max(0, f - 2), 0.2, -3.6)      # noqa: E731
    hx = zhx.HostExecScene(sc)
    r = api.Renderer(sc, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_GI)
    r.set_rgi_spatial(num_samples, 12.0 if num_samples == 1 else 0.0)
    rays = 0
    for f, cb in _frames(sc, w, h, 5, cam, offs):
        r.render_frame(cb)
        got = r.final()
        want, cnt = zrs.spatial(hx, cb, r.gbuffer.download(), _planes(r.p_indirect), num_samples, 12.0 if num_samples == 1 else 0.0)
        assert not np.isnan(got).any()
        mism = int((got[..., :3].view(np.uint32) != want[..., :3].view(np.uint32)).any(axis=2).sum())
        assert mism == 0, f"{case} frame {f}: {mism} pixels differ"
        assert _spatial_counters(r.p_indirect) == cnt, f"{case} frame {f}: ray counters"
        rays += cnt[1]
    assert got[..., :3].max() > 0 and rays > 0


def test_rgi_spatial_off_is_unchanged(api, cornell_emissive):
    """num_samples = 0 after having been on: FINAL, planes A / B / C and the counters equal a pass that never had it on"""
    w, h = 96, 64
    prm = wire.default_params()
    a = api.Renderer(cornell_emissive, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_GI)
    b = api.Renderer(cornell_emissive, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_GI)
    a.set_rgi_spatial(2)
    differed = False
    for f, cb in _frames(cornell_emissive, w, h, 6, CORNELL_CAM):
        if f == 4:
            a.set_rgi_spatial(0)
        a.render_frame(cb)
        b.render_frame(cb)
        pa, pb = _planes(a.p_indirect), _planes(b.p_indirect)
        for k in "ABC":      # the spatial stage writes nothing back, on or off
            assert np.array_equal(pa[k].view(np.uint8), pb[k].view(np.uint8)), f"frame {f}: plane {k}"
        ca, cb_ = a.p_indirect.kernel_counters(), b.p_indirect.kernel_counters()
        a.p_indirect.read_counters(reset=True), b.p_indirect.read_counters(reset=True)
        if f >= 4:
            assert np.array_equal(a.final().view(np.uint32), b.final().view(np.uint32)), f"frame {f}: FINAL"
            assert ca == cb_ and "rgi_spatial" not in ca, f"frame {f}: counters {ca} {cb_}"
            assert "rgi_spatial" not in a.p_indirect.timings()
        else:
            differed = differed or not np.array_equal(a.final().view(np.uint32), b.final().view(np.uint32))
            assert ca.get("rgi") == cb_.get("rgi")
    assert differed, "the stage never changed FINAL while it was on"


def test_rgi_spatial_staged_and_tiled(api, cornell_emissive):
    """TEMPORAL then SPATIAL through zr_pass_render_stage == zr_pass_render; two half-screen tiles with a 32-px apron on one device, ZR_HALO_FINAL packed /
    unpacked between the stages, == the full frame on the owned pixels, bit for bit"""
    from zetaray_amd import tiling
    w, h = 192, 128
    prm = wire.default_params()
    full = api.Renderer(cornell_emissive, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_GI)
    staged = tiling.TiledRestirPT(cornell_emissive, w, h, 1, 0, params=prm, kind="restir_gi")
    ranks = [tiling.TiledRestirPT(cornell_emissive, w, h, 2, k, params=prm, kind="restir_gi") for k in range(2)]
    assert ranks[0].bpp == 40 and all(r.ext != r.tile for r in ranks)
    full.set_rgi_spatial(2)
    for t in [staged] + ranks:
        t.set_rgi_spatial(2)
    cam = lambda f: (0.05 * f, 1.2, -4.043 + 0.02 * f)      # noqa: E731
    for f, cb in _frames(cornell_emissive, w, h, 4, cam):
        full.render_frame(cb)
        want = full.final()
        staged.stage_temporal(cb)
        staged.stage_spatial(cb)
        assert np.array_equal(staged.final_tile()[1].view(np.uint32), want.view(np.uint32)), f"frame {f}: staged"
        n = tiling.render_frame_in_process(ranks, cb)
        assert n == 1, "one exchange per frame: ZR_HALO_FINAL between the stages"
        img = np.zeros_like(want)
        for r in ranks:
            (x0, y0, tw, th), t = r.final_tile()
            img[y0:y0 + th, x0:x0 + tw] = t
        mism = int((img.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())
        assert mism == 0, f"frame {f}: {mism} pixels of the tiled frame differ"
    assert want[..., :3].max() > 0


def test_rgi_spatial_tiled_switched_on_and_off_mid_sequence(api, cornell_emissive):
    """the setter takes effect with the next frame, so the stage may come on after frames rendered without it (and go off again).  Two half-screen
    tiles, camera moving every frame (the temporal reprojection crosses the seam): off for frames 1-2, on for 3-4, off for 5-6; the tiled frame equals
    the full frame on the owned pixels bit for bit in every frame.  The exchange count shows the policy: whether the apron already holds the "previous"
    set depends on whether the PREVIOUS frame exchanged ZR_HALO_FINAL between its stages, not on this frame's setting -- frame 3 exchanges twice (before
    it and between its stages), frame 5 not at all.
    A radius whose taps would leave the 32-px apron is refused on a split frame (ValueError), not on a whole one."""
    from zetaray_amd import tiling
    w, h = 192, 128
    prm = wire.default_params()
    full = api.Renderer(cornell_emissive, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_GI)
    ranks = [tiling.TiledRestirPT(cornell_emissive, w, h, 2, k, params=prm, kind="restir_gi") for k in range(2)]
    whole = tiling.TiledRestirPT(cornell_emissive, w, h, 1, 0, params=prm, kind="restir_gi")
    # reach = ceil(radius * |(-0.875, 7/9)| + 0.5) px per axis: 26.9 -> 32, 27 -> 33, the 64-px maximum -> 76
    assert [tiling.rgi_spatial_reach(r) for r in (0.0, 26.9, 27.0, 64.0)] == [20, 32, 33, 76]
    for bad in (27.0, 64.0):
        with pytest.raises(ValueError):
            ranks[0].set_rgi_spatial(2, bad)
        assert not ranks[0].rgi_spatial
    ranks[0].set_rgi_spatial(0, 64.0), ranks[0].set_rgi_spatial(1, 26.9), ranks[0].set_rgi_spatial(0)
    whole.set_rgi_spatial(2, 64.0)
    cam = lambda f: (0.05 * f, 1.2, -4.043 + 0.02 * f)      # noqa: E731
    on = {1: 0, 2: 0, 3: 2, 4: 2, 5: 0, 6: 0}
    exchanges = {1: 0, 2: 1, 3: 2, 4: 1, 5: 0, 6: 1}
    for f, cb in _frames(cornell_emissive, w, h, 6, cam):
        full.set_rgi_spatial(on[f])
        for t in ranks:
            t.set_rgi_spatial(on[f])
        full.render_frame(cb)
        want = full.final()
        n = tiling.render_frame_in_process(ranks, cb)
        img = np.zeros_like(want)
        for r in ranks:
            (x0, y0, tw, th), t = r.final_tile()
            img[y0:y0 + th, x0:x0 + tw] = t
        mism = int((img.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())
        assert mism == 0, f"frame {f} (stage {'on' if on[f] else 'off'}): {mism} pixels of the tiled frame differ"
        assert n == exchanges[f], f"frame {f}: {n} exchanges"
    assert want[..., :3].max() > 0


def _block_err(x, ref):
    """relative L2 of the 8 x 8-block means of x against ref's"""
    b = lambda a: a[..., :3].reshape(a.shape[0] // 8, 8, a.shape[1] // 8, 8, 3).mean(axis=(1, 3))      # noqa: E731
    return float(np.linalg.norm(b(x) - b(ref)) / np.linalg.norm(b(ref)))


def test_rgi_spatial_agrees_with_k9_at_scale(api, cornell_emissive):
    """emissive Cornell 256 x 256, 1024 frames, static camera.  E(x) = relative L2 of the 8 x 8-block means of x's average against K9's; K9' = K9 over
    the disjoint frame numbers 1025..2048.  E(spatial) <= E(temporal-only) + E(K9'): two estimates of one mean differ by at most the sum of their noises.
    The same run holds the shipped default radius (16 px, which this frame is large enough for) to the variance condition of
    tests/test_rgi_spatial_cpu.py: per-pixel variance over the last 100 frames, averaged over the image and the channels, spatial on / off < 1.
    Measured on the MI355X: see DESIGN.md section 9."""
    w, h, n = 256, 256, 1024
    prm = wire.default_params()
    k9 = api.Renderer(cornell_emissive, w, h, params=prm)
    gt = api.Renderer(cornell_emissive, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_GI)
    gs = api.Renderer(cornell_emissive, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_GI)
    gs.set_rgi_spatial(2)
    acc = {k: np.zeros((h, w, 4), np.float64) for k in ("k9", "k9b", "t", "s")}
    sq, last = {k: np.zeros((h, w, 3), np.float64) for k in "ts"}, {k: np.zeros((h, w, 3), np.float64) for k in "ts"}
    cam = lambda f: (0.0, 1.2, -4.043)      # noqa: E731
    for f, cb in _frames(cornell_emissive, w, h, n, cam):
        for key, r in (("k9", k9), ("t", gt), ("s", gs)):
            r.render_frame(cb)
            img = r.final()
            acc[key] += img
            if key in sq and f > n - 100:
                last[key] += img[..., :3]
                sq[key] += img[..., :3].astype(np.float64) ** 2
    for f, cb in _frames(cornell_emissive, w, h, n, cam, first=n + 1):
        k9.render_frame(cb)
        acc["k9b"] += k9.final()
    assert not any(np.isnan(a).any() for a in acc.values())
    e_s, e_t, e_0 = _block_err(acc["s"], acc["k9"]), _block_err(acc["t"], acc["k9"]), _block_err(acc["k9b"], acc["k9"])
    print("rgi spatial at scale: E(spatial) %.5f E(temporal-only) %.5f E(K9') %.5f" % (e_s, e_t, e_0))
    var = {k: float((sq[k] / 100 - (last[k] / 100) ** 2).mean()) for k in "ts"}
    print("rgi spatial at scale: variance ratio (on / off) at the 16-px default %.4f" % (var["s"] / var["t"]))
    assert e_s <= e_t + e_0, (e_s, e_t, e_0)
    assert var["s"] / var["t"] < 1.0, var


def test_rgi_spatial_accumulates_once_per_frame(api, cornell_emissive):
    """cb.accumulate with a static camera: FINAL after n frames == the sum of the per-frame spatial outputs (the host executor accumulating onto its own
    plane over the GPU's planes), bit for bit -- k_rgi's own radiance does not reach FINAL"""
    from tests.hostexec import zhx
    from tests.rgispatial import zrs
    w, h = 96, 64
    prm = wire.default_params()
    hx = zhx.HostExecScene(cornell_emissive)
    r = api.Renderer(cornell_emissive, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_GI)
    r.set_rgi_spatial(2)
    acc, single = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 3), np.float64)
    for f in range(1, 7):
        cb = scene_io.make_frame_constants(w, h, frame_num=f, num_emissives=len(cornell_emissive.emissives), accumulate=1, camera_static=1, num_frames_static=f)
        r.render_frame(cb)
        gb, planes = r.gbuffer.download(), _planes(r.p_indirect)
        zrs.spatial(hx, cb, gb, planes, 2, final=acc)
        cb1 = cb.copy()
        cb1["accumulate"] = 0
        single += zrs.spatial(hx, cb1, gb, planes, 2)[0][..., :3]
        got = r.final()
        assert np.array_equal(got[..., :3].view(np.uint32), acc[..., :3].view(np.uint32)), f"frame {f}"
    assert got[..., :3].max() > 0
    # ... and that sum is the sum of the frames' single contributions (float32 running sum against a float64 one)
    assert np.allclose(got[..., :3], single, rtol=1e-5, atol=1e-7)


def test_rgi_spatial_setter_arguments_on_device(api, cornell_emissive):
    """every argument error; with ReSTIR PT and with the path tracer the value is stored and changes nothing"""
    from tests.rgispatial import setter
    setter.check_setter_arguments()
    w, h = 96, 64
    for integ in (api.INTEGRATOR_RESTIR_PT, api.INTEGRATOR_PATH_TRACING):
        a = api.Renderer(cornell_emissive, w, h, params=wire.default_params(), integrator=integ)
        b = api.Renderer(cornell_emissive, w, h, params=wire.default_params(), integrator=integ)
        a.set_rgi_spatial(2, 8.0)
        for f, cb in _frames(cornell_emissive, w, h, 3, CORNELL_CAM):
            a.render_frame(cb)
            b.render_frame(cb)
            assert np.array_equal(a.final().view(np.uint32), b.final().view(np.uint32)), f"integrator {integ} frame {f}"
            assert a.p_indirect.kernel_counters() == b.p_indirect.kernel_counters()
            assert "rgi_spatial" not in a.p_indirect.timings()
