"""The ReSTIR PT reconnection debug views on the GPU (zetaray_amd.h zr_pass_set_rpt_debug_view), through the C ABI, tolerance 0 throughout.

tests/golden/rpt_views.npz holds what the REFERENCE's own shaders draw with each "Debug View" of its indirect-lighting pass selected
(tools/make_rpt_view_goldens.py) on the cases of tools/rpt_view_cases.py: between them K11, Reconnect_TtC and Reconnect_StC each are the kernel
that writes FINAL, with the early outs that write black, two spatial rounds, the sun + sky permutation and an accumulating sequence.  A view changes
nothing but FINAL: every other output of the same runs is compared with the sequence rendered without a view."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rpt_view_cases as VC  # noqa: E402
from zetaray_amd import scene_io, wire  # noqa: E402

pytestmark = pytest.mark.gpu
# what a view must leave alone: the seven reservoir planes, the target, the neighbour plane, both thread maps (+ the ray counters)
STATE_PLANES = ("A", "B", "C", "D", "E", "F", "G", "target", "neighbor", "map_ctn", "map_ntc")


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api as a
    assert a.device_count() >= 1, "no HIP device visible"
    return a


@pytest.fixture(scope="module")
def gold():
    return np.load(VC.GOLD)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8).ravel(), np.ascontiguousarray(b).view(np.uint8).ravel())


def _state(p):
    """the outputs a view must not change (plane A without its unused 4th byte)"""
    out = {}
    for nm in STATE_PLANES:
        a = p.download_plane(nm)
        out[nm] = (a & 0xffffff) if nm == "A" else a
    return out


def _run(api, case, view, overlap=False, view_until=None):
    """renders the case's sequence with `view` selected (view_until: NONE from that frame on); {frame: (FINAL rgb, state planes)} of the recorded
    frames + the ray counters of the whole sequence"""
    sc, _, prm = VC.scene_and_params(case)
    r = api.Renderer(sc, VC.W, VC.H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    if overlap:
        r.enable_frame_overlap(True)
    p = r.p_indirect
    p.set_rpt_debug_view(view)
    p.read_counters(reset=True)
    out = {}
    for f, cb in VC.frames_of(case):
        if view_until is not None and f == view_until:
            p.set_rpt_debug_view(wire.RPT_VIEW_NONE)
        r.render_frame(cb)
        if f in VC.recorded(case):
            out[f] = (np.ascontiguousarray(r.final()[..., :3]), _state(p))
    return out, p.read_counters()


_PLAIN = {}


def _plain(api, case):
    if case not in _PLAIN:
        _PLAIN[case] = _run(api, case, wire.RPT_VIEW_NONE)
    return _PLAIN[case]


@pytest.mark.parametrize("view", VC.VIEWS, ids=[VC.VIEW_NAMES[v] for v in VC.VIEWS])
@pytest.mark.parametrize("case", list(VC.CASES))
def test_view_equals_reference_and_changes_nothing_else(api, gold, case, view):
    got, counters = _run(api, case, view)
    plain, plain_counters = _plain(api, case)
    for f in VC.recorded(case):
        final, state = got[f]
        want = gold[VC.key(case, view, f)]
        mism = int((final.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())
        assert mism == 0, f"frame {f}: {mism} pixels of FINAL differ from the reference shaders' view"
        for nm in STATE_PLANES:
            assert _same(state[nm], plain[f][1][nm]), f"frame {f}: plane {nm} differs from the frame rendered without a view"
    assert counters == plain_counters, "ray counters differ from the sequence rendered without a view"


def test_view_differs_from_the_ordinary_frame(api, gold):
    """(guards the comparison above against a fixture that holds ordinary frames)"""
    for case in VC.CASES:
        plain, _ = _plain(api, case)
        f = VC.recorded(case)[-1]
        assert not _same(plain[f][0], gold[VC.key(case, wire.RPT_VIEW_K, f)])


def test_none_after_a_view_restores_the_ordinary_frame(api):
    case = "stc_cornell_moving"
    n = VC.num_frames(case)
    got, counters = _run(api, case, wire.RPT_VIEW_CASE, view_until=n - 1)      # the view up to frame n - 2, NONE for the recorded two
    plain, plain_counters = _plain(api, case)
    for f in VC.recorded(case):
        assert _same(got[f][0], plain[f][0]), f"frame {f}: FINAL differs from a pass that never had a view selected"
        for nm in STATE_PLANES:
            assert _same(got[f][1][nm], plain[f][1][nm]), f"frame {f}: plane {nm}"
    assert counters == plain_counters


def test_setter_argument_checks(api, cornell_emissive):
    L = api.lib()
    INVALID = 1      # ZR_ERR_INVALID_ARG
    assert L.zr_pass_set_rpt_debug_view(None, wire.RPT_VIEW_K) == INVALID
    p = api.Pass(api.PASS_INDIRECT, 64, 48, api.INTEGRATOR_RESTIR_PT)
    for bad in (-1, wire.RPT_VIEW_COUNT, 99):
        assert L.zr_pass_set_rpt_debug_view(p.h, bad) == INVALID
        assert b"unknown view" in L.zr_last_error()
    for v in range(wire.RPT_VIEW_COUNT):
        assert L.zr_pass_set_rpt_debug_view(p.h, v) == 0
    g = api.Pass(api.PASS_GBUFFER, 64, 48)
    assert L.zr_pass_set_rpt_debug_view(g.h, wire.RPT_VIEW_K) == INVALID
    assert b"INDIRECT" in L.zr_last_error()
    with pytest.raises(api.ZetaRayError):
        g.set_rpt_debug_view(wire.RPT_VIEW_K)


@pytest.mark.parametrize("integrator", ["restir_gi", "path_tracing"])
def test_other_integrators_ignore_the_view(api, cornell_emissive, integrator):
    integ = api.INTEGRATOR_RESTIR_GI if integrator == "restir_gi" else api.INTEGRATOR_PATH_TRACING
    finals = []
    for view in (wire.RPT_VIEW_NONE, wire.RPT_VIEW_K):
        r = api.Renderer(cornell_emissive, VC.W, VC.H, params=wire.default_params(), integrator=integ)
        r.p_indirect.set_rpt_debug_view(view)      # stored, never read
        for f in range(1, 4):
            r.render_frame(scene_io.make_frame_constants(VC.W, VC.H, frame_num=f, num_emissives=len(cornell_emissive.emissives)))
        finals.append(r.final())
    assert finals[0][..., :3].max() > 0 and _same(finals[0], finals[1])


def test_view_on_a_two_tile_split(api, cornell_emissive):
    """two tiles of one frame sequence on one device, halos through zr_pass_halo_pack / unpack (as test_restir_pt_tile_split_with_halo_exchange_on_gpu):
    the stitched view equals the single-pass view"""
    from zetaray_amd import tiling
    w, h, world, view = 200, 120, 2, wire.RPT_VIEW_K
    prm = wire.default_params()
    ranks = [tiling.TiledRestirPT(cornell_emissive, w, h, world, r, params=prm) for r in range(world)]
    single = api.Renderer(cornell_emissive, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    single.p_indirect.set_rpt_debug_view(view)
    for r in ranks:
        r.hp.set_rpt_debug_view(view)
    prev = None
    for f in range(1, 5):
        cb = scene_io.make_frame_constants(w, h, frame_num=f, num_emissives=len(cornell_emissive.emissives), cam_pos=(0.05 * f, 1.2, -4.043 + 0.02 * f))
        if prev is not None:
            cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
        prev = cb.copy()
        for r in ranks:
            r.stage_temporal(cb)
        tiling.exchange_in_process(ranks, api.HALO_POST_TEMPORAL)
        for r in ranks:
            r.stage_spatial(cb)
        tiling.exchange_in_process(ranks, api.HALO_FINAL)
        single.render_frame(cb)
        want = single.final()
        img = np.zeros_like(want)
        for r in ranks:
            (x0, y0, tw, th), t = r.final_tile()
            img[y0:y0 + th, x0:x0 + tw] = t
        mism = int((img[..., :3].view(np.uint32) != want[..., :3].view(np.uint32)).any(axis=2).sum())
        assert mism == 0, f"frame {f}: {mism} pixels of the stitched view differ from the single-pass view"
    colours = [c for c in VC.COLORS["K"].values() if VC.has_color(want, c)]
    assert colours and VC.has_color(want, VC.BLACK)      # a view was drawn


@pytest.mark.parametrize("case", ["stc_cornell_moving", "ttc_no_spatial_moving"])
def test_view_with_frame_overlap(api, gold, case):
    """zr_pass_set_frame_overlap on: the view equals the plain order's, i.e. the reference's"""
    view = wire.RPT_VIEW_LOBE_K_MIN_1
    got, counters = _run(api, case, view, overlap=True)
    for f in VC.recorded(case):
        assert _same(got[f][0], gold[VC.key(case, view, f)]), f"frame {f}: FINAL with frame overlap differs from the reference shaders' view"
    assert counters == _plain(api, case)[1]


def test_cpp_mirror_set_debug_view(api, gold):
    """IndirectLighting::SetDebugView on the C++ mirror (the reference's DebugViewCallback) draws what the setter draws"""
    case, view = "stc_cornell_moving", wire.RPT_VIEW_CASE
    sc, _, _ = VC.scene_and_params(case)      # (the case runs the pass's default parameters)
    api.lib()
    L = C.CDLL(os.path.join(ROOT, "zetaray_amd", "libzetaray_host.so"))
    L.zrh_render_sequence_debug_view.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    cbs = np.ascontiguousarray(np.stack([cb for _, cb in VC.frames_of(case)]))
    desc = sc.desc()
    out = np.zeros((VC.H, VC.W, 4), np.float32)
    assert L.zrh_render_sequence_debug_view(C.addressof(desc), cbs.ctypes.data, len(cbs), VC.W, VC.H, 2, view, out.ctypes.data) == 0
    assert _same(out[..., :3], gold[VC.key(case, view, VC.num_frames(case))])
