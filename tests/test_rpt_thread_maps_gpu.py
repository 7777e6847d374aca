"""The K12 thread maps of the ReSTIR PT pass as OUTPUTS (zr_pass_get_output(ZR_OUT_RPT_THREAD_MAP_CTN / _NTC)), and the temporal replay work lists.

A stage launches the sort whose map one of its kernels reads (Sort_CtT, Sort_StC) and puts the other one off until somebody asks for its map (Sort_TtC,
Sort_CtS: zr_api.hip RptPendingSort); the temporal stage's classification into the replay work lists runs in the blocks behind its sort tiles.  None of
that may show: the maps hold what they have always held at every point a caller can ask -- after a whole frame (CtS / StC), after the temporal stage alone
(CtT / TtC), after each spatial round, with spatial reuse or a sort flag off, with frame overlap on and the next frame's candidates already enqueued --
and a frame computes the same whether or not anybody ever asks.

Every expectation comes from the host executor (tests/hostexec: the stage functions of zr_rpt.h run serially, which tests/test_rpt_cpu.py holds to the
oracle), stage by stage, computed once per configuration.  Three frames each, the camera moving from the second, so that temporal and spatial reuse are
live and the reprojection of Sort_TtC is not the identity.  96 x 80: three tile columns, partial 32 x 32 tiles on the right and bottom edges."""
import numpy as np
import pytest

from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu

W, H, FRAMES = 96, 80, 3
MAPS = ("map_ctn", "map_ntc")
RES = ("A", "B", "C", "D", "E", "F", "G")
RBUF = tuple(f"{s}_{c}" for s in ("ctn", "ntc") for c in "ABCD")

# name -> (flags cleared, num_spatial_passes)
CONFIGS = {
    "default": (0, 1),
    "no_spatial": (wire.IND_SPATIAL_RESAMPLE, 1),
    "zero_rounds": (0, 0),
    "two_rounds": (0, 2),
    "no_sort_spatial": (wire.IND_SORT_SPATIAL, 1),
    "no_sort_temporal": (wire.IND_SORT_TEMPORAL, 1),
    "no_sorts": (wire.IND_SORT_TEMPORAL | wire.IND_SORT_SPATIAL, 1),
}


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


def _params(config):
    off, rounds = CONFIGS[config]
    prm = wire.default_params()
    prm.flags &= ~off
    prm.num_spatial_passes = rounds
    return prm


def _frames(scene, cam0):
    out, prev = [], None
    for f in range(1, FRAMES + 1):
        cb = scene_io.make_frame_constants(W, H, frame_num=f, num_emissives=len(scene.emissives), cam_pos=(cam0[0] + 0.07 * max(0, f - 1), cam0[1], cam0[2]))
        if prev is not None:
            cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
        prev = cb.copy()
        out.append(cb)
    return out


def _maps_of(x):
    return {nm: x.plane(nm).copy() for nm in MAPS}


def _expect(hx, scene, cam0, prm):
    """per frame: the maps after the temporal stage, after the first spatial round and after the frame; FINAL, reservoir planes, r-buffers, neighbour
    plane and ray counters at the end of the frame"""
    from tests.hostexec import zhx
    x = zhx.HostExecRPT(hx, W, H)
    out = []
    for cb in _frames(scene, cam0):
        e = {}
        x.render_stage(cb, prm, 1)
        e["temporal"] = _maps_of(x)
        x.render_stage(cb, prm, 2)
        e["round1"] = _maps_of(x)
        if prm.num_spatial_passes == 2:
            x.render_stage(cb, prm, 4)
        e["frame"] = _maps_of(x)
        e["final"] = x.final.copy()
        e["planes"] = {nm: x.plane(nm).copy() for nm in RES + RBUF + ("neighbor",)}
        e["counters"] = x.counters
        out.append(e)
    return out


@pytest.fixture(scope="module")
def cornell(cornell_emissive, oracle_emissive):
    from tests.hostexec import zhx
    hx = zhx.HostExecScene(cornell_emissive, oracle_emissive.alias)
    cam0 = (0.0, 1.2, -4.043)
    cache = {}

    def expected(config):
        if config not in cache:
            cache[config] = _expect(hx, cornell_emissive, cam0, _params(config))
        return cache[config]
    return cornell_emissive, cam0, expected


@pytest.fixture(scope="module")
def materials():
    """metal, coat, glass: reservoirs that reconnect beyond the first indirect vertex (k > 2), so the replay work lists are not empty"""
    from oracle import zro
    from tests.hostexec import zhx
    sc = scene_io.make_synthetic_scene(num_tris=3000, num_emissive=1500, seed=11)
    o = zro.OracleScene(sc, force_bvh=True)
    hx = zhx.HostExecScene(sc, o.alias)
    cam0 = (0.0, 0.0, -3.5)
    prm = _params("default")
    prm.max_non_tr_bounces, prm.max_glossy_tr_bounces = 6, 8      # (long enough paths for the k >= 5 class)
    return sc, cam0, prm, _expect(hx, sc, cam0, prm)


def _same_maps(p, want, where):
    for nm in MAPS:
        got = p.download_plane(nm)
        bad = int((got != want[nm]).sum())
        print(f"{where}: {nm}: {bad} of {got.size} entries differ")
        assert bad == 0, f"{where}: {nm}: {bad} entries differ"


def _same_state(r, e, where, planes=RES + RBUF + ("neighbor",)):
    got = r.final()
    bad = int((got.view(np.uint32) != e["final"].view(np.uint32)).any(axis=2).sum())
    print(f"{where}: FINAL: {bad} pixels differ")
    assert bad == 0, f"{where}: FINAL: {bad} pixels differ"
    for nm in planes:
        a, b = r.p_indirect.download_plane(nm), e["planes"][nm]
        if nm == "A":      # RGBA8: the w channel is never written
            a, b = a & 0xffffff, b & 0xffffff
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{where}: plane {nm} differs"


def _renderer(api, scene, config):
    return api.Renderer(scene, W, H, params=_params(config), integrator=api.INTEGRATOR_RESTIR_PT)


def _staged_frame(api, r, cb, first, stages):
    """a frame through zr_pass_render_stage: the G-buffer (and, once, the alias table) first, then `stages` one call each; yields after every stage"""
    r.p_gbuffer.render(cb, r.scene, r.gbuffer)
    if first:
        r.p_prelight.render(cb, r.scene)
    for st in stages:
        r.p_indirect.render_stage(cb, r.scene, r.gbuffer, st)
        yield st


@pytest.mark.parametrize("config", ["default", "no_spatial", "zero_rounds", "two_rounds", "no_sort_spatial", "no_sort_temporal", "no_sorts"])
def test_maps_after_every_frame(api, cornell, config):
    """cases 1 and 4: both maps after every frame -- CtS / StC where the frame sorted spatially, else what the temporal stage left (CtT / TtC)"""
    scene, cam0, expected = cornell
    want = expected(config)
    r = _renderer(api, scene, config)
    for f, cb in enumerate(_frames(scene, cam0)):
        r.p_indirect.read_counters(reset=True)
        r.render_frame(cb)
        _same_maps(r.p_indirect, want[f]["frame"], f"{config}, frame {f + 1}")
        assert r.p_indirect.read_counters() == want[f]["counters"], f"{config}, frame {f + 1}: ray counters"
    _same_state(r, want[-1], f"{config}, frame {FRAMES}")
    if config == "default":
        m = want[-1]["frame"]
        assert all(int(((m[nm] & 0x7fff) != (31 | (31 << 7))).sum()) > 500 for nm in MAPS), "the sorts permuted nothing: the test compares identity maps"
        assert (want[-1]["temporal"]["map_ntc"] != m["map_ntc"]).any() and (want[-1]["temporal"]["map_ctn"] != m["map_ctn"]).any()


@pytest.mark.parametrize("config", ["default", "no_spatial", "two_rounds", "no_sort_spatial"])
def test_maps_after_the_last_frame_only(api, cornell, config):
    """case 2: nobody asks before frame 3 has been rendered"""
    scene, cam0, expected = cornell
    want = expected(config)
    r = _renderer(api, scene, config)
    for cb in _frames(scene, cam0):
        r.render_frame(cb)
    _same_maps(r.p_indirect, want[-1]["frame"], f"{config}, frame {FRAMES}")
    _same_state(r, want[-1], f"{config}, frame {FRAMES}")


@pytest.mark.parametrize("config", ["default", "two_rounds", "no_sort_spatial", "no_sort_temporal"])
def test_maps_between_the_stages(api, cornell, config):
    """case 3: CANDIDATES, TEMPORAL_REUSE, fetch (CtT / TtC), SPATIAL, fetch (CtS / StC of the first round) [, SPATIAL2, fetch]"""
    scene, cam0, expected = cornell
    want = expected(config)
    r = _renderer(api, scene, config)
    rounds = CONFIGS[config][1]
    stages = [api.STAGE_CANDIDATES, api.STAGE_TEMPORAL_REUSE, api.STAGE_SPATIAL] + ([api.STAGE_SPATIAL2] if rounds == 2 else [])
    for f, cb in enumerate(_frames(scene, cam0)):
        for st in _staged_frame(api, r, cb, f == 0, stages):
            where = f"{config}, frame {f + 1}, after stage {st}"
            if st == api.STAGE_TEMPORAL_REUSE:
                _same_maps(r.p_indirect, want[f]["temporal"], where)
            elif st == api.STAGE_SPATIAL:
                _same_maps(r.p_indirect, want[f]["round1"], where)
            elif st == api.STAGE_SPATIAL2:
                _same_maps(r.p_indirect, want[f]["frame"], where)
    _same_state(r, want[-1], f"{config}, frame {FRAMES}")


def test_temporal_maps_asked_for_late(api, cornell):
    """case 3, the other order of asking: the temporal stage's maps are first asked for only after the NEXT stage has been enqueued where that stage leaves
    them alone (SORT_SPATIAL off: the spatial round overwrites the reservoir set Sort_TtC reads, the map must have been built before), and one map is
    asked for without the other"""
    scene, cam0, expected = cornell
    want = expected("no_sort_spatial")
    r = _renderer(api, scene, "no_sort_spatial")
    for f, cb in enumerate(_frames(scene, cam0)):
        for st in _staged_frame(api, r, cb, f == 0, [api.STAGE_TEMPORAL, api.STAGE_SPATIAL]):
            pass
        got = r.p_indirect.download_plane("map_ntc")
        assert np.array_equal(got, want[f]["frame"]["map_ntc"]), f"frame {f + 1}: map_ntc after the spatial round"
    _same_maps(r.p_indirect, want[-1]["frame"], f"frame {FRAMES}")
    _same_state(r, want[-1], f"frame {FRAMES}")


@pytest.mark.parametrize("carry", [True, False])
def test_maps_with_frame_overlap(api, cornell, carry):
    """case 5: frame overlap on; the maps of frame N are asked for while the candidates of frame N + 1 are already enqueued on the other stream"""
    scene, cam0, expected = cornell
    want = expected("default")
    r = _renderer(api, scene, "default")
    r.enable_frame_overlap(True, carry=carry)
    a = r.p_indirect.frame_overlap_stream()
    reuse = api.STAGE_TEMPORAL_REUSE | api.STAGE_SPATIAL | api.STAGE_SPATIAL2
    cbs = _frames(scene, cam0)
    r.render_frame(cbs[0])
    for f in (1, 2):
        r.p_gbuffer.render(cbs[f], r.scene, r.gbuffer, a)
        r.p_indirect.render_stage(cbs[f], r.scene, r.gbuffer, api.STAGE_CANDIDATES, a)
        _same_maps(r.p_indirect, want[f - 1]["frame"], f"frame {f} with the candidates of frame {f + 1} enqueued")
        r.p_indirect.render_stage(cbs[f], r.scene, r.gbuffer, reuse)
    _same_maps(r.p_indirect, want[-1]["frame"], f"frame {FRAMES}")
    # (without carry the bytes a reservoir record does not use are the rotation's: FINAL alone; tests/test_gpu_parity.py compares the used bytes)
    _same_state(r, want[-1], f"frame {FRAMES}", planes=RES + RBUF + ("neighbor",) if carry else ())


def test_replay_lists_are_complete(api, materials):
    """case 6.  The work lists have no getter; what depends on their being complete has: a pixel missing from a temporal list keeps a stale r-buffer record,
    and the reconnect pass behind it shifts a different path -- so both r-buffers, all reservoir planes, FINAL and the ray counters (a replay traces rays)
    of every frame equal the host executor's, which replays every pixel.  The scene's reservoirs must reach every replay class (k = 3, 4, >= 5)."""
    scene, cam0, prm, want = materials
    r = api.Renderer(scene, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    classes = set()
    for f, cb in enumerate(_frames(scene, cam0)):
        r.p_indirect.read_counters(reset=True)
        r.render_frame(cb)
        where = f"materials, frame {f + 1}"
        assert r.p_indirect.read_counters() == want[f]["counters"], f"{where}: ray counters"
        _same_state(r, want[f], where)
        _same_maps(r.p_indirect, want[f]["frame"], where)
        k = want[f]["planes"]["A"][..., 0] & 0xf
        classes |= {min(int(v), 3) for v in np.unique(k) if v != 15 and v != 0}
    assert classes == {1, 2, 3}, f"replay classes reached: {classes}"
    assert any(want[-1]["planes"][nm].any() for nm in RBUF), "no replay wrote an r-buffer"


@pytest.mark.parametrize("ask", [False, True])
def test_frames_do_not_depend_on_the_maps_being_asked_for(api, cornell, ask):
    """case 7: FINAL, the seven reservoir planes and the ray counters of frame 3, with the maps asked for after every stage of every frame and with no map
    ever asked for"""
    scene, cam0, expected = cornell
    want = expected("default")
    r = _renderer(api, scene, "default")
    for f, cb in enumerate(_frames(scene, cam0)):
        r.p_indirect.read_counters(reset=True)
        for st in _staged_frame(api, r, cb, f == 0, [api.STAGE_CANDIDATES, api.STAGE_TEMPORAL_REUSE, api.STAGE_SPATIAL]):
            if ask:
                for nm in MAPS:
                    r.p_indirect.download_plane(nm)
        assert r.p_indirect.read_counters() == want[f]["counters"], f"frame {f + 1}: ray counters"
    _same_state(r, want[-1], f"frame {FRAMES}, maps {'asked for' if ask else 'never asked for'}", planes=RES)
