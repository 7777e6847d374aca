"""zr_scene_set_morph: morph targets weighted and applied on the device by every zr_scene_animate (zr_tu_pose.hip), against the host form --
zrh_scene_data_animate, zr_scene_update_vertices with the vertices include/zr_morph.h (then include/zr_skin.h, where the range is skinned) computes on the
host, then the host-form emissive and instance updates -- bit for bit: the vertex buffer, both instance buffers, toWorld, the emissive records, rendered
frames (through which the hit tables and the refit tree are held), a fresh scene made from the posed vertices, two streams, the picked-instance mask,
clearing, and the calls refused.  No tolerance anywhere."""
import numpy as np
import pytest

from tests.animmath import cases as acases
from tests.morphmath import cases
from tests.skinmath import cases as scases
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
RPT_PLANES = ("A", "B", "C", "D", "E", "F", "G", "neighbor", "map_ctn", "map_ntc")
W, H = 96, 64
TIMES = acases.TIMES
TV = scases.TUBE_VERTS


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


@pytest.fixture(scope="module")
def world():
    """the Cornell box + two tubes; tube k's vertices start at firsts[k]"""
    return scases.skinned_cornell(1)


@pytest.fixture(scope="module")
def plain_anim():
    """an animation that moves no instance: a morph set needs one to be set (zr_scene_animate owns the frame's time)"""
    return scases.joint_chain(2)[0]


def _skin(sc, aj, ranges, seed=1):
    anim, joints = aj
    rng = np.random.default_rng(seed)
    infl, rr, k = [], [], 0
    for first, count in ranges:
        infl.append(scases.tube_influences(sc.vertices[first:first + count], len(joints), rng))
        rr.append((first, count, k))
        k += count
    return wire.SkinDesc(joints, np.array(rr, wire.SKIN_RANGE), np.concatenate(infl))


def _assert_scene_bytes(B, A, host, what):
    va, vb = A.download_vertices(), B.download_vertices()
    assert vb.tobytes() == va.tobytes(), f"{what}: {int((vb != va).sum())} vertices differ from the host form's"
    for which in (0, 1):
        ib, xb = B.download_instances(which)
        ia, xa = A.download_instances(which)
        assert ib.tobytes() == ia.tobytes(), f"{what}: instance buffer {which}"
        assert xb.tobytes() == xa.tobytes(), f"{what}: toWorld"
    assert B.download_instances(0)[0].tobytes() == host.inst.tobytes()
    assert B.download_emissives().tobytes() == A.download_emissives().tobytes() == host.ems.tobytes(), f"{what}: emissive records"


def _run_twins(api, sc, anim, skin, morph, what, times=TIMES, expect_motion=True):
    """A takes the host sequence, B set_morph + animate: every device byte equal at every time; vertices outside the ranges never change"""
    host = acases.HostData.from_scene(sc)
    assert host.set_animation(anim) == 0
    A, B = api.Scene(sc), api.Scene(sc)
    B.set_animation(anim)
    if skin is not None:
        B.set_skinning(skin)
    B.set_morph(morph)
    assert B.has_morph() and not A.has_morph()
    untouched = np.ones(len(sc.vertices), bool)
    for d in (morph, skin):
        for r in (d.ranges if d is not None else ()):
            untouched[int(r["first_vertex"]):int(r["first_vertex"]) + int(r["num_vertices"])] = False
    seen = set()
    for t in times:
        posed = cases.apply_host_form(A, host, anim, skin, morph, sc.vertices, t)
        B.animate(t)
        _assert_scene_bytes(B, A, host, f"{what}, t = {t}")
        got = B.download_vertices()
        assert got[untouched].tobytes() == sc.vertices[untouched].tobytes(), f"{what}: a vertex outside the ranges changed"
        seen.add(posed.tobytes())
    if expect_motion:
        assert len(seen) >= 3 and posed["pos"].tobytes() != cases.rest_of_ranges(morph, sc.vertices)["pos"].tobytes()
    A.close(); B.close(); host.close()


# ---------------------------------------------------------------------------------------------------------------- ranges, targets, weights, tracks
@pytest.mark.parametrize("count,offset", [(1, 0), (63, 1), (65, 2), (255, 3), (256, 0), (257, 1), (1025, 2), (1025, 3)])
def test_range_sizes_and_first_vertices(api, world, plain_anim, count, offset):
    """twin scenes at the six times of tests/animmath/cases.py; 1 / 63 / 65 / 255 / 256 / 257 / 1 025 morphed vertices: lanes end inside a wave, at a wave boundary,
    at a block's boundary and across blocks.  The range starts at vertex 130 + offset, even and odd: the 28-byte records start 8, 4, 0 and 12 bytes behind a
    16-byte boundary, the 12-byte delta triples of the second and later arrays at whatever place the arrays before them leave"""
    sc, firsts = world
    rng = np.random.default_rng(count)
    morph = cases.morph_set([(firsts[0] + offset, count, 0)], [cases.keyed_track(rng, 2, loop=offset % 2)], lacks=[0, 0], seed=count + offset)
    _run_twins(api, sc, plain_anim, None, morph, f"{count} vertices from {firsts[0] + offset}")


@pytest.mark.parametrize("T", [1, 2, 5, 9])
def test_target_counts(api, world, plain_anim, T):
    """1, 2, 5 and 9 targets over 257 vertices; from the second on the targets lack NORMAL, TANGENT, both, nothing, ... in turn"""
    sc, firsts = world
    morph = cases.morph_set([(firsts[0] + 3, 257, 0)], [cases.keyed_track(np.random.default_rng(T), T, loop=1)], lacks=[0, 1, 2, 3], seed=T)
    _run_twins(api, sc, plain_anim, None, morph, f"{T} targets")


@pytest.mark.parametrize("lack", [cases.LACK_NRM, cases.LACK_TAN, cases.LACK_BOTH])
def test_targets_lacking_attributes(api, world, plain_anim, lack):
    """every target of the range lacks NORMAL / TANGENT / both: those code words stay the rest pose's at every time, in the vertex buffer and (through the
    twin's table fill) in the hit tables"""
    sc, firsts = world
    first, n = firsts[1] + 1, 300
    morph = cases.morph_set([(first, n, 0)], [cases.keyed_track(np.random.default_rng(lack), 2)], lacks=[lack], seed=lack)
    _run_twins(api, sc, plain_anim, None, morph, f"lack {lack}")
    S = api.Scene(sc)
    S.set_animation(plain_anim)
    S.set_morph(morph)
    S.animate(0.8125)
    got = S.download_vertices(first, n)
    rest = sc.vertices[first:first + n]
    assert (got["pos"] != rest["pos"]).any()
    assert (got["normal"].tobytes() == rest["normal"].tobytes()) == (lack in (cases.LACK_NRM, cases.LACK_BOTH))
    assert (got["tangent"].tobytes() == rest["tangent"].tobytes()) == (lack in (cases.LACK_TAN, cases.LACK_BOTH))
    S.close()


def test_zero_weights_at_some_times_and_all_zeros_at_one(api, world, plain_anim):
    """a track (not looping) whose key 1 (t = 0.5, one of the times) has an exact zero for target 0, and whose last key (1.25) is all zeros: from t = 1.25 on
    every target is skipped and the device's records are the rest bytes"""
    sc, firsts = world
    first, n = firsts[0] + 5, 513
    morph = cases.morph_set([(first, n, 0)], [cases.keyed_track(np.random.default_rng(3), 3, zero_at=[(1, 0)], all_zero_key=2)], lacks=[0, 1, 2])
    _run_twins(api, sc, plain_anim, None, morph, "zero weights", expect_motion=False)
    S = api.Scene(sc)
    S.set_animation(plain_anim)
    S.set_morph(morph)
    S.animate(0.5)
    assert S.download_vertices(first, n)["pos"].tobytes() != sc.vertices[first:first + n]["pos"].tobytes()
    for t in (1.25, 3.7):
        S.animate(t)
        assert S.download_vertices().tobytes() == sc.vertices.tobytes()
    S.close()


def test_shared_tracks_two_tracks_and_a_static_track(api, world, plain_anim):
    """two ranges under one track (a node's primitives share the node's weights) with targets of their own; two tracks with 3 and 5 keys, one looping with
    t0 != 0; a track with num_keys == 0, whose rest weights pose its range once and for all"""
    sc, firsts = world
    rng = np.random.default_rng(8)
    tracks = [cases.keyed_track(rng, 3), cases.keyed_track(rng, 2, times=(0.1, 0.4, 0.9, 1.6, 2.0), loop=1, t0=0.25), cases.static_track([0.75, -0.25, 0.0, 1.0])]
    morph = cases.morph_set([(firsts[0], 200, 0), (firsts[0] + 333, 129, 0), (firsts[1] + 1, 640, 1), (firsts[0] + 600, 65, 2)], tracks, lacks=[0, 2, 1])
    _run_twins(api, sc, plain_anim, None, morph, "tracks")
    S = api.Scene(sc)
    S.set_animation(plain_anim)
    S.set_morph(morph)
    S.animate(0.0)
    a = S.download_vertices(firsts[0] + 600, 65)
    S.animate(2.5)
    assert S.download_vertices(firsts[0] + 600, 65).tobytes() == a.tobytes() != sc.vertices[firsts[0] + 600:firsts[0] + 665].tobytes()
    S.close()


# ---------------------------------------------------------------------------------------------------------------- with skinning
@pytest.mark.parametrize("nj", [64, 65])
def test_morphed_and_skinned_tube(api, world, nj):
    """257 vertices of the tube morphed (3 targets) AND skinned over 64 / 65 joints: one range listed in both tables, posed once by the fused kernel"""
    sc, firsts = world
    aj = scases.joint_chain(nj)
    skin = _skin(sc, aj, [(firsts[0] + 1, 257)])
    morph = cases.morph_set([(firsts[0] + 1, 257, 0)], [cases.keyed_track(np.random.default_rng(nj), 3, loop=1)], lacks=[0, 1, 2], seed=nj)
    _run_twins(api, sc, aj[0], skin, morph, f"morph + skin, {nj} joints")


def test_a_morph_only_a_skin_only_and_a_range_with_both(api, world):
    """one scene, three ranges: morphed only (tube 1), skinned only and morphed + skinned (tube 0) -- what catches a range posed twice, by the wrong kernel
    or from the wrong rest records (the two sets keep theirs in buffers of their own, the skin set's ranges in another order than the morph set's)"""
    sc, firsts = world
    aj = scases.joint_chain(6)
    skin = _skin(sc, aj, [(firsts[0] + 2, 401), (firsts[0] + 500, 333)])      # skin-only first, then the range with both
    rng = np.random.default_rng(21)
    morph = cases.morph_set([(firsts[0] + 500, 333, 1), (firsts[1] + 7, 290, 0)], [cases.keyed_track(rng, 2), cases.keyed_track(rng, 4, loop=1, zero_at=[(1, 2)])], lacks=[0, 1, 0, 3])
    _run_twins(api, sc, aj[0], skin, morph, "three kinds of range")


# ---------------------------------------------------------------------------------------------------------------- rendered frames
def _cb(sc, f, prev):
    cb = scene_io.make_frame_constants(W, H, frame_num=f, num_emissives=len(sc.emissives))
    if prev is not None:
        cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
    return cb


def _everything(r, di):
    out = {"final": r.final().copy(), "di": di.download().copy(), "counters": r.p_indirect.read_counters()}
    for nm, pl in zip(wire.GB_PLANE_NAMES, r.gbuffer.download()[0]):
        out["gb_" + nm] = np.asarray(pl).copy()
    for nm in RPT_PLANES:
        a = r.p_indirect.download_plane(nm)
        out["rpt_" + nm] = (a & 0xffffff) if nm == "A" else a
    return out


FRAME_TIMES = {2: 0.2, 3: 0.45, 4: 0.7, 5: 1.1}      # frame 1 is rendered at rest


def _moving_setup(sc, firsts):
    """tube 0 morphed and skinned over 6 joints, tube 1 morphed only, and the short box (instance 8) translating as an animated instance of its own"""
    M = sc.instance_to_world[8].reshape(3, 4).astype(np.float64)
    s = float(np.linalg.norm(M[:, 0]))
    ang = float(np.arctan2(M[0, 2], M[0, 0]))
    aj = scases.joint_chain(6, moving_instances=[(8, (np.float32([s] * 3), scases.quat([0, 1, 0], ang), M[:, 3].astype(np.float32)))])
    skin = _skin(sc, aj, [(firsts[0], TV)])
    rng = np.random.default_rng(31)
    morph = cases.morph_set([(firsts[0], TV, 0), (firsts[1], TV, 1)], [cases.keyed_track(rng, 3, loop=1), cases.keyed_track(rng, 5, zero_at=[(1, 1)])], lacks=[0, 1, 2, 0, 3])
    return aj[0], skin, morph


def _frames_twin(api, sc, anim, skin, morph, host, offs=None):
    prm = wire.default_params()
    ra = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    rb = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    da, db = ra.enable_direct(wire.default_params_di()), rb.enable_direct(wire.default_params_di())
    rb.scene.set_object_emissives(host.init)
    rb.set_animation(anim)
    rb.set_skinning(skin)
    rb.set_morph(morph)
    prev, frames = None, []
    for f in range(1, 6):
        if f in FRAME_TIMES:
            cases.apply_host_form(ra.scene, host, anim, skin, morph, sc.vertices, FRAME_TIMES[f])
            rb.animate(FRAME_TIMES[f])
        cb = _cb(sc, f, prev)
        if offs is not None:
            scene_io.set_texture_heap_offsets(cb, offs)
        prev = cb.copy()
        for r in (ra, rb):
            r.p_indirect.read_counters(reset=True)
            r.render_frame(cb)
        want, got = _everything(ra, da), _everything(rb, db)
        for k, v in want.items():
            if k == "counters":
                assert got[k] == v, f"frame {f}: ray counters"
            else:
                assert np.asarray(got[k]).tobytes() == np.asarray(v).tobytes(), f"frame {f}: {k}"
        frames.append(want)
    _assert_scene_bytes(rb.scene, ra.scene, host, "after the frames")
    assert frames[1]["gb_depth"].tobytes() != frames[4]["gb_depth"].tobytes()      # the morphed meshes really moved on screen
    assert float(frames[-1]["final"][..., :3].max()) > 0


def test_rendered_frames_equal_the_host_form(api, world):
    """ReSTIR PT at 96 x 64 with emissive ReSTIR DI attached, frame 1 at rest and four frames at advancing t: G-buffer planes, FINAL, the DI image, every
    reservoir plane and the ray counters equal the host form's -- the hit tables and the refit tree, current and previous, are held through these"""
    sc, firsts = world
    anim, skin, morph = _moving_setup(sc, firsts)
    host = acases.HostData.from_scene(sc)
    assert host.set_animation(anim) == 0
    _frames_twin(api, sc, anim, skin, morph, host)
    host.close()


def test_the_loaded_fixture_renders_as_the_host_form(api, tmp_path):
    """tests/golden/morph_gltf through load_gltf_native -- the light translates, the boxes move, the face morphs under 5 targets (a sparse one among them),
    the tube morphs and bends -- with the loader's own tables (sc.animation, sc.skinning, sc.morph) on both sides: the same frame sequence, the same equalities"""
    path = cases.morphed_gltf(tmp_path)
    sc, offs = scene_io.load_gltf_native(path)
    host = acases.HostData.from_gltf(path)
    _frames_twin(api, sc, sc.animation, sc.skinning, sc.morph, host, offs)
    host.close()


def _gbuffer_and_final(r, cb, stream=None):
    r.render_frame(cb) if stream is None else r.render_frame(cb, stream=stream)
    return [np.asarray(p).copy() for p in r.gbuffer.download()[0]], r.final().copy()


def _fresh(sc, vertices):
    import os
    fresh = scene_io.load_npz(os.path.join(scases.ROOT, "tests", "golden", "cornell_emissive.npz"))
    for name in ("indices", "instances", "instance_to_world", "instance_mask", "instance_num_tris"):
        setattr(fresh, name, getattr(sc, name).copy())
    fresh.vertices = vertices.copy()
    return fresh


def test_one_frame_against_a_fresh_scene(api, world, plain_anim):
    """a morph-only scene -- no instance moves, the moved list is empty -- at two times: after animate(t) the G-buffer and a path-traced frame equal those of a
    scene CREATED from the host-posed vertices (a tree built over the deformed triangles against the refit one; its hit tables filled from the records),
    and the two times' frames differ: the refit read the rewritten vertex buffer although nothing moved"""
    sc, firsts = world
    rng = np.random.default_rng(41)
    morph = cases.morph_set([(firsts[0], TV, 0), (firsts[1] + 40, 1000, 0)], [cases.keyed_track(rng, 4, loop=1)], lacks=[0, 1, 2, 3], seed=5)
    prm = wire.default_params()
    rb = api.Renderer(sc, W, H, params=prm)
    rb.set_animation(plain_anim)
    rb.set_morph(morph)
    cb = scene_io.make_frame_constants(W, H, frame_num=1, num_emissives=len(sc.emissives))
    finals = []
    for t in (0.45, 1.1):
        rb.animate(t)
        assert not rb.scene.instances_in_motion
        want = cases.posed_scene_vertices(plain_anim, None, morph, sc.vertices, t)
        assert rb.scene.download_vertices().tobytes() == want.tobytes()
        rc = api.Renderer(_fresh(sc, want), W, H, params=prm)
        (gb_b, fin_b), (gb_c, fin_c) = _gbuffer_and_final(rb, cb), _gbuffer_and_final(rc, cb)
        for nm, b, c in zip(wire.GB_PLANE_NAMES, gb_b, gb_c):
            assert b.tobytes() == c.tobytes(), f"t = {t}: G-buffer plane {nm} differs from the fresh scene's"
        assert fin_b.tobytes() == fin_c.tobytes(), f"t = {t}: the path-traced frame differs from the fresh scene's"
        finals.append((gb_b[wire.GB_PLANE_NAMES.index("depth")], fin_b))
    assert finals[0][0].tobytes() != finals[1][0].tobytes() and finals[0][1].tobytes() != finals[1][1].tobytes()


def test_animate_on_a_second_stream_while_a_render_is_in_flight(api, world):
    """the frame rendered on one stream, animate enqueued on another with no host wait in between, then the next frame on the first: the morph kernels wait
    for the render that still reads the vertices and the hit tables, and the next render for them -- frames and scene bytes equal the host-form twin's,
    which runs on the null stream with waits"""
    import torch
    sc, firsts = world
    anim, skin, morph = _moving_setup(sc, firsts)
    host = acases.HostData.from_scene(sc)
    assert host.set_animation(anim) == 0
    prm = wire.default_params()
    ra, rb = api.Renderer(sc, W, H, params=prm), api.Renderer(sc, W, H, params=prm)
    rb.scene.set_object_emissives(host.init)
    rb.set_animation(anim)
    rb.set_skinning(skin)
    rb.set_morph(morph)
    s_render, s_update = torch.cuda.Stream(), torch.cuda.Stream()
    cb = scene_io.make_frame_constants(W, H, frame_num=1, num_emissives=len(sc.emissives))
    for t in (0.2, 0.7, 1.1):
        cases.apply_host_form(ra.scene, host, anim, skin, morph, sc.vertices, t)
        gb_a, fin_a = _gbuffer_and_final(ra, cb)
        rb.render_frame(cb, stream=s_render.cuda_stream)      # (a frame of the previous pose, still in flight when the update is enqueued)
        rb.animate(t, stream=s_update.cuda_stream)
        rb.render_frame(cb, stream=s_render.cuda_stream)
        torch.cuda.synchronize()
        gb_b, fin_b = [np.asarray(p).copy() for p in rb.gbuffer.download()[0]], rb.final().copy()
        for nm, a, b in zip(wire.GB_PLANE_NAMES, gb_a, gb_b):
            assert a.tobytes() == b.tobytes(), f"t = {t}: G-buffer plane {nm}"
        assert fin_a.tobytes() == fin_b.tobytes(), f"t = {t}: FINAL"
        _assert_scene_bytes(rb.scene, ra.scene, host, f"two streams, t = {t}")
    host.close()


def test_the_picked_outline_follows_the_morph(api, world, plain_anim):
    """the picked-instance mask (ZR_OUT_PICK_MASK) of the morphed instance after animate: tests/pickcheck.py's restatement fed the host-posed vertices, and
    not the mask of the rest pose"""
    from tests import pickcheck as pk
    from tests.test_pick_outline_gpu import Frame
    sc, firsts = world
    morph = cases.morph_set([(firsts[0], TV, 0)], [cases.keyed_track(np.random.default_rng(2), 2)], seed=6)
    morph.deltas[:TV] *= np.float32(3.0)      # (target 0's POSITION deltas: a silhouette that moves by whole pixels at 96 x 64)
    tube_inst = len(sc.instances) - 2
    fb = Frame(sc, (W, H), (W, H))
    fb.scene.set_animation(plain_anim)
    fb.scene.set_morph(morph)
    fb.pick(48, 40)
    fb.show([tube_inst])
    at_rest = fb.p.download_plane("pick_mask").copy()
    fb.scene.animate(1.1)
    fb.show([tube_inst])
    got = fb.p.download_plane("pick_mask")
    vertices = cases.posed_scene_vertices(plain_anim, None, morph, sc.vertices, 1.1)
    base, ib = int(sc.instances["base_vtx_offset"][tube_inst]), int(sc.instances["base_idx_offset"][tube_inst])
    idx = sc.indices[ib:ib + 3 * int(sc.instance_num_tris[tube_inst])].astype(np.int64) + base
    tris = vertices["pos"][idx].reshape(-1, 3, 3).astype(np.float32)
    want = pk.raster_mask(tris, pk.wvp(sc.instance_to_world[tube_inst], fb.cb["curr_view_proj"]), (W, H), (W, H))
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} mask pixels differ from the restatement's"
    assert want.any() and not np.array_equal(want, at_rest)


# ---------------------------------------------------------------------------------------------------------------- clearing, refusals
def test_clearing_restores_the_rest_bytes(api, world):
    """set_morph(None) puts the rest bytes back (and a later animate leaves them); a replacing set poses its ranges from the REST records and lets the old
    ones go back to rest; set_skinning and set_animation clear the morph set, the skinned range's rest pose coming from the skin set's records"""
    sc, firsts = world
    aj = scases.joint_chain(4)
    anim = aj[0]
    skin = _skin(sc, aj, [(firsts[0] + 1, 500)])
    rng = np.random.default_rng(12)
    morph = cases.morph_set([(firsts[0] + 1, 500, 0), (firsts[1], 300, 0)], [cases.keyed_track(rng, 2)])
    S = api.Scene(sc)
    rest = sc.vertices.tobytes()
    assert not S.has_morph()
    S.set_animation(anim)
    S.set_skinning(skin)
    S.set_morph(morph)
    assert S.has_morph() and S.has_skinning()
    S.animate(0.8)
    assert S.download_vertices().tobytes() == cases.posed_scene_vertices(anim, skin, morph, sc.vertices, 0.8).tobytes() != rest
    S.set_morph(None)
    assert not S.has_morph() and S.has_skinning() and S.download_vertices().tobytes() == rest
    S.animate(0.8)      # the skin alone poses its range again
    want = sc.vertices.copy()
    want[firsts[0] + 1:firsts[0] + 501] = scases.host_posed(anim, skin, scases.rest_of_ranges(skin, sc.vertices), 0.8)
    assert S.download_vertices().tobytes() == want.tobytes()
    S.set_morph(morph)
    S.animate(0.5)
    other = cases.morph_set([(firsts[1] + 100, 400, 0)], [cases.keyed_track(rng, 3, loop=1)], seed=13)      # meets the old set's second range, posed at the call
    S.set_morph(other)
    assert S.has_morph()
    S.animate(0.5)
    want = sc.vertices.copy()
    want[firsts[0] + 1:firsts[0] + 501] = scases.host_posed(anim, skin, scases.rest_of_ranges(skin, sc.vertices), 0.5)
    want[firsts[1] + 100:firsts[1] + 500] = cases.host_posed(anim, skin, other, cases.rest_of_ranges(other, sc.vertices), 0.5)
    assert S.download_vertices().tobytes() == want.tobytes()
    S.set_morph(morph)
    S.animate(1.1)
    S.set_skinning(skin)      # a new skin set: the morph set laid out against the old one goes
    assert not S.has_morph() and S.has_skinning() and S.download_vertices().tobytes() == rest
    S.set_morph(morph)
    S.animate(1.1)
    assert S.download_vertices().tobytes() != rest
    S.set_skinning(None)
    assert not S.has_morph() and not S.has_skinning() and S.download_vertices().tobytes() == rest
    S.set_morph(morph)      # without a skin set both ranges are morph-only
    S.animate(1.1)
    assert S.download_vertices().tobytes() == cases.posed_scene_vertices(anim, None, morph, sc.vertices, 1.1).tobytes()
    S.set_animation(anim)      # a new animation: the morph set goes, the rest pose comes back
    assert not S.has_morph() and S.download_vertices().tobytes() == rest
    S.animate(0.8)
    assert S.download_vertices().tobytes() == rest
    S.set_morph(morph)
    S.animate(0.8)
    S.set_animation(None)
    assert not S.has_morph() and S.download_vertices().tobytes() == rest
    S.close()


def _skin_only(anim, skin, vertices, t):
    """the whole vertex array of the host form at time t with the skin set alone"""
    out = vertices.copy()
    sk = scases.host_posed(anim, skin, scases.rest_of_ranges(skin, vertices), t)
    k = 0
    for r in skin.ranges:
        f, n = int(r["first_vertex"]), int(r["num_vertices"])
        out[f:f + n] = sk[k:k + n]
        k += n
    return out


def test_the_skin_only_ranges_follow_the_morph_set(api, world):
    """a skin set with two ranges R0, R1; morph set A lists R0, then B lists R1 and not R0 (R0 is skin-only again, R1 fused), then no morph set (both skin-only):
    every animate equals the host form.  A replaced or cleared morph set puts ITS ranges back to rest at the call; a skin-only range keeps its last pose until
    the next animate.  set_skinning(None) leaves the rest bytes"""
    sc, firsts = world
    aj = scases.joint_chain(4)
    anim = aj[0]
    R0, R1 = (firsts[0] + 1, 201), (firsts[0] + 300, 130)
    skin = _skin(sc, aj, [R0, R1])
    rng = np.random.default_rng(51)
    A = cases.morph_set([R0 + (0,)], [cases.keyed_track(rng, 2)], seed=52)
    B = cases.morph_set([R1 + (0,)], [cases.keyed_track(rng, 2, loop=1)], seed=53)
    rest = sc.vertices
    S = api.Scene(sc)
    S.set_animation(anim)
    S.set_skinning(skin)
    S.set_morph(A)
    S.animate(0.5)
    at_a = cases.posed_scene_vertices(anim, skin, A, rest, 0.5)
    assert S.download_vertices().tobytes() == at_a.tobytes() != rest.tobytes()
    S.set_morph(B)
    want = at_a.copy()
    want[R0[0]:R0[0] + R0[1]] = rest[R0[0]:R0[0] + R0[1]]      # A's range is at rest; R1, skin-only under A, still holds the pose of t = 0.5
    assert S.download_vertices().tobytes() == want.tobytes()
    S.animate(0.8)
    at_b = cases.posed_scene_vertices(anim, skin, B, rest, 0.8)
    assert S.download_vertices().tobytes() == at_b.tobytes() != at_a.tobytes()
    S.set_morph(None)
    want = at_b.copy()
    want[R1[0]:R1[0] + R1[1]] = rest[R1[0]:R1[0] + R1[1]]
    assert S.has_skinning() and not S.has_morph() and S.download_vertices().tobytes() == want.tobytes()
    S.animate(1.1)
    assert S.download_vertices().tobytes() == _skin_only(anim, skin, rest, 1.1).tobytes() != rest.tobytes()
    S.set_skinning(None)
    assert not S.has_skinning() and S.download_vertices().tobytes() == rest.tobytes()
    S.close()


def test_a_new_skin_set_over_a_morphed_only_range(api, world):
    """no skin set, [f, f + 300) morphed and animated; set_skinning with [f + 100, f + 400), which partly covers it: the morph set goes, the vertices are the
    rest bytes right after the call, and animate poses the skin range from the REST records -- not from the morphed bytes the buffer held at the call"""
    sc, firsts = world
    aj = scases.joint_chain(4)
    anim = aj[0]
    f = firsts[1] + 3
    morph = cases.morph_set([(f, 300, 0)], [cases.keyed_track(np.random.default_rng(54), 2)], seed=55)
    skin = _skin(sc, aj, [(f + 100, 300)])
    rest = sc.vertices
    S = api.Scene(sc)
    S.set_animation(anim)
    S.set_morph(morph)
    S.animate(0.8)
    assert S.download_vertices().tobytes() == cases.posed_scene_vertices(anim, None, morph, rest, 0.8).tobytes() != rest.tobytes()
    S.set_skinning(skin)
    assert not S.has_morph() and S.has_skinning() and S.download_vertices().tobytes() == rest.tobytes()
    S.animate(0.5)
    assert S.download_vertices().tobytes() == _skin_only(anim, skin, rest, 0.5).tobytes() != rest.tobytes()
    S.set_skinning(None)
    assert S.download_vertices().tobytes() == rest.tobytes()
    S.close()


def test_empty_ranges(api, world):
    """a skin set and morph sets that each list a range of no vertices between two non-empty ones, one empty morph range starting where a skin range starts:
    set, two times, a replacing morph set, clearing -- the host form / the rest bytes at every step"""
    sc, firsts = world
    aj = scases.joint_chain(4)
    anim = aj[0]
    a, c = firsts[0] + 5, firsts[0] + 400
    skin = _skin(sc, aj, [(a, 100), (a + 150, 0), (c, 120)])
    rng = np.random.default_rng(56)
    first = cases.morph_set([(firsts[1] + 3, 150, 0), (a, 0, 0), (firsts[1] + 500, 0, 0), (c, 120, 0)], [cases.keyed_track(rng, 2)], seed=57)
    second = cases.morph_set([(a, 100, 0), (c, 0, 0), (firsts[1] + 100, 200, 0)], [cases.keyed_track(rng, 2, loop=1)], seed=58)
    rest = sc.vertices
    S = api.Scene(sc)
    S.set_animation(anim)
    S.set_skinning(skin)
    S.set_morph(first)
    for t in (0.5, 1.1):
        S.animate(t)
        assert S.download_vertices().tobytes() == cases.posed_scene_vertices(anim, skin, first, rest, t).tobytes() != rest.tobytes()
    S.set_morph(second)
    for t in (0.2, 0.8):
        S.animate(t)
        assert S.download_vertices().tobytes() == cases.posed_scene_vertices(anim, skin, second, rest, t).tobytes()
    S.set_morph(None)
    S.animate(0.8)
    assert S.download_vertices().tobytes() == _skin_only(anim, skin, rest, 0.8).tobytes() != rest.tobytes()
    S.set_morph(first)
    S.animate(0.5)
    S.set_skinning(None)
    assert not S.has_morph() and not S.has_skinning() and S.download_vertices().tobytes() == rest.tobytes()
    S.close()


def test_update_vertices_inside_a_posed_range(api, world):
    """16 arbitrary records written by hand into a morphed and skinned range: the next animate overwrites them from the rest records captured when the sets
    were laid out, and clearing puts THOSE back, not the records written by hand"""
    sc, firsts = world
    aj = scases.joint_chain(4)
    anim = aj[0]
    first, n = firsts[0] + 7, 257
    skin = _skin(sc, aj, [(first, n)])
    morph = cases.morph_set([(first, n, 0)], [cases.keyed_track(np.random.default_rng(59), 2)], seed=60)
    rest = sc.vertices
    S = api.Scene(sc)
    S.set_animation(anim)
    S.set_skinning(skin)
    S.set_morph(morph)
    S.animate(0.5)
    junk = rest[first + 40:first + 56].copy()
    junk["pos"] += np.float32(0.37)
    junk["normal"], junk["tangent"] = junk["tangent"].copy(), junk["normal"].copy()
    S.update_vertices(first + 100, junk)
    got = S.download_vertices()
    assert got[first + 100:first + 116].tobytes() == junk.tobytes()
    S.animate(0.8)
    assert S.download_vertices().tobytes() == cases.posed_scene_vertices(anim, skin, morph, rest, 0.8).tobytes()
    S.update_vertices(first + 100, junk)
    S.set_skinning(None)
    assert not S.has_morph() and not S.has_skinning() and S.download_vertices().tobytes() == rest.tobytes()
    S.close()


def test_refusals_change_nothing(api, world):
    """every refusal of zr_scene_set_morph with download_vertices() -- and the instance and light records -- unchanged, the set in place still the one that
    runs; without an animation the call is refused as not initialised"""
    sc, firsts = world
    aj = scases.joint_chain(4)
    anim = aj[0]
    skin = _skin(sc, aj, [(firsts[0] + 1, 500)])
    rng = np.random.default_rng(14)
    good = cases.morph_set([(firsts[0] + 1, 500, 0), (firsts[1], 300, 1)], [cases.keyed_track(rng, 3), cases.keyed_track(rng, 2)], lacks=[0, 1, 2])
    nv = len(sc.vertices)
    S = api.Scene(sc)

    def state():
        return S.download_vertices().tobytes() + S.download_instances(0)[0].tobytes() + S.download_emissives().tobytes()

    s0 = state()
    with pytest.raises(api.ZetaRayError) as e:
        S.set_morph(good)
    assert e.value.code == 6 and "zr_scene_set_animation" in str(e.value) and state() == s0 and not S.has_morph()
    S.set_animation(anim)
    S.set_skinning(skin)
    S.set_morph(good)
    S.animate(0.5)
    s1 = state()
    assert s1 != s0

    def bad(edit):
        parts = {k: getattr(good, k).copy() for k in ("tracks", "targets", "ranges", "times", "values", "rest_weights", "deltas")}
        edit(parts)
        return wire.MorphDesc(**parts)

    def past_scene(p): p["ranges"]["first_vertex"][1] = nv - 299
    def past_deltas(p): p["targets"]["first_pos"][0] = len(good.deltas) - 499
    def past_targets(p): p["ranges"]["first_target"][1] = len(good.targets) - 1
    def overlap(p): p["ranges"]["first_vertex"][1] = firsts[0] + 500
    def meets_skin(p): p["ranges"]["num_vertices"][0] = 499
    def target_count(p): p["ranges"]["num_targets"][1] = 1
    def one_key(p): p["tracks"]["num_keys"][1] = 1
    def time_inf(p): p["times"][1] = np.inf
    def time_order(p): p["times"][4] = p["times"][3]
    def weight_nan(p): p["values"][2] = np.nan
    def t0_inf(p): p["tracks"]["t0"][0] = -np.inf
    def delta_nan(p): p["deltas"][17, 1] = np.nan
    for edit, word in ((past_scene, "the scene has"), (past_deltas, "deltas ["), (past_targets, "targets ["), (overlap, "overlaps an earlier range"),
                       (meets_skin, "meets skin range 0 without being equal"), (target_count, "1 targets, its track 1 has 2"), (one_key, "num_keys == 1"),
                       (time_inf, "time is not finite"), (time_order, "not strictly increasing"), (weight_nan, "a weight is not finite"), (t0_inf, "t0 is not finite"),
                       (delta_nan, "delta 17")):
        with pytest.raises(api.ZetaRayError) as e:
            S.set_morph(bad(edit))
        assert e.value.code == 1 and word in str(e.value), str(e.value)
        assert state() == s1 and S.has_morph()
    static = cases.morph_set([(firsts[1], 8, 0)], [cases.static_track([0.5, np.nan])])
    with pytest.raises(api.ZetaRayError) as e:
        S.set_morph(static)
    assert e.value.code == 1 and "a rest weight is not finite" in str(e.value) and state() == s1
    import ctypes as C
    L = api.lib()
    d = good.c_desc()
    d.deltas = None
    assert L.zr_scene_set_morph(S.h, C.addressof(d)) == 1 and b"null table with a non-zero count" in L.zr_last_error() and state() == s1
    # the old set is still the one that runs, and equals the host form
    S.animate(1.25)
    assert S.download_vertices().tobytes() == cases.posed_scene_vertices(anim, skin, good, sc.vertices, 1.25).tobytes()
    S.close()


def test_cpp_mirror_poses_a_morphed_file_either_way(api, tmp_path):
    """zrh_scene_animate (zr_host.h) on the loaded fixture, twin scenes: the host form (begin_frame, zrh_scene_data_animate, the skin's and the morph set's
    posed vertices handed over with zr_scene_update_vertices_async, then the instance hand-over) and, after zrh_scene_data_set_device_animation +
    _set_device_skinning + _set_device_morph, the time alone -- the tables reach the device scene with the first frame.  Vertices, instance buffers,
    matrices and light records are the same bytes, the vertices are those of the host form computed in the test, and they are not the rest pose's"""
    import ctypes as C
    import os
    path = cases.morphed_gltf(tmp_path)
    sc, _ = scene_io.load_gltf_native(path)
    host, dev = acases.HostData.from_gltf(path), acases.HostData.from_gltf(path)
    A, B = api.Scene(sc), api.Scene(sc)
    L = acases.sio()
    for fn in (L.zrh_scene_data_set_device_animation, L.zrh_scene_data_set_device_skinning, L.zrh_scene_data_set_device_morph):
        fn.argtypes = [C.c_void_p, C.c_int]
        fn(dev.h, 1)
    Hl = C.CDLL(os.path.join(scases.ROOT, "zetaray_amd", "libzetaray_host.so"))
    Hl.zrh_scene_animate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    assert not A.has_morph() and not B.has_morph()
    for t in acases.TIMES:
        assert Hl.zrh_scene_animate(host.h, A.h, None, t) == 0, api.lib().zr_last_error()
        assert Hl.zrh_scene_animate(dev.h, B.h, None, t) == 0, api.lib().zr_last_error()
        api._check(api.lib().zr_device_synchronize(0))
        _assert_scene_bytes(B, A, host, f"t = {t}")
        want = cases.posed_scene_vertices(sc.animation, sc.skinning, sc.morph, sc.vertices, t)
        assert A.download_vertices().tobytes() == want.tobytes(), f"t = {t}: the mirror's host form"
    assert B.has_morph() and B.has_skinning() and not A.has_morph() and not A.has_skinning()
    assert A.download_vertices()["pos"].tobytes() != sc.vertices["pos"].tobytes()
    A.close(); B.close(); host.close(); dev.close()
