"""zr_scene_update_vertices / zr_scene_set_skinning: skinned vertices posed on the device by every zr_scene_animate (zr_tu_pose.hip), against the host form --
zrh_scene_data_animate, zr_scene_update_vertices with the vertices include/zr_skin.h computes on the host, then the host-form emissive and instance
updates -- bit for bit: the vertex buffer, both instance buffers, toWorld, the emissive records, rendered frames (through which the hit tables and the
refit tree are held), a fresh scene made from the posed vertices, update_vertices on its own across streams and under the background rebuild, the
picked-instance mask, and the calls refused.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests.animmath import cases as acases
from tests.skinmath import cases
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RPT_PLANES = ("A", "B", "C", "D", "E", "F", "G", "neighbor", "map_ctn", "map_ntc")
W, H = 96, 64
TIMES = acases.TIMES      # before every first key (the bind pose), between keys, on the chain's last key (1.25), beyond it (looping and not: joint_chain alternates)


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


@pytest.fixture(scope="module")
def world():
    """the Cornell box + two tubes; tube k's vertices start at firsts[k]"""
    sc, firsts = cases.skinned_cornell(1)
    return sc, firsts


def _skin(sc, anim_joints, ranges, seed=1):
    """a SkinDesc over vertex ranges [(first, count)] of the scene: influence records range after range"""
    anim, joints = anim_joints
    rng = np.random.default_rng(seed)
    infl, rr, k = [], [], 0
    for first, count in ranges:
        infl.append(cases.tube_influences(sc.vertices[first:first + count], len(joints), rng))
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


def _twins(api, sc, anim, skin, moving=False):
    host = acases.HostData.from_scene(sc)
    assert host.set_animation(anim) == 0
    A, B = api.Scene(sc), api.Scene(sc)
    if moving:
        B.set_object_emissives(host.init)
    B.set_animation(anim)
    B.set_skinning(skin)
    return host, A, B


def _run_twins(api, sc, anim, skin, what):
    host, A, B = _twins(api, sc, anim, skin)
    rest = cases.rest_of_ranges(skin, sc.vertices)
    untouched = np.ones(len(sc.vertices), bool)
    for r in skin.ranges:
        untouched[int(r["first_vertex"]):int(r["first_vertex"]) + int(r["num_vertices"])] = False
    seen = set()
    for t in TIMES:
        posed = cases.apply_host_form(A, host, anim, skin, rest, t)
        B.animate(t)
        _assert_scene_bytes(B, A, host, f"{what}, t = {t}")
        got = B.download_vertices()
        assert got[untouched].tobytes() == sc.vertices[untouched].tobytes(), f"{what}: a vertex outside the ranges changed"
        seen.add(posed.tobytes())
    assert len(rest) < 63 or (len(seen) >= 3 and posed["pos"].tobytes() != rest["pos"].tobytes())      # (the lowest ring hangs on the static root alone)
    A.close(); B.close(); host.close()


@pytest.mark.parametrize("count,offset", [(1, 0), (63, 1), (65, 2), (255, 3), (256, 0), (257, 1), (1025, 2), (1025, 3)])
def test_vertex_counts_and_window_alignments(api, world, count, offset):
    """twin scenes at the six times of tests/animmath/cases.py; 1 / 63 / 65 / 255 / 256 / 257 / 1 025 skinned vertices: lanes end inside a wave, at a wave boundary, at a block's
    boundary and across blocks.  The range starts at vertex 130 + offset, even and odd: the 28-byte records of the range start 8, 4, 0 and 12 bytes behind
    a 16-byte boundary of the vertex buffer, and the influence records at even and odd places of their table (a 16-byte word first, or an 8-byte one)"""
    sc, firsts = world
    skin = _skin(sc, cases.joint_chain(4), [(firsts[0] + offset, count)])
    _run_twins(api, sc, cases.joint_chain(4)[0], skin, f"{count} vertices from {firsts[0] + offset}")


@pytest.mark.parametrize("nj", [1, 2, 64, 65])
def test_joint_counts(api, world, nj):
    """1, 2, 64 and 65 joints (the joint kernel's lanes end inside a wave, at its boundary and past it), the whole tube skinned"""
    sc, firsts = world
    aj = cases.joint_chain(nj)
    _run_twins(api, sc, aj[0], _skin(sc, aj, [(firsts[0], cases.TUBE_VERTS)]), f"{nj} joints")


def test_two_ranges_under_one_skin_and_two_skins(api, world):
    """two ranges of one tube under one joint table (the second starts at an odd vertex and shares no influence with the first); then two joint chains in
    one table, one tube each"""
    sc, firsts = world
    aj = cases.joint_chain(5)
    _run_twins(api, sc, aj[0], _skin(sc, aj, [(firsts[0], 300), (firsts[0] + 333, 515)]), "two ranges")
    a, ja = cases.joint_chain(4, seed=3)
    b, jb = cases.joint_chain(3, seed=9, x=cases.TUBE_X + 0.45)
    anim, joints = cases.concat(a, ja, b, jb)
    rng = np.random.default_rng(2)
    f0 = cases.tube_influences(sc.vertices[firsts[0]:firsts[0] + cases.TUBE_VERTS], 4, rng)
    f1 = cases.tube_influences(sc.vertices[firsts[1]:firsts[1] + cases.TUBE_VERTS], 3, rng)
    f1["joint"] += 4
    skin = wire.SkinDesc(joints, np.array([(firsts[0], cases.TUBE_VERTS, 0), (firsts[1], cases.TUBE_VERTS, cases.TUBE_VERTS)], wire.SKIN_RANGE), np.concatenate([f0, f1]))
    _run_twins(api, sc, anim, skin, "two skins")


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
    """the tube skinned over 6 joints and the short box (instance 8) translating as an animated instance of its own"""
    M = sc.instance_to_world[8].reshape(3, 4).astype(np.float64)
    s = float(np.linalg.norm(M[:, 0]))
    ang = float(np.arctan2(M[0, 2], M[0, 0]))
    aj = cases.joint_chain(6, moving_instances=[(8, (np.float32([s] * 3), cases.quat([0, 1, 0], ang), M[:, 3].astype(np.float32)))])
    return aj[0], _skin(sc, aj, [(firsts[0], cases.TUBE_VERTS)])


def _frames_twin(api, sc, anim, skin, host, offs=None):
    rest = cases.rest_of_ranges(skin, sc.vertices)
    prm = wire.default_params()
    ra = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    rb = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    da, db = ra.enable_direct(wire.default_params_di()), rb.enable_direct(wire.default_params_di())
    rb.scene.set_object_emissives(host.init)
    rb.set_animation(anim)
    rb.set_skinning(skin)
    prev, frames = None, []
    for f in range(1, 6):
        if f in FRAME_TIMES:
            cases.apply_host_form(ra.scene, host, anim, skin, rest, FRAME_TIMES[f])
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
    assert frames[1]["gb_depth"].tobytes() != frames[4]["gb_depth"].tobytes()      # the tube really moved on screen
    assert float(frames[-1]["final"][..., :3].max()) > 0


def test_rendered_frames_equal_the_host_form(api, world):
    """ReSTIR PT at 96 x 64 with emissive ReSTIR DI attached, frame 1 at rest and four frames at advancing t: G-buffer planes, FINAL, the DI image, every
    reservoir plane and the ray counters equal the host form's -- the hit tables and the refit tree, current and previous, are held through these"""
    sc, firsts = world
    anim, skin = _moving_setup(sc, firsts)
    host = acases.HostData.from_scene(sc)
    assert host.set_animation(anim) == 0
    _frames_twin(api, sc, anim, skin, host)
    host.close()


def test_the_loaded_fixture_renders_as_the_host_form(api, tmp_path):
    """tests/golden/skin_gltf through load_gltf_native -- the light translates, the boxes move, three skinned tubes bend -- with the loader's own tables
    (sc.animation, sc.skinning) on both sides: the same frame sequence, the same equalities"""
    path = cases.skinned_gltf(tmp_path)
    sc, offs = scene_io.load_gltf_native(path)
    host = acases.HostData.from_gltf(path)
    _frames_twin(api, sc, sc.animation, sc.skinning, host, offs)
    host.close()


def _gbuffer_and_final(r, cb):
    r.render_frame(cb)
    return [np.asarray(p).copy() for p in r.gbuffer.download()[0]], r.final().copy()


def test_one_frame_against_a_fresh_scene_and_a_skin_only_scene(api, world):
    """a skin-only scene -- no instance moves, the moved list is empty -- at two times: after animate(t) the G-buffer and a path-traced frame equal those of
    a scene CREATED from the host-posed vertices (a tree built over the deformed triangles against the refit one; no temporal pass), and the two times'
    frames differ: the refit read the rewritten vertex buffer although nothing moved"""
    sc, firsts = world
    aj = cases.joint_chain(6)
    anim, skin = aj[0], _skin(sc, aj, [(firsts[0], cases.TUBE_VERTS)])
    assert len(anim.instance_idx) == 0
    rest = cases.rest_of_ranges(skin, sc.vertices)
    prm = wire.default_params()
    rb = api.Renderer(sc, W, H, params=prm)
    rb.set_animation(anim)
    rb.set_skinning(skin)
    cb = scene_io.make_frame_constants(W, H, frame_num=1, num_emissives=len(sc.emissives))
    finals = []
    for t in (0.45, 1.1):
        rb.animate(t)
        assert not rb.scene.instances_in_motion
        fresh = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_emissive.npz"))
        for name in ("vertices", "indices", "instances", "instance_to_world", "instance_mask", "instance_num_tris"):
            setattr(fresh, name, getattr(sc, name).copy())
        fresh.vertices[firsts[0]:firsts[0] + cases.TUBE_VERTS] = cases.host_posed(anim, skin, rest, t)
        assert rb.scene.download_vertices().tobytes() == fresh.vertices.tobytes()
        rc = api.Renderer(fresh, W, H, params=prm)
        (gb_b, fin_b), (gb_c, fin_c) = _gbuffer_and_final(rb, cb), _gbuffer_and_final(rc, cb)
        for nm, b, c in zip(wire.GB_PLANE_NAMES, gb_b, gb_c):
            assert b.tobytes() == c.tobytes(), f"t = {t}: G-buffer plane {nm} differs from the fresh scene's"
        assert fin_b.tobytes() == fin_c.tobytes(), f"t = {t}: the path-traced frame differs from the fresh scene's"
        finals.append((gb_b[wire.GB_PLANE_NAMES.index("depth")], fin_b))
    assert finals[0][0].tobytes() != finals[1][0].tobytes() and finals[0][1].tobytes() != finals[1][1].tobytes()


# ---------------------------------------------------------------------------------------------------------------- update_vertices on its own
def _deformed(sc, firsts, k):
    """the tube bent by hand: a caller's own deformation of vertices [first + 7, first + 7 + 900)"""
    first, n = firsts[0] + 7, 900
    v = sc.vertices[first:first + n].copy()
    y = v["pos"][:, 1]
    v["pos"][:, 0] += np.float32(0.05 * k) * np.sin(3 * y).astype(np.float32)
    v["normal"] = np.roll(v["normal"], k, axis=0)
    return first, v


def _fresh_with(sc, first, v):
    fresh = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_emissive.npz"))
    for name in ("vertices", "indices", "instances", "instance_to_world", "instance_mask", "instance_num_tris"):
        setattr(fresh, name, getattr(sc, name).copy())
    fresh.vertices[first:first + len(v)] = v
    return fresh


def test_update_vertices_then_an_instance_update_renders_the_new_geometry(api, world):
    """a replaced range + an instance update with unchanged records: the frame equals that of a scene created with those vertices; before the instance
    update the vertex buffer already holds the new records.  Then the same on two streams: the updates enqueued on one, the frame rendered on another,
    no host wait in between"""
    import torch
    sc, firsts = world
    prm = wire.default_params()
    cb = scene_io.make_frame_constants(W, H, frame_num=1, num_emissives=len(sc.emissives))
    r = api.Renderer(sc, W, H, params=prm)
    v0 = r.scene.version
    for k, streams in ((1, None), (2, (torch.cuda.Stream(), torch.cuda.Stream()))):
        first, v = _deformed(sc, firsts, k)
        rc = api.Renderer(_fresh_with(sc, first, v), W, H, params=prm)
        gb_c, fin_c = _gbuffer_and_final(rc, cb)
        if streams is None:
            r.scene.update_vertices(first, v)
            assert r.scene.download_vertices(first, len(v)).tobytes() == v.tobytes()
            r.scene.update_instances(sc.instances, sc.instance_to_world)
            gb_r, fin_r = _gbuffer_and_final(r, cb)
        else:
            r.scene.update_vertices(first, v, stream=streams[0].cuda_stream)
            r.scene.update_instances(sc.instances, sc.instance_to_world, stream=streams[0].cuda_stream)
            r.render_frame(cb, stream=streams[1].cuda_stream)
            torch.cuda.synchronize()
            gb_r, fin_r = [np.asarray(p).copy() for p in r.gbuffer.download()[0]], r.final().copy()
        for nm, a, b in zip(wire.GB_PLANE_NAMES, gb_r, gb_c):
            assert a.tobytes() == b.tobytes(), f"deformation {k}: G-buffer plane {nm}"
        assert fin_r.tobytes() == fin_c.tobytes(), f"deformation {k}: the path-traced frame"
    assert r.scene.version == v0 + 4


def test_update_vertices_with_the_background_rebuild_installed_mid_sequence(api, world):
    """zr_scene_set_background_rebuild on B only; every frame replaces the range and moves the short box until a background tree has been installed: B's
    frames stay A's (the builder delivers topology; the installing update's refit makes the boxes from the device's vertices)"""
    sc, firsts = world
    prm = wire.default_params()
    ra, rb = api.Renderer(sc, W, H, params=prm), api.Renderer(sc, W, H, params=prm)
    rb.scene.set_background_rebuild(True)
    cb = scene_io.make_frame_constants(W, H, frame_num=1, num_emissives=len(sc.emissives))
    installed, f = 0, 0
    while installed < 1 and f < 40:
        f += 1
        first, v = _deformed(sc, firsts, f % 5)
        xf = sc.instance_to_world.copy()
        xf[8, 7] += np.float32(0.01 * f)
        inst = sc.instances.copy()
        inst["translation"][8, 1] = xf[8, 7]
        for r in (ra, rb):
            r.scene.update_vertices(first, v)
            r.scene.update_instances(inst, xf)
        t0 = time.perf_counter()
        while rb.scene.background_rebuild_stats()[2] == 1 and time.perf_counter() - t0 < 20.0:      # (the builder's thread: a deterministic schedule)
            time.sleep(0.002)
        (gb_a, fin_a), (gb_b, fin_b) = _gbuffer_and_final(ra, cb), _gbuffer_and_final(rb, cb)
        for nm, a, b in zip(wire.GB_PLANE_NAMES, gb_a, gb_b):
            assert a.tobytes() == b.tobytes(), f"frame {f}: G-buffer plane {nm}"
        assert fin_a.tobytes() == fin_b.tobytes(), f"frame {f}: FINAL"
        installed = rb.scene.background_rebuild_stats()[1]
    assert installed >= 1, f"no background tree installed within {f} frames"


def test_the_picked_outline_follows_the_pose(api, world):
    """the picked-instance mask (ZR_OUT_PICK_MASK) of the skinned instance after animate: tests/pickcheck.py's restatement fed the host-posed vertices, and
    not the mask of the rest pose"""
    from tests import pickcheck as pk
    from tests.test_pick_outline_gpu import Frame
    sc, firsts = world
    aj = cases.joint_chain(6)
    anim, skin = aj[0], _skin(sc, aj, [(firsts[0], cases.TUBE_VERTS)])
    rest = cases.rest_of_ranges(skin, sc.vertices)
    tube_inst = len(sc.instances) - 2
    fb = Frame(sc, (W, H), (W, H))
    fb.scene.set_animation(anim)
    fb.scene.set_skinning(skin)
    fb.pick(48, 40)
    fb.show([tube_inst])
    at_rest = fb.p.download_plane("pick_mask").copy()
    fb.scene.animate(1.1)
    fb.show([tube_inst])
    got = fb.p.download_plane("pick_mask")
    posed = cases.host_posed(anim, skin, rest, 1.1)
    base, ib = int(sc.instances["base_vtx_offset"][tube_inst]), int(sc.instances["base_idx_offset"][tube_inst])
    vertices = sc.vertices.copy()
    vertices[firsts[0]:firsts[0] + cases.TUBE_VERTS] = posed
    idx = sc.indices[ib:ib + 3 * int(sc.instance_num_tris[tube_inst])].astype(np.int64) + base
    tris = vertices["pos"][idx].reshape(-1, 3, 3).astype(np.float32)
    want = pk.raster_mask(tris, pk.wvp(sc.instance_to_world[tube_inst], fb.cb["curr_view_proj"]), (W, H), (W, H))
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} mask pixels differ from the restatement's"
    assert want.any() and not np.array_equal(want, at_rest)


# ---------------------------------------------------------------------------------------------------------------- refusals, clearing
def test_refusals_change_nothing_and_clearing_restores_the_rest_pose(api, world):
    """every refusal with the scene's buffers unchanged; a clear puts the rest-pose bytes back; set_animation clears a skin"""
    sc, firsts = world
    aj = cases.joint_chain(4)
    anim = aj[0]
    good = _skin(sc, aj, [(firsts[0] + 1, 700)])
    S = api.Scene(sc)

    def state():
        return S.download_vertices().tobytes() + S.download_instances(0)[0].tobytes() + S.download_emissives().tobytes()

    s0 = state()
    assert S.download_vertices().tobytes() == sc.vertices.tobytes()
    with pytest.raises(api.ZetaRayError) as e:
        S.set_skinning(good)
    assert e.value.code == 6 and "zr_scene_set_animation" in str(e.value) and state() == s0
    L = api.lib()
    L.zr_scene_update_vertices.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    some = sc.vertices[:8].copy()
    assert L.zr_scene_update_vertices(S.h, len(sc.vertices) - 7, 8, some.ctypes.data) == 1 and b"exceeds" in L.zr_last_error() and state() == s0
    assert L.zr_scene_update_vertices(S.h, 0xfffffff0, 0x20, some.ctypes.data) == 1 and state() == s0      # first + count wraps in 32 bits
    assert L.zr_scene_update_vertices(S.h, 0, 8, None) == 1 and b"null" in L.zr_last_error() and state() == s0
    S.set_animation(anim)
    S.set_skinning(good)
    S.animate(0.5)
    s1 = state()
    assert s1 != s0

    def bad(edit):
        j, r, f = good.joints.copy(), good.ranges.copy(), good.influences.copy()
        edit(j, r, f)
        return wire.SkinDesc(j, r, f)

    def node(j, r, f): j["node"][2] = len(anim.nodes)
    def joint(j, r, f): f["joint"][5, 3] = 4
    def past(j, r, f): r["first_vertex"][0] = len(sc.vertices) - 699
    def weight(j, r, f): f["weight"][9, 0] = np.nan
    def matrix(j, r, f): j["inverse_bind"][0, 3] = np.inf
    for edit, word in ((node, f"node {len(anim.nodes)}"), (joint, "joint 4, the table has 4"), (past, "the scene has"), (weight, "weight is not finite"), (matrix, "inverse bind matrix is not finite")):
        with pytest.raises(api.ZetaRayError) as e:
            S.set_skinning(bad(edit))
        assert e.value.code == 1 and word in str(e.value), str(e.value)
        assert state() == s1
    two = wire.SkinDesc(good.joints, np.array([(firsts[0], 100, 0), (firsts[0] + 99, 100, 100)], wire.SKIN_RANGE), good.influences)
    with pytest.raises(api.ZetaRayError) as e:
        S.set_skinning(two)
    assert e.value.code == 1 and "overlaps" in str(e.value) and state() == s1
    many = np.zeros(65536, wire.SKIN_JOINT)
    many["inverse_bind"] = cases.IDENTITY
    with pytest.raises(api.ZetaRayError) as e:
        S.set_skinning(wire.SkinDesc(many, good.ranges, good.influences))
    assert e.value.code == 1 and "65536 joints" in str(e.value) and state() == s1
    # the old set is still the one that runs, and equals the host form
    host = acases.HostData.from_scene(sc)
    assert host.set_animation(anim) == 0
    A = api.Scene(sc)
    rest = cases.rest_of_ranges(good, sc.vertices)
    for t in (0.5, 1.25):
        cases.apply_host_form(A, host, anim, good, rest, t)
    S.animate(1.25)
    assert S.download_vertices().tobytes() == A.download_vertices().tobytes()
    # a replacing set: the old ranges go back to rest, the new ones are posed from the REST records
    other = _skin(sc, aj, [(firsts[0] + 400, 600)], seed=4)
    S.set_skinning(other)
    assert S.download_vertices().tobytes() == sc.vertices.tobytes()
    S.animate(0.5)
    want = sc.vertices.copy()
    want[firsts[0] + 400:firsts[0] + 1000] = cases.host_posed(anim, other, cases.rest_of_ranges(other, sc.vertices), 0.5)
    assert S.download_vertices().tobytes() == want.tobytes()
    S.set_skinning(None)
    assert S.download_vertices().tobytes() == sc.vertices.tobytes()
    S.animate(0.8)
    assert S.download_vertices().tobytes() == sc.vertices.tobytes()
    S.set_skinning(good)
    S.animate(0.8)
    assert S.download_vertices().tobytes() != sc.vertices.tobytes()
    S.set_animation(anim)      # a new animation: the skin set on the old one goes, the rest pose comes back
    assert S.download_vertices().tobytes() == sc.vertices.tobytes()
    S.animate(0.8)
    assert S.download_vertices().tobytes() == sc.vertices.tobytes()
    A.close(); S.close(); host.close()


def test_cpp_mirror_poses_a_skinned_file_either_way(api, tmp_path):
    """zrh_scene_animate (zr_host.h) on the loaded fixture, twin scenes: the host form (begin_frame, zrh_scene_data_animate, zrh_scene_data_skin_pose handed
    over with zr_scene_update_vertices_async, then the instance hand-over) and, after zrh_scene_data_set_device_animation + _set_device_skinning, the time
    alone -- the animation and skin tables reach the device scene with the first frame.  Vertices, instance buffers, matrices and light records are the
    same bytes, the vertices are those of the host form computed in the test, and they are not the bind pose's: the file does not render frozen"""
    path = cases.skinned_gltf(tmp_path)
    sc, _ = scene_io.load_gltf_native(path)
    host, dev = acases.HostData.from_gltf(path), acases.HostData.from_gltf(path)
    A, B = api.Scene(sc), api.Scene(sc)
    L = acases.sio()
    for fn in (L.zrh_scene_data_set_device_animation, L.zrh_scene_data_set_device_skinning):
        fn.argtypes = [C.c_void_p, C.c_int]
        fn(dev.h, 1)
    Hl = C.CDLL(os.path.join(ROOT, "zetaray_amd", "libzetaray_host.so"))
    Hl.zrh_scene_animate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    rest = cases.rest_of_ranges(sc.skinning, sc.vertices)
    assert not A.has_skinning() and not B.has_skinning()
    for t in acases.TIMES:
        assert Hl.zrh_scene_animate(host.h, A.h, None, t) == 0, api.lib().zr_last_error()
        assert Hl.zrh_scene_animate(dev.h, B.h, None, t) == 0, api.lib().zr_last_error()
        api._check(api.lib().zr_device_synchronize(0))
        _assert_scene_bytes(B, A, host, f"t = {t}")
        want = sc.vertices.copy()
        k = 0
        posed = cases.host_posed(sc.animation, sc.skinning, rest, t)
        for r in sc.skinning.ranges:
            want[int(r["first_vertex"]):int(r["first_vertex"]) + int(r["num_vertices"])] = posed[k:k + int(r["num_vertices"])]
            k += int(r["num_vertices"])
        assert A.download_vertices().tobytes() == want.tobytes(), f"t = {t}: the mirror's host form"
    assert B.has_skinning() and not A.has_skinning()
    assert A.download_vertices()["pos"].tobytes() != sc.vertices["pos"].tobytes()
    A.close(); B.close(); host.close(); dev.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from zetaray_amd import api, scene_io
sc = scene_io.load_npz(sys.argv[2])
s = api.Scene(sc)
before = s.download_vertices().tobytes()
try:
    s.update_vertices(3, sc.vertices[10:20])
    print("NOT REFUSED")
except api.ZetaRayError as e:
    print("refused", e.code, "unchanged" if s.download_vertices().tobytes() == before else "CHANGED", str(e))
"""


@pytest.mark.parametrize("mode", ["rebuild", "rebuild_host"])
def test_rebuild_mode_refuses_update_vertices(api, mode):
    """the host-synchronous update modes: ZR_SCENE_UPDATE set for a fresh child process, not for this one"""
    env = dict(os.environ, ZR_SCENE_UPDATE=mode)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests", "golden", "cornell_emissive.npz")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("refused 5 unchanged") and f"ZR_SCENE_UPDATE={mode} " in out.stdout, out.stdout
