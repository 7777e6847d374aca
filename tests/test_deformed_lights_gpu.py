"""Deformed lights: the EmissiveTriangle records of posed meshes re-derived on the device (k_refresh_emissives, zr_tu_scene_update.hip) -- the listed form
behind every zr_scene_animate of a scene with a skin or morph set, the range form as zr_scene_refresh_emissives -- against the host form
(zrh_scene_data_refresh_emissives between the vertex hand-over and the host-form emissive and instance updates), byte for byte: vertex buffer, both
instance buffers, toWorld, world and object-space light records, rendered frames (through which the hit tables and the refit tree are held), a fresh scene
made from the posed vertices and the host-form records, the alias table, two streams, clearing, and the calls refused.  No tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.animmath import cases as acases
from tests.lightmath import cases as lcases
from tests.morphmath import cases as mcases
from tests.skinmath import cases as scases
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
W, H = 96, 64
TIMES = (0.0, 0.3, 0.5, 1.25, 2.0)
TUBE0, TUBE1, LAMP = lcases.TUBE0, lcases.TUBE1, lcases.LAMP
COUNTS = [(1, 1), (63, 1), (65, 0), (255, 1), (256, 0), (257, 1), (1025, 0), (1025, 1)]      # kBlock = 256, wave 64; the range starts at an even / odd vertex


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


@pytest.fixture(scope="module")
def world():
    """the Cornell box + two emissive tubes: tube 0's light triangles, the lamp's two, tube 1's"""
    return lcases.lit_world()


@pytest.fixture(scope="module")
def plain_anim():
    """an animation that moves no instance"""
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
    eb, ea = B.download_emissives(), A.download_emissives()
    assert eb.tobytes() == ea.tobytes() == host.ems.tobytes(), f"{what}: {int((eb != ea).sum())} emissive records differ from the host form's, {int((ea != host.ems).sum())} of the host form's from the host's"
    ob, oh = B.download_object_emissives(), lcases.object_records(host)
    assert ob.tobytes() == oh.tobytes(), f"{what}: {int((ob != oh).sum())} object-space records differ from the host's"


def _device_scene(api, sc, anim, skin, morph):
    B = api.Scene(sc)
    B.set_object_emissives(sc.emissives_initial)
    B.set_animation(anim)
    if skin is not None:
        B.set_skinning(skin)
    if morph is not None:
        B.set_morph(morph)
    return B


def _run_twins(api, sc, anim, skin, morph, what, times=TIMES, still=(LAMP,)):
    """A takes the host sequence, B the sets + animate: every device byte equal at every time.  The lights no range touches, of instances in `still`, keep
    the bytes they had; the listed ones do not"""
    host = acases.HostData.from_scene(sc)
    assert host.set_animation(anim) == 0
    ra, rb = api.Renderer(sc, W, H), api.Renderer(sc, W, H)
    A, B = ra.scene, rb.scene
    B.set_object_emissives(sc.emissives_initial)
    B.set_animation(anim)
    if skin is not None:
        B.set_skinning(skin)
    if morph is not None:
        B.set_morph(morph)
    listed = lcases.listed_lights(sc, lcases.set_ranges(skin, morph))
    rigid = np.ones(len(sc.emissives), bool)
    rigid[listed] = False
    for i in range(len(sc.instances)):
        b = int(sc.instances[i]["base_emissive_tri_offset"])
        if b != lcases.NONE and i not in still and i in [int(j) for j in anim.instance_idx]:
            rigid[b:b + int(sc.instance_num_tris[i])] = False
    assert rigid.any() and len(listed)
    before = B.download_emissives()
    changed = np.zeros(len(sc.emissives), bool)
    for t in times:
        lcases.apply_host_form(A, host, sc, anim, skin, morph, t)
        B.animate(t)
        _assert_scene_bytes(B, A, host, f"{what}, t = {t}")
        got = B.download_emissives()
        assert got[rigid].tobytes() == before[rigid].tobytes(), f"{what}, t = {t}: a rigid light's record changed"
        changed |= got != before
    # (a skinned vertex that hangs on the static root joint alone never moves: most of the listed lights change, not each)
    assert changed[listed].mean() > 0.5, f"{what}: {int((~changed[listed]).sum())} of {len(listed)} listed lights never changed"
    # the two hit tables and the refit tree have no read-back: one frame rendered from either twin holds them at this shape -- every G-buffer plane (the
    # hits, the interpolated normals and tangents) and the path-traced frame, which samples the lights and hits them
    cb = scene_io.make_frame_constants(W, H, frame_num=1, num_emissives=len(sc.emissives))
    ra.render_frame(cb); rb.render_frame(cb)
    for nm, pa, pb in zip(wire.GB_PLANE_NAMES, ra.gbuffer.download()[0], rb.gbuffer.download()[0]):
        assert np.asarray(pa).tobytes() == np.asarray(pb).tobytes(), f"{what}: G-buffer plane {nm}"
    assert ra.final().tobytes() == rb.final().tobytes(), f"{what}: the path-traced frame"
    host.close()
    return listed


# ---------------------------------------------------------------------------------------------------------------- the listed form
@pytest.mark.parametrize("count,parity", COUNTS)
def test_listed_counts(api, world, plain_anim, count, parity):
    """1 / 63 / 65 / 255 / 256 / 257 / 1 025 listed light triangles of tube 0 under a morph-only range: lanes end inside a wave, at a wave's and a block's
    boundary and across blocks.  The owner does not move and its matrix is the identity: k_move_emissives alone would leave these records stale, and the
    records differ from the loader's identity shortcut (decode and re-encode).  The list is not contiguous (a triangle is listed when ANY vertex lies in
    the range: triangles with one, two and three vertices inside, sharing vertices); tube 0's other lights, the lamp's and tube 1's keep their bytes"""
    sc, firsts, base = world
    # (every vertex of a tube is a corner of three triangles or more: the single light is one of the lamp's two, whose owner's matrix is not the identity)
    first, nv = lcases.range_touching(sc, TUBE0 if count > 1 else LAMP, count, parity)
    rng = np.random.default_rng(count)
    morph = mcases.morph_set([(first, nv, 0)], [mcases.keyed_track(rng, 2, loop=parity)], lacks=[0, 0], seed=count + parity)
    listed = _run_twins(api, sc, plain_anim, None, morph, f"{count} lights", still=(LAMP, TUBE0, TUBE1))
    assert len(listed) == count
    if count == 1:
        return
    inside = ((lcases.light_vertices(sc, TUBE0)[listed - base[TUBE0]] >= first) & (lcases.light_vertices(sc, TUBE0)[listed - base[TUBE0]] < first + nv)).sum(axis=1)
    assert count < 63 or {1, 2, 3} <= set(inside.tolist())
    assert count < 63 or (np.diff(listed) != 1).any()


@pytest.mark.parametrize("kind", ["skin", "morph", "both", "all"])
def test_kinds_of_range_with_a_moving_owner(api, world, kind):
    """a skin-only range, a morph-only range, a range that is both, and all three in one scene.  Tube 1 (morph-only in "morph" and "all") is also an animated
    instance: its owner moves (identity at t = 0, translated later), so its listed lights are written by k_move_emissives and then by k_refresh_emissives,
    and its lights outside the range by k_move_emissives alone; tube 0 never moves.  The lamp's records, between the two in the buffer, keep their bytes"""
    sc, firsts, base = world
    ident = (np.float32([1, 1, 1]), np.float32([0, 0, 0, 1]), np.float32([0, 0, 0]))
    aj = scases.joint_chain(6, moving_instances=[(TUBE1, ident)])
    rng = np.random.default_rng(21)
    skin_ranges = {"skin": [(firsts[0] + 2, 401)], "morph": [], "both": [(firsts[0] + 500, 333)], "all": [(firsts[0] + 2, 401), (firsts[0] + 500, 333)]}[kind]
    morph_ranges = {"skin": [], "morph": [(firsts[1] + 7, 290, 0)], "both": [(firsts[0] + 500, 333, 0)], "all": [(firsts[0] + 500, 333, 1), (firsts[1] + 7, 290, 0)]}[kind]
    skin = _skin(sc, aj, skin_ranges) if skin_ranges else None
    morph = mcases.morph_set(morph_ranges, [mcases.keyed_track(rng, 2), mcases.keyed_track(rng, 4, loop=1, zero_at=[(1, 2)])], lacks=[0, 1, 0, 3]) if morph_ranges else None
    _run_twins(api, sc, aj[0], skin, morph, kind)


def test_zero_weights_pose_equals_rest(api, world, plain_anim):
    """a track whose last key (1.25) is all zeros, not looping: from then on the pose IS the rest pose, the object-space records are the bytes the scene
    was created with (the same function on the same positions) and the world records are those re-encoded through the identity matrix"""
    sc, firsts, base = world
    morph = mcases.morph_set([(firsts[0] + 5, 513, 0)], [mcases.keyed_track(np.random.default_rng(3), 3, all_zero_key=2)], lacks=[0, 1, 2])
    B = _device_scene(api, sc, plain_anim, None, morph)
    listed = lcases.listed_lights(sc, [(firsts[0] + 5, 513)])
    B.animate(0.5)
    assert (B.download_object_emissives()[listed] != sc.emissives_initial[listed]).all()
    for t in (1.25, 3.7):
        B.animate(t)
        assert B.download_object_emissives().tobytes() == sc.emissives_initial.tobytes()
        want = sc.emissives.copy()
        want[listed] = scene_io.emissive_to_world(sc.emissives_initial[listed], scases.IDENTITY)
        assert B.download_emissives().tobytes() == want.tobytes()
    B.close()


# ---------------------------------------------------------------------------------------------------------------- the range form
def _bent(sc, seed):
    """every vertex of both tubes displaced by up to 0.03: a deformation the caller made itself"""
    v = sc.vertices.copy()
    rng = np.random.default_rng(seed)
    lo = int(sc.instances[TUBE0]["base_vtx_offset"])
    v["pos"][lo:] += rng.uniform(-0.03, 0.03, (len(v) - lo, 3)).astype(np.float32)
    return v


@pytest.mark.parametrize("count,parity", COUNTS + [(2 * lcases.TUBE_TRIS + 5 - 100, 0)])
def test_range_form_equals_the_host_form(api, count, parity):
    """zr_scene_update_vertices, then zr_scene_refresh_emissives over light triangles [first, first + count) at the count edges, first even and odd -- called
    BEFORE the frame's instance update (B1) and AFTER it (B2), tube 0 moved by that update: the same bytes, and those of the host form
    (zrh_scene_data_set_instance_world, zrh_scene_data_refresh_emissives, the host-form updates).  The scene has three light records no instance carries
    between the lamp's and tube 1's: the last case's range spans them, and they keep their bytes"""
    sc, firsts, base = lcases.lit_world(ownerless=3)
    bent = _bent(sc, count)
    first = 100 + parity
    M = scases.trs12([0.05, 0.1, -0.02], [0, 1, 0], 0.3, [1.1, 0.9, 1.05])
    host = acases.HostData.from_scene(sc)
    L = lcases.sio()
    A, B1, B2 = api.Scene(sc), api.Scene(sc), api.Scene(sc)
    lo = int(sc.instances[TUBE0]["base_vtx_offset"])
    for S in (A, B1, B2):
        S.update_vertices(lo, bent[lo:])
    # the host form
    L.zrh_scene_data_begin_frame(host.h)
    assert L.zrh_scene_data_set_instance_world(host.h, TUBE0, np.ascontiguousarray(M, np.float32).ctypes.data) == 0
    assert L.zrh_scene_data_refresh_emissives(host.h, bent.ctypes.data, first, count) == 0, L.zrh_scene_io_last_error()
    f, c = C.c_uint32(), C.c_uint32()
    L.zrh_scene_data_dirty_emissives(host.h, C.byref(f), C.byref(c))
    A.update_emissives(host.ems[f.value:f.value + c.value].copy(), f.value)
    A.update_instances(host.inst.copy(), host.world.copy())
    # the device form, both orders
    for S in (B1, B2):
        S.set_object_emissives(sc.emissives_initial)
    B1.refresh_emissives(first, count)
    B1.move_instances([TUBE0], [M])
    B2.move_instances([TUBE0], [M])
    B2.refresh_emissives(first, count)
    for S, what in ((B1, "refresh, then move"), (B2, "move, then refresh")):
        _assert_scene_bytes(S, A, host, f"{what}, [{first}, {first + count})")
    got = B1.download_emissives()
    if first + count > base[LAMP] + 2:
        assert got[base[LAMP] + 2:base[TUBE1]].tobytes() == sc.emissives[base[LAMP] + 2:base[TUBE1]].tobytes()      # the ownerless records
        assert (got[base[TUBE1]:first + count] != sc.emissives[base[TUBE1]:first + count]).all()
    assert (got[first:min(first + count, lcases.TUBE_TRIS)] != sc.emissives[first:min(first + count, lcases.TUBE_TRIS)]).all()
    assert got[first + count:].tobytes() == A.download_emissives()[first + count:].tobytes()
    for S in (A, B1, B2):
        S.close()
    host.close()


def test_range_form_on_a_scene_no_update_has_touched(api, world):
    """the first call on a fresh scene: the owner's matrices are still the host's alone, and reach the device with the call"""
    sc, firsts, base = world
    bent = _bent(sc, 7)
    B = api.Scene(sc)
    B.set_object_emissives(sc.emissives_initial)
    lo = int(sc.instances[TUBE1]["base_vtx_offset"])
    B.update_vertices(lo, bent[lo:])
    B.refresh_emissives(base[TUBE1] + 3, 300)
    import copy
    want = copy.copy(sc)
    want._desc, want.emissives, want.emissives_initial = None, sc.emissives.copy(), sc.emissives_initial.copy()
    assert scene_io.refresh_emissives(want, bent, base[TUBE1] + 3, 300) == (base[TUBE1] + 3, 300)
    assert B.download_emissives().tobytes() == want.emissives.tobytes() != sc.emissives.tobytes()
    assert B.download_object_emissives().tobytes() == want.emissives_initial.tobytes()
    B.close()


# ---------------------------------------------------------------------------------------------------------------- rendered frames
def _cb(sc, f, prev):
    cb = scene_io.make_frame_constants(W, H, frame_num=f, num_emissives=len(sc.emissives))
    if prev is not None:
        cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
    return cb


RPT_PLANES = ("A", "B", "C", "D", "E", "F", "G", "neighbor", "map_ctn", "map_ntc")


def _everything(r, di):
    out = {"final": r.final().copy(), "di": di.download().copy(), "counters": r.p_indirect.read_counters()}
    for nm, pl in zip(wire.GB_PLANE_NAMES, r.gbuffer.download()[0]):
        out["gb_" + nm] = np.asarray(pl).copy()
    for nm in RPT_PLANES:
        a = r.p_indirect.download_plane(nm)
        out["rpt_" + nm] = (a & 0xffffff) if nm == "A" else a
    return out


def _assert_same_frames(want, got, what):
    for k, v in want.items():
        if k == "counters":
            assert got[k] == v, f"{what}: ray counters"
        else:
            assert np.asarray(got[k]).tobytes() == np.asarray(v).tobytes(), f"{what}: {k}"


def _placed_world():
    """lit_world with tube 1 under a static matrix that is NOT the identity (scaled, turned, shifted), its records made through that matrix.  Why: with the
    identity EmissiveToWorld is a decode and a re-encode of the same triangle, so a kernel that read the wrong row of toWorld, or none, would still
    pass; under this matrix the fresh scene's records (the host form's) can only be met by reading tube 1's own row"""
    sc, firsts, base = lcases.lit_world()
    M = np.ascontiguousarray(scases.trs12([-0.35, 0.12, 0.2], [0, 1, 0], 0.4, [0.8, 0.85, 0.8]), np.float32).reshape(12)
    sc.instance_to_world[TUBE1] = M
    L = scene_io._sceneio_lib()
    L.zrh_fill_mesh_instance.argtypes = [C.c_void_p, C.c_void_p]
    inst = sc.instances[TUBE1:TUBE1 + 1].copy()
    L.zrh_fill_mesh_instance(M.ctypes.data, inst.ctypes.data)
    sc.instances[TUBE1] = inst[0]
    b = base[TUBE1]
    sc.emissives[b:b + lcases.TUBE_TRIS] = scene_io.emissive_to_world(sc.emissives_initial[b:b + lcases.TUBE_TRIS], M)
    return sc, firsts, base


def test_frames_equal_a_fresh_scene_made_from_the_pose(api, plain_anim):
    """no stale data anywhere: at two times, the animated scene (sets on the device, animate(t), invalidate_alias_table) renders three ReSTIR PT frames with
    emissive ReSTIR DI attached; a scene CREATED from the posed vertices and the host-form records renders the same three -- G-buffer, FINAL, the DI
    image, every reservoir plane, the ray counters.  Light sampling (alias table, presampled sets, voxel grid, K2's powers) reads the records, a ray
    that hits a light finds the posed triangle in the refit tree: a stale record on either side of the MIS pair shows here.  Both scenes estimate
    their powers from the same records (the invalidate); animate(t) runs before every frame, so previous = current on both sides"""
    import copy
    sc, firsts, base = _placed_world()
    rng = np.random.default_rng(41)
    morph = mcases.morph_set([(firsts[0], scases.TUBE_VERTS, 0), (firsts[1] + 40, 1000, 0)], [mcases.keyed_track(rng, 4, loop=1)], lacks=[0, 1, 2, 3], seed=5)
    ranges = lcases.set_ranges(None, morph)
    prm = wire.default_params()
    seen = []
    for t in (0.45, 1.1):
        rb = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
        db = rb.enable_direct(wire.default_params_di())
        rb.scene.set_object_emissives(sc.emissives_initial)
        rb.set_animation(plain_anim)
        rb.set_morph(morph)
        fresh = copy.copy(sc)
        fresh._desc, fresh.emissives, fresh.emissives_initial = None, sc.emissives.copy(), sc.emissives_initial.copy()
        fresh.vertices = lcases.posed_vertices(plain_anim, None, morph, sc.vertices, t)
        for first, count in lcases.runs(lcases.listed_lights(sc, ranges)):
            scene_io.refresh_emissives(fresh, fresh.vertices, first, count)
        rc = api.Renderer(fresh, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
        dc = rc.enable_direct(wire.default_params_di())
        prev = None
        for f in (1, 2, 3):
            rb.animate(t)
            assert not rb.scene.instances_in_motion
            if f == 1:
                rb.invalidate_alias_table()
                assert rb.scene.download_emissives().tobytes() == fresh.emissives.tobytes()
            cb = _cb(sc, f, prev)
            prev = cb.copy()
            for r in (rb, rc):
                r.p_indirect.read_counters(reset=True)
                r.render_frame(cb)
            got, want = _everything(rb, db), _everything(rc, dc)
            del got["counters"], want["counters"]      # (one tree is refit, the other built: the images are held, not the traversal)
            _assert_same_frames(want, got, f"t = {t}, frame {f}")
        assert float(got["di"][..., :3].max()) > 0
        seen.append(got)
    assert seen[0]["di"].tobytes() != seen[1]["di"].tobytes() and seen[0]["gb_depth"].tobytes() != seen[1]["gb_depth"].tobytes()


class _FlaggedHost(acases.HostData):
    @classmethod
    def from_gltf(cls, path, flags=scene_io.LOAD_DEFORMED_LIGHTS):
        L = acases.sio()
        rho, dim = scene_io.load_rho_default()
        rho = np.ascontiguousarray(rho, np.uint16)
        h = C.c_void_p()
        assert L.zrh_gltf_load_ex(os.fsencode(path), rho.ctypes.data, (C.c_uint32 * 3)(*dim), flags, C.byref(h)) == 0, L.zrh_scene_io_last_error()
        return cls(h)


FRAME_TIMES = {2: 0.2, 3: 0.45, 4: 0.7}      # frame 1 is rendered at rest


def test_the_loaded_emissive_fixture_renders_as_the_host_form(api, tmp_path):
    """the morph fixture with the face's material emissive, loaded with deformed_lights=True: the loader's own tables on twin renderers, the host sequence
    against animate, the alias table invalidated on both before every frame -- ReSTIR PT + emissive DI frames, and every scene byte"""
    path = lcases.emissive_morphed_gltf(tmp_path)
    sc, offs = scene_io.load_gltf_native(path, deformed_lights=True)
    anim, skin, morph = sc.animation, sc.skinning, sc.morph
    listed = lcases.listed_lights(sc, lcases.set_ranges(skin, morph))
    assert len(listed) and len(listed) < len(sc.emissives)
    host = _FlaggedHost.from_gltf(path)
    prm = wire.default_params()
    ra = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    rb = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    da, db = ra.enable_direct(wire.default_params_di()), rb.enable_direct(wire.default_params_di())
    rb.scene.set_object_emissives(host.init)
    rb.set_animation(anim)
    if skin is not None:
        rb.set_skinning(skin)
    rb.set_morph(morph)
    prev = None
    for f in range(1, 5):
        if f in FRAME_TIMES:
            lcases.apply_host_form(ra.scene, host, sc, anim, skin, morph, FRAME_TIMES[f])
            rb.animate(FRAME_TIMES[f])
        cb = _cb(sc, f, prev)
        scene_io.set_texture_heap_offsets(cb, offs)
        prev = cb.copy()
        for r in (ra, rb):
            r.invalidate_alias_table()
            r.p_indirect.read_counters(reset=True)
            r.render_frame(cb)
        _assert_same_frames(_everything(ra, da), _everything(rb, db), f"frame {f}")
    _assert_scene_bytes(rb.scene, ra.scene, host, "after the frames")
    assert (rb.scene.download_emissives()[listed] != sc.emissives[listed]).any()
    host.close()


def test_the_loaded_emissive_fixture_against_a_fresh_scene(api, tmp_path):
    """no stale data on the loaded fixture either, and independently of a twin: at two times, the animated scene (animate(t) twice, so that the records
    describe rest at that pose) against a scene CREATED from the posed vertices, the device's instance records and matrices, and light records made
    on the host -- zrh_emissive_to_world for the lights of the instances the animation moves, the rule for the posed ones.  The light records are those
    bytes; one frame with no history on either side -- every G-buffer plane but the motion vectors (one side's records went through the moving-instance
    rule), the emissive DI image and the path-traced frame -- is the same, with both alias tables built from those records"""
    import copy
    path = lcases.emissive_morphed_gltf(tmp_path)
    sc, offs = scene_io.load_gltf_native(path, deformed_lights=True)
    anim, skin, morph = sc.animation, sc.skinning, sc.morph
    listed = lcases.listed_lights(sc, lcases.set_ranges(skin, morph))
    prm = wire.default_params()
    cb = scene_io.make_frame_constants(W, H, frame_num=1, num_emissives=len(sc.emissives))
    scene_io.set_texture_heap_offsets(cb, offs)
    images = []
    for t in (0.45, 1.1):
        rb = api.Renderer(sc, W, H, params=prm)
        db = rb.enable_direct(wire.default_params_di())
        rb.scene.set_object_emissives(sc.emissives_initial)
        rb.set_animation(anim)
        if skin is not None:
            rb.set_skinning(skin)
        rb.set_morph(morph)
        rb.animate(t); rb.animate(t)
        rb.invalidate_alias_table()
        inst, xf = rb.scene.download_instances(0)
        fresh = copy.copy(sc)
        fresh._desc, fresh.emissives, fresh.emissives_initial = None, sc.emissives.copy(), sc.emissives_initial.copy()
        fresh.vertices, fresh.instances, fresh.instance_to_world = lcases.posed_vertices(anim, skin, morph, sc.vertices, t), inst, xf
        for i in (int(j) for j in anim.instance_idx):
            b, n = int(sc.instances[i]["base_emissive_tri_offset"]), int(sc.instance_num_tris[i])
            if b != lcases.NONE:
                fresh.emissives[b:b + n] = scene_io.emissive_to_world(sc.emissives_initial[b:b + n], xf[i])
        for first, count in lcases.runs(listed):
            scene_io.refresh_emissives(fresh, fresh.vertices, first, count)
        assert rb.scene.download_emissives().tobytes() == fresh.emissives.tobytes(), f"t = {t}: light records"
        assert (fresh.emissives[listed] != sc.emissives[listed]).any()
        rc = api.Renderer(fresh, W, H, params=prm)
        dc = rc.enable_direct(wire.default_params_di())
        rb.render_frame(cb); rc.render_frame(cb)
        for nm, pb, pc in zip(wire.GB_PLANE_NAMES, rb.gbuffer.download()[0], rc.gbuffer.download()[0]):
            assert nm == "motion_vector" or np.asarray(pb).tobytes() == np.asarray(pc).tobytes(), f"t = {t}: G-buffer plane {nm}"
        assert db.download().tobytes() == dc.download().tobytes(), f"t = {t}: the DI image"
        assert rb.final().tobytes() == rc.final().tobytes(), f"t = {t}: the path-traced frame"
        images.append(db.download().copy())
    assert images[0].tobytes() != images[1].tobytes() and float(images[0][..., :3].max()) > 0


# ---------------------------------------------------------------------------------------------------------------- the alias table
def test_alias_table_follows_only_when_invalidated(api, plain_anim):
    """animate, then a PRELIGHTING render under set_alias_build("device"): without invalidate_alias_table the table is the old one, byte for byte (moving or
    deforming a light re-estimates nothing: the reference's rule); with it, zr_pass_get_emissive_powers and the table equal, in every bit, those of a scene
    created from the posed vertices and the host-form records"""
    import copy
    sc, firsts, base = _placed_world()
    morph = mcases.morph_set([(firsts[0], scases.TUBE_VERTS, 0), (firsts[1] + 40, 1000, 0)], [mcases.keyed_track(np.random.default_rng(9), 3, loop=1)], lacks=[0, 1, 2], seed=2)
    n, t = len(sc.emissives), 0.7
    cb = scene_io.make_frame_constants(32, 32, frame_num=1, num_emissives=n)
    r = api.Renderer(sc, 32, 32)
    r.set_alias_build("device")
    r.scene.set_object_emissives(sc.emissives_initial)
    r.set_animation(plain_anim)
    r.set_morph(morph)
    r.p_prelight.render(cb, r.scene)
    old_table, old_power = r.scene.get_alias_table(), r.p_prelight.get_emissive_powers(n)
    r.animate(t)
    r.p_prelight.render(cb, r.scene)
    assert r.scene.get_alias_table().tobytes() == old_table.tobytes()
    r.invalidate_alias_table()
    r.p_prelight.render(cb, r.scene)
    fresh = copy.copy(sc)
    fresh._desc, fresh.emissives, fresh.emissives_initial = None, sc.emissives.copy(), sc.emissives_initial.copy()
    fresh.vertices = lcases.posed_vertices(plain_anim, None, morph, sc.vertices, t)
    for first, count in lcases.runs(lcases.listed_lights(sc, lcases.set_ranges(None, morph))):
        scene_io.refresh_emissives(fresh, fresh.vertices, first, count)
    q = api.Renderer(fresh, 32, 32)
    q.set_alias_build("device")
    q.p_prelight.render(cb, q.scene)
    power = r.p_prelight.get_emissive_powers(n)
    assert power.tobytes() == q.p_prelight.get_emissive_powers(n).tobytes() != old_power.tobytes()
    assert r.scene.get_alias_table().tobytes() == q.scene.get_alias_table().tobytes() != old_table.tobytes()


# ---------------------------------------------------------------------------------------------------------------- lifetime
def test_clearing_and_replacing_sets_restores_the_saved_records(api, world):
    """clearing the morph set, the skin set or the animation puts back the records (world and object-space) the lights had before the set, with the rest
    vertices; a set that replaces another keeps the records the first one saved, although the device's had been posed by then"""
    sc, firsts, base = world
    aj = scases.joint_chain(6)
    skin = _skin(sc, aj, [(firsts[0] + 2, 401)])
    rng = np.random.default_rng(4)
    morph = mcases.morph_set([(firsts[1] + 7, 290, 0)], [mcases.keyed_track(rng, 2, loop=1)], lacks=[0])
    morph2 = mcases.morph_set([(firsts[1] + 100, 400, 0)], [mcases.keyed_track(rng, 3, loop=1)], lacks=[0, 1], seed=8)
    B = api.Scene(sc)
    B.set_object_emissives(sc.emissives_initial)
    w0, o0 = B.download_emissives(), B.download_object_emissives()
    assert w0.tobytes() == sc.emissives.tobytes() and o0.tobytes() == sc.emissives_initial.tobytes()

    def posed():
        return (B.download_emissives() != w0), (B.download_object_emissives() != o0)

    def at_rest(what):
        assert B.download_emissives().tobytes() == w0.tobytes(), f"{what}: world records"
        assert B.download_object_emissives().tobytes() == o0.tobytes(), f"{what}: object-space records"
        assert B.download_vertices().tobytes() == sc.vertices.tobytes(), f"{what}: vertices"
    tube0, tube1 = slice(base[TUBE0], base[TUBE0] + lcases.TUBE_TRIS), slice(base[TUBE1], base[TUBE1] + lcases.TUBE_TRIS)
    B.set_animation(aj[0]); B.set_skinning(skin); B.set_morph(morph)
    B.animate(0.3)
    pw, po = posed()
    assert pw[tube0].any() and pw[tube1].any() and po[tube0].any() and po[tube1].any()
    B.set_morph(morph2)      # replaces: tube 1's lights go back to rest first, the skin's keep their pose
    pw, po = posed()
    assert not pw[tube1].any() and not po[tube1].any() and pw[tube0].any()
    B.animate(0.6)
    B.set_morph(None)        # the lights morph2 posed -- some of them morph's too -- go back to the bytes before the FIRST set
    pw, po = posed()
    assert not pw[tube1].any() and not po[tube1].any() and pw[tube0].any() and po[tube0].any()
    B.set_morph(morph)
    B.animate(0.9)
    B.set_skinning(None)     # ... and takes the morph set with it
    at_rest("set_skinning(None)")
    assert not B.has_morph()
    B.set_skinning(skin); B.set_morph(morph)
    B.animate(1.1)
    assert posed()[0].any()
    B.set_animation(None)
    at_rest("set_animation(None)")
    B.close()


def test_clearing_a_set_whose_owner_has_moved(api, world):
    """tube 1 is morphed AND an animated instance: when the morph set goes after the animation has moved it, the listed lights' object-space records are
    the saved bytes and their world records stand where the owner stands now -- the moved-light rule on the saved record, what k_move_emissives gave the
    tube's unlisted lights -- not at the placement they were saved at; clearing the animation afterwards leaves all of them there"""
    sc, firsts, base = world
    ident = (np.float32([1, 1, 1]), np.float32([0, 0, 0, 1]), np.float32([0, 0, 0]))
    aj = scases.joint_chain(2, moving_instances=[(TUBE1, ident)])
    morph = mcases.morph_set([(firsts[1] + 7, 290, 0)], [mcases.keyed_track(np.random.default_rng(6), 2, loop=1)], lacks=[0])
    B = _device_scene(api, sc, aj[0], None, morph)
    B.animate(0.6)
    xf = B.download_instances(0)[1][TUBE1]
    assert not np.array_equal(xf, scases.IDENTITY)
    tube1 = slice(base[TUBE1], base[TUBE1] + lcases.TUBE_TRIS)
    want = sc.emissives.copy()
    want[tube1] = scene_io.emissive_to_world(sc.emissives_initial[tube1], xf)
    assert B.download_emissives().tobytes() != want.tobytes()
    B.set_morph(None)
    assert B.download_object_emissives().tobytes() == sc.emissives_initial.tobytes()
    assert B.download_emissives().tobytes() == want.tobytes()
    B.set_animation(None)
    assert B.download_emissives().tobytes() == want.tobytes() and B.download_vertices().tobytes() == sc.vertices.tobytes()
    B.close()


# ---------------------------------------------------------------------------------------------------------------- ordering
def test_animate_on_a_second_stream_while_a_render_samples_the_lights(api, world):
    """a frame that samples the lights rendered on one stream, animate enqueued on another with no host wait in between, then the next frame on the first:
    k_refresh_emissives waits for the render that still reads the records, and the next render for it -- frames and scene bytes equal the host-form
    twin's, which runs on the null stream with waits"""
    import torch
    sc, firsts, base = world
    ident = (np.float32([1, 1, 1]), np.float32([0, 0, 0, 1]), np.float32([0, 0, 0]))
    aj = scases.joint_chain(6, moving_instances=[(TUBE1, ident)])
    skin = _skin(sc, aj, [(firsts[0], scases.TUBE_VERTS)])
    morph = mcases.morph_set([(firsts[0], scases.TUBE_VERTS, 0), (firsts[1], scases.TUBE_VERTS, 1)],
                             [mcases.keyed_track(np.random.default_rng(31), 3, loop=1), mcases.keyed_track(np.random.default_rng(32), 5, zero_at=[(1, 1)])], lacks=[0, 1, 2, 0, 3])
    anim = aj[0]
    host = acases.HostData.from_scene(sc)
    assert host.set_animation(anim) == 0
    prm = wire.default_params()
    ra, rb = api.Renderer(sc, W, H, params=prm), api.Renderer(sc, W, H, params=prm)
    da, db = ra.enable_direct(wire.default_params_di()), rb.enable_direct(wire.default_params_di())
    rb.scene.set_object_emissives(host.init)
    rb.set_animation(anim); rb.set_skinning(skin); rb.set_morph(morph)
    s_render, s_update = torch.cuda.Stream(), torch.cuda.Stream()
    cb = scene_io.make_frame_constants(W, H, frame_num=1, num_emissives=len(sc.emissives))
    for t in (0.2, 0.7, 1.1):
        ra.render_frame(cb)      # (the twin renders the previous pose too: the DI pass keeps a temporal history)
        lcases.apply_host_form(ra.scene, host, sc, anim, skin, morph, t)
        ra.render_frame(cb)
        rb.render_frame(cb, stream=s_render.cuda_stream)      # (a frame of the previous pose, still in flight when the update is enqueued)
        rb.animate(t, stream=s_update.cuda_stream)
        rb.render_frame(cb, stream=s_render.cuda_stream)
        torch.cuda.synchronize()
        assert rb.final().tobytes() == ra.final().tobytes(), f"t = {t}: FINAL"
        assert db.download().tobytes() == da.download().tobytes(), f"t = {t}: the DI image"
        _assert_scene_bytes(rb.scene, ra.scene, host, f"two streams, t = {t}")
    host.close()


# ---------------------------------------------------------------------------------------------------------------- refusals, the C++ mirror
def test_refusals_change_nothing(api, world, plain_anim, monkeypatch):
    sc, firsts, base = world
    n = len(sc.emissives)
    morph = mcases.morph_set([(firsts[0] + 5, 100, 0)], [mcases.keyed_track(np.random.default_rng(1), 2)], lacks=[0])
    B = api.Scene(sc)
    w0 = B.download_emissives()
    # before zr_scene_set_object_emissives: the range form, and a set whose ranges touch lights
    with pytest.raises(api.ZetaRayError) as e:
        B.refresh_emissives(0, 10)
    assert e.value.code == 6 and "zr_scene_set_object_emissives" in str(e.value)
    B.set_animation(plain_anim)
    with pytest.raises(api.ZetaRayError) as e:
        B.set_morph(morph)
    assert e.value.code == 6 and "zr_scene_set_object_emissives" in str(e.value) and not B.has_morph()
    assert B.download_vertices().tobytes() == sc.vertices.tobytes()
    # ... while a set whose ranges touch no light needs none
    wall = mcases.morph_set([(0, 20, 0)], [mcases.keyed_track(np.random.default_rng(2), 2)], lacks=[0])
    B.set_morph(wall)
    B.animate(0.4)
    assert B.download_emissives().tobytes() == w0.tobytes()
    B.set_morph(None)
    B.set_object_emissives(sc.emissives_initial)
    o0 = B.download_object_emissives()
    # a range past the emissive count
    for first, count in ((n, 1), (n - 1, 2), (0xFFFFFFFF, 2), (0, n + 1)):
        with pytest.raises(api.ZetaRayError) as e:
            B.refresh_emissives(first, count)
        assert e.value.code == 1 and "exceeds the scene's" in str(e.value)
    B.refresh_emissives(n, 0)      # (an empty range at the end is no error)
    # ZR_SCENE_UPDATE=rebuild / rebuild_host
    for mode in ("rebuild", "rebuild_host"):
        monkeypatch.setenv("ZR_SCENE_UPDATE", mode)
        with pytest.raises(api.ZetaRayError) as e:
            B.refresh_emissives(0, 10)
        assert e.value.code == 5 and "zr_scene_refresh_emissives" in str(e.value)
    monkeypatch.delenv("ZR_SCENE_UPDATE")
    assert B.download_emissives().tobytes() == w0.tobytes() and B.download_object_emissives().tobytes() == o0.tobytes()
    B.refresh_emissives(0, 10)      # accepted now: at rest, object records as created, world records without the identity shortcut
    assert B.download_object_emissives().tobytes() == o0.tobytes()
    # new object-space records while a set poses lights: refused, the set and its saved records stand; accepted again once the set is cleared
    B.set_morph(morph)
    B.animate(0.4)
    posed = B.download_object_emissives()
    with pytest.raises(api.ZetaRayError) as e:
        B.set_object_emissives(sc.emissives_initial)
    assert e.value.code == 5 and "clear it first" in str(e.value)
    assert B.has_morph() and B.download_object_emissives().tobytes() == posed.tobytes() != o0.tobytes()
    B.set_morph(None)
    assert B.download_object_emissives().tobytes() == o0.tobytes()
    B.set_object_emissives(sc.emissives_initial)
    B.close()


@pytest.mark.parametrize("switches", ["all", "animation"])
@pytest.mark.parametrize("fixture", ["morph", "skin"])
def test_cpp_mirror_poses_an_emissive_file_either_way(api, tmp_path, fixture, switches):
    """zrh_scene_animate (zr_host.h) on the emissive fixtures loaded with ZRH_LOAD_DEFORMED_LIGHTS, twin scenes: the host path (pose, zr_scene_update_vertices,
    zrh_scene_data_refresh_emissives, the host-form updates) and, with every device switch on, the time alone.  With the animation switch alone the sets
    are posed on the host and handed over, the instances move on the device, and the mirror follows the update with zr_scene_refresh_emissives_async over the
    posed lights.  The same bytes each way, and the listed lights move"""
    path = lcases.emissive_morphed_gltf(tmp_path) if fixture == "morph" else lcases.emissive_skinned_gltf(tmp_path)
    sc, _ = scene_io.load_gltf_native(path, deformed_lights=True)
    listed = lcases.listed_lights(sc, lcases.set_ranges(sc.skinning, sc.morph))
    assert len(listed)
    host, dev = _FlaggedHost.from_gltf(path), _FlaggedHost.from_gltf(path)
    A, B = api.Scene(sc), api.Scene(sc)
    L = acases.sio()
    for fn in (L.zrh_scene_data_set_device_animation, L.zrh_scene_data_set_device_skinning, L.zrh_scene_data_set_device_morph)[:3 if switches == "all" else 1]:
        fn.argtypes = [C.c_void_p, C.c_int]
        fn(dev.h, 1)
    Hl = C.CDLL(os.path.join(scases.ROOT, "zetaray_amd", "libzetaray_host.so"))
    Hl.zrh_scene_animate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    moved = np.zeros(len(sc.emissives), bool)
    for t in acases.TIMES[:4]:
        assert Hl.zrh_scene_animate(host.h, A.h, None, t) == 0, api.lib().zr_last_error()
        assert Hl.zrh_scene_animate(dev.h, B.h, None, t) == 0, api.lib().zr_last_error()
        api._check(api.lib().zr_device_synchronize(0))
        _assert_scene_bytes(B, A, host, f"t = {t}")
        moved |= B.download_emissives() != sc.emissives
    assert moved[listed].all()
    assert B.has_skinning() == (switches == "all" and sc.skinning is not None) and B.has_morph() == (switches == "all" and sc.morph is not None)
    A.close(); B.close(); host.close(); dev.close()
