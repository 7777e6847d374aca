"""Skinning, the arithmetic contract of include/zr_skin.h on the host (tests/skinmath/libzsk.so) against a float64 restatement, stage by stage -- each stage
fed the previous stage's float32 outputs --, the tables zr_scene_set_skinning refuses (zrsk::ValidateSkin), and the surface the feature adds."""
import os
import re

import numpy as np
import pytest

from tests.skinmath import cases, zsk
from zetaray_amd import wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
N = 640


@pytest.fixture(scope="module", params=["uniform", "nonuniform"])
def case(request):
    """N vertices over 7 joints: node matrices and inverse bind matrices -> the header's joint matrices; influences of 1, 2, 3 and 4 non-zero weights"""
    rng = np.random.default_rng(11 if request.param == "uniform" else 12)
    nj = 7
    world = cases.joint_set(rng, nj, request.param == "nonuniform")
    bind = cases.joint_set(rng, nj, False)
    ibm = np.array([cases.inverse12(b) for b in bind], F32)
    J = zsk.joint_matrix(world, ibm)
    joint, weight = cases.influence_cases(rng, nj, N)
    return {"world": world, "ibm": ibm, "J": J, "joint": joint, "weight": weight, "rng": rng, "J4": J[joint.astype(np.int64)]}


def test_joint_matrices_against_float64(case):
    """J = nodeWorld x inverseBind through zr_anim.h's Mul: per entry fma(a1 b1, a0 b0) + fma(a3 b3, a2 b2) -- three roundings on the longest path, so
    |J - J64| <= gamma_3 * sum |a_k| |b_k| componentwise"""
    want, mag = cases.joint_matrix64(case["world"], case["ibm"])
    err = np.abs(case["J"].astype(F64) - want)
    print(f"joint matrices: largest error / bound {float((err / (cases.gamma(3) * mag + 1e-300)).max()):.3f}")
    assert (err <= cases.gamma(3) * mag).all()


def test_blend_against_float64(case):
    """M[e] = fma(w3 J3, fma(w2 J2, fma(w1 J1, w0 J0))): four roundings; |M - M64| <= gamma_4 * sum_j |w_j| |J_j[e]|"""
    M = zsk.blend(case["J4"], case["weight"])
    want, mag = cases.blend64(case["J4"], case["weight"])
    err = np.abs(M.astype(F64) - want)
    print(f"blend: largest error / bound {float((err / (cases.gamma(4) * mag + 1e-300)).max()):.3f}")
    assert (err <= cases.gamma(4) * mag).all()
    one = case["weight"][:, 0] == 1      # a single weight of 1 with idle slots naming joint 0 or the last joint: the joint matrix itself, to the bit
    assert one.sum() >= N // 5 and np.array_equal(M[one], case["J4"][one, 0])
    for k in (2, 3, 4):
        assert ((case["weight"] != 0).sum(1) == k).sum() >= N // 6


def test_positions_against_float64(case):
    """p' = M (p, 1) from the joint matrices: four roundings of the blend and four of the row, so componentwise
    |p' - p'64| <= gamma_8 * sum_j |w_j| (|J_j| (|x|, |y|, |z|, 1)); the test computes the bound"""
    p = case["rng"].uniform(-2, 2, (N, 3)).astype(F32)
    got = zsk.position(zsk.blend(case["J4"], case["weight"]), p)
    want, mag = cases.position64(case["J4"], case["weight"], p)
    err = np.abs(got.astype(F64) - want)
    print(f"positions: largest error / bound {float((err / (cases.gamma(8) * mag)).max()):.3f}")
    assert (err <= cases.gamma(8) * mag).all()


def _direction_stage(case, which):
    M = zsk.blend(case["J4"], case["weight"])
    M3 = M.astype(F64).reshape(-1, 3, 4)[:, :, :3]
    cond, det = np.linalg.cond(M3), np.linalg.det(M3)
    assert (cond <= 4).all() and (det > 0).all(), (float(cond.max()), float(det.min()))
    rest = zsk.encode(cases.directions(case["rng"], N))      # normals on both hemispheres and on the fold lines, as stored codes
    d32 = zsk.decode(rest)                                   # the stage's float32 input
    v = np.zeros(N, wire.VERTEX)
    v["normal"] = v["tangent"] = rest
    posed = zsk.pose_vertex(v, M)
    want = (cases.normal64 if which == "normal" else cases.tangent64)(M, d32)
    got = cases.decode_oct64(posed[which])
    a_q = cases.round_trip_angle(want)
    a_f = 32 * 2.0 ** -24 * cond
    ang = cases.angle(got, want)
    print(f"{which}: largest angle {float(ang.max()):.3e} rad, A_q {a_q:.3e}, largest A_f {float(a_f.max()):.3e}, largest cond {float(cond.max()):.3f}")
    assert (ang <= a_q + a_f).all()
    # the header's own decode is the device's table entry: against the float64 decode of the same codes
    assert float(cases.angle(zsk.decode(posed[which]), got).max()) <= 16 * 2.0 ** -24      # (fewer than 16 roundings from the codes to the direction)
    return posed


def test_normals_against_float64(case):
    """n' = normalize(cof(M3) n), re-encoded: the decoded direction within A_q + A_f of the float64 restatement's, A_q the largest angle the oct32 round
    trip of the case's float64 normals produces, A_f = 32 * 2^-24 * cond(M3) per vertex; cond <= 4 and det > 0 checked on the float64 side"""
    _direction_stage(case, "normal")


def test_tangents_against_float64(case):
    """t' = normalize(M3 t), re-encoded: the same bar"""
    posed = _direction_stage(case, "tangent")
    assert np.array_equal(posed["uv"], np.zeros((N, 2), F32))


def test_uv_is_copied_and_identity_is_exact():
    rng = np.random.default_rng(4)
    v = np.zeros(64, wire.VERTEX)
    v["pos"], v["uv"] = rng.uniform(-3, 3, (64, 3)), rng.uniform(-1, 2, (64, 2))
    v["normal"] = v["tangent"] = zsk.encode(cases.directions(rng, 64))
    out = zsk.pose_vertex(v, np.tile(cases.IDENTITY, (64, 1)))
    assert out["uv"].tobytes() == v["uv"].tobytes() and out["pos"].tobytes() == v["pos"].tobytes()
    assert float(cases.angle(cases.decode_oct64(out["normal"]), cases.decode_oct64(v["normal"])).max()) <= 2 * cases.round_trip_angle(cases.decode_oct64(v["normal"])) + 32 * 2.0 ** -24


def test_chain_with_an_animated_middle_joint_and_a_static_leaf():
    """three joints root > middle > leaf, the middle one animated, the leaf static: the leaf's joint matrix follows its ancestor (what the loader's closure
    rule keeps the leaf in the table for), and the header's matrices equal float64 products of the node matrices and the inverse binds within gamma_3"""
    anim, joints = cases.joint_chain(3)
    assert [int(n) for n in anim.nodes["num_keys"]] == [0, 3, 0]
    skin = wire.SkinDesc(joints, np.zeros(0, wire.SKIN_RANGE), np.zeros(0, wire.SKIN_INFLUENCE))
    Js = []
    for t in (-1.0, 0.3, 0.9):
        world = cases.node_worlds(anim, t)
        J = zsk.eval_joint_matrices(skin, world)
        want, mag = cases.joint_matrix64(world, joints["inverse_bind"])
        assert (np.abs(J.astype(F64) - want) <= cases.gamma(3) * mag).all()
        Js.append(J)
    assert np.abs(Js[0] - np.tile(cases.IDENTITY, (3, 1))).max() <= 1e-5      # the bind pose: every joint matrix is the identity
    assert np.abs(Js[1][2] - Js[0][2]).max() > 1e-3 and np.abs(Js[2][2] - Js[1][2]).max() > 1e-3      # the static leaf moves with its parent
    assert np.array_equal(Js[1][0], Js[0][0])                                                           # the static root does not


def _tables(nj=4, nv=10):
    joints = np.zeros(nj, wire.SKIN_JOINT)
    joints["node"], joints["inverse_bind"] = np.arange(nj), cases.IDENTITY
    f = np.zeros(nv, wire.SKIN_INFLUENCE)
    f["joint"], f["weight"] = [0, 1, 2, 3], [0.25, 0.25, 0.25, 0.25]
    r = np.zeros(2, wire.SKIN_RANGE)
    r["first_vertex"], r["num_vertices"], r["first_influence"] = [3, 20], [5, 5], [0, 5]
    return joints, r, f


def test_what_the_setter_refuses():
    """zrsk::ValidateSkin, the check zr_scene_set_skinning runs before it touches anything: every refusal by its message, and the valid tables pass"""
    j, r, f = _tables()
    assert zsk.validate(wire.SkinDesc(j, r, f), 4, 25) is None

    def refused(edit, anim_nodes=4, verts=25):
        jj, rr, ff = _tables()
        edit(jj, rr, ff)
        return zsk.validate(wire.SkinDesc(jj, rr, ff), anim_nodes, verts)

    assert "node 3, the animation has 3" in refused(lambda j, r, f: None, anim_nodes=3)

    def joint_index(j, r, f): f["joint"][7, 2] = 4
    assert "influence 7: joint 4, the table has 4" in refused(joint_index)

    def overlap(j, r, f): r["first_vertex"][1] = 7
    assert "overlaps an earlier range at vertex 7" in refused(overlap)
    assert "vertices [20, 25), the scene has 24" in refused(lambda j, r, f: None, verts=24)

    def influence_range(j, r, f): r["first_influence"][1] = 6
    assert "influences [6, 11), the table has 10" in refused(influence_range)

    def weight(j, r, f): f["weight"][2, 1] = np.inf
    assert "influence 2: a weight is not finite" in refused(weight)

    def matrix(j, r, f): j["inverse_bind"][1, 5] = np.nan
    assert "joint 1: the inverse bind matrix is not finite" in refused(matrix)
    big = np.zeros(65536, wire.SKIN_JOINT)
    big["inverse_bind"] = cases.IDENTITY
    assert "65536 joints" in zsk.validate(wire.SkinDesc(big, r, f), 1, 25)
    assert zsk.validate(wire.SkinDesc(big[:65535], r[:0], f[:0]), 1, 25) is None


def test_wire_records_and_the_surface():
    """the records' sizes as zr_wire.h asserts them, the four entry points declared and listed, the translation unit in the build"""
    assert wire.SKIN_JOINT.itemsize == 52 and wire.SKIN_INFLUENCE.itemsize == 24 and wire.SKIN_RANGE.itemsize == 12
    import ctypes as C
    assert C.sizeof(wire.SkinDescC) == 48
    hdr = open(os.path.join(ROOT, "include", "zr_wire.h")).read()
    for rec, size in (("zr_skin_joint", 52), ("zr_skin_influence", 24), ("zr_skin_range", 12), ("zr_skin_desc", 48)):
        assert re.search(r"static_assert\(sizeof\(%s\) == %d" % (rec, size), hdr), rec
    from zetaray_amd import api
    names = {"zr_scene_update_vertices", "zr_scene_update_vertices_async", "zr_scene_get_vertices", "zr_scene_set_skinning"}
    assert names <= set(api.EXPORTS)
    L = api.lib()
    assert all(hasattr(L, n) for n in names)
    for m in ("update_vertices", "download_vertices", "set_skinning"):
        assert hasattr(api.Scene, m)
    assert hasattr(api.Renderer, "set_skinning")
    mk = open(os.path.join(ROOT, "zetaray_amd", "csrc", "Makefile")).read()
    assert "zr_tu_pose.o" in mk.split("OBJS :=")[1].split("\n")[0]


# ---------------------------------------------------------------------------------------------------------------- the loader (zrh_gltf_load: "skins", JOINTS_0, WEIGHTS_0)
@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    from zetaray_amd import scene_io
    path = cases.skinned_gltf(tmp_path_factory.mktemp("skin_gltf"))
    sc, _ = scene_io.load_gltf_native(path)
    import json
    return sc, json.load(open(path))


def test_loader_ranges_instances_and_the_closure(loaded):
    """tests/golden/skin_gltf: three skinned nodes, two of them sharing a mesh -- a vertex range of its own per node (equal bytes, different places), the
    instances at the identity (TubeA's translation ignored) and outside the animation's instance list; the closure keeps Rig (a static ancestor), Hip,
    Knee (animated) and Toe (a static leaf); the joint matrices at the bind pose are the identity, which holds the inverse bind matrices to the handedness
    rule of the nodes"""
    sc, g = loaded
    k, a = sc.skinning, sc.animation
    assert k is not None and a is not None and zsk.validate(k, len(a.nodes), len(sc.vertices)) is None
    tubes = [len(sc.instances) - 3 + i for i in range(3)]
    assert [int(r["num_vertices"]) for r in k.ranges] == [72, 72, 72]
    assert [int(r["first_vertex"]) for r in k.ranges] == [int(sc.instances["base_vtx_offset"][i]) for i in tubes]
    assert [int(r["first_influence"]) for r in k.ranges] == [0, 72, 144]
    assert len({int(r["first_vertex"]) for r in k.ranges}) == 3 and int(k.ranges["first_vertex"][2]) + 72 == len(sc.vertices)
    v = [sc.vertices[int(r["first_vertex"]):int(r["first_vertex"]) + 72] for r in k.ranges]
    assert v[0].tobytes() == v[1].tobytes() and v[0].tobytes() != v[2].tobytes()      # TubeA and TubeA2: one mesh, two ranges
    assert int(sc.instances["base_idx_offset"][tubes[0]]) == int(sc.instances["base_idx_offset"][tubes[1]])      # (the indices are mesh-local and shared)
    for i in tubes:
        assert sc.instance_to_world[i].tobytes() == cases.IDENTITY.tobytes() and i not in set(a.instance_idx.tolist())
        assert np.array_equal(sc.instances["translation"][i], np.zeros(3, F32))
    names = [n.get("name") for n in g["nodes"]]
    assert [names[j] for j in g["skins"][0]["joints"]] == ["Hip", "Knee", "Toe"]
    hip, knee, toe = (int(n) for n in k.joints["node"])
    assert int(a.nodes["parent"][toe]) == knee and int(a.nodes["parent"][knee]) == hip and int(a.nodes["num_keys"][knee]) == 4
    rig = int(a.nodes["parent"][hip])
    assert rig != wire.ANIM_ROOT and int(a.nodes["parent"][rig]) == wire.ANIM_ROOT and [int(a.nodes["num_keys"][n]) for n in (rig, hip, toe)] == [0, 0, 0]
    J = zsk.eval_joint_matrices(k, cases.node_worlds(a, -1.0))
    assert np.abs(J - cases.IDENTITY).max() <= 1e-6
    J = zsk.eval_joint_matrices(k, cases.node_worlds(a, 0.5))
    assert np.abs(J[0] - cases.IDENTITY).max() <= 1e-6 and np.abs(J[1] - cases.IDENTITY).max() > 0.05 and np.abs(J[2] - cases.IDENTITY).max() > 0.05


def test_loader_accessor_forms_and_renormalised_weights(loaded):
    """JOINTS_0 as unsigned bytes with float WEIGHTS_0 that sum to 0.5 (Tube) and as unsigned shorts with normalised-short weights (Tube16): the same
    influences within the 16-bit quantisation, every weight vector summing to 1 within 2 ulp after the float32 renormalisation"""
    sc, g = loaded
    f = sc.skinning.influences
    a, b = f[:72], f[144:]
    assert np.array_equal(a["joint"], b["joint"]) and np.array_equal(a["joint"], f[72:144]["joint"])
    assert np.abs(f["weight"].sum(1, dtype=np.float64) - 1).max() <= 2 * 2.0 ** -23
    assert np.abs(a["weight"] - b["weight"]).max() <= 2.0 / 65535 and a["weight"].tobytes() != b["weight"].tobytes()
    assert (a["weight"][::7] == F32([1, 0, 0, 0])).all() and ((a["weight"] > 0).sum(1) == 3).any() and int(a["joint"].max()) == 2
    acc = {n: g["accessors"][g["meshes"][-2]["primitives"][0]["attributes"][n]] for n in ("JOINTS_0", "WEIGHTS_0")}
    acc16 = {n: g["accessors"][g["meshes"][-1]["primitives"][0]["attributes"][n]] for n in ("JOINTS_0", "WEIGHTS_0")}
    assert (acc["JOINTS_0"]["componentType"], acc["WEIGHTS_0"]["componentType"]) == (5121, 5126)
    assert (acc16["JOINTS_0"]["componentType"], acc16["WEIGHTS_0"]["componentType"], acc16["WEIGHTS_0"].get("normalized")) == (5123, 5123, True)


def _refused(tmp_path, edit, blob_edit=None):
    from zetaray_amd import scene_io
    with pytest.raises(Exception) as e:
        scene_io.load_gltf_native(cases.skinned_gltf(tmp_path, edit=edit, blob_edit=blob_edit, name="bad"))
    return str(e.value)


def test_loader_refusals_by_name_and_reason(tmp_path):
    def prim(g, mesh=-2):
        return g["meshes"][mesh]["primitives"][0]

    def joint_not_a_node(g): g["skins"][0]["joints"][1] = len(g["nodes"])
    assert "skin 0 ('Leg'): joint 1 is not a node of the file" in _refused(tmp_path, joint_not_a_node)

    def no_weights(g): del prim(g)["attributes"]["WEIGHTS_0"]
    assert "JOINTS_0 without WEIGHTS_0" in _refused(tmp_path, no_weights)

    def no_joints(g): del prim(g, -1)["attributes"]["JOINTS_0"]
    assert "WEIGHTS_0 without JOINTS_0" in _refused(tmp_path, no_joints)

    def second_set(g): prim(g)["attributes"]["JOINTS_1"] = prim(g)["attributes"]["JOINTS_0"]
    assert "JOINTS_1 / WEIGHTS_1: more than four influences" in _refused(tmp_path, second_set)

    def emissive(g):
        prim(g)["material"] = next(i for i, m in enumerate(g["materials"]) if "emissiveFactor" in m or "KHR_materials_emissive_strength" in m.get("extensions", {}))
    assert "a skinned primitive with an emissive material" in _refused(tmp_path, emissive)

    def no_animation(g): del g["animations"]
    assert "a skin but no animation" in _refused(tmp_path, no_animation)

    def joint_outside_the_scene(g):
        knee = [n.get("name") for n in g["nodes"]].index("Knee")
        g["nodes"].append({"name": "Stray"})
        g["skins"][0]["joints"][2] = len(g["nodes"]) - 1
    assert "joint 2" in _refused(tmp_path, joint_outside_the_scene) and "not part of the scene's node hierarchy" in _refused(tmp_path, joint_outside_the_scene)

    def short_joint_list(g): g["skins"][0]["joints"] = g["skins"][0]["joints"][:2]
    assert "joint 2, the skin has 2" in _refused(tmp_path, short_joint_list)

    def skin_index(g): g["nodes"][-1]["skin"] = 3
    assert "names skin 3 but the file has 1" in _refused(tmp_path, skin_index)


PARENT_FIXTURE_SHA256 = {      # sha256 over the loaded arrays (fixture_hash below) of every glTF fixture, taken with the loader as it was before it read skins
    ("cornell.gltf", "decoded"): "08373c46cb863720136d09937148ee41d8ff658218e3d553c8333501f79b3e7a",
    ("cornell.gltf", "compressed"): "ae30f8bc6d303e3a374af4103b22e8262be29060bd2c4f27909be8722dfca2a1",
    ("cornell_emissive.gltf", "decoded"): "65ba79c1da882e0b2b74a60a2ff0192d8fe21c5f02142d23c39212cbdbcbdcce",
    ("cornell_emissive.gltf", "compressed"): "85c5686f3bd36c579c3920f3966ef81b5a4ca27738b812f2e9e8bf51a2b7bf8c",
    ("cornell_animated.gltf", "decoded"): "5d7dec8228098d3ba60b6c679c041f8ed5fb00e6a63d17dd9189ddaf63fb4915",
    ("cornell_animated.gltf", "compressed"): "ae6a5253a427f42341eec3dec79c82a81770b785159b1390661a050e3eb0b18d",
}


def fixture_hash(sc):
    import hashlib
    h = hashlib.sha256()
    for name in ("vertices", "indices", "instances", "instance_to_world", "instance_mask", "instance_num_tris", "materials", "emissives", "textures", "texels"):
        h.update(np.ascontiguousarray(getattr(sc, name)).tobytes())
    a = sc.animation
    if a is not None:
        for arr in (a.nodes, a.keys, a.instance_idx, a.instance_node, sc.emissives_initial):
            h.update(np.ascontiguousarray(arr).tobytes())
    return h.hexdigest()


def test_files_without_skins_load_exactly_as_before(tmp_path):
    """every glTF fixture of tests/golden/cornell_gltf, in both texture modes: the bytes the loader produced before it knew skins, and no skin tables"""
    import json
    from tests.animmath import cases as acases
    from zetaray_amd import scene_io
    acases.cornell_animated(tmp_path)
    for (name, mode), want in PARENT_FIXTURE_SHA256.items():
        g = json.load(open(os.path.join(acases.REF_GLTF, name)))
        (tmp_path / name).write_text(json.dumps(g))
        sc, _ = scene_io.load_gltf_native(str(tmp_path / name), textures=mode)
        assert fixture_hash(sc) == want, (name, mode)
        assert sc.skinning is None


def test_cpp_mirror_host_form_and_its_setter(tmp_path):
    """zrh_scene_data_skin_pose on the loaded fixture: the posed records of include/zr_skin.h compiled for the test, range after range, and not the rest
    pose; zrh_scene_data_set_skinning on a scene made from a desc: refused before an animation is set and for an invalid table, cleared by a new animation"""
    import ctypes as C
    from tests.animmath import cases as acases
    from zetaray_amd import scene_io
    path = cases.skinned_gltf(tmp_path)
    sc, _ = scene_io.load_gltf_native(path)
    L = acases.sio()
    L.zrh_scene_data_skin_pose.argtypes, L.zrh_scene_data_skin_pose.restype = [C.c_void_p, C.c_float], C.c_void_p
    L.zrh_scene_data_skinning.argtypes, L.zrh_scene_data_skinning.restype = [C.c_void_p], C.c_void_p
    L.zrh_scene_data_set_skinning.argtypes = [C.c_void_p, C.c_void_p]
    L.zrh_scene_data_device_skinning.argtypes = [C.c_void_p]
    host = acases.HostData.from_gltf(path)
    k, a = sc.skinning, sc.animation
    rest = cases.rest_of_ranges(k, sc.vertices)
    for t in (-0.5, 0.5, 1.25):
        p = L.zrh_scene_data_skin_pose(host.h, t)
        assert p
        got = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (len(rest) * wire.VERTEX.itemsize,)).view(wire.VERTEX).copy()
        assert got.tobytes() == cases.host_posed(a, k, rest, t).tobytes() == scene_io.skin_pose(a, k, rest, t).tobytes()
    assert got["pos"].tobytes() != rest["pos"].tobytes() and L.zrh_scene_data_device_skinning(host.h) == 0
    other = acases.HostData.from_scene(sc)
    assert not L.zrh_scene_data_skinning(other.h) and not L.zrh_scene_data_skin_pose(other.h, 0.5)
    d = k.c_desc()
    assert L.zrh_scene_data_set_skinning(other.h, C.addressof(d)) == -1 and b"no animation set" in L.zrh_scene_io_last_error()
    assert other.set_animation(a) == 0 and L.zrh_scene_data_set_skinning(other.h, C.addressof(d)) == 0 and L.zrh_scene_data_skinning(other.h)
    bad = wire.SkinDesc(k.joints, k.ranges, k.influences[:-1])
    bd = bad.c_desc()
    assert L.zrh_scene_data_set_skinning(other.h, C.addressof(bd)) == -1 and b"influences" in L.zrh_scene_io_last_error() and L.zrh_scene_data_skinning(other.h)
    p = L.zrh_scene_data_skin_pose(other.h, 0.5)
    assert np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (len(rest) * 28,)).tobytes() == cases.host_posed(a, k, rest, 0.5).tobytes()
    assert other.set_animation(a) == 0 and not L.zrh_scene_data_skinning(other.h)      # a new animation clears the skin, as on the device
    host.close(); other.close()
