"""Morph targets, the arithmetic of include/zr_morph.h on the host (tests/morphmath/libzmo.so): the weight sampling pinned to zran::SampleAnimation bit for
bit, MorphVertex against a float64 restatement within derived bounds, the bit-level rules (the zero-weight skip, untouched code words), the composition
with skinning, the tables zr_scene_set_morph refuses (zrmo::ValidateMorph) and the surface the feature adds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.morphmath import cases, zmo
from tests.skinmath import cases as scases
from tests.skinmath import zsk
from zetaray_amd import scene_io, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
U = 2.0 ** -24
N = 512


# ---------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("nk", [2, 3, 17])
@pytest.mark.parametrize("loop", [0, 1])
@pytest.mark.parametrize("t0", [0.0, 0.3125, -1.7])
def test_weight_sampling_equals_the_animations(nk, loop, t0):
    """SampleWeights restates zran::SampleAnimation's control flow over a plain array of times: every weight equals, to the bit, the translation.x of a
    keyframe track with the same times that carries the weight values -- before the first key, on every key, between keys, on the last key, beyond it
    (whole periods later too, where the loop wrap can land on the last key and FindInterval's clamp to numKeys - 2 applies) and at random times"""
    rng = np.random.default_rng(100 * nk + 10 * loop + int(abs(t0) * 16))
    times = np.cumsum(rng.uniform(0.05, 0.6, nk)).astype(F32)
    T = 4
    values = rng.uniform(-0.5, 1.5, (nk, T)).astype(F32)
    values[nk // 2, 1] = 0.0
    period = float(times[-1]) - float(times[0])
    ts = [float(times[0]) + t0 - 1.0, float(times[0]) + t0 - 1e-6]
    ts += [float(F32(tk) + F32(t0)) for tk in times]                                         # on the keys (where t - t0 gives the key time back, and near it)
    ts += [float(times[0]) + t0 + period * k for k in (1, 2, 3, 7, 100)]                    # whole periods: the wrap's end points
    ts += [float(np.nextafter(F32(times[-1] + F32(t0)), F32(np.inf))), float(times[-1]) + t0 + 0.37, float(times[-1]) + t0 + 5.0 * period + 0.01]
    ts += list(rng.uniform(float(times[0]) + t0 - 0.5, float(times[0]) + t0 + 4 * period, 400))
    clamped = 0
    for t in ts:
        got = zmo.sample_weights(times, values, t0, loop, t)
        want = np.array([zmo.sample_animation_tx(times, values[:, k], t0, loop, t) for k in range(T)], F32)
        assert got.tobytes() == want.tobytes(), (t, got, want)
        u = F32(t) - F32(t0)
        if u <= times[0]:
            assert got.tobytes() == values[0].tobytes()
        if not loop and u >= times[-1]:
            assert got.tobytes() == values[-1].tobytes()
            clamped += 1
    assert clamped >= 3 or loop


def test_a_track_without_keys_yields_its_rest_weights():
    m = cases.morph_set([(0, 4, 0), (4, 4, 1)], [cases.static_track([0.25, -0.0, 1.5]), cases.keyed_track(np.random.default_rng(1), 2)])
    for t in (-1.0, 0.3, 9.0):
        W = zmo.eval_weights(m, t)
        assert W[:3].tobytes() == F32([0.25, -0.0, 1.5]).tobytes()      # unchanged, the sign of the zero included
        assert W[3:].tobytes() == zmo.sample_weights(m.times, m.values.reshape(3, 2), 0.0, 0, t).tobytes()


# ---------------------------------------------------------------------------------------------------------------- one vertex against float64
def _vertex_case(T, lacks, seed, wscale=1.5):
    rng = np.random.default_rng(seed)
    rest = np.zeros(N, wire.VERTEX)
    rest["pos"], rest["uv"] = rng.uniform(-2, 2, (N, 3)), rng.uniform(-1, 2, (N, 2))
    rest["normal"] = zsk.encode(scases.directions(rng, N))
    rest["tangent"] = zsk.encode(scases.directions(rng, N)[::-1])
    m = cases.morph_set([(0, N, 0)], [cases.static_track(np.zeros(T))], lacks=lacks, seed=seed)
    w = rng.uniform(-wscale, wscale, T).astype(F32)
    return rest, m, w


@pytest.mark.parametrize("T,lacks", [(1, [0]), (2, [0, 1]), (5, [0, 1, 2, 3]), (9, [0, 0, 2, 1]), (16, [0])])
def test_morph_vertex_against_float64(T, lacks):
    """MorphVertex (float32, the header) against cases.morph64 (float64 on the same float32 inputs).

    Positions: acc <- fma(w_k, d_k, acc) is one rounding per applied target, so with T' applied targets every component is within
    gamma_T' * (|p_c| + sum_k |w_k| |d_k,c|) (the rest value passes through all T' roundings, term k through T' - k + 1).

    Normals and tangents, by angle between the decoded stored codes and the float64 direction: A_q + c * 2^-24 * (1 + S) / |acc|, S = sum_k |w_k| |d_k|
    (Euclidean), |acc| the length of the float64 sum, A_q the largest angle the oct32 round trip of the case's float64 directions produces (the allowance
    of tests/test_skin_cpu.py).  c, with u = 2^-24:
      * the float32 decode of the rest codes is within 16 u of the float64 decode by angle (the bar test_skin_cpu.py holds zsk.decode to) and 4.5 u in
        length (dot: gamma_3, halved by the square root; sqrt, divide, multiply one rounding each): a vector error of at most 21 u on a unit vector;
      * the fma chain adds at most gamma_T' (|n_c| + sum |w| |d_c|) per component, T' u (1 + S) in Euclidean length;
      * so the sum is off by at most (21 + T') (1 + S) u, an angle of at most 1.01 (21 + T') (1 + S) u / |acc| while that is small;
      * Normalize3 scales all components by one factor; only the final multiply rounds per component: 2 u;
      * EncodeOct32 in float32 (a divide by the L1 length, the fold, scale and offset: fewer than 5 roundings in coordinates whose stretch to angle is
        below 2) moves the value that is then rounded to a code by 10 u at most: beyond A_q, which already holds the half step of the rounding;
      * 12 u <= 12 u (1 + S) / |acc| since |acc| <= 1 + S.  Total c = 1.01 (21 + T') + 12 <= 36 + T' for T' <= 16.
    Precondition, asserted in float64 on every vertex: |acc| >= 0.25"""
    rest, m, w = _vertex_case(T, lacks, 40 + T)
    got = zmo.morph_vertices(rest, m.targets, w, m.deltas)
    ref = cases.morph64(rest, m.targets, w, m.deltas)
    Ta = ref["applied"]
    assert Ta == T
    err = np.abs(got["pos"].astype(F64) - ref["pos"])
    bound = cases.gamma(Ta) * ref["pos_mag"]
    print(f"T = {T}: positions: largest error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert got["uv"].tobytes() == rest["uv"].tobytes()
    for a in ("normal", "tangent"):
        if not ref[a + "_applied"]:
            assert got[a].tobytes() == rest[a].tobytes()
            continue
        length = np.linalg.norm(ref[a], axis=1)
        assert (length >= 0.25).all(), float(length.min())
        want = scases.unit(ref[a])
        a_q = scases.round_trip_angle(want)
        allow = a_q + (36 + Ta) * U * (1 + ref[a + "_mag"]) / length
        ang = scases.angle(scases.decode_oct64(got[a]), want)
        print(f"T = {T}: {a}: largest angle {float(ang.max()):.3e} rad, A_q {a_q:.3e}, largest angle / allowance {float((ang / allow).max()):.3f}, smallest |acc| {float(length.min()):.3f}")
        assert (ang <= allow).all()
        assert (got[a] != rest[a]).any()


# ---------------------------------------------------------------------------------------------------------------- bit-level rules
def test_zero_weights_return_the_rest_bytes_and_minus_zero_is_zero():
    """all weights zero: the rest record's bytes (the code words are copied: a decode + encode round trip need not give them back); a -0 weight
    behaves as +0, on its own and among applied targets"""
    rest, m, w = _vertex_case(5, [0, 1, 2, 3], 7)
    for zeros in (np.zeros(5, F32), -np.zeros(5, F32), F32([0, -0.0, 0, -0.0, 0])):
        assert zmo.morph_vertices(rest, m.targets, zeros, m.deltas).tobytes() == rest.tobytes()
    trip = zsk.encode(zsk.decode(rest["normal"]))
    print(f"oct32 round trip moves {int((trip != rest['normal']).any(1).sum())} of {N} code pairs")
    plus, minus = w.copy(), w.copy()
    plus[[1, 3]], minus[[1, 3]] = 0.0, -0.0
    assert zmo.morph_vertices(rest, m.targets, plus, m.deltas).tobytes() == zmo.morph_vertices(rest, m.targets, minus, m.deltas).tobytes()
    # ... and equals the set without targets 1 and 3
    keep = [0, 2, 4]
    assert zmo.morph_vertices(rest, m.targets[keep], w[keep], m.deltas).tobytes() == zmo.morph_vertices(rest, m.targets, plus, m.deltas).tobytes()


def test_targets_without_normal_deltas_keep_the_code_words():
    """a vertex whose APPLIED targets all lack NORMAL keeps its normal code words (a target that has them but a zero weight does not count); likewise the
    tangent; the position moves all the same"""
    rest, m, w = _vertex_case(4, [cases.LACK_NONE, cases.LACK_NRM, cases.LACK_TAN, cases.LACK_BOTH], 9)
    only = lambda ks: F32([w[k] if k in ks else 0.0 for k in range(4)])
    a = zmo.morph_vertices(rest, m.targets, only({1, 3}), m.deltas)
    assert a["normal"].tobytes() == rest["normal"].tobytes() and (a["tangent"] != rest["tangent"]).any() and (a["pos"] != rest["pos"]).all(1).any()
    b = zmo.morph_vertices(rest, m.targets, only({2, 3}), m.deltas)
    assert b["tangent"].tobytes() == rest["tangent"].tobytes() and (b["normal"] != rest["normal"]).any()
    c = zmo.morph_vertices(rest, m.targets, only({3}), m.deltas)
    assert c["normal"].tobytes() == rest["normal"].tobytes() and c["tangent"].tobytes() == rest["tangent"].tobytes() and (c["pos"] != rest["pos"]).any()


def test_skipping_a_zero_weight_matters():
    """the constructed case: a rest coordinate of -0.0 under a zero weight.  fma(0, d, -0.0) is +0.0 -- applying the target would flip the sign bit -- so the
    skip is part of the definition: the record keeps -0.0"""
    rest = np.zeros(1, wire.VERTEX)
    rest["pos"] = F32([-0.0, 1.0, -0.0])
    rest["normal"] = rest["tangent"] = zsk.encode([[0, 0, 1]])
    targets = np.array([(0, wire.MORPH_NONE, wire.MORPH_NONE)], wire.MORPH_TARGET)
    deltas = F32([[3.0, 2.0, 5.0]])
    applied = F32(0.0) * deltas[0] + rest["pos"][0]      # what the fma would give: the products are exact zeros
    assert applied.tobytes() == F32([0.0, 1.0, 0.0]).tobytes() and applied.tobytes() != rest["pos"].tobytes()
    for zero in (0.0, -0.0):
        assert zmo.morph_vertices(rest, targets, F32([zero]), deltas).tobytes() == rest.tobytes()


# ---------------------------------------------------------------------------------------------------------------- with skinning
def _morph_and_skin():
    """a tube of the skinning tests: one range morphed and skinned, one morphed only, over 5 joints"""
    rng = np.random.default_rng(5)
    verts, _ = scases.tube(rng)
    anim, joints = scases.joint_chain(5)
    infl = scases.tube_influences(verts[:300], 5, rng)
    skin = wire.SkinDesc(joints, np.array([(0, 300, 0)], wire.SKIN_RANGE), infl)
    morph = cases.morph_set([(0, 300, 0), (400, 77, 1)], [cases.keyed_track(rng, 3, loop=1), cases.keyed_track(rng, 2, zero_at=[(1, 0)])], lacks=[0, 1, 2])
    return verts, anim, skin, morph


def test_morph_then_skin_is_the_composition():
    """the host form of a morphed and skinned range is zrh_morph_pose for the morph alone followed by zrh_skin_pose on its output -- the morphed record with
    its ENCODED words is the rest record the skin takes; the morph-only range is untouched by the skin; tests/morphmath's compilation of the header agrees"""
    verts, anim, skin, morph = _morph_and_skin()
    rest = cases.rest_of_ranges(morph, verts)
    for t in (-0.5, 0.5, 0.8125, 2.125):
        both = scene_io.morph_pose(anim, skin, morph, rest, t)
        morphed = scene_io.morph_pose(None, None, morph, rest, t)
        want = morphed.copy()
        want[:300] = scene_io.skin_pose(anim, skin, morphed[:300], t)
        assert both.tobytes() == want.tobytes()
        assert both[300:].tobytes() == morphed[300:].tobytes() and (both[:300]["pos"] != morphed[:300]["pos"]).any()
        J = zsk.eval_joint_matrices(skin, scases.node_worlds(anim, t))
        assert zmo.morph_ranges(morph, zmo.eval_weights(morph, t), rest, skin, J).tobytes() == both.tobytes()
        assert zmo.morph_ranges(morph, zmo.eval_weights(morph, t), rest).tobytes() == morphed.tobytes()
    assert (scene_io.morph_pose(None, None, morph, rest, 0.8125)["pos"] != rest["pos"]).any()


# ---------------------------------------------------------------------------------------------------------------- what the setter refuses
def test_what_the_setter_refuses():
    """zrmo::ValidateMorph, one case per refusal zr_scene_set_morph lists, each with its own message; the good set passes"""
    verts, anim, skin, good = _morph_and_skin()
    nv = len(verts)
    assert zmo.validate(good, skin, nv) is None and zmo.validate(good, None, nv) is None

    def bad(edit):
        parts = {k: getattr(good, k).copy() for k in ("tracks", "targets", "ranges", "times", "values", "rest_weights", "deltas")}
        edit(parts)
        return wire.MorphDesc(**parts)

    def past_scene(p): p["ranges"]["first_vertex"][1] = nv - 76
    def past_deltas(p): p["targets"]["first_nrm"][0] = len(good.deltas) - 299
    def past_targets(p): p["ranges"]["first_target"][1] = len(good.targets) - 1
    def overlap(p): p["ranges"]["first_vertex"][1] = 299
    def meets_skin(p): p["ranges"]["num_vertices"][0] = 299
    def target_count(p): p["ranges"]["num_targets"][1] = 1
    def one_key(p): p["tracks"]["num_keys"][1] = 1
    def time_nan(p): p["times"][1] = np.nan
    def time_order(p): p["times"][4] = p["times"][3]
    def weight_inf(p): p["values"][2] = np.inf
    def t0_nan(p): p["tracks"]["t0"][0] = np.nan
    def delta_nan(p): p["deltas"][17, 1] = np.nan
    def no_track(p): p["ranges"]["track"][0] = 2
    def past_times(p): p["tracks"]["first_key"][1] = len(good.times) - 2
    def past_values(p): p["tracks"]["first_value"][1] = len(good.values) - 5

    for edit, sk, word in ((past_scene, None, "the scene has"), (past_deltas, None, "deltas ["), (past_targets, None, "targets ["), (overlap, None, "overlaps an earlier range"),
                           (meets_skin, skin, "meets skin range 0 without being equal"), (target_count, None, "1 targets, its track 1 has 2"), (one_key, None, "num_keys == 1"),
                           (time_nan, None, "time is not finite"), (time_order, None, "not strictly increasing"), (weight_inf, None, "a weight is not finite"),
                           (t0_nan, None, "t0 is not finite"), (delta_nan, None, "delta 17"), (no_track, None, "track 2, the table has 2"),
                           (past_times, None, "key times ["), (past_values, None, "values [")):
        msg = zmo.validate(bad(edit), sk, nv)
        assert msg is not None and word in msg, (edit.__name__, msg)
    assert zmo.validate(bad(meets_skin), None, nv) is None      # (without the skin set, the same ranges are fine)
    static = cases.morph_set([(0, 8, 0)], [cases.static_track([0.5, np.nan])])
    assert "a rest weight is not finite" in zmo.validate(static, None, nv)
    static.tracks["first_rest"][0] = 1
    assert "rest weights [" in zmo.validate(static, None, nv)
    for name in ("tracks", "targets", "ranges", "times", "values", "deltas"):
        d = good.c_desc()
        setattr(d, name, None)
        assert zmo.validate(good, None, nv, c_desc=d) == "null table with a non-zero count", name


def test_wire_records_and_the_surface():
    """the numpy dtypes against the C records' static_asserts, and the declarations the feature adds"""
    wireh = open(os.path.join(ROOT, "include", "zr_wire.h")).read()
    for name, size in (("zr_morph_track", wire.MORPH_TRACK.itemsize), ("zr_morph_target", wire.MORPH_TARGET.itemsize), ("zr_morph_range", wire.MORPH_RANGE.itemsize),
                       ("zr_morph_desc", C.sizeof(wire.MorphDescC))):
        assert re.search(rf"static_assert\(sizeof\({name}\) == {size},", wireh), name
    assert re.search(r"#define ZR_MORPH_NONE 0xffffffffu", wireh) and wire.MORPH_NONE == 0xffffffff
    api = open(os.path.join(ROOT, "include", "zetaray_amd.h")).read()
    assert "int zr_scene_set_morph(zr_scene* scene, const zr_morph_desc* desc);" in api and "int zr_scene_has_morph(const zr_scene* scene);" in api
    mk = open(os.path.join(ROOT, "zetaray_amd", "csrc", "Makefile")).read()
    assert "zr_tu_pose.o" in mk.split("OBJS :=")[1].split("\n")[0]


# ---------------------------------------------------------------------------------------------------------------- the loader
@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    import json
    d = tmp_path_factory.mktemp("morph_gltf")
    path = cases.morphed_gltf(d)
    sc, _ = scene_io.load_gltf_native(path)
    return sc, json.load(open(path)), d


def _file_array(g, blob, acc_index):
    """an accessor of the fixture's own buffer as float64 (dense float, strided normalised, or sparse), in the file's handedness"""
    a = g["accessors"][acc_index]
    n, comp = a["count"], a["componentType"]
    dt = {5126: np.float32, 5122: np.int16, 5120: np.int8, 5123: np.uint16}[comp]

    def read(view_index, offset, count, dtype, ncomp):
        bv = g["bufferViews"][view_index]
        assert bv["buffer"] == len(g["buffers"]) - 1
        stride = bv.get("byteStride", np.dtype(dtype).itemsize * ncomp)
        start = bv.get("byteOffset", 0) + offset
        rows = [np.frombuffer(blob, dtype, ncomp, start + i * stride) for i in range(count)]
        return np.array(rows, np.float64).reshape(count, ncomp)

    out = np.zeros((n, 3))
    if "bufferView" in a:
        out = read(a["bufferView"], a.get("byteOffset", 0), n, dt, 3)
        if a.get("normalized"):
            out = np.maximum(out / {5122: 32767.0, 5120: 127.0}[comp], -1.0)
    if "sparse" in a:
        sp = a["sparse"]
        idx = read(sp["indices"]["bufferView"], sp["indices"].get("byteOffset", 0), sp["count"], np.uint16, 1).astype(np.int64).reshape(-1)
        out[idx] = read(sp["values"]["bufferView"], sp["values"].get("byteOffset", 0), sp["count"], np.float32, 3)
    return out


def test_loader_tables_z_negation_and_accessor_forms(loaded):
    """tests/golden/morph_gltf: two tracks (the tube's, visited first, and the face's) on different input accessors; the tube's range is the skin's range
    (one range listed in both tables), the face's a copy of its own; the instance of the face, a node with no animated transform, is in the animation's
    list; every delta array equals the file's with z negated -- the dense floats, the sparse ones (over zeros and over a base), the normalised shorts
    and bytes; rest weights are the node's, which override the mesh's"""
    sc, g, d = loaded
    m, k, a = sc.morph, sc.skinning, sc.animation
    assert m is not None and k is not None and a is not None and zmo.validate(m, k, len(sc.vertices)) is None
    blob = open(os.path.join(str(d), "morph.bin"), "rb").read()
    assert [tuple(int(x) for x in r) for r in m.ranges[["num_vertices", "first_target", "num_targets", "track"]].tolist()] == [(72, 0, 2, 0), (42, 2, 5, 1)]
    assert (int(m.ranges["first_vertex"][0]), int(m.ranges["num_vertices"][0])) == (int(k.ranges["first_vertex"][0]), int(k.ranges["num_vertices"][0]))
    face_first = int(m.ranges["first_vertex"][1])
    assert face_first + 42 == len(sc.vertices) and int(sc.instances["base_vtx_offset"][-1]) == face_first
    assert len(sc.instances) - 1 in set(a.instance_idx.tolist()) and len(sc.instances) - 2 not in set(a.instance_idx.tolist())      # the face moves as an instance, the skinned tube does not
    assert m.times.tolist() == [0.0, 0.75, 1.5, 0.0, 0.6000000238418579, 1.399999976158142]
    assert [tuple(int(x) for x in t) for t in m.tracks[["num_targets", "first_key", "num_keys", "first_value", "first_rest", "loop"]].tolist()] == [(2, 0, 3, 0, 0, 1), (5, 3, 3, 6, 2, 1)]
    assert m.rest_weights.tolist() == [0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0]
    v = m.values[6:].reshape(3, 5)
    assert (v == 0).any() and (v < 0).any() and (v > 1).any()
    names = ("POSITION", "NORMAL", "TANGENT")
    for mesh, first_target, nv in ((g["meshes"][-1], 0, 72), (g["meshes"][-2], 2, 42)):
        for t, tg in enumerate(mesh["primitives"][0]["targets"]):
            rec = m.targets[first_target + t]
            for f, nm in zip(("first_pos", "first_nrm", "first_tan"), names):
                if nm not in tg:
                    assert int(rec[f]) == wire.MORPH_NONE
                    continue
                want = _file_array(g, blob, tg[nm]) * np.array([1.0, 1.0, -1.0])
                got = m.deltas[int(rec[f]):int(rec[f]) + nv]
                assert got.tobytes() == want.astype(F32).tobytes(), (mesh["name"], t, nm)
    face_t = g["meshes"][-2]["primitives"][0]["targets"]
    assert "NORMAL" not in face_t[1] and "TANGENT" not in face_t[2] and "sparse" in g["accessors"][face_t[3]["POSITION"]] and "bufferView" not in g["accessors"][face_t[3]["POSITION"]]
    assert g["accessors"][face_t[4]["POSITION"]]["componentType"] == 5122 and g["accessors"][face_t[4]["NORMAL"]]["componentType"] == 5120


def test_sparse_targets_equal_their_dense_equivalent(loaded, tmp_path):
    """the face's sparse target rewritten as dense float accessors holding the same values: every table the loader makes is the same bytes"""
    sc, g0, d = loaded

    def densify(blob, g):
        tg = g["meshes"][-2]["primitives"][0]["targets"][3]
        for nm in ("POSITION", "NORMAL"):
            dense = _file_array(g, bytes(blob), tg[nm]).astype(np.float32)
            while len(blob) % 4:
                blob += b"\0"
            g["bufferViews"].append({"buffer": len(g["buffers"]) - 1, "byteOffset": len(blob), "byteLength": dense.nbytes})
            g["accessors"].append({"bufferView": len(g["bufferViews"]) - 1, "componentType": 5126, "count": len(dense), "type": "VEC3"})
            tg[nm] = len(g["accessors"]) - 1
            blob += dense.tobytes()
        return blob

    dense, _ = scene_io.load_gltf_native(cases.morphed_gltf(tmp_path, blob_edit=densify, name="dense"))
    for name in ("tracks", "targets", "ranges", "times", "values", "rest_weights", "deltas"):
        assert getattr(dense.morph, name).tobytes() == getattr(sc.morph, name).tobytes(), name
    assert dense.vertices.tobytes() == sc.vertices.tobytes()


def test_default_weights_are_baked_without_a_channel_and_a_weights_only_animation_sets_one(loaded, tmp_path):
    """the face's weights channel removed: no range of the set is the face's, and its vertices -- still a copy of the node's own -- are MorphVertex of the
    rest copy at the node's weights, which override the mesh's; without the node's weights the mesh's apply.  All channels but the weights channels
    removed: the file still has an animation to set, with the face's node in it"""
    sc, g0, d = loaded
    face_first = int(sc.morph.ranges["first_vertex"][1])
    rest = sc.vertices[face_first:face_first + 42]
    targets = sc.morph.targets[2:7].copy()

    def no_channel(g):
        a = g["animations"][0]
        face = [n.get("name") for n in g["nodes"]].index("Face", 11)
        a["channels"] = [c for c in a["channels"] if not (c["target"]["path"] == "weights" and c["target"]["node"] == face)]

    def mesh_weights_only(g):
        no_channel(g)
        del g["nodes"][[n.get("name") for n in g["nodes"]].index("Face", 11)]["weights"]

    for edit, w in ((no_channel, [0.0, 0.25, 0.0, 0.0, 0.0]), (mesh_weights_only, [0.1, 0.0, 0.0, 0.0, 0.2])):
        baked, _ = scene_io.load_gltf_native(cases.morphed_gltf(tmp_path, edit=edit, name="baked"))
        assert len(baked.morph.ranges) == 1 and int(baked.morph.ranges["num_vertices"][0]) == 72 and len(baked.morph.targets) == 2
        assert len(baked.vertices) == len(sc.vertices)
        got = baked.vertices[face_first:face_first + 42]
        want = zmo.morph_vertices(rest, targets, F32(w), sc.morph.deltas)
        assert got.tobytes() == want.tobytes() != rest.tobytes()

    def weights_only(g):
        a = g["animations"][0]
        a["channels"] = [c for c in a["channels"] if c["target"]["path"] == "weights"]

    only, _ = scene_io.load_gltf_native(cases.morphed_gltf(tmp_path, edit=weights_only, name="weights_only"))
    assert only.animation is not None and only.morph is not None and len(only.morph.ranges) == 2
    assert int(only.animation.nodes["num_keys"].sum()) == 0 and len(only.instances) - 1 in set(only.animation.instance_idx.tolist())
    assert only.morph.deltas.tobytes() == sc.morph.deltas.tobytes()


def _refused(tmp_path, edit=None, blob_edit=None):
    with pytest.raises(Exception) as e:
        scene_io.load_gltf_native(cases.morphed_gltf(tmp_path, edit=edit, blob_edit=blob_edit, name="bad"))
    return str(e.value)


def test_loader_refusals_by_name_and_reason(tmp_path):
    import copy

    def face(g): return g["meshes"][-2]
    def face_node(g): return [n.get("name") for n in g["nodes"]].index("Face", 11)
    def face_sampler(g):
        a = g["animations"][0]
        return a["samplers"][next(c["sampler"] for c in a["channels"] if c["target"]["path"] == "weights" and c["target"]["node"] == face_node(g))]

    def target_counts(g):
        p = copy.deepcopy(face(g)["primitives"][0])
        p["targets"] = p["targets"][:4]
        face(g)["primitives"].append(p)
    msg = _refused(tmp_path, target_counts)
    assert "mesh" in msg and "'Face'" in msg and "different morph target counts (5 and 4)" in msg

    def mesh_weights(g): face(g)["weights"] = [0.0] * 4
    assert "a weights array of 4 entries, the mesh has 5 morph targets" in _refused(tmp_path, mesh_weights)

    def node_weights(g): g["nodes"][face_node(g)]["weights"] = [0.0] * 6
    assert "a weights array of 6 entries, its mesh has 5 morph targets" in _refused(tmp_path, node_weights)

    def short_target(g): g["accessors"][face(g)["primitives"][0]["targets"][1]["TANGENT"]]["count"] = 41
    msg = _refused(tmp_path, short_target)
    assert "target 1 TANGENT" in msg and "target accessor shorter than POSITION" in msg

    for interp in ("CUBICSPLINE", "STEP"):
        def sampler(g, interp=interp): face_sampler(g)["interpolation"] = interp
        msg = _refused(tmp_path, sampler)
        assert f"target path 'weights': {interp} samplers are not supported (LINEAR is)" in msg and "node 16" in msg

    def emissive(g):
        face(g)["primitives"][0]["material"] = next(i for i, m in enumerate(g["materials"]) if "emissiveFactor" in m or "KHR_materials_emissive_strength" in m.get("extensions", {}))
    assert "a morphed primitive with an emissive material" in _refused(tmp_path, emissive)

    def no_targets(g): del face(g)["primitives"][0]["targets"], face(g)["weights"], g["nodes"][face_node(g)]["weights"]
    msg = _refused(tmp_path, no_targets)
    assert "target path 'weights': the node's mesh has no morph targets" in msg and "node 16" in msg and "animation 0" in msg

    def few_values(g): g["accessors"][face_sampler(g)["output"]]["count"] = 14
    assert "do not match the weights path (a SCALAR output of keys x 5 targets)" in _refused(tmp_path, few_values)

    def sparse_index(blob, g):
        sp = g["accessors"][g["meshes"][-2]["primitives"][0]["targets"][3]["POSITION"]]["sparse"]
        off = g["bufferViews"][sp["indices"]["bufferView"]]["byteOffset"]
        blob[off + 2:off + 4] = np.uint16(42).tobytes()
        return blob
    assert "sparse index 42 out of range: the accessor has 42 elements" in _refused(tmp_path, blob_edit=sparse_index)

    def sparse_view(g):
        sp = g["accessors"][face(g)["primitives"][0]["targets"][3]["NORMAL"]]["sparse"]
        sp["count"] = 4000
    assert "sparse accessor reads past its buffer" in _refused(tmp_path, sparse_view)

    def byte_type(g): g["accessors"][face(g)["primitives"][0]["targets"][4]["NORMAL"]]["normalized"] = False
    assert "a target attribute must be VEC3 of floats, or of normalised bytes / shorts" in _refused(tmp_path, byte_type)


PARENT_FIXTURE_SHA256 = {      # sha256 over the loaded arrays (fixture_hash below) of every glTF fixture, taken with the loader as it was before it read morph targets
    ("cornell.gltf", "decoded"): "08373c46cb863720136d09937148ee41d8ff658218e3d553c8333501f79b3e7a",
    ("cornell.gltf", "compressed"): "ae30f8bc6d303e3a374af4103b22e8262be29060bd2c4f27909be8722dfca2a1",
    ("cornell_emissive.gltf", "decoded"): "65ba79c1da882e0b2b74a60a2ff0192d8fe21c5f02142d23c39212cbdbcbdcce",
    ("cornell_emissive.gltf", "compressed"): "85c5686f3bd36c579c3920f3966ef81b5a4ca27738b812f2e9e8bf51a2b7bf8c",
    ("cornell_animated.gltf", "decoded"): "5d7dec8228098d3ba60b6c679c041f8ed5fb00e6a63d17dd9189ddaf63fb4915",
    ("cornell_animated.gltf", "compressed"): "ae6a5253a427f42341eec3dec79c82a81770b785159b1390661a050e3eb0b18d",
    ("cornell_skinned.gltf", "decoded"): "e0336c46ccfed645e45a0d483b9e3ebb0088a346f46355574dd2eed48d942d39",
    ("cornell_skinned.gltf", "compressed"): "aed8c0870ea694da658eb3074b3d12a471884cde8bb01480619c127819860857",
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
    k = sc.skinning
    if k is not None:
        for arr in (k.joints, k.ranges, k.influences):
            h.update(np.ascontiguousarray(arr).tobytes())
    return h.hexdigest()


def test_files_without_targets_load_exactly_as_before(tmp_path):
    """every glTF fixture without morph targets, the skinned one included, in both texture modes: the bytes the loader produced before it knew targets, and no morph tables"""
    import json
    from tests.animmath import cases as acases
    scases.skinned_gltf(tmp_path)
    for (name, mode), want in PARENT_FIXTURE_SHA256.items():
        if name != "cornell_skinned.gltf":
            g = json.load(open(os.path.join(acases.REF_GLTF, name)))
            (tmp_path / name).write_text(json.dumps(g))
        sc, _ = scene_io.load_gltf_native(str(tmp_path / name), textures=mode)
        assert fixture_hash(sc) == want, (name, mode)
        assert sc.morph is None


def test_cpp_mirror_host_form_and_its_setter(loaded, tmp_path):
    """zrh_scene_data_morph_pose on the loaded fixture: the posed records of zrh_morph_pose on the loader's tables (the tube morphed, then skinned), and not
    the rest pose; zrh_scene_data_set_morph on a scene made from a desc: refused before an animation is set and for an invalid table, cleared by a new
    skin set and by a new animation, as on the device"""
    from tests.animmath import cases as acases
    sc, g, d = loaded
    L = acases.sio()
    L.zrh_scene_data_morph_pose.argtypes, L.zrh_scene_data_morph_pose.restype = [C.c_void_p, C.c_float], C.c_void_p
    L.zrh_scene_data_morph.argtypes, L.zrh_scene_data_morph.restype = [C.c_void_p], C.c_void_p
    L.zrh_scene_data_set_morph.argtypes = [C.c_void_p, C.c_void_p]
    L.zrh_scene_data_set_skinning.argtypes = [C.c_void_p, C.c_void_p]
    L.zrh_scene_data_device_morph.argtypes = [C.c_void_p]
    host = acases.HostData.from_gltf(os.path.join(str(d), "cornell_morphed.gltf"))
    m, k, a = sc.morph, sc.skinning, sc.animation
    rest = cases.rest_of_ranges(m, sc.vertices)

    def posed(h, t):
        p = L.zrh_scene_data_morph_pose(h, t)
        assert p, L.zrh_scene_io_last_error()
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (len(rest) * wire.VERTEX.itemsize,)).view(wire.VERTEX).copy()

    for t in (-0.5, 0.6, 1.0, 2.125):
        got = posed(host.h, t)
        assert got.tobytes() == scene_io.morph_pose(a, k, m, rest, t).tobytes()
        J = zsk.eval_joint_matrices(k, scases.node_worlds(a, t))
        assert got.tobytes() == zmo.morph_ranges(m, zmo.eval_weights(m, t), rest, k, J).tobytes()
    assert posed(host.h, 1.0)["pos"].tobytes() != rest["pos"].tobytes() and L.zrh_scene_data_device_morph(host.h) == 0
    other = acases.HostData.from_scene(sc)
    assert not L.zrh_scene_data_morph(other.h) and not L.zrh_scene_data_morph_pose(other.h, 0.5)
    md, kd = m.c_desc(), k.c_desc()
    assert L.zrh_scene_data_set_morph(other.h, C.addressof(md)) == -1 and b"no animation set" in L.zrh_scene_io_last_error()
    assert other.set_animation(a) == 0 and L.zrh_scene_data_set_skinning(other.h, C.addressof(kd)) == 0
    assert L.zrh_scene_data_set_morph(other.h, C.addressof(md)) == 0 and L.zrh_scene_data_morph(other.h)
    bad = wire.MorphDesc(m.tracks, m.targets, m.ranges, m.times, m.values, m.rest_weights, m.deltas[:-1])
    bd = bad.c_desc()
    assert L.zrh_scene_data_set_morph(other.h, C.addressof(bd)) == -1 and b"deltas [" in L.zrh_scene_io_last_error() and L.zrh_scene_data_morph(other.h)
    assert posed(other.h, 1.0).tobytes() == scene_io.morph_pose(a, k, m, rest, 1.0).tobytes()
    assert L.zrh_scene_data_set_skinning(other.h, C.addressof(kd)) == 0 and not L.zrh_scene_data_morph(other.h)      # a new skin set clears the morph set
    assert L.zrh_scene_data_set_morph(other.h, C.addressof(md)) == 0 and other.set_animation(a) == 0 and not L.zrh_scene_data_morph(other.h)      # ... and a new animation
    host.close(); other.close()
