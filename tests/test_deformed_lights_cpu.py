"""Deformed lights on the host: the loader's opt-in flag (ZRH_LOAD_DEFORMED_LIGHTS), the rule zrsm::EmissiveFromVertices as the host compiles it
(zrh_emissive_from_vertices) against the loader's own records, against zrh_emissive_to_world and against float64, and the host form of the refresh
(zrh_scene_data_refresh_emissives, zrh_scene_data_pose_lights).  The stand-alone sanitizer program of the same paths is `make -C tests/lightmath fuzz`."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.animmath import cases as acases
from tests.lightmath import cases as lcases
from tests.morphmath import cases as mcases
from tests.skinmath import cases as scases
from zetaray_amd import scene_io, wire

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
REFUSALS = {"morph": "a morphed primitive with an emissive material is not supported (a deformed light would keep shining from its rest pose)",
            "skin": "a skinned primitive with an emissive material is not supported (a deformed light would keep shining from its rest pose)"}


def _emissive_file(tmp_path, which):
    d = tmp_path / which
    d.mkdir(exist_ok=True)
    return lcases.emissive_morphed_gltf(d) if which == "morph" else lcases.emissive_skinned_gltf(d)


# ---------------------------------------------------------------------------------------------------------------- the loader
@pytest.mark.parametrize("which", ["morph", "skin"])
def test_the_flag_lifts_the_refusal_and_nothing_else(tmp_path, which):
    """an emissive morphed / skinned file: refused by today's words without the flag, loaded with it -- lights whose vertices lie in the file's own pose
    ranges, light records made from the rest pose as for any mesh"""
    path = _emissive_file(tmp_path, which)
    with pytest.raises(RuntimeError) as e:
        scene_io.load_gltf_native(path)
    assert REFUSALS[which] in str(e.value)
    sc, _ = scene_io.load_gltf_native(path, deformed_lights=True)
    listed = lcases.listed_lights(sc, lcases.set_ranges(sc.skinning, sc.morph))
    assert 0 < len(listed) < len(sc.emissives)
    # every record of the file, deformable or not: the object-space record is the rule at the rest pose, byte for byte -- the loader's geometry step IS
    # the rule's first half -- and its world record is zrh_emissive_to_world of that, unless the loader took the identity shortcut
    for i in range(len(sc.instances)):
        b = int(sc.instances[i]["base_emissive_tri_offset"])
        if b == lcases.NONE:
            continue
        M = sc.instance_to_world[i]
        for t, v in enumerate(lcases.light_vertices(sc, i)):
            p = sc.vertices["pos"][v]
            obj, world = scene_io.emissive_from_vertices(sc.emissives_initial[b + t], p[0], p[1], p[2], M)
            assert obj.tobytes() == sc.emissives_initial[b + t].tobytes(), f"instance {i}, triangle {t}: object-space record"
            assert world.tobytes() == scene_io.emissive_to_world(sc.emissives_initial[b + t:b + t + 1], M)[0].tobytes()
            if not np.array_equal(M, scases.IDENTITY):
                assert world.tobytes() == sc.emissives[b + t].tobytes(), f"instance {i}, triangle {t}: world record"
            else:
                assert sc.emissives[b + t].tobytes() == sc.emissives_initial[b + t].tobytes()


def _arrays(sc):
    out = [np.ascontiguousarray(getattr(sc, n)).tobytes() for n in ("vertices", "indices", "instances", "instance_to_world", "instance_mask", "instance_num_tris", "materials", "emissives", "textures", "texels")]
    if sc.animation is not None:
        out += [np.ascontiguousarray(a).tobytes() for a in (sc.animation.nodes, sc.animation.keys, sc.animation.instance_idx, sc.animation.instance_node, sc.emissives_initial)]
    if sc.skinning is not None:
        out += [np.ascontiguousarray(a).tobytes() for a in (sc.skinning.joints, sc.skinning.ranges, sc.skinning.influences)]
    if sc.morph is not None:
        m = sc.morph
        out += [np.ascontiguousarray(a).tobytes() for a in (m.tracks, m.targets, m.ranges, m.times, m.values, m.rest_weights, m.deltas)]
    return out


def test_every_fixture_loads_to_the_same_bytes_with_and_without_the_flag(tmp_path):
    """the glTF fixtures of tests/golden (plain, emissive, animated, skinned, morphed), in both texture modes: every loaded array and table, compared whole"""
    scases.skinned_gltf(tmp_path)
    mcases.morphed_gltf(tmp_path)
    names = ["cornell.gltf", "cornell_emissive.gltf", "cornell_animated.gltf", "cornell_skinned.gltf", "cornell_morphed.gltf"]
    for name in names:
        if not (tmp_path / name).exists():
            (tmp_path / name).write_text(json.dumps(json.load(open(os.path.join(acases.REF_GLTF, name)))))
        for mode in ("decoded", "compressed"):
            a, oa = scene_io.load_gltf_native(str(tmp_path / name), textures=mode)
            b, ob = scene_io.load_gltf_native(str(tmp_path / name), textures=mode, deformed_lights=True)
            assert _arrays(a) == _arrays(b) and oa == ob, (name, mode)
            assert (a.skinning is None) == (b.skinning is None) and (a.morph is None) == (b.morph is None)


# ---------------------------------------------------------------------------------------------------------------- the rule against float64
def _decode64(rec):
    """the three vertices a record MEANS, in float64: vtx0 + unit(oct16 direction) * fp16 length"""
    v0 = rec["vtx0"].astype(F64)
    ln = rec["edge_lengths"].view(np.float16).astype(F64)
    return v0, v0 + scases.decode_oct64(rec["v0v1"])[0] * ln[0], v0 + scases.decode_oct64(rec["v0v2"])[0] * ln[1]


def test_world_record_against_float64():
    """The vertices decoded from the world record lie within the record's own encoding error of M x posed position.

    An edge e of length L is stored as a direction in 16-bit octahedral code words and a length in fp16.
      direction: each of the two code words is rounded to the nearest of 65 535 steps over [-1, 1]: an error of at most d = 1 / 65535 in each octahedral
        coordinate.  The decoded, unnormalised vector (x, y, z) has |x| + |y| + |z| = 1, so a Euclidean length of at least 1 / sqrt(3), and moves by at
        most (d, d, 2 d), i.e. sqrt(6) d: an angle of at most A = sqrt(18) d (1 + 18 d^2) (asin x <= x (1 + x^2)) = 6.47e-5 rad.
      length: fp16 round to nearest inside the normal range [2^-14, 65504]: a relative error of at most h = 2^-11.
      So a decoded end point is off by at most L (A + h) (1 + h): the chord of the angle plus the length error on the turned edge.
    The rule encodes twice: the object-space triangle, then -- decoded, taken through M -- the world one.  With s = the largest singular value of M's 3 x 3,
      stage 1 leaves an end point off by at most L (A + h)(1 + h) in object space, s times that in world space;
      stage 2 encodes an edge of length at most s L (1 + (A + h)(1 + h)) and adds that length times (A + h)(1 + h).
    The fp32 chain, counted rounding by rounding on the path from the inputs to one decoded coordinate of v1 (abs, negation, the sign select, int -> float
      and "+ 0" are exact; the roundings to a code word and to fp16 are d and h above):
        encode (StoreEmissiveVertices + EncodeOct32): e = v1 - v0 (1); the squared length, 3 products + 2 sums (5); sqrt (1); e / l (1); the octahedral
          denominator, 2 sums (2); n / denom (1); the fold 1 - |p| (1); fma(enc, 0.5, 0.5) (1); * 65535 (1)                                  = 14
        decode (DecodeEmissiveVertices): code / 65535 (1); fma(., 2, -1) (1); z = 1 - (|ux| + |uy|) (2); dx = ux + t (1); the squared norm, 3 products
          + 2 sums (5); sqrt (1); d / n (1); fma(d, len, vtx0) (1)                                                                           = 13
        MulPoint: one product and three fmas (4), for the end point and for vertex 0, whose difference is the world edge (4)                 =  8
        encode again                                                                                                                        = 14
      49 roundings (the last decode is the test's own, in float64), each at most U = 2^-24 relative to a quantity no larger than
      mag = |M| |p| + |t| (the largest such row sum over the triangle's vertices), or to a unit-scale quantity that is later multiplied by an edge length
      <= mag: 49 U mag per coordinate, sqrt(3) times that in Euclidean norm.
    vtx0 is stored in fp32 as it comes out of M x p0: within the fp32 term alone.
    The inputs are drawn so that the bound holds for the reference arithmetic alone: every edge, before and after M, inside fp16's normal range and at
    least 1e-3 long, asserted below."""
    rng = np.random.default_rng(2024)
    d = 1.0 / 65535.0
    A = np.sqrt(18.0) * d * (1 + 18 * d * d)
    h = 2.0 ** -11
    q = (A + h) * (1 + h)
    template = scene_io.load_npz(os.path.join(scases.ROOT, "tests", "golden", "cornell_emissive.npz")).emissives_initial[0]
    worst = 0.0
    for case in range(400):
        L0 = 10.0 ** rng.uniform(-2.5, 0.5)
        p0 = rng.uniform(-2, 2, 3)
        p = np.stack([p0, p0 + scases.unit(rng.normal(size=3)) * L0 * rng.uniform(0.5, 1.0), p0 + scases.unit(rng.normal(size=3)) * L0 * rng.uniform(0.5, 1.0)]).astype(F32)
        ident = case % 8 == 0
        M = scases.IDENTITY.copy() if ident else scases.trs12(rng.uniform(-3, 3, 3), rng.normal(size=3), rng.uniform(-3.1, 3.1), rng.uniform(0.5, 2.0, 3))
        obj, world = scene_io.emissive_from_vertices(template, p[0], p[1], p[2], M)
        for f in ("id", "packed_a", "packed_b", "uv0", "uv1", "uv2"):
            assert np.array_equal(obj[f], template[f]) and np.array_equal(world[f], template[f]), f
        assert obj["vtx0"].tobytes() == p[0].tobytes()
        M64 = M.astype(F64).reshape(3, 4)
        want = p.astype(F64) @ M64[:, :3].T + M64[:, 3]
        s = float(np.linalg.svd(M64[:, :3], compute_uv=False)[0])
        mag = float((np.abs(p.astype(F64)) @ np.abs(M64[:, :3]).T + np.abs(M64[:, 3])).max())
        fp32 = np.sqrt(3.0) * 49 * U * mag
        got = _decode64(world)
        for k in (1, 2):
            L = float(np.linalg.norm(p[k].astype(F64) - p[0].astype(F64)))
            Lw = float(np.linalg.norm(want[k] - want[0]))
            assert 1e-3 <= L <= 65504 and 1e-3 <= Lw <= 65504 and min(L, Lw) >= 2.0 ** -14
            bound = s * L * q + s * L * (1 + q) * q + fp32
            err = float(np.linalg.norm(got[k] - want[k]))
            worst = max(worst, err / bound)
            assert err <= bound, f"case {case}, vertex {k}: {err:.3e} > {bound:.3e}"
        assert float(np.linalg.norm(got[0] - want[0])) <= fp32
    print("largest error / bound:", worst)
    assert worst > 0.02      # (the bound is not vacuous: the encoding error is really there)


# ---------------------------------------------------------------------------------------------------------------- the host form of the refresh
def _own(sc):
    w = copy.copy(sc)
    w._desc, w.emissives, w.emissives_initial = None, sc.emissives.copy(), sc.emissives_initial.copy()
    return w


def test_host_refresh_over_ranges_and_ownerless_triangles():
    """zrh_scene_data_refresh_emissives on the lit scene with three records no instance carries: the triangles of the range become the rule's records at the
    given vertices with their owners' matrices, object-space and world; the ownerless ones and everything outside the range keep their bytes; the dirty
    range is the range's owned part; a range past the end and a scene without object-space records are refused with nothing changed"""
    sc, firsts, base = lcases.lit_world(ownerless=3)
    bent = sc.vertices.copy()
    bent["pos"][firsts[0]:] += np.random.default_rng(5).uniform(-0.03, 0.03, (len(bent) - firsts[0], 3)).astype(F32)
    n = len(sc.emissives)
    first, count = lcases.TUBE_TRIS - 7, 7 + 2 + 3 + 9      # tube 0's last 7, the lamp's 2, the 3 ownerless, tube 1's first 9
    w = _own(sc)
    assert scene_io.refresh_emissives(w, bent, first, count) == (first, count)
    for k in range(n):
        owner = next((i for i in (lcases.TUBE0, lcases.LAMP, lcases.TUBE1) if base[i] <= k < base[i] + int(sc.instance_num_tris[i])), None)
        if k < first or k >= first + count or owner is None:
            assert w.emissives[k].tobytes() == sc.emissives[k].tobytes() and w.emissives_initial[k].tobytes() == sc.emissives_initial[k].tobytes(), k
            continue
        v = lcases.light_vertices(sc, owner)[k - base[owner]]
        obj, world = scene_io.emissive_from_vertices(sc.emissives_initial[k], *bent["pos"][v], sc.instance_to_world[owner])
        assert w.emissives_initial[k].tobytes() == obj.tobytes() and w.emissives[k].tobytes() == world.tobytes(), k
        assert (owner == lcases.LAMP) or w.emissives[k].tobytes() != sc.emissives[k].tobytes()
    # vertices = None: the scene's own, so the tubes' records come back
    assert scene_io.refresh_emissives(w, None, 0, n) == (0, n)
    tubes = np.r_[0:lcases.TUBE_TRIS, base[lcases.TUBE1]:n]
    assert w.emissives[tubes].tobytes() == sc.emissives[tubes].tobytes() and w.emissives_initial.tobytes() == sc.emissives_initial.tobytes()
    for bad in ((n, 1), (0, n + 1), (0xFFFFFFFF, 2)):
        with pytest.raises(ValueError) as e:
            scene_io.refresh_emissives(w, bent, *bad)
        assert "exceeds the scene's emissive triangles" in str(e.value)
    assert scene_io.refresh_emissives(w, bent, n, 0) == (0, 0)
    bare = _own(sc)
    bare.emissives_initial = np.zeros(0, wire.EMISSIVE_TRI)
    with pytest.raises(ValueError) as e:
        scene_io.refresh_emissives(bare, bent, 0, 4)
    assert "no object-space light records" in str(e.value)


@pytest.mark.parametrize("which", ["morph", "skin"])
def test_pose_lights_of_a_loaded_file(tmp_path, which):
    """zrh_scene_data_pose_lights on the emissive fixtures: the triangles the numpy restatement lists, ascending"""
    path = _emissive_file(tmp_path, which)
    sc, _ = scene_io.load_gltf_native(path, deformed_lights=True)
    L = lcases.sio()
    L.zrh_scene_data_pose_lights.argtypes, L.zrh_scene_data_pose_lights.restype = [C.c_void_p, C.c_void_p], C.c_uint32
    rho, dim = scene_io.load_rho_default()
    rho = np.ascontiguousarray(rho, np.uint16)
    h = C.c_void_p()
    assert L.zrh_gltf_load_ex(os.fsencode(path), rho.ctypes.data, (C.c_uint32 * 3)(*dim), scene_io.LOAD_DEFORMED_LIGHTS, C.byref(h)) == 0
    p = C.POINTER(C.c_uint32)()
    n = L.zrh_scene_data_pose_lights(h, C.byref(p))
    want = lcases.listed_lights(sc, lcases.set_ranges(sc.skinning, sc.morph))
    assert n == len(want) > 0 and [p[i] for i in range(n)] == want.tolist()
    L.zrh_scene_data_destroy(h)
