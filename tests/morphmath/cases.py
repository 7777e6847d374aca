"""What the morph-target tests share (tests/test_morph_cpu.py, tests/test_morph_gpu.py): a float64 restatement of include/zr_morph.h's MorphVertex, the
builder of morph sets over vertex ranges of a scene, and the host form the device form is held to.  The scene is the skinning tests' (the Cornell box plus
tubes, tests/skinmath/cases.py): a tube is the "face" here."""
import os

import numpy as np

from tests.skinmath import cases as scases
from tests.skinmath import zsk
from zetaray_amd import scene_io, wire

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
NONE = wire.MORPH_NONE
KEY_TIMES = (0.0, 0.5, 1.25)      # 0.5 and 1.25 are among tests/animmath/cases.py's TIMES: weights ON a key


def gamma(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------------------------------------------- float64 restatement
def morph64(rest, targets, weights, deltas):
    """MorphVertex in float64 on the float32 inputs, vertex i reading triple first_* + i.  Returns a dict: pos (n, 3) and pos_mag = |p_c| + sum_k |w_k| |d_k,c|;
    for a in ("normal", "tangent"): a (n, 3) the unnormalised sum, a + "_mag" = sum_k |w_k| |d_k| (Euclidean), a + "_applied" whether any delta was applied;
    applied = the number of applied (non-zero weight) targets"""
    rest = np.asarray(rest).reshape(-1)
    n = len(rest)
    idx = np.arange(n)
    deltas = np.asarray(deltas, F64).reshape(-1, 3)
    out = {"pos": rest["pos"].astype(F64), "pos_mag": np.abs(rest["pos"].astype(F64)), "applied": 0}
    for a, field in (("normal", "normal"), ("tangent", "tangent")):
        out[a] = scases.decode_oct64(rest[field])
        out[a + "_mag"] = np.zeros(n)
        out[a + "_applied"] = False
    for m, w in zip(np.asarray(targets).reshape(-1), np.asarray(weights, F32).reshape(-1)):
        w = float(w)
        if w == 0.0:
            continue
        out["applied"] += 1
        if int(m["first_pos"]) != NONE:
            d = deltas[int(m["first_pos"]) + idx]
            out["pos"] = out["pos"] + w * d
            out["pos_mag"] = out["pos_mag"] + abs(w) * np.abs(d)
        for a, f in (("normal", "first_nrm"), ("tangent", "first_tan")):
            if int(m[f]) != NONE:
                d = deltas[int(m[f]) + idx]
                out[a] = out[a] + w * d
                out[a + "_mag"] = out[a + "_mag"] + abs(w) * np.linalg.norm(d, axis=1)
                out[a + "_applied"] = True
    return out


# ---------------------------------------------------------------------------------------------------------------- morph sets
LACK_NONE, LACK_NRM, LACK_TAN, LACK_BOTH = 0, 1, 2, 3


def keyed_track(rng, num_targets, times=KEY_TIMES, loop=0, t0=0.0, zero_at=(), all_zero_key=None):
    """a track description: weights in [-0.5, 1.5] (a negative value and one above 1 among them); zero_at: [(key, target)] set to an exact 0; all_zero_key:
    a key whose weights are all 0"""
    v = rng.uniform(-0.5, 1.5, (len(times), num_targets)).astype(F32)
    v[0, 0], v[-1, -1] = -0.375, 1.25
    for k, j in zero_at:
        v[k, j] = 0.0
    if all_zero_key is not None:
        v[all_zero_key] = 0.0
    return {"num_targets": num_targets, "times": np.asarray(times, F32), "values": v, "loop": loop, "t0": t0}


def static_track(weights):
    """num_keys == 0: the rest weights at every time"""
    return {"num_targets": len(weights), "times": np.zeros(0, F32), "values": np.zeros((0, len(weights)), F32), "rest": np.asarray(weights, F32), "loop": 0, "t0": 0.0}


def morph_set(ranges, tracks, lacks=None, seed=11, share_targets=False):
    """wire.MorphDesc over ranges [(first_vertex, num_vertices, track index)] with tracks as keyed_track / static_track describe them.  Every range gets targets
    of its own (share_targets: ranges of equal size and track share them), target k of a range lacking what lacks[k % len(lacks)] says.  POSITION deltas
    are at most 0.04 per component, NORMAL and TANGENT deltas at most 0.25 / T: under weights of at most 1.5 in magnitude the summed direction keeps a
    length of at least 1 - 1.5 * 0.25 * sqrt(3) = 0.35"""
    rng = np.random.default_rng(seed)
    lacks = lacks or [LACK_NONE]
    tr = np.zeros(len(tracks), wire.MORPH_TRACK)
    times, values, rest_w = [], [], []
    for i, t in enumerate(tracks):
        tr[i]["num_targets"], tr[i]["num_keys"], tr[i]["loop"], tr[i]["t0"] = t["num_targets"], len(t["times"]), t["loop"], t["t0"]
        tr[i]["first_key"], tr[i]["first_value"], tr[i]["first_rest"] = sum(map(len, times)), sum(map(len, values)), sum(map(len, rest_w))
        times.append(np.asarray(t["times"], F32))
        values.append(np.asarray(t["values"], F32).reshape(-1))
        rest_w.append(np.asarray(t.get("rest", np.zeros(t["num_targets"])), F32))
    targets, rr, deltas, nd, shared = [], [], [], 0, {}
    for first, count, track in ranges:
        T = int(tr[track]["num_targets"])
        if share_targets and (count, track) in shared:
            rr.append((first, count, shared[(count, track)], T, track))
            continue
        shared[(count, track)] = len(targets)
        rr.append((first, count, len(targets), T, track))
        for k in range(T):
            lack = lacks[k % len(lacks)]
            m = [NONE, NONE, NONE]
            for a, (have, scale) in enumerate(((True, 0.04), (lack not in (LACK_NRM, LACK_BOTH), 0.25 / T), (lack not in (LACK_TAN, LACK_BOTH), 0.25 / T))):
                if have:
                    m[a] = nd
                    deltas.append(rng.uniform(-scale, scale, (count, 3)).astype(F32))
                    nd += count
            targets.append(tuple(m))
    cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape, F32)
    return wire.MorphDesc(tr, np.array(targets, wire.MORPH_TARGET), np.array(rr, wire.MORPH_RANGE), cat(times, 0), cat(values, 0), cat(rest_w, 0), cat(deltas, (0, 3)))


def rest_of_ranges(morph, vertices):
    return scases.rest_of_ranges(morph, vertices)


def same_range(r, skin):
    return skin is not None and any(int(r["first_vertex"]) == int(q["first_vertex"]) and int(r["num_vertices"]) == int(q["num_vertices"]) for q in skin.ranges)


def host_posed(anim, skin, morph, rest, t):
    """the host form's vertices of the morph ranges for time t (zrh_morph_pose: zr_morph.h, then zr_skin.h where the range is a skin range too)"""
    return scene_io.morph_pose(anim, skin, morph, rest, t)


def apply_host_form(scene, host, anim, skin, morph, vertices, t, stream=False):
    """the host sequence the device form is held to: zrh_scene_data_animate(t); zr_scene_update_vertices with the vertices zr_morph.h computes on the host,
    followed by zr_skin.h where the range is skinned (and with the skin-only ranges' vertices from zr_skin.h alone); then the host-form emissive and
    instance updates.  vertices: the scene's rest pose.  Returns the posed records of the morph ranges"""
    posed = host_posed(anim, skin, morph, rest_of_ranges(morph, vertices), t)
    k = 0
    for r in morph.ranges:
        n = int(r["num_vertices"])
        if n:
            scene.update_vertices(int(r["first_vertex"]), posed[k:k + n], stream=stream)
        k += n
    if skin is not None:
        sk = scases.host_posed(anim, skin, scases.rest_of_ranges(skin, vertices), t)
        k = 0
        for r in skin.ranges:
            n = int(r["num_vertices"])
            if n and not same_range(r, morph):
                scene.update_vertices(int(r["first_vertex"]), sk[k:k + n], stream=stream)
            k += n
    host.apply(scene, t, stream=stream)
    return posed


def posed_scene_vertices(anim, skin, morph, vertices, t):
    """the whole vertex array of the host form at time t"""
    out = vertices.copy()
    if skin is not None:
        sk = scases.host_posed(anim, skin, scases.rest_of_ranges(skin, vertices), t)
        k = 0
        for r in skin.ranges:
            n = int(r["num_vertices"])
            out[int(r["first_vertex"]):int(r["first_vertex"]) + n] = sk[k:k + n]
            k += n
    posed = host_posed(anim, skin, morph, rest_of_ranges(morph, vertices), t)
    k = 0
    for r in morph.ranges:
        n = int(r["num_vertices"])
        out[int(r["first_vertex"]):int(r["first_vertex"]) + n] = posed[k:k + n]
        k += n
    return out


# ---------------------------------------------------------------------------------------------------------------- the loader's fixture
MORPH_GLTF = os.path.join(scases.ROOT, "tests", "golden", "morph_gltf")


def morphed_gltf(tmp_path, edit=None, name="cornell_morphed", blob_edit=None):
    """tests/golden/morph_gltf/cornell_morphed.gltf (tools/make_morph_gltf.py) laid out next to the animated Cornell fixture's files, as it references
    them; edit(gltf dict) changes the JSON first, blob_edit(bytearray) the added buffer (it may return a longer one: the buffer's byteLength follows)"""
    import json
    from tests.animmath import cases as acases
    acases.cornell_animated(tmp_path)
    blob = bytearray(open(os.path.join(MORPH_GLTF, "morph.bin"), "rb").read())
    g = json.load(open(os.path.join(MORPH_GLTF, "cornell_morphed.gltf")))
    if blob_edit is not None:
        blob = blob_edit(blob, g) or blob
    g["buffers"][-1]["byteLength"] = len(blob)
    (tmp_path / "morph.bin").write_bytes(bytes(blob))
    if edit is not None:
        edit(g)
    p = tmp_path / (name + ".gltf")
    p.write_text(json.dumps(g))
    return str(p)
