#!/usr/bin/env python3
"""Writes tests/golden/morph_gltf/cornell_morphed.gltf + morph.bin: the animated Cornell box (tests/golden/cornell_gltf/cornell_animated.gltf, whose buffers
and images are referenced by their names there, not copied) plus two meshes with morph targets.

  - mesh "Face": a 7 x 6 grid with TEXCOORD_0 and TANGENT and 5 targets -- 0: POSITION + NORMAL + TANGENT as floats; 1: POSITION + TANGENT (no NORMAL);
    2: POSITION + NORMAL (no TANGENT); 3: SPARSE -- POSITION over zeros (no bufferView), NORMAL over a bufferView base; 4: POSITION as normalised shorts,
    NORMAL as normalised bytes.  mesh.weights gives defaults, node "Face" overrides them, and a weights channel of 3 keys drives them: the values hold an
    exact 0, a negative value and a value above 1;
  - the skinned tube of tools/make_skin_gltf.py (its rig, skin and knee rotation) with 2 targets (POSITION + NORMAL, POSITION alone) on node "TubeA",
    driven by a weights channel of its own whose input accessor is not the face's.

tests/morphmath lays the files out next to the Cornell fixture's (tests/morphmath/cases.py: morphed_gltf)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_skin_gltf as mk      # noqa: E402

ROOT = mk.ROOT
DIR = os.path.join(ROOT, "tests", "golden", "morph_gltf")
GX, GY = 7, 6


def face(rng):
    j, i = np.divmod(np.arange(GX * GY), GX)
    u, v = i / (GX - 1), j / (GY - 1)
    pos = np.stack([-0.75 + 0.4 * u, 0.9 + 0.4 * v, 0.5 + 0.05 * np.sin(3 * u) * np.cos(2 * v)], 1).astype(np.float32)
    nrm = np.stack([-0.15 * np.cos(3 * u), 0.1 * np.sin(2 * v), np.ones(len(u))], 1)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    tan = np.stack([np.ones(len(u)), np.zeros(len(u)), 0.15 * np.cos(3 * u)], 1)
    tan = np.concatenate([tan / np.linalg.norm(tan, axis=1, keepdims=True), np.ones((len(u), 1))], 1).astype(np.float32)
    uv = np.stack([u, v], 1).astype(np.float32)
    idx = []
    for y in range(GY - 1):
        for x in range(GX - 1):
            p = y * GX + x
            idx += [p, p + 1, p + GX, p + 1, p + GX + 1, p + GX]
    return pos, nrm, tan, uv, np.asarray(idx, np.uint16)


def main():
    g = json.load(open(os.path.join(mk.SRC, "cornell_animated.gltf")))
    os.makedirs(DIR, exist_ok=True)
    rng = np.random.default_rng(77)
    blob = b""
    buf = len(g["buffers"])

    def view(data):
        nonlocal blob
        while len(blob) % 4:
            blob += b"\0"
        data = np.ascontiguousarray(data)
        g["bufferViews"].append({"buffer": buf, "byteOffset": len(blob), "byteLength": data.nbytes})
        blob += data.tobytes()
        return len(g["bufferViews"]) - 1

    def accessor(data, comp, typ, normalized=False):
        data = np.ascontiguousarray(data)
        acc = {"bufferView": view(data), "componentType": comp, "count": len(data), "type": typ}
        if normalized:
            acc["normalized"] = True
        if typ == "VEC3" and comp == 5126:
            acc["min"], acc["max"] = [float(x) for x in data.min(0)], [float(x) for x in data.max(0)]
        g["accessors"].append(acc)
        return len(g["accessors"]) - 1

    def sparse(count, indices, values, base=None):
        acc = {"componentType": 5126, "count": count, "type": "VEC3",
               "sparse": {"count": len(indices), "indices": {"bufferView": view(indices.astype(np.uint16)), "componentType": 5123}, "values": {"bufferView": view(values.astype(np.float32))}}}
        if base is not None:
            acc["bufferView"] = view(base.astype(np.float32))
        g["accessors"].append(acc)
        return len(g["accessors"]) - 1

    plain = next(i for i, m in enumerate(g["materials"]) if "emissiveFactor" not in m and "emissiveTexture" not in m and "KHR_materials_emissive_strength" not in m.get("extensions", {}))
    # ---- the face
    pos, nrm, tan, uv, idx = face(rng)
    n = len(pos)
    d = lambda s: rng.uniform(-s, s, (n, 3)).astype(np.float32)
    sp_i = np.sort(rng.choice(n, 11, replace=False))
    sp_j = np.sort(rng.choice(n, 9, replace=False))
    q_pos = np.rint(rng.uniform(-0.05, 0.05, (n, 3)) * 32767).astype(np.int16)
    q_pos = np.concatenate([q_pos, np.zeros((n, 1), np.int16)], 1)      # (3 shorts padded to a 4-byte multiple: the view is strided)
    q_nrm = np.concatenate([np.rint(rng.uniform(-0.06, 0.06, (n, 3)) * 127).astype(np.int8), np.zeros((n, 1), np.int8)], 1)

    def strided(data, comp):
        acc = {"bufferView": view(data), "componentType": comp, "count": n, "type": "VEC3", "normalized": True}
        g["bufferViews"][-1]["byteStride"] = data.strides[0]
        g["accessors"].append(acc)
        return len(g["accessors"]) - 1

    targets = [{"POSITION": accessor(d(0.05), 5126, "VEC3"), "NORMAL": accessor(d(0.06), 5126, "VEC3"), "TANGENT": accessor(d(0.06), 5126, "VEC3")},
               {"POSITION": accessor(d(0.05), 5126, "VEC3"), "TANGENT": accessor(d(0.06), 5126, "VEC3")},
               {"POSITION": accessor(d(0.05), 5126, "VEC3"), "NORMAL": accessor(d(0.06), 5126, "VEC3")},
               {"POSITION": sparse(n, sp_i, rng.uniform(-0.08, 0.08, (11, 3))), "NORMAL": sparse(n, sp_j, rng.uniform(-0.06, 0.06, (9, 3)), base=d(0.02))},
               {"POSITION": strided(q_pos, 5122), "NORMAL": strided(q_nrm, 5120)}]
    at = {"POSITION": accessor(pos, 5126, "VEC3"), "NORMAL": accessor(nrm, 5126, "VEC3"), "TANGENT": accessor(tan, 5126, "VEC4"), "TEXCOORD_0": accessor(uv, 5126, "VEC2")}
    face_mesh = len(g["meshes"])
    g["meshes"].append({"name": "Face", "weights": [0.1, 0.0, 0.0, 0.0, 0.2],
                        "primitives": [{"attributes": at, "indices": accessor(idx, 5123, "SCALAR"), "material": plain, "targets": targets}]})
    # ---- the skinned tube with two targets
    tpos, tnrm, tuv, tidx, joints, weights = mk.tube(-0.15)
    tn = len(tpos)
    at = {"POSITION": accessor(tpos, 5126, "VEC3"), "NORMAL": accessor(tnrm, 5126, "VEC3"), "TEXCOORD_0": accessor(tuv, 5126, "VEC2"),
          "JOINTS_0": accessor(joints.astype(np.uint8), 5121, "VEC4"), "WEIGHTS_0": accessor(weights.astype(np.float32), 5126, "VEC4")}
    bulge = (tnrm * (0.04 * np.sin(np.linspace(0, np.pi, tn)))[:, None]).astype(np.float32)
    ttargets = [{"POSITION": accessor(bulge, 5126, "VEC3"), "NORMAL": accessor(rng.uniform(-0.1, 0.1, (tn, 3)).astype(np.float32), 5126, "VEC3")},
                {"POSITION": accessor(rng.uniform(-0.02, 0.02, (tn, 3)).astype(np.float32), 5126, "VEC3")}]
    tube_mesh = len(g["meshes"])
    g["meshes"].append({"name": "Tube", "primitives": [{"attributes": at, "indices": accessor(tidx, 5123, "SCALAR"), "material": plain, "targets": ttargets}]})
    n0 = len(g["nodes"])
    rig, hip, knee, toe, tube_a, face_node = range(n0, n0 + 6)
    rig_q, hip_q, knee_q, toe_q = mk.quat([0, 1, 0], 0.4), mk.quat([1, 0, 0], 0.15), mk.quat([0, 0, 1], -0.1), mk.quat([1, 1, 0], 0.2)
    rig_t, hip_t, knee_t, toe_t = [0.0, 0.0, 0.35], [0.02, mk.JOINT_Y[0], -0.03], [0.01, 0.4, 0.02], [0.0, 0.4, -0.01]
    g["nodes"] += [{"name": "Rig", "translation": rig_t, "rotation": rig_q, "children": [hip]},
                   {"name": "Hip", "translation": hip_t, "rotation": hip_q, "children": [knee]},
                   {"name": "Knee", "translation": knee_t, "rotation": knee_q, "children": [toe]},
                   {"name": "Toe", "translation": toe_t, "rotation": toe_q},
                   {"name": "TubeA", "mesh": tube_mesh, "skin": 0},
                   {"name": "Face", "mesh": face_mesh, "weights": [0.0, 0.25, 0.0, 0.0, 0.0], "translation": [0.05, 0.0, 0.0]}]
    g["scenes"][g.get("scene", 0)]["nodes"] += [rig, tube_a, face_node]
    W = mk.trs(rig_t, rig_q)
    ibm = []
    for t, q in ((hip_t, hip_q), (knee_t, knee_q), (toe_t, toe_q)):
        W = W @ mk.trs(t, q)
        ibm.append(np.linalg.inv(W).T.reshape(16))
    g["skins"] = [{"name": "Leg", "joints": [hip, knee, toe], "inverseBindMatrices": accessor(np.asarray(ibm, np.float32), 5126, "MAT4")}]
    a = g["animations"][0]

    def channel(node, path, times, out, typ):
        a["samplers"].append({"input": accessor(np.float32(times), 5126, "SCALAR"), "output": accessor(np.float32(out), 5126, typ), "interpolation": "LINEAR"})
        a["channels"].append({"sampler": len(a["samplers"]) - 1, "target": {"node": node, "path": path}})

    channel(knee, "rotation", [0.0, 0.5, 1.0, 1.5], [knee_q, mk.quat([1, 0, 0], 0.5), mk.quat([0, 0, 1], 0.45), knee_q], "VEC4")
    channel(face_node, "weights", [0.0, 0.6, 1.4], [0.0, 0.5, -0.25, 1.0, 0.0,   1.25, 0.0, 0.75, 0.0, 0.5,   0.0, 0.5, -0.25, 1.0, 0.0], "SCALAR")
    channel(tube_a, "weights", [0.0, 0.75, 1.5], [0.0, 0.0,   1.0, -0.5,   0.0, 0.0], "SCALAR")
    g["buffers"].append({"uri": "morph.bin", "byteLength": len(blob)})
    open(os.path.join(DIR, "morph.bin"), "wb").write(blob)
    json.dump(g, open(os.path.join(DIR, "cornell_morphed.gltf"), "w"), indent=1)
    print(f"wrote {DIR}: {len(blob)} B of geometry, nodes {n0}..{n0 + 5}")


if __name__ == "__main__":
    main()
