#!/usr/bin/env python3
"""Writes tests/golden/skin_gltf/cornell_skinned.gltf + skin_tube.bin: the animated Cornell box (tests/golden/cornell_gltf/cornell_animated.gltf, whose
buffers and images are referenced by their names there, not copied) plus a small bent tube skinned over a chain of three joints.

  - joints "Hip" > "Knee" > "Toe": Hip is static and stands on a static, rotated and translated parent ("Rig"), Knee turns about x and z over 4 keys,
    Toe is a static leaf -- a joint that moves only because its ancestor does;
  - mesh "Tube": JOINTS_0 as unsigned bytes, WEIGHTS_0 as floats that sum to 0.5 (the loader renormalises);
  - mesh "Tube16": the same tube 0.3 to the side, JOINTS_0 as unsigned shorts, WEIGHTS_0 as normalised unsigned shorts;
  - nodes "TubeA" and "TubeA2" both use mesh "Tube" with the skin (each gets a vertex range of its own); TubeA carries a translation, which glTF
    ignores for a skinned node; node "TubeB" uses "Tube16".

tests/skinmath lays the files out next to the Cornell fixture's (tests/skinmath/cases.py: skinned_gltf)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "golden", "cornell_gltf")
DIR = os.path.join(ROOT, "tests", "golden", "skin_gltf")
RINGS, SEGS = 9, 8
Y0, Y1, R = 0.15, 1.35, 0.07
JOINT_Y = (0.15, 0.55, 0.95)      # Hip, Knee, Toe (world height at rest)


def quat(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return [float(x) for x in np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]])]


def rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def trs(t, q, s=(1, 1, 1)):
    M = np.eye(4)
    M[:3, :3] = rot(q) * np.asarray(s, np.float64).reshape(1, 3)
    M[:3, 3] = t
    return M


def tube(dx):
    ring, seg = np.divmod(np.arange(RINGS * SEGS), SEGS)
    a = 2 * np.pi * seg / SEGS
    y = Y0 + (Y1 - Y0) * ring / (RINGS - 1)
    pos = np.stack([dx + R * np.cos(a), y, 0.35 + R * np.sin(a)], 1).astype(np.float32)
    nrm = np.stack([np.cos(a), np.zeros(len(a)), np.sin(a)], 1).astype(np.float32)
    uv = np.stack([seg / SEGS, ring / (RINGS - 1)], 1).astype(np.float32)
    idx = []
    for r in range(RINGS - 1):
        for s in range(SEGS):
            p, q = r * SEGS + s, r * SEGS + (s + 1) % SEGS
            idx += [p, p + SEGS, q, q, p + SEGS, q + SEGS]
    # by height: the two joints around the vertex, a third slot with a small weight, an idle slot naming the last joint
    h = (y - JOINT_Y[0]) / (JOINT_Y[2] - JOINT_Y[0]) * 2
    j0 = np.clip(np.floor(h), 0, 1).astype(np.int64)
    fr = np.clip(h - j0, 0, 1)
    joints = np.stack([j0, j0 + 1, np.where(j0 == 0, 2, 0), np.full(len(y), 2)], 1)
    weights = np.stack([1 - fr, fr, np.full(len(y), 0.1), np.zeros(len(y))], 1)
    weights[::7] = [1, 0, 0, 0]
    return pos, nrm, uv, np.asarray(idx, np.uint16), joints, weights / weights.sum(1, keepdims=True)


def main():
    g = json.load(open(os.path.join(SRC, "cornell_animated.gltf")))
    os.makedirs(DIR, exist_ok=True)
    blob = b""
    buf = len(g["buffers"])

    def accessor(data, comp, typ, normalized=False):
        nonlocal blob
        while len(blob) % 4:
            blob += b"\0"
        data = np.ascontiguousarray(data)
        g["bufferViews"].append({"buffer": buf, "byteOffset": len(blob), "byteLength": data.nbytes})
        acc = {"bufferView": len(g["bufferViews"]) - 1, "componentType": comp, "count": len(data), "type": typ}
        if normalized:
            acc["normalized"] = True
        if typ == "VEC3" and comp == 5126:
            acc["min"], acc["max"] = [float(x) for x in data.min(0)], [float(x) for x in data.max(0)]
        g["accessors"].append(acc)
        blob += data.tobytes()
        return len(g["accessors"]) - 1

    plain = next(i for i, m in enumerate(g["materials"]) if "emissiveFactor" not in m and "emissiveTexture" not in m and "KHR_materials_emissive_strength" not in m.get("extensions", {}))
    meshes = []
    for name, dx, wide in (("Tube", -0.15, False), ("Tube16", 0.15, True)):
        pos, nrm, uv, idx, joints, weights = tube(dx)
        at = {"POSITION": accessor(pos, 5126, "VEC3"), "NORMAL": accessor(nrm, 5126, "VEC3"), "TEXCOORD_0": accessor(uv, 5126, "VEC2")}
        if wide:
            at["JOINTS_0"] = accessor(joints.astype(np.uint16), 5123, "VEC4")
            at["WEIGHTS_0"] = accessor(np.rint(weights * 65535).astype(np.uint16), 5123, "VEC4", normalized=True)
        else:
            at["JOINTS_0"] = accessor(joints.astype(np.uint8), 5121, "VEC4")
            at["WEIGHTS_0"] = accessor((0.5 * weights).astype(np.float32), 5126, "VEC4")
        meshes.append(len(g["meshes"]))
        g["meshes"].append({"name": name, "primitives": [{"attributes": at, "indices": accessor(idx, 5123, "SCALAR"), "material": plain}]})
    n0 = len(g["nodes"])
    rig, hip, knee, toe, tube_a, tube_a2, tube_b = range(n0, n0 + 7)
    rig_q, hip_q, knee_q, toe_q = quat([0, 1, 0], 0.4), quat([1, 0, 0], 0.15), quat([0, 0, 1], -0.1), quat([1, 1, 0], 0.2)
    rig_t, hip_t, knee_t, toe_t = [0.0, 0.0, 0.35], [0.02, JOINT_Y[0], -0.03], [0.01, 0.4, 0.02], [0.0, 0.4, -0.01]
    g["nodes"] += [{"name": "Rig", "translation": rig_t, "rotation": rig_q, "children": [hip]},
                   {"name": "Hip", "translation": hip_t, "rotation": hip_q, "children": [knee]},
                   {"name": "Knee", "translation": knee_t, "rotation": knee_q, "children": [toe]},
                   {"name": "Toe", "translation": toe_t, "rotation": toe_q},
                   {"name": "TubeA", "mesh": meshes[0], "skin": 0, "translation": [5.0, 5.0, 5.0]},
                   {"name": "TubeA2", "mesh": meshes[0], "skin": 0},
                   {"name": "TubeB", "mesh": meshes[1], "skin": 0}]
    g["scenes"][g.get("scene", 0)]["nodes"] += [rig, tube_a, tube_a2, tube_b]
    # inverse bind matrices: the inverses of the joints' world matrices at rest, column-major
    W = trs(rig_t, rig_q)
    ibm = []
    for t, q in ((hip_t, hip_q), (knee_t, knee_q), (toe_t, toe_q)):
        W = W @ trs(t, q)
        ibm.append(np.linalg.inv(W).T.reshape(16))
    g["skins"] = [{"name": "Leg", "joints": [hip, knee, toe], "inverseBindMatrices": accessor(np.asarray(ibm, np.float32), 5126, "MAT4")}]
    times = np.float32([0.0, 0.5, 1.0, 1.5])
    rots = np.float32([knee_q, quat([1, 0, 0], 0.5), quat([0, 0, 1], 0.45), knee_q])
    a = g["animations"][0]
    a["samplers"].append({"input": accessor(times, 5126, "SCALAR"), "output": accessor(rots, 5126, "VEC4"), "interpolation": "LINEAR"})
    a["channels"].append({"sampler": len(a["samplers"]) - 1, "target": {"node": knee, "path": "rotation"}})
    g["buffers"].append({"uri": "skin_tube.bin", "byteLength": len(blob)})
    open(os.path.join(DIR, "skin_tube.bin"), "wb").write(blob)
    json.dump(g, open(os.path.join(DIR, "cornell_skinned.gltf"), "w"), indent=1)
    print(f"wrote {DIR}: {len(blob)} B of geometry, nodes {n0}..{n0 + 6}")


if __name__ == "__main__":
    main()
