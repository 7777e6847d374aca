#!/usr/bin/env python3
"""Writes tests/golden/cornell_gltf/cornell_animated.gltf + cornell_anim.bin: the emissive Cornell box with keyframe animation.

  - the short box (Cube.003) turns about y over 4 keys (rotation channel);
  - the light (Plane) translates over 3 keys (translation channel);
  - one extra parent node, "Carrier", carries the tall box (Cube.004) as a child and grows over 2 keys (scale channel): the tall box is a static
    node of the dynamic closure.

All samplers are LINEAR; the channels of a node share one input accessor.  The geometry buffer (cornell.bin) is referenced, not copied."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "cornell_gltf")


def main():
    g = json.load(open(os.path.join(DIR, "cornell_emissive.gltf")))
    names = [n.get("name") for n in g["nodes"]]
    short, tall, light = names.index("Cube.003"), names.index("Cube.004"), names.index("Plane")
    carrier = len(g["nodes"])
    g["nodes"].append({"name": "Carrier", "children": [tall]})
    roots = g["scenes"][g.get("scene", 0)]["nodes"]
    roots[roots.index(tall)] = carrier
    blob = b""
    buf = len(g["buffers"])

    def accessor(data, typ):
        nonlocal blob
        data = np.ascontiguousarray(data, np.float32)
        g["bufferViews"].append({"buffer": buf, "byteOffset": len(blob), "byteLength": data.nbytes})
        acc = {"bufferView": len(g["bufferViews"]) - 1, "componentType": 5126, "count": len(data), "type": typ}
        if typ == "SCALAR":
            acc["min"], acc["max"] = [float(data.min())], [float(data.max())]
        g["accessors"].append(acc)
        blob += data.tobytes()
        return len(g["accessors"]) - 1

    q0 = np.float32(g["nodes"][short]["rotation"])
    a0 = 2 * np.arctan2(q0[1], q0[3])
    ang = [a0 + 0.35 * k for k in range(4)]
    rot = np.float32([[0.0, np.sin(a / 2), 0.0, np.cos(a / 2)] for a in ang])
    t0 = np.float32(g["nodes"][light]["translation"])
    tr = np.float32([t0, t0 + np.float32([0.12, -0.05, 0.08]), t0 + np.float32([-0.1, -0.1, -0.06])])
    sc = np.float32([[1, 1, 1], [1.1, 1.05, 1.1]])
    samplers = [{"input": accessor([0.0, 0.5, 1.0, 1.5], "SCALAR"), "output": accessor(rot, "VEC4"), "interpolation": "LINEAR"},
                {"input": accessor([0.0, 0.75, 1.5], "SCALAR"), "output": accessor(tr, "VEC3"), "interpolation": "LINEAR"},
                {"input": accessor([0.25, 1.25], "SCALAR"), "output": accessor(sc, "VEC3")}]
    channels = [{"sampler": 0, "target": {"node": short, "path": "rotation"}}, {"sampler": 1, "target": {"node": light, "path": "translation"}},
                {"sampler": 2, "target": {"node": carrier, "path": "scale"}}]
    g["animations"] = [{"name": "cornell", "samplers": samplers, "channels": channels}]
    g["buffers"].append({"uri": "cornell_anim.bin", "byteLength": len(blob)})
    open(os.path.join(DIR, "cornell_anim.bin"), "wb").write(blob)
    json.dump(g, open(os.path.join(DIR, "cornell_animated.gltf"), "w"), indent=1)
    print(f"cornell_animated.gltf: nodes short {short} tall {tall} light {light} carrier {carrier}; cornell_anim.bin {len(blob)} bytes")


if __name__ == "__main__":
    main()
