"""The scene and the animations the keyframe-animation tests share (tests/test_anim_cpu.py, tests/test_anim_gpu.py): a glTF file written into a
temporary directory, wire.AnimDesc tables over its nodes, and the host path (zrh_scene_data_animate) as ctypes calls."""
import ctypes as C
import gzip
import json
import os
import shutil

import numpy as np

from zetaray_amd import scene_io, wire

NONE = 0xFFFFFFFF
LIGHT_TRIS = (1, 63, 130)      # the owner array changes inside a wave (1) and inside a block (1 + 63 = 64, 64 + 130 = 194)
PLAIN_TRIS = (24, 40, 30, 36)
NUM_FILLERS = 257
# instance numbering of the loader (scene roots in order, depth first, one instance per primitive)
BASE = list(range(7))                          # plain, light 1, plain, light 63, plain, light 130, plain
LIGHTS = (1, 3, 5)
HIER_INST = {"root": (7, 8), "child": (9, 10), "grandchild": (11, 12)}
FILLER0 = 13
NUM_INSTANCES = FILLER0 + NUM_FILLERS
# the six times of the checks, against the three key-time templates below: before every first key / on keys of B and C, between A's / between keys
# everywhere / B's last key / C's last key / beyond every last key (looping and not)
TIMES = (-0.5, 0.5, 0.8125, 1.25, 2.125, 3.7)
KEY_TIMES = (np.float32([0.25, 1.0]), np.float32([0.0, 0.5, 1.25]), np.linspace(0.125, 2.125, 17).astype(np.float32))


def _quat(rng):
    q = rng.normal(size=4)
    return (q / np.linalg.norm(q)).astype(np.float32)


def _node_trs(k):
    """the rest transform of scene node k as written into the file (glTF convention)"""
    a = 0.3 * k
    return ([float(-1.5 + 0.5 * (k % 9)), float(0.6 + 0.2 * (k % 3)), float(0.3 * (k % 2))], [0.0, float(np.sin(a / 2)), 0.0, float(np.cos(a / 2))], [1.0 + 0.1 * (k % 5)] * 3)


def rest_of(trs):
    """glTF T / R / S -> the loader's convention: translation z negated, rotation x and y negated (zr_scene_io.cpp)"""
    t, q, s = trs
    return (np.float32(s), np.float32([-np.float32(q[0]), -np.float32(q[1]), q[2], q[3]]), np.float32([t[0], t[1], -np.float32(t[2])]))


def write_scene(tmp_path):
    """7 base instances (plain / light alternating: light triangles [0, 1), [1, 64), [64, 194)), a three-level hierarchy root > child > grandchild
    whose meshes have two primitives each, and 257 one-primitive fillers sharing a mesh.  Returns (path, {scene node name: glTF TRS})"""
    rng = np.random.default_rng(17)
    blob, views, accessors, meshes, nodes = b"", [], [], [], []

    def prim(nt, mat):
        nonlocal blob
        c = rng.uniform(-0.5, 0.5, (nt, 1, 3))
        pos = (c + rng.uniform(-0.12, 0.12, (nt, 3, 3)) + np.float32([0.2, 0, 0]) * np.arange(3).reshape(1, 3, 1)).astype(np.float32).reshape(-1, 3)
        nrm = np.tile(np.float32([0, 1, 0]), (3 * nt, 1))
        uv = rng.random((3 * nt, 2)).astype(np.float32)
        idx = np.arange(3 * nt, dtype=np.uint16)
        first = len(accessors)
        for data, comp, typ in ((pos, 5126, "VEC3"), (nrm, 5126, "VEC3"), (uv, 5126, "VEC2"), (idx, 5123, "SCALAR")):
            while len(blob) % 4:
                blob += b"\0"
            views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": data.nbytes})
            accessors.append({"bufferView": len(views) - 1, "componentType": comp, "count": len(data), "type": typ})
            blob += data.tobytes()
        return {"attributes": {"POSITION": first, "NORMAL": first + 1, "TEXCOORD_0": first + 2}, "indices": first + 3, "material": mat}

    trs = {}
    counts = [PLAIN_TRIS[0], LIGHT_TRIS[0], PLAIN_TRIS[1], LIGHT_TRIS[1], PLAIN_TRIS[2], LIGHT_TRIS[2], PLAIN_TRIS[3]]
    for k, nt in enumerate(counts):
        meshes.append({"primitives": [prim(nt, k % 2)]})
        t, q, s = trs[f"base{k}"] = _node_trs(k)
        nodes.append({"mesh": k, "translation": t, "rotation": q, "scale": s})
    for j, name in enumerate(("root", "child", "grandchild")):
        meshes.append({"primitives": [prim(3, 0), prim(2, 0)]})
        t, q, s = trs[name] = _node_trs(7 + j)
        n = {"mesh": 7 + j, "translation": t, "rotation": q, "scale": s}
        if j < 2:
            n["children"] = [7 + j + 1]
        nodes.append(n)
    meshes.append({"primitives": [prim(2, 0)]})
    for f in range(NUM_FILLERS):
        t, q, s = trs[f"filler{f}"] = _node_trs(10 + f)
        nodes.append({"mesh": 10, "translation": t, "rotation": q, "scale": s})
    (tmp_path / "geo.bin").write_bytes(blob)
    roots = list(range(7)) + [7] + list(range(10, 10 + NUM_FILLERS))
    g = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": roots}], "nodes": nodes, "meshes": meshes,
         "materials": [{"name": "plain", "pbrMetallicRoughness": {"baseColorFactor": [0.7, 0.6, 0.5, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.6}, "doubleSided": True},
                       {"name": "light", "emissiveFactor": [1.0, 0.8, 0.6], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 6.0}},
                        "pbrMetallicRoughness": {"metallicFactor": 0}, "doubleSided": True}],
         "buffers": [{"uri": "geo.bin", "byteLength": len(blob)}], "bufferViews": views, "accessors": accessors}
    p = tmp_path / "anim_scene.gltf"
    p.write_text(json.dumps(g))
    return str(p), trs


REF_GLTF = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests", "golden", "cornell_gltf")


def cornell_animated(tmp_path, edit=None, name="cornell_animated"):
    """the animated Cornell fixture (tools/make_anim_gltf.py) laid out as the scene references its files; edit(gltf dict) changes the JSON first"""
    for f in ("cornell.bin", "cornell_anim.bin"):
        if not (tmp_path / f).exists():
            shutil.copy(os.path.join(REF_GLTF, f), tmp_path / f)
    if not (tmp_path / "compressed").exists():
        (tmp_path / "compressed").mkdir()
        with gzip.open(os.path.join(REF_GLTF, "compressed", "checkerboard.dds.gz"), "rb") as src:
            (tmp_path / "compressed" / "checkerboard.dds").write_bytes(src.read())
    g = json.load(open(os.path.join(REF_GLTF, "cornell_animated.gltf")))
    if edit is not None:
        edit(g)
    p = tmp_path / (name + ".gltf")
    p.write_text(json.dumps(g))
    return str(p)


IDENTITY = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


class Builder:
    """a closure table built node by node (a parent before its children)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.nodes, self.keys, self.inst_idx, self.inst_node = [], [], [], []

    def node(self, rest, instances, parent=wire.ANIM_ROOT, animated=True, template=None, loop=None, t0=None):
        k = len(self.nodes)
        n = np.zeros((), wire.ANIM_NODE)
        n["parent"], n["parent_world"] = parent, IDENTITY
        n["rest_scale"], n["rest_rotation"], n["rest_translation"] = rest
        if animated:
            times = KEY_TIMES[k % 3 if template is None else template]
            n["first_key"], n["num_keys"] = len(self.keys), len(times)
            n["loop"] = (k // 3) % 2 if loop is None else loop
            n["t0"] = (0.0, 0.0, 0.375)[(k // 2) % 3] if t0 is None else t0
            for tm in times:
                key = np.zeros((), wire.KEYFRAME)
                key["scale"] = rest[0] * self.rng.uniform(0.6, 1.5, 3).astype(np.float32)
                key["rotation"] = _quat(self.rng)
                key["translation"] = rest[2] + self.rng.uniform(-0.4, 0.4, 3).astype(np.float32)
                key["time"] = tm
                self.keys.append(key)
        self.nodes.append(n)
        for i in instances:
            self.inst_idx.append(i); self.inst_node.append(k)
        return k

    def desc(self):
        keys = np.array(self.keys, wire.KEYFRAME) if self.keys else np.zeros(0, wire.KEYFRAME)
        return wire.AnimDesc(np.array(self.nodes, wire.ANIM_NODE), keys, self.inst_idx, self.inst_node)


def hierarchy(b, trs):
    """animated root, static child, animated grandchild, two instances per node"""
    r = b.node(rest_of(trs["root"]), HIER_INST["root"], template=1, loop=1, t0=0.0)
    c = b.node(rest_of(trs["child"]), HIER_INST["child"], parent=r, animated=False)
    g = b.node(rest_of(trs["grandchild"]), HIER_INST["grandchild"], parent=c, template=2, loop=0, t0=0.375)
    return r, c, g


def animation(trs, n_animated, seed=5):
    """a table with n_animated animated nodes: 1 -> the 63-triangle light alone; 63 -> the three lights + fillers; 65 and more -> the hierarchy (2
    animated nodes + its static child) + the three lights + fillers, the fillers listed from the last one down (a list that is not in index order)"""
    b = Builder(seed)
    if n_animated == 1:
        b.node(rest_of(trs["base3"]), [3], template=1, loop=1, t0=0.0)
        return b.desc()
    left = n_animated
    if n_animated >= 65:
        hierarchy(b, trs)
        left -= 2
    for i in LIGHTS[::-1]:
        b.node(rest_of(trs[f"base{i}"]), [i])
    left -= 3
    for f in range(NUM_FILLERS - 1, NUM_FILLERS - 1 - left, -1):
        b.node(rest_of(trs[f"filler{f}"]), [FILLER0 + f])
    d = b.desc()
    assert int((d.nodes["num_keys"] > 0).sum()) == n_animated
    return d


# ---------------------------------------------------------------------------------------------------------------- the host path
def sio():
    L = scene_io._sceneio_lib()
    vp = C.c_void_p
    L.zrh_scene_data_begin_frame.argtypes = [vp]
    L.zrh_scene_data_set_instance_world.argtypes = [vp, C.c_uint32, vp]
    L.zrh_scene_data_dirty_emissives.argtypes = [vp] * 3
    L.zrh_scene_data_initial_emissives.restype = vp
    L.zrh_scene_data_initial_emissives.argtypes = [vp]
    L.zrh_scene_data_from_desc.argtypes = [vp] * 3
    L.zrh_scene_data_set_animation.argtypes = [vp, vp]
    L.zrh_scene_data_animation.argtypes = [vp]
    L.zrh_scene_data_animation.restype = C.POINTER(wire.AnimDescC)
    L.zrh_scene_data_animate.argtypes = [vp, C.c_float]
    L.zrh_compose_world.argtypes = [vp] * 5
    return L


class HostData:
    """a zrh_scene_data and numpy views of the arrays it maintains"""

    def __init__(self, handle):
        L = sio()
        self.h = handle
        d = L.zrh_scene_data_desc(handle).contents
        self.n, self.ne = d.num_instances, d.num_emissives
        self.inst = np.ctypeslib.as_array(C.cast(d.instances, C.POINTER(C.c_uint8)), (self.n * wire.MESH_INSTANCE.itemsize,)).view(wire.MESH_INSTANCE)
        self.world = np.ctypeslib.as_array(C.cast(d.instance_to_world, C.POINTER(C.c_float)), (self.n, 12))
        if self.ne:
            self.ems = np.ctypeslib.as_array(C.cast(d.emissives, C.POINTER(C.c_uint8)), (self.ne * 48,)).view(wire.EMISSIVE_TRI)
            self.init = np.ctypeslib.as_array(C.cast(L.zrh_scene_data_initial_emissives(handle), C.POINTER(C.c_uint8)), (self.ne * 48,)).view(wire.EMISSIVE_TRI).copy()
        else:
            self.ems = self.init = np.zeros(0, wire.EMISSIVE_TRI)

    @classmethod
    def from_gltf(cls, path):
        L = sio()
        rho, dim = scene_io.load_rho_default()
        rho = np.ascontiguousarray(rho, np.uint16)
        h = C.c_void_p()
        assert L.zrh_gltf_load(os.fsencode(path), rho.ctypes.data, (C.c_uint32 * 3)(*dim), C.byref(h)) == 0, L.zrh_scene_io_last_error()
        return cls(h)

    @classmethod
    def from_scene(cls, sc):
        L = sio()
        desc = sc.desc()
        init = np.ascontiguousarray(sc.emissives_initial, wire.EMISSIVE_TRI)
        h = C.c_void_p()
        assert L.zrh_scene_data_from_desc(C.addressof(desc), init.ctypes.data, C.byref(h)) == 0, L.zrh_scene_io_last_error()
        return cls(h)

    def set_animation(self, desc):
        """0, or -1 with zrh_scene_io_last_error()"""
        if desc is None:
            return sio().zrh_scene_data_set_animation(self.h, None)
        d = desc.c_desc()
        return sio().zrh_scene_data_set_animation(self.h, C.addressof(d))

    def frame(self, t=None, moved=()):
        """the host's frame: begin_frame, (the animation at time t), set_instance_world for `moved` in list order; returns the dirty light range"""
        L = sio()
        L.zrh_scene_data_begin_frame(self.h)
        if t is not None:
            assert L.zrh_scene_data_animate(self.h, t) == 0, L.zrh_scene_io_last_error()
        for i, M in moved:
            assert L.zrh_scene_data_set_instance_world(self.h, i, np.ascontiguousarray(M, np.float32).ctypes.data) == 0
        first, count = C.c_uint32(), C.c_uint32()
        L.zrh_scene_data_dirty_emissives(self.h, C.byref(first), C.byref(count))
        return first.value, count.value

    def apply(self, scene, t=None, moved=(), stream=False):
        """... handed to the device scene in the host form: the dirty light records, then all instance records and matrices"""
        first, count = self.frame(t, moved)
        if count:
            scene.update_emissives(self.ems[first:first + count].copy(), first, stream=stream)
        scene.update_instances(self.inst.copy(), self.world.copy(), stream=stream)

    def close(self):
        if self.h:
            sio().zrh_scene_data_destroy(self.h)
            self.h = None
