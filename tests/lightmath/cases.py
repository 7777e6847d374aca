"""What the deformed-light tests share (tests/test_deformed_lights_cpu.py, tests/test_deformed_lights_gpu.py): the skinning tests' scene (the Cornell box plus
two tubes, tests/skinmath/cases.py) with both tubes EMISSIVE, the numpy restatement of which light triangles a set of vertex ranges touches, and the host
form the device form is held to."""
import ctypes as C

import numpy as np

from tests.animmath import cases as acases
from tests.morphmath import cases as mcases
from tests.skinmath import cases as scases
from zetaray_amd import scene_io, wire

F32 = np.float32
NONE = 0xFFFFFFFF
LAMP, TUBE0, TUBE1 = 6, 10, 11      # instances: the Cornell box's lamp (a rigid light), the two tubes
TUBE_TRIS = 2 * (scases.TUBE_RINGS - 1) * scases.TUBE_SEGS      # 2 112


def lit_world(ownerless=0):
    """skinned_cornell(1) with the tubes emissive (the lamp's material).  Light triangles: tube 0's [0, 2112), the lamp's two [2112, 2114) -- rigid lights of
    another instance between the deformable ones -- `ownerless` records no instance carries, then tube 1's.  Every record is zrh_emissive_from_vertices of the
    lamp's record (a new ID each) at the rest pose.  Returns (scene, [first vertex of each tube], {instance: first light triangle})"""
    sc, firsts = scases.skinned_cornell(1)
    lamp = sc.emissives.copy()
    lamp_init = sc.emissives_initial.copy()
    assert len(lamp) == 2 and int(sc.instances[LAMP]["base_emissive_tri_offset"]) == 0
    base = {TUBE0: 0, LAMP: TUBE_TRIS, TUBE1: TUBE_TRIS + 2 + ownerless}
    n = 2 * TUBE_TRIS + 2 + ownerless
    world, obj = np.zeros(n, wire.EMISSIVE_TRI), np.zeros(n, wire.EMISSIVE_TRI)
    world[TUBE_TRIS:TUBE_TRIS + 2], obj[TUBE_TRIS:TUBE_TRIS + 2] = lamp, lamp_init
    for j in range(ownerless):      # records of no instance: a copy of the lamp's, never to change
        world[TUBE_TRIS + 2 + j] = obj[TUBE_TRIS + 2 + j] = lamp[j % 2]
    for inst in (TUBE0, TUBE1):
        I = sc.instances[inst]
        sc.instances[inst]["base_emissive_tri_offset"] = base[inst]
        sc.instances[inst]["mat_idx"] = sc.instances[LAMP]["mat_idx"]
        sc.instance_mask[inst] = sc.instance_mask[LAMP]
        tri = light_vertices(sc, inst)
        for t in range(TUBE_TRIS):
            rec = lamp_init[0].copy()
            rec["id"] = 0x9E3779B1 * (inst * 4096 + t + 1) & 0xFFFFFFFF
            p = sc.vertices["pos"][tri[t]]
            obj[base[inst] + t], world[base[inst] + t] = scene_io.emissive_from_vertices(rec, p[0], p[1], p[2], sc.instance_to_world[inst])
    sc.instances[LAMP]["base_emissive_tri_offset"] = base[LAMP]
    sc.emissives, sc.emissives_initial = world, obj
    return sc, firsts, base


def _emissive_material(g):
    return next(i for i, m in enumerate(g["materials"]) if "emissiveFactor" in m or "KHR_materials_emissive_strength" in m.get("extensions", {}))


def emissive_morphed_gltf(tmp_path, name="cornell_morphed"):
    """the morph fixture with the face's material swapped for the file's emissive one"""
    def edit(g):
        mesh = next(m for m in g["meshes"] if any("targets" in p for p in m["primitives"]))
        mesh["primitives"][0]["material"] = _emissive_material(g)
    return mcases.morphed_gltf(tmp_path, edit=edit, name=name)


def emissive_skinned_gltf(tmp_path, name="cornell_skinned"):
    """the skin fixture with the skinned primitives' material swapped for the file's emissive one"""
    def edit(g):
        for n in g["nodes"]:
            if "skin" in n and "mesh" in n:
                for p in g["meshes"][n["mesh"]]["primitives"]:
                    p["material"] = _emissive_material(g)
    return scases.skinned_gltf(tmp_path, edit=edit, name=name)


def light_vertices(sc, inst):
    """(num_tris, 3) absolute vertex indices of the instance's triangles"""
    I = sc.instances[inst]
    nt = int(sc.instance_num_tris[inst])
    idx = sc.indices[int(I["base_idx_offset"]):int(I["base_idx_offset"]) + 3 * nt].astype(np.int64).reshape(nt, 3)
    return idx + int(I["base_vtx_offset"])


def listed_lights(sc, ranges):
    """the light triangles with a vertex in one of `ranges` [(first_vertex, num_vertices)], ascending -- what ScenePoseRebuild lists, restated"""
    out = []
    for inst in range(len(sc.instances)):
        b = int(sc.instances[inst]["base_emissive_tri_offset"])
        if b == NONE:
            continue
        v = light_vertices(sc, inst)
        hit = np.zeros(len(v), bool)
        for first, count in ranges:
            hit |= ((v >= first) & (v < first + count)).any(axis=1)
        out.append(b + np.nonzero(hit)[0])
    return np.sort(np.concatenate(out)) if out else np.zeros(0, np.int64)


def range_touching(sc, inst, n, parity):
    """a vertex range (first, count) of the instance that touches exactly n of its triangles; first has the given parity"""
    v = light_vertices(sc, inst)
    lo, hi = int(v.min()), int(v.max()) + 1
    # (on a tube an interior vertex adds triangles in pairs: the odd counts come from ranges that start in its first ring)
    for first in range(lo + (parity - lo) % 2, hi, 2):
        thr = np.sort(np.where(v >= first, v - first, 1 << 40).min(axis=1))      # the triangle is touched by ranges longer than this
        count = int(thr[n - 1]) + 1
        if count < (1 << 40) and (n == len(thr) or thr[n] >= count):
            assert len(listed_lights(sc, [(first, count)])) == n
            return first, count
    raise AssertionError(f"no range touches exactly {n} triangles")


def runs(tris):
    """[(first, count)] of the runs of consecutive indices"""
    tris = np.asarray(tris, np.int64)
    if not len(tris):
        return []
    cut = np.nonzero(np.diff(tris) != 1)[0] + 1
    return [(int(r[0]), len(r)) for r in np.split(tris, cut)]


def posed_vertices(anim, skin, morph, vertices, t):
    """the whole vertex array of the host form at time t (either set may be None)"""
    if morph is not None:
        return mcases.posed_scene_vertices(anim, skin, morph, vertices, t)
    out = vertices.copy()
    sk = scases.host_posed(anim, skin, scases.rest_of_ranges(skin, vertices), t)
    k = 0
    for r in skin.ranges:
        n = int(r["num_vertices"])
        out[int(r["first_vertex"]):int(r["first_vertex"]) + n] = sk[k:k + n]
        k += n
    return out


def set_ranges(skin, morph):
    return [(int(r["first_vertex"]), int(r["num_vertices"])) for d in (skin, morph) if d is not None for r in d.ranges]


def sio():
    L = acases.sio()
    L.zrh_scene_data_refresh_emissives.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    return L


def object_records(host):
    """the host data's object-space records as they stand now (HostData.init is a copy taken at creation)"""
    L = sio()
    return np.ctypeslib.as_array(C.cast(L.zrh_scene_data_initial_emissives(host.h), C.POINTER(C.c_uint8)), (host.ne * 48,)).view(wire.EMISSIVE_TRI).copy()


def apply_host_form(scene, host, sc, anim, skin, morph, t, stream=False):
    """the host sequence zr_scene_animate with deformed lights is held to: begin_frame; zrh_scene_data_animate(t); zr_scene_update_vertices with the posed
    ranges; zrh_scene_data_refresh_emissives over the listed light triangles from the posed vertex array; the host-form emissive and instance updates.
    Returns the posed vertex array"""
    L = sio()
    L.zrh_scene_data_begin_frame(host.h)
    assert L.zrh_scene_data_animate(host.h, t) == 0, L.zrh_scene_io_last_error()
    posed = np.ascontiguousarray(posed_vertices(anim, skin, morph, sc.vertices, t))
    ranges = set_ranges(skin, morph)
    for first, count in ranges:
        if count:
            scene.update_vertices(first, posed[first:first + count], stream=stream)
    for first, count in runs(listed_lights(sc, ranges)):
        assert L.zrh_scene_data_refresh_emissives(host.h, posed.ctypes.data, first, count) == 0, L.zrh_scene_io_last_error()
    first, count = C.c_uint32(), C.c_uint32()
    L.zrh_scene_data_dirty_emissives(host.h, C.byref(first), C.byref(count))
    if count.value:
        scene.update_emissives(host.ems[first.value:first.value + count.value].copy(), first.value, stream=stream)
    scene.update_instances(host.inst.copy(), host.world.copy(), stream=stream)
    return posed
