"""zr_scene_move_instances: the frame's scene update from matrices alone, its records computed on the device (zr_tu_scene_update.hip), against the
existing host path -- zrh_scene_data_begin_frame / _set_instance_world, then zr_scene_update_emissives + zr_scene_update_instances -- byte for byte:
device buffers, rendered frames, across streams, with the background SAH rebuild, and the calls it refuses."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
RPT_PLANES = ("A", "B", "C", "D", "E", "F", "G", "neighbor", "map_ctn", "map_ntc")


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


def _sio():
    L = scene_io._sceneio_lib()
    L.zrh_scene_data_begin_frame.argtypes = [C.c_void_p]
    L.zrh_scene_data_set_instance_world.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.zrh_scene_data_dirty_emissives.argtypes = [C.c_void_p] * 3
    L.zrh_scene_data_initial_emissives.restype = C.c_void_p
    L.zrh_scene_data_initial_emissives.argtypes = [C.c_void_p]
    L.zrh_scene_data_from_desc.argtypes = [C.c_void_p] * 3
    return L


class HostData:
    """a zrh_scene_data and numpy views of the arrays it maintains"""

    def __init__(self, handle):
        L = _sio()
        self.h = handle
        d = L.zrh_scene_data_desc(handle).contents
        self.n, self.ne = d.num_instances, d.num_emissives
        self.inst = np.ctypeslib.as_array(C.cast(d.instances, C.POINTER(C.c_uint8)), (self.n * wire.MESH_INSTANCE.itemsize,)).view(wire.MESH_INSTANCE)
        self.world = np.ctypeslib.as_array(C.cast(d.instance_to_world, C.POINTER(C.c_float)), (self.n, 12))
        self.ems = np.ctypeslib.as_array(C.cast(d.emissives, C.POINTER(C.c_uint8)), (self.ne * 48,)).view(wire.EMISSIVE_TRI)
        self.init = np.ctypeslib.as_array(C.cast(L.zrh_scene_data_initial_emissives(handle), C.POINTER(C.c_uint8)), (self.ne * 48,)).view(wire.EMISSIVE_TRI).copy()

    @classmethod
    def from_gltf(cls, path):
        L = _sio()
        rho, dim = scene_io.load_rho_default()
        rho = np.ascontiguousarray(rho, np.uint16)
        h = C.c_void_p()
        assert L.zrh_gltf_load(os.fsencode(path), rho.ctypes.data, (C.c_uint32 * 3)(*dim), C.byref(h)) == 0, L.zrh_scene_io_last_error()
        return cls(h)

    @classmethod
    def from_scene(cls, sc):
        L = _sio()
        desc = sc.desc()
        init = np.ascontiguousarray(sc.emissives_initial, wire.EMISSIVE_TRI)
        h = C.c_void_p()
        assert L.zrh_scene_data_from_desc(C.addressof(desc), init.ctypes.data, C.byref(h)) == 0, L.zrh_scene_io_last_error()
        return cls(h)

    def frame(self, moved):
        """the host's frame: begin_frame, set_instance_world in list order; returns the dirty light range"""
        L = _sio()
        L.zrh_scene_data_begin_frame(self.h)
        for i, M in moved:
            assert L.zrh_scene_data_set_instance_world(self.h, i, np.ascontiguousarray(M, np.float32).ctypes.data) == 0
        first, count = C.c_uint32(), C.c_uint32()
        L.zrh_scene_data_dirty_emissives(self.h, C.byref(first), C.byref(count))
        return first.value, count.value

    def apply(self, scene, moved, stream=False):
        """... handed to the device scene the existing way: the dirty light records, then all instance records and matrices"""
        first, count = self.frame(moved)
        if count:
            scene.update_emissives(self.ems[first:first + count].copy(), first, stream=stream)
        scene.update_instances(self.inst.copy(), self.world.copy(), stream=stream)

    def close(self):
        if self.h:
            _sio().zrh_scene_data_destroy(self.h)
            self.h = None


def _move(scene, moved, stream=False):
    scene.move_instances([i for i, _ in moved], [np.asarray(M, np.float32).reshape(12) for _, M in moved], stream=stream)


# ---------------------------------------------------------------------------------------------------------------- the scene of checks 1, 4, 5
LIGHT_TRIS = (1, 63, 130)      # the owner array changes inside a wave (1) and inside a block (1 + 63 = 64, 64 + 130 = 194)
PLAIN_TRIS = (24, 40, 30, 36)


def _write_scene(tmp_path):
    """7 instances: plain, light (1 triangle), plain, light (63), plain, light (130), plain -- light triangles [0, 1), [1, 64), [64, 194)"""
    rng = np.random.default_rng(17)
    counts = [PLAIN_TRIS[0], LIGHT_TRIS[0], PLAIN_TRIS[1], LIGHT_TRIS[1], PLAIN_TRIS[2], LIGHT_TRIS[2], PLAIN_TRIS[3]]
    blob, views, accessors, meshes, nodes = b"", [], [], [], []
    for k, nt in enumerate(counts):
        c = rng.uniform(-0.5, 0.5, (nt, 1, 3))
        pos = (c + rng.uniform(-0.12, 0.12, (nt, 3, 3)) + np.float32([0.2, 0, 0]) * np.arange(3).reshape(1, 3, 1)).astype(np.float32).reshape(-1, 3)
        nrm = np.tile(np.float32([0, 1, 0]), (3 * nt, 1))
        uv = rng.random((3 * nt, 2)).astype(np.float32)
        idx = np.arange(3 * nt, dtype=np.uint16)
        for data, comp, typ in ((pos, 5126, "VEC3"), (nrm, 5126, "VEC3"), (uv, 5126, "VEC2"), (idx, 5123, "SCALAR")):
            while len(blob) % 4:
                blob += b"\0"
            views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": data.nbytes})
            accessors.append({"bufferView": len(views) - 1, "componentType": comp, "count": len(data), "type": typ})
            blob += data.tobytes()
        meshes.append({"primitives": [{"attributes": {"POSITION": 4 * k, "NORMAL": 4 * k + 1, "TEXCOORD_0": 4 * k + 2}, "indices": 4 * k + 3, "material": k % 2}]})
        a = 0.3 * k
        nodes.append({"mesh": k, "translation": [float(-1.5 + 0.5 * k), float(0.6 + 0.2 * (k % 3)), float(0.3 * (k % 2))],
                      "rotation": [0.0, float(np.sin(a / 2)), 0.0, float(np.cos(a / 2))], "scale": [1.0 + 0.1 * k] * 3})
    (tmp_path / "geo.bin").write_bytes(blob)
    g = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": list(range(len(counts)))}], "nodes": nodes, "meshes": meshes,
         "materials": [{"name": "plain", "pbrMetallicRoughness": {"baseColorFactor": [0.7, 0.6, 0.5, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.6}, "doubleSided": True},
                       {"name": "light", "emissiveFactor": [1.0, 0.8, 0.6], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 6.0}},
                        "pbrMetallicRoughness": {"metallicFactor": 0}, "doubleSided": True}],
         "buffers": [{"uri": "geo.bin", "byteLength": len(blob)}], "bufferViews": views, "accessors": accessors}
    p = tmp_path / "seven.gltf"
    p.write_text(json.dumps(g))
    return str(p)


def _matrix(rng, k):
    """translation, rotation about a changing axis and non-uniform scale (object-space scale: R x diag(s), which decomposes without shear)"""
    ang = rng.uniform(-3.0, 3.0)
    ax = k % 3
    R = np.eye(3)
    a, b = [(1, 2), (2, 0), (0, 1)][ax]
    R[a, a], R[a, b], R[b, a], R[b, b] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
    M = np.zeros((3, 4), np.float32)
    M[:, :3] = (R @ np.diag(rng.uniform(0.5, 1.6, 3))).astype(np.float32)
    M[:, 3] = (np.float32([-1.5 + 0.5 * k, 0.8, 0.2]) + rng.uniform(-0.3, 0.3, 3)).astype(np.float32)
    return M


def _schedule():
    """the six frames of the buffer-parity check: (instance, matrix) lists in list order"""
    rng = np.random.default_rng(23)
    plain, la, lb, lc = 0, 1, 3, 5
    frames = [[], [(2, _matrix(rng, 2))], [(lb, _matrix(rng, lb))],
              [(lc, _matrix(rng, lc)), (4, _matrix(rng, 4)), (la, _matrix(rng, la))],      # descending index order
              [], [(i, _matrix(rng, i)) for i in range(7)]]
    return frames


def _assert_buffers(B, A, host, what):
    for which in (0, 1):
        ib, xb = B.download_instances(which)
        ia, xa = A.download_instances(which)
        assert ib.tobytes() == ia.tobytes(), f"{what}: instance buffer {which} differs from the host path's"
        assert xb.tobytes() == xa.tobytes(), f"{what}: toWorld differs from the host path's"
    ib, xb = B.download_instances(0)
    assert ib.tobytes() == host.inst.tobytes(), f"{what}: current records differ from zrh_scene_data's"
    assert xb.tobytes() == host.world.tobytes(), f"{what}: toWorld differs from zrh_scene_data's"
    eb = B.download_emissives()
    assert eb.tobytes() == A.download_emissives().tobytes(), f"{what}: emissive records differ from the host path's"
    assert eb.tobytes() == host.ems.tobytes(), f"{what}: emissive records differ from zrh_scene_data's"


def test_device_records_equal_the_host_path_in_every_buffer(api, tmp_path):
    """check 1: two scenes from one description, A driven by the host path, B by move_instances, six frames (nothing / one plain instance / the
    63-triangle light alone, a dirty range [1, 64) / the 1- and 130-triangle lights with the unmoved 63 between them plus a plain instance, listed in
    descending order / nothing / all seven): both instance buffers, toWorld and the emissive records equal A's and the host's own arrays"""
    path = _write_scene(tmp_path)
    sc, _ = scene_io.load_gltf_native(path)
    host = HostData.from_gltf(path)
    assert host.n == 7 and [int(x) for x in host.inst["base_emissive_tri_offset"]] == [NONE, 0, NONE, 1, NONE, 64, NONE] and host.ne == 194
    A, B = api.Scene(sc), api.Scene(sc)
    B.set_object_emissives(host.init)
    before = B.download_emissives()
    for f, moved in enumerate(_schedule(), 1):
        host.apply(A, moved)
        _move(B, moved)
        _assert_buffers(B, A, host, f"frame {f}")
    assert not np.array_equal(before.view(np.uint8), B.download_emissives().view(np.uint8))
    A.close(); B.close(); host.close()


def test_cpp_mirror_hands_over_matrices_alone(api, tmp_path):
    """the C++ mirror's per-frame scene step in its device form (zrh_scene_data_set_device_records, then the same zrh_scene_apply_updates the
    RenderGraph driver calls): the schedule of check 1, with one instance named twice in a frame, against the host form on a second scene"""
    path = _write_scene(tmp_path)
    sc, _ = scene_io.load_gltf_native(path)
    host, dev = HostData.from_gltf(path), HostData.from_gltf(path)
    A, B, B2 = api.Scene(sc), api.Scene(sc), api.Scene(sc)      # B2: one zrh_scene_data drives a second device scene as well
    L = _sio()
    L.zrh_scene_data_set_device_records.argtypes = [C.c_void_p, C.c_int]
    H = C.CDLL(os.path.join(ROOT, "zetaray_amd", "libzetaray_host.so"))
    H.zrh_scene_apply_updates.argtypes = [C.c_void_p, C.c_void_p]
    L.zrh_scene_data_set_device_records(dev.h, 1)
    for f, moved in enumerate(_schedule(), 1):
        if f == 4:
            moved = [(moved[0][0], moved[1][1])] + moved      # set twice: the last matrix holds, the previous one is still the frame's start
        host.apply(A, moved)
        dev.frame(moved)
        for X in (B, B2):
            assert H.zrh_scene_apply_updates(X.h, dev.h) == 0, api.lib().zr_last_error()
        api._check(api.lib().zr_device_synchronize(0))
        _assert_buffers(B, A, host, f"frame {f}")
        _assert_buffers(B2, A, host, f"frame {f}, second device scene")
    A.close(); B.close(); B2.close(); host.close(); dev.close()


def test_refused_calls_change_nothing(api, tmp_path):
    """check 5: an index >= n, an index listed twice, a null pointer with n_moved > 0 and a moved light before set_object_emissives each return their
    error and leave the device buffers as they were; the next valid call still gives the host path's bytes"""
    path = _write_scene(tmp_path)
    sc, _ = scene_io.load_gltf_native(path)
    host = HostData.from_gltf(path)
    A, B = api.Scene(sc), api.Scene(sc)
    frames = _schedule()
    L = api.lib()
    L.zr_scene_move_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    M = frames[2][0][1]

    def state():
        return [B.download_instances(0), B.download_instances(1), B.download_emissives()]

    def same(a, b):
        return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for p, q in zip(a[:2], b[:2]) for x, y in zip(p, q)) and a[2].tobytes() == b[2].tobytes()

    s0 = state()
    py0 = (B.version, B.instances_in_motion)
    with pytest.raises(api.ZetaRayError) as e:       # the 63-triangle light before its object-space records were handed over
        _move(B, frames[2])
    assert e.value.code == 6 and "zr_scene_set_object_emissives" in str(e.value) and same(s0, state())
    assert (B.version, B.instances_in_motion) == py0      # ... nor does the Python mirror's own state change
    B.set_object_emissives(host.init)
    host.apply(A, frames[1]); _move(B, frames[1])
    _assert_buffers(B, A, host, "first valid frame")
    s1, py1 = state(), (B.version, B.instances_in_motion)
    for bad, code, word in (([(7, M)], 1, "instance 7"), ([(3, M), (2, M), (3, M)], 1, "twice")):
        with pytest.raises(api.ZetaRayError) as e:
            _move(B, bad)
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert same(s1, state()), word
        assert (B.version, B.instances_in_motion) == py1
    idx = np.array([2], np.uint32)
    for ip, xp in ((None, np.ascontiguousarray(M).ctypes.data), (idx.ctypes.data, None)):
        assert L.zr_scene_move_instances(B.h, ip, xp, 1) == 1 and b"null" in L.zr_last_error()
        assert same(s1, state())
    host.apply(A, frames[3]); _move(B, frames[3])
    _assert_buffers(B, A, host, "valid frame after the refusals")
    A.close(); B.close(); host.close()


def test_object_space_texture_indices_are_held_to_the_table_bounds(api, tmp_path):
    """a moved light's record takes its emissive texture index from the object-space record: an index outside the scene's texture heap is caught by the
    descriptor-table check of the next render, as it is for a record handed to zr_scene_update_emissives -- never sampled"""
    path = _write_scene(tmp_path)
    sc, _ = scene_io.load_gltf_native(path)
    host = HostData.from_gltf(path)
    assert len(sc.textures) == 0
    w, h = 32, 32
    cb = scene_io.make_frame_constants(w, h, frame_num=1, num_emissives=len(sc.emissives), cam_pos=(0.0, 1.0, -4.0))
    bad = host.init.copy()
    bad["packed_b"][70] = (int(bad["packed_b"][70]) & 0xFFFF0000) | 3      # one triangle of the 130-triangle light names texture 3 of an empty heap
    msgs = []
    for how in ("host", "device"):
        r = api.Renderer(sc, w, h)
        r.render_frame(cb)
        M = _schedule()[3][0][1]
        if how == "host":
            rec = scene_io.emissive_to_world(bad[64:194], M)
            r.scene.update_emissives(rec, 64)
        else:
            r.scene.set_object_emissives(bad)
            r.scene.move_instances([5], [M.reshape(12)])
        with pytest.raises(api.ZetaRayError) as e:
            r.render_frame(cb)
        assert e.value.code == 1 and "texture table 3" in str(e.value), str(e.value)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    host.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from zetaray_amd import api, scene_io
sc, _ = scene_io.load_gltf_native(sys.argv[2])
s = api.Scene(sc)
before = s.download_instances(0)[0].tobytes()
M = np.float32([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0]])
try:
    s.move_instances([0], [M.reshape(12)])
    print("NOT REFUSED")
except api.ZetaRayError as e:
    print("refused", e.code, "unchanged" if s.download_instances(0)[0].tobytes() == before else "CHANGED", str(e))
"""


@pytest.mark.parametrize("mode", ["rebuild", "rebuild_host"])
def test_rebuild_modes_are_refused(api, tmp_path, mode):
    """check 5, the host-synchronous update modes: ZR_SCENE_UPDATE set for a fresh child process, not for this one"""
    path = _write_scene(tmp_path)
    env = dict(os.environ, ZR_SCENE_UPDATE=mode)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("refused 5 unchanged") and mode in out.stdout, out.stdout


def test_background_sah_rebuild_under_the_device_form(api, tmp_path):
    """check 4: zr_scene_set_background_rebuild on B only; the scene of check 1 (324 triangles: the host builder makes a tree of it, bvh_info has
    nodes, so builds are started) moves until a background tree has been installed -- G-buffer planes and the path-traced image stay A's, and B's
    buffers the host path's.  No install within 40 frames fails the test."""
    path = _write_scene(tmp_path)
    sc, _ = scene_io.load_gltf_native(path)
    host = HostData.from_gltf(path)
    w, h = 96, 64
    prm = wire.default_params()
    ra, rb = api.Renderer(sc, w, h, params=prm), api.Renderer(sc, w, h, params=prm)
    assert sc.num_tris > 8 and rb.scene.bvh_info()[0] > 0      # more than one leaf: the builder has a tree to build
    rb.scene.set_background_rebuild(True)
    rb.scene.set_object_emissives(host.init)
    rng = np.random.default_rng(31)
    prev, installed, f = None, 0, 0
    while installed < 1 and f < 40:
        f += 1
        moved = [(i, _matrix(rng, i)) for i in ((f % 7), ((f + 3) % 7))] if f > 1 else []
        host.apply(ra.scene, moved)
        _move(rb.scene, moved)
        t0 = time.perf_counter()
        while rb.scene.background_rebuild_stats()[2] == 1 and time.perf_counter() - t0 < 20.0:      # (the builder's thread: a deterministic schedule)
            time.sleep(0.002)
        cb = scene_io.make_frame_constants(w, h, frame_num=f, num_emissives=len(sc.emissives), cam_pos=(0.0, 1.0, -4.0))
        if prev is not None:
            cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
        prev = cb.copy()
        ra.render_frame(cb); rb.render_frame(cb)
        pa, pb = ra.gbuffer.download()[0], rb.gbuffer.download()[0]
        for nm, a, b in zip(wire.GB_PLANE_NAMES, pa, pb):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), f"frame {f}: G-buffer plane {nm}"
        assert ra.final().tobytes() == rb.final().tobytes(), f"frame {f}: FINAL"
        _assert_buffers(rb.scene, ra.scene, host, f"frame {f}")
        installed = rb.scene.background_rebuild_stats()[1]
    assert installed >= 1, f"no background tree installed within {f} frames: {rb.scene.background_rebuild_stats()}"
    host.close()


# ---------------------------------------------------------------------------------------------------------------- the moving Cornell light
W, H = 96, 64


def _light_motion(sc, frames):
    """the motion of test_moving_light_on_gpu (tests/test_gpu_parity.py), stated again: the light quad translates by (0.05, -0.02, 0.03) and turns by
    0.2 rad about y per frame from frame 2 on.  Returns (light instance, {frame: its 3 x 4 world matrix})"""
    idx = [i for i in range(len(sc.instances)) if sc.instances["base_emissive_tri_offset"][i] != NONE][0]
    scratch = copy.deepcopy(sc)
    t0, xf, out = scratch.instances["translation"][idx].copy(), {}, {}
    for f in range(2, frames + 1):
        a = 0.2 * (f - 1)
        scene_io.move_instance(scratch, idx, translation=t0 + np.float32([0.05 * (f - 1), -0.02 * (f - 1), 0.03 * (f - 1)]),
                               rotation=np.array([0.0, np.sin(a / 2), 0.0, np.cos(a / 2)], np.float32), xform_of=xf)
        out[f] = np.array(scratch.instance_to_world[idx], np.float32).reshape(3, 4).copy()
    return idx, out


def _cornell():
    return scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_emissive.npz"))


def _cb(sc, f, prev):
    cb = scene_io.make_frame_constants(W, H, frame_num=f, num_emissives=len(sc.emissives))
    if prev is not None:
        cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
    return cb


def _everything(r, di):
    out = {"final": r.final().copy(), "di": di.download().copy(), "counters": r.p_indirect.read_counters()}
    for nm, pl in zip(wire.GB_PLANE_NAMES, r.gbuffer.download()[0]):
        out["gb_" + nm] = np.asarray(pl).copy()
    for nm in RPT_PLANES:
        a = r.p_indirect.download_plane(nm)
        out["rpt_" + nm] = (a & 0xffffff) if nm == "A" else a
    return out


@pytest.fixture(scope="module")
def host_path_frames(api):
    """renderer A: six frames of the moving light through update_emissives + update_instances fed from zrh_scene_data_set_instance_world"""
    sc = _cornell()
    idx, mats = _light_motion(sc, 6)
    host = HostData.from_scene(sc)
    prm, dprm = wire.default_params(), wire.default_params_di()
    r = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    di = r.enable_direct(dprm)
    frames, prev = [], None
    for f in range(1, 7):
        if f >= 2:
            host.apply(r.scene, [(idx, mats[f])])
        cb = _cb(sc, f, prev)
        prev = cb.copy()
        r.p_indirect.read_counters(reset=True)
        r.render_frame(cb)
        frames.append(_everything(r, di))
    ems = r.scene.download_emissives()
    host.close()
    return frames, ems


def test_rendered_frames_equal_the_host_path(api, host_path_frames):
    """check 2: ReSTIR PT with emissive ReSTIR DI attached over the moving light; renderer B uses move_instances.  G-buffer planes, FINAL, the DI
    image, every reservoir plane (A masked like test_moving_light_on_gpu) and the ray counters identical every frame"""
    want, ems_a = host_path_frames
    sc = _cornell()
    idx, mats = _light_motion(sc, 6)
    prm, dprm = wire.default_params(), wire.default_params_di()
    r = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    di = r.enable_direct(dprm)
    r.scene.set_object_emissives(sc.emissives_initial)
    before = r.scene.download_emissives()
    prev = None
    for f in range(1, 7):
        if f >= 2:
            r.move_instances([idx], [mats[f].reshape(12)])
        cb = _cb(sc, f, prev)
        prev = cb.copy()
        r.p_indirect.read_counters(reset=True)
        r.render_frame(cb)
        got = _everything(r, di)
        for k, v in want[f - 1].items():
            if k == "counters":
                assert got[k] == v, f"frame {f}: ray counters"
            else:
                assert np.asarray(got[k]).tobytes() == np.asarray(v).tobytes(), f"frame {f}: {k}"
    after = r.scene.download_emissives()
    assert after.tobytes() == ems_a.tobytes()
    assert not np.array_equal(before.view(np.uint8), after.view(np.uint8))      # the light really moved
    assert float(want[-1]["di"][..., :3].max()) > 0


def test_stream_ordered_moves_across_streams(api, host_path_frames):
    """check 3: every move_instances ENQUEUED on one non-blocking stream, every frame rendered on another, six frames back to back without a host wait,
    images copied out on the render stream (the pattern of test_stream_ordered_scene_updates_across_streams): the images of check 2"""
    import torch
    want, _ = host_path_frames
    sc = _cornell()
    idx, mats = _light_motion(sc, 6)
    prm, dprm = wire.default_params(), wire.default_params_di()
    r = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    di = r.enable_direct(dprm)
    r.scene.set_object_emissives(sc.emissives_initial)
    s_upd, s_ren = torch.cuda.Stream(), torch.cuda.Stream()
    nbytes = W * H * 16
    hip_path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)      # the HIP runtime this process already uses
    hip = C.CDLL(hip_path)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    snaps, prev = [], None
    for f in range(1, 7):
        if f >= 2:
            i_dev, x_dev = np.array([idx], np.uint32), mats[f].reshape(1, 12).copy()
            r.scene.move_instances(i_dev, x_dev, stream=s_upd.cuda_stream)
            i_dev[:] = 0xffffffff; x_dev[:] = 0      # the caller's arrays may be reused at once (pinned staging ring)
        cb = _cb(sc, f, prev)
        prev = cb.copy()
        r.render_frame(cb, stream=s_ren.cuda_stream)
        snap = torch.zeros(2 * nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()          # the allocation's fill, not the renders
        pt_ptr, di_ptr = r.p_indirect.output_ptr()[0], di.output_ptr()[0]
        assert hip.hipMemcpyAsync(snap.data_ptr(), pt_ptr, nbytes, 3, s_ren.cuda_stream) == 0
        assert hip.hipMemcpyAsync(snap.data_ptr() + nbytes, di_ptr, nbytes, 3, s_ren.cuda_stream) == 0
        snaps.append(snap)
    torch.cuda.synchronize()
    for f, snap in enumerate(snaps, 1):
        got = snap.cpu().numpy().view(np.float32).reshape(2, H, W, 4)
        assert got[0].tobytes() == want[f - 1]["final"].tobytes(), f"frame {f}: ReSTIR PT"
        assert got[1].tobytes() == want[f - 1]["di"].tobytes(), f"frame {f}: ReSTIR DI"
