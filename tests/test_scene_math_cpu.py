"""include/zr_scene_math.h -- the scene math the device form of the scene update compiles (zr_tu_scene_update.hip) -- compiled for the host on its
own (tests/scenemath) and held, byte for byte, against the host library's zrh_* entry points (zetaray_amd/host/zr_scene_io.cpp, pinned to the
reference's code by tests/test_scene_io.py) and, where oracle/_ref is built, against the reference's own code.  No GPU.

What these tests can and cannot show: the host library compiles the very same header with the same flags, so the `*_matches_the_host_library` tests
compare the header with itself and fail only where the header is missing or mis-wired (the parent commit, a wrapper that drops an argument).  The
independent pins of the math are the unchanged tests/test_scene_io.py (host library == the reference's code), test_header_math_matches_the_reference_code
below, and the comparison with scene_io.emissive_to_world; that the DEVICE compilation gives the same bytes is tests/test_scene_move_gpu.py's to show."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.scenemath import zsm
from tests.test_scene_io import ZREF, _Ref, _write_gltf, random_trs, sio
from zetaray_amd import scene_io, wire

IDENT = np.hstack([np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32)])


def _rot(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    R = np.eye(3)
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return R


def _branch(M):
    """the row quaternionFromRotationMat1 selects for the 3 x 4 matrix M: 0 / 1 / 2 = R00 / R11 / R22 dominant, 3 = the trace"""
    A = np.asarray(M, np.float64).reshape(3, 4)[:, :3]
    d = np.diag(A / np.linalg.norm(A, axis=0, keepdims=True))
    return (2 + (d[0] >= -d[1])) if d[2] >= 0 else int(d[1] >= d[0])


def matrices():
    """the matrices of tests/test_scene_io.py's transform test (random S / R / T chains composed by the host library), then rotations that take each
    of the four branches of the quaternion-from-matrix selection under scales from 1e-2 to 1e2"""
    L = sio()
    rng = np.random.default_rng(3)
    out = []
    for it in range(1500):
        mine = IDENT.copy()
        for level in range(3):
            s, q, t = random_trs(rng)
            if it % 7 == 0:
                q = np.array([0, 0, 0, 1], np.float32)
            if it % 5 == 0:
                s = np.full(3, s[0], np.float32)
            nxt = np.zeros((3, 4), np.float32)
            L.zrh_compose_world(s.ctypes.data, q.ctypes.data, t.ctypes.data, mine.ctypes.data, nxt.ctypes.data)
            mine = nxt
            out.append(mine.copy())
            if it % 5 != 0:
                break
    seen = set()
    for axis, want in ((0, 0), (1, 1), (2, 2), (None, 3)):
        for k in range(60):
            ang = rng.uniform(2.6, 3.1) * rng.choice([-1, 1]) if axis is not None else rng.uniform(-0.5, 0.5)
            R = _rot(axis if axis is not None else k % 3, ang) @ _rot((k + 1) % 3, rng.uniform(-0.05, 0.05))
            scale = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), 3)) if k % 2 else np.full(3, [1e-2, 1.0, 1e2][k % 3])
            M = np.zeros((3, 4), np.float32)
            M[:, :3] = (R @ np.diag(scale)).astype(np.float32)
            M[:, 3] = rng.uniform(-10, 10, 3).astype(np.float32)
            assert _branch(M) == want, (axis, k)
            seen.add(_branch(M))
            out.append(M)
    assert seen == {0, 1, 2, 3}
    return out


def triangles():
    """the object-space light records and matrices of tests/test_scene_io.py's emissive transform test"""
    L = sio()
    rng = np.random.default_rng(21)
    out = []
    for it in range(4000):
        v = (rng.normal(size=(3, 3)) * rng.choice([0.01, 0.3, 2.0, 30.0])).astype(np.float32)
        if it % 7 == 0:
            v[1] = v[0] + np.float32([rng.normal(), 0, 0])
        v0, v1, v2 = (np.ascontiguousarray(x) for x in v)
        uv = rng.random(6).astype(np.float32)
        e = np.zeros(1, wire.EMISSIVE_TRI)
        L.zrh_pack_emissive_triangle(v0.ctypes.data, v1.ctypes.data, v2.ctypes.data, uv.ctypes.data, 0x804020, 0xffff, 0x4000, it, 1, e.ctypes.data)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        sc = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), 3)) if it % 3 == 0 else rng.uniform(0.1, 3, 3)
        M = np.zeros((3, 4), np.float32)
        M[:, :3] = (q @ np.diag(sc)).astype(np.float32) if it % 11 else np.diag(sc).astype(np.float32)
        M[:, 3] = (rng.normal(size=3) * 5).astype(np.float32)
        out.append((e, M, v))
    return out


def _ref_layout(M):
    return np.ascontiguousarray(np.vstack([M[:, :3].T, M[:, 3][None, :]]).astype(np.float32))


def test_header_decomposition_matches_the_host_library():
    """DecomposeSRT / Unorm16FromNormalized / FillMeshInstance of the header == zrh_decompose_srt / zrh_fill_mesh_instance over the random chains and
    over every branch of the quaternion selection, scales 1e-2 .. 1e2"""
    L, Z = sio(), zsm.lib()
    for k, M in enumerate(matrices()):
        a, b = [np.zeros(n, np.float32) for n in (3, 4, 3)], [np.zeros(n, np.float32) for n in (3, 4, 3)]
        L.zrh_decompose_srt(M.ctypes.data, *(x.ctypes.data for x in a))
        Z.zsm_decompose_srt(M.ctypes.data, *(x.ctypes.data for x in b))
        for x, y, what in zip(a, b, ("scale", "quaternion", "translation")):
            assert x.tobytes() == y.tobytes(), (k, what, x, y)
        ia, ib = np.zeros(1, wire.MESH_INSTANCE), np.zeros(1, wire.MESH_INSTANCE)
        ia["mat_idx"] = ib["mat_idx"] = 7       # the other fields are kept
        L.zrh_fill_mesh_instance(M.ctypes.data, ia.ctypes.data)
        Z.zsm_fill_mesh_instance(M.ctypes.data, ib.ctypes.data)
        assert ia.tobytes() == ib.tobytes(), (k, ia, ib)
        u = np.zeros(4, np.uint16)
        Z.zsm_unorm16(b[1].ctypes.data, u.ctypes.data, 4)
        assert np.array_equal(u, ia["rotation"][0]), k


def test_header_emissive_transform_matches_the_host_library():
    """EmissiveToWorld (decode, three point transforms, normalise, re-encode) of the header == zrh_emissive_to_world; the inputs hold edges whose
    octahedral z is negative before and after the transform (the fold of the decode and of the encode)"""
    L, Z = sio(), zsm.lib()
    L.zrh_emissive_to_world.argtypes = [C.c_void_p] * 3
    folds_in = folds_out = 0
    for k, (e, M, v) in enumerate(triangles()):
        a, b = np.zeros(1, wire.EMISSIVE_TRI), np.zeros(1, wire.EMISSIVE_TRI)
        L.zrh_emissive_to_world(e.ctypes.data, M.ctypes.data, a.ctypes.data)
        Z.zsm_emissive_to_world(e.ctypes.data, M.ctypes.data, b.ctypes.data)
        assert a.tobytes() == b.tobytes(), (k, a, b)
        folds_in += int((v[1] - v[0])[2] < 0) + int((v[2] - v[0])[2] < 0)
        w = np.zeros(9, np.float32)
        Z.zsm_decode_emissive_vertices(b.ctypes.data, w.ctypes.data)
        w = w.reshape(3, 3)
        folds_out += int((w[1] - w[0])[2] < 0) + int((w[2] - w[0])[2] < 0)
        # ... and the decode + point transform on their own, against the Python statement the fixtures were made with
        assert scene_io.emissive_to_world(e, M).tobytes() == b.tobytes(), k
    assert folds_in > 1000 and folds_out > 1000, (folds_in, folds_out)


def test_header_record_update_matches_the_host_scene_maintenance(tmp_path):
    """the body of zrh_scene_data_begin_frame / _set_instance_world, as k_move_instances and k_move_emissives apply it per element (begin-frame rule for
    every record, set-world rule from the new and the previous matrix for a moved one, EmissiveToWorld of the object-space records of a moved light),
    against the host library over six frames of a loaded scene: all records, all matrices, the dirty light range"""
    L, Z = sio(), zsm.lib()
    L.zrh_scene_data_begin_frame.argtypes = [C.c_void_p]
    L.zrh_scene_data_set_instance_world.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.zrh_scene_data_dirty_emissives.argtypes = [C.c_void_p] * 3
    L.zrh_scene_data_initial_emissives.restype = C.c_void_p
    L.zrh_scene_data_initial_emissives.argtypes = [C.c_void_p]
    path, g, pos = _write_gltf(tmp_path)
    rho, dim = scene_io.load_rho_default()
    rho = np.ascontiguousarray(rho, np.uint16)
    h = C.c_void_p()
    assert L.zrh_gltf_load(os.fsencode(path), rho.ctypes.data, (C.c_uint32 * 3)(*dim), C.byref(h)) == 0
    d = L.zrh_scene_data_desc(h).contents
    n, ne = d.num_instances, d.num_emissives
    inst = np.ctypeslib.as_array(C.cast(d.instances, C.POINTER(C.c_uint8)), (n * wire.MESH_INSTANCE.itemsize,)).view(wire.MESH_INSTANCE)
    world = np.ctypeslib.as_array(C.cast(d.instance_to_world, C.POINTER(C.c_float)), (n, 12))
    ems = np.ctypeslib.as_array(C.cast(d.emissives, C.POINTER(C.c_uint8)), (ne * 48,)).view(wire.EMISSIVE_TRI)
    ntris = [int(C.cast(d.instance_num_tris, C.POINTER(C.c_uint32))[i]) for i in range(n)]
    init = np.ctypeslib.as_array(C.cast(L.zrh_scene_data_initial_emissives(h), C.POINTER(C.c_uint8)), (ne * 48,)).view(wire.EMISSIVE_TRI).copy()
    mine_inst, mine_world, mine_ems = inst.copy(), world.copy(), ems.copy()
    rng = np.random.default_rng(5)
    for frame in range(6):
        moved = {}
        for i in range(n):
            if frame in (0, 4) or rng.random() < 0.4:
                continue
            a = rng.uniform(-3.0, 3.0)
            s = np.exp(rng.uniform(np.log(1e-2), np.log(1e2))) if frame == 3 else rng.uniform(0.5, 2)
            M = np.zeros((3, 4), np.float32)
            M[:, :3] = (_rot(frame % 3, a) @ np.diag([s] * 3)).astype(np.float32)
            M[:, 3] = rng.uniform(-3, 3, 3).astype(np.float32)
            moved[i] = M
        L.zrh_scene_data_begin_frame(h)
        for i, M in moved.items():
            assert L.zrh_scene_data_set_instance_world(h, i, M.ctypes.data) == 0
        lo, hi = 0xffffffff, 0
        for i in range(n):
            rec = mine_inst[i:i + 1]
            M = moved.get(i)
            Z.zsm_move_instance(rec.ctypes.data, None if M is None else M.ctypes.data, mine_world[i].ctypes.data)
            if M is None:
                continue
            mine_world[i] = M.reshape(12)
            b = int(rec["base_emissive_tri_offset"][0])
            if b != 0xffffffff:
                for k in range(b, b + int(ntris[i])):
                    Z.zsm_emissive_to_world(init[k:k + 1].ctypes.data, M.ctypes.data, mine_ems[k:k + 1].ctypes.data)
                lo, hi = min(lo, b), max(hi, b + int(ntris[i]))
        assert mine_inst.tobytes() == inst.tobytes(), frame
        assert mine_world.tobytes() == world.tobytes(), frame
        assert mine_ems.tobytes() == ems.tobytes(), frame
        first, count = C.c_uint32(), C.c_uint32()
        L.zrh_scene_data_dirty_emissives(h, C.byref(first), C.byref(count))
        assert (first.value, count.value) == ((lo, hi - lo) if hi > lo else (0, 0)), frame
    L.zrh_scene_data_destroy(h)


@pytest.mark.skipif(not os.path.exists(ZREF), reason="oracle/_ref (the reference's own code) is not built on this machine")
def test_header_math_matches_the_reference_code():
    """the same matrices and light records through the reference's own FillMeshInstanceData / LoadVertices -> mul -> StoreVertices"""
    R, Z = _Ref(), zsm.lib()
    for k, M in enumerate(matrices()):
        if abs(np.linalg.det(M[:, :3].astype(np.float64))) < 1e-30:
            continue
        s3, q4, t3 = np.zeros(3, np.float32), np.zeros(4, np.float32), np.zeros(3, np.float32)
        Z.zsm_decompose_srt(M.ctypes.data, s3.ctypes.data, q4.ctypes.data, t3.ctypes.data)
        inst = np.zeros(1, wire.MESH_INSTANCE)
        Z.zsm_fill_mesh_instance(M.ctypes.data, inst.ctypes.data)
        rs, rq, rt, rrot, rscale = np.zeros(3, np.float32), np.zeros(4, np.float32), np.zeros(3, np.float32), np.zeros(4, np.uint16), np.zeros(3, np.uint16)
        ref = _ref_layout(M)
        R.zref_fill_mesh_instance(ref.ctypes.data, rs.ctypes.data, rq.ctypes.data, rt.ctypes.data, rrot.ctypes.data, rscale.ctypes.data)
        for a, b, what in ((s3, rs, "scale"), (q4, rq, "quaternion"), (t3, rt, "translation")):
            assert a.tobytes() == b.tobytes(), (k, what, a, b)
        assert np.array_equal(inst["rotation"][0], rrot) and np.array_equal(inst["scale"][0], rscale), k
    for k, (e, M, v) in enumerate(triangles()):
        a, b = np.zeros(1, wire.EMISSIVE_TRI), np.zeros(1, wire.EMISSIVE_TRI)
        Z.zsm_emissive_to_world(e.ctypes.data, M.ctypes.data, a.ctypes.data)
        ref = _ref_layout(M)
        R.zref_emissive_to_world(e.ctypes.data, ref.ctypes.data, b.ctypes.data)
        assert a.tobytes() == b.tobytes(), (k, a, b)
