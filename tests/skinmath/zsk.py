"""ctypes binding of tests/skinmath/libzsk.so (TEST-ONLY host compilation of include/zr_skin.h: skin_math.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from zetaray_amd import wire

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
F32 = np.float32


def lib():
    global _LIB
    if _LIB is None:
        import fcntl
        with open(os.path.join(_HERE, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-s", "-C", _HERE, "libzsk.so"])
            L = C.CDLL(os.path.join(_HERE, "libzsk.so"))
        vp, u32 = C.c_void_p, C.c_uint32
        for name in ("zsk_joint_matrix", "zsk_blend", "zsk_position", "zsk_normal", "zsk_tangent", "zsk_pose_vertex"):
            getattr(L, name).argtypes = [vp, vp, vp, u32]
        L.zsk_decode.argtypes = [vp, vp, u32]
        L.zsk_encode.argtypes = [vp, vp, u32]
        L.zsk_eval_joint_matrices.argtypes = [vp, vp, vp]
        L.zsk_skin_ranges.argtypes = [vp, vp, vp, vp]
        L.zsk_validate.argtypes = [vp, u32, u32, vp, u32]
        _LIB = L
    return _LIB


def _call3(name, a, b, shape, dtype=F32):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    out = np.zeros(shape, dtype)
    getattr(lib(), name)(a.ctypes.data, b.ctypes.data, out.ctypes.data, shape[0] if isinstance(shape, tuple) else shape)
    return out


def joint_matrix(node_world, inverse_bind):
    w = np.ascontiguousarray(node_world, F32).reshape(-1, 12)
    return _call3("zsk_joint_matrix", w, np.ascontiguousarray(inverse_bind, F32).reshape(-1, 12), (len(w), 12))


def blend(J4, w):
    J4 = np.ascontiguousarray(J4, F32).reshape(-1, 4, 12)
    return _call3("zsk_blend", J4, np.ascontiguousarray(w, F32).reshape(-1, 4), (len(J4), 12))


def position(M, p):
    M = np.ascontiguousarray(M, F32).reshape(-1, 12)
    return _call3("zsk_position", M, np.ascontiguousarray(p, F32).reshape(-1, 3), (len(M), 3))


def normal(M, n):
    M = np.ascontiguousarray(M, F32).reshape(-1, 12)
    return _call3("zsk_normal", M, np.ascontiguousarray(n, F32).reshape(-1, 3), (len(M), 3))


def tangent(M, t):
    M = np.ascontiguousarray(M, F32).reshape(-1, 12)
    return _call3("zsk_tangent", M, np.ascontiguousarray(t, F32).reshape(-1, 3), (len(M), 3))


def decode(codes):
    c = np.ascontiguousarray(codes, np.uint16).reshape(-1, 2)
    out = np.zeros((len(c), 3), F32)
    lib().zsk_decode(c.ctypes.data, out.ctypes.data, len(c))
    return out


def encode(dirs):
    d = np.ascontiguousarray(dirs, F32).reshape(-1, 3)
    out = np.zeros((len(d), 2), np.uint16)
    lib().zsk_encode(d.ctypes.data, out.ctypes.data, len(d))
    return out


def pose_vertex(rest, M):
    rest = np.ascontiguousarray(rest, wire.VERTEX).reshape(-1)
    return _call3("zsk_pose_vertex", rest, np.ascontiguousarray(M, F32).reshape(-1, 12), len(rest), wire.VERTEX)


def eval_joint_matrices(skin, node_world):
    d = skin.c_desc()
    w = np.ascontiguousarray(node_world, F32)
    J = np.zeros((len(skin.joints), 12), F32)
    lib().zsk_eval_joint_matrices(C.addressof(d), w.ctypes.data, J.ctypes.data)
    return J


def skin_ranges(skin, J, rest):
    """rest: the rest records of the ranges, range after range; returns the posed ones in that order"""
    d = skin.c_desc()
    J, rest = np.ascontiguousarray(J, F32), np.ascontiguousarray(rest, wire.VERTEX).reshape(-1)
    assert len(rest) == int(skin.ranges["num_vertices"].sum())
    out = np.zeros(len(rest), wire.VERTEX)
    lib().zsk_skin_ranges(C.addressof(d), J.ctypes.data, rest.ctypes.data, out.ctypes.data)
    return out


def validate(skin, anim_nodes, scene_vertices):
    """None, or the message"""
    d = skin.c_desc()
    msg = C.create_string_buffer(256)
    return None if lib().zsk_validate(C.addressof(d), anim_nodes, scene_vertices, msg, 256) == 0 else msg.value.decode()
