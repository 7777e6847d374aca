"""ctypes binding of tests/morphmath/libzmo.so (TEST-ONLY host compilation of include/zr_morph.h: morph_math.cpp)."""
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
            subprocess.check_call(["make", "-s", "-C", _HERE, "libzmo.so"])
            L = C.CDLL(os.path.join(_HERE, "libzmo.so"))
        vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
        L.zmo_sample_weights.argtypes = [vp, vp, u32, u32, f32, u32, f32, vp]
        L.zmo_sample_animation_tx.argtypes = [vp, u32, f32, u32, f32]
        L.zmo_sample_animation_tx.restype = f32
        L.zmo_morph_vertices.argtypes = [vp, vp, u32, vp, vp, vp, u32]
        L.zmo_num_weights.argtypes = [vp]
        L.zmo_num_weights.restype = u32
        L.zmo_eval_weights.argtypes = [vp, f32, vp]
        L.zmo_morph_ranges.argtypes = [vp] * 6
        L.zmo_validate.argtypes = [vp, vp, u32, vp, u32]
        _LIB = L
    return _LIB


def sample_weights(times, values, t0, loop, t):
    """values: (numKeys, numTargets), key-major"""
    times, values = np.ascontiguousarray(times, F32), np.ascontiguousarray(values, F32)
    values = values.reshape(len(times), -1)
    out = np.zeros(values.shape[1], F32)
    lib().zmo_sample_weights(times.ctypes.data, values.ctypes.data, len(times), values.shape[1], float(t0), int(loop), float(t), out.ctypes.data)
    return out


def sample_animation_tx(times, tx, t0, loop, t):
    """zran::SampleAnimation's translation.x for a keyframe track with these times that carries tx as translation.x"""
    keys = np.zeros(len(times), wire.KEYFRAME)
    keys["scale"], keys["rotation"], keys["time"] = 1, (0, 0, 0, 1), np.asarray(times, F32)
    keys["translation"][:, 0] = np.asarray(tx, F32)
    return F32(lib().zmo_sample_animation_tx(keys.ctypes.data, len(keys), float(t0), int(loop), float(t)))


def morph_vertices(rest, targets, weights, deltas):
    """vertex i of `rest` under the targets (MORPH_TARGET) with `weights`: it reads triple first_* + i of the pool `deltas` (n, 3)"""
    rest = np.ascontiguousarray(rest, wire.VERTEX).reshape(-1)
    targets = np.ascontiguousarray(targets, wire.MORPH_TARGET).reshape(-1)
    weights, deltas = np.ascontiguousarray(weights, F32).reshape(-1), np.ascontiguousarray(deltas, F32).reshape(-1, 3)
    assert len(weights) == len(targets)
    out = np.zeros(len(rest), wire.VERTEX)
    lib().zmo_morph_vertices(rest.ctypes.data, targets.ctypes.data, len(targets), weights.ctypes.data, deltas.ctypes.data, out.ctypes.data, len(rest))
    return out


def eval_weights(morph, t):
    d = morph.c_desc()
    W = np.zeros(lib().zmo_num_weights(C.addressof(d)), F32)
    lib().zmo_eval_weights(C.addressof(d), float(t), W.ctypes.data)
    return W


def morph_ranges(morph, W, rest, skin=None, J=None):
    """rest: the rest records of the morph ranges, range after range; returns the posed ones in that order.  skin + J (its joint matrices): a range that is
    also a skin range goes on through zrsk::SkinVertex"""
    d = morph.c_desc()
    k = skin.c_desc() if skin is not None else None
    W, rest = np.ascontiguousarray(W, F32), np.ascontiguousarray(rest, wire.VERTEX).reshape(-1)
    J = np.ascontiguousarray(J, F32) if J is not None else None
    assert len(rest) == int(morph.ranges["num_vertices"].sum())
    out = np.zeros(len(rest), wire.VERTEX)
    lib().zmo_morph_ranges(C.addressof(d), W.ctypes.data, C.addressof(k) if k is not None else None, J.ctypes.data if J is not None else None, rest.ctypes.data, out.ctypes.data)
    return out


def validate(morph, skin, scene_vertices, c_desc=None):
    """None, or the message.  c_desc: a MorphDescC to check in place of morph's own (null tables)"""
    d = c_desc if c_desc is not None else morph.c_desc()
    k = skin.c_desc() if skin is not None else None
    msg = C.create_string_buffer(256)
    return None if lib().zmo_validate(C.addressof(d), C.addressof(k) if k is not None else None, scene_vertices, msg, 256) == 0 else msg.value.decode()
