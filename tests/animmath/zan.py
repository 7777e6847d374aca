"""ctypes binding of tests/animmath/libzan.so (TEST-ONLY host compilation of include/zr_anim.h: anim_math.cpp)."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        import fcntl
        with open(os.path.join(_HERE, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-s", "-C", _HERE, "libzan.so"])
            L = C.CDLL(os.path.join(_HERE, "libzan.so"))
        vp, f32, u32 = C.c_void_p, C.c_float, C.c_uint32
        L.zan_slerp.argtypes = [vp, vp, vp, vp, vp, u32]
        L.zan_acos.argtypes = [f32]; L.zan_acos.restype = f32
        L.zan_sin.argtypes = [f32]; L.zan_sin.restype = f32
        L.zan_interpolate.argtypes = [vp, vp, f32, vp]
        L.zan_sample.argtypes = [vp, u32, f32, u32, f32, vp]
        L.zan_local_matrix.argtypes = [vp, vp]
        L.zan_compose_world.argtypes = [vp, vp, vp]
        L.zan_eval_node_worlds.argtypes = [vp, f32, vp]
        L.zan_validate.argtypes = [vp, u32, vp, vp, u32]
        _LIB = L
    return _LIB
