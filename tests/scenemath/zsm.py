"""ctypes binding of tests/scenemath/libzsm.so (TEST-ONLY host compilation of include/zr_scene_math.h: scene_math.cpp)."""
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
            subprocess.check_call(["make", "-s", "-C", _HERE, "libzsm.so"])
            L = C.CDLL(os.path.join(_HERE, "libzsm.so"))
        vp = C.c_void_p
        L.zsm_decompose_srt.argtypes = [vp] * 4
        L.zsm_fill_mesh_instance.argtypes = [vp] * 2
        L.zsm_unorm16.argtypes = [vp, vp, C.c_uint32]
        L.zsm_emissive_to_world.argtypes = [vp] * 3
        L.zsm_decode_emissive_vertices.argtypes = [vp] * 2
        L.zsm_mul_point.argtypes = [vp] * 3
        L.zsm_move_instance.argtypes = [vp] * 3
        _LIB = L
    return _LIB
