"""ctypes binding of tests/aliasmath/libzal.so (TEST-ONLY host compilation of include/zr_alias.h: alias_math.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from zetaray_amd import wire

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        import fcntl
        with open(os.path.join(_HERE, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-s", "-C", _HERE, "libzal.so"])
            L = C.CDLL(os.path.join(_HERE, "libzal.so"))
        vp, u32 = C.c_void_p, C.c_uint32
        L.zal_build.argtypes = [vp, u32, vp]
        L.zal_kahan_sum.argtypes = [vp, u32]; L.zal_kahan_sum.restype = C.c_float
        L.zal_weights.argtypes = [vp, u32, vp]
        _LIB = L
    return _LIB


def build(power):
    """the header's table (zral::Build) for these powers"""
    power = np.ascontiguousarray(power, np.float32)
    out = np.zeros(len(power), wire.ALIAS_ENTRY)
    lib().zal_build(power.ctypes.data, len(power), out.ctypes.data)
    return out


def weights(power):
    power = np.ascontiguousarray(power, np.float32)
    out = np.zeros(len(power), np.uint64)
    lib().zal_weights(power.ctypes.data, len(power), out.ctypes.data)
    return out
