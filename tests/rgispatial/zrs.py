"""ctypes binding of tests/rgispatial/libzrs.so (TEST-ONLY serial executor of rgi::SpatialResample, zr_rgi_spatial.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        import fcntl
        with open(os.path.join(_HERE, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-s", "-C", _HERE, "libzrs.so"])
            L = C.CDLL(os.path.join(_HERE, "libzrs.so"))
        L.zrs_rgi_spatial.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def spatial(hxscene, cb, gb, planes, num_samples, radius_px=0.0, final=None):
    """One frame of the spatial stage.  hxscene: tests.hostexec.zhx.HostExecScene; gb: a (view, zr_gbuffer_planes) pair as HostExecScene.gbuffer / the
    GPU download helpers return it; planes: {"A": (h, w, 4) f32, "B": (h, w, 4) u16, "C": (h, w, 4) f32}, the set k_rgi wrote this frame;
    final: the FINAL plane to store into or accumulate onto (default: zeros).  Returns (final, (n_closest, n_shadow))."""
    from zetaray_amd import wire
    cbb = np.ascontiguousarray(cb)
    h, w = planes["A"].shape[:2]
    a, b, c = (np.ascontiguousarray(planes["A"], np.float32), np.ascontiguousarray(planes["B"], np.uint16), np.ascontiguousarray(planes["C"], np.float32))
    out = np.zeros((h, w, 4), np.float32) if final is None else final
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (h, w, 4)
    cnt = wire.Counters()
    lib().zrs_rgi_spatial(hxscene.h, cbb.ctypes.data, C.addressof(gb[1]), a.ctypes.data, b.ctypes.data, c.ctypes.data, num_samples, radius_px,
                          out.ctypes.data, C.addressof(cnt))
    return out, (cnt.n_closest, cnt.n_shadow)
