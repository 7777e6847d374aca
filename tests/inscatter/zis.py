"""ctypes binding of tests/inscatter/libzis.so (TEST-ONLY serial executor of the inscattering voxel grid and its compositing branch,
written from the reference's shaders: inscatter.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
SLICES = 128


def lib():
    global _LIB
    if _LIB is None:
        import fcntl
        with open(os.path.join(_HERE, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-s", "-C", _HERE, "libzis.so"])
            L = C.CDLL(os.path.join(_HERE, "libzis.so"))
        vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
        L.zis_scene_create.restype = vp
        L.zis_scene_create.argtypes = [vp]
        L.zis_scene_destroy.argtypes = [vp]
        L.zis_scene_update_instances.argtypes = [vp, vp, vp, u32]
        L.zis_grid.argtypes = [vp, vp, u32, u32, f32, f32, f32, vp, vp, vp]
        L.zis_wave_prefix_sum.argtypes = [vp, vp]
        L.zis_composite.argtypes = [vp, vp, vp, vp, u32, u32, f32, f32, f32, vp, u32, u32]
        _LIB = L
    return _LIB


class Scene:
    """the oracle's scene (world-space triangles) for the visibility rays"""

    def __init__(self, scene):
        self._desc = scene.desc()
        self.h = lib().zis_scene_create(C.addressof(self._desc))

    def update_instances(self, instances, instance_to_world):
        i, x = np.ascontiguousarray(instances), np.ascontiguousarray(instance_to_world, np.float32)
        lib().zis_scene_update_instances(self.h, i.ctypes.data, x.ctypes.data, len(i))

    def __del__(self):
        if getattr(self, "h", None):
            lib().zis_scene_destroy(self.h)
            self.h = None


def grid(scene, cb, voxels=(192, 108), depth_map_exp=2.0, near_z=0.5, far_z=30.0, with_ls=False):
    """Inscattering.hlsl over the whole grid: (128, ny, nx) uint32 R11G11B10 texels [, Ls before the store (128, ny, nx, 3) f32, sun
    visibility (128, ny, nx) u8]"""
    nx, ny = voxels
    g = np.zeros((SLICES, ny, nx), np.uint32)
    ls = np.zeros((SLICES, ny, nx, 3), np.float32) if with_ls else None
    vis = np.zeros((SLICES, ny, nx), np.uint8) if with_ls else None
    cbb = np.ascontiguousarray(cb)
    lib().zis_grid(scene.h, cbb.ctypes.data, nx, ny, depth_map_exp, near_z, far_z, g.ctypes.data,
                   None if ls is None else ls.ctypes.data, None if vis is None else vis.ctypes.data)
    return (g, ls, vis) if with_ls else g


def wave_prefix_sum(x):
    """the pinned WavePrefixSum of 32 fp32 values"""
    x = np.ascontiguousarray(x, np.float32)
    assert x.shape == (32,)
    out = np.zeros(32, np.float32)
    lib().zis_wave_prefix_sum(x.ctypes.data, out.ctypes.data)
    return out


def composite(cb, mr_plane, depth, color, grid_texels, depth_map_exp=2.0, near_z=0.5, far_z=30.0):
    """Compositing.hlsl:74-97 on a composited (h, w, 4) f32 image: returns the image with the inscattering term added"""
    mr = np.ascontiguousarray(mr_plane)
    h, w = mr.shape[:2]
    mr8 = mr.view(np.uint8).reshape(h, w, 2)
    d = np.ascontiguousarray(depth, np.float32).reshape(h, w)
    out = np.ascontiguousarray(color, np.float32).copy()
    gt = np.ascontiguousarray(grid_texels, np.uint32)
    cbb = np.ascontiguousarray(cb)
    lib().zis_composite(cbb.ctypes.data, mr8.ctypes.data, d.ctypes.data, gt.ctypes.data, gt.shape[2], gt.shape[1], depth_map_exp, near_z, far_z,
                        out.ctypes.data, w, h)
    return out


def decode(texels):
    """R11G11B10_FLOAT -> (..., 3) float64"""
    t = np.asarray(texels, np.uint32)

    def uf(bits, mb):
        e = (bits >> mb).astype(np.int64)
        m = (bits & ((1 << mb) - 1)).astype(np.float64)
        return np.where(e == 0, m / (1 << mb) * 2.0 ** -14, (1.0 + m / (1 << mb)) * 2.0 ** (e - 15))
    return np.stack([uf(t & 0x7ff, 6), uf((t >> 11) & 0x7ff, 6), uf(t >> 22, 5)], axis=-1)
