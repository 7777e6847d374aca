"""ctypes binding of tests/bcnmath/libzbc.so (TEST-ONLY host compilation of include/zr_bcn.h: bcn_math.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
RAW, BC7, BC5 = 0, 1, 2      # ZR_TEX_SRC_*


def lib():
    global _LIB
    if _LIB is None:
        import fcntl
        with open(os.path.join(_HERE, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-s", "-C", _HERE, "libzbc.so"])
            L = C.CDLL(os.path.join(_HERE, "libzbc.so"))
        vp, u32 = C.c_void_p, C.c_uint32
        L.zbc_decode_mip.argtypes = [u32, vp, u32, u32, vp]
        L.zbc_bc7_fields.argtypes = [vp, vp]
        _LIB = L
    return _LIB


def mip_blocks(w, h):
    return ((w + 3) // 4) * ((h + 3) // 4)


def decode_mip(encoding, blocks, w, h):
    """the header's lane form on the host: w x h texels (h, w, 4) for BC7, (h, w, 2) for BC5"""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1)
    assert len(blocks) == 16 * mip_blocks(w, h)
    out = np.zeros((h, w, 4 if encoding == BC7 else 2), np.uint8)
    lib().zbc_decode_mip(encoding, blocks.ctypes.data, w, h, out.ctypes.data)
    return out


def decode_blocks(encoding, blocks):
    """n blocks (n, 16) -> (n, 16, C) texels, texel 4 y + x of each block: the blocks as one row of a 4 n x 4 mip"""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    n = len(blocks)
    img = decode_mip(encoding, blocks, 4 * n, 4)
    return img.reshape(4, n, 4, -1).transpose(1, 0, 2, 3).reshape(n, 16, -1).copy()


def bc7_fields(block):
    """(mode or 8, partition, rotation, index selector, p-bit mask) of one block"""
    block = np.ascontiguousarray(block, np.uint8)
    out = np.zeros(5, np.uint32)
    lib().zbc_bc7_fields(block.ctypes.data, out.ctypes.data)
    return tuple(int(v) for v in out)
