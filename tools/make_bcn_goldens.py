#!/usr/bin/env python3
"""tests/golden/bcn_blocks.npz: BC7 / BC5 blocks and the texels they decode to (tests/test_bcn_cpu.py, tests/test_bcn_gpu.py).

BC7: for each mode 0 - 7 the six bits behind the mode's unary prefix take each value 0 .. 63, with four random fillings of the other bits per value
(2 048 blocks), plus 64 reserved-mode blocks (byte 0 == 0, the rest random).  Those six bits hold the partition of every partitioned mode, rotation and
index selector of mode 4 and the rotation of mode 5, so every partition, all eight rotation x selector settings and all four rotations occur; that, and
both values of a p-bit per mode that has p-bits, is asserted below from the decoded fields.
BC5: 1 024 random blocks plus 16 whose endpoints are equal in one or both channels.

The expected texels are the host loader's (zrh_bc7_decode / zrh_bc5_decode).  Run it with --lib pointing at a libzetaray_sceneio.so built from the
commit BEFORE include/zr_bcn.h existed to regenerate the fixture independently of the header; with Pillow importable the texels are also held to
Pillow's decoder.  The multiply-by-reciprocal divisions of the header's lane form are checked exhaustively here as well."""
import argparse
import ctypes as C
import io
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dds(w, h, fmt, payload):
    """a DX10-header .dds with one mip (DXGI_FORMAT 98 = BC7_UNORM, 83 = BC5_UNORM)"""
    hdr = bytearray(128)
    hdr[0:4] = b"DDS "
    struct.pack_into("<7I", hdr, 4, 124, 0x1007 | 0x80000, h, w, len(payload), 0, 1)
    struct.pack_into("<2I4s", hdr, 76, 32, 4, b"DX10")
    struct.pack_into("<I", hdr, 108, 0x1000)
    return bytes(hdr) + struct.pack("<5I", fmt, 3, 0, 1, 0) + bytes(payload)


def pillow_decode(blocks, fmt):
    from PIL import Image
    n = len(blocks)
    im = Image.open(io.BytesIO(dds(4 * n, 4, fmt, blocks.tobytes())))
    a = np.asarray(im.convert("RGBA") if fmt == 98 else im.convert("RGB"))
    a = a[..., :4] if fmt == 98 else a[..., :2]
    return a.reshape(4, n, 4, -1).transpose(1, 0, 2, 3).reshape(n, 16, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "zetaray_amd", "libzetaray_sceneio.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bcn_blocks.npz"))
    args = ap.parse_args()
    L = C.CDLL(args.lib)
    for f in (L.zrh_bc7_decode, L.zrh_bc5_decode):
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    rng = np.random.default_rng(0xBC7)

    # ---- BC7
    blocks = []
    for mode in range(8):
        for v in range(64):
            for _ in range(4):
                bits = rng.integers(0, 2, 128, dtype=np.uint8)
                bits[:mode] = 0
                bits[mode] = 1
                bits[mode + 1:mode + 7] = [(v >> k) & 1 for k in range(6)]
                blocks.append(np.packbits(bits, bitorder="little"))
    for _ in range(64):
        b = rng.integers(0, 256, 16, dtype=np.uint8)
        b[0] = 0
        blocks.append(b)
    bc7 = np.stack(blocks).astype(np.uint8)
    n7 = len(bc7)
    bc7_texels = np.zeros((4, 4 * n7, 4), np.uint8)
    L.zrh_bc7_decode(bc7.ctypes.data, 4 * n7, 4, bc7_texels.ctypes.data)
    bc7_texels = bc7_texels.reshape(4, n7, 4, 4).transpose(1, 0, 2, 3).reshape(n7, 16, 4).copy()

    # coverage, from the decoded fields (tests/bcnmath: the header's Field on the host)
    from tests.bcnmath import zbc
    NS = [3, 2, 3, 2, 1, 1, 1, 2]
    PB = [4, 6, 6, 6, 0, 0, 0, 6]
    NP = [6, 2, 0, 4, 0, 0, 2, 4]
    seen = [dict(part=set(), rot=set(), rotsel=set(), p0=0, p1=0) for _ in range(9)]
    for b in bc7:
        mode, part, rot, isel, pbits = zbc.bc7_fields(b)
        s = seen[mode]
        s["part"].add(part); s["rot"].add(rot); s["rotsel"].add((rot, isel))
        if mode < 8 and NP[mode]:
            s["p1"] |= pbits
            s["p0"] |= ~pbits & ((1 << NP[mode]) - 1)
    for mode in range(8):
        assert seen[mode]["part"] == set(range(1 << PB[mode])), ("partitions of mode", mode)
        if NP[mode]:
            full = (1 << NP[mode]) - 1
            assert seen[mode]["p0"] == full and seen[mode]["p1"] == full, ("p-bits of mode", mode)
    assert seen[4]["rotsel"] == {(r, s) for r in range(4) for s in range(2)}
    assert seen[5]["rot"] == set(range(4))
    assert len([b for b in bc7 if b[0] == 0]) == 64
    assert all(NS[m] in (1, 2, 3) for m in range(8))

    # ---- BC5
    bc5 = rng.integers(0, 256, (1024 + 16, 16), dtype=np.uint8)
    for k in range(16):
        b = bc5[1024 + k]
        if k % 3 in (0, 2):
            b[1] = b[0]
        if k % 3 in (1, 2):
            b[9] = b[8]
    n5 = len(bc5)
    bc5_texels = np.zeros((4, 4 * n5, 2), np.uint8)
    L.zrh_bc5_decode(bc5.ctypes.data, 4 * n5, 4, bc5_texels.ctypes.data)
    bc5_texels = bc5_texels.reshape(4, n5, 4, 2).transpose(1, 0, 2, 3).reshape(n5, 16, 2).copy()

    try:
        import PIL  # noqa: F401
        # (the reserved mode is this project's to define: (0, 0, 0, 0) here, opaque black in Pillow)
        live = bc7[:, 0] != 0
        assert np.array_equal(pillow_decode(bc7, 98)[live], bc7_texels[live]), "BC7 differs from Pillow"
        assert not bc7_texels[~live].any()
        assert np.array_equal(pillow_decode(bc5, 83), bc5_texels), "BC5 differs from Pillow"
        print("equal to Pillow", PIL.__version__)
    except ImportError:
        print("Pillow is not importable: not compared")

    # ---- the reciprocals of the lane form
    for bits, rcp, ref in ((2, 21846, [0, 21, 43, 64]), (3, 9363, [0, 9, 18, 27, 37, 46, 55, 64]),
                           (4, 4370, [0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64])):
        d = (1 << bits) - 1
        assert [((64 * i + d // 2) * rcp) >> 16 for i in range(1 << bits)] == ref
    assert all((x * 9363) >> 16 == x // 7 for x in range(7 * 255 + 1)) and all((x * 13108) >> 16 == x // 5 for x in range(5 * 255 + 1))

    np.savez_compressed(args.out, bc7=bc7, bc7_texels=bc7_texels, bc5=bc5, bc5_texels=bc5_texels)
    print("%s: %d BC7 + %d BC5 blocks, %d bytes" % (args.out, n7, n5, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
