"""Writes the valid PNG files tests/mipmath/host_check.cpp decodes and mutates (make -C tests/mipmath check): every supported colour type and bit depth,
the five row filters, stored / fixed / dynamic deflate blocks, tRNS, a split IDAT; small, so that a few hundred thousand mutants take a minute."""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.mipmath import zmg      # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else "corpus"
os.makedirs(out, exist_ok=True)
rng = np.random.default_rng(1)
COMP = [(0, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)]
n = 0
for ctype, ch in ((0, 1), (2, 3), (3, 1), (4, 2), (6, 4)):
    for depth in ((8,) if ctype == 3 else (8, 16)):
        for k, (w, h) in enumerate(((1, 1), (3, 5), (19, 12))):
            flt, (level, strategy) = (n + k) % 5, COMP[(n + k) % 3]
            palette = rng.integers(0, 256, (23, 3), dtype=np.uint8) if ctype == 3 else None
            hi = 23 if ctype == 3 else (65536 if depth == 16 else 256)
            s = (rng.integers(0, hi, (h, w, ch)) // (1 if ctype == 3 else 37) * (1 if ctype == 3 else 37)).astype(np.uint16 if depth == 16 else np.uint8)
            trns = None
            if ctype == 3:
                trns = rng.integers(0, 256, 9, dtype=np.uint8).tobytes()
            elif ctype in (0, 2) and k:
                trns = s[0, 0].astype(">u2").tobytes()
            data = zmg.png_bytes(s, ctype, depth, flt, level, strategy, palette, trns, idat_split=61 if k == 2 else None)
            open(os.path.join(out, "c%d_d%d_%dx%d_f%d_l%d.png" % (ctype, depth, w, h, flt, level)), "wb").write(data)
            n += 1
print("%d files in %s" % (n, out))
