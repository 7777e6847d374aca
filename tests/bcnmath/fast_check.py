"""Run by tests/test_bcn_gpu.py in a process of its own with ZETARAY_AMD_LIB = the tolerance-mode library (the library is chosen at load time):
zr_bcn_decode_device on the blocks of tests/golden/bcn_blocks.npz, one JSON line with the number of blocks whose texels differ from the fixture's."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from zetaray_amd import api, wire      # noqa: E402

z = np.load(os.path.join(ROOT, "tests", "golden", "bcn_blocks.npz"))
out = {"lib": os.path.basename(api.LIB_PATH)}
for name, enc, fmt in (("bc7", 1, wire.TEX_RGBA8), ("bc5", 2, wire.TEX_RG8)):
    blocks, want = np.ascontiguousarray(z[name]), z[name + "_texels"]
    n, ch = len(blocks), want.shape[2]
    d = np.zeros(1, wire.TEXTURE_DESC)
    d["width"], d["height"], d["num_mips"], d["format"] = 4 * n, 4, 1, fmt
    s = np.zeros(1, wire.TEXTURE_SOURCE)
    s["encoding"] = enc
    got = api.bcn_decode_device(d, s, blocks.reshape(-1), 16 * n * ch).reshape(4, n, 4, ch).transpose(1, 0, 2, 3).reshape(n, 16, ch)
    out[name] = n
    out[name + "_bad"] = int((got != want).any(axis=(1, 2)).sum())
print(json.dumps(out))
