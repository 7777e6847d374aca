"""Run by tests/test_mipgen_gpu.py in a process of its own with ZETARAY_AMD_LIB = the tolerance-mode library (the library is chosen at load time):
zr_mipgen_device on one chain per format against include/zr_mipgen.h on the host, one JSON line with the number of bytes that differ."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.mipmath import zmg      # noqa: E402
from zetaray_amd import api, scene_io      # noqa: E402

rng = np.random.default_rng(6)
out = {"lib": os.path.basename(api.LIB_PATH)}
for name, fmt in zmg.FORMATS.items():
    w, h = 65, 33
    mips = zmg.full_mips(w, h)
    heap = np.zeros(zmg.chain_bytes(w, h, mips, fmt), np.uint8)
    heap[:w * h * zmg.channels(fmt)] = rng.integers(0, 256, w * h * zmg.channels(fmt), dtype=np.uint8)
    d = zmg.descs([(0, w, h, mips, fmt)])
    want = scene_io.mip_generate(d, heap.copy())
    got = api.mipgen_device(d, heap)
    out[name] = int(len(want) - w * h * zmg.channels(fmt))
    out[name + "_bad"] = int((got != want).sum())
print(json.dumps(out))
