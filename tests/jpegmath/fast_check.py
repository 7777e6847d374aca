"""Run by tests/test_jpeg_gpu.py in a process of its own with ZETARAY_AMD_LIB = the tolerance-mode library (the library is chosen at load time):
zr_jpeg_decode_device on fixture files of every sampling and channel map against include/zr_jpeg.h on the host, one JSON line with the number of bytes
that differ."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.jpegmath import zjp      # noqa: E402
from zetaray_amd import api, scene_io, wire      # noqa: E402

files = {n: d for n, d, _ in zjp.load_fixture()}
out = {"lib": os.path.basename(api.LIB_PATH), "bytes": 0, "bad": 0}
for name, cmap, fmt in (("33x17_420_q90_noise", wire.JPEG_MAP_RGBA, wire.TEX_RGBA8_SRGB), ("33x17_422_restart_rows", wire.JPEG_MAP_BG, wire.TEX_RG8),
                        ("16x16_444_q100_smooth", wire.JPEG_MAP_RG, wire.TEX_RG8), ("17x23_gray_optimize", wire.JPEG_MAP_RGBA, wire.TEX_RGBA8)):
    rec = scene_io.pack_jpeg(files[name], name, cmap)
    want = scene_io.jpeg_expand(rec)
    d = np.zeros(1, wire.TEXTURE_DESC)
    d["width"], d["height"], d["num_mips"], d["format"] = want.shape[1], want.shape[0], 1, fmt
    s = np.zeros(1, wire.TEXTURE_SOURCE)
    s["encoding"] = wire.TEX_SRC_JPEG_COEF
    got = api.jpeg_decode_device(d, s, rec, want.size)
    out["bytes"] += int(want.size)
    out["bad"] += int((got != want.reshape(-1)).sum())
print(json.dumps(out))
