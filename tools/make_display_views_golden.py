"""Generates tests/golden/display_views.npz: the reference's K1 G-buffer (oracle/zref.py RefGBuffer) of the display-view scene for each camera
of tools/display_view_cases.py, and what the reference's Display.hlsl mainPS (tests/displaycheck.py) draws from it for every DisplayOption.
Needs oracle/_ref (built where the reference sources exist)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import display_view_cases as dv  # noqa: E402
import displaycheck as dc  # noqa: E402
import post_cases as pc  # noqa: E402
from oracle import zref  # noqa: E402
from zetaray_amd import api  # noqa: E402


def compute(camera):
    sc = dv.scene()
    cb = dv.frame_constants(sc, camera)
    planes, _ = zref.RefGBuffer(sc).render(cb)
    out = {f"{camera}/gb{k}": p for k, p in enumerate(planes)}
    for o in dv.OPTIONS:
        out[f"{camera}/view{o}"] = dc.shader_display(dv.image(), planes, dv.params(), cb, o, dv.ROUGHNESS_TH, pc.DISPLAY_EXPOSURE, api.load_tonemap_lut())
    return out


if __name__ == "__main__":
    data = {}
    for cam in dv.CAMERAS:
        data.update(compute(cam))
    np.savez_compressed(dv.GOLD, **data)
    print(dv.GOLD, os.path.getsize(dv.GOLD), "bytes")
