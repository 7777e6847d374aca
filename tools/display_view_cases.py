"""The scenes and cameras of the display pass's G-buffer debug views, shared by their fixture generator (tools/make_display_views_golden.py)
and the tests (tests/test_display_views_cpu.py, tests/test_display_views_gpu.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import post_cases as pc  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "display_views.npz")
RENDER, DISPLAY = (48, 36), (60, 45)
ROUGHNESS_TH = 0.5
# camera position, view direction: "front" sees metal, coat, transmissive and emissive surfaces; "up" looks out of the open top (misses)
CAMERAS = {"front": ((0.0, 0.5, -3.5), (0.0, 0.35, 1.0)), "up": ((0.0, 2.0, -3.5), (0.0, 0.6, 0.8))}
OPTIONS = range(10)       # enum zr_display_option, DEFAULT .. DEPTH


def scene():
    from zetaray_amd import scene_io
    return scene_io.make_synthetic_scene(num_tris=3000, num_emissive=150, seed=11, open_top=True)


def frame_constants(sc, camera, render=RENDER, display=DISPLAY):
    from zetaray_amd import scene_io
    pos, vd = CAMERAS[camera]
    vd = np.array(vd, np.float32)
    vd /= np.linalg.norm(vd)
    cb = scene_io.make_frame_constants(render[0], render[1], cam_pos=pos, view_dir=tuple(float(x) for x in vd), num_emissives=len(sc.emissives))
    cb["display_width"], cb["display_height"] = display
    return cb


def image(render=RENDER):
    """the composited input: RGBA16F bits"""
    return pc.to_half_bits(pc.hdr_image(seed=23, w=render[0], h=render[1]))


def params():
    return pc.params("neutral", True)
