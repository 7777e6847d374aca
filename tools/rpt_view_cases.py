"""The scenarios of the ReSTIR PT reconnection debug views (zetaray_amd.h zr_pass_set_rpt_debug_view): shared by the fixture generator
(tools/make_rpt_view_goldens.py -> tests/golden/rpt_views.npz) and tests/test_rpt_debug_views_{cpu,gpu}.py.

A case = a scenario of tools/ref_pass_cases.py (scene, camera path, frames_of) + the pass parameters it runs with here.  Between them the cases
make each of the three kernels that can write FINAL the writer (K11 without temporal reuse, Reconnect_TtC without spatial reuse, Reconnect_StC
otherwise) and exercise the early outs that write black.  Every case is rendered with each of the five views; the fixture holds FINAL (rgb) of the
last two frames.

Classes of RPT_Util::DebugColor the 96 x 64 scenes do not reach (the generator prints which classes it saw): see UNREACHED below."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_pass_cases as RC  # noqa: E402

W, H = RC.W, RC.H
GOLD = os.path.join(ROOT, "tests", "golden", "rpt_views.npz")
VIEW_NAMES = {1: "K", 2: "CASE", 3: "FOUND_CONNECTION", 4: "LOBE_K_MIN_1", 5: "LOBE_K"}      # enum zr_rpt_debug_view
VIEWS = tuple(VIEW_NAMES)
RECORDED_FRAMES = 2      # the last two frames of a sequence

# name -> (scenario of ref_pass_cases.CASES: scene / camera / frames, params kwargs of ref_pass_cases._params)
CASES = {
    "k11_no_temporal": ("rpt_no_reuse", dict(flags_off=(1 << 0))),                      # cornell_emissive, moving: K11 writes
    "ttc_no_spatial_moving": ("rpt_cornell_moving", dict(spatial_passes=0)),            # TtC writes; pixels without history take the early outs
    "stc_cornell_moving": ("rpt_cornell_moving", {}),                                   # StC writes
    "stc_materials_rr": ("rpt_materials_rr", dict(bounces=(6, 8))),                     # deep k, transmission lobes
    "stc_two_spatial": ("rpt_two_spatial", dict(spatial_passes=2)),                     # the second round writes over the first
    "stc_sun_sky": ("rpt_sun_sky", {}),                                                 # cornell (sun + sky): the NEE_EMISSIVE == 0 permutation
    "stc_accumulate": ("rpt_accumulate", {}),                                           # Accumulate && CameraStatic: the colour is summed, 0 added at early outs
}
NO_SPATIAL_CASES = ("ttc_no_spatial_moving",)

# the colour tables (zetaray_amd.h, enum zr_rpt_debug_view), as the float32 values the kernels store
BLACK = (0.0, 0.0, 0.0)
COLORS = {
    "K": {2: (0.1, 0.25, 0.88), 3: (0.13, 0.55, 0.14), 4: (0.69, 0.45, 0.1), 5: (0.88, 0.08, 0.1)},
    "CASE": {1: (0.85, 0.096, 0.1), 2: (0.13, 0.6, 0.14), 3: (0.1, 0.27, 0.888)},
    "FOUND_CONNECTION": {1: (0.234, 0.12, 0.2134)},
    "LOBE_K_MIN_1": {"DIFFUSE_R": (0.384, 0.12, 0.2134), "GLOSSY_R": (0.12, 0.4284, 0.2134), "GLOSSY_T": (0.1134, 0.12, 0.634),
                     "DIFFUSE_T": (0.25, 0.25, 0.25), "OTHER": (0.55, 0.55, 0.0)},
    "LOBE_K": {"DIFFUSE_R": (0.384, 0.12, 0.2134), "GLOSSY_R": (0.12, 0.284, 0.2134), "GLOSSY_T": (0.1134, 0.12, 0.634),
               "DIFFUSE_T": (0.25, 0.25, 0.0), "OTHER": (0.25, 0.25, 0.25)},
}
# classes no case reaches (the generator's report; the coverage conditions it asserts do not include them)
UNREACHED = {
    # the "else" colour of the x_{k-1} table stands for LOBE::COAT and LOBE::ALL: no reservoir of these 96 x 64 frames ends up with either at x_{k-1}
    # (also not with the `materials` scene or more bounces) -- the coat lobes of the synthetic scene are rarely sampled, and LOBE::ALL at x_{k-1} only
    # comes from a case-3 light sample taken at k = 2 that survives resampling.  DebugColor's host test covers the branch.  Every other class is drawn:
    # DIFFUSE_T in both lobe views and the "else" colour of the x_k table (LOBE::ALL at x_k: case 2 with a light sample) included.
    ("LOBE_K_MIN_1", "OTHER"): "no recorded frame holds LOBE::COAT or LOBE::ALL at x_{k-1}",
}


def scenario(case):
    return CASES[case][0]


def frames_of(case):
    return RC.frames_of(scenario(case))


def scene_and_params(case):
    """(scene, force_bvh, params) of a case"""
    base, kw = CASES[case]
    sc, force_bvh, integ, _ = RC.scene_and_params(base)
    assert integ == "rpt"
    return sc, force_bvh, RC._params(kind="rpt", **kw)


def num_frames(case):
    return RC.CASES[scenario(case)][2]


def recorded(case):
    n = num_frames(case)
    return tuple(range(n - RECORDED_FRAMES + 1, n + 1))


def key(case, view, f):
    return f"{case}/view{view}/final_{f}"


def has_color(img, rgb):
    """does any pixel of img (h, w, >= 3) hold exactly the float32 colour rgb?"""
    c = np.asarray(rgb, np.float32)
    return bool(np.any(np.all(np.ascontiguousarray(img[..., :3], np.float32).view(np.uint32) == c.view(np.uint32), axis=-1)))
