"""Generates tests/golden/rpt_views.npz: FINAL (rgb) of the REFERENCE's own ReSTIR PT shaders (oracle/zref.py RefRestirPT) with each "Debug View" of its
indirect-lighting pass selected, on the cases of tools/rpt_view_cases.py.

How the view reaches the reference's shaders: IndirectLighting::DebugViewCallback (IndirectLighting.cpp:1543-1550) stores the view in bits 28-31 of
cb_ReSTIR_PT_PathTrace::Packed / cb_ReSTIR_PT_Reuse::Packed.  The reference-shader harness builds that word as max_non_tr_bounces | (max_glossy_tr_bounces
<< 4) | ... without masking the first term, and every shader reads the bounce count as Packed & 0xf -- so max_non_tr_bounces = bounces | (view << 28)
on the params handed to RefRestirPT.render is exactly the word the callback produces.  (Reference side only: the product validates
max_non_tr_bounces <= 15 and takes the view through zr_pass_set_rpt_debug_view.)

Needs oracle/_ref (built where the reference sources exist).  Asserts the coverage conditions of the fixture on the reference's output alone."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_ref_pass_goldens as M  # noqa: E402
import rpt_view_cases as VC  # noqa: E402
from oracle import zref, zro  # noqa: E402


def ref_params(prm, view):
    q = copy.copy(prm)
    q.max_non_tr_bounces = int(prm.max_non_tr_bounces) | (int(view) << 28)
    return q


def render_reference(case, view):
    """{frame: FINAL rgb float32 (H, W, 3)} of the recorded frames of `case` drawn with `view` (0 = the ordinary frame) by the reference's shaders"""
    sc, force_bvh, prm = VC.scene_and_params(case)
    o = zro.OracleScene(sc, force_bvh=force_bvh, cb=VC.RC.first_cb(VC.scenario(case)))
    k1 = zref.RefGBuffer(sc, force_bvh)
    ref = M.make_ref(zref, sc, "rpt", prm, force_bvh)
    q = ref_params(prm, view)
    out = {}
    for f, cb in VC.frames_of(case):
        M.prepare(ref, o, sc, cb, f, prm)
        arrays, planes = k1.render(cb)
        final = ref.render(cb, q, (arrays, planes))
        if f in VC.recorded(case):
            out[f] = np.ascontiguousarray(final[..., :3])
    return out


def check_coverage(data, plain):
    """the coverage conditions (over all cases): every class listed here is drawn somewhere"""
    def seen(view, rgb):
        return [c for c in VC.CASES if any(VC.has_color(data[VC.key(c, view, f)], rgb) for f in VC.recorded(c))]
    report = {}
    for view, name in VC.VIEW_NAMES.items():
        for cls, rgb in list(VC.COLORS[name].items()) + [("black", VC.BLACK)]:
            report[(name, cls)] = seen(view, rgb)
    for k, v in report.items():
        print("%-18s %-10s %s" % (k[0], k[1], ", ".join(v) if v else "-- not reached"))
    need = [("K", "black"), ("K", 2), ("K", 3), ("K", 4), ("K", 5), ("CASE", 1), ("CASE", 2), ("CASE", 3), ("FOUND_CONNECTION", 1), ("FOUND_CONNECTION", "black")]
    need += [(v, l) for v in ("LOBE_K_MIN_1", "LOBE_K") for l in ("DIFFUSE_R", "GLOSSY_R", "GLOSSY_T")]
    missing = [k for k in need if not report[k]]
    assert not missing, f"coverage: not reached: {missing}"
    # an early-out pixel of a frame without spatial reuse: black in the view, lit in the ordinary frame
    early = 0
    for c in VC.NO_SPATIAL_CASES:
        for f in VC.recorded(c):
            black = np.all(data[VC.key(c, 1, f)] == 0, axis=-1) & np.all(data[VC.key(c, 3, f)] == 0, axis=-1)
            early += int(np.count_nonzero(black & np.any(plain[c][f] != 0, axis=-1)))
    print("pixels black in the K and FOUND_CONNECTION views and lit in the ordinary frame (no-spatial cases):", early)
    assert early > 0, "coverage: no early-out pixel that is black in the view and non-black in the ordinary frame"


def main():
    data, plain = {}, {}
    for case in VC.CASES:
        plain[case] = render_reference(case, 0)
        for view in VC.VIEWS:
            for f, img in render_reference(case, view).items():
                data[VC.key(case, view, f)] = img
        print(case, "done", flush=True)
    check_coverage(data, plain)
    np.savez_compressed(VC.GOLD, **data)
    print(VC.GOLD, os.path.getsize(VC.GOLD), "bytes")


if __name__ == "__main__":
    main()
