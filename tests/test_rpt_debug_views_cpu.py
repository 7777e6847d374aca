"""The ReSTIR PT reconnection debug views without a GPU: the committed fixture against a live run of the reference's shaders, rpt::DebugColor
(compiled for the host: tests/rptview) against the colour table of include/zetaray_amd.h, and the C ABI's declarations."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rpt_view_cases as VC  # noqa: E402
from zetaray_amd import api, wire  # noqa: E402

LOBES = {"DIFFUSE_R": 0, "DIFFUSE_T": 1, "GLOSSY_R": 2, "GLOSSY_T": 3, "COAT": 4, "ALL": 5}      # BSDF::LOBE
EMPTY = 0xf                                                                                     # Reconnection::EMPTY
LT_NONE, LT_SUN, LT_SKY, LT_EMISSIVE = range(4)
KEEP = (7.0, 8.0, 9.0)      # the radiance handed in: what a class without a colour must return


def test_fixture_holds_every_case_view_and_frame():
    g = np.load(VC.GOLD)
    want = {VC.key(c, v, f) for c in VC.CASES for v in VC.VIEWS for f in VC.recorded(c)}
    assert set(g.files) == want
    for k in g.files:
        assert g[k].shape == (VC.H, VC.W, 3) and g[k].dtype == np.float32
    assert os.path.getsize(VC.GOLD) < 1 << 20


@pytest.mark.parametrize("case", list(VC.CASES))
def test_fixture_equals_live_reference(case):
    """re-runs the reference's compiled shaders with the view in bits 28-31 of Packed: guards the stored file against a stale build"""
    from oracle import zref
    if not zref.available():
        pytest.skip("oracle/_ref not built (no reference sources on this machine): the committed reference outputs are used instead")
    import make_rpt_view_goldens as M
    g = np.load(VC.GOLD)
    for view in VC.VIEWS:
        for f, img in M.render_reference(case, view).items():
            assert np.array_equal(img.view(np.uint32), g[VC.key(case, view, f)].view(np.uint32)), f"view {VC.VIEW_NAMES[view]}, frame {f}"


@pytest.fixture(scope="module")
def debug_color():
    d = os.path.join(ROOT, "tests", "rptview")
    import fcntl
    with open(os.path.join(d, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", d, "libzrv.so"])
        L = C.CDLL(os.path.join(d, "libzrv.so"))
    L.zrv_debug_color.argtypes = [C.c_uint32] * 6 + [C.c_void_p]

    def call(view, k, lobe_k_min_1=0, lobe_k=0, lt_k=LT_NONE, lt_k_plus_1=LT_NONE):
        rgb = np.array(KEEP, np.float32)
        L.zrv_debug_color(view, k, lobe_k_min_1, lobe_k, lt_k, lt_k_plus_1, rgb.ctypes.data)
        return tuple(rgb)
    return call


def _f32(rgb):
    return tuple(np.asarray(rgb, np.float32))


def test_debug_color_returns_the_headers_table(debug_color):
    col = {v: {k: _f32(c) for k, c in t.items()} for v, t in VC.COLORS.items()}
    black, keep = _f32(VC.BLACK), _f32(KEEP)
    # NONE leaves the radiance alone, whatever the record
    for k in (EMPTY, 2, 5):
        assert debug_color(wire.RPT_VIEW_NONE, k) == keep
    # an empty record is black in every view
    for v in VC.VIEWS:
        assert debug_color(v, EMPTY, LOBES["GLOSSY_R"], LOBES["GLOSSY_T"], LT_NONE, LT_EMISSIVE) == black
    # K: 2, 3, 4, and one colour from 5 up
    for k, want in ((2, col["K"][2]), (3, col["K"][3]), (4, col["K"][4]), (5, col["K"][5]), (6, col["K"][5]), (14, col["K"][5])):
        assert debug_color(wire.RPT_VIEW_K, k) == want
    # CASE: 1 = no light at x_k or x_{k+1}; 2 = x_{k+1} is a light sample; 3 = x_k is one
    assert debug_color(wire.RPT_VIEW_CASE, 3) == col["CASE"][1]
    for lt in (LT_SUN, LT_SKY, LT_EMISSIVE):
        assert debug_color(wire.RPT_VIEW_CASE, 3, lt_k_plus_1=lt) == col["CASE"][2]
        assert debug_color(wire.RPT_VIEW_CASE, 3, lt_k=lt) == col["CASE"][3]
    assert debug_color(wire.RPT_VIEW_FOUND_CONNECTION, 2) == col["FOUND_CONNECTION"][1]
    # the two lobe views: different tables; LOBE_K is also black for case 3
    for name, idx in LOBES.items():
        cls = name if name in col["LOBE_K"] else "OTHER"
        assert debug_color(wire.RPT_VIEW_LOBE_K_MIN_1, 4, lobe_k_min_1=idx, lobe_k=LOBES["DIFFUSE_R"]) == col["LOBE_K_MIN_1"][cls], name
        assert debug_color(wire.RPT_VIEW_LOBE_K, 4, lobe_k_min_1=LOBES["DIFFUSE_R"], lobe_k=idx) == col["LOBE_K"][cls], name
        assert debug_color(wire.RPT_VIEW_LOBE_K, 4, lobe_k=idx, lt_k=LT_EMISSIVE) == black
        assert debug_color(wire.RPT_VIEW_LOBE_K_MIN_1, 4, lobe_k_min_1=idx, lt_k=LT_EMISSIVE) == col["LOBE_K_MIN_1"][cls]
    assert col["LOBE_K_MIN_1"]["GLOSSY_R"] != col["LOBE_K"]["GLOSSY_R"] and col["LOBE_K_MIN_1"]["DIFFUSE_T"] != col["LOBE_K"]["DIFFUSE_T"]


def test_header_comment_states_the_colour_table():
    """the colours are data of the contract: every one of them stands in the header comment of enum zr_rpt_debug_view"""
    hdr = open(os.path.join(ROOT, "include", "zetaray_amd.h")).read()
    text = hdr[hdr.index("The ReSTIR PT reconnection debug views"):hdr.index("typedef enum zr_rpt_debug_view")]
    for view, table in VC.COLORS.items():
        for cls, rgb in table.items():
            s = "(" + ", ".join(repr(float(c)).rstrip("0").rstrip(".") if float(c) != int(c) else str(int(c)) for c in rgb) + ")"
            assert s in text, f"{view} {cls}: {s} is not in the header comment"


def test_c_abi_declares_the_view_setter():
    L = api.lib()
    assert "zr_pass_set_rpt_debug_view" in api.EXPORTS
    assert L.zr_pass_set_rpt_debug_view(None, 1) == 1          # ZR_ERR_INVALID_ARG
    assert b"INDIRECT" in L.zr_last_error()
    hdr = open(os.path.join(ROOT, "include", "zetaray_amd.h")).read()
    body = re.search(r"enum zr_rpt_debug_view\s*\{(.*?)\}", hdr, re.S).group(1)
    names = re.findall(r"\bZR_RPT_VIEW_(\w+)", body)
    assert names == ["NONE", "K", "CASE", "FOUND_CONNECTION", "LOBE_K_MIN_1", "LOBE_K", "COUNT"]
    for i, n in enumerate(names):
        assert getattr(wire, "RPT_VIEW_" + n) == i
    assert [VC.VIEW_NAMES[v] for v in VC.VIEWS] == names[1:-1]
    assert hasattr(api.Pass, "set_rpt_debug_view")
    # the C++ mirror: IndirectLighting::SetDebugView + the sequence entry the GPU test drives
    host = C.CDLL(os.path.join(ROOT, "zetaray_amd", "libzetaray_host.so"))
    assert hasattr(host, "zrh_render_sequence_debug_view")
    if api.device_count() == 0:
        with pytest.raises(api.ZetaRayError) as e:
            api.Pass(api.PASS_INDIRECT, 64, 64, api.INTEGRATOR_RESTIR_PT)
        assert e.value.code == 2                                 # ZR_ERR_NO_DEVICE
