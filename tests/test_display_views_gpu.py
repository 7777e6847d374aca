"""The display pass's G-buffer debug views on the GPU (k_display_view, zr_tu_display.hip): every DisplayOption from the HIP G-buffer equals
the reference's Display.hlsl mainPS (tests/displaycheck.py) on the same planes bit for bit, at display = render and display != render; the
sRGB8 plane is the back buffer's store of that float4.  Where oracle/_ref is absent the recorded fixture (tests/golden/display_views.npz)
stands in for the reference."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import display_view_cases as dv  # noqa: E402
import displaycheck as dc  # noqa: E402
import post_cases as pc  # noqa: E402
from zetaray_amd import api, wire  # noqa: E402


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = (g.view(np.uint32) != w.view(np.uint32)) if g.dtype == np.float32 else (g != w)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def _upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


class Setup:
    """the materials scene's HIP G-buffer at the render size, and a DISPLAY pass of `display` size reading the composited image"""

    def __init__(self, camera, display, render=dv.RENDER):
        import torch
        self.sc = dv.scene()
        self.scene = api.Scene(self.sc)
        self.cb = dv.frame_constants(self.sc, camera, render=render, display=display)
        self.gb = api.GBuffer(*render)
        api.Pass(api.PASS_GBUFFER, *render).render(self.cb, self.scene, self.gb)
        torch.cuda.synchronize()
        self.img = dv.image(render)
        self.dev_img, self.dev_exp = _upload(self.img), _upload(pc.DISPLAY_EXPOSURE)
        self.display = display

    def display_pass(self):
        p = api.Pass(api.PASS_DISPLAY, *self.display, params=dv.params())
        p.set_tonemap_lut()
        p.set_input(api.IN_POST_SIGNAL_F16, self.dev_img.data_ptr())
        p.set_input(api.IN_DISPLAY_EXPOSURE, self.dev_exp.data_ptr())
        return p

    def render(self, p, gbuffer=True):
        import torch
        p.render(self.cb, self.scene, self.gb if gbuffer else None)
        torch.cuda.synchronize()
        dw, dh = self.display
        return p.download_raw(api.OUT_DISPLAY, np.float32, (dh, dw, 4)), p.download_raw(api.OUT_DISPLAY_SRGB8, np.uint8, (dh, dw, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("camera", list(dv.CAMERAS))
@pytest.mark.parametrize("size", ["display_eq_render", "display_ne_render"])
def test_hip_views_equal_reference_shader(camera, size):
    s = Setup(camera, dv.RENDER if size == "display_eq_render" else dv.DISPLAY)
    planes, _ = s.gb.download()
    live = dc.available()
    gold = np.load(dv.GOLD)
    if size == "display_ne_render":
        for k in range(10):
            assert_same(planes[k], gold[f"{camera}/gb{k}"], f"HIP G-buffer plane {k} vs the fixture")
    elif not live:
        pytest.skip("display = render needs oracle/_ref (the fixture holds display != render)")
    p = s.display_pass()
    for o in dv.OPTIONS:
        p.set_display_option(o, dv.ROUGHNESS_TH)
        rgba, srgb = s.render(p)
        want = dc.shader_display(s.img, planes, dv.params(), s.cb, o, dv.ROUGHNESS_TH, pc.DISPLAY_EXPOSURE, api.load_tonemap_lut()) if live \
            else gold[f"{camera}/view{o}"]
        assert_same(rgba, want, f"{camera} option {o}")
        assert_same(srgb, dc.linear_to_srgb8(want), f"{camera} option {o} sRGB8")
    p.close()


@pytest.mark.gpu
def test_hip_views_1080p_equal_reference_shader():
    """full size, 1920 x 1080 display from a 1280 x 720 render: the NORMAL, COAT_COLOR and DEPTH views"""
    if not dc.available():
        pytest.skip("needs oracle/_ref")
    s = Setup("front", (1920, 1080), render=(1280, 720))
    planes, _ = s.gb.download()
    p = s.display_pass()
    for o in (wire.DISPLAY_NORMAL, wire.DISPLAY_COAT_COLOR, wire.DISPLAY_DEPTH):
        p.set_display_option(o)
        rgba, srgb = s.render(p)
        want = dc.shader_display(s.img, planes, dv.params(), s.cb, o, 1.0, pc.DISPLAY_EXPOSURE, api.load_tonemap_lut())
        assert_same(rgba, want, f"1080p option {o}")
        assert_same(srgb, dc.linear_to_srgb8(want), f"1080p option {o} sRGB8")
    p.close()


@pytest.mark.gpu
def test_default_is_unchanged_by_the_new_entry_point():
    """DEFAULT after a round trip through another view is byte-identical to a pass that never set an option, with or without a gbuffer"""
    s = Setup("front", dv.DISPLAY)
    fresh = s.display_pass()
    want = s.render(fresh, gbuffer=False)
    p = s.display_pass()
    p.set_display_option(wire.DISPLAY_COAT_COLOR, 0.25)
    s.render(p)
    p.set_display_option(wire.DISPLAY_DEFAULT)
    for gbuffer in (False, True):
        got = s.render(p, gbuffer)
        assert_same(got[0], want[0], "DEFAULT rgba")
        assert_same(got[1], want[1], "DEFAULT sRGB8")
    fresh.close()
    p.close()


@pytest.mark.gpu
def test_views_refuse_bad_inputs():
    s = Setup("front", dv.DISPLAY)
    p = s.display_pass()
    for bad in ((-1, 1.0), (wire.DISPLAY_COUNT, 1.0), (wire.DISPLAY_DEPTH, float("nan"))):
        with pytest.raises(api.ZetaRayError) as e:
            p.set_display_option(*bad)
        assert e.value.code == 1
    with pytest.raises(api.ZetaRayError) as e:
        api.Pass(api.PASS_TAA, 32, 32).set_display_option(wire.DISPLAY_DEPTH)
    assert e.value.code == 1
    p.set_display_option(wire.DISPLAY_NORMAL)
    with pytest.raises(api.ZetaRayError) as e:          # no gbuffer
        s.render(p, gbuffer=False)
    assert e.value.code == 1
    other = api.GBuffer(dv.RENDER[0] + 8, dv.RENDER[1])
    with pytest.raises(api.ZetaRayError) as e:          # not the render size
        p.render(s.cb, s.scene, other)
    assert e.value.code == 1
    s.gb.set_tile_origin(0, 32)
    with pytest.raises(api.ZetaRayError) as e:          # a screen tile
        s.render(p)
    assert e.value.code == 1
    p.close()
