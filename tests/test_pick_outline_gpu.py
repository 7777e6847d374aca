"""The picked-instance outline of the display pass on the GPU (k_pick_setup / k_pick_cover / k_pick_outline, zr_tu_display.hip): pick a pixel
with the G-buffer pass, read the pick back, outline that instance.  The mask (ZR_OUT_PICK_MASK) and the display planes must equal the numpy
restatement of the raster contract and of Sobel.hlsl (tests/pickcheck.py) bit for bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import displaycheck as dc  # noqa: E402
import pickcheck as pk  # noqa: E402
import post_cases as pc  # noqa: E402
from zetaray_amd import api, scene_io, wire  # noqa: E402


def cornell():
    return scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))


def instance_tris(sc, idx):
    inst = sc.instances[idx]
    n = int(sc.instance_num_tris[idx])
    ib = sc.indices[int(inst["base_idx_offset"]):int(inst["base_idx_offset"]) + 3 * n].astype(np.int64) + int(inst["base_vtx_offset"])
    return sc.vertices["pos"][ib].reshape(n, 3, 3).astype(np.float32)


class Frame:
    def __init__(self, sc, render, display, **cam):
        import torch
        self.sc, self.render, self.display = sc, render, display
        self.scene = api.Scene(sc)
        self.cb = scene_io.make_frame_constants(render[0], render[1], num_emissives=len(sc.emissives), **cam)
        self.cb["display_width"], self.cb["display_height"] = display
        self.cb["curr_view_proj"] = pk.view_proj(self.cb)
        self.gb = api.GBuffer(*render)
        self.p_gb = api.Pass(api.PASS_GBUFFER, *render)
        img = pc.to_half_bits(pc.hdr_image(seed=5, w=render[0], h=render[1]))
        self.dev_img, self.dev_exp = torch.from_numpy(img).to("cuda"), torch.from_numpy(pc.DISPLAY_EXPOSURE).to("cuda")
        self.p = api.Pass(api.PASS_DISPLAY, *display, params=pc.params("agx_default", False))
        self.p.set_input(api.IN_POST_SIGNAL_F16, self.dev_img.data_ptr())

    def pick(self, x, y):
        import torch
        self.p_gb.pick_pixel(x, y)
        self.p_gb.render(self.cb, self.scene, self.gb)
        torch.cuda.synchronize()
        return self.p_gb.read_pick()

    def show(self, picks):
        import torch
        self.p.set_picked_instances(picks)
        self.p.render(self.cb, self.scene, self.gb)
        torch.cuda.synchronize()
        dw, dh = self.display
        return self.p.download_raw(api.OUT_DISPLAY, np.float32, (dh, dw, 4)), self.p.download_raw(api.OUT_DISPLAY_SRGB8, np.uint8, (dh, dw, 4))

    def check(self, picks, to_world=None):
        """the outline of `picks` against the restatement; returns the last pick's mask"""
        base = self.show([])
        got = self.show(picks)
        xf = self.sc.instance_to_world if to_world is None else to_world
        outlines, mask = [], None
        for idx in picks:
            mask = pk.raster_mask(instance_tris(self.sc, idx), pk.wvp(xf[idx], self.cb["curr_view_proj"]), self.display, self.render)
            outlines.append(pk.outline(mask, self.display))
        word = dc.linear_to_srgb8(pk.OUTLINE_RGBA.reshape(1, 1, 4)).view(np.uint32)[0, 0]
        want = pk.apply_outlines(base[0], base[1], outlines, word)
        got_mask = self.p.download_plane("pick_mask")
        assert got_mask.shape == mask.shape and np.array_equal(got_mask, mask), f"mask: {int((got_mask != mask).sum())} pixels differ"
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"display: {int((got[0] != want[0]).any(-1).sum())} pixels differ"
        assert np.array_equal(got[1], want[1])
        assert any(o.any() for o in outlines)
        return mask


@pytest.mark.gpu
@pytest.mark.parametrize("display", [(96, 64), (120, 80)], ids=["display_eq_render", "display_ne_render"])
def test_cornell_instance(display):
    f = Frame(cornell(), (96, 64), display)
    idx = f.pick(48, 40)
    assert idx < len(f.sc.instances)
    mask = f.check([idx])
    assert mask.any() and not mask.all()


@pytest.mark.gpu
def test_partly_off_screen_and_two_picks():
    f = Frame(cornell(), (96, 64), (96, 64), cam_pos=(0.6, 1.0, -2.5))
    a, b = f.pick(2, 32), f.pick(48, 60)
    assert a != b and max(a, b) < len(f.sc.instances)
    f.check([a])
    f.check([a, b])


@pytest.mark.gpu
def test_camera_inside_the_instance_box():
    """the camera inside the Cornell box: the walls cross the near plane and lie partly behind the camera"""
    f = Frame(cornell(), (96, 64), (96, 64), cam_pos=(0.0, 1.0, 0.3), view_dir=(0.4, -0.2, 1.0))
    idx = f.pick(48, 32)
    f.check([idx])


@pytest.mark.gpu
def test_moved_instance():
    sc = cornell()
    f = Frame(sc, (96, 64), (96, 64))
    idx = f.pick(48, 40)
    xf = sc.instance_to_world.copy()
    xf[idx, 3] += np.float32(0.25)
    xf[idx, 7] += np.float32(0.125)
    f.scene.update_instances(sc.instances, xf)
    f.check([idx], to_world=xf)


@pytest.mark.gpu
def test_atrium_largest_instance_1080p():
    sc = scene_io.make_synthetic_scene(num_tris=262144, num_emissive=100000, layout="atrium")
    f = Frame(sc, (1920, 1080), (1920, 1080))
    idx = int(np.argmax(sc.instance_num_tris))
    f.check([idx])


@pytest.mark.gpu
def test_pick_refusals():
    f = Frame(cornell(), (96, 64), (96, 64))
    with pytest.raises(api.ZetaRayError) as e:
        f.show([len(f.sc.instances)])
    assert e.value.code == 1
    with pytest.raises(api.ZetaRayError) as e:
        api.Pass(api.PASS_TAA, 32, 32).set_picked_instances([0])
    assert e.value.code == 1
    f.show([])      # n = 0 clears


@pytest.mark.gpu
def test_cpp_entry_equals_python():
    """zrh_render_display_pick (the C++ mirror: GBufferRT::PickPixel -> ReadPick -> DisplayPass with a view and the outline, through the
    RenderGraph) against the same passes driven from Python, byte for byte"""
    import ctypes as C
    import torch
    sc = cornell()
    f = Frame(sc, (96, 64), (96, 64))
    f.p.set_display_option(wire.DISPLAY_NORMAL)
    idx = f.pick(48, 40)
    f.p_gb.render(f.cb, f.scene, f.gb)
    torch.cuda.synchronize()
    rgba, srgb = f.show([idx])
    mask = f.p.download_plane("pick_mask")
    host = C.CDLL(os.path.join(ROOT, "zetaray_amd", "libzetaray_host.so"))
    img = pc.to_half_bits(pc.hdr_image(seed=5, w=96, h=64))
    out, out8, m8, pick = np.zeros_like(rgba), np.zeros_like(srgb), np.zeros_like(mask), C.c_uint32(0)
    desc, cbb = sc.desc(), np.ascontiguousarray(f.cb)
    vp = C.c_void_p
    host.zrh_render_display_pick.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_float, vp, vp, vp, vp]
    assert host.zrh_render_display_pick(C.addressof(desc), cbb.ctypes.data, 96, 64, img.ctypes.data, 48, 40, wire.DISPLAY_NORMAL, 1.0,
                                        out.ctypes.data, out8.ctypes.data, m8.ctypes.data, C.byref(pick)) == 0
    assert pick.value == idx
    assert np.array_equal(out.view(np.uint32), rgba.view(np.uint32)) and np.array_equal(out8, srgb) and np.array_equal(m8, mask)
