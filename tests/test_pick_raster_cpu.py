"""The raster contract of the picked-instance outline (zetaray_amd.h zr_pass_set_picked_instances) held to properties on its numpy restatement
(tests/pickcheck.py), which the GPU tests compare the kernels with bit for bit; and the outline's C ABI without a device."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pickcheck as pk  # noqa: E402
from zetaray_amd import api, wire  # noqa: E402

D = 64                                      # display = render = 64 x 64; w = 1: pixel (px, py) <-> ndc (px / 32 - 1, 1 - py / 32), exact
IDENT = np.eye(4, dtype=np.float32)


def ndc(px, py, z=0.5):
    return [np.float32(px) / np.float32(32) - 1, 1 - np.float32(py) / np.float32(32), z]


def raster(tris, m=IDENT):
    return pk.raster_mask(np.array(tris, np.float32), m, (D, D), (D, D)) != 0


def count(tris):
    """per pixel, how many of the triangles cover it"""
    return sum(raster([t]).astype(int) for t in tris)


def test_quad_split_in_two_covers_every_pixel_once():
    a, b, c, d = ndc(3.3, 5.1), ndc(50.7, 4.2), ndc(55.5, 47.9), ndc(8.25, 44.0)
    n = count([[a, b, c], [a, c, d]])
    assert n.max() == 1
    assert (n == raster([[a, b, c], [a, c, d]])).all() and n.sum() > 1500


def test_fan_has_no_gaps_and_no_double_coverage():
    rng = np.random.default_rng(3)
    centre = ndc(31.5, 30.25)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 13))
    rim = [ndc(32 + 25 * np.cos(t), 32 + 25 * np.sin(t)) for t in ang]
    fan = [[centre, rim[i], rim[(i + 1) % len(rim)]] for i in range(len(rim))]
    n = count(fan)
    assert n.max() == 1
    # no gaps: every pixel strictly inside the rim polygon is covered
    inner = count([[rim[0], rim[i], rim[i + 1]] for i in range(1, len(rim) - 1)])
    assert (n == inner).all()


def test_edges_and_vertices_on_pixel_centres():
    # a 4 x 4-pixel square whose edges run through pixel centres: top-left rule -> exactly 4 x 4 pixels, each once
    a, b, c, d = ndc(10.5, 10.5), ndc(14.5, 10.5), ndc(14.5, 14.5), ndc(10.5, 14.5)
    n = count([[a, b, c], [a, c, d]])
    assert n.max() == 1 and n.sum() == 16 and n[10:14, 10:14].all()
    # the same with the opposite winding and another diagonal
    n2 = count([[a, d, b], [b, d, c]])
    assert (n2 == n).all()


def test_near_plane_and_behind_the_camera():
    # row-vector projection: w = z_view, z_clip = near (infinite reverse-Z); a triangle from in front of the camera to behind it
    near = np.float32(0.1)
    P = np.zeros((4, 4), np.float32)
    P[0, 0], P[1, 1], P[2, 3], P[3, 2] = 1, 1, 1, near
    front = [[-0.5, -0.5, 1.0], [0.5, -0.5, 1.0], [0.0, 0.5, -2.0]]
    m = raster([front], P)
    assert m.any() and not m.all()
    assert not raster([[[-0.5, -0.5, -1.0], [0.5, -0.5, -1.0], [0.0, 0.5, -2.0]]], P).any()      # wholly behind
    # a huge triangle through the near plane (the guard band clips it) still covers the whole screen
    assert raster([[[-50, -50, 0.05], [50, -50, 0.05], [0, 80, 5.0]]], P)[:, :].sum() > 0


def test_mask_does_not_depend_on_triangle_order():
    rng = np.random.default_rng(7)
    tris = rng.uniform(-1.2, 1.2, (200, 3, 3)).astype(np.float32)
    tris[..., 2] = 0.5
    a = raster(tris)
    perm = rng.permutation(len(tris))
    rot = np.roll(tris[perm], 1, axis=1)        # shuffled triangles, rotated vertex order
    assert (raster(rot) == a).all() and a.any()


def test_outline_is_the_mask_edge():
    mask = np.zeros((D, D), np.uint8)
    mask[10:20, 30:40] = 255
    o = pk.outline(mask, (D, D))
    ring = np.zeros((D, D), bool)
    ring[9:21, 29:41] = True
    ring[11:19, 31:39] = False
    assert (o == ring).all()
    # display larger than the mask: out-of-range loads are 0; an empty mask outlines nothing
    assert not pk.outline(np.zeros((D, D), np.uint8), (80, 70)).any()
    full = pk.outline(np.full((D, D), 255, np.uint8), (80, 70))
    want = np.zeros((70, 80), bool)
    want[:D + 1, :D + 1] = True
    want[1:D - 1, 1:D - 1] = False        # the mask's own border rows / columns and the row / column just past the render size
    assert (full == want).all()


def test_c_abi_declares_picked_instances():
    L = api.lib()
    assert "zr_pass_set_picked_instances" in api.EXPORTS
    assert L.zr_pass_set_picked_instances(None, None, 0) == 1
    assert b"DISPLAY" in L.zr_last_error()
    hdr = open(os.path.join(ROOT, "include", "zetaray_amd.h")).read()
    assert re.search(r"#define\s+ZR_OUT_PICK_MASK\s+50\b", hdr) and wire.OUT_PICK_MASK == 50
    import ctypes as C
    host = C.CDLL(os.path.join(ROOT, "zetaray_amd", "libzetaray_host.so"))
    assert hasattr(host, "zrh_render_display_pick")
    if api.device_count() == 0:
        with pytest.raises(api.ZetaRayError) as e:
            api.Pass(api.PASS_DISPLAY, 64, 64)
        assert e.value.code == 2
