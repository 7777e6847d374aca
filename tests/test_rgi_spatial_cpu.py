"""ReSTIR GI's spatial reuse stage (zr_rgi_spatial.h, zr_pass_set_rgi_spatial) on the CPU: the stage function k_rgi_spatial inlines, compiled for the
host (tests/rgispatial) and run behind the host executor of k_rgi (tests/hostexec).  The stage has no reference counterpart, so it is held to
properties: its mean agrees with the K9 path tracer, without neighbours it returns k_rgi's own radiance, and it lowers the variance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.hostexec import zhx
from tests.rgispatial import setter, zrs
from zetaray_amd import api, scene_io, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the 8-point tap table of the contract (zr_rgi_spatial.h, item 2)
TAPS = np.array([(0.0, -7 / 9), (-0.5, -5 / 9), (0.5, -3 / 9), (-0.75, -1 / 9), (0.25, 1 / 9), (-0.25, 3 / 9), (0.75, 5 / 9), (-0.875, 7 / 9)])


def _cb(sc, w, h, f, **kw):
    return scene_io.make_frame_constants(w, h, frame_num=f, num_emissives=len(sc.emissives), **kw)


@pytest.fixture(scope="module")
def hx_emissive(cornell_emissive, oracle_emissive):
    return zhx.HostExecScene(cornell_emissive, oracle_emissive.alias)


# The 16-px default radius is sized for a 1080p frame.  In the 48 x 32 frame of the tests below most of its taps (offsets of 4.4 .. 18.7 px) leave
# the frame or land on another wall, so hardly anything is reused; a radius of 4 px keeps every offset (1.1 .. 4.7 px) inside the frame for all but
# the border pixels.  Both are run: the mean must agree with K9 at both, the variance must fall where the stage has neighbours to reuse.
RADII = (0.0, 4.0)


@pytest.fixture(scope="module")
def run200(cornell_emissive, oracle_emissive, hx_emissive):
    """emissive Cornell, 48 x 32, 200 frames, static camera: per frame K9 (the oracle's path tracer), temporal-only GI (k_rgi's own radiance) and
    temporal + spatial GI (2 neighbours; the default radius and 4 px) on the same reservoirs -- the spatial stage writes nothing back, so one k_rgi
    run serves all three; then K9 once more over the disjoint frame numbers 201..400 (the noise floor)"""
    w, h, n = 48, 32, 200
    prm = wire.default_params()
    gi = zhx.HostExecRGI(hx_emissive, w, h)
    s9, s9b, st = (np.zeros((h, w, 3), np.float64) for _ in range(3))
    ss = {r: np.zeros((h, w, 3), np.float64) for r in RADII}
    last_t, last_s, rays = [], {r: [] for r in RADII}, {r: 0 for r in RADII}
    for f in range(1, n + 1):
        cb = _cb(cornell_emissive, w, h, f)
        gb9 = oracle_emissive.gbuffer(cb)      # (held: the planes struct points into its arrays)
        s9 += oracle_emissive.pathtrace(cb, gb9[1], prm)[0][..., :3]
        gb = hx_emissive.gbuffer(cb)
        t = gi.render(cb, prm, gb)[..., :3].copy()
        st += t
        if f > n - 100:
            last_t.append(t)
        planes = {k: gi.plane(k) for k in "ABC"}
        for r in RADII:
            s, cnt = zrs.spatial(hx_emissive, cb, gb, planes, 2, r)
            assert not np.isnan(s).any()
            ss[r] += s[..., :3]
            rays[r] += cnt[1]
            if f > n - 100:
                last_s[r].append(s[..., :3].copy())
    for f in range(n + 1, 2 * n + 1):
        cb = _cb(cornell_emissive, w, h, f)
        gb9 = oracle_emissive.gbuffer(cb)
        s9b += oracle_emissive.pathtrace(cb, gb9[1], prm)[0][..., :3]
    return {"m9": s9.mean(axis=(0, 1)) / n, "m9b": s9b.mean(axis=(0, 1)) / n, "mt": st.mean(axis=(0, 1)) / n,
            "ms": {r: ss[r].mean(axis=(0, 1)) / n for r in RADII}, "var_t": float(np.var(np.stack(last_t), axis=0).mean()),
            "var_s": {r: float(np.var(np.stack(last_s[r]), axis=0).mean()) for r in RADII}, "rays": {r: rays[r] / (w * h * n) for r in RADII}}


def test_rgi_spatial_mean_agrees_with_k9(run200):
    """image-mean RGB over 200 frames: d_s = |spatial - K9| <= d_t + d_0 per channel, d_t = |temporal-only - K9|, d_0 = |K9' - K9| (two K9 runs over
    disjoint frame numbers): two estimates of one mean differ by at most the sum of their noises.
    Measured (K9 mean 0.01327, 0.00860, 0.00451): d_t = (4.6e-4, 2.2e-4, 6.3e-5), d_0 = (4.5e-4, 2.5e-4, 2.2e-4); d_s = (4.2e-4, 2.0e-4, 5.2e-5) at the
    16-px default, (3.4e-4, 1.7e-4, 3.7e-5) at 4 px."""
    d_t, d_0 = np.abs(run200["mt"] - run200["m9"]), np.abs(run200["m9b"] - run200["m9"])
    print("rgi spatial vs K9: means K9 %s temporal-only %s; d_t %s d_0 %s" % (run200["m9"], run200["mt"], d_t, d_0))
    for r in RADII:
        d_s = np.abs(run200["ms"][r] - run200["m9"])
        print("  radius %g: mean %s d_s %s" % (r or 16.0, run200["ms"][r], d_s))
        assert np.all(d_s <= d_t + d_0), (r, d_s, d_t, d_0)


def test_rgi_spatial_lowers_variance(run200):
    """per-pixel variance over the last 100 frames, averaged over the image and the channels: spatial on / off < 1 at the radius that fits the frame
    (4 px; RADII above).  At the 16-px default the 48 x 32 frame leaves the stage next to nothing to reuse and the ratio is 1 within noise: printed.
    Measured: 0.917 at 4 px (1.54 visibility rays per pixel and frame), 1.0045 at 16 px (0.66)."""
    ratio = {r: run200["var_s"][r] / run200["var_t"] for r in RADII}
    for r in RADII:
        print("rgi spatial variance ratio (on / off), radius %g: %.4f with %.2f visibility rays per pixel and frame" % (r or 16.0, ratio[r], run200["rays"][r]))
    assert run200["rays"][4.0] > run200["rays"][0.0], "the fitting radius reuses more"
    assert ratio[4.0] < 1.0, ratio


def test_rgi_spatial_without_neighbours_returns_k_rgi_radiance(cornell_emissive, hx_emissive):
    """k = 0: with no accepted tap the stage streams the canonical reservoir alone, and the radiance is k_rgi's own within relative 2^-10 per channel --
    the only difference is the half rounding of Lo (11-bit significand) through a product linear in Lo.
    The pixel set: every pixel of a 12 x 8 frame at radius 64.  The shortest tap offset is 64 * min |table point| = 17.5 px, rint moves a tap by at
    most sqrt(0.5) px, and no two pixels of the frame are further apart than its diagonal, 13.04 px: every tap of every pixel is out of bounds."""
    w, h, radius = 12, 8, 64.0
    shortest = radius * np.linalg.norm(TAPS, axis=1).min() - np.sqrt(0.5)
    assert shortest > np.hypot(w - 1, h - 1), (shortest, np.hypot(w - 1, h - 1))
    prm = wire.default_params()
    gi = zhx.HostExecRGI(hx_emissive, w, h)
    lit = 0
    for f in range(1, 9):
        cb = _cb(cornell_emissive, w, h, f)
        gb = hx_emissive.gbuffer(cb)
        t = gi.render(cb, prm, gb)[..., :3].copy()
        s, cnt = zrs.spatial(hx_emissive, cb, gb, {k: gi.plane(k) for k in "ABC"}, 2, radius)
        assert cnt == (0, 0), "no neighbour, no visibility ray"
        s = s[..., :3]
        lit += int((t > 0).any(axis=-1).sum())
        err = np.abs(s.astype(np.float64) - t)
        worst = float((err / np.maximum(t, 1e-30)).max())
        print("frame %d: lit pixels %d, worst relative difference %.3e" % (f, int((t > 0).any(axis=-1).sum()), worst))
        assert np.all(err <= 2.0 ** -10 * t), f"frame {f}: worst relative difference {worst}"
    assert lit > 0, "the pixel set is empty"


def test_rgi_spatial_setter_arguments():
    """the C ABI, the Python layer and the C++ host layer declare the setter, and a null pass is ZR_ERR_INVALID_ARG.
    PARTIAL WITHOUT A DEVICE: a pass cannot be created without one, so on a machine without a GPU this test checks the declarations and the null-pass
    error only and returns; every other argument error and the stored-without-effect behaviour for the other integrators (setter.check_setter_arguments)
    run here only when a device is present, and always in tests/test_rgi_spatial_gpu.py::test_rgi_spatial_setter_arguments_on_device."""
    L = api.lib()
    assert "zr_pass_set_rgi_spatial" in api.EXPORTS
    assert L.zr_pass_set_rgi_spatial(None, 1, 0.0) == 1          # ZR_ERR_INVALID_ARG
    assert b"INDIRECT" in L.zr_last_error()
    hdr = open(os.path.join(ROOT, "include", "zetaray_amd.h")).read()
    assert re.search(r"int zr_pass_set_rgi_spatial\(zr_pass\* pass, uint32_t num_samples, float radius_px\);", hdr)
    assert hasattr(api.Pass, "set_rgi_spatial") and hasattr(api.Renderer, "set_rgi_spatial")
    assert (wire.RGI_SPATIAL_MAX_SAMPLES, wire.RGI_SPATIAL_DEFAULT_RADIUS, wire.RGI_SPATIAL_MAX_RADIUS) == (2, 16.0, 64.0)
    assert "SetGISpatialResampling" in open(os.path.join(ROOT, "zetaray_amd", "host", "zr_host.h")).read()
    assert wire.default_params().flags & wire.IND_SPATIAL_RESAMPLE, "the default params keep the bit ReSTIR GI ignores"
    assert L.zr_abi_version() == 3
    if api.device_count() == 0:
        with pytest.raises(api.ZetaRayError) as e:
            api.Pass(api.PASS_INDIRECT, 64, 64, api.INTEGRATOR_RESTIR_GI)
        assert e.value.code == 2                                 # ZR_ERR_NO_DEVICE
        return
    setter.check_setter_arguments()
