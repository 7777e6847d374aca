"""ZR_ALIAS_BUILD_DEVICE on the GPU: the kernels of zr_tu_alias.hip against include/zr_alias.h on the host (tests/aliasmath/libzal.so), byte for byte, on
caller buffers and through the scene path -- a PRELIGHTING render that builds the table on its stream, the same frame sampling it -- and the estimator
it feeds against the host-built table's.

Measured on the MI355X: test_estimator_agrees_with_the_host_table, Cornell box E_dev = 0 (identical frames: its two lights leave both builds one
pairing), E_0 = 0.001395; 3 000-light scene E_dev = 0.011111, E_0 = 0.039361; test_fast_arith_build_is_valid 0.2855 of the bound.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.aliasmath import cases, zal
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST_LIB = os.path.join(ROOT, "zetaray_amd", "libzetaray_amd_fast.so")


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


@pytest.fixture(scope="module")
def many_lights():
    return scene_io.make_synthetic_scene(num_tris=2000, num_emissive=3000, seed=5)


def _frame(scene, w, h, frame=1, **kw):
    return scene_io.make_frame_constants(w, h, frame_num=frame, num_emissives=len(scene.emissives), **kw)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _quadruple_strength(e):
    """the record of one light with 4 x its strength (f16 in packed_b's high half, its low 4 bits repeated in packed_a's top nibble)"""
    e = e.copy()
    s_old = np.uint16(int(e["packed_b"][0]) >> 16).view(np.float16)
    s_new = int(np.float16(np.float32(s_old) * np.float32(4.0)).view(np.uint16))
    e["packed_b"] = (int(e["packed_b"][0]) & 0xFFFF) | (s_new << 16)
    e["packed_a"] = (int(e["packed_a"][0]) & 0x0FFFFFFF) | ((s_new & 0xF) << 28)
    return e


# ---- (a) the kernels on caller buffers
@pytest.mark.parametrize("case", cases.all_cases(cases.SIZES + cases.SIZES_GPU_EXTRA) + list(cases.LARGE_CASES), ids=lambda c: "%s-%d" % c)
def test_build_device_equals_the_header(api, case):
    p = cases.powers(*case)
    got, want = api.alias_table_build_device(p), zal.build(p)
    for f in ("cached_p_orig", "alias", "p_curr", "cached_p_alias"):
        assert _same(got[f], want[f]), (f, int((got[f].view(np.uint32) != want[f].view(np.uint32)).sum()))
    assert _same(got, want)


def test_build_device_refuses_empty_input(api):
    assert api.lib().zr_alias_table_build_device(0, None, None, 0, None) == 1


def test_build_device_survives_unspecified_input(api):
    """outside the caller guarantee (NaN, inf, negative, all zero) the bytes are unspecified, but every alias is < n (after the quantisation everything is integer and bounded by the counts)"""
    p = cases.powers("log_uniform", 1000).copy()
    p[3], p[500], p[700] = np.nan, np.inf, -1.0
    # powers that cancel: probs of 1e9 or so in 70 000 lights, every weight at the clamp, the integer sums wrap around 2^64
    c = np.where(np.arange(70000) % 2 == 1, np.float32(1e6), np.float32(-1e6 + 1e-3)).astype(np.float32)
    for q in (p, np.zeros(257, np.float32), c):
        t, h = api.alias_table_build_device(q), zal.build(q)
        assert (t["alias"] < len(q)).all() and (h["alias"] < len(q)).all()
        assert (t["p_curr"] >= 0).all() and (t["p_curr"] <= 1).all()


def test_fast_arith_build_is_valid(api):
    """the tolerance-mode library (its divide is the 2.5-ulp one, so its bytes are its own) still builds a valid table: the bound of the CPU test"""
    assert os.path.exists(FAST_LIB), "libzetaray_amd_fast.so is missing: __graft_entry__.build() builds it"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "aliasmath", "fast_check.py")], env=dict(os.environ, ZETARAY_AMD_LIB=FAST_LIB),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep["lib"] == "libzetaray_amd_fast.so"
    print("fast build, max of the bound:", max(rep["excess"].values()))
    assert max(rep["excess"].values()) <= 1.0, rep


# ---- (b), (e) the scene path
@pytest.mark.parametrize("which", ["cornell", "many_lights"])
def test_prelighting_builds_the_headers_table_on_the_device(api, cornell_emissive, many_lights, which):
    sc = cornell_emissive if which == "cornell" else many_lights
    n = len(sc.emissives)
    cb = _frame(sc, 32, 32)
    dev, host = api.Renderer(sc, 32, 32), api.Renderer(sc, 32, 32)
    dev.set_alias_build("device")
    dev.p_prelight.render(cb, dev.scene)
    host.p_prelight.render(cb, host.scene)
    power = dev.p_prelight.get_emissive_powers(n)
    assert _same(power, host.p_prelight.get_emissive_powers(n)) and power.sum() > 0
    got = dev.scene.get_alias_table()
    assert _same(got, zal.build(power))
    t_host = host.scene.get_alias_table()
    assert _same(got["cached_p_orig"], t_host["cached_p_orig"])
    # (e) with nothing set the table is the reference's
    assert _same(t_host, api.alias_table_build(power))
    if which == "many_lights":
        assert not _same(got, t_host)                       # ... and the device mode's is not
    # back to the host mode: the next rebuild is the host's again
    dev.set_alias_build("host")
    dev.scene.invalidate_alias_table()
    dev.p_prelight.render(cb, dev.scene)
    assert _same(dev.scene.get_alias_table(), t_host)


def test_setter_refuses_bad_modes_and_keeps_the_mode(api, cornell_emissive):
    r = api.Renderer(cornell_emissive, 32, 32)
    r.set_alias_build("device")
    for bad in (-1, 2, 100):
        with pytest.raises(api.ZetaRayError) as e:
            r.scene.set_alias_build(bad)
        assert e.value.code == 1
    cb = _frame(cornell_emissive, 32, 32)
    r.p_prelight.render(cb, r.scene)
    power = r.p_prelight.get_emissive_powers(len(cornell_emissive.emissives))
    assert _same(r.scene.get_alias_table(), zal.build(power))          # still the device mode
    with pytest.raises(api.ZetaRayError):
        r.p_gbuffer.get_emissive_powers(len(cornell_emissive.emissives))


# ---- (c) the frame that finds the table stale samples the new one
@pytest.mark.parametrize("deferred", [False, True], ids=["invalidate", "invalidate_deferred"])
@pytest.mark.parametrize("which", ["cornell", "many_lights"])
def test_same_frame_samples_the_rebuilt_table(api, cornell_emissive, many_lights, which, deferred):
    import copy
    import torch
    sc = copy.copy(cornell_emissive if which == "cornell" else many_lights)      # the shared scene, with light records of this test's own
    sc._desc, sc.emissives = None, sc.emissives.copy()
    n = len(sc.emissives)
    w, h = 64, 48
    dprm = wire.default_params_di()
    st = torch.cuda.Stream()
    a = api.Renderer(sc, w, h)
    a.set_alias_build("device")
    di_a = a.enable_direct(dprm)
    a.skip_indirect = True
    cam = {} if which == "cornell" else dict(cam_pos=(0, 0, -3.5))                  # (inside the synthetic room)
    a.p_prelight.render(_frame(sc, w, h, 1, **cam), a.scene, None, st.cuda_stream)    # the table of the old strengths
    old = a.scene.get_alias_table()
    # everything from here to the read-backs is enqueued on one stream, no host wait in between
    e = _quadruple_strength(sc.emissives[0:1])
    a.scene.update_emissives(e, 0, stream=st.cuda_stream)
    a.invalidate_alias_table(deferred=deferred)
    cb = _frame(sc, w, h, 2, **cam)
    a.p_gbuffer.render(cb, a.scene, a.gbuffer, st.cuda_stream)
    a.p_prelight.render(cb, a.scene, None, st.cuda_stream)
    di_a.render(cb, a.scene, a.gbuffer, st.cuda_stream)
    st.synchronize()
    power = a.p_prelight.get_emissive_powers(n, st.cuda_stream)
    table = a.scene.get_alias_table()
    assert _same(table, zal.build(power)) and not _same(table, old)
    # a fresh device-mode scene created with the new records, same frame number, no temporal history on either side
    sc.emissives[0:1] = e
    b = api.Renderer(sc, w, h)
    b.set_alias_build("device")
    di_b = b.enable_direct(dprm)
    b.skip_indirect = True
    b.render_frame(cb)
    assert _same(b.p_prelight.get_emissive_powers(n), power)
    assert _same(b.scene.get_alias_table(), table)
    fa, fb = di_a.download(stream=st.cuda_stream), di_b.download()
    assert fb[..., :3].max() > 0
    assert _same(fa, fb)
    assert di_a.read_counters(stream=st.cuda_stream) == di_b.read_counters()


# ---- (d) the estimator
def _di_block_means(api, sc, mode, frames, w=256, h=256, **cam):
    r = api.Renderer(sc, w, h)
    r.set_alias_build(mode)
    di = r.enable_direct(wire.default_params_di())
    r.skip_indirect = True
    acc = np.zeros((h, w, 3), np.float64)
    for f in frames:
        r.render_frame(_frame(sc, w, h, f, camera_static=1, **cam))
        acc += di.download()[..., :3]
    acc /= len(frames)
    return acc.reshape(h // 8, 8, w // 8, 8, 3).mean(axis=(1, 3))


@pytest.mark.parametrize("which", ["cornell", "many_lights"])
def test_estimator_agrees_with_the_host_table(api, cornell_emissive, many_lights, which):
    """emissive DI, 256 x 256, 64 frames, static camera: the 8 x 8-block means (32 x 32 x 3 = 3 072 values) of the device-table frames differ from the
    host-table frames' by no more than 1.25 x what two host-table runs over disjoint frame numbers differ by (relative L2).  On the Cornell box (the
    scene the bound was set for) both builds pair its two lights the same way and the frames are identical; the 3 000-light scene is where the two
    tables differ in most entries, so a table whose draws and pdf disagreed would show there"""
    sc = cornell_emissive if which == "cornell" else many_lights
    cam = {} if which == "cornell" else dict(cam_pos=(0, 0, -3.5))
    host_1 = _di_block_means(api, sc, "host", range(1, 65), **cam)
    host_2 = _di_block_means(api, sc, "host", range(65, 129), **cam)
    dev = _di_block_means(api, sc, "device", range(1, 65), **cam)

    def rel_l2(x, ref):
        return float(np.sqrt(((x - ref) ** 2).sum() / (ref ** 2).sum()))
    e_dev, e_0 = rel_l2(dev, host_1), rel_l2(host_2, host_1)
    print("alias estimator agreement (%s): E_dev = %.6f, E_0 = %.6f" % (which, e_dev, e_0))
    assert e_0 > 0
    assert e_dev <= 1.25 * e_0, (e_dev, e_0)


def test_mode_change_drops_a_pending_deferred_rebuild(api, cornell_emissive):
    """a deferred host rebuild whose read-back is in flight when the scene goes to device mode must not feed a later host build with its old powers"""
    import copy
    import torch
    sc = copy.copy(cornell_emissive)
    sc._desc, sc.emissives = None, sc.emissives.copy()
    n = len(sc.emissives)
    r = api.Renderer(sc, 32, 32)
    cb = _frame(sc, 32, 32)
    r.p_prelight.render(cb, r.scene)
    old_power = r.p_prelight.get_emissive_powers(n)
    r.scene.invalidate_alias_table_deferred()
    r.p_prelight.render(cb, r.scene)                      # host mode, phase 1: K2 + read-back in flight
    r.set_alias_build("device")
    r.p_prelight.render(cb, r.scene)                      # the table was stale: built on the device, the pending rebuild dropped
    r.scene.update_emissives(_quadruple_strength(sc.emissives[0:1]), 0)
    r.set_alias_build("host")
    r.scene.invalidate_alias_table_deferred()
    for _ in range(2):                                    # phase 1 with the new records, then the build once the read-back has landed
        r.p_prelight.render(cb, r.scene)
        torch.cuda.synchronize()
    power = r.p_prelight.get_emissive_powers(n)
    assert not _same(power, old_power)
    assert _same(r.scene.get_alias_table(), api.alias_table_build(power))
