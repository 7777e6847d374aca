"""The used-byte table of tests/overlapcheck.py (used_mask, target_mask), checked on the CPU: what it calls unused really is.

Frame overlap's product mode (zetaray_amd.h zr_pass_set_frame_overlap) leaves the bytes of a reservoir record that no pass reads to whatever the rotating
third set held, and the GPU tests compare its planes with the oracle's on the used bytes only.  That comparison is as good as the table.  Here oracle
sequences are rendered twice: once untouched, once with every byte the table calls unused overwritten with 0xff (NaN as a float, an impossible index as
an integer) in the frame's final reservoir set after every frame.  FINAL, the ray counters and the used bytes of every later frame must not change.  The
scenes are chosen so that every branch of the table occurs: the emissive Cornell box and a materials scene (NEE_EMISSIVE variant, cases 1 - 3), the sun +
sky Cornell box and an open materials scene under the sky (the other variant, with and without a sky light at x_k / x_k+1).
The target plane has no write access in the oracle; the host executor (the HIP stage functions run serially) has: all of it is poisoned between frames.
"""
import collections
import ctypes as C
import os

import numpy as np
import pytest

from oracle import zro
from zetaray_amd import scene_io, wire
from tests import overlapcheck as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 72, 44      # (not a multiple of the 16-px tiles nor of the 32-px sort tiles)
POISON = 0xff
_hits = collections.Counter()
_scenes_done = set()


def _scene(kind, cornell_emissive, oracle_emissive):
    if kind == "cornell_emissive":
        return cornell_emissive, oracle_emissive, (0.0, 1.2, -4.043), None
    if kind == "cornell_sky":
        sc = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))
        return sc, zro.OracleScene(sc), (0.0, 1.2, -4.043), None
    if kind == "materials":
        sc = scene_io.make_synthetic_scene(num_tris=3000, num_emissive=150, seed=11)
        return sc, zro.OracleScene(sc, force_bvh=True), (0.0, 0.0, -3.5), None
    sc = scene_io.make_synthetic_scene(num_tris=1500, num_emissive=0, seed=5, open_top=True)      # "materials_sky"
    return sc, zro.OracleScene(sc, force_bvh=True), (0.0, 2.0, -3.5), (0.3, -0.8, 0.4)


def _cbs(sc, cam0, sun, frames):
    out, prev = [], None
    for f in range(1, frames + 1):
        cb = scene_io.make_frame_constants(W, H, frame_num=f, num_emissives=len(sc.emissives), cam_pos=(cam0[0] + 0.05 * max(0, f - 2), cam0[1], cam0[2]))
        if sun is not None:
            sd = np.array(sun, np.float32)
            cb["sun_dir"] = sd / np.float32(np.linalg.norm(sd))
        if prev is not None:
            cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
        prev = cb.copy()
        out.append(cb)
    return out


def _write_final_set(o, name, arr):
    L = zro.lib()
    L.zro_rpt_rw_plane_rect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_uint32] * 7 + [C.c_int]
    buf = np.ascontiguousarray(arr)
    assert L.zro_rpt_rw_plane_rect(o.r, 0, zro.OracleRPT.PLANES[name][0], buf.ctypes.data, 0, 0, W, 0, 0, W, H, 1) == 0


def _poison_unused(o, emissive, skip, wrote):
    """overwrite the unused bytes of the set the next frame reads as "previous"; returns how often each branch of the table was taken"""
    planes = {nm: o.plane(nm) for nm in oc.RES_PLANES}
    masks, hit = oc.used_mask(planes["A"], emissive, skip, wrote)
    for nm in oc.RES_PLANES:
        b = planes[nm].view(np.uint8).reshape(H, W, -1).copy()
        assert b.shape == masks[nm].shape
        b[~masks[nm]] = POISON
        _write_final_set(o, nm, b.view(planes[nm].dtype).reshape(planes[nm].shape))
        back = o.plane(nm).view(np.uint8).reshape(H, W, -1)
        assert np.array_equal(back, b), f"plane {nm}: the poisoned bytes did not arrive"
    return hit


@pytest.mark.parametrize("kind,frames,nsp,temporal", [("cornell_emissive", 5, 1, True), ("cornell_emissive", 4, 2, True), ("cornell_emissive", 4, 1, False),
                                                      ("cornell_sky", 4, 1, True), ("materials", 4, 1, True), ("materials_sky", 4, 1, True)])
def test_unused_bytes_of_a_record_are_never_read(cornell_emissive, oracle_emissive, kind, frames, nsp, temporal):
    """temporal = False: ZR_IND_TEMPORAL_RESAMPLE off -- from the second frame on no record is written, and the whole set is poisoned"""
    sc, osc, cam0, sun = _scene(kind, cornell_emissive, oracle_emissive)
    emissive = len(sc.emissives) > 0
    prm = wire.default_params()
    prm.num_spatial_passes = nsp
    if not temporal:
        prm.flags &= ~wire.IND_TEMPORAL_RESAMPLE
    cbs = _cbs(sc, cam0, sun, frames)
    ref, poisoned = zro.OracleRPT(osc, W, H), zro.OracleRPT(osc, W, H)
    n_poisoned = 0
    for f, cb in enumerate(cbs, 1):
        if not emissive:
            osc.sky_lut(cb, 256, 128)
        if f == frames and frames > 4:
            ref.reset_temporal(); poisoned.reset_temporal()      # (a frame without temporal reuse writes its records over the poisoned set's other half)
        gb = osc.gbuffer(cb)
        want = ref.render(cb, prm, gb=gb).copy()
        got = poisoned.render(cb, prm, gb=gb)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{kind}, frame {f}: FINAL changed when the unused bytes of frame {f - 1} were poisoned"
        assert poisoned.counters == ref.counters, f"{kind}, frame {f}: ray counters changed"
        a_ref = ref.plane("A")
        skip = (np.asarray(gb[0][2]).reshape(H, W).astype(np.uint32) & 0x6) != 0
        reset = f == frames and frames > 4
        wrote = (temporal and f >= 2 and not reset) or f == 1 or reset
        masks, _ = oc.used_mask(a_ref, emissive, skip, wrote)
        for nm in oc.RES_PLANES:
            assert oc.masked_equal(poisoned.plane(nm), ref.plane(nm), masks[nm]), f"{kind}, frame {f}: used bytes of plane {nm} changed"
        hit = _poison_unused(poisoned, emissive, skip, wrote)
        _hits.update(hit)
        n_poisoned += sum(int((~m).sum()) for m in masks.values())
    assert n_poisoned > 0 and want[..., :3].max() > 0
    _scenes_done.add(kind)
    print(f"\n{kind} nsp={nsp}: branches so far {dict(_hits)}")


def test_every_branch_of_the_table_occurred():
    """(runs after the sequences above, in file order) each case x variant branch of used_mask was taken by at least one record that was then poisoned"""
    assert _scenes_done == {"cornell_emissive", "cornell_sky", "materials", "materials_sky"}, f"the sequences above did not all run: {_scenes_done}"
    missing = [b for b in oc.BRANCHES if _hits[b] == 0]
    assert not missing, f"branches of used_mask that no record took: {missing}; taken: {dict(_hits)}"


def test_target_plane_carries_nothing_between_frames(cornell_emissive, oracle_emissive):
    """target_mask: nothing reads what another frame left in the target plane.  The host executor's whole target plane is poisoned after every frame (moving
    camera, then a temporal reset): FINAL, counters and every reservoir plane stay the untouched run's.  Within a frame the plane's own values are what the
    frame's K11 wrote, at every pixel with a non-emissive surface: checked against the G-buffer flags."""
    from tests.hostexec import zhx
    hx = zhx.HostExecScene(cornell_emissive, oracle_emissive.alias)
    prm = wire.default_params()
    ref, poisoned = zhx.HostExecRPT(hx, W, H), zhx.HostExecRPT(hx, W, H)
    junk = np.full((H, W, 4), np.nan, np.float32)
    junk.view(np.uint32)[...] = 0xffffffff
    for f, cb in enumerate(_cbs(cornell_emissive, (0.0, 1.2, -4.043), None, 5), 1):
        if f == 5:
            ref.reset_temporal(); poisoned.reset_temporal()
        gb = hx.gbuffer(cb)
        want = ref.render(cb, prm, gb=gb).copy()
        got = poisoned.render(cb, prm, gb=gb)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"frame {f}: FINAL changed when the target plane was poisoned after frame {f - 1}"
        assert poisoned.counters == ref.counters
        for nm in oc.RES_PLANES:
            assert np.array_equal(poisoned.plane(nm).view(np.uint8), ref.plane(nm).view(np.uint8)), f"frame {f}: plane {nm} changed"
        skip = (np.asarray(gb[0][2]).reshape(H, W).astype(np.uint32) & 0x6) != 0
        do_temporal = 2 <= f < 5
        tm = oc.target_mask(skip, do_temporal)
        t_ref, t_poi = ref.plane("target").view(np.uint32), poisoned.plane("target").view(np.uint32)
        assert np.array_equal(t_poi[tm], t_ref[tm]), f"frame {f}: the target plane differs where the frame wrote it"
        if f > 1:
            assert (t_poi[~tm] == 0xffffffff).all(), f"frame {f}: pixels outside target_mask were written"
        if do_temporal:
            assert tm.any() and (t_ref[tm][:, 3] == 0).all()
        poisoned.write_plane_rect("target", 0, junk, (0, 0, W, H))
