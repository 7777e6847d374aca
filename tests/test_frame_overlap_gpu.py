"""Frame overlap (zetaray_amd.h zr_pass_set_frame_overlap) under forced stream skew: every ordering the event graph allows, against the CPU oracle.

The parity tests of tests/test_gpu_parity.py wait on the host after every frame, so the two halves of consecutive frames never share the device there, and
the back-to-back test relies on 1920 x 1080 kernels happening to overlap.  Here the order is forced (tests/overlapcheck.py): a 150 x 90 sequence of six
frames is rendered stage by stage on two streams without a host wait, and from frame 2 on one bounded spin per frame holds one stream back while the
other runs as far ahead as the library's events let it.  Every frame's FINAL, reservoir planes, target plane and denoised image are snapshotted in
stream order and compared: FINAL, the reservoirs and the ray counters with zro.OracleRPT at tolerance 0, the target plane and the denoise pass's output
(a consumer enqueued behind the frame, reading FINAL) with a single-stream run of the same library.

Cases (overlapcheck.CASES): moving camera + temporal reset; the same with two spatial rounds; three accumulating sequences (FINAL is NOT rotated there, and
K11 adds into it whenever the frame has no temporal reuse).  Schedules: none, reuse_held, spatial_held, consumer_held (stream B held before the temporal
reuse / between it and the spatial stage / before the consumer), candidates_held (stream A held before the G-buffer render).  For the non-accumulating
cases the harness also proves that the skew happened: product mode lets the first half of frame N + 1 finish before the held part of frame N begins;
carry mode lets CANDIDATES(N + 1) finish before SPATIAL(N) begins unless frame N ran two spatial rounds (the set carried over is then written by its
first round, so that frame's K11 waits for the whole of it).  These same assertions pin that the ordering added for accumulating frames does not
serialise the others -- the path bench.py times.  (zr_pass_reset_temporal waits for the device and clears FINAL: the frame it precedes overlaps nothing, and
the oracle's accumulation is cleared with it.)

The stall of a case is 4 x the wall time of two of its plain-order frames (host submission + device), never below 10 ms nor above 50 ms.
Measured on an MI355X (three runs of this file): torch.cuda._sleep counts 2.38 - 2.40 million cycles per ms (the 6.4-million-cycle probe took 2.66 - 2.69 ms);
two plain-order frames take 1.11 ms (moving), 0.95 ms (two_rounds), 0.87 ms (acc_no_temporal), 0.86 ms (acc_reset), 0.84 ms (acc_starts), so every case runs
with the 10 ms floor; a held sequence takes 52 - 54 ms, an unheld one 2 - 3 ms; the 52 tests of the file take 6.6 - 6.8 s.
"""
import numpy as np
import pytest

from tests import overlapcheck as oc

pytestmark = pytest.mark.gpu

W, H = oc.CASES["moving"].w, oc.CASES["moving"].h
_cache = {}


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


@pytest.fixture(scope="module")
def stalls(api, cornell_emissive):
    """per case: (wall ms of two plain-order frames, stall in ms); the spin is calibrated first and fails loudly when it cannot be"""
    cpm = oc.cycles_per_ms()
    out = {}
    for name, case in oc.CASES.items():
        two = oc.plain_frames_wall_ms(api, case, cornell_emissive, 2)
        out[name] = (two, oc.stall_ms_for(two))
    print(f"\nstall calibration: {cpm:.0f} cycles/ms (probe {oc._CAL['probe']}); " + "; ".join(f"{k}: two plain frames {v[0]:.2f} ms -> stall {v[1]:.1f} ms" for k, v in out.items()))
    return out


def _reference(api, name, scene, oscene):
    """per case, computed once: the oracle's sequence and the same library's plain single-stream run"""
    if name not in _cache:
        case = oc.CASES[name]
        want, counters = oc.oracle_sequence(case, scene, oscene)
        plain = oc.drive(api, case, scene, None)
        # the plain order is itself the oracle's (what test_gpu_parity pins; asserted here so that a difference below is the schedule's)
        for f, (g, o) in enumerate(zip(plain.frames, want), 1):
            assert np.array_equal(g["final"].view(np.uint32), o["final"].view(np.uint32)), f"{name}: plain order, frame {f}: FINAL differs from the oracle"
        assert plain.counters == counters, (name, plain.counters, counters)
        _cache[name] = (want, counters, plain)
    return _cache[name]


@pytest.mark.parametrize("schedule", oc.SCHEDULES)
@pytest.mark.parametrize("mode", ["product", "carry"])
@pytest.mark.parametrize("name", list(oc.CASES))
def test_skewed_schedule_equals_oracle(api, cornell_emissive, oracle_emissive, stalls, name, mode, schedule):
    case = oc.CASES[name]
    want, counters, plain = _reference(api, name, cornell_emissive, oracle_emissive)
    two_ms, stall_ms = stalls[name]
    assert (case.frames - 1) * stall_ms < 500.0
    got = oc.drive(api, case, cornell_emissive, mode, schedule, stall_ms)
    print(f"\n{name} {mode} {schedule}: stall {stall_ms:.1f} ms, sequence {got.wall_ms:.1f} ms, ran ahead {got.ran_ahead}")
    bad = []
    for f, (g, o, p) in enumerate(zip(got.frames, want, plain.frames), 1):
        mism = int((g["final"].view(np.uint32) != o["final"].view(np.uint32)).any(axis=2).sum())
        if mism:
            bad.append(f"frame {f}: FINAL differs from the oracle at {mism} pixels (max abs {np.abs(g['final'] - o['final']).max():.3g})")
        if mode == "carry":
            for nm in oc.RES_PLANES:
                a, b = g[nm], o["planes"][nm]
                if nm == "A":
                    a, b = a & 0xffffff, b & 0xffffff
                if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
                    bad.append(f"frame {f}: reservoir plane {nm} differs from the oracle")
            if not np.array_equal(g["target"].view(np.uint8), p["target"].view(np.uint8)):
                bad.append(f"frame {f}: target plane differs from the plain order")
        else:
            masks, _ = oc.used_mask(o["planes"]["A"], True, o["skip"], o["wrote"])
            for nm in oc.RES_PLANES:
                if not oc.masked_equal(g[nm], o["planes"][nm], masks[nm]):
                    bad.append(f"frame {f}: reservoir plane {nm} differs from the oracle on its used bytes")
            tm = np.repeat(oc.target_mask(o["skip"], o["do_temporal"])[..., None], 16, axis=2)
            if not oc.masked_equal(g["target"], p["target"], tm):
                bad.append(f"frame {f}: target plane differs from the plain order at pixels the frame wrote")
        dm = int((g["denoised"].view(np.uint32) != p["denoised"].view(np.uint32)).any(axis=2).sum())
        if dm:
            bad.append(f"frame {f}: denoised plane differs from the plain order at {dm} pixels")
    assert not bad, f"{name} / {mode} / {schedule}:\n  " + "\n  ".join(bad)
    assert got.counters == counters, f"{name} / {mode} / {schedule}: ray counters {got.counters} != oracle {counters}"
    # the harness's own teeth: the skew happened wherever the event graph allows it (zr_pass_reset_temporal is a host call that waits for the device, so
    # nothing of the frame it precedes can run beside the frame before it)
    if name in ("moving", "two_rounds"):
        got.ran_ahead.pop(case.reset_at - 1, None)
        if mode == "product" and schedule in ("reuse_held", "consumer_held"):
            late = [n for n, ok in got.ran_ahead.items() if not ok]
            assert not late, f"{name} / product / {schedule}: the first half of frame N + 1 did not finish before the held part of frame N began, N = {late} " \
                             f"(first halves done at {got.t_first_half}, held parts began at {got.t_held})"
        if mode == "carry" and schedule == "spatial_held":
            # (a frame with two spatial rounds is waited for as a whole: its first round writes the set CANDIDATES(N + 1) carries over.  With num_spatial_passes = 2
            # every frame with temporal reuse runs both rounds; frames 1 and 4 -- the first one and the one after the reset -- run none)
            allowed = [n for n in got.ran_ahead if not (case.nsp == 2 and want[n - 1]["do_temporal"])]
            assert allowed, "no frame left to check"
            late = [n for n in allowed if not got.ran_ahead[n]]
            assert not late, f"{name} / carry / spatial_held: CANDIDATES(N + 1) did not finish before SPATIAL(N) began, N = {late} " \
                             f"(first halves done at {got.t_first_half}, held parts began at {got.t_held})"


@pytest.mark.parametrize("k", [2, 3])
def test_enabling_overlap_keeps_the_previous_gbuffer(api, cornell_emissive, k):
    """zr_pass_set_frame_overlap gives the G-buffer its third plane set.  Whatever renders between that call and the next GBUFFER render must still see the
    previous frame's planes as "previous": two identical renderers with a denoise pass that has history and a moving camera; at frame k both render the
    G-buffer and the indirect pass, one of them then switches overlap on, both run the denoise pass (which reprojects into the previous G-buffer).  Same
    image; k = 2 and 3 are the two parities of the G-buffer's current set.  One more frame after that: the rotation goes on from the right set."""
    from zetaray_amd import wire
    case = oc.Case("switch", lambda f: dict(cam_pos=(0.05 * (f - 1), 1.2, -4.043)), frames=k + 1)
    cbs = case.frame_constants(cornell_emissive)
    rs = []
    for _ in range(2):
        r = api.Renderer(cornell_emissive, W, H, params=wire.default_params(), integrator=api.INTEGRATOR_RESTIR_PT)
        r.enable_denoise()
        for cb in cbs[:k - 1]:
            r.render_frame(cb)
        rs.append(r)
    cb = cbs[k - 1]
    for i, r in enumerate(rs):
        r.p_gbuffer.render(cb, r.scene, r.gbuffer)
        r.p_indirect.render(cb, r.scene, r.gbuffer)
        if i == 1:
            r.enable_frame_overlap(True)
        r.p_denoise.set_input(api.IN_DENOISE_SIGNAL, r.p_indirect.output_ptr()[0])
        r.p_denoise.render(cb, r.scene, r.gbuffer)
    a, b = (r.p_denoise.download_plane("denoised") for r in rs)
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    mism = int((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum())
    assert mism == 0, f"frame {k}: the denoise pass rendered right after overlap was switched on differs at {mism} pixels"
    for r in rs:
        r.render_frame(cbs[k])
    fa, fb = (r.final() for r in rs)
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), f"frame {k + 1}: FINAL differs after the switch"
    a, b = (r.p_denoise.download_plane("denoised") for r in rs)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"frame {k + 1}: denoised plane differs after the switch"
