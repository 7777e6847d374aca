"""Frame overlap under forced stream skew (zetaray_amd.h zr_pass_set_frame_overlap): a helper module like tests/raycheck.py.

Two things live here.

1. used_mask / target_mask: which bytes of a ReSTIR PT reservoir record, and which pixels of the target plane, any pass ever reads.  The product mode of
   frame overlap promises the plain order's values for exactly those (the others are whatever the rotating third set held), so they are what its tests
   compare.  tests/test_frame_overlap_cpu.py checks the table on the CPU by poisoning everything outside it.

2. The skewed-schedule driver: a ReSTIR PT sequence rendered stage by stage on two streams without a host wait, one stream held back by a bounded spin
   (torch.cuda._sleep) while the other runs as far ahead as the library's events allow, every frame's planes snapshotted on the device in stream order.
   What overlaps is then decided by the schedule, not by the size of the kernels: frames of a hundred pixels a side are enough.
"""
import ctypes as C

import numpy as np

RES_PLANES = ("A", "B", "C", "D", "E", "F", "G")
PLANE_BYTES = {"A": 4, "B": 8, "C": 16, "D": 16, "E": 2, "F": 8, "G": 8, "target": 16, "final": 16, "denoised": 16}
SCHEDULES = ("none", "reuse_held", "spatial_held", "consumer_held", "candidates_held")

# ------------------------------------------------------------------------------------------------ used bytes of a reservoir record
# zetaray_amd/csrc/zr_rpt.h, the three loaders are the definition:
#   UnpackMetadata (345-356)        A: bytes 0, 1, 2 (k and M; the two lobes and lt_k; lt_k_plus_1 and x_k_in_motion).  Byte 3 is never read.
#   Load_NonReconnection (460-461)  B: both floats, for every record.
#   Load_Reconnection (358-395)     by the record's case (Reconnection::IsCase1 / 2 / 3, 236-238: case 2 = lt_k_plus_1 != NONE, case 3 = lt_k != NONE and
#                                   not case 2, case 1 = neither) and the pass's NEE_EMISSIVE variant:
#       not emissive, case 2 (364-372)   C.x C.y C.z C.w  D.x D.y  G.y ; D.z D.w only when lt_k_plus_1 == SKY (370)
#       not emissive, case 3 (364-373)   C.x C.y C.z ; D.z D.w only when lt_k == SKY (373)
#       case 1, either variant (377-381) C (all), D (all), E, G.y
#       emissive, case 2 (377-387)       C (all), D (all), E, F.x F.y, G.x G.y
#       emissive, case 3 (377-393)       C (all: C.x is the jacobian or, with lobe_k_min_1 == ALL, seed_nee), D (all), E, F.x
#   An empty record (k == EMPTY, 235) is never handed to Load_Reconnection by a pass that uses the result, and the lobes and light types UnpackMetadata takes
#   from bytes 1 and 2 of A describe a reconnection vertex it does not have: byte 0 of A (k, M) and B only.  (The spatial pass's copy of an empty record writes no
#   more than that: StcCopyToNextFrame -> WriteReservoirData, 2582-2585, 398-403.)
# Which records are there to be loaded at all comes before the table.  K11 leaves a pixel without a surface, or with an emissive one, untouched (PtInitLane_*,
# 1259-1263) and every later pass tests the same G-buffer flags before it loads a record, so what such a pixel holds is another frame's leftover: no byte counts.
# And a frame that neither resamples temporally nor follows a reset writes no record anywhere (prm.writeReservoirs, zr_api.hip RenderReSTIR_PT): its "planes"
# are the leftovers of the set whose turn it is, and no byte counts.
LT_NONE, LT_SKY = 0, 2      # zr_rpt.h:57 enum LT: NONE, SUN, SKY, EMISSIVE
BRANCHES = ("skipped", "empty", "case1_emissive", "case2_emissive", "case3_emissive", "case1_sky", "case2_sky_lt_sky", "case2_sky_lt_other", "case3_sky_lt_sky", "case3_sky_lt_other")


def record_cases(A):
    """per pixel, from plane A alone (what UnpackMetadata reads): empty, case 1 / 2 / 3, lt_k, lt_k_plus_1"""
    a = np.asarray(A, np.uint32).reshape(A.shape[0], A.shape[1])
    empty = (a & 0xf) == 0xf
    lt_k = (a >> 14) & 0x3
    lt_k1 = (a >> 16) & 0x3
    case2 = lt_k1 != LT_NONE
    case3 = (lt_k != LT_NONE) & ~case2
    case1 = ~case2 & ~case3
    return empty, case1, case2, case3, lt_k, lt_k1


def used_mask(A, emissive, skip=None, wrote=True):
    """A: plane A of a reservoir set, (h, w[, 1]) uint32; emissive: the pass runs its NEE_EMISSIVE variant (the scene has emissive triangles); skip: (h, w) bool,
    the pixels the frame's K11 left alone (oracle_sequence); wrote: the frame wrote its records (prm.writeReservoirs).
    Returns ({plane: (h, w, bytes per pixel) bool}, {branch of the table: number of records that took it})."""
    empty, case1, case2, case3, lt_k, lt_k1 = record_cases(A)
    h, w = empty.shape
    there = np.full((h, w), bool(wrote)) if skip is None else (~np.asarray(skip, bool) & bool(wrote))
    m = {nm: np.zeros((h, w, PLANE_BYTES[nm]), bool) for nm in RES_PLANES}
    m["A"][there, 0:1] = True
    m["B"][there] = True
    live = ~empty & there
    m["A"][live, 1:3] = True
    hit = {"skipped": int((~there).sum()), "empty": int((empty & there).sum())}

    def put(name, sel, plane_bytes):
        hit[name] = int(sel.sum())
        for nm, lo, hi in plane_bytes:
            m[nm][sel, lo:hi] = True

    if emissive:
        put("case1_emissive", live & case1, [("C", 0, 16), ("D", 0, 16), ("E", 0, 2), ("G", 4, 8)])
        put("case2_emissive", live & case2, [("C", 0, 16), ("D", 0, 16), ("E", 0, 2), ("F", 0, 8), ("G", 0, 8)])
        put("case3_emissive", live & case3, [("C", 0, 16), ("D", 0, 16), ("E", 0, 2), ("F", 0, 4)])
    else:
        put("case1_sky", live & case1, [("C", 0, 16), ("D", 0, 16), ("E", 0, 2), ("G", 4, 8)])
        put("case2_sky_lt_sky", live & case2 & (lt_k1 == LT_SKY), [("C", 0, 16), ("D", 0, 16), ("G", 4, 8)])
        put("case2_sky_lt_other", live & case2 & (lt_k1 != LT_SKY), [("C", 0, 16), ("D", 0, 8), ("G", 4, 8)])
        put("case3_sky_lt_sky", live & case3 & (lt_k == LT_SKY), [("C", 0, 12), ("D", 8, 16)])
        put("case3_sky_lt_other", live & case3 & (lt_k != LT_SKY), [("C", 0, 12)])
    return m, hit


def target_mask(gb_mr_flags_invalid_or_emissive, do_temporal):
    """The target plane is one frame's scratch: K11 writes it (PtFinishLane, zr_rpt.h:1665: all four components, at every pixel with a non-emissive surface,
    in frames with temporal reuse), K14 and K16 of the SAME frame read x, y, z at those pixels (2256, 2613) and K14 rewrites them (2296).  Nothing reads a
    value another frame left there, so between frames no byte counts (tests/test_frame_overlap_cpu.py poisons the whole plane); what one frame leaves behind
    is defined -- and compared -- at the pixels that frame wrote.  Returns (h, w) bool."""
    skip = np.asarray(gb_mr_flags_invalid_or_emissive, bool)
    return (~skip) if do_temporal else np.zeros_like(skip)


def masked_equal(a, b, mask):
    """a, b: planes of the same shape and dtype; mask: (h, w, bytes per pixel) bool.  True when they agree on every masked byte."""
    h, w = mask.shape[:2]
    ab = np.ascontiguousarray(a).view(np.uint8).reshape(h, w, -1)
    bb = np.ascontiguousarray(b).view(np.uint8).reshape(h, w, -1)
    return bool(np.array_equal(ab[mask], bb[mask]))


def used_bytes_digest(planes, emissive, skip=None, do_temporal=True, wrote=True):
    """sha1 over the used bytes of a reservoir set (every other byte taken as 0) and, when `skip` is given (the pixels K11 skips, see oracle_sequence), over
    the target plane at the pixels the frame wrote.  planes: {"A" .. "G"[, "target"]: array}."""
    import hashlib
    m, _ = used_mask(planes["A"], emissive, skip, wrote)
    hh = hashlib.sha1()
    for nm in RES_PLANES:
        b = np.ascontiguousarray(planes[nm]).view(np.uint8).reshape(m[nm].shape)
        hh.update(np.where(m[nm], b, 0).tobytes())
    if skip is not None:
        tm = target_mask(skip, do_temporal)
        t = np.ascontiguousarray(planes["target"]).view(np.uint8).reshape(tm.shape[0], tm.shape[1], 16)
        hh.update(np.where(tm[..., None], t, 0).tobytes())
    return hh.hexdigest()


# ------------------------------------------------------------------------------------------------ bounded spins
_CAL = {}
MAX_SPIN_CYCLES = 1 << 26


def cycles_per_ms():
    """torch.cuda._sleep counts "cycles" of a clock whose rate is not documented for this device: measured once per process with timing events.  Starts at
    1e5 cycles and doubles until one spin measures at least 2 ms; fails loudly when 2^26 cycles do not get there."""
    import torch
    if "cpm" in _CAL:
        return _CAL["cpm"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)      # (the spin kernel's code object is loaded by its first launch)
    s.synchronize()
    cycles = 100000
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            torch.cuda._sleep(cycles)
            e1.record(s)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 2.0:
            break
        cycles *= 2
        assert cycles <= MAX_SPIN_CYCLES, f"stall calibration: {cycles // 2} cycles of torch.cuda._sleep measure {ms:.3f} ms, 2 ms not reached within 2^26 cycles"
    _CAL["cpm"] = cycles / ms
    _CAL["probe"] = (cycles, ms)
    return _CAL["cpm"]


def stall(stream, ms):
    """one bounded spin of `ms` milliseconds on `stream` (a torch.cuda.Stream; the pass's own stream A: torch.cuda.ExternalStream(frame_overlap_stream()))"""
    import torch
    n = int(cycles_per_ms() * ms)
    with torch.cuda.stream(stream):
        while n > 0:      # (no launch spins for more than 2^26 cycles)
            k = min(n, MAX_SPIN_CYCLES)
            torch.cuda._sleep(k)
            n -= k


def stall_ms_for(two_frames_wall_ms):
    """4 x the wall time of two plain-order frames (so that the leading stream's half AND the host's submission of the next frame fit inside), within [10, 50] ms"""
    return float(min(50.0, max(10.0, 4.0 * two_frames_wall_ms)))


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, cb_kw, reset_at=None, num_spatial_passes=1, temporal=True, w=150, h=90, frames=6):
        self.name, self.cb_kw, self.reset_at, self.nsp, self.temporal, self.w, self.h, self.frames = name, cb_kw, reset_at, num_spatial_passes, temporal, w, h, frames

    def params(self):
        from zetaray_amd import wire
        prm = wire.default_params()
        prm.num_spatial_passes = self.nsp
        if not self.temporal:
            prm.flags &= ~wire.IND_TEMPORAL_RESAMPLE
        return prm

    def frame_constants(self, scene):
        """the sequence's frame constants, each frame's "previous view" being the view of the frame before it"""
        from zetaray_amd import scene_io
        out, prev = [], None
        for f in range(1, self.frames + 1):
            cb = scene_io.make_frame_constants(self.w, self.h, frame_num=f, num_emissives=len(scene.emissives), **self.cb_kw(f))
            if prev is not None:
                cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
            prev = cb.copy()
            out.append(cb)
        return out


_MOVING = lambda f: dict(cam_pos=(0.05 * max(0, f - 2), 1.2, -4.043))      # noqa: E731  (moves from frame 3 on)
_ACC_STATIC = lambda f: dict(accumulate=1, camera_static=1, num_frames_static=f)      # noqa: E731
# the camera moves in frames 1 - 2 and stops: frames >= 3 accumulate (tools/ref_pass_cases.py _ACC: the first static frame counts as frame 1 of the accumulation)
_ACC_STARTS = lambda f: dict(accumulate=1, camera_static=1 if f >= 3 else 0, num_frames_static=max(0, f - 2), cam_pos=(0.05 * (min(f, 2) - 1), 1.2, -4.043))      # noqa: E731
CASES = {
    "moving": Case("moving", _MOVING, reset_at=4),
    "two_rounds": Case("two_rounds", _MOVING, reset_at=4, num_spatial_passes=2),
    "acc_no_temporal": Case("acc_no_temporal", _ACC_STATIC, temporal=False),
    "acc_reset": Case("acc_reset", _ACC_STATIC, reset_at=4),
    "acc_starts": Case("acc_starts", _ACC_STARTS),
}


def oracle_sequence(case, scene, oscene):
    """the CPU oracle's frames of a case: per frame FINAL, the reservoir planes, the pixels K11 skips (no surface, or an emissive one: GBuffer flags in the
    low byte of the metallic-roughness plane, zr_wire.h ZR_GBUF_EMISSIVE | ZR_GBUF_INVALID) and whether the frame ran temporal reuse; and the counters' sum"""
    from oracle import zro
    o = zro.OracleRPT(oscene, case.w, case.h)
    prm = case.params()
    frames, nc, ns = [], 0, 0
    for f, cb in enumerate(case.frame_constants(scene), 1):
        if case.reset_at == f:
            o.reset_temporal()
            o.final[...] = 0      # (zr_pass_reset_temporal clears FINAL too -- the accumulation starts over -- and waits for the device: a host call between frames)
        gb = oscene.gbuffer(cb)
        fin = o.render(cb, prm, gb=gb).copy()
        planes = {nm: o.plane(nm) for nm in RES_PLANES}
        nc, ns = nc + o.counters[0], ns + o.counters[1]
        skip = (np.asarray(gb[0][2]).reshape(case.h, case.w).astype(np.uint32) & 0x6) != 0
        do_temporal = bool(case.temporal and f >= 2 and f != case.reset_at)
        frames.append({"final": fin, "planes": planes, "skip": skip, "do_temporal": do_temporal, "wrote": do_temporal or f == 1 or f == case.reset_at})
    return frames, (nc, ns)


# ------------------------------------------------------------------------------------------------ the driver
_HIP = {}


def _hip():
    """the HIP runtime this process already has loaded (torch's), for hipMemcpyAsync on a stream of ours (tools/dbg_stream.py)"""
    if "lib" not in _HIP:
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
        lib = C.CDLL(path)
        lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        lib.hipMemcpyAsync.restype = C.c_int
        _HIP["lib"] = lib
    return _HIP["lib"]


class Run:
    """what one driven sequence leaves: frames[f] = {"final", "A".."G", "target", "denoised"} (numpy), the ray counters, and -- per frame -- the device time
    (ms from the start of the sequence) at which its first half completed on stream A and at which the held part began on stream B (None without a stall)"""


def drive(api, case, scene, mode, schedule="none", stall_ms=0.0):
    """Render `case` stage by stage.  mode: None = everything on one stream, frame overlap off (the plain order); "product" / "carry" = frame overlap on, the
    first half of every frame on the pass's stream A and the reuse stages, the snapshots and the denoise pass on a stream B.  No host wait between the first
    enqueue of frame 1 and the device synchronize at the end."""
    import torch
    assert schedule in SCHEDULES and (mode in ("product", "carry") or (mode is None and schedule == "none"))
    w, h, n = case.w, case.h, case.frames
    prm = case.params()
    cbs = case.frame_constants(scene)
    r = api.Renderer(scene, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    dn = r.enable_denoise()
    sb = torch.cuda.Stream()
    b = sb.cuda_stream
    if mode is not None:
        r.enable_frame_overlap(True, carry=(mode == "carry"))
        sa = torch.cuda.ExternalStream(r.p_indirect.frame_overlap_stream())
    else:
        sa = sb
    a = sa.cuda_stream
    # the alias table is built once, before the sequence (PRELIGHTING has nothing else to do without presampled sets)
    r.p_prelight.render(cbs[0], r.scene, None, b)
    r._alias_ready = True
    r.p_indirect.read_counters(reset=True)
    names = ("final",) + RES_PLANES + ("target", "denoised")
    snaps = [{nm: torch.zeros(w * h * PLANE_BYTES[nm], dtype=torch.uint8, device="cuda") for nm in names} for _ in range(n)]
    ev_base = torch.cuda.Event(enable_timing=True)
    ev_a = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    ev_held = [torch.cuda.Event(enable_timing=True) if (schedule != "none" and f >= 1) else None for f in range(n)]
    hip = _hip()
    import time
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    ev_base.record(sb)

    def snap(dst, which, pass_, nbytes):
        ptr, pw, ph, bpp = pass_.output_ptr(which)
        assert (pw, ph) == (w, h) and pw * ph * bpp == nbytes, (which, pw, ph, bpp, nbytes)
        rc = hip.hipMemcpyAsync(dst.data_ptr(), ptr, nbytes, 3, b)      # hipMemcpyDeviceToDevice, in stream B's order
        assert rc == 0, f"hipMemcpyAsync failed: {rc}"

    def hold(f, where):
        if schedule == where and f >= 1:
            stall(sa if where == "candidates_held" else sb, stall_ms)
            ev_held[f].record(sa if where == "candidates_held" else sb)

    for f, cb in enumerate(cbs):
        if case.reset_at == f + 1:
            r.p_indirect.reset_temporal()
        hold(f, "candidates_held")
        r.p_gbuffer.render(cb, r.scene, r.gbuffer, a)
        r.p_indirect.render_stage(cb, r.scene, r.gbuffer, api.STAGE_CANDIDATES, a)
        ev_a[f].record(sa)
        hold(f, "reuse_held")
        r.p_indirect.render_stage(cb, r.scene, r.gbuffer, api.STAGE_TEMPORAL_REUSE, b)
        hold(f, "spatial_held")
        r.p_indirect.render_stage(cb, r.scene, r.gbuffer, api.STAGE_SPATIAL, b)
        r.p_indirect.render_stage(cb, r.scene, r.gbuffer, api.STAGE_SPATIAL2, b)
        hold(f, "consumer_held")
        snap(snaps[f]["final"], api.OUT_FINAL, r.p_indirect, w * h * 16)
        for nm in RES_PLANES + ("target",):
            snap(snaps[f][nm], api.RPT_OUTPUTS[nm][0], r.p_indirect, w * h * PLANE_BYTES[nm])
        dn.set_input(api.IN_DENOISE_SIGNAL, r.p_indirect.output_ptr()[0])
        dn.render(cb, r.scene, r.gbuffer, b)
        snap(snaps[f]["denoised"], api.OUT_DENOISED, dn, w * h * 16)
    torch.cuda.synchronize()

    out = Run()
    out.wall_ms = (time.perf_counter() - t_start) * 1e3      # host submission + device, first enqueue to the end of the last copy
    out.frames = []
    for f in range(n):
        d = {}
        for nm in names:
            raw = snaps[f][nm].cpu().numpy()
            if nm in ("final", "target", "denoised"):
                d[nm] = raw.view(np.float32).reshape(h, w, 4)
            else:
                _, dt, ch = api.RPT_OUTPUTS[nm]
                d[nm] = raw.view(dt).reshape(h, w, ch)
        out.frames.append(d)
    out.counters = r.p_indirect.read_counters()
    out.t_first_half = [ev_base.elapsed_time(e) for e in ev_a]
    out.t_held = [ev_base.elapsed_time(e) if e is not None else None for e in ev_held]
    # frame f + 1's first half completed before the held part of frame f began (f counted from 0: frames 2 .. n - 1 of the sequence)
    out.ran_ahead = {f + 1: (out.t_first_half[f + 1] < out.t_held[f]) for f in range(1, n - 1) if out.t_held[f] is not None}
    del dn, r
    return out


def plain_frames_wall_ms(api, case, scene, frames=2):
    """host submission + device time of `frames` plain-order frames of the case (one stream, overlap off), after one such run to warm everything up"""
    short = Case(case.name, case.cb_kw, case.reset_at, case.nsp, case.temporal, case.w, case.h, frames)
    drive(api, short, scene, None)
    return drive(api, short, scene, None).wall_ms
