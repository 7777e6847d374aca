"""Cost of creating a scene whose material textures arrive as level 0 alone (what a PNG image decodes to), at two texture counts (--textures A B, default
16 128; each --size^2, default 2048, with a full mip chain in the heap; three quarters RGBA8_SRGB, one quarter RG8; random texels).  The scene is one quad
(the first instance of the Cornell fixture), so texture work is all there is.
  (A) the way to the same heap before ZR_TEX_SRC_RAW_MIP0: zr_scene_create_compressed with full RAW chains.  Generating those chains on the host
      (zrh_mip_generate, include/zr_mipgen.h) is NOT in (A)'s time; it is timed on its own, --host-reps times (default 1), and reported
  (B) zr_scene_create_compressed with RAW_MIP0 sources: three quarters of (A)'s bytes cross the bus, the level launches of zr_tu_mipgen.hip make the rest
Median and p10 / p90 of --reps creations after --warmup (default 16 after 4), host wall time.  Also: the stream time of the level launches alone
(zr_mipgen_device between two events) and the bytes they read + write per second as a fraction of the copy probe's rate (which counts read + written
bytes too).  Prints one JSON line with the device probes.  Exit status 1 unless, at both counts, (B)'s median is not above (A)'s median plus (A)'s
p10 - p90 spread and the two heaps are equal.  GPU only; scripts/gpu.sh mipgen runs it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                        # noqa: E402
from zetaray_amd import api, scene_io, wire        # noqa: E402


def _stats(x):
    x = np.asarray(x, np.float64)
    return {"median": round(float(np.median(x)), 3), "p10": round(float(np.percentile(x, 10)), 3), "p90": round(float(np.percentile(x, 90)), 3)}


def _quad():
    sc = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))
    for f in ("instances", "instance_to_world", "instance_mask", "instance_num_tris"):
        setattr(sc, f, getattr(sc, f)[:1].copy())
    return sc


def _time_creations(sc, reps, warmup):
    t, heap = [], None
    for k in range(warmup + reps):
        a = time.perf_counter()
        s = api.Scene(sc)
        b = time.perf_counter()
        if k >= warmup:
            t.append((b - a) * 1e3)
        if k == 0:
            heap = s.get_texels()
        s.close()
    return t, heap


def run(counts, size, reps, warmup, host_reps):
    import torch
    out = {"mode": "mipgen", "texture_size": size, "reps": reps, "warmup": warmup, "host_reps": host_reps,
           "library": os.path.basename(api.LIB_PATH), "device_state": bench.device_state(api, 0), "sizes": []}
    copy_rate = out["device_state"].get("probe_copy_GBs")
    rng = np.random.default_rng(2048)
    ok = True

    def note(*a):      # (progress on stderr: the one JSON line is all stdout gets)
        print(*a, file=sys.stderr, flush=True)
    mips = int(np.log2(size)) + 1
    sides = [max(1, size >> m) for m in range(mips)]
    pool = rng.integers(0, 256, size * size * 4 + 16 * 256, dtype=np.uint8)      # one pool read at a rolling shift: 128 textures do not cost 128 draws
    for n in counts:
        note("textures", n)
        fmts = [wire.TEX_RG8 if i % 4 == 3 else wire.TEX_RGBA8_SRGB for i in range(n)]
        bpp = [2 if f == wire.TEX_RG8 else 4 for f in fmts]
        chain = [b * sum(s * s for s in sides) for b in bpp]
        slot = [(c + 3) // 4 * 4 for c in chain]      # (an RG8 chain is 2 mod 4 bytes long: its 1 x 1 level; heap offsets are multiples of 4)
        descs = np.zeros(n, wire.TEXTURE_DESC)
        descs["offset"] = np.concatenate([[0], np.cumsum(slot)[:-1]])
        descs["width"], descs["height"], descs["num_mips"], descs["format"] = size, size, mips, fmts
        heap_bytes = int(sum(slot))
        # ---- the full chains on the host (what (A) uploads), timed apart
        heap = np.zeros(heap_bytes, np.uint8)
        for i in range(n):
            o, n0 = int(descs["offset"][i]), size * size * bpp[i]
            heap[o:o + n0] = pool[16 * (i % 256):16 * (i % 256) + n0]
        level0 = heap.copy()
        t_host = []
        for k in range(host_reps):
            heap[:] = level0
            a = time.perf_counter()
            scene_io.mip_generate(descs, heap)
            t_host.append((time.perf_counter() - a) * 1e3)
            note("host generation", k, round(t_host[-1] / 1e3, 2), "s")
        res = {"textures": n, "heap_MB": round(heap_bytes / 1e6, 1), "host_generation_ms": _stats(t_host)}
        # ---- (A) full RAW chains
        sa = _quad()
        sa.textures, sa.texel_heap_bytes, sa.texture_payload = descs.copy(), heap_bytes, heap
        sa.texture_sources = np.zeros(n, wire.TEXTURE_SOURCE)
        sa.texture_sources["offset"], sa.texture_sources["encoding"] = descs["offset"], wire.TEX_SRC_RAW
        t_a, heap_a = _time_creations(sa, reps, warmup)
        note("A done")
        res["A_payload_MB"] = round(len(sa.texture_payload) / 1e6, 1)
        res["A_wall_ms"] = _stats(t_a)
        res["A_heap_is_the_host_heap"] = bool(np.array_equal(heap_a, heap))
        # ---- (B) level 0 alone
        sb = _quad()
        sb.textures, sb.texel_heap_bytes = descs.copy(), heap_bytes
        n0 = [size * size * b for b in bpp]
        sb.texture_sources = np.zeros(n, wire.TEXTURE_SOURCE)
        sb.texture_sources["offset"], sb.texture_sources["encoding"] = np.concatenate([[0], np.cumsum(n0)[:-1]]), wire.TEX_SRC_RAW_MIP0
        sb.texture_payload = np.concatenate([level0[int(o):int(o) + k] for o, k in zip(descs["offset"], n0)])
        t_b, heap_b = _time_creations(sb, reps, warmup)
        note("B done")
        res["B_payload_MB"] = round(len(sb.texture_payload) / 1e6, 1)
        res["B_wall_ms"] = _stats(t_b)
        res["heaps_equal"] = bool(np.array_equal(heap_a, heap_b))
        del heap_a, heap_b
        res["B_limit_ms"] = round(res["A_wall_ms"]["median"] + (res["A_wall_ms"]["p90"] - res["A_wall_ms"]["p10"]), 3)
        res["B_within_limit"] = bool(res["B_wall_ms"]["median"] <= res["B_limit_ms"])
        # ---- the level launches alone
        d_texels = torch.from_numpy(level0).cuda()
        st = torch.cuda.Stream()
        ms = []
        for k in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            api._check(api.lib().zr_mipgen_device(0, st.cuda_stream, descs.ctypes.data, n, d_texels.data_ptr(), heap_bytes))
            e1.record(st)
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
        res["launches"] = mips - 1
        res["levels_equal_the_host"] = bool(np.array_equal(d_texels.cpu().numpy(), heap))
        res["levels_stream_ms"] = _stats(ms)
        moved = sum(b * sum(sides[m - 1] ** 2 + sides[m] ** 2 for m in range(1, mips)) for b in bpp)      # every level read once and written once
        res["levels_read_plus_written_GBs"] = round(moved / 1e9 / (res["levels_stream_ms"]["median"] * 1e-3), 1)
        res["probe_copy_GBs_read_plus_written"] = copy_rate
        res["levels_fraction_of_copy_rate"] = round(res["levels_read_plus_written_GBs"] / copy_rate, 3) if copy_rate else None
        del d_texels, level0, heap, sa, sb
        ok = ok and res["heaps_equal"] and res["A_heap_is_the_host_heap"] and res["levels_equal_the_host"] and res["B_within_limit"]
        out["sizes"].append(res)
    out["B_within_limit_at_both_sizes"] = bool(ok)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--textures", type=int, nargs=2, default=[16, 128])
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    sys.exit(run(a.textures, a.size, a.reps, a.warmup, a.host_reps))
