"""Cost of creating a scene whose material textures arrive block-compressed, at two texture counts (--textures A B, default 16 128; each --size^2, default
2048, with its full mip chain; three quarters BC7, one quarter BC5; random blocks).  The scene is one quad (the first instance of the Cornell fixture),
so texture work is all there is.
  (A) the path before zr_scene_create_compressed: the loader's decode of every mip on the host (zrh_bc7_decode / zrh_bc5_decode, what LoadDDS runs) into
      the texel heap, then zr_scene_create with the texels.  The decode takes seconds per creation and does not depend on the device; it is timed on
      its own, --host-reps times after --host-warmup (default: as --reps / --warmup), and its median added to the creation's
  (B) zr_scene_create_compressed with the blocks
Median and p10 / p90 of --reps creations after --warmup (default 16 after 4), host wall time.  Also: the stream time of the decode launch alone
(zr_bcn_decode_device between two events) and the bytes it writes per second next to the copy probe's rate (which counts read + written bytes).
Prints one JSON line with the device probes.  Exit status 1 unless (B)'s wall time is below (A)'s at both counts and the two heaps are equal.
GPU only; scripts/gpu.sh texdecode runs it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                        # noqa: E402
from zetaray_amd import api, scene_io, wire        # noqa: E402

BC7, BC5 = wire.TEX_SRC_BC7, wire.TEX_SRC_BC5


def _stats(x):
    x = np.asarray(x, np.float64)
    return {"median": round(float(np.median(x)), 3), "p10": round(float(np.percentile(x, 10)), 3), "p90": round(float(np.percentile(x, 90)), 3)}


def _quad():
    sc = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))
    for f in ("instances", "instance_to_world", "instance_mask", "instance_num_tris"):
        setattr(sc, f, getattr(sc, f)[:1].copy())
    return sc


def _mips(size):
    return [max(1, size >> m) for m in range(int(np.log2(size)) + 1)]


def run(counts, size, reps, warmup, host_reps, host_warmup):
    import torch
    out = {"mode": "texture_decode", "texture_size": size, "reps": reps, "warmup": warmup, "host_reps": host_reps, "host_warmup": host_warmup,
           "library": os.path.basename(api.LIB_PATH), "device_state": bench.device_state(api, 0), "sizes": []}
    copy_rate = out["device_state"].get("probe_copy_GBs")
    rng = np.random.default_rng(2048)
    ok = True
    def note(*a):      # (progress on stderr: the one JSON line is all stdout gets)
        print(*a, file=sys.stderr, flush=True)
    for n in counts:
        note("textures", n)
        sc = _quad()
        mips = _mips(size)
        nblk = sum(((m + 3) // 4) ** 2 for m in mips)
        # random blocks, one pool repeated with a rolling shift so that 128 textures do not cost 128 draws (the decode does not care)
        pool = rng.integers(0, 256, 16 * nblk + 4096, dtype=np.uint8)
        for i in range(n):
            enc = BC5 if i % 4 == 3 else BC7
            chain = pool[16 * (i % 256):16 * (i % 256) + 16 * nblk]
            sc.add_texture_blocks(chain, size, size, len(mips), wire.TEX_RG8 if enc == BC5 else wire.TEX_RGBA8_SRGB, enc)
        res = {"textures": n, "payload_MB": round(len(sc.texture_payload) / 1e6, 1), "heap_MB": round(sc.texel_heap_bytes / 1e6, 1), "blocks": n * nblk}
        # ---- (A) host decode + zr_scene_create
        dec = _quad()
        dec.textures = sc.textures.copy()
        t_dec = []
        for k in range(host_warmup + host_reps):
            a = time.perf_counter()
            sc.decode_textures()
            b = time.perf_counter()
            if k >= host_warmup:
                t_dec.append((b - a) * 1e3)
            note("host decode", k, round(b - a, 3), "s")
        dec.texels = sc.texels
        sc.texels = np.zeros(0, np.uint8)
        t_create = []
        for k in range(warmup + reps):
            a = time.perf_counter()
            s = api.Scene(dec)
            b = time.perf_counter()
            if k >= warmup:
                t_create.append((b - a) * 1e3)
            if k == 0:
                heap_a = s.get_texels()
            s.close()
        note("A done")
        res["A_host_decode_ms"] = _stats(t_dec)
        res["A_scene_create_ms"] = _stats(t_create)
        res["A_wall_ms"] = round(res["A_host_decode_ms"]["median"] + res["A_scene_create_ms"]["median"], 3)
        # ---- (B) zr_scene_create_compressed
        t_b = []
        for k in range(warmup + reps):
            a = time.perf_counter()
            s = api.Scene(sc)
            b = time.perf_counter()
            if k >= warmup:
                t_b.append((b - a) * 1e3)
            if k == 0:
                res["heaps_equal"] = bool(np.array_equal(s.get_texels(), heap_a))
            s.close()
        del heap_a
        note("B done")
        res["B_wall_ms"] = _stats(t_b)
        res["wall_ratio_A_over_B"] = round(res["A_wall_ms"] / res["B_wall_ms"]["median"], 2)
        # ---- the decode launch alone
        d_payload = torch.from_numpy(sc.texture_payload).cuda()
        d_texels = torch.zeros(sc.texel_heap_bytes, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        ms = []
        for k in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            api._check(api.lib().zr_bcn_decode_device(0, st.cuda_stream, sc.textures.ctypes.data, sc.texture_sources.ctypes.data, len(sc.textures), d_payload.data_ptr(),
                                                      len(sc.texture_payload), d_texels.data_ptr(), sc.texel_heap_bytes))
            e1.record(st)
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
        res["decode_stream_ms"] = _stats(ms)
        written = sum((2 if i % 4 == 3 else 4) * sum(m * m for m in mips) for i in range(n))
        res["decode_written_GBs"] = round(written / 1e9 / (res["decode_stream_ms"]["median"] * 1e-3), 1)
        res["decode_read_plus_written_GBs"] = round((written + len(sc.texture_payload)) / 1e9 / (res["decode_stream_ms"]["median"] * 1e-3), 1)
        res["probe_copy_GBs_read_plus_written"] = copy_rate
        del d_payload, d_texels
        ok = ok and res["heaps_equal"] and res["B_wall_ms"]["median"] < res["A_wall_ms"]
        out["sizes"].append(res)
    out["B_below_A_at_both_sizes"] = bool(ok)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--textures", type=int, nargs=2, default=[16, 128])
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=None)
    ap.add_argument("--host-warmup", type=int, default=None)
    a = ap.parse_args()
    sys.exit(run(a.textures, a.size, a.reps, a.warmup, a.reps if a.host_reps is None else a.host_reps, a.warmup if a.host_warmup is None else a.host_warmup))
