#!/usr/bin/env python
"""bench.py -- one "step" = one frame of the hot path (G-buffer + indirect-lighting pass) on synthetic/fixture input.

  python bench.py --gpus N --steps K --warmup W          (N > 1: launched by torch.distributed.run, one rank per GPU)
  python bench.py ... --dump-outputs DIR                 (+ the last timed frame's output images as DIR/<name>.npy)
  python bench.py ... --full                             (+ everything the headline figure does not need: see below)

Metric (BASELINE.json): Mrays/s (+ ms/frame) at 1920x1080, 3 non-transmissive bounces, Cornell-Box-class scene.
A ray = one BVH query (closest-hit or any-hit), counted on the device.  Scene, BVH, G-buffer
and all queues are resident in HBM before the timed region; the timed region is K frames bracketed by barrier +
torch.cuda.synchronize(), max over ranks.  N > 1 shards the frame by 32-px-aligned screen tiles (scene replicated);
the path-tracing integrator has no cross-pixel reads, so there is no data-path collective ("scaling": weak would be
wrong here -- the total work is fixed, so this reports "strong").

A plain run sets up, settles and warms up, times the K frames, writes --dump-outputs and prints the line; nothing else.
--full adds what takes runs or processes of its own, each after the timed region except "device_state" (the device
probes, before it): "general_kernels" and "frame_overlap_off" (the same frames on the general kernels / in the plain
order), "roofline" for the dominant kernel (hipEvent timing inside the library, algorithmic bytes from the per-ray model
of DESIGN.md section 6) with config.frame_ms_median / p95, "cpu_baseline" (the CPU oracle's single-thread traversal of
its own BVH2 over a bounded sample of the same frame's rays), "extra_workloads" (BASELINE configs 4 and 5) and
"tolerance_mode" (the fast-arithmetic build) on the default line, and for N > 1 "multi_gpu" and the whole-job roofline.
The --no-* switches below drop single items of --full.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# per-ray algorithmic bytes; split by the kernel that touches them
BYTES_CLOSEST = 296          # 64 ray w+r, 40 hit w+r, 192 vertex/index/instance/material gathers
BYTES_SHADOW = 72            # 64 ray w+r, 8 result w+r
TRACE_CLOSEST = 32 + 20      # trace kernel: ray record read + hit record written
TRACE_SHADOW = 32 + 4
SHADE_CLOSEST = BYTES_CLOSEST - TRACE_CLOSEST
SHADE_SHADOW = BYTES_SHADOW - TRACE_SHADOW
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8 TB/s
# ReSTIR PT: algorithmic per-pixel bytes of each pass besides its rays: G-buffer planes read
# (38 B: base colour 4, normal 4, mr 2, depth 4, ior 1, coat 8 (rare), tri diffs 0 -- not carried, motion 4, ...) and
# reservoir (62 B per set), r-buffer (42 B), target (16 B), final (16 B) planes read / written
RPT_PIXEL_BYTES = {
    "rpt_pathtrace": 23 + 62 + 16,                       # G-buffer in, reservoir + target (or final) out
    "rpt_reconnect_temporal": 2 * 27 + 4 + 2 * 62 + 16 + 2 * 42 + 62 + 16,   # CtT + TtC fused
    "rpt_reconnect_spatial": 2 + 2 * 27 + 3 * 62 + 16 + 2 * 42 + 62 + 16,   # CtS + StC fused
    "rpt_spatial_search": 4 * 14 + 2 + 8,
    "rpt_classify_temporal": 2 + 4 + 8,
    # replay passes (both directions in one launch): per listed pixel the reservoir (62) + G-buffer planes (27) in, one r-buffer (42) out --
    # an upper bound per pixel of the frame, the lists hold a subset; sort: plane A's k / flags (4) in, two u16 maps out
    "rpt_replay_temporal": 2 * (62 + 27 + 42),
    "rpt_replay_spatial": 2 * (62 + 27 + 42),
    "rpt_sort_temporal": 2 * 4 + 2 * 2,
    "rpt_sort_spatial": 2 * 4 + 2 * 2,
}


# the denoise pass (zr_svgf.h, definition 3), algorithmic bytes per pixel and launch: temporal = signal 16 + depth / normal / motion 12 + previous depth / normal 8 +
# history colour 16 + moments 8 in, accumulated 16 + moments 8 + guide normal 8 + depth slope 4 out; variance = accumulated 16 + moments 8 + guide normal 8 in, stage texel 16 out;
# one a-trous iteration = stage texel 16 + depth 4 in, 16 out (the 24 neighbour taps are re-reads of what other pixels load once: cache hits in the model)
DENOISE_PIXEL_BYTES = {"denoise_temporal": 60 + 36, "denoise_variance": 32 + 16, "denoise_atrous": 20 + 16}


from zetaray_amd.tiling import tile_grid, tile_rect  # noqa: E402  (shared with the tests and the tiled renderer)

_CORNELL_SKY = os.path.join(ROOT, "tests", "golden", "cornell.npz")
# --config presets: BASELINE.json "configs"  -> the flags below
CONFIGS = {
    "2a": ("config 2, emissive half: Cornell (emissive) 1080p, ReSTIR DI only (K5/K6)", dict(direct=True, di_only=True, integrator="pt")),
    "2b": ("config 2, sun + sky half: the reference's default Cornell box 1080p, SkyDI only (K7/K8)", dict(scene=_CORNELL_SKY, sky_direct=True, di_only=True, integrator="pt")),
    "3": ("config 3: Cornell (emissive) 1080p ReSTIR GI, 3 bounces, temporal reuse", dict(integrator="restir_gi")),
    "4": ("config 4 on one GPU: 380k-triangle / 100k-light atrium 1080p ReSTIR PT", dict(scene="synthetic", steps=32, warmup=8)),
    "4k": ("config 5 without the denoise pass: the atrium at 3840x2160 ReSTIR PT", dict(scene="synthetic", width=3840, height=2160, steps=16, warmup=4)),
    "5": ("config 5: the atrium at 3840x2160, ReSTIR PT + the denoise pass (spatiotemporal variance-guided filter, 5 a-trous iterations; tile-split with the integrator for N > 1)",
          dict(scene="synthetic", width=3840, height=2160, steps=16, warmup=4, denoise=True)),
    "pt": ("K9 unidirectional path tracer on the Cornell box (config 1's integrator at 1080p)", dict(integrator="pt")),
}


def source_hash():
    """identifies the kernel sources a profile was taken with: sha1 over zetaray_amd/csrc + include (profiles/*.json carry it; a
    roofline.traffic / valu block is only reported from a profile whose hash matches the sources of the library being benchmarked)"""
    import glob
    import hashlib
    h = hashlib.sha1()
    for f in sorted(glob.glob(os.path.join(ROOT, "zetaray_amd", "csrc", "*.h*")) + glob.glob(os.path.join(ROOT, "include", "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


_SMI_SNIPPET = r"""
import json, sys
out = {}
try:
    import amdsmi as A
    A.amdsmi_init()
    hs = A.amdsmi_get_processor_handles()
    h = hs[min(int(sys.argv[1]), len(hs) - 1)]
    def grab(name, fn):
        try:
            v = fn()
            out[name] = v if isinstance(v, (int, float, str, list, dict, type(None))) else str(v)
        except Exception as e:
            out[name] = "n/a: " + type(e).__name__
    grab("sclk", lambda: A.amdsmi_get_clock_info(h, A.AmdSmiClkType.SYS))
    grab("mclk", lambda: A.amdsmi_get_clock_info(h, A.AmdSmiClkType.MEM))
    grab("fclk", lambda: A.amdsmi_get_clock_info(h, A.AmdSmiClkType.DF))
    grab("socclk", lambda: A.amdsmi_get_clock_info(h, A.AmdSmiClkType.SOC))
    grab("power_cap", lambda: A.amdsmi_get_power_cap_info(h))
    grab("power", lambda: A.amdsmi_get_power_info(h))
    grab("perf_level", lambda: A.amdsmi_get_gpu_perf_level(h))
    grab("memory_partition", lambda: A.amdsmi_get_gpu_memory_partition(h))
    grab("compute_partition", lambda: A.amdsmi_get_gpu_compute_partition(h))
    grab("activity", lambda: A.amdsmi_get_gpu_activity(h))
    A.amdsmi_shut_down()
except Exception as e:
    out["error"] = repr(e)[:200]
print(json.dumps(out, default=str))
"""


def device_state(api, device, min_ms=60.0):
    """What the device of this process delivers right now: static properties + the copy / FMA / shader-clock probes of zr_device_probe_run (measured here,
    before the timed region) + what amdsmi reports about clocks, power cap and partition modes (a child process with a timeout: the bench line must
    not depend on the management library being usable by an ordinary user).  VERDICT r5: the same command ran 18 % apart on two boxes of the pool."""
    import ctypes as C
    import subprocess

    class Probe(C.Structure):
        _fields_ = [("name", C.c_char * 64), ("arch", C.c_char * 32), ("compute_units", C.c_uint32), ("clock_khz_max", C.c_uint32),
                    ("mem_clock_khz_max", C.c_uint32), ("mem_bus_bits", C.c_uint32), ("l2_bytes", C.c_uint32), ("wall_clock_khz", C.c_uint32),
                    ("hbm_bytes", C.c_uint64), ("copy_GBs", C.c_float), ("copy_ms", C.c_float), ("fma_tflops", C.c_float), ("fma_ms", C.c_float),
                    ("sclk_mhz_under_load", C.c_float)]
    L = api.lib()
    pr = Probe()
    L.zr_device_probe_run.argtypes = [C.c_int, C.c_float, C.c_void_p]
    rc = L.zr_device_probe_run(int(device), float(min_ms), C.byref(pr))
    if rc != 0:
        return {"error": L.zr_last_error().decode(errors="replace")}
    st = {"name": pr.name.decode(errors="replace"), "arch": pr.arch.decode(errors="replace"), "compute_units": pr.compute_units,
          "clock_mhz_max": pr.clock_khz_max / 1e3, "mem_clock_mhz_max": pr.mem_clock_khz_max / 1e3, "mem_bus_bits": pr.mem_bus_bits,
          "l2_MiB": round(pr.l2_bytes / 2**20, 2), "hbm_GiB": round(pr.hbm_bytes / 2**30, 1),
          "probe_copy_GBs": round(pr.copy_GBs, 1), "probe_copy_ms": round(pr.copy_ms, 1),
          "probe_fma_tflops": round(pr.fma_tflops, 2), "probe_fma_ms": round(pr.fma_ms, 1),
          "probe_sclk_mhz_under_load": round(pr.sclk_mhz_under_load, 1),
          "probe_note": "copy = device-to-device hipMemcpyAsync of 512 MiB, read + written bytes per second; fma = fp32 v_fma_f32 issue rate with 8 waves per SIMD on "
                        "every CU (2 flops per FMA); sclk = shader-clock counter over the 100 MHz wall clock inside the FMA kernel"}
    try:
        cp = subprocess.run([sys.executable, "-c", _SMI_SNIPPET, str(device)], capture_output=True, text=True, timeout=30)
        st["smi"] = json.loads(cp.stdout.strip().splitlines()[-1])
    except Exception as e:
        st["smi"] = {"error": repr(e)[:200]}
    return st


def cpu_baseline(scene_host, cb, max_rays=1_000_000, rpt_params=None, sample=(2, 8)):
    """Single-thread CPU traversal (oracle BVH2 + ABI intersection) over primary + diffuse-bounce rays of this frame."""
    from oracle import zro
    o = zro.OracleScene(scene_host, force_bvh=True)
    w, h = int(cb["render_width"]), int(cb["render_height"])
    rng = np.random.default_rng(0x5EED)
    n = max_rays // 2
    # primary rays (subsampled pixel grid)
    px = rng.integers(0, w, n)
    py = rng.integers(0, h, n)
    ndc_x = ((px + 0.5) / w) * 2 - 1
    ndc_y = -(((py + 0.5) / h) * 2 - 1)
    d = np.stack([ndc_x * float(cb["aspect_ratio"]) * float(cb["tan_half_fov"]), ndc_y * float(cb["tan_half_fov"]), np.ones(n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o3 = np.tile(np.asarray(cb["camera_pos"], np.float64), (n, 1))
    prim = np.concatenate([o3, np.zeros((n, 1)), d, np.full((n, 1), 3.0e38)], 1).astype(np.float32)
    hits = o.trace_closest(prim)
    ok = hits[:, 3] != 0xFFFFFFFF
    t = hits[ok, 0].view(np.float32)
    p = prim[ok, 0:3] + prim[ok, 4:7] * (t[:, None] * 0.999)
    d2 = rng.normal(size=p.shape)
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    sec = np.concatenate([p, np.full((len(p), 1), 1e-4), d2, np.full((len(p), 1), 3.0e38)], 1).astype(np.float32)
    rays = np.concatenate([prim, sec], 0)
    _, dt = o.trace_closest(rays, timed=True)
    trace_only = len(rays) / dt / 1e6
    if rpt_params is None:
        # repeat the ray set until ~10 s of CPU work have been timed
        reps, tot = 0, 0.0
        while tot < 10.0 and reps < 200:
            _, d1 = o.trace_closest(rays, timed=True)
            tot += d1
            reps += 1
        return {"value": round(reps * len(rays) / tot / 1e6, 4), "unit": "Mrays/s", "cores": 1, "kind": "port",
                "sample": f"{reps} x {len(rays)} closest-hit rays (random primary + diffuse bounce) of the same frame, oracle BVH2, "
                          f"{tot:.1f} s, host has {os.cpu_count()} logical cores"}
    # the whole workload on a bounded sample: the oracle's G-buffer + ReSTIR PT (same parameters) at reduced resolution for a few frames
    # (temporal + spatial reuse active from frame 2), one thread; rays = the oracle's own ray counters.  Cornell: half resolution x 8 frames
    # (~12 s); the atrium: quarter resolution x 4 frames (~25 s)
    import time
    div, nframes = sample
    sw, sh = max(64, w // div), max(36, h // div)
    orpt = zro.OracleRPT(o, sw, sh)
    rays_total, t0 = 0, time.perf_counter()
    for f in range(1, nframes + 1):
        cbs = cb.copy()
        cbs["render_width"], cbs["render_height"], cbs["frame_num"] = sw, sh, f
        if rpt_params.presampling:
            o.presample(f, int(rpt_params.num_sample_sets), int(rpt_params.sample_set_size))      # K3, the light sets this frame's NEE draws from
        orpt.render(cbs, rpt_params)
        rays_total += sum(orpt.counters)
    dt_rpt = time.perf_counter() - t0
    return {"value": round(rays_total / dt_rpt / 1e6, 4), "unit": "Mrays/s", "cores": 1, "kind": "port",
            "sample": f"oracle G-buffer + ReSTIR PT, {sw}x{sh} x {nframes} frames ({rays_total} rays, {dt_rpt:.1f} s, 1 thread of "
                      f"{os.cpu_count()} logical cores); BVH traversal alone: {trace_only:.2f} Mrays/s"}


def read_prof(api):
    """Section counters of a -DZR_PROF build of the library (zr_dev_scene.h ProfScope): wave cycles per kernel and section, and the
    vote statistics of the BVH traversal.  None for the product build, which has no such export."""
    import ctypes as C
    L = api.lib()
    if not hasattr(L, "zr_debug_prof_read"):
        return None
    buf = (C.c_ulonglong * 256)()
    L.zr_debug_prof_read.argtypes = [C.c_void_p]
    if L.zr_debug_prof_read(buf) != 0:
        return None
    names = ["kernel", "trav", "trav_calls", "rays", "node_iters", "node_lanes", "tri_iters", "tri_lanes", "material", "nee", "bsdf",
             "misc0", "misc1", "misc2", "misc3", "misc4", "steals", "steal_pairs"]
    kernels = {0: "other", 1: "rpt_pathtrace", 2: "rpt_temporal", 3: "rpt_stc"}
    res = {}
    for k, kn in kernels.items():
        v = {n: int(buf[32 * k + i]) for i, n in enumerate(names)}
        if not any(v.values()):
            continue
        d = dict(v)
        if v["kernel"]:
            for n in ("trav", "material", "nee", "bsdf", "misc0", "misc1", "misc2", "misc3", "misc4"):
                d[n + "_frac"] = round(v[n] / v["kernel"], 4)
        it = v["node_iters"] + v["tri_iters"]
        if it:
            d["trav_lane_util"] = round((v["node_lanes"] + v["tri_lanes"]) / (64.0 * it), 4)
            d["node_lane_util"] = round(v["node_lanes"] / (64.0 * max(1, v["node_iters"])), 4)
            d["tri_lane_util"] = round(v["tri_lanes"] / (64.0 * max(1, v["tri_iters"])), 4)
            d["nodes_per_ray"] = round(v["node_lanes"] / max(1, v["rays"]), 3)
            d["tris_per_ray"] = round(v["tri_lanes"] / max(1, v["rays"]), 3)
            d["iters_per_call"] = round(it / max(1, v["trav_calls"]), 2)
            d["rays_per_call"] = round(v["rays"] / max(1, v["trav_calls"]), 2)
            d["steals_per_call"] = round(v["steals"] / max(1, v["trav_calls"]), 3)
            d["pairs_per_steal"] = round(v["steal_pairs"] / max(1, v["steals"]), 2)
        res[kn] = d
    return res


DUMP_LIMIT_BYTES = 64_000_000
DUMP_SAMPLE_SEED = 0


def dump_outputs(args, ctx, r, p_denoise, ext, tile, frame_num):
    """--dump-outputs: the images the timed path handed its caller in its last frame -- the indirect integrator's FINAL radiance, the DI passes'
    outputs, the denoised image -- as DIR/<name>.npy (float32, H x W x 4 over the full frame; N > 1: every rank's owned tile, stitched on rank 0).
    When they would exceed DUMP_LIMIT_BYTES together, every array keeps the same fixed, seeded sample of pixels (rows of a (pixels, 4) array, pixel
    indices ascending, np.random.default_rng(DUMP_SAMPLE_SEED)).  Returns the description that goes on the JSON line (rank 0), None elsewhere."""
    planes = {}
    if not r.skip_indirect:
        planes["final"] = r.final()
    if r.p_direct is not None:
        planes["direct"] = r.p_direct.download()
    if r.p_sky_direct is not None:
        planes["sky_direct"] = r.p_sky_direct.download()
    if p_denoise is not None:
        planes["denoised"] = p_denoise.download_plane("denoised")
    x0, y0, tw, th = tile
    ox, oy = x0 - ext[0], y0 - ext[1]
    mine = (tile, {k: np.ascontiguousarray(v[oy:oy + th, ox:ox + tw], np.float32) for k, v in planes.items()})
    parts = [mine]
    if ctx["dist"] is not None:
        parts = [None] * ctx["world"] if ctx["rank"] == 0 else None
        ctx["dist"].gather_object(mine, parts, dst=0)
    if ctx["rank"] != 0:
        return None
    W, H = args.width, args.height
    full = {}
    for (x0, y0, tw, th), arrays in parts:
        for k, v in arrays.items():
            full.setdefault(k, np.zeros((H, W) + v.shape[2:], np.float32))[y0:y0 + th, x0:x0 + tw] = v
    n = W * H
    per_pixel = sum(v.nbytes // n for v in full.values())
    sample = None
    if n * per_pixel > DUMP_LIMIT_BYTES - 4096:      # (room for the .npy headers)
        k = (DUMP_LIMIT_BYTES - 4096) // per_pixel
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, k, replace=False))
        full = {name: v.reshape(n, -1)[idx] for name, v in full.items()}
        sample = {"pixels": int(k), "of": n, "seed": DUMP_SAMPLE_SEED}
    os.makedirs(args.dump_outputs, exist_ok=True)
    for name, v in full.items():
        np.save(os.path.join(args.dump_outputs, name + ".npy"), v)
    return {"dir": args.dump_outputs, "frame_num": frame_num, "arrays": {name: list(v.shape) for name, v in full.items()}, "pixel_sample": sample}


def measure(args, ctx):
    """One workload end to end on the devices of this job: scene + passes resident in HBM, settle + warm-up frames, the timed region of
    args.steps frames (barrier + torch.cuda.synchronize() on both sides, max over ranks), then -- with --full only -- the device probes (before the
    settle frames), the general-kernel and plain-order timings, the roofline block of the dominant kernel (hipEvent timing inside the library), the
    CPU baseline and the N > 1 blocks.  Returns the JSON line as a dict."""
    import torch
    from zetaray_amd import api, scene_io, wire
    world, rank, local_rank, dist, cdev = ctx["world"], ctx["rank"], ctx["local_rank"], ctx["dist"], ctx["cdev"]
    W, H = args.width, args.height
    cam = {}
    tex_offsets = None
    assert not args.textured or args.scene == "synthetic", "--textured needs --scene synthetic"
    if args.scene == "synthetic":
        sc = scene_io.make_synthetic_scene(num_tris=args.synthetic_tris, num_emissive=args.synthetic_emissives, layout=args.synthetic_layout)
        cam = dict(cam_pos=(0, 0, -3.5))
        scene_name = f"synthetic Sponza-class {args.synthetic_layout} ({sc.num_tris} triangles, {len(sc.emissives)} emissive, alias table + presampled sets 128x512)"
        if args.textured:
            tex_offsets = scene_io.add_test_textures(sc)
            scene_name += ", textured (base colour / normal / metallic-roughness / emissive maps, alpha-tested instance)"
    else:
        sc = scene_io.load_npz(args.scene)
        scene_name = f"Cornell Box ({os.path.basename(args.scene)[:-4]}: {sc.num_tris} triangles, {len(sc.emissives)} emissive" + (", sun + sky" if len(sc.emissives) == 0 else "") + ")"
    prm = wire.default_params()
    if args.scene == "synthetic":
        # the reference turns light presampling on above a light-count threshold (PreLighting.cpp:289-297)
        prm.presampling, prm.num_sample_sets, prm.sample_set_size = 1, 128, 512
    x0, y0, tw, th = tile_rect(W, H, world, rank)
    rpt = args.integrator == "restir_pt"
    tiled = None
    if rpt or args.integrator == "restir_gi":
        # ReSTIR PT / GI read neighbouring pixels' reservoirs: each rank owns a 32-px-aligned tile, renders the G-buffer of the
        # tile + a 32-px apron, and exchanges reservoir halos point-to-point over RCCL before the spatial stage and after
        # the frame (zetaray_amd/tiling.py); N = 1 degenerates to the plain renderer
        from zetaray_amd import tiling
        # N > 1: the halo exchange runs in C++ (libzetaray_host.so zr_halo.cpp: one pack kernel, grouped ncclSend / ncclRecv over RCCL on the
        # pass's stream, one unpack kernel); ZR_HALO_TRANSPORT=torch_p2p selects the per-plane copies + torch.distributed P2P path
        transport = os.environ.get("ZR_HALO_TRANSPORT", "rccl_cpp")
        tiled = tiling.TiledRestirPT(sc, W, H, world, rank, device=local_rank, params=prm, dist=dist, kind=args.integrator, transport=transport)
        r = tiled.r
        layout_kind = "equal-area grid"
        if world > 1 and rpt and os.environ.get("ZR_TILE_LAYOUT", "cost") == "cost":
            # cost-balanced split: a few frames on the equal-area grid with the per-cell ray counters on, every rank contributes the cells of
            # its own tile, and all ranks cut the frame by the same kd-split on the summed map (tiling.balanced_layout)
            r.p_indirect.enable_cost_map(True)
            for i in range(12):
                cbp = scene_io.make_frame_constants(W, H, frame_num=1 + i, num_emissives=len(sc.emissives), **cam)
                tiled.render_frame(cbp, exchange_final=not args.no_final_halo)
            torch.cuda.synchronize()
            cost = torch.tensor(tiled.owned_cost_cells(), dtype=torch.float64, device=cdev)
            dist.all_reduce(cost, op=dist.ReduceOp.SUM)
            layout = tiling.choose_layout(W, H, world, cost.cpu().numpy())
            r.p_indirect.enable_cost_map(False)
            # (--dump-outputs: fresh passes whichever layout the timing-dependent probe chose, so that its frames never make the history of the dumped frame)
            if layout is not None or args.dump_outputs:
                if tiled.native is not None:
                    tiled.native.close()
                del tiled, r
                tiled = tiling.TiledRestirPT(sc, W, H, world, rank, device=local_rank, params=prm, dist=dist, kind=args.integrator, transport=transport, layout=layout)
                r = tiled.r
            if layout is not None:
                layout_kind = "cost-balanced kd-split on the per-cell GPU time of 12 probe frames: " + str([list(t) for t in layout])
            else:
                layout_kind = "equal-area grid (the probe frames' cost map predicts < 15 % gain from re-balancing)"
        x0, y0, tw, th = tiled.tile
    elif args.di_only and world > 1:
        # BASELINE config 2 on N devices: the DI pass is the pass whose reservoirs cross tile borders (TEMPORAL stage -> exchange ZR_HALO_POST_TEMPORAL -> SPATIAL
        # stage, 24 / 13 B per pixel; tiling.TiledRestirPT kind "di" / "sky_di", tests/test_gpu_parity.py::test_tile_split_with_halo_exchange_other_passes_on_gpu)
        from zetaray_amd import tiling
        assert not rpt and (args.direct != args.sky_direct), "--di-only with N > 1 takes exactly one of --direct / --sky-direct"
        transport = os.environ.get("ZR_HALO_TRANSPORT", "rccl_cpp")
        if args.direct:
            dip = wire.default_params_di()
            dip.presampling, dip.num_sample_sets, dip.sample_set_size = prm.presampling, prm.num_sample_sets, prm.sample_set_size
        else:
            dip = wire.default_params_sky_di()
        tiled = tiling.TiledRestirPT(sc, W, H, world, rank, device=local_rank, params=prm, dist=dist, kind="di" if args.direct else "sky_di", pass_params=dip, transport=transport)
        r = tiled.r
        x0, y0, tw, th = tiled.tile
    else:
        r = api.Renderer(sc, tw, th, device=local_rank, params=prm, tile_origin=(x0, y0), integrator=api.INTEGRATOR_PATH_TRACING)

    if args.direct and r.p_direct is None:
        assert world == 1, "--direct next to an indirect integrator has no tile split (only --di-only shards the DI pass)"
        dip = wire.default_params_di()
        dip.presampling, dip.num_sample_sets, dip.sample_set_size = prm.presampling, prm.num_sample_sets, prm.sample_set_size
        r.enable_direct(dip, device=local_rank)

    if args.sky_direct and r.p_sky_direct is None:
        assert world == 1, "--sky-direct next to an indirect integrator has no tile split (only --di-only shards the DI pass)"
        r.enable_sky_direct(wire.default_params_sky_di(), device=local_rank)
    if args.di_only:
        assert not rpt and (args.direct or args.sky_direct), "--di-only needs --integrator pt and a DI pass"
        r.skip_indirect = True
    di_passes = [q for q in (r.p_direct, r.p_sky_direct) if q is not None]
    overlap = bool(args.frame_overlap) and rpt and not di_passes
    p_denoise = None
    if args.denoise:
        # N > 1: every rank filters its tile + apron and trades halos between the steps whose stencil would outrun the apron (tiling.denoise_schedule:
        # 3 exchanges per frame for the default 5 a-trous iterations); the stitched result equals one device's (tests/test_denoise_tiles_cpu.py, test_denoise.py)
        assert not args.di_only, "--denoise filters the indirect integrator's image"
        p_denoise = tiled.enable_denoise() if tiled is not None else r.enable_denoise()
    if overlap:
        # consecutive frames software-pipelined on two streams (zetaray_amd.h zr_pass_set_frame_overlap): K1 + K11 of frame N + 1 beside K15 / K12 / K13 / K16 of
        # frame N.  Bit-identical frames (test_frame_overlap_changes_nothing); ms_per_step is then a THROUGHPUT, the latency of one frame is frame_ms_median
        (tiled if tiled is not None else r).enable_frame_overlap(True)

    def frame_constants(i):
        cb = scene_io.make_frame_constants(W, H, frame_num=i, num_emissives=len(sc.emissives), **cam)
        if tex_offsets is not None:
            scene_io.set_texture_heap_offsets(cb, tex_offsets)
        return cb

    def frame(i):
        cb = frame_constants(i)
        if tiled is not None:
            tiled.render_frame(cb, exchange_final=not args.no_final_halo)      # (runs the denoise schedule too when the pass is enabled)
        else:
            r.render_frame(cb)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # steady state first: the ray count per frame grows until the temporal reservoirs sit at their M caps (7.98 M rays / frame after 5
    # frames against 8.74 M after 64 on the Cornell box), so a short --warmup must not change the reported rate
    settle = args.settle if args.settle is not None else (32 if (rpt or args.integrator == "restir_gi" or di_passes) else 0)
    settle_frames = settle
    # the device as it is right now, measured before anything is timed (every rank probes its own device; rank 0's block goes on the line as `device_state`,
    # N > 1 adds one summary row per rank; --full only)
    dev_state = device_state(api, local_rank) if (args.full and not args.no_device_state) else None
    barrier()
    t_s = time.perf_counter()
    for i in range(settle):
        frame(1 + i)
    barrier()
    t_settle = time.perf_counter() - t_s
    # clock ramp: real frames of this workload until >= args.ramp_s seconds of them have run back to back (a 44 ms timed region after 80 ms of
    # warm-up measures the governor as much as the code).  Every rank renders the same number of frames (the halo exchange is collective).
    ramp = 0
    if args.ramp_s > 0:
        per_frame = t_settle / settle if settle else None
        if per_frame is None:
            barrier(); t_s = time.perf_counter(); frame(1 + settle); barrier(); per_frame = time.perf_counter() - t_s
        ramp = int(min(4000, max(0, np.ceil(args.ramp_s / max(per_frame, 1e-5)))))
        if dist is not None:
            tr = torch.tensor([ramp], dtype=torch.int64, device=cdev)
            dist.all_reduce(tr, op=dist.ReduceOp.MAX)
            ramp = int(tr.item())
        if args.dump_outputs:
            # the ramp's length follows the clock: its frames go to a renderer of their own (same scene, tile and passes), so that the renderer
            # that is timed -- and dumped -- sees the same frames in every run with these arguments (N > 1: the rank's tile + apron, no halo exchanges)
            ex0, ey0, ew, eh = tiled.ext if tiled is not None else (x0, y0, tw, th)
            rr = api.Renderer(sc, ew, eh, device=local_rank, params=prm, tile_origin=(ex0, ey0),
                              integrator={"restir_pt": api.INTEGRATOR_RESTIR_PT, "restir_gi": api.INTEGRATOR_RESTIR_GI}.get(args.integrator, api.INTEGRATOR_PATH_TRACING))
            if r.p_direct is not None:
                dip = wire.default_params_di()
                dip.presampling, dip.num_sample_sets, dip.sample_set_size = prm.presampling, prm.num_sample_sets, prm.sample_set_size
                rr.enable_direct(dip, device=local_rank)
            if r.p_sky_direct is not None:
                rr.enable_sky_direct(wire.default_params_sky_di(), device=local_rank)
            rr.skip_indirect = r.skip_indirect
            if tiled is not None and world > 1:      # (the tile object's halo pass owns the tile inside its G-buffer apron)
                (rr.p_direct if tiled.kind == "di" else rr.p_sky_direct if tiled.kind == "sky_di" else rr.p_indirect).set_owned_rect(*tiled.tile)
            if p_denoise is not None:
                rr.enable_denoise(device=local_rank)
            if overlap:
                rr.enable_frame_overlap(True)
            for i in range(ramp):
                rr.render_frame(frame_constants(1 + settle + i))
            torch.cuda.synchronize()
            del rr
        else:
            for i in range(ramp):
                frame(1 + settle + i)
            settle += ramp
    for i in range(args.warmup):
        frame(1 + settle + i)
    barrier()
    r.p_gbuffer.read_counters(reset=True)
    r.p_indirect.read_counters(reset=True)
    for q in di_passes:
        q.read_counters(reset=True)
    barrier()
    exch0 = tiled.exchanges_done if tiled is not None else 0
    t0 = time.perf_counter()
    for i in range(args.steps):
        frame(1 + settle + args.warmup + i)
    barrier()
    dt = time.perf_counter() - t0
    exch_per_frame = ((tiled.exchanges_done - exch0) / args.steps) if tiled is not None else 0.0
    dumped = None
    if args.dump_outputs:      # (before anything else renders on these passes)
        dumped = dump_outputs(args, ctx, r, p_denoise, tiled.ext if tiled is not None else (x0, y0, tw, th), (x0, y0, tw, th),
                              settle + args.warmup + args.steps)

    c1 = r.p_gbuffer.read_counters(reset=True)
    c2 = r.p_indirect.read_counters(reset=True)
    c3 = [0, 0]
    for q in di_passes:
        cq = q.read_counters(reset=True)
        c3[0] += cq[0]
        c3[1] += cq[1]
    # primary rays: RenderGBuffer counts every pixel of the G-buffer it renders, which in tiled mode includes the 32-px apron around
    # the owned tile (rendered redundantly on every neighbour).  Only owned pixels are useful work: report those, and the
    # redundant apron rays separately.
    apron_rays = max(0, c1[0] - tw * th * args.steps) if (tiled is not None and world > 1) else 0
    rays = np.array([c1[0] - apron_rays + c2[0] + c3[0], c1[1] + c2[1] + c3[1]], np.float64)
    tmax = dt
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64, device=cdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        tmax = float(tt.item())
        rr = torch.tensor(rays, dtype=torch.float64, device=cdev)
        dist.all_reduce(rr, op=dist.ReduceOp.SUM)
        rays = rr.cpu().numpy()
        ar = torch.tensor([float(apron_rays)], dtype=torch.float64, device=cdev)
        dist.all_reduce(ar, op=dist.ReduceOp.SUM)
        apron_rays = float(ar.item())
    n_closest, n_shadow = float(rays[0]), float(rays[1])
    ms_per_step = tmax / args.steps * 1e3
    mrays = (n_closest + n_shadow) / tmax / 1e6

    out = {
        "metric": "Mrays/s", "value": round(mrays, 2), "unit": "Mrays/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": (f"{scene_name} {W}x{H}, sky-view LUT + G-buffer + ReSTIR DI only (K17 + K1 + "
                                f"{'K5/K6 emissive ' if args.direct else ''}{'K7/K8 sun + sky ' if args.sky_direct else ''}"
                                f"initial candidates, temporal + pairwise-MIS spatial reuse, static camera)") if args.di_only else
                               (f"{scene_name} {W}x{H}, G-buffer + ReSTIR PT "
                                f"(K1 + K11-K16: initial candidates, temporal + spatial reconnection reuse, boiling "
                                f"suppression; 3 non-transmissive / 4 glossy-transmissive bounces, static camera)"
                                + (" + denoise pass (temporal accumulation, variance estimate, 5 a-trous iterations)" if args.denoise else "")) if rpt else
                               (f"{scene_name} {W}x{H}, G-buffer + ReSTIR GI (K1+K10, "
                                f"3 bounces, temporal reuse, static camera)") if args.integrator == "restir_gi" else
                               (f"{scene_name} {W}x{H}, G-buffer + 1-spp "
                                f"path tracer (K1+K9, NEE+MIS, 3 non-transmissive bounces, static camera)"),
                   "integrator": ("" if args.di_only else args.integrator) + ("+restir_di" if args.direct else "") + ("+sky_di" if args.sky_direct else ""),
                   "parallelism": f"screen tiles {tile_grid(world)}" + (f" ({layout_kind})" if (tiled is not None and world > 1 and rpt) else "") + (
                       f", 32-px apron, RCCL p2p halo exchange of reservoir planes ({tiled.bpp} B/px): {tiled.halo_bytes} B sent per "
                       f"rank per exchange, {exch_per_frame:g} exchanges per frame (the previous frame's final reservoirs are fetched only by frames whose reprojection can cross a tile border: not while camera and scene stand still)"
                       if (tiled is not None and world > 1) else "") + ("; every rank's FINAL tile stays on its device (no gather inside the timed region)" if world > 1 else ""),
                   "halo_transport": (tiled.transport if (tiled is not None and world > 1) else None),
                   "preset": args.config, "settle_frames": settle_frames, "ramp_frames": ramp, "arith": args.arith, "library": os.path.basename(api.LIB_PATH),
                   # which permutation of the ReSTIR kernels this scene ran (zr_kernels.h PLAIN: scenes whose material table has no metal, transmission, thin
                   # wall, coat or texture run kernels without code for those lobes; one such material anywhere and the frame runs the general kernels)
                   "frame_overlap": overlap,
                   "kernel_class": ("plain" if (r.scene.material_class() == 1 and not args.textured and args.kernel_class != "general") else "general"),
                   "rays_per_frame": round((n_closest + n_shadow) / args.steps, 1),
                   "redundant_apron_primary_rays_per_frame": round(apron_rays / args.steps, 1),
                   "fps": round(1e3 / ms_per_step, 2)},
    }

    if dumped is not None:
        out["dump_outputs"] = dumped
    if dev_state is not None:
        out["device_state"] = dev_state
        if dist is not None:
            # first contact with a multi-GPU node: one row per rank -- device index, name, the three probes -- so that a slow or misplaced rank is visible in the line
            row = {"rank": rank, "device": local_rank, "name": dev_state.get("name"), "copy_GBs": dev_state.get("probe_copy_GBs"), "fma_tflops": dev_state.get("probe_fma_tflops"),
                   "sclk_mhz": dev_state.get("probe_sclk_mhz_under_load"), "error": dev_state.get("error")}
            rows = [None] * world
            dist.all_gather_object(rows, row)
            out["device_state"]["ranks"] = rows
    if args.full and world == 1 and (rpt or args.integrator == "restir_gi") and out["config"]["kernel_class"] == "plain" and not args.no_general_kernels:
        # the same frames on the GENERAL kernel permutations (zr_debug_set_material_class_kernels(0): what this scene would run with one glass sphere in it),
        # same protocol: a few frames to settle, then args.steps frames between two barriers.  Results are identical (test_material_class_kernels_change_nothing)
        L = api.lib()
        L.zr_debug_set_material_class_kernels(0)
        try:
            for i in range(max(args.warmup, 8)):
                frame(3000 + i)
            barrier()
            t1 = time.perf_counter()
            for i in range(args.steps):
                frame(3100 + i)
            barrier()
            out["general_kernels"] = {"kernel_class": "general", "ms_per_step": round((time.perf_counter() - t1) / args.steps * 1e3, 4), "steps": args.steps,
                                      "note": "the same scene and frames with the material-class permutations switched off (zr_debug_set_material_class_kernels(0)); bit-identical output"}
        finally:
            L.zr_debug_set_material_class_kernels(1)
        for i in range(4):      # back on the PLAIN kernels before the per-kernel timing below
            frame(3200 + i)
        barrier()
        r.p_gbuffer.read_counters(reset=True)
        r.p_indirect.read_counters(reset=True)
    if os.environ.get("ZR_K11") == "trip" and rpt and world == 1:
        # diagnostic build of K11: lanes alive at its bounce boundaries; the timings of this run mean nothing
        a, b, wds = r.p_indirect.debug_trip_stats()
        out["config"]["k11_bounce_boundaries"] = {"alive_lanes": a, "lane_slots": b, "alive_frac": round(a / max(b, 1), 4), "carried_state_bytes_per_path": 4 * wds}
    if args.full and overlap and world == 1:
        # what follows times kernels and single frames one at a time: the plain order on one stream (kernel times under overlap are the times of two kernels sharing the device).
        # Before that, the same protocol once more with the switch off: the pair (overlapped, plain) goes on the line
        barrier()
        (tiled if tiled is not None else r).enable_frame_overlap(False)
        for i in range(max(args.warmup, 8)):
            frame(2500 + i)
        barrier()
        t1 = time.perf_counter()
        for i in range(args.steps):
            frame(2600 + i)
        barrier()
        out["frame_overlap_off"] = {"ms_per_step": round((time.perf_counter() - t1) / args.steps * 1e3, 4), "steps": args.steps,
                                    "note": "the same frames in the plain order on one stream (zr_pass_set_frame_overlap(0)); bit-identical output"}
        r.p_gbuffer.read_counters(reset=True)
        r.p_indirect.read_counters(reset=True)
    if args.full and rank == 0 and world == 1:
        # ---- roofline of the dominant kernel: hipEvent timing inside the library over a few timed frames
        r.p_gbuffer.enable_timing(True)
        r.p_indirect.enable_timing(True)
        if r.p_sky is not None:
            r.p_sky.enable_timing(True)
        for q in di_passes:
            q.enable_timing(True)
        if p_denoise is not None:
            p_denoise.enable_timing(True)
        agg = {}
        nfr = 8
        r.p_indirect.read_counters(reset=True)
        for q in di_passes:
            q.read_counters(reset=True)
        for i in range(nfr):
            frame(1000 + i)
            torch.cuda.synchronize()
            tm = {**r.p_gbuffer.timings(), **({} if args.di_only else r.p_indirect.timings())}
            for q in di_passes + ([r.p_sky] if r.p_sky is not None else []) + ([p_denoise] if p_denoise is not None else []):
                tm.update(q.timings())
            for name, (ms, launches) in tm.items():
                a = agg.setdefault(name, [0.0, 0])
                a[0] += ms
                a[1] += launches
        prof = read_prof(api)      # only a -DZR_PROF measurement build exports the section counters (scripts/gpu.sh prof)
        if prof is not None:
            out["prof"] = prof
        kern_rays = r.p_indirect.kernel_counters()
        di_rays = {}
        for q in di_passes:      # the DI passes' per-kernel ray counts over the same nfr frames
            di_rays.update(q.kernel_counters())
        cc, cs = r.p_indirect.read_counters(reset=True)
        r.p_gbuffer.read_counters(reset=True)
        r.p_gbuffer.enable_timing(False)
        r.p_indirect.enable_timing(False)
        # per-frame wall time distribution (SURVEY 8(d) timing protocol): host clock around one frame + device sync
        ft = []
        for i in range(64 if ms_per_step < 10.0 else 16):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            frame(2000 + i)
            torch.cuda.synchronize()
            ft.append((time.perf_counter() - t1) * 1e3)
        out["config"]["frame_ms_median"] = round(float(np.median(ft)), 4)
        out["config"]["frame_ms_p95"] = round(float(np.percentile(ft, 95)), 4)
        dom = max(agg, key=lambda k: agg[k][0])
        launches = agg[dom][1]
        avg_ms = agg[dom][0] / launches
        if dom == "rgi":
            kcc, kcs = kern_rays.get(dom, (0, 0))
            bytes_launch = (BYTES_CLOSEST * kcc + BYTES_SHADOW * kcs) / launches + (23 + 2 * 40 + 27 + 16) * W * H
        elif dom.startswith("rpt_"):
            # per-ray model of SURVEY.md section 8(d) on the rays this kernel issued + the per-pixel reservoir / G-buffer
            # bytes it must touch
            kcc, kcs = kern_rays.get(dom, (0, 0))
            bytes_launch = (BYTES_CLOSEST * kcc + BYTES_SHADOW * kcs) / launches + RPT_PIXEL_BYTES.get(dom, 0) * W * H
        elif dom == "trace":
            bytes_launch = (TRACE_CLOSEST * cc + TRACE_SHADOW * cs) / launches
        elif dom == "pt_shade":
            bytes_launch = (SHADE_CLOSEST * cc + SHADE_SHADOW * cs) / launches
        elif dom in ("sdi_temporal", "sdi_spatial", "rdi_temporal", "rdi_spatial"):
            # DI: shadow / visibility rays of this kernel + the G-buffer planes (27 B) and reservoir planes it reads and writes
            kcc, kcs = di_rays.get(dom, (0, 0))
            bytes_launch = (BYTES_CLOSEST * kcc + BYTES_SHADOW * kcs) / launches + (27 * 3 + 2 * 13 + 32) * W * H
        elif dom == "gbuffer":
            bytes_launch = (BYTES_CLOSEST + 47) * W * H
        elif dom.startswith("denoise_"):
            bytes_launch = DENOISE_PIXEL_BYTES[dom] * W * H
        else:
            raise RuntimeError(f"bench.py has no algorithmic-bytes model for the dominant kernel '{dom}' (timed kernels: {sorted(agg)}): "
                               f"add it to the byte tables instead of reporting a roofline of 0")
        if dom.startswith("rpt_") and dom not in RPT_PIXEL_BYTES:
            raise RuntimeError(f"bench.py: ReSTIR PT kernel '{dom}' is missing from RPT_PIXEL_BYTES")
        achieved = bytes_launch / (avg_ms * 1e-3) / 1e9
        plane_px = (RPT_PIXEL_BYTES.get(dom) if dom.startswith("rpt_") else (23 + 2 * 40 + 27 + 16) if dom == "rgi" else (27 * 3 + 2 * 13 + 32) if dom in ("sdi_temporal", "sdi_spatial", "rdi_temporal", "rdi_spatial") else
                    47 if dom == "gbuffer" else DENOISE_PIXEL_BYTES.get(dom))
        plane_bytes = round(plane_px * W * H) if plane_px else None
        frame_bytes = (BYTES_CLOSEST * (cc / nfr + W * H) + BYTES_SHADOW * (cs / nfr) + (47 + 38 + 16) * W * H)
        # measured HBM-side bytes per launch of that kernel: PMC passes (FETCH_SIZE x 2 x 1024 + WRITE_SIZE x 1024, MI355X_MICROARCH.md) of
        # exactly this command, collected by scripts/gpu.sh profiles and committed under profiles/ (rocprofv3 cannot run inside the bench)
        traffic, traffic_src, valu = None, None, None
        plain = not (args.direct or args.sky_direct or args.textured or args.di_only)
        scene_tag = ("cornell" if args.scene.endswith("cornell_emissive.npz") else
                     "atrium" if (args.scene == "synthetic" and args.synthetic_layout == "atrium" and args.synthetic_tris == 262144
                                  and args.synthetic_emissives == 100000) else None)
        wl_tag = {"restir_pt": "rpt", "restir_gi": "gi", "pt": "pt"}[args.integrator] + ("" if (W, H) == (1920, 1080) else f"_{W}x{H}")
        pmc_rel = next((q for q in (os.path.join("profiles", f"{rnd}_pmc_{wl_tag}_{scene_tag}.json") for rnd in ("r06", "r05", "r04", "r03"))
                        if os.path.exists(os.path.join(ROOT, q))), "")
        # BASELINE config 2's halves (--config 2a / 2b: the DI pass alone on its own Cornell scene at 1080p) have profiles of their own
        di_cfg = args.di_only and not args.textured and (W, H) == (1920, 1080) and os.path.basename(args.scene) in ("cornell_emissive.npz", "cornell.npz")
        if di_cfg:
            plain, scene_tag = True, "cornell"
            pmc_rel = os.path.join("profiles", "r06_pmc_2a.json" if args.direct else "r06_pmc_2b.json")
            pmc_rel = pmc_rel if os.path.exists(os.path.join(ROOT, pmc_rel)) else ""
        if plain and scene_tag and pmc_rel:
            table = json.load(open(os.path.join(ROOT, pmc_rel)))
            # only a profile of THESE kernel sources describes the library that was just timed
            if table.get("_meta", {}).get("source_hash") == source_hash():
                # kernel names as rocprofv3 prints them carry their template arguments (NEE_EMISSIVE, TEXTURED, PLAIN: k_rpt_pathtrace<true, true>, k_rgi<true>, ...):
                # every permutation of the stage's kernel is a candidate ...
                kmap = {"rpt_pathtrace": ["k_rpt_pathtrace", "k_rpt_pathtrace_w4", "k_rpt_pathtrace_tex", "k_rpt_pathtrace_coop", "k_rpt_pathtrace_coop_w4"],
                        "rpt_reconnect_spatial": ["k_rpt_stc"], "rpt_reconnect_temporal": ["k_rpt_temporal"],
                        "gbuffer": ["k_gbuffer"], "rgi": ["k_rgi", "k_rgi_tex"], "trace": ["k_trace_simple", "k_trace"], "pt_shade": ["k_pt_shade", "k_pt_shade_tex"],
                        "rdi_temporal": ["k_rdi_temporal"], "rdi_spatial": ["k_rdi_spatial"], "sdi_temporal": ["k_sdi_temporal"], "sdi_spatial": ["k_sdi_spatial"]}
                # ... and the launch-count filter drops a permutation that only ran during warm-up
                cands = [rec_ for k, rec_ in table.items() if k != "_meta" and k.split("<")[0] in kmap.get(dom, [])]
                rec = max(cands, key=lambda r: r.get("launches_sampled", 0)) if cands else None
                if rec:
                    traffic, traffic_src = round(rec["traffic_bytes"]), pmc_rel
                    if "valu" in rec:
                        valu = dict(rec["valu"], source=pmc_rel)
        hbm_frac = achieved / HBM_PEAK_GBS
        # which resource bounds the dominant kernel: the VALU issue slots when the PMC pass shows them busier than the HBM pipe
        bound = "valu" if (valu is not None and valu.get("busy_frac", 0) > max(hbm_frac, (traffic or 0) / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS)) else "hbm"
        out["roofline"] = {"bound": bound, "kernel": dom, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": round(hbm_frac, 5), "traffic": traffic, "traffic_unit": "bytes per launch",
                           "traffic_source": traffic_src, "algorithmic_bytes_per_launch": round(bytes_launch),
                           "traffic_over_algorithmic": (round(traffic / bytes_launch, 3) if (traffic and bytes_launch) else None),
                           # against the planes alone (what the pass must read / write per pixel; the per-ray record bytes of SURVEY 8(d) never
                           # leave the registers of a megakernel): everything above ~1 is scene data that missed the caches + scratch spills
                           "plane_bytes_per_launch": plane_bytes, "traffic_over_plane_bytes": (round(traffic / plane_bytes, 3) if (traffic and plane_bytes) else None),
                           "measured_traffic_GBs": (round(traffic / (avg_ms * 1e-3) / 1e9, 2) if traffic else None),
                           "valu": valu,
                           "avg_launch_ms": round(avg_ms, 4), "launches_per_frame": launches / nfr,
                           "frame_model_GBs": round(frame_bytes / (ms_per_step * 1e-3) / 1e9, 2),
                           "kernel_ms_per_frame": {k: round(v[0] / nfr, 4) for k, v in agg.items()},
                           "kernel_ms_note": f"hipEvent pairs around every launch over {nfr} frames rendered one at a time AFTER the timed region; the events and the per-frame "
                                             "synchronisation make that pass a few per cent slower than the untimed frames ms_per_step is measured on, so the sum may exceed it"}
        if not args.no_cpu_baseline:
            cbf = scene_io.make_frame_constants(W, H, frame_num=1, num_emissives=len(sc.emissives), **cam)
            if tex_offsets is not None:
                scene_io.set_texture_heap_offsets(cbf, tex_offsets)
            out["cpu_baseline"] = cpu_baseline(sc, cbf, rpt_params=prm if rpt else None, max_rays=1_000_000 if args.scene != "synthetic" else 200_000,
                                               sample=(2, 8) if args.scene != "synthetic" else (4, 4))
    if args.full and world > 1 and tiled is not None:
        # ---- first contact with a multi-GPU node (a run nobody can debug afterwards): every rank reports where it ran, what it sends and how long ONE halo
        # exchange takes on its own (8 back-to-back exchanges of the planes as they stand -- idempotent -- between two barriers)
        post, _final = tiled.EXCHANGES[tiled.kind]
        which = api.HALO_POST_TEMPORAL if post else api.HALO_FINAL
        exch_ms, exch_err = None, None
        try:
            barrier()
            t1 = time.perf_counter()
            for _ in range(8):
                tiled.exchange(which)
            barrier()
            exch_ms = round((time.perf_counter() - t1) / 8 * 1e3, 4)
            tiled.exchanges_done -= 8
        except Exception as e:      # the line must not die over an annotation
            exch_err = repr(e)[:200]
        try:
            rccl = ".".join(str(v) for v in torch.cuda.nccl.version()) if dist.get_backend() == "nccl" else None
        except Exception:
            rccl = None
        row = {"rank": rank, "device": local_rank, "tile": list(tiled.tile), "halo_bytes_sent_per_exchange": int(tiled.halo_bytes), "halo_bytes_per_pixel": int(tiled.bpp),
               "peers": len(tiled.plan), "transport": tiled.transport, "exchange_ms": exch_ms, "exchange_error": exch_err}
        rows = [None] * world
        dist.all_gather_object(rows, row)
        out["multi_gpu"] = {"backend": dist.get_backend(), "rccl_version": rccl, "communicator_size": dist.get_world_size(), "exchanges_per_frame": exch_per_frame,
                            "halo_pass": tiled.kind, "ranks": rows}
    if args.full and world > 1 and tiled is not None and rpt:
        # ---- N > 1: the fraction of the HBM roofline of the whole job (north_star: "at 1 / 2 / 4 / 8 GPUs ... as fraction of the HBM roofline").  Every rank
        # times the metric's kernel (K11) on its tile with the library's hipEvents over a few frames; achieved = the ranks' algorithmic bytes per launch
        # (per-ray model on the rays the kernel issued + the planes of the OWNED pixels) summed, over the slowest rank's launch time; peak = N x 8 TB/s.
        dom = "rpt_pathtrace"
        if overlap:
            barrier()
            tiled.enable_frame_overlap(False)      # a kernel's own time: the plain order (under overlap it shares the device with the other half's kernels)
        r.p_indirect.enable_timing(True)
        r.p_indirect.read_counters(reset=True)
        nfr, agg_ms, agg_n = 8, 0.0, 0
        dist.barrier()
        for i in range(nfr):
            frame(1000 + i)      # (collective: every rank renders the same number of frames whatever its timers say)
            torch.cuda.synchronize()
            ms, launches = r.p_indirect.timings().get(dom, (0.0, 0))
            agg_ms += ms
            agg_n += launches
        try:      # a rank that cannot produce its share contributes zeros: the line must not die (or hang the others) over an annotation
            kcc, kcs = r.p_indirect.kernel_counters().get(dom, (0, 0))
            r.p_indirect.read_counters(reset=True)
            r.p_indirect.enable_timing(False)
            avg_ms = agg_ms / max(agg_n, 1)
            bytes_launch = (BYTES_CLOSEST * kcc + BYTES_SHADOW * kcs) / max(agg_n, 1) + RPT_PIXEL_BYTES[dom] * tw * th
        except Exception:
            bytes_launch, avg_ms = 0.0, 0.0
        mine = torch.tensor([bytes_launch, avg_ms], dtype=torch.float64, device=cdev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        if rank == 0:
            per = [(float(t[0]), float(t[1])) for t in every]
            slowest = max(max(m for _, m in per), 1e-9)
            achieved = sum(b for b, _ in per) / (slowest * 1e-3) / 1e9
            out["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS * world, "unit": "GB/s",
                               "frac": round(achieved / (HBM_PEAK_GBS * world), 5), "traffic": None,
                               "per_rank_achieved_GBs": [round(b / (m * 1e-3) / 1e9, 2) if m > 0 else None for b, m in per],
                               "per_rank_avg_launch_ms": [round(m, 4) for _, m in per],
                               "note": "whole job: the ranks' algorithmic bytes per launch of the metric's kernel summed over the slowest rank's launch time, against N x the HBM peak; "
                                       "traffic / VALU counters are collected at N = 1 (profiles/)"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed frames (default 256, or the --config preset's when it names one)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed frames right before the timed ones (default 64, or the --config preset's)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: device probes, general-kernel and plain-order timings, roofline, CPU baseline, "
                         "and on the default line BASELINE configs 4 and 5 and the tolerance-mode build; N > 1: the multi_gpu block and the whole-job roofline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the cpu_baseline block")
    ap.add_argument("--arith", choices=["contract", "fast"], default="contract",
                    help="contract = libzetaray_amd.so, the bit-exact arithmetic contract of include/zr_detmath.h (the product default, what every parity test "
                         "loads); fast = libzetaray_amd_fast.so, the tolerance-mode build of the same sources (hardware rcp / rsq / exp / log / sin / cos, "
                         "contracted FMAs; parity = tests/test_fast_arith.py).  A fast line says so in config.arith and is never the default.")
    ap.add_argument("--no-extra-workloads", action="store_true",
                    help="--full on the default line also measures BASELINE configs 4 and 5 in the same process (extra_workloads) and the tolerance-mode build "
                         "in a child process (tolerance_mode); this skips them")
    ap.add_argument("--denoise", action="store_true", help="add the denoise pass (ZR_PASS_DENOISE) on the indirect image (tile-split like the integrator for N > 1)")
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "cornell_emissive.npz"),
                    help="wire-format .npz, or 'synthetic' = the procedural Sponza-class scene of BASELINE config 4 "
                         "(262144 triangles + 100000 emissive triangles, presampled light sets on)")
    ap.add_argument("--synthetic-tris", type=int, default=262144)
    ap.add_argument("--synthetic-layout", choices=["atrium", "soup"], default="atrium")
    ap.add_argument("--synthetic-emissives", type=int, default=100000)
    ap.add_argument("--no-final-halo", action="store_true",
                    help="skip the post-frame halo exchange (exact for a static camera, which this bench uses)")
    ap.add_argument("--direct", action="store_true", help="also run the ReSTIR DI (emissive) pass every frame (N = 1)")
    ap.add_argument("--sky-direct", action="store_true", help="also run the sun + sky ReSTIR DI pass (K7/K8) every frame (N = 1)")
    ap.add_argument("--textured", action="store_true",
                    help="bind the procedural test texture set to the synthetic scene (TEXTURED kernel permutations: ray differentials, material maps)")
    ap.add_argument("--di-only", action="store_true", help="skip the indirect pass: BASELINE config 1 (ReSTIR DI only)")
    ap.add_argument("--integrator", choices=["restir_pt", "restir_gi", "pt"], default="restir_pt",
                    help="restir_pt = K11-K16 (BASELINE metric); pt = K9 unidirectional path tracer")
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None,
                    help="BASELINE.json configuration presets (same JSON line; the default without --config is the metric's own configuration, "
                         "Cornell (emissive) 1920x1080 ReSTIR PT): " + "; ".join(f"{k} = {v[0]}" for k, v in sorted(CONFIGS.items())))
    ap.add_argument("--ramp-s", type=float, default=0.6,
                    help="seconds of back-to-back frames of the workload rendered before --warmup so that the device's clocks have ramped (0 = none)")
    ap.add_argument("--no-device-state", action="store_true", help="--full without the device_state block (zr_device_probe_run + amdsmi)")
    ap.add_argument("--no-general-kernels", action="store_true", help="--full without the general-kernel timing of a plain-class scene (general_kernels)")
    ap.add_argument("--kernel-class", choices=["auto", "general"], default="auto",
                    help="general = run a plain-class scene on the general kernel permutations (zr_debug_set_material_class_kernels(0)) for the whole run")
    ap.add_argument("--frame-overlap", type=int, choices=[0, 1], default=1,
                    help="1 (default) = consecutive ReSTIR PT frames software-pipelined on two streams: the G-buffer and K11 of frames N + 1 / N + 2 beside the reuse passes of frame N "
                         "(zetaray_amd.h zr_pass_set_frame_overlap; bit-identical frames) -- ms_per_step is then the frame THROUGHPUT; with --full, config.frame_ms_median is the latency "
                         "of one frame rendered alone and frame_overlap_off carries the plain order's ms_per_step; 0 = the plain order on one stream")
    ap.add_argument("--settle", type=int, default=None,
                    help="untimed frames rendered BEFORE the warm-up so that the temporal reservoirs have reached their M caps whatever --warmup is "
                         "(default: 32 for the ReSTIR integrators, 0 otherwise)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed frames, write the images the timed path returned in its last frame as DIR/<name>.npy (float32, full frame; a fixed "
                         "seeded sample of pixels when they would exceed 64 MB).  The clock-ramp frames then run on a renderer of their own, so that the "
                         "timed renderer sees the same frames in every run with the same arguments")
    args = ap.parse_args()
    if args.config:
        for k, v in CONFIGS[args.config][1].items():
            if k in ("steps", "warmup") and getattr(args, k) is not None:
                continue        # an explicit --steps / --warmup wins over the preset's
            setattr(args, k, v)
    args.steps = 256 if args.steps is None else args.steps
    args.warmup = 64 if args.warmup is None else args.warmup
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher (the shape of the driver's N = 1 command): start the N ranks here -- one process per GPU
        # under torch.distributed.run on the loopback address, exactly the command the contract names -- and pass rank 0's JSON line through.
        # (Launched by torchrun / the driver, WORLD_SIZE is set and this branch is skipped.)
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this driver
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        if os.environ.get("ZR_BENCH_LAUNCH_ECHO") == "1":      # (tests on a box without GPUs: show the launch instead of performing it)
            print(json.dumps({"launch": cmd}))
            sys.exit(0)
        sys.exit(subprocess.call(cmd, env=env))
    if args.arith == "fast":
        os.environ["ZETARAY_AMD_LIB"] = os.path.join(ROOT, "zetaray_amd", "libzetaray_amd_fast.so")      # read by zetaray_amd/api.py at import
    import torch
    from zetaray_amd import api, scene_io, wire

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("ZR_BENCH_SHARED_GPU") == "1":
            # test rig for a box with one GPU (tests/test_gpu_parity.py): every rank renders on device 0, the ranks talk over gloo and the halo
            # strips go through the host -- the orchestration (probe frames, cost-balanced re-tiling, timing protocol) is the multi-GPU one
            local_rank = 0
            os.environ["ZR_HALO_TRANSPORT"] = "torch_p2p"
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    torch.cuda.set_device(local_rank)
    cdev = "cpu" if (dist is not None and dist.get_backend() == "gloo") else "cuda"      # where the few scalars of the timing protocol are reduced

    ctx = dict(world=world, rank=rank, local_rank=local_rank, dist=dist, cdev=cdev)
    if args.kernel_class == "general":
        api.lib().zr_debug_set_material_class_kernels(0)
    out = measure(args, ctx)
    default_line = (args.config is None and world == 1 and args.scene.endswith("cornell_emissive.npz") and args.integrator == "restir_pt"
                    and (args.width, args.height) == (1920, 1080) and not (args.direct or args.sky_direct or args.denoise or args.di_only or args.textured))
    if default_line and args.full and not args.no_extra_workloads:
        # `bench.py --gpus 1 --full`: `value` stays the metric's own configuration (Cornell), and BASELINE config 4's scene -- the
        # 380k-triangle / 100k-light atrium at 1080p -- is measured in the same process with its own roofline and CPU baseline
        # ... and config 5's (the same scene at 3840 x 2160 with the denoise pass; its CPU sample would be the very one of config 4 -- the oracle at
        # 480 x 270 on that scene -- so it is referenced, not re-run)
        extra = []
        for preset in ("4", "5"):
            a2 = argparse.Namespace(**vars(args))
            a2.config = preset
            a2.dump_outputs = None      # (the dump is the metric's own workload)
            for k, v in CONFIGS[preset][1].items():
                setattr(a2, k, v)
            if preset == "5":
                a2.no_cpu_baseline = True
            o2 = measure(a2, ctx)
            cpu = o2.get("cpu_baseline")
            if preset == "5" and extra and extra[0].get("cpu_baseline"):
                cpu = dict(extra[0]["cpu_baseline"], sample=extra[0]["cpu_baseline"]["sample"] + " (config 4's sample: same scene, same integrator)")
            extra.append({"preset": preset, "workload": o2["config"]["workload"], "ms_per_step": o2["ms_per_step"], "value": o2["value"], "unit": o2["unit"],
                          "steps": o2["steps"], "warmup": o2["warmup"], "rays_per_frame": o2["config"]["rays_per_frame"], "fps": o2["config"]["fps"],
                          "roofline": o2.get("roofline"), "cpu_baseline": cpu})
        out["extra_workloads"] = extra
        # ... and the metric's own configuration on the tolerance-mode build (libzetaray_amd_fast.so: the same sources with hardware rcp / rsq / exp /
        # log / sin / cos and contracted FMAs, include/zr_detmath.h).  The library is chosen at import time, so this is a child process, run after
        # this process's measurements; its line is reported next to `value`, never as `value` (the product default is the bit-exact contract).
        fast_lib = os.path.join(ROOT, "zetaray_amd", "libzetaray_amd_fast.so")
        if os.path.exists(fast_lib):
            import subprocess
            try:
                cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--arith", "fast", "--full", "--no-extra-workloads", "--no-cpu-baseline", "--no-device-state", "--no-general-kernels",
                                     "--steps", str(args.steps), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=600)
                o3 = json.loads([l for l in cp.stdout.splitlines() if l.startswith("{")][-1])
                out["tolerance_mode"] = {"arith": "fast", "library": o3["config"]["library"], "ms_per_step": o3["ms_per_step"], "value": o3["value"], "unit": o3["unit"],
                                         "steps": o3["steps"], "warmup": o3["warmup"], "speedup_vs_contract": round(out["ms_per_step"] / o3["ms_per_step"], 4),
                                         "roofline": {k: o3["roofline"].get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_ms", "kernel_ms_per_frame")},
                                         "parity": "tests/test_fast_arith.py: 256-frame accumulated radiance vs the oracle rel. L2 <= 0.08, frame-1 integer reservoir state equal on >= 0.999 of the pixels"}
            except Exception as e:      # the default line must not die with the child
                out["tolerance_mode"] = {"arith": "fast", "error": repr(e)[:300]}
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
