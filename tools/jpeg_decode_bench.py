"""Cost of creating a scene whose material textures arrive as JPEG files, at two texture counts (--textures A B, default 16 128; each --size^2, default
2048, with a full mip chain in the heap; three quarters 4:2:0 colour files as RGBA8_SRGB maps, one quarter grey files as RG8 maps).  The files are the two
64 x 64 bench files of tests/golden/jpeg_cases.npz repeated to --size^2 by tile_jpeg below (they carry one restart interval per MCU row of the tile, so
their entropy-coded intervals can be repeated as they are).  The scene is one quad, so texture work is all there is.
  (A) what the same bytes cost without the device decode: zrh_jpeg_decode on the host (entropy decode + include/zr_jpeg.h), then
      zr_scene_create_compressed with RAW_MIP0 sources
  (B) zrh_jpeg_pack on the host (the entropy decode alone), then zr_scene_create_compressed with JPEG_COEF sources
The host step is timed per distinct file, --host-reps times (default 3), and counted once per texture; the creation is the median and p10 / p90 of --reps
after --warmup (default 16 after 4), host wall time.  Also: the bytes over the bus, and the time of a whole zr_jpeg_decode_device call between two events on its stream, beside that of
its payload read-back alone.  The call validates the records on the host between the two events, so this is NOT the stream time of the two launches;
that takes a kernel trace.  Prints one JSON line.  Exit status 1 unless, at both counts, (B)'s total
median is not above (A)'s plus (A)'s p10 - p90 spread and the heaps are equal.  GPU only; scripts/gpu.sh jpeg runs it."""
import ctypes as C
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


def _segments(d):
    """[(marker, start, end)] of the segments before the scan, and where the entropy-coded data starts"""
    at, out = 2, []
    while True:
        m, n = d[at + 1], (d[at + 2] << 8) | d[at + 3]
        out.append((m, at, at + 2 + n))
        at += 2 + n
        if m == 0xDA:
            return out, at


def tile_jpeg(data, size):
    """a 64 x 64 file whose restart interval is one MCU row of it -> the same content repeated to size x size (a multiple of 64): the frame header gets the
    new size, interval (r, c) of the result is interval r mod (rows of the tile) of the file, the restart markers are numbered anew"""
    d = bytes(data)
    segs, scan = _segments(d)
    head = bytearray(d[:scan])
    sof = next(s for s in segs if s[0] == 0xC0)
    assert head[sof[1] + 5:sof[1] + 9] == bytes([0, 64, 0, 64]) and size % 64 == 0
    head[sof[1] + 5:sof[1] + 9] = size.to_bytes(2, "big") * 2
    body, parts, at = d[scan:d.rindex(b"\xff\xd9")], [], 0
    for i in range(len(body) - 1):
        if body[i] == 0xFF and 0xD0 <= body[i + 1] <= 0xD7:
            parts.append(body[at:i])
            at = i + 2
    parts.append(body[at:])
    out, k = [bytes(head)], 0
    for r in range(len(parts) * (size // 64)):
        for c in range(size // 64):
            if k:
                out.append(bytes([0xFF, 0xD0 + (k - 1) % 8]))
            out.append(parts[r % len(parts)])
            k += 1
    return b"".join(out) + b"\xff\xd9"


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
    from tests.jpegmath import zjp
    L = scene_io._sceneio_lib()
    L.zrh_jpeg_decode.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.zrh_jpeg_pack.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    out = {"mode": "jpeg_decode", "texture_size": size, "reps": reps, "warmup": warmup, "host_reps": host_reps,
           "library": os.path.basename(api.LIB_PATH), "device_state": bench.device_state(api, 0), "sizes": []}
    copy_rate = out["device_state"].get("probe_copy_GBs")

    def note(*a):      # (progress on stderr: the one JSON line is all stdout gets)
        print(*a, file=sys.stderr, flush=True)
    fx = {n: d for n, d, _ in zjp.load_fixture()}
    files = {"colour": tile_jpeg(fx["64x64_420_q90_bench"], size), "grey": tile_jpeg(fx["64x64_gray_q90_bench"], size)}
    # ---- the host steps, one call each, per distinct file
    host, level0, record = {}, {}, {}
    for kind, data in files.items():
        cmap = wire.JPEG_MAP_RGBA if kind == "colour" else wire.JPEG_MAP_RG
        w, h, nrec = C.c_uint32(), C.c_uint32(), C.c_size_t()
        rgba = np.zeros((size, size, 4), np.uint8)
        rec = np.zeros(496 + (4 + 128) * (size // 8) ** 2 * 2 + 64, np.uint8)      # (room for every coefficient of every block)
        t_dec, t_pack = [], []
        for _ in range(host_reps):
            a = time.perf_counter()
            assert L.zrh_jpeg_decode(b"bench.jpg", data, len(data), C.byref(w), C.byref(h), rgba.ctypes.data, rgba.nbytes) == 0, L.zrh_scene_io_last_error()
            b = time.perf_counter()
            assert L.zrh_jpeg_pack(b"bench.jpg", data, len(data), cmap, rec.ctypes.data, rec.nbytes, C.byref(nrec)) == 0, L.zrh_scene_io_last_error()
            c = time.perf_counter()
            t_dec.append((b - a) * 1e3)
            t_pack.append((c - b) * 1e3)
        assert (w.value, h.value) == (size, size)
        tile = scene_io.decode_jpeg(fx["64x64_420_q90_bench" if kind == "colour" else "64x64_gray_q90_bench"])
        # (the chroma filter reaches one sample across a tile's edge: compare what it cannot reach)
        assert np.array_equal(rgba[:60, :60], tile[:60, :60]) and np.array_equal(rgba[-60:, -60:], tile[-60:, -60:]), "the tiled file does not decode to the tile"
        level0[kind] = rgba.reshape(-1).copy() if kind == "colour" else np.ascontiguousarray(rgba[..., [0, 1]]).reshape(-1)
        record[kind] = rec[:nrec.value].copy()
        host[kind] = {"file_bytes": len(data), "record_bytes": int(nrec.value), "decode_ms": _stats(t_dec), "entropy_decode_ms": _stats(t_pack)}
        note(kind, host[kind])
    out["host_per_texture"] = host
    mips = int(np.log2(size)) + 1
    sides = [max(1, size >> m) for m in range(mips)]
    ok = True
    for n in counts:
        note("textures", n)
        kinds = ["grey" if i % 4 == 3 else "colour" for i in range(n)]
        fmts = [wire.TEX_RG8 if k == "grey" else wire.TEX_RGBA8_SRGB for k in kinds]
        chain = [(2 if k == "grey" else 4) * sum(s * s for s in sides) for k in kinds]
        slot = [(c + 3) // 4 * 4 for c in chain]
        descs = np.zeros(n, wire.TEXTURE_DESC)
        descs["offset"] = np.concatenate([[0], np.cumsum(slot)[:-1]])
        descs["width"], descs["height"], descs["num_mips"], descs["format"] = size, size, mips, fmts
        heap_bytes = int(sum(slot))
        res = {"textures": n, "heap_MB": round(heap_bytes / 1e6, 1), "file_MB": round(sum(len(files[k]) for k in kinds) / 1e6, 2)}
        res["A_host_decode_ms"] = round(sum(host[k]["decode_ms"]["median"] for k in kinds), 1)
        res["B_host_entropy_decode_ms"] = round(sum(host[k]["entropy_decode_ms"]["median"] for k in kinds), 1)
        # ---- (A) the host's level 0 as RAW_MIP0 sources
        sa = _quad()
        sa.textures, sa.texel_heap_bytes = descs.copy(), heap_bytes
        sa.texture_sources = np.zeros(n, wire.TEXTURE_SOURCE)
        n0 = [len(level0[k]) for k in kinds]
        sa.texture_sources["offset"], sa.texture_sources["encoding"] = np.concatenate([[0], np.cumsum(n0)[:-1]]), wire.TEX_SRC_RAW_MIP0
        sa.texture_payload = np.concatenate([level0[k] for k in kinds])
        t_a, heap_a = _time_creations(sa, reps, warmup)
        note("A done")
        res["A_payload_MB"] = round(len(sa.texture_payload) / 1e6, 1)
        res["A_create_ms"] = _stats(t_a)
        del sa
        # ---- (B) the records as JPEG_COEF sources
        sb = _quad()
        sb.textures, sb.texel_heap_bytes = descs.copy(), heap_bytes
        sb.texture_sources = np.zeros(n, wire.TEXTURE_SOURCE)
        nr = [len(record[k]) for k in kinds]
        sb.texture_sources["offset"], sb.texture_sources["encoding"] = np.concatenate([[0], np.cumsum(nr)[:-1]]), wire.TEX_SRC_JPEG_COEF
        sb.texture_payload = np.concatenate([record[k] for k in kinds])
        t_b, heap_b = _time_creations(sb, reps, warmup)
        note("B done")
        res["B_payload_MB"] = round(len(sb.texture_payload) / 1e6, 1)
        res["B_create_ms"] = _stats(t_b)
        res["heaps_equal"] = bool(np.array_equal(heap_a, heap_b))
        del heap_a, heap_b
        res["A_total_ms"] = round(res["A_host_decode_ms"] + res["A_create_ms"]["median"], 1)
        res["B_total_ms"] = round(res["B_host_entropy_decode_ms"] + res["B_create_ms"]["median"], 1)
        res["B_limit_ms"] = round(res["A_total_ms"] + (res["A_create_ms"]["p90"] - res["A_create_ms"]["p10"]), 1)
        res["B_within_limit"] = bool(res["B_total_ms"] <= res["B_limit_ms"])
        # ---- the stand-alone entry between events (read-back, host validation, the two launches), and the read-back alone
        one = np.zeros(n, wire.TEXTURE_DESC)
        one["offset"], one["width"], one["height"], one["num_mips"], one["format"] = np.concatenate([[0], np.cumsum(n0)[:-1]]), size, size, 1, fmts
        d_payload = torch.from_numpy(sb.texture_payload).cuda()
        d_texels = torch.zeros(int(sum(n0)), dtype=torch.uint8, device="cuda:0")
        back = torch.empty(len(sb.texture_payload), dtype=torch.uint8)
        st = torch.cuda.Stream()
        ms_call, ms_back = [], []
        for k in range(warmup + reps):
            for what, sink in (("call", ms_call), ("back", ms_back)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                if what == "call":
                    api._check(api.lib().zr_jpeg_decode_device(0, st.cuda_stream, one.ctypes.data, sb.texture_sources.ctypes.data, n, d_payload.data_ptr(),
                                                               len(sb.texture_payload), d_texels.data_ptr(), int(sum(n0))))
                else:
                    with torch.cuda.stream(st):
                        back.copy_(d_payload, non_blocking=True)
                    st.synchronize()
                e1.record(st)
                torch.cuda.synchronize()
                if k >= warmup:
                    sink.append(e0.elapsed_time(e1))
        res["level0_equals_the_host"] = bool(np.array_equal(d_texels.cpu().numpy(), np.concatenate([level0[k] for k in kinds])))
        res["call_stream_ms"], res["readback_stream_ms"] = _stats(ms_call), _stats(ms_back)
        del d_payload, d_texels, back, sb
        ok = ok and res["heaps_equal"] and res["level0_equals_the_host"] and res["B_within_limit"]
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
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    sys.exit(run(a.textures, a.size, a.reps, a.warmup, a.host_reps))
