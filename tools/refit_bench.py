"""Latency of zr_scene_update_instances on the BASELINE config-4 stand-in (262k-triangle atrium): device refit (default) next to the host rebuild
(ZR_SCENE_UPDATE=rebuild), and the ReSTIR PT frame time on the refit / rebuilt tree after the largest non-emissive clutter instance moved.
Prints one JSON line; scripts/gpu_refit.sh [rounds 1-4: git history up to 31e92fa; today scripts/gpu.sh ab] runs it once per mode.  GPU only.

--device-records: one dynamic frame's SCENE UPDATE both ways on the same scene with its light instance moving every frame -- the host path
(zrh_scene_data_begin_frame / _set_instance_world, zr_scene_update_emissives_async + zr_scene_update_instances_async) and the device form
(zr_scene_move_instances_async) -- as host wall time from the first call to the last return and as stream time between two events, at two light
counts a factor of 8 apart (--emissive N and N / 8).  Median and p10 / p90 of --frames frames after --warmup; one JSON line.  Exit status 1 when the
device path's host time at the larger count exceeds that at the smaller by more than the smaller run's p10 - p90 spread.

--animate: keyframe animation of N single-quad instances, all animated, two keys each, flat hierarchy (--instances N and 16 N; the smaller scene
carries one static clutter instance that brings it to the larger one's triangle count, so that both refit trees are equally deep and the refit's one
launch per level costs either size the same host time).  (A) the C++ mirror samples on the host (zrh_scene_data_begin_frame + zrh_scene_data_animate)
and hands the moved list to zr_scene_move_instances_async; (B) zr_scene_animate_async.  Host wall time of the update and stream time between two events,
median and p10 / p90 of --frames frames after --warmup; one JSON line with the device probes.  Exit status 1 when (B)'s host time at 16 N exceeds that
at N by more than the smaller run's p10 - p90 spread, or (B)'s stream time is longer than (A)'s at either size.

--skin: one skinned tube of N vertices over 64 joints, all animated (--vertices N and 16 N; the smaller scene carries one static clutter instance that
brings it to the larger one's triangle count, as under --animate).  (A) the host form: zrh_skin_pose on the host, zr_scene_update_vertices_async, then
the host-form instance update; (B) zr_scene_animate_async with the skin set; (C) the same animation without a skin, whose stream time taken from (B)'s
leaves the two skin kernels' own, reported next to the bytes they must move (28 + 24 in, 28 + 16 out per vertex).  Same statistics, same JSON line,
exit status 1 under the same two conditions on (B), or when the twin scenes' vertex buffers differ.

--morph: the same tube of N vertices (--vertices N and 16 N, the clutter as above) under 8 morph targets, each with POSITION and NORMAL deltas, driven by
one looping track of 3 keys.  (A) the host form: zrh_morph_pose on the host, zr_scene_update_vertices_async, then the host-form instance update;
(B) zr_scene_animate_async with the morph set, in two variants: all 8 weights non-zero at every time, and 1 of 8 non-zero (the other 7 targets are
skipped: no loads); (C) the same animation without the set, whose stream time taken from (B)'s leaves the morph kernels' own, reported next to the
bytes they must move (28 in, 28 + 16 out and 24 per applied target per vertex).  Same statistics, same JSON line; exit status 1 when (B)'s host time
at 16 N exceeds that at N by more than the smaller run's p10 - p90 spread, or when the twin scenes' vertex buffers differ.

--lights: the --skin tube (--vertices N and 16 N, the clutter as above) with an EMISSIVE material: every tube triangle is a light triangle the pose
deforms, about 2 N of them.  (A) the host form: zrh_skin_pose, zr_scene_update_vertices_async, zrh_scene_data_refresh_emissives over all lights, the
host-form emissive and instance updates; (B) zr_scene_animate_async with the skin set, which lists the lights and runs k_refresh_emissives; (C) the same
tube, animation and skin set with the material not emissive.  B - C is the light kernel's stream time, reported next to the bytes it moves (per light:
the 16-byte entry, the owner word, three 12-byte positions, 48 bytes of object record in, two 48-byte records out: 200) and, unless the difference lies
within the two runs' p10 - p90 drift, the bandwidth that implies; the device state carries the copy probe.  Whether (B)'s host time grows with the light
count and whether its stream time is below (A)'s are reported, not gated: exit status 1 only when the twin scenes' vertices or light records differ."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zetaray_amd import api, scene_io, wire


def main():
    w, h = 1920, 1080
    sc = scene_io.make_synthetic_scene(num_tris=262144, num_emissive=100000, layout="atrium")
    prm = wire.default_params()
    prm.presampling, prm.num_sample_sets, prm.sample_set_size = 1, 128, 512
    r = api.Renderer(sc, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    cand = [i for i in range(1, len(sc.instances)) if sc.instance_mask[i] & wire.SUBGROUP_NON_EMISSIVE]
    idx = max(cand, key=lambda i: int(sc.instance_num_tris[i]))
    t0, xf = sc.instances["translation"][idx].copy(), {}
    import torch
    upd, frames, kern = [], [], {"static": {}, "moving": {}}
    n_static, n_moving = 24, int(os.environ.get("REFIT_MOVING_FRAMES", "16"))
    r.p_gbuffer.enable_timing(True); r.p_indirect.enable_timing(True)
    for f in range(1, n_static + n_moving + 1):
        moving = f > n_static
        if moving:
            k = f - n_static
            ang = 0.05 * k
            q = np.array([0.0, np.sin(ang / 2), 0.0, np.cos(ang / 2)], np.float32)
            scene_io.move_instance(sc, idx, translation=t0 + np.float32([0.02 * k, 0.0, 0.01 * k]), rotation=q, xform_of=xf)
            torch.cuda.synchronize(); a = time.perf_counter()
            r.scene.update_instances(sc.instances, sc.instance_to_world)
            torch.cuda.synchronize(); upd.append((time.perf_counter() - a) * 1e3)
        cb = scene_io.make_frame_constants(w, h, frame_num=f, num_emissives=len(sc.emissives), cam_pos=(0, 0, -3.5))
        torch.cuda.synchronize(); a = time.perf_counter()
        r.render_frame(cb)
        torch.cuda.synchronize(); frames.append((time.perf_counter() - a) * 1e3)
        if (not moving and f > 12) or (moving and f > n_static + 4):      # steady state of either phase
            for name, (ms, launches) in {**r.p_gbuffer.timings(), **r.p_indirect.timings()}.items():
                kern["moving" if moving else "static"].setdefault(name, []).append(ms)
    kms = {ph: {k: round(float(np.mean(v)), 3) for k, v in d.items() if np.mean(v) > 0.05} for ph, d in kern.items()}
    print(json.dumps({"mode": os.environ.get("ZR_SCENE_UPDATE", "refit"), "background_rebuilds": list(r.scene.background_rebuild_stats()), "instance": int(idx), "instance_tris": int(sc.instance_num_tris[idx]),
                      "bvh": list(r.scene.bvh_info()), "update_ms": [round(x, 3) for x in upd], "update_ms_median": round(float(np.median(upd)), 3), "update_ms_mean": round(float(np.mean(upd[4:])), 3),
                      # ZR_BVH_GROUP (and every other A/B switch) is read by the EXPERIMENTS build only (libzetaray_amd_exp.so, ZR_EXP_ENV); the product library groups always
                      "library": os.path.basename(api.LIB_PATH),
                      "group": (os.environ.get("ZR_BVH_GROUP", "1") if os.path.basename(api.LIB_PATH) == "libzetaray_amd_exp.so" else "1 (product library: the ZR_BVH_GROUP switch exists in libzetaray_amd_exp.so only)"), "frame_ms_moving_series": [round(x, 2) for x in frames[n_static:]],
                      "frame_ms_static": round(float(np.median(frames[12:n_static])), 3), "frame_ms_moving": round(float(np.median(frames[n_static + 4:])), 3),
                      "kernel_ms_static": kms["static"], "kernel_ms_moving": kms["moving"]}))


def _stats(x):
    x = np.asarray(x, np.float64)
    return {"median": round(float(np.median(x)), 4), "p10": round(float(np.percentile(x, 10)), 4), "p90": round(float(np.percentile(x, 90)), 4)}


def device_records(num_emissive, frames, warmup):
    import ctypes as C
    import torch
    out = {"mode": "device_records", "frames": frames, "warmup": warmup, "library": os.path.basename(api.LIB_PATH), "sizes": []}
    L = scene_io._sceneio_lib()
    L.zrh_scene_data_begin_frame.argtypes = [C.c_void_p]
    L.zrh_scene_data_set_instance_world.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.zrh_scene_data_dirty_emissives.argtypes = [C.c_void_p] * 3
    L.zrh_scene_data_from_desc.argtypes = [C.c_void_p] * 3
    raw = {}      # unrounded host wall times, for the requirement below
    for ne in (num_emissive // 8, num_emissive):
        # the same total triangle count at both sizes (the clutter takes what the lights give up): the refit's kernel launches, one per tree level,
        # are host time of either path and would otherwise differ with the tree's depth, not with the light count
        sc = scene_io.make_synthetic_scene(num_tris=262144 + num_emissive - ne, num_emissive=ne, layout="atrium")
        light = [i for i in range(len(sc.instances)) if sc.instances["base_emissive_tri_offset"][i] != 0xFFFFFFFF][0]
        base = np.array(sc.instance_to_world[light], np.float32).reshape(3, 4)
        assert np.array_equal(base, np.eye(3, 4, dtype=np.float32)), "the light instance's records are object-space ones only under the identity"
        desc, init = sc.desc(), np.ascontiguousarray(sc.emissives.copy())
        h = C.c_void_p()
        assert L.zrh_scene_data_from_desc(C.addressof(desc), init.ctypes.data, C.byref(h)) == 0
        d = L.zrh_scene_data_desc(h).contents
        n = d.num_instances
        inst = np.ctypeslib.as_array(C.cast(d.instances, C.POINTER(C.c_uint8)), (n * wire.MESH_INSTANCE.itemsize,)).view(wire.MESH_INSTANCE)
        world = np.ctypeslib.as_array(C.cast(d.instance_to_world, C.POINTER(C.c_float)), (n, 12))
        ems = np.ctypeslib.as_array(C.cast(d.emissives, C.POINTER(C.c_uint8)), (ne * 48,)).view(wire.EMISSIVE_TRI)
        A, B = api.Scene(sc), api.Scene(sc)
        B.set_object_emissives(init)
        st = torch.cuda.Stream()
        idx = np.array([light], np.uint32)

        def matrix(k):
            a = 0.01 * k
            M = np.zeros((3, 4), np.float32)
            M[:, :3] = np.float32([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            M[:, 3] = np.float32([0.002 * k, 0.0, 0.001 * k])
            return M

        def host_frame(M):
            L.zrh_scene_data_begin_frame(h)
            L.zrh_scene_data_set_instance_world(h, light, M.ctypes.data)
            first, count = C.c_uint32(), C.c_uint32()
            L.zrh_scene_data_dirty_emissives(h, C.byref(first), C.byref(count))
            A.update_emissives(ems[first.value:first.value + count.value], first.value, stream=st.cuda_stream)
            A.update_instances(inst, world, stream=st.cuda_stream)

        def device_frame(M):
            B.move_instances(idx, M.reshape(1, 12), stream=st.cuda_stream)

        def static_frame(M):
            B.move_instances(idx[:0], M.reshape(1, 12)[:0], stream=st.cuda_stream)

        res = {"num_emissive": ne, "num_instances": int(n), "bvh": list(A.bvh_info())}
        for name, fn in (("host_path", host_frame), ("device_path", device_frame), ("device_path_nothing_moved", static_frame)):
            wall, stream_ms = [], []
            for k in range(1, warmup + frames + 1):
                M = matrix(k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                a = time.perf_counter()
                fn(M)
                b = time.perf_counter()
                e1.record(st)
                torch.cuda.synchronize()
                if k > warmup:
                    wall.append((b - a) * 1e3); stream_ms.append(e0.elapsed_time(e1))
            res[name] = {"host_wall_ms": _stats(wall), "stream_ms": _stats(stream_ms)}
            raw[(ne, name)] = np.asarray(wall, np.float64)
        res["host_wall_ratio_host_over_device"] = round(res["host_path"]["host_wall_ms"]["median"] / res["device_path"]["host_wall_ms"]["median"], 2)
        # k_mark_moved + k_move_emissives + the 52-byte copy: the device path's stream time over the same update with nothing moved.  k_move_instances
        # runs in both (every update rewrites the instance buffer), so its time stays inside device_path_nothing_moved's, next to the refit's
        res["mark_and_emissive_kernels_stream_ms"] = round(res["device_path"]["stream_ms"]["median"] - res["device_path_nothing_moved"]["stream_ms"]["median"], 4)
        same = (A.download_emissives().tobytes() == ems.tobytes())
        res["host_path_records_on_device"] = bool(same)
        out["sizes"].append(res)
        A.close(); B.close(); L.zrh_scene_data_destroy(h)
    # required: the device path's host time does not grow with the number of light triangles -- at the larger size it may exceed that at the
    # smaller by no more than the p10 - p90 spread of the smaller (unrounded values)
    small, large = raw[(num_emissive // 8, "device_path")], raw[(num_emissive, "device_path")]
    growth, spread = float(np.median(large) - np.median(small)), float(np.percentile(small, 90) - np.percentile(small, 10))
    out["device_host_wall_growth_ms"], out["small_p10_p90_spread_ms"], out["device_host_wall_flat"] = growth, spread, bool(growth <= spread)
    print(json.dumps(out))
    return 0 if out["device_host_wall_flat"] else 1


def _quad_scene(n_quads, clutter_tris, seed=3):
    """n_quads instances of one shared unit quad on a jittered grid (+ one static instance of clutter_tris small triangles)"""
    rng = np.random.default_rng(seed)
    sc = scene_io.Scene()
    sc.materials = np.array([scene_io.pack_material(metallic=0.0, roughness=0.3), scene_io.pack_material(base_color=(0.7, 0.6, 0.5, 1), roughness=0.6, double_sided=True)], wire.MATERIAL)
    quad = np.float32([[-0.5, 0, -0.5], [0.5, 0, -0.5], [0.5, 0, 0.5], [-0.5, 0, 0.5]]) * np.float32(0.02)
    P = [quad]
    I = [np.uint32([0, 1, 2, 0, 2, 3])]
    if clutter_tris:
        c = rng.uniform(-3, 3, (clutter_tris, 1, 3)).astype(np.float32)
        P.append((c + rng.uniform(-0.01, 0.01, (clutter_tris, 3, 3)).astype(np.float32)).reshape(-1, 3))
        I.append(np.arange(3 * clutter_tris, dtype=np.uint32))
    v = np.zeros(sum(len(p) for p in P), wire.VERTEX)
    v["pos"] = np.concatenate(P)
    v["normal"] = scene_io.encode_octahedral(np.tile(np.float32([0, 1, 0]), (len(v), 1)), sse_order=False)
    sc.vertices, sc.indices = v, np.concatenate(I)
    n = n_quads + (1 if clutter_tris else 0)
    side = int(np.ceil(np.sqrt(n_quads)))
    g = np.arange(n_quads)
    pos = np.stack([(g % side) * 0.03 - side * 0.015, rng.uniform(-1, 1, n_quads), (g // side) * 0.03 - side * 0.015], 1).astype(np.float32)
    xf = np.tile(np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), (n, 1))
    xf[:n_quads, 3], xf[:n_quads, 7], xf[:n_quads, 11] = pos[:, 0], pos[:, 1], pos[:, 2]
    inst = np.zeros(n, wire.MESH_INSTANCE)
    ident_q = np.rint((np.array([0, 0, 0, 1], np.float32) * np.float32(0.5) + np.float32(0.5)) * np.float32(65535.0)).astype(np.uint16)
    inst["rotation"] = inst["prev_rotation"] = ident_q
    inst["scale"] = inst["prev_scale"] = scene_io.f32_to_f16_bits([1, 1, 1])
    inst["translation"][:n_quads] = pos
    inst["mat_idx"], inst["base_emissive_tri_offset"], inst["base_color_tex"], inst["alpha_factor_cutoff"] = 1, 0xFFFFFFFF, 0xFFFF, 255 | (128 << 8)
    ntris = np.full(n, 2, np.uint32)
    if clutter_tris:
        inst["base_vtx_offset"][-1], inst["base_idx_offset"][-1], ntris[-1] = 4, 6, clutter_tris
    sc.instances, sc.instance_to_world, sc.instance_num_tris = inst, xf, ntris
    sc.instance_mask = np.full(n, wire.SUBGROUP_NON_EMISSIVE, np.uint8)
    sc.emissives = np.zeros(0, wire.EMISSIVE_TRI)
    sc.rho, sc.rho_dim = scene_io.load_rho_default()
    return sc, pos


def animate(n_small, frames, warmup):
    import ctypes as C
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bench
    out = {"mode": "animate", "frames": frames, "warmup": warmup, "library": os.path.basename(api.LIB_PATH), "device_state": bench.device_state(api, 0), "sizes": []}
    L = scene_io._sceneio_lib()
    vp = C.c_void_p
    L.zrh_scene_data_begin_frame.argtypes = [vp]
    L.zrh_scene_data_from_desc.argtypes = [vp] * 3
    L.zrh_scene_data_set_animation.argtypes = [vp, vp]
    L.zrh_scene_data_animate.argtypes = [vp, C.c_float]
    L.zrh_scene_data_set_device_records.argtypes = [vp, C.c_int]
    H = C.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "libzetaray_host.so"))
    H.zrh_scene_apply_updates_on.argtypes = [vp, vp, vp]
    n_large, raw = 16 * n_small, {}
    for nq in (n_small, n_large):
        sc, pos = _quad_scene(nq, 2 * (n_large - nq))
        rng = np.random.default_rng(9)
        nodes, keys = np.zeros(nq, wire.ANIM_NODE), np.zeros(2 * nq, wire.KEYFRAME)
        nodes["parent"], nodes["first_key"], nodes["num_keys"], nodes["loop"] = wire.ANIM_ROOT, 2 * np.arange(nq), 2, 1
        nodes["rest_scale"], nodes["rest_rotation"], nodes["rest_translation"], nodes["parent_world"] = 1, (0, 0, 0, 1), pos, np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
        q = rng.normal(size=(2 * nq, 4))
        keys["rotation"], keys["scale"], keys["time"] = q / np.linalg.norm(q, axis=1, keepdims=True), rng.uniform(0.8, 1.2, (2 * nq, 3)), np.tile(np.float32([0.0, 1.0]), nq)
        keys["translation"] = np.repeat(pos, 2, axis=0) + rng.uniform(-0.01, 0.01, (2 * nq, 3)).astype(np.float32)
        anim = wire.AnimDesc(nodes, keys, np.arange(nq), np.arange(nq))
        desc, ad = sc.desc(), anim.c_desc()
        h = vp()
        assert L.zrh_scene_data_from_desc(C.addressof(desc), None, C.byref(h)) == 0
        assert L.zrh_scene_data_set_animation(h, C.addressof(ad)) == 0, L.zrh_scene_io_last_error()
        L.zrh_scene_data_set_device_records(h, 1)
        A, B = api.Scene(sc), api.Scene(sc)
        B.set_animation(anim)
        st = torch.cuda.Stream()

        def host_samples(t):
            L.zrh_scene_data_begin_frame(h)
            assert L.zrh_scene_data_animate(h, t) == 0
            assert H.zrh_scene_apply_updates_on(A.h, h, st.cuda_stream) == 0

        def device_animates(t):
            B.animate(t, stream=st.cuda_stream)

        res = {"animated_instances": nq, "num_instances": len(sc.instances), "num_tris": int(sc.num_tris), "bvh": list(A.bvh_info())}
        for name, fn in (("A_host_samples_then_move_instances", host_samples), ("B_scene_animate", device_animates)):
            wall, stream_ms = [], []
            for k in range(1, warmup + frames + 1):
                t = 0.013 * k
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                a = time.perf_counter()
                fn(t)
                b = time.perf_counter()
                e1.record(st)
                torch.cuda.synchronize()
                if k > warmup:
                    wall.append((b - a) * 1e3); stream_ms.append(e0.elapsed_time(e1))
            res[name] = {"host_wall_ms": _stats(wall), "stream_ms": _stats(stream_ms)}
            raw[(nq, name)] = (np.asarray(wall, np.float64), np.asarray(stream_ms, np.float64))
        ia, xa = A.download_instances(0)
        ib, xb = B.download_instances(0)
        res["same_device_bytes"] = bool(ia.tobytes() == ib.tobytes() and xa.tobytes() == xb.tobytes())
        res["host_wall_ratio_A_over_B"] = round(res["A_host_samples_then_move_instances"]["host_wall_ms"]["median"] / res["B_scene_animate"]["host_wall_ms"]["median"], 2)
        out["sizes"].append(res)
        A.close(); B.close(); L.zrh_scene_data_destroy(h)
    small, large = raw[(n_small, "B_scene_animate")][0], raw[(n_large, "B_scene_animate")][0]
    growth, spread = float(np.median(large) - np.median(small)), float(np.percentile(small, 90) - np.percentile(small, 10))
    out["B_host_wall_growth_ms"], out["small_p10_p90_spread_ms"], out["B_host_wall_flat"] = growth, spread, bool(growth <= spread)
    out["B_stream_not_longer_than_A"] = [bool(np.median(raw[(nq, "B_scene_animate")][1]) <= np.median(raw[(nq, "A_host_samples_then_move_instances")][1])) for nq in (n_small, n_large)]
    out["B_faster_than_A_on_the_host_at_small_n"] = bool(np.median(small) < np.median(raw[(n_small, "A_host_samples_then_move_instances")][0]))
    ok = out["B_host_wall_flat"] and all(out["B_stream_not_longer_than_A"]) and all(r["same_device_bytes"] for r in out["sizes"])
    print(json.dumps(out))
    return 0 if ok else 1


def _tube_scene(n_verts, clutter_tris, segs=64):
    """one instance: a tube of n_verts vertices (segs per ring) up the y axis, identity world matrix (+ one static instance of clutter_tris small triangles)"""
    rng = np.random.default_rng(5)
    rings = n_verts // segs
    assert rings * segs == n_verts and rings >= 2
    ring, seg = np.divmod(np.arange(n_verts), segs)
    a = 2 * np.pi * seg / segs
    v = np.zeros(n_verts + 3 * clutter_tris, wire.VERTEX)
    v["pos"][:n_verts] = np.stack([0.2 * np.cos(a), 4.0 * ring / (rings - 1) - 2.0, 0.2 * np.sin(a)], 1).astype(np.float32)
    nrm = np.tile(np.float32([0, 1, 0]), (len(v), 1))
    nrm[:n_verts] = np.stack([np.cos(a), np.zeros(n_verts), np.sin(a)], 1)
    v["normal"] = scene_io.encode_octahedral(nrm, sse_order=False)
    v["tangent"] = scene_io.encode_octahedral(np.tile(np.float32([0, 1, 0]), (len(v), 1)), sse_order=False)
    p = (ring[:-segs] * segs + seg[:-segs]).astype(np.uint32)
    q = (ring[:-segs] * segs + (seg[:-segs] + 1) % segs).astype(np.uint32)
    idx = [np.stack([p, q, p + segs, q, q + segs, p + segs], 1).reshape(-1).astype(np.uint32)]
    if clutter_tris:
        c = rng.uniform(-3, 3, (clutter_tris, 1, 3)).astype(np.float32) + np.float32([6, 0, 0])
        v["pos"][n_verts:] = (c + rng.uniform(-0.01, 0.01, (clutter_tris, 3, 3)).astype(np.float32)).reshape(-1, 3)
        idx.append(np.arange(3 * clutter_tris, dtype=np.uint32))
    sc = scene_io.Scene()
    sc.materials = np.array([scene_io.pack_material(base_color=(0.7, 0.6, 0.5, 1), roughness=0.6, double_sided=True)], wire.MATERIAL)
    sc.vertices, sc.indices = v, np.concatenate(idx)
    n = 2 if clutter_tris else 1
    inst = np.zeros(n, wire.MESH_INSTANCE)
    inst["rotation"] = inst["prev_rotation"] = np.rint((np.array([0, 0, 0, 1], np.float32) * np.float32(0.5) + np.float32(0.5)) * np.float32(65535.0)).astype(np.uint16)
    inst["scale"] = inst["prev_scale"] = scene_io.f32_to_f16_bits([1, 1, 1])
    inst["base_emissive_tri_offset"], inst["base_color_tex"], inst["alpha_factor_cutoff"] = 0xFFFFFFFF, 0xFFFF, 255 | (128 << 8)
    ntris = np.uint32([len(idx[0]) // 3] + ([clutter_tris] if clutter_tris else []))
    if clutter_tris:
        inst["base_vtx_offset"][1], inst["base_idx_offset"][1] = n_verts, len(idx[0])
    sc.instances, sc.instance_to_world, sc.instance_num_tris = inst, np.tile(np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), (n, 1)), ntris
    sc.instance_mask = np.full(n, wire.SUBGROUP_NON_EMISSIVE, np.uint8)
    sc.emissives = np.zeros(0, wire.EMISSIVE_TRI)
    sc.rho, sc.rho_dim = scene_io.load_rho_default()
    return sc


def _tube_skin(sc, n_verts, nj=64):
    """nj joints up the tube, each a root node of its own with three keys (a small turn about z, a translation); a vertex hangs on the four joints around
    its height.  Inverse bind matrices: the joints' translations at rest, negated"""
    rng = np.random.default_rng(6)
    nodes, keys = np.zeros(nj, wire.ANIM_NODE), np.zeros(3 * nj, wire.KEYFRAME)
    jy = (4.0 * (np.arange(nj) + 0.5) / nj - 2.0).astype(np.float32)
    nodes["parent"], nodes["first_key"], nodes["num_keys"], nodes["loop"] = wire.ANIM_ROOT, 3 * np.arange(nj), 3, 1
    nodes["rest_scale"], nodes["rest_rotation"], nodes["parent_world"] = 1, (0, 0, 0, 1), np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    nodes["rest_translation"][:, 1] = jy
    ang = rng.uniform(-0.2, 0.2, 3 * nj)
    keys["rotation"] = np.stack([np.zeros(3 * nj), np.zeros(3 * nj), np.sin(ang / 2), np.cos(ang / 2)], 1)
    keys["scale"], keys["time"] = 1, np.tile(np.float32([0.0, 0.5, 1.0]), nj)
    keys["translation"][:, 1] = np.repeat(jy, 3)
    keys["translation"][:, 0] = rng.uniform(-0.05, 0.05, 3 * nj)
    anim = wire.AnimDesc(nodes, keys, [], [])
    joints = np.zeros(nj, wire.SKIN_JOINT)
    joints["node"], joints["inverse_bind"] = np.arange(nj), np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    joints["inverse_bind"][:, 7] = -jy
    h = (sc.vertices["pos"][:n_verts, 1].astype(np.float64) + 2.0) / 4.0 * nj - 0.5
    j0 = np.clip(np.floor(h), 0, nj - 1).astype(np.int64)
    fr = np.clip(h - j0, 0, 1)
    f = np.zeros(n_verts, wire.SKIN_INFLUENCE)
    f["joint"] = np.stack([j0, np.minimum(j0 + 1, nj - 1), np.maximum(j0 - 1, 0), np.minimum(j0 + 2, nj - 1)], 1)
    w = np.stack([1 - fr, fr, np.full(n_verts, 0.05), np.full(n_verts, 0.05)], 1).astype(np.float32)
    f["weight"] = w / w.sum(1, dtype=np.float32, keepdims=True)
    return anim, wire.SkinDesc(joints, np.array([(0, n_verts, 0)], wire.SKIN_RANGE), f)


def skin(n_small, frames, warmup):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bench
    out = {"mode": "skin", "frames": frames, "warmup": warmup, "library": os.path.basename(api.LIB_PATH), "device_state": bench.device_state(api, 0), "joints": 64, "sizes": []}
    n_large, raw = 16 * n_small, {}
    for nv in (n_small, n_large):
        sc = _tube_scene(nv, 2 * (n_large - nv))
        anim, sk = _tube_skin(sc, nv)
        rest = sc.vertices[:nv].copy()
        A, B, Cn = api.Scene(sc), api.Scene(sc), api.Scene(sc)
        B.set_animation(anim); B.set_skinning(sk)
        Cn.set_animation(anim)
        st = torch.cuda.Stream()

        def host_form(t):
            A.update_vertices(0, scene_io.skin_pose(anim, sk, rest, t), stream=st.cuda_stream)
            A.update_instances(sc.instances, sc.instance_to_world, stream=st.cuda_stream)

        def device_form(t):
            B.animate(t, stream=st.cuda_stream)

        def without_skin(t):
            Cn.animate(t, stream=st.cuda_stream)

        res = {"skinned_vertices": nv, "num_tris": int(sc.num_tris), "bvh": list(A.bvh_info())}
        for name, fn in (("A_host_form", host_form), ("B_scene_animate", device_form), ("C_animate_without_skin", without_skin)):
            wall, stream_ms = [], []
            for k in range(1, warmup + frames + 1):
                t = 0.013 * k
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                a = time.perf_counter()
                fn(t)
                b = time.perf_counter()
                e1.record(st)
                torch.cuda.synchronize()
                if k > warmup:
                    wall.append((b - a) * 1e3); stream_ms.append(e0.elapsed_time(e1))
            res[name] = {"host_wall_ms": _stats(wall), "stream_ms": _stats(stream_ms)}
            raw[(nv, name)] = (np.asarray(wall, np.float64), np.asarray(stream_ms, np.float64))
        res["same_device_bytes"] = bool(A.download_vertices().tobytes() == B.download_vertices().tobytes())
        kern_ms = res["B_scene_animate"]["stream_ms"]["median"] - res["C_animate_without_skin"]["stream_ms"]["median"]
        moved = nv * (28 + 24 + 28 + 16) + 64 * (4 + 48 + 48 + 48)
        res["skin_kernels_stream_ms"] = round(kern_ms, 4)
        res["skin_kernels_bytes"] = int(moved)
        res["skin_kernels_gb_per_s"] = round(moved / (kern_ms * 1e-3) / 1e9, 1) if kern_ms > 0 else None
        res["host_wall_ratio_A_over_B"] = round(res["A_host_form"]["host_wall_ms"]["median"] / res["B_scene_animate"]["host_wall_ms"]["median"], 2)
        out["sizes"].append(res)
        A.close(); B.close(); Cn.close()
    small, large = raw[(n_small, "B_scene_animate")][0], raw[(n_large, "B_scene_animate")][0]
    growth, spread = float(np.median(large) - np.median(small)), float(np.percentile(small, 90) - np.percentile(small, 10))
    out["B_host_wall_growth_ms"], out["small_p10_p90_spread_ms"], out["B_host_wall_flat"] = growth, spread, bool(growth <= spread)
    out["B_stream_not_longer_than_A"] = [bool(np.median(raw[(nv, "B_scene_animate")][1]) <= np.median(raw[(nv, "A_host_form")][1])) for nv in (n_small, n_large)]
    ok = out["B_host_wall_flat"] and all(out["B_stream_not_longer_than_A"]) and all(r["same_device_bytes"] for r in out["sizes"])
    print(json.dumps(out))
    return 0 if ok else 1


def _tube_morph(n_verts, applied, num_targets=8):
    """one node that moves nothing (an animation to set), and a morph set over the tube: num_targets targets with POSITION and NORMAL deltas under one looping
    track of 3 keys whose first `applied` targets have non-zero weights at every time, the others exact zeros"""
    rng = np.random.default_rng(7)
    nodes, keys = np.zeros(1, wire.ANIM_NODE), np.zeros(2, wire.KEYFRAME)
    nodes["parent"], nodes["num_keys"], nodes["loop"] = wire.ANIM_ROOT, 2, 1
    nodes["rest_scale"], nodes["rest_rotation"], nodes["parent_world"] = 1, (0, 0, 0, 1), np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    keys["rotation"], keys["scale"], keys["time"] = (0, 0, 0, 1), 1, np.float32([0.0, 1.0])
    anim = wire.AnimDesc(nodes, keys, [], [])
    values = rng.uniform(0.1, 1.0, (3, num_targets)).astype(np.float32)
    values[:, applied:] = 0.0
    track = np.zeros(1, wire.MORPH_TRACK)
    track["num_targets"], track["num_keys"], track["loop"] = num_targets, 3, 1
    targets = np.zeros(num_targets, wire.MORPH_TARGET)
    targets["first_pos"], targets["first_nrm"], targets["first_tan"] = 2 * n_verts * np.arange(num_targets), 2 * n_verts * np.arange(num_targets) + n_verts, wire.MORPH_NONE
    deltas = rng.uniform(-0.02, 0.02, (2 * num_targets * n_verts, 3)).astype(np.float32)
    return anim, wire.MorphDesc(track, targets, np.array([(0, n_verts, 0, num_targets, 0)], wire.MORPH_RANGE), np.float32([0.0, 0.5, 1.0]), values, np.zeros(num_targets, np.float32), deltas)


def morph(n_small, frames, warmup):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bench
    out = {"mode": "morph", "frames": frames, "warmup": warmup, "library": os.path.basename(api.LIB_PATH), "device_state": bench.device_state(api, 0), "targets": 8, "sizes": []}
    n_large, raw = 16 * n_small, {}
    for nv in (n_small, n_large):
        sc = _tube_scene(nv, 2 * (n_large - nv))
        anim, m8 = _tube_morph(nv, 8)
        _, m1 = _tube_morph(nv, 1)
        rest = sc.vertices[:nv].copy()
        A, B8, B1, Cn = api.Scene(sc), api.Scene(sc), api.Scene(sc), api.Scene(sc)
        for S, m in ((B8, m8), (B1, m1)):
            S.set_animation(anim); S.set_morph(m)
        Cn.set_animation(anim)
        st = torch.cuda.Stream()

        def host_form(t):
            A.update_vertices(0, scene_io.morph_pose(anim, None, m8, rest, t), stream=st.cuda_stream)
            A.update_instances(sc.instances, sc.instance_to_world, stream=st.cuda_stream)

        res = {"morphed_vertices": nv, "num_tris": int(sc.num_tris), "bvh": list(A.bvh_info())}
        for name, fn in (("A_host_form", host_form), ("B_scene_animate_8_of_8", lambda t: B8.animate(t, stream=st.cuda_stream)),
                         ("B_scene_animate_1_of_8", lambda t: B1.animate(t, stream=st.cuda_stream)), ("C_animate_without_morph", lambda t: Cn.animate(t, stream=st.cuda_stream))):
            wall, stream_ms = [], []
            for k in range(1, warmup + frames + 1):
                t = 0.013 * k
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                a = time.perf_counter()
                fn(t)
                b = time.perf_counter()
                e1.record(st)
                torch.cuda.synchronize()
                if k > warmup:
                    wall.append((b - a) * 1e3); stream_ms.append(e0.elapsed_time(e1))
            res[name] = {"host_wall_ms": _stats(wall), "stream_ms": _stats(stream_ms)}
            raw[(nv, name)] = (np.asarray(wall, np.float64), np.asarray(stream_ms, np.float64))
        res["same_device_bytes"] = bool(A.download_vertices().tobytes() == B8.download_vertices().tobytes())
        for name, applied in (("8_of_8", 8), ("1_of_8", 1)):
            kern_ms = res["B_scene_animate_" + name]["stream_ms"]["median"] - res["C_animate_without_morph"]["stream_ms"]["median"]
            moved = nv * (28 + 28 + 16 + 24 * applied)
            res["morph_kernels_stream_ms_" + name] = round(kern_ms, 4)
            res["morph_kernels_bytes_" + name] = int(moved)
            res["morph_kernels_gb_per_s_" + name] = round(moved / (kern_ms * 1e-3) / 1e9, 1) if kern_ms > 0 else None
        res["host_wall_ratio_A_over_B"] = round(res["A_host_form"]["host_wall_ms"]["median"] / res["B_scene_animate_8_of_8"]["host_wall_ms"]["median"], 2)
        out["sizes"].append(res)
        A.close(); B8.close(); B1.close(); Cn.close()
    small, large = raw[(n_small, "B_scene_animate_8_of_8")][0], raw[(n_large, "B_scene_animate_8_of_8")][0]
    growth, spread = float(np.median(large) - np.median(small)), float(np.percentile(small, 90) - np.percentile(small, 10))
    out["B_host_wall_growth_ms"], out["small_p10_p90_spread_ms"], out["B_host_wall_flat"] = growth, spread, bool(growth <= spread)
    ok = out["B_host_wall_flat"] and all(r["same_device_bytes"] for r in out["sizes"])
    print(json.dumps(out))
    return 0 if ok else 1


def _lit_tube(api_mod, sc, nv):
    """the tube of _tube_scene with an emissive material: one light triangle per tube triangle.  The records are made by the library itself -- records whose
    non-geometric fields are set and whose geometry is not go to a throw-away scene, whose range form derives both records of every triangle at rest"""
    lit = scene_io.Scene()
    for name in ("vertices", "indices", "instance_to_world", "instance_num_tris", "rho", "rho_dim"):
        setattr(lit, name, getattr(sc, name))
    lit.materials = np.concatenate([sc.materials, np.array([scene_io.pack_material(base_color=(0.8, 0.8, 0.8, 1), roughness=1.0, double_sided=True,
                                                                                     emissive_factor=(1.0, 0.85, 0.7), emissive_strength=5.0)], wire.MATERIAL)])
    lit.instances, lit.instance_mask = sc.instances.copy(), sc.instance_mask.copy()
    n = int(sc.instance_num_tris[0])
    lit.instances["mat_idx"][0], lit.instances["base_emissive_tri_offset"][0], lit.instance_mask[0] = 1, 0, wire.SUBGROUP_EMISSIVE
    one = scene_io.pack_emissive_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0], [(0, 0), (1, 0), (0, 1)], 0xB3D9FF, 0xFFFF, int(scene_io.f32_to_f16_bits([5.0])[0]), 0, True)
    rec = np.repeat(np.array([one], wire.EMISSIVE_TRI), n)
    rec["id"] = (np.arange(1, n + 1, dtype=np.uint64) * 0x9E3779B1 & 0xFFFFFFFF).astype(np.uint32)
    lit.emissives = lit.emissives_initial = rec
    S = api_mod.Scene(lit)
    S.set_object_emissives(rec)
    S.refresh_emissives(0, n)
    lit.emissives, lit.emissives_initial = S.download_emissives(), S.download_object_emissives()
    lit._desc = None
    S.close()
    return lit


def lights(n_small, frames, warmup):
    """--lights: the --skin tube with an emissive material, so every tube triangle is a light the pose deforms (about 2 N lights)"""
    import ctypes as C
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bench
    out = {"mode": "lights", "frames": frames, "warmup": warmup, "library": os.path.basename(api.LIB_PATH), "device_state": bench.device_state(api, 0), "joints": 64, "sizes": []}
    L = scene_io._sceneio_lib()
    vp = C.c_void_p
    L.zrh_scene_data_from_desc.argtypes = [vp] * 3
    L.zrh_scene_data_begin_frame.argtypes = [vp]
    L.zrh_scene_data_refresh_emissives.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.zrh_scene_data_dirty_emissives.argtypes = [vp] * 3
    n_large, raw = 16 * n_small, {}
    for nv in (n_small, n_large):
        plain = _tube_scene(nv, 2 * (n_large - nv))
        anim, sk = _tube_skin(plain, nv)
        lit = _lit_tube(api, plain, nv)
        nl = len(lit.emissives)
        rest = lit.vertices[:nv].copy()
        A, B, Cn = api.Scene(lit), api.Scene(lit), api.Scene(plain)
        B.set_object_emissives(lit.emissives_initial)
        B.set_animation(anim); B.set_skinning(sk)
        Cn.set_animation(anim); Cn.set_skinning(sk)
        desc, init = lit.desc(), np.ascontiguousarray(lit.emissives_initial.copy())
        h = vp()
        assert L.zrh_scene_data_from_desc(C.addressof(desc), init.ctypes.data, C.byref(h)) == 0, L.zrh_scene_io_last_error()
        d = L.zrh_scene_data_desc(h).contents
        ems = np.ctypeslib.as_array(C.cast(d.emissives, C.POINTER(C.c_uint8)), (nl * 48,)).view(wire.EMISSIVE_TRI)
        posed_all = lit.vertices.copy()
        st = torch.cuda.Stream()

        def host_form(t):
            posed_all[:nv] = scene_io.skin_pose(anim, sk, rest, t)
            A.update_vertices(0, posed_all[:nv], stream=st.cuda_stream)
            L.zrh_scene_data_begin_frame(h)
            assert L.zrh_scene_data_refresh_emissives(h, posed_all.ctypes.data, 0, nl) == 0
            f, c = C.c_uint32(), C.c_uint32()
            L.zrh_scene_data_dirty_emissives(h, C.byref(f), C.byref(c))
            A.update_emissives(ems[f.value:f.value + c.value], f.value, stream=st.cuda_stream)
            A.update_instances(lit.instances, lit.instance_to_world, stream=st.cuda_stream)

        def device_form(t):
            B.animate(t, stream=st.cuda_stream)

        def not_emissive(t):
            Cn.animate(t, stream=st.cuda_stream)

        res = {"skinned_vertices": nv, "light_triangles": nl, "num_tris": int(lit.num_tris)}
        for name, fn in (("A_host_form", host_form), ("B_scene_animate", device_form), ("C_animate_not_emissive", not_emissive)):
            wall, stream_ms = [], []
            for k in range(1, warmup + frames + 1):
                t = 0.013 * k
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                a = time.perf_counter()
                fn(t)
                b = time.perf_counter()
                e1.record(st)
                torch.cuda.synchronize()
                if k > warmup:
                    wall.append((b - a) * 1e3); stream_ms.append(e0.elapsed_time(e1))
            res[name] = {"host_wall_ms": _stats(wall), "stream_ms": _stats(stream_ms)}
            raw[(nv, name)] = (np.asarray(wall, np.float64), np.asarray(stream_ms, np.float64))
        res["same_device_bytes"] = bool(A.download_vertices().tobytes() == B.download_vertices().tobytes() and A.download_emissives().tobytes() == B.download_emissives().tobytes())
        bs, cs = raw[(nv, "B_scene_animate")][1], raw[(nv, "C_animate_not_emissive")][1]
        kern_ms = float(np.median(bs) - np.median(cs))
        drift = float(max(np.percentile(bs, 90) - np.percentile(bs, 10), np.percentile(cs, 90) - np.percentile(cs, 10)))
        # per light: the 16-byte entry, the owner word, three 12-byte positions, the 48-byte object record read, two 48-byte records written (the owner's
        # 48-byte matrix row is one line for every lane here and is not counted)
        moved = nl * (16 + 4 + 36 + 48 + 96)
        res["refresh_kernel_stream_ms"], res["stream_p10_p90_drift_ms"] = round(kern_ms, 4), round(drift, 4)
        res["refresh_kernel_within_drift"] = bool(kern_ms <= drift)
        res["refresh_kernel_bytes"], res["bytes_per_light"] = int(moved), 200
        res["refresh_kernel_gb_per_s"] = None if kern_ms <= drift else round(moved / (kern_ms * 1e-3) / 1e9, 1)
        res["host_wall_ratio_A_over_B"] = round(res["A_host_form"]["host_wall_ms"]["median"] / res["B_scene_animate"]["host_wall_ms"]["median"], 2)
        out["sizes"].append(res)
        A.close(); B.close(); Cn.close()
        L.zrh_scene_data_destroy(h)
    small, large = raw[(n_small, "B_scene_animate")][0], raw[(n_large, "B_scene_animate")][0]
    growth, spread = float(np.median(large) - np.median(small)), float(np.percentile(small, 90) - np.percentile(small, 10))
    out["B_host_wall_growth_ms"], out["small_p10_p90_spread_ms"], out["B_host_wall_flat"] = growth, spread, bool(growth <= spread)
    out["B_stream_below_A"] = [bool(np.median(raw[(nv, "B_scene_animate")][1]) < np.median(raw[(nv, "A_host_form")][1])) for nv in (n_small, n_large)]
    out["not_measured"] = "hardware counters; several ranges (one launch per range of the pose kernel; the light kernel is one launch however many ranges)"
    ok = all(r["same_device_bytes"] for r in out["sizes"])
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-records", action="store_true")
    ap.add_argument("--animate", action="store_true")
    ap.add_argument("--skin", action="store_true")
    ap.add_argument("--morph", action="store_true")
    ap.add_argument("--lights", action="store_true")
    ap.add_argument("--vertices", type=int, default=65536)
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--emissive", type=int, default=100000)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    a = ap.parse_args()
    if a.lights:
        sys.exit(lights(a.vertices, max(a.frames, 64), max(a.warmup, 16)))
    elif a.morph:
        sys.exit(morph(a.vertices, max(a.frames, 64), max(a.warmup, 16)))
    elif a.skin:
        sys.exit(skin(a.vertices, max(a.frames, 64), max(a.warmup, 16)))
    elif a.animate:
        sys.exit(animate(a.instances, max(a.frames, 64), max(a.warmup, 16)))
    elif a.device_records:
        sys.exit(device_records(a.emissive, max(a.frames, 64), max(a.warmup, 16)))
    else:
        main()
