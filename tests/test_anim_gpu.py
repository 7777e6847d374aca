"""zr_scene_set_animation / zr_scene_animate: keyframe animation sampled, composed down the hierarchy and applied on the device (zr_tu_anim.hip), against
the host path -- zrh_scene_data_begin_frame / zrh_scene_data_animate (include/zr_anim.h on the host), then zr_scene_update_emissives +
zr_scene_update_instances -- byte for byte: device buffers, rendered frames, the readers of the host copies, across streams, the calls it refuses, and
frames moved by hand in between."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests.animmath import cases
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RPT_PLANES = ("A", "B", "C", "D", "E", "F", "G", "neighbor", "map_ctn", "map_ntc")
W, H = 96, 64


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    path, trs = cases.write_scene(tmp_path_factory.mktemp("anim_gpu"))
    sc, _ = scene_io.load_gltf_native(path)
    assert len(sc.instances) == cases.NUM_INSTANCES
    return path, trs, sc


def _assert_buffers(B, A, host, what):
    for which in (0, 1):
        ib, xb = B.download_instances(which)
        ia, xa = A.download_instances(which)
        assert ib.tobytes() == ia.tobytes(), f"{what}: instance buffer {which} differs from the host path's"
        assert xb.tobytes() == xa.tobytes(), f"{what}: toWorld differs from the host path's"
    ib, xb = B.download_instances(0)
    assert ib.tobytes() == host.inst.tobytes(), f"{what}: current records differ from zrh_scene_data's"
    assert xb.tobytes() == host.world.tobytes(), f"{what}: toWorld differs from zrh_scene_data's"
    eb = B.download_emissives()
    assert eb.tobytes() == A.download_emissives().tobytes(), f"{what}: emissive records differ from the host path's"
    assert eb.tobytes() == host.ems.tobytes(), f"{what}: emissive records differ from zrh_scene_data's"


@pytest.mark.parametrize("n_animated", [1, 63, 65, 257])
def test_every_buffer_equals_the_host_path(api, scene, n_animated):
    """check 1: twin scenes, A through the host path, B through Scene.animate, at the six times of tests/animmath/cases.py (before the first keys, on
    keys, between keys, on last keys, beyond them with and without loop, t0 != 0 among the nodes).  1 / 63 / 65 / 257 animated nodes: lanes end inside
    a wave, at a wave boundary and across a block; from 65 on with the three-level hierarchy; the lights carry 1, 63 and 130 triangles"""
    path, trs, sc = scene
    desc = cases.animation(trs, n_animated)
    host = cases.HostData.from_gltf(path)
    assert host.set_animation(desc) == 0
    A, B = api.Scene(sc), api.Scene(sc)
    B.set_object_emissives(host.init)
    B.set_animation(desc)
    before = B.download_emissives()
    v0 = B.version
    for t in cases.TIMES:
        host.apply(A, t)
        B.animate(t)
        assert B.instances_in_motion
        _assert_buffers(B, A, host, f"{n_animated} animated nodes, t = {t}")
    assert B.version == v0 + len(cases.TIMES)
    assert not np.array_equal(before.view(np.uint8), B.download_emissives().view(np.uint8))
    A.close(); B.close(); host.close()


def test_mixing_with_a_frame_moved_by_hand(api, scene):
    """check 6: a move_instances frame between two animate frames, moving an instance the animation does not list, one frame later one it does, and later a hand-moved frame in which nothing moves"""
    path, trs, sc = scene
    desc = cases.animation(trs, 65)
    host = cases.HostData.from_gltf(path)
    assert host.set_animation(desc) == 0
    A, B = api.Scene(sc), api.Scene(sc)
    B.set_object_emissives(host.init)
    B.set_animation(desc)
    M = np.float32([[0.9, 0, 0.1, 0.4], [0, 1.1, 0, 0.9], [-0.1, 0, 0.9, 0.2]])
    listed = int(desc.instance_idx[4])
    for f, (t, moved) in enumerate([(0.5, None), (None, [(0, M)]), (0.8125, None), (None, [(listed, M)]), (1.25, None), (None, []), (2.125, None)], 1):
        if t is not None:
            host.apply(A, t); B.animate(t)
        else:
            host.apply(A, None, moved); B.move_instances([i for i, _ in moved], [m.reshape(12) for _, m in moved])
        _assert_buffers(B, A, host, f"frame {f}")
    A.close(); B.close(); host.close()


def test_refusals_change_nothing(api, scene):
    """check 5: animate before set_animation; a setter refusal after a valid set (an invalid table, and lights before their object-space records)
    leaves the old animation running"""
    path, trs, sc = scene
    host = cases.HostData.from_gltf(path)
    A, B = api.Scene(sc), api.Scene(sc)

    def state():
        return [B.download_instances(0), B.download_instances(1), B.download_emissives()]

    def same(a, b):
        return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for p, q in zip(a[:2], b[:2]) for x, y in zip(p, q)) and a[2].tobytes() == b[2].tobytes()

    s0, py0 = state(), (B.version, B.instances_in_motion)
    with pytest.raises(api.ZetaRayError) as e:
        B.animate(0.5)
    assert e.value.code == 6 and "zr_scene_set_animation" in str(e.value) and same(s0, state()) and (B.version, B.instances_in_motion) == py0
    with pytest.raises(api.ZetaRayError) as e:       # the lights before their object-space records were handed over
        B.set_animation(cases.animation(trs, 63))
    assert e.value.code == 6 and "zr_scene_set_object_emissives" in str(e.value) and same(s0, state())
    with pytest.raises(api.ZetaRayError) as e:
        B.animate(0.5)
    assert e.value.code == 6
    B.set_object_emissives(host.init)
    good = cases.animation(trs, 65)
    assert host.set_animation(good) == 0
    B.set_animation(good)
    host.apply(A, 0.5); B.animate(0.5)
    _assert_buffers(B, A, host, "first valid frame")
    s1 = state()
    bad = cases.animation(trs, 63)
    bad.keys["time"][1] = bad.keys["time"][0]
    bad2 = cases.animation(trs, 63)
    bad2.instance_idx[1] = cases.NUM_INSTANCES
    for d, word in ((bad, "strictly increasing"), (bad2, f"instance {cases.NUM_INSTANCES}")):
        with pytest.raises(api.ZetaRayError) as e:
            B.set_animation(d)
        assert e.value.code == 1 and word in str(e.value), str(e.value)
        assert same(s1, state())
    host.apply(A, 1.25); B.animate(1.25)      # the old animation is still the one that runs
    _assert_buffers(B, A, host, "valid frame after the refusals")
    B.set_animation(None)
    with pytest.raises(api.ZetaRayError) as e:
        B.animate(2.0)
    assert e.value.code == 6
    A.close(); B.close(); host.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from zetaray_amd import api, scene_io, wire
sc, _ = scene_io.load_gltf_native(sys.argv[2])
s = api.Scene(sc)
n = np.zeros(1, wire.ANIM_NODE); k = np.zeros(2, wire.KEYFRAME)
n["parent"], n["num_keys"], n["rest_scale"], n["rest_rotation"] = wire.ANIM_ROOT, 2, 1, (0, 0, 0, 1)
n["parent_world"] = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
k["scale"], k["rotation"], k["time"], k["translation"] = 1, (0, 0, 0, 1), (0, 1), ((0, 0, 0), (1, 0, 0))
s.set_animation(wire.AnimDesc(n, k, [0], [0]))
before = s.download_instances(0)[0].tobytes()
try:
    s.animate(0.5)
    print("NOT REFUSED")
except api.ZetaRayError as e:
    print("refused", e.code, "unchanged" if s.download_instances(0)[0].tobytes() == before else "CHANGED", str(e))
"""


def test_rebuild_mode_is_refused(api, scene):
    """check 5, the host-synchronous update mode: ZR_SCENE_UPDATE set for a fresh child process, not for this one"""
    path, _, _ = scene
    env = dict(os.environ, ZR_SCENE_UPDATE="rebuild")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("refused 5 unchanged") and "rebuild" in out.stdout, out.stdout


def test_background_sah_rebuild_under_animate(api, scene):
    """check 3, the builder's snapshot of the host matrices: zr_scene_set_background_rebuild on B only; the scene animates until a background tree has
    been installed -- G-buffer planes and the path-traced image stay A's, and B's buffers the host path's.  No install within 40 frames fails the test"""
    path, trs, sc = scene
    desc = cases.animation(trs, 65)
    host = cases.HostData.from_gltf(path)
    assert host.set_animation(desc) == 0
    prm = wire.default_params()
    ra, rb = api.Renderer(sc, W, H, params=prm), api.Renderer(sc, W, H, params=prm)
    assert rb.scene.bvh_info()[0] > 0
    rb.scene.set_background_rebuild(True)
    rb.scene.set_object_emissives(host.init)
    rb.set_animation(desc)
    prev, installed, f = None, 0, 0
    while installed < 1 and f < 40:
        f += 1
        t = 0.11 * f
        host.apply(ra.scene, t)
        rb.animate(t)
        t0 = time.perf_counter()
        while rb.scene.background_rebuild_stats()[2] == 1 and time.perf_counter() - t0 < 20.0:      # (the builder's thread: a deterministic schedule)
            time.sleep(0.002)
        cb = scene_io.make_frame_constants(W, H, frame_num=f, num_emissives=len(sc.emissives), cam_pos=(0.0, 1.0, -4.0))
        if prev is not None:
            cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
        prev = cb.copy()
        ra.render_frame(cb); rb.render_frame(cb)
        pa, pb = ra.gbuffer.download()[0], rb.gbuffer.download()[0]
        for nm, a, b in zip(wire.GB_PLANE_NAMES, pa, pb):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), f"frame {f}: G-buffer plane {nm}"
        assert ra.final().tobytes() == rb.final().tobytes(), f"frame {f}: FINAL"
        _assert_buffers(rb.scene, ra.scene, host, f"frame {f}")
        installed = rb.scene.background_rebuild_stats()[1]
    assert installed >= 1, f"no background tree installed within {f} frames: {rb.scene.background_rebuild_stats()}"
    host.close()


# ---------------------------------------------------------------------------------------------------------------- the animated Cornell box (the loader's fixture)
@pytest.fixture(scope="module")
def cornell(tmp_path_factory):
    """tests/golden/cornell_gltf/cornell_animated.gltf through load_gltf_native: (path, scene with sc.animation, texture-table offsets); the light
    translates, the short box turns, the tall box hangs on an animated parent"""
    path = cases.cornell_animated(tmp_path_factory.mktemp("cornell_anim"))
    sc, offs = scene_io.load_gltf_native(path)
    assert sc.animation is not None and len(sc.animation.instance_idx) == 3
    return path, sc, offs


def _cb(sc, offs, f, prev):
    cb = scene_io.make_frame_constants(W, H, frame_num=f, num_emissives=len(sc.emissives))
    scene_io.set_texture_heap_offsets(cb, offs)
    if prev is not None:
        cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
    return cb


def _everything(r, di):
    out = {"final": r.final().copy(), "di": di.download().copy(), "counters": r.p_indirect.read_counters()}
    for nm, pl in zip(wire.GB_PLANE_NAMES, r.gbuffer.download()[0]):
        out["gb_" + nm] = np.asarray(pl).copy()
    for nm in RPT_PLANES:
        a = r.p_indirect.download_plane(nm)
        out["rpt_" + nm] = (a & 0xffffff) if nm == "A" else a
    return out


FRAME_TIMES = {2: 0.2, 3: 0.45, 4: 0.7, 5: 1.1}      # frame 1 is rendered at rest


@pytest.fixture(scope="module")
def host_path_frames(api, cornell):
    """renderer A: five frames, four of them animated through the host path (the loader's own tables in its zrh_scene_data)"""
    path, sc, offs = cornell
    host = cases.HostData.from_gltf(path)
    r = api.Renderer(sc, W, H, params=wire.default_params(), integrator=api.INTEGRATOR_RESTIR_PT)
    di = r.enable_direct(wire.default_params_di())
    frames, prev = [], None
    for f in range(1, 6):
        if f in FRAME_TIMES:
            host.apply(r.scene, FRAME_TIMES[f])
        cb = _cb(sc, offs, f, prev)
        prev = cb.copy()
        r.p_indirect.read_counters(reset=True)
        r.render_frame(cb)
        frames.append(_everything(r, di))
    ems = r.scene.download_emissives()
    host.close()
    return frames, ems


def test_rendered_frames_equal_the_host_path(api, cornell, host_path_frames):
    """check 2: ReSTIR PT at 96 x 64 with emissive ReSTIR DI attached, 4 frames at advancing t through Renderer.animate: G-buffer planes, FINAL, the DI
    image, every reservoir plane and the ray counters equal the host path's"""
    want, ems_a = host_path_frames
    path, sc, offs = cornell
    desc = sc.animation
    r = api.Renderer(sc, W, H, params=wire.default_params(), integrator=api.INTEGRATOR_RESTIR_PT)
    di = r.enable_direct(wire.default_params_di())
    r.scene.set_object_emissives(sc.emissives_initial)
    r.set_animation(desc)
    before = r.scene.download_emissives()
    prev = None
    for f in range(1, 6):
        if f in FRAME_TIMES:
            r.animate(FRAME_TIMES[f])
        cb = _cb(sc, offs, f, prev)
        prev = cb.copy()
        r.p_indirect.read_counters(reset=True)
        r.render_frame(cb)
        got = _everything(r, di)
        for k, v in want[f - 1].items():
            if k == "counters":
                assert got[k] == v, f"frame {f}: ray counters"
            else:
                assert np.asarray(got[k]).tobytes() == np.asarray(v).tobytes(), f"frame {f}: {k}"
    after = r.scene.download_emissives()
    assert after.tobytes() == ems_a.tobytes()
    assert not np.array_equal(before.view(np.uint8), after.view(np.uint8))      # the light really moved
    assert float(want[-1]["di"][..., :3].max()) > 0
    assert want[1]["gb_" + wire.GB_PLANE_NAMES[0]].tobytes() != want[4]["gb_" + wire.GB_PLANE_NAMES[0]].tobytes() or want[1]["final"].tobytes() != want[4]["final"].tobytes()


def test_animate_on_one_stream_renders_on_another(api, cornell, host_path_frames):
    """check 4: every animate ENQUEUED on one non-blocking stream, every frame rendered on another, back to back without a host wait, images copied out
    on the render stream: the images of check 2"""
    import torch
    want, _ = host_path_frames
    path, sc, offs = cornell
    desc = sc.animation
    r = api.Renderer(sc, W, H, params=wire.default_params(), integrator=api.INTEGRATOR_RESTIR_PT)
    di = r.enable_direct(wire.default_params_di())
    r.scene.set_object_emissives(sc.emissives_initial)
    r.set_animation(desc)
    s_upd, s_ren = torch.cuda.Stream(), torch.cuda.Stream()
    nbytes = W * H * 16
    hip_path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)      # the HIP runtime this process already uses
    hip = C.CDLL(hip_path)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    snaps, prev = [], None
    for f in range(1, 6):
        if f in FRAME_TIMES:
            r.animate(FRAME_TIMES[f], stream=s_upd.cuda_stream)
        cb = _cb(sc, offs, f, prev)
        prev = cb.copy()
        r.render_frame(cb, stream=s_ren.cuda_stream)
        snap = torch.zeros(2 * nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()          # the allocation's fill, not the renders
        pt_ptr, di_ptr = r.p_indirect.output_ptr()[0], di.output_ptr()[0]
        assert hip.hipMemcpyAsync(snap.data_ptr(), pt_ptr, nbytes, 3, s_ren.cuda_stream) == 0
        assert hip.hipMemcpyAsync(snap.data_ptr() + nbytes, di_ptr, nbytes, 3, s_ren.cuda_stream) == 0
        snaps.append(snap)
    torch.cuda.synchronize()
    for f, snap in enumerate(snaps, 1):
        got = snap.cpu().numpy().view(np.float32).reshape(2, H, W, 4)
        assert got[0].tobytes() == want[f - 1]["final"].tobytes(), f"frame {f}: ReSTIR PT"
        assert got[1].tobytes() == want[f - 1]["di"].tobytes(), f"frame {f}: ReSTIR DI"


def test_readers_of_the_host_matrices_after_animate(api, cornell):
    """check 3: after animate the host's copies of the matrices are brought up to date where they are read: download_instances gives the device's
    matrices, which are the host path's, and the picked-instance mask (ZR_OUT_PICK_MASK) of an animated instance equals the host path's -- and is
    not the mask of the instance at rest"""
    from tests.test_pick_outline_gpu import Frame
    path, sc, offs = cornell
    desc = sc.animation
    short, tall = int(desc.instance_idx[1]), int(desc.instance_idx[2])      # the turning box; the tall box, on its animated parent
    host = cases.HostData.from_gltf(path)
    fa, fb = Frame(sc, (W, H), (W, H)), Frame(sc, (W, H), (W, H))
    fb.scene.set_object_emissives(sc.emissives_initial)
    fb.scene.set_animation(desc)
    fa.pick(48, 40); fb.pick(48, 40)      # (renders the G-buffer the display pass reads)
    rest = {}
    for inst in (short, tall):
        fb.show([inst])
        rest[inst] = fb.p.download_plane("pick_mask").copy()
    masks = {short: [], tall: []}
    for t in (0.4, 1.4):
        host.apply(fa.scene, t)
        fb.scene.animate(t)
        xa, xb = fa.scene.download_instances(0)[1], fb.scene.download_instances(0)[1]
        assert xb.tobytes() == xa.tobytes() == host.world.tobytes()
        for inst in (short, tall):
            fa.show([inst]); fb.show([inst])
            ma, mb = fa.p.download_plane("pick_mask"), fb.p.download_plane("pick_mask")
            assert np.array_equal(ma, mb), f"t = {t}, instance {inst}: {int((ma != mb).sum())} mask pixels differ from the host path's"
            masks[inst].append(mb.copy())
    for inst in (short, tall):
        assert masks[inst][-1].any() and not np.array_equal(masks[inst][-1], rest[inst]), inst
    assert not np.array_equal(masks[short][0], masks[short][1])
    host.close()


def test_cpp_mirror_animates_either_way(api, scene):
    """zrh_scene_animate (zr_host.h) in its two forms on twin scenes: the host path (begin_frame, zrh_scene_data_animate, hand-over) and, after
    zrh_scene_data_set_device_animation, the time alone -- the tables and the object-space lights reach the device scene with the first frame"""
    path, trs, sc = scene
    desc = cases.animation(trs, 65)
    host, dev = cases.HostData.from_gltf(path), cases.HostData.from_gltf(path)
    assert host.set_animation(desc) == 0 and dev.set_animation(desc) == 0
    A, B = api.Scene(sc), api.Scene(sc)
    L = cases.sio()
    L.zrh_scene_data_set_device_animation.argtypes = [C.c_void_p, C.c_int]
    L.zrh_scene_data_set_device_animation(dev.h, 1)
    Hl = C.CDLL(os.path.join(ROOT, "zetaray_amd", "libzetaray_host.so"))
    Hl.zrh_scene_animate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    for t in cases.TIMES[1:5]:
        assert Hl.zrh_scene_animate(host.h, A.h, None, t) == 0, api.lib().zr_last_error()
        assert Hl.zrh_scene_animate(dev.h, B.h, None, t) == 0, api.lib().zr_last_error()
        api._check(api.lib().zr_device_synchronize(0))
        _assert_buffers(B, A, host, f"t = {t}")
    A.close(); B.close(); host.close(); dev.close()
