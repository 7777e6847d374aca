"""The scene's current / previous buffer sets across the forms of the frame's update ON ONE SCENE: host records (zr_scene_update_instances), moved
matrices (zr_scene_move_instances), the animation (zr_scene_animate) and the install of a background SAH tree, one after the other.  The other suites
check each form by itself against the host path; this one checks that whatever form a frame takes, the set it leaves behind is the one the next
frame -- of any form -- demotes to "previous"."""
import time

import numpy as np
import pytest

from tests.animmath import cases
from tests.test_scene_move_gpu import _matrix, _write_scene
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
W, H = 64, 48
N_RAYS = 2000


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


def _animation():
    """the two larger lights and a plain instance on nodes of their own, a plain instance on an animated node with a static child that carries another"""
    b = cases.Builder(5)
    for i in (3, 2, 5):
        b.node(cases.rest_of(cases._node_trs(i)), [i])
    root = b.node(cases.rest_of(cases._node_trs(4)), [4])
    b.node(cases.rest_of(cases._node_trs(6)), [6], parent=root, animated=False)
    return b.desc()


def _rays():
    """origins in a box around the seven instances, directions uniform on the sphere, tmin 0, tmax 100"""
    rng = np.random.default_rng(41)
    d = rng.normal(size=(N_RAYS, 3))
    r = np.empty((N_RAYS, 8), np.float32)
    r[:, 0:3] = rng.uniform([-3.0, -0.5, -2.0], [3.0, 2.5, 2.0], (N_RAYS, 3))
    r[:, 3] = 0.0
    r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 7] = 100.0
    return r


def _closest(api, scene, d_rays):
    import torch
    d_hits = torch.zeros((N_RAYS, 4), dtype=torch.int32, device="cuda")
    api._check(api.lib().zr_trace_closest(scene.h, None, d_rays.data_ptr(), N_RAYS, 3, d_hits.data_ptr()))
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(np.uint32)


def test_role_changes_across_update_forms(api, tmp_path):
    """Scene A: host records / move_instances / animate / move_instances with an empty list / host records / background rebuild switched on and
    move_instances until a tree has been installed / animate / host records, one update per frame.  Scene B: the same matrices through the host
    form only.  After every frame: (a) A's previous instance buffer is what its current one was a frame ago, bit for bit; (b) A's current records and
    matrices are B's; (c) bvh_info reports the scene's 324 triangles and a tree; (d) 2 000 closest-hit queries answer alike on A and B; (e) a 64 x 48
    ReSTIR PT frame, chained with the previous frame's constants -- its temporal passes bind the previous set -- is bit-identical between A and B"""
    import torch
    path = _write_scene(tmp_path)
    sc, _ = scene_io.load_gltf_native(path)
    assert sc.num_tris == 324
    host = cases.HostData.from_gltf(path)
    desc = _animation()
    assert host.set_animation(desc) == 0
    prm = wire.default_params()
    ra = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    rb = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    A, B = ra.scene, rb.scene
    A.set_object_emissives(host.init)
    A.set_animation(desc)
    d_rays = torch.from_numpy(_rays()).cuda()
    rng = np.random.default_rng(37)
    state = {"f": 0, "prev_cb": None, "was_current": A.download_instances(0)[0].tobytes(), "hit_any": False}

    def frame(form, t=None, moved=()):
        """one update of the given form on A, the same matrices in the host form on B, then the five checks"""
        state["f"] += 1
        what = f"frame {state['f']} ({form})"
        first, count = host.frame(t, moved)
        for X in (A, B) if form == "host" else (B,):
            if count:
                X.update_emissives(host.ems[first:first + count].copy(), first)
            X.update_instances(host.inst.copy(), host.world.copy())
        if form == "move":
            A.move_instances([i for i, _ in moved], [np.asarray(M, np.float32).reshape(12) for _, M in moved])
        elif form == "animate":
            A.animate(t)
        t0 = time.perf_counter()
        while A.background_rebuild_stats()[2] == 1 and time.perf_counter() - t0 < 20.0:      # (the builder's thread: a deterministic schedule)
            time.sleep(0.002)
        cur, xf = A.download_instances(0)
        assert A.download_instances(1)[0].tobytes() == state["was_current"], f"{what}: (a) the previous records are not last frame's current ones"
        state["was_current"] = cur.tobytes()
        cur_b, xf_b = B.download_instances(0)
        assert cur.tobytes() == cur_b.tobytes() and cur.tobytes() == host.inst.tobytes(), f"{what}: (b) current records"
        assert xf.tobytes() == xf_b.tobytes() and xf.tobytes() == host.world.tobytes(), f"{what}: (b) matrices"
        assert A.download_emissives().tobytes() == B.download_emissives().tobytes(), f"{what}: (b) emissive records"
        for X in (A, B):
            nodes, tris, _ = X.bvh_info()
            assert tris == sc.num_tris and nodes > 0, f"{what}: (c) bvh_info {(nodes, tris)}"
        hits = _closest(api, A, d_rays)
        assert np.array_equal(hits, _closest(api, B, d_rays)), f"{what}: (d) closest hits"
        state["hit_any"] |= bool((hits[:, 3] != 0xFFFFFFFF).any())
        cb = scene_io.make_frame_constants(W, H, frame_num=state["f"], num_emissives=len(sc.emissives), cam_pos=(0.0, 1.0, -4.0))
        if state["prev_cb"] is not None:
            p = state["prev_cb"]
            cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = p["curr_view"], p["curr_view_inv"], p["curr_camera_jitter"]
        state["prev_cb"] = cb.copy()
        ra.render_frame(cb); rb.render_frame(cb)
        assert ra.final().tobytes() == rb.final().tobytes(), f"{what}: (e) ReSTIR PT frame"

    frame("host", moved=[(2, _matrix(rng, 2))])
    frame("move", moved=[(3, _matrix(rng, 3)), (0, _matrix(rng, 0))])
    frame("animate", t=0.5)
    frame("move", moved=[])
    frame("host", moved=[(5, _matrix(rng, 5)), (1, _matrix(rng, 1))])
    A.set_background_rebuild(True)
    while A.background_rebuild_stats()[1] < 1 and state["f"] < 45:
        k = state["f"]
        frame("move", moved=[(i, _matrix(rng, i)) for i in (k % 7, (k + 3) % 7)])
    assert A.background_rebuild_stats()[1] >= 1, f"no background tree installed within {state['f']} frames: {A.background_rebuild_stats()}"
    frame("animate", t=1.25)
    frame("host", moved=[(4, _matrix(rng, 4))])
    assert state["hit_any"] and float(ra.final()[..., :3].max()) > 0      # the rays and the camera do see the scene
    host.close()
