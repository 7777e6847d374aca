"""Ray queries on the GPU against brute force at seams, edges and grazing rays (zr_trace_closest / zr_trace_any through the C-ABI).

The same ray families and scenes as tests/test_ray_queries_cpu.py, on every tree the device can hold: the host SAH build, the device LBVH
(ZR_BVH_BUILD=device), the device LBVH under a depth cap of 7, the SAH tree after a device refit of a moved and rotated instance, and a
background SAH rebuild after it was installed.  Within the condition of zr_intersect.h every answer equals brute force bit for bit; on the
host SAH tree every answer also equals the host-executed traversal of the same tree.  Run with -m gpu."""
import time

import numpy as np
import pytest

from tests import raycheck as rc
from tests.hostexec import zhx
from tests.raycheck import SCENES, check_against_brute

pytestmark = pytest.mark.gpu
N_RAYS = 2000


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


def _trace(api, handle, rays, mask):
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d_occ = torch.zeros((n,), dtype=torch.int32, device="cuda")
    api._check(api.lib().zr_trace_closest(handle.h, None, d_rays.data_ptr(), n, mask, d_hits.data_ptr()))
    api._check(api.lib().zr_trace_any(handle.h, None, d_rays.data_ptr(), n, mask, d_occ.data_ptr()))
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(np.uint32), d_occ.cpu().numpy().view(np.uint32)


def _family_batch(br, seed):
    """every family, N_RAYS each (the t_* families expand), concatenated; plus the family name of each ray"""
    parts, names = [], []
    for i, fam in enumerate(sorted(rc.FAMILIES)):
        r = rc.family_rays(fam, br, seed + i, N_RAYS)
        parts.append(r)
        names += [fam] * len(r)
    return np.concatenate(parts), np.array(names)


def _check_tree(api, handle, br, rays, label, hx=None):
    for mask in rc.ALL_MASKS + (0x80 | 2,):
        got, occ = _trace(api, handle, rays, mask)
        check_against_brute(br, rays, got, occ, mask, f"{label}/mask {mask}")
        if hx is not None:
            assert np.array_equal(got, hx.trace_closest(rays, mask)), f"{label}/mask {mask}: GPU != host-executed closest hit"
            assert np.array_equal(occ, hx.trace_any(rays, mask)), f"{label}/mask {mask}: GPU != host-executed any hit"


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_host_sah_tree(api, scene):
    sc = SCENES[scene]()
    br = rc.Brute(sc)
    rays, _ = _family_batch(br, 100)
    handle = api.Scene(sc)
    try:
        _check_tree(api, handle, br, rays, f"{scene}/host SAH", hx=zhx.HostExecScene(sc))
    finally:
        handle.close()


@pytest.mark.parametrize("scene", ["cornell", "seams", "synthetic"])
@pytest.mark.parametrize("cap", [0, 7])
def test_device_lbvh(api, monkeypatch, scene, cap):
    """ZR_BVH_BUILD=device, with its natural depth and under zr_debug_set_bvh_depth_cap(7)"""
    monkeypatch.setenv("ZR_BVH_BUILD", "device")
    sc = SCENES[scene]()
    br = rc.Brute(sc)
    rays, _ = _family_batch(br, 200)
    if cap:
        assert api.lib().zr_debug_set_bvh_depth_cap(cap) == 0
    try:
        handle = api.Scene(sc)
        try:
            if cap:
                assert handle.bvh_info()[2] <= cap
            _check_tree(api, handle, br, rays, f"{scene}/device LBVH cap {cap}")
        finally:
            handle.close()
    finally:
        if cap:
            api.lib().zr_debug_set_bvh_depth_cap(0)


def test_refit_of_moved_instance(api):
    """the seams scene's scaled + rotated instance moved and turned; the device refits the host SAH tree's boxes"""
    sc = rc.make_seams_scene()
    handle = api.Scene(sc)
    try:
        s2, _ = rc.moved_seams_scene(sc)
        handle.update_instances(s2.instances, s2.instance_to_world)
        br = rc.Brute(s2)
        rays, _ = _family_batch(br, 300)
        _check_tree(api, handle, br, rays, "seams/device refit")
    finally:
        handle.close()


def test_background_rebuild_installed(api):
    """zr_scene_set_background_rebuild: the host rebuilds an SAH tree for the moved instance on a thread; a later update installs it"""
    sc = rc.make_seams_scene()
    handle = api.Scene(sc)
    try:
        handle.set_background_rebuild(True)
        s2, _ = rc.moved_seams_scene(sc)
        handle.update_instances(s2.instances, s2.instance_to_world)
        t0 = time.perf_counter()
        while handle.background_rebuild_stats()[2] == 1 and time.perf_counter() - t0 < 20.0:
            time.sleep(0.005)
        handle.update_instances(s2.instances, s2.instance_to_world)
        started, installed, _ = handle.background_rebuild_stats()
        assert started >= 1 and installed >= 1, (started, installed)
        br = rc.Brute(s2)
        rays, _ = _family_batch(br, 400)
        _check_tree(api, handle, br, rays, "seams/background SAH rebuild")
    finally:
        handle.close()


@pytest.mark.parametrize("scene", ["cornell", "seams"])
def test_schedule_independence(api, scene):
    """the voted traversal runs 64 rays per wave: the adversarial rays, shuffled in among ordinary random rays, give the same answer per ray"""
    sc = SCENES[scene]()
    br = rc.Brute(sc)
    adv, _ = _family_batch(br, 500)
    handle = api.Scene(sc)
    try:
        alone, alone_occ = _trace(api, handle, adv, 3)
        rng = np.random.default_rng(17)
        n = 3 * len(adv)
        o = rc._origins_around(br, rng, rc._random_tris(br, rng, n), 0.0)
        plain = rc._rays(o, 0.0, rc._normalize(rng.normal(size=(n, 3))), 3.0e38)
        mixed = np.concatenate([adv, plain])
        perm = rng.permutation(len(mixed))
        got, occ = _trace(api, handle, mixed[perm], 3)
        back = np.empty_like(got); back[perm] = got
        back_occ = np.empty_like(occ); back_occ[perm] = occ
        assert np.array_equal(back[:len(adv)], alone) and np.array_equal(back_occ[:len(adv)], alone_occ)
        check_against_brute(br, plain, back[len(adv):], back_occ[len(adv):], 3, f"{scene}/ordinary rays")
    finally:
        handle.close()
