"""Ray queries against brute force at seams, edges and grazing rays (CPU: the product's traversal compiled for the host, and the oracle's BVH2).

include/zr_intersect.h claims that closest hit (with the index tie-break) and any hit do not depend on the acceptance structure, within a
stated condition on the ray.  Every bit-exact comparison between two different trees rests on that claim.  Here each adversarial ray family of
tests/raycheck.py runs on four scenes against the numpy restatement of zr_ray_tri over all triangles:
  - inside the condition: equal bit for bit, closest and any hit, every mask;
  - outside it, the weaker property of zr_intersect.h (raycheck.check_against_brute): every hit returned is one zr_ray_tri accepts, at most
    CLOSEST_SLACK behind the brute-force hit; any hit never reports an occlusion brute force does not see; and the queries that lose a
    brute-force hit (a miss, or an any-hit leak) stay below OUTSIDE_LOSS of the rays outside the condition.
The float64 leg judges zr_ray_tri itself against exact intersections of the stored triangles."""
import numpy as np
import pytest

from oracle import zro
from tests import raycheck as rc
from tests.hostexec import zhx

N_RAYS = 4000                     # per family and scene (the t_* families expand this several times)
# float64 leg
ROBUST_MARGIN, ROBUST_COS, ROBUST_REACH = 1e-4, 1e-2, 16.0
T_REL_BOUND = 1e-4               # robust rays: |t32 - t64| <= T_REL_BOUND x max(|t64|, s / |d|)
DIST_BOUND = 2.0 ** -14          # every hit: float64 distance from o + t d to the triangle <= DIST_BOUND x (|o - v0| + s) / |cos|
COND_REACH = rc.COND_REACH
SCENES = rc.SCENES
check_against_brute = rc.check_against_brute
_cornell = rc.cornell_scene

REPRODUCER = np.array([0xbd356687, 0x3fc03a63, 0xbf130bfd, 0x0, 0x3982f83a, 0xbf7ffffc, 0x3a0d2896, 0x7f61b1e6], np.uint32).view(np.float32)


@pytest.fixture(scope="module", params=sorted(SCENES))
def world(request):
    sc = SCENES[request.param]()
    br = rc.Brute(sc)
    return request.param, sc, br, zhx.HostExecScene(sc), zro.OracleScene(sc, force_bvh=True)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_brute_force_equals_oracle_brute_force(cornell_emissive, oracle_emissive):
    """the numpy restatement of zr_ray_tri + closest / any hit == the oracle's brute force (<= 256 triangles), bit for bit, every family"""
    br = rc.Brute(cornell_emissive)
    for i, fam in enumerate(rc.FAMILIES):
        rays = rc.family_rays(fam, br, 1000 + i, 2500)
        for mask in (3, 1, 2):
            assert np.array_equal(br.closest(rays, mask), oracle_emissive.trace_closest(rays, mask)), (fam, mask)
            assert np.array_equal(br.any(rays, mask), oracle_emissive.trace_any(rays, mask)), (fam, mask)


def test_reproducer_ray():
    """the ray of the issue: brute force hits triangle 35 at its vertex (u = v = 0) at t = 1.4690353; so must both trees, also with the
    segment ending just past that hit"""
    sc = _cornell()
    br = rc.Brute(sc)
    hx, ob = zhx.HostExecScene(sc), zro.OracleScene(sc, force_bvh=True)
    rays = np.stack([REPRODUCER, REPRODUCER.copy()])
    rays[1, 7] = np.float32(1.4692)
    want = br.closest(rays)
    assert want[0, 3] == 35 and (want[0, 1:3] & 0x7fffffff == 0).all()
    assert np.isclose(want[0, :1].view(np.float32)[0], 1.4690353)
    for tree in (hx, ob):
        assert np.array_equal(tree.trace_closest(rays), want)
        assert np.array_equal(tree.trace_any(rays), np.ones(2, np.uint32))


def test_float64_leg(world):
    """zr_ray_tri against exact intersections: robust rays (barycentric margin >= 1e-4, |cos| >= 1e-2, inside the stated condition, no other
    triangle within the margin before the hit) hit the float64 triangle with t within T_REL_BOUND; every hit returned lies within DIST_BOUND x (|o - v0| + s) / |cos| of its triangle"""
    name, sc, br, hx, ob = world
    n_robust = 0
    for i, fam in enumerate(("edge_random", "edge_near_axis", "edge_grazing", "axis_parallel", "scaled", "near_axis_random")):
        rays = rc.family_rays(fam, br, 2000 + i, N_RAYS)
        got = br.closest(rays)
        tri64, t64, marg, cos = br.exact(rays)
        # robust: the exact hit is well inside, not grazing, and not near tmin / tmax
        tt = np.where(tri64 >= 0, t64, 0)
        robust = (tri64 >= 0) & (marg >= ROBUST_MARGIN) & (cos >= ROBUST_COS)
        # float32's own error grows with |o - v0| / |cos| (also for the triangles the ray passes near on its way): a 1e-4 margin is robust for
        # origins within ROBUST_REACH x s of the hit triangle, s = its largest |coordinate|
        k = np.maximum(tri64, 0)
        sk = np.abs(np.stack([br.v0[k], br.v0[k] + br.e1[k], br.v0[k] + br.e2[k]], 1).astype(np.float64)).max((1, 2))
        robust &= np.linalg.norm(rays[:, 0:3].astype(np.float64) - br.v0[k], axis=1) <= ROBUST_REACH * sk
        # ... and for triangles not small against their own coordinates (at 1e4 a float32 step is 1e-3: a 0.3-wide triangle has no 1e-4 margin)
        size = np.maximum(np.linalg.norm(br.e1[k].astype(np.float64), axis=1), np.linalg.norm(br.e2[k].astype(np.float64), axis=1))
        robust &= size * ROBUST_REACH >= sk
        robust &= (tt - rays[:, 3] > 1e-3 * np.abs(tt)) & (rays[:, 7] - tt > 1e-3 * np.abs(tt))
        # ... and no other triangle passes within the same margin of the ray before it (a near miss at an edge that float32 may accept)
        tri_l, t_l = br.exact(rays, slack=ROBUST_MARGIN)[:2]
        robust &= (tri_l == tri64) | (np.abs(t_l - tt) <= T_REL_BOUND * np.abs(tt))
        n_robust += int(robust.sum())
        r = np.nonzero(robust & (got[:, 3] != rc.MISS))[0]
        assert len(r) == robust.sum(), f"{name}/{fam}: a robust ray misses"
        # the returned triangle is the exact one, or one whose exact t ties with it within T_REL_BOUND (coplanar or duplicated geometry)
        k = got[r, 3].astype(np.int64)
        tk = br.exact_t(rays[r], k)
        nk = np.cross(br.e1[k].astype(np.float64), br.e2[k].astype(np.float64))
        dk = rays[r, 4:7].astype(np.float64)
        cos_k = np.abs((nk * dk).sum(1)) / (np.linalg.norm(nk, axis=1) * np.linalg.norm(dk, axis=1))
        # ... or a triangle the ray grazes on its way (|cos| < ROBUST_COS: zr_ray_tri's barycentrics are not robust there)
        assert np.all((k == tri64[r]) | (np.abs(tk - t64[r]) <= T_REL_BOUND * np.abs(t64[r])) | (cos_k < ROBUST_COS)), \
            f"{name}/{fam}: robust ray hits another triangle"
        same = (k == tri64[r]) | (np.abs(tk - t64[r]) <= T_REL_BOUND * np.abs(t64[r]))
        t32 = got[r, 0].view(np.float32).astype(np.float64)
        tscale = np.maximum(np.abs(t64[r]), sk[r] / np.linalg.norm(rays[r, 4:7].astype(np.float64), axis=1))
        assert np.all((np.abs(t32 - t64[r]) <= T_REL_BOUND * tscale) | ~same), f"{name}/{fam}: t beyond the relative bound"
        h = np.nonzero(got[:, 3] != rc.MISS)[0]
        k = got[h, 3].astype(np.int64)
        t = got[h, 0].view(np.float32).astype(np.float64)
        P = rays[h, 0:3].astype(np.float64) + t[:, None] * rays[h, 4:7].astype(np.float64)
        dist = br.distance_to_triangle(P, k)
        v0, e1, e2 = br.v0[k].astype(np.float64), br.e1[k].astype(np.float64), br.e2[k].astype(np.float64)
        s = np.abs(np.stack([v0, v0 + e1, v0 + e2], 1)).max((1, 2))
        n = np.cross(e1, e2)
        d = rays[h, 4:7].astype(np.float64)
        c = np.abs((n * d).sum(1)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d, axis=1))
        reach = np.linalg.norm(rays[h, 0:3].astype(np.float64) - v0, axis=1) + s
        assert np.all(dist <= DIST_BOUND * reach / np.maximum(c, 1e-30)), f"{name}/{fam}: a hit point lies off its triangle beyond the bound"
    assert n_robust >= 100, (name, n_robust)


# ------------------------------------------------------------------------------------------------ trees against brute force
@pytest.mark.parametrize("fam", sorted(rc.FAMILIES))
def test_host_trees_match_brute_force(world, fam):
    """the product's SAH BVH4 (host-executed) and the oracle's BVH2 == brute force inside the condition, bounded outside it"""
    name, sc, br, hx, ob = world
    rays = rc.family_rays(fam, br, 3000 + sorted(rc.FAMILIES).index(fam), N_RAYS if name != "synthetic" else N_RAYS // 4)
    inside = 0
    for tree, tn in ((hx, "product BVH4"), (ob, "oracle BVH2")):
        inside, outside, lost, leaks = check_against_brute(br, rays, tree.trace_closest(rays), tree.trace_any(rays), 3, f"{name}/{fam}/{tn}")
    assert inside >= 0.3 * len(rays), (name, fam, inside, len(rays))      # >= 30 % of every family tests the bit-exact claim


@pytest.mark.parametrize("mask", rc.ALL_MASKS)
def test_masks(world, mask):
    """instance masks 0 .. 7 (0x80 = the non-opaque bit is not a mask bit of these queries), closest and any hit"""
    name, sc, br, hx, ob = world
    rays = np.concatenate([rc.family_rays(f, br, 4000 + mask, 800) for f in ("edge_random", "edge_near_axis", "axis_parallel")])
    for tree, tn in ((hx, "product BVH4"), (ob, "oracle BVH2")):
        check_against_brute(br, rays, tree.trace_closest(rays, mask), tree.trace_any(rays, mask), mask, f"{name}/mask {mask}/{tn}")
    if mask == 0:
        assert (hx.trace_closest(rays, 0)[:, 3] == rc.MISS).all()


def test_t_interval_rules():
    """the rules pinned in include/zetaray_amd.h, both sides: accepted iff tmin < t < tmax (open at both ends), tmin may be negative (hits
    behind the origin count), tmax <= tmin hits nothing, a NaN anywhere in the ray hits nothing"""
    sc = rc.make_seams_scene()
    br = rc.Brute(sc)
    hx = zhx.HostExecScene(sc)
    base = rc.family_rays("edge_near_axis", br, 5000, 2000)
    h = br.closest(base)
    base = base[h[:, 3] != rc.MISS]
    t = br.closest(base)[:, 0].view(np.float32)
    tri = br.closest(base)[:, 3]
    one = base.copy(); one[:, 7] = t
    assert (hx.trace_closest(one)[:, 3] != tri).all()                 # tmax = t: that triangle is not hit
    one[:, 7] = np.nextafter(t, np.float32(np.inf))
    got = hx.trace_closest(one)
    assert np.array_equal(got, br.closest(one)) and (got[:, 3] == tri).mean() > 0.95
    one = base.copy(); one[:, 3] = t
    assert (hx.trace_closest(one)[:, 3] != tri).all()                 # tmin = t: skipped
    back = base.copy(); back[:, 4:7] = -back[:, 4:7]; back[:, 3] = np.float32(-np.inf)
    got = hx.trace_closest(back)
    assert np.array_equal(got, br.closest(back))          # behind the origin: the smallest (most negative) t wins
    assert (got[:, 3] != rc.MISS).all() and (got[:, 0].view(np.float32) < 0).all()
    assert (hx.trace_any(back) == 1).all()
    back[:, 3] = 0.0
    assert np.array_equal(hx.trace_closest(back), br.closest(back))
    empty = base.copy(); empty[:, 3] = 1.0; empty[:, 7] = 1.0
    assert (hx.trace_closest(empty)[:, 3] == rc.MISS).all() and (hx.trace_any(empty) == 0).all()
    for col in range(8):
        nan = base.copy(); nan[:, col] = np.nan
        assert (hx.trace_closest(nan)[:, 3] == rc.MISS).all() and (hx.trace_any(nan) == 0).all(), col


def test_duplicated_instance_ties():
    """the seams scene's fan exists twice (instances 4 and 5, identical world triangles): every hit on it reports the smaller global index"""
    sc = rc.make_seams_scene()
    br = rc.Brute(sc)
    hx, ob = zhx.HostExecScene(sc), zro.OracleScene(sc, force_bvh=True)
    first = int(sc.instance_num_tris[:4].sum())
    nfan = int(sc.instance_num_tris[4])
    rng = np.random.default_rng(9)
    k = rng.integers(first, first + nfan, 4000)
    P = br.v0[k] + rng.uniform(0, 0.5, (4000, 1)).astype(np.float32) * br.e1[k] + rng.uniform(0, 0.5, (4000, 1)).astype(np.float32) * br.e2[k]
    o = (P + np.float32([0, 1.5, 0])).astype(np.float32)
    rays = rc._rays(o, 0.0, rc._normalize(P - o), 3.0e38)
    want = br.closest(rays)
    on_fan = (want[:, 3] >= first) & (want[:, 3] < first + 2 * nfan)
    assert on_fan.sum() > 1000 and (want[on_fan, 3] < first + nfan).all()
    assert np.array_equal(hx.trace_closest(rays), want) and np.array_equal(ob.trace_closest(rays), want)


def test_refit_and_rebuild_on_host():
    """the product's host-executed tree after its instance update (refit of the moved, rotated instance) and after a rebuild that keeps the
    mover in a subtree of its own: both equal brute force over the moved scene"""
    sc = rc.make_seams_scene()
    hx = zhx.HostExecScene(sc)
    s2, k = rc.moved_seams_scene(sc)
    br = rc.Brute(s2)
    hx.update_instances(s2.instances, s2.instance_to_world)
    rays = np.concatenate([rc.family_rays(f, br, 6000 + i, 1500) for i, f in enumerate(rc.BASE_FAMILIES)])
    check_against_brute(br, rays, hx.trace_closest(rays), hx.trace_any(rays), 3, "seams moved/host update")
    own = np.zeros(len(s2.instances), np.uint8); own[k] = 1
    hx.set_own_subtree(own)
    hx.update_instances(s2.instances, s2.instance_to_world)
    check_against_brute(br, rays, hx.trace_closest(rays), hx.trace_any(rays), 3, "seams moved/own subtree")
