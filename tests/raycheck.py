"""Brute-force reference for ray queries, adversarial ray families and the scenes they run on (test helper, no GPU).

The reference restates include/zr_intersect.h zr_ray_tri in numpy float32 -- the same operations in the same order, every product and sum
rounded on its own (no fused operations) -- over the scene's world-space triangles built by the 3x4 rule of the same header.  Closest hit takes
the smallest t and, among equal t, the smallest global triangle index; any hit is "some triangle accepts".  Results use the packing of
zr_trace_closest: (t bits, u bits, v bits, triangle), a miss = (0, 0, 0, 0xffffffff).

A float64 leg judges the shared arithmetic itself: exact intersections of the stored (float32) triangles, computed in float64."""
import os

import numpy as np

from zetaray_amd import scene_io, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
MISS = 0xFFFFFFFF
ALL_MASKS = tuple(range(8))


# ---------------------------------------------------------------------------------------------------- world-space triangles
def world_tris(scene):
    """(v0, e1, e2), each (N, 3) float32, in global order (instances in order, each instance's triangles in index order), and the
    instance mask of every triangle.  row . (p, 1) summed left to right, e = v - v0, as zr_bvh.h Build / zro_scene.h BuildTris."""
    v0s, e1s, e2s, masks = [], [], [], []
    for i in range(len(scene.instances)):
        inst = scene.instances[i]
        M = scene.instance_to_world[i].astype(F).reshape(3, 4)
        n = int(scene.instance_num_tris[i])
        idx = scene.indices[int(inst["base_idx_offset"]): int(inst["base_idx_offset"]) + 3 * n].astype(np.int64) + int(inst["base_vtx_offset"])
        P = scene.vertices["pos"][idx].astype(F).reshape(n, 3, 3)
        W = np.empty_like(P)
        for r in range(3):
            W[:, :, r] = M[r, 0] * P[:, :, 0] + M[r, 1] * P[:, :, 1] + M[r, 2] * P[:, :, 2] + M[r, 3]
        v0s.append(W[:, 0]); e1s.append(W[:, 1] - W[:, 0]); e2s.append(W[:, 2] - W[:, 0])
        masks.append(np.full(n, scene.instance_mask[i], np.uint32))
    return (np.concatenate(v0s).astype(F), np.concatenate(e1s).astype(F), np.concatenate(e2s).astype(F), np.concatenate(masks))


class Brute:
    """zr_ray_tri over every triangle of a scene, float32, chunked over rays."""

    def __init__(self, scene, chunk_elems=1 << 22):
        self.v0, self.e1, self.e2, self.mask = world_tris(scene)
        self.n = len(self.v0)
        self.chunk = max(1, chunk_elems // max(1, self.n))

    def _chunk(self, rays, mask):
        o, tmin, d, tmax = rays[:, None, 0:3], rays[:, None, 3], rays[:, None, 4:7], rays[:, None, 7]
        ox, oy, oz = o[..., 0], o[..., 1], o[..., 2]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        v0x, v0y, v0z = self.v0[None, :, 0], self.v0[None, :, 1], self.v0[None, :, 2]
        e1x, e1y, e1z = self.e1[None, :, 0], self.e1[None, :, 1], self.e1[None, :, 2]
        e2x, e2y, e2z = self.e2[None, :, 0], self.e2[None, :, 1], self.e2[None, :, 2]
        with np.errstate(all="ignore"):
            px = dy * e2z - dz * e2y
            py = dz * e2x - dx * e2z
            pz = dx * e2y - dy * e2x
            det = e1x * px + e1y * py + e1z * pz
            inv = F(1) / det
            tx, ty, tz = ox - v0x, oy - v0y, oz - v0z
            u = (tx * px + ty * py + tz * pz) * inv
            qx = ty * e1z - tz * e1y
            qy = tz * e1x - tx * e1z
            qz = tx * e1y - ty * e1x
            v = (dx * qx + dy * qy + dz * qz) * inv
            t = (e2x * qx + e2y * qy + e2z * qz) * inv
            ok = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & ((u + v) <= 1) & (t > tmin) & (t < tmax)
        ok &= (self.mask[None, :] & np.uint32(mask)) != 0
        return ok, t, u, v

    def closest(self, rays, mask=3):
        rays = np.ascontiguousarray(rays, F)
        out = np.zeros((len(rays), 4), np.uint32)
        out[:, 3] = MISS
        for a in range(0, len(rays), self.chunk):
            ok, t, u, v = self._chunk(rays[a:a + self.chunk], mask)
            tt = np.where(ok, t, F(np.inf))
            best = tt.min(1)
            anyok = ok.any(1)
            win = ok & (tt == best[:, None])             # -0 == +0: an exact tie, the smaller index wins
            j = np.argmax(win, 1)
            r = np.arange(len(j))
            blk = np.stack([t[r, j].view(np.uint32), u[r, j].view(np.uint32), v[r, j].view(np.uint32), j.astype(np.uint32)], 1)
            out[a:a + self.chunk] = np.where(anyok[:, None], blk, np.array([0, 0, 0, MISS], np.uint32))
        return out

    def any(self, rays, mask=3):
        rays = np.ascontiguousarray(rays, F)
        out = np.zeros(len(rays), np.uint32)
        for a in range(0, len(rays), self.chunk):
            ok, _, _, _ = self._chunk(rays[a:a + self.chunk], mask)
            out[a:a + self.chunk] = ok.any(1)
        return out

    def accepts(self, rays, tri):
        """zr_ray_tri of each ray against one given triangle (tri >= 0), with the ray's own tmin / tmax: (accepted, t)"""
        rays = np.ascontiguousarray(rays, F)
        acc = np.zeros(len(rays), bool)
        tt = np.zeros(len(rays), F)
        for k in np.unique(tri):
            sel = np.nonzero(tri == k)[0]
            sub = Brute.__new__(Brute)
            sub.v0, sub.e1, sub.e2, sub.mask = self.v0[k:k + 1], self.e1[k:k + 1], self.e2[k:k + 1], np.full(1, 0xFF, np.uint32)
            ok, t, _, _ = sub._chunk(rays[sel], 0xFF)
            acc[sel], tt[sel] = ok[:, 0], t[:, 0]
        return acc, tt

    # ---- float64 leg: the exact intersection of the stored triangles
    def exact(self, rays, mask=3, slack=0.0):
        """per ray, float64: (triangle or -1, t, barycentric margin min(u, v, 1 - u - v), |cos| between ray and face normal).  Closest over
        triangles whose exact hit lies inside (margin >= -slack) with tmin < t < tmax; rays with non-finite components miss."""
        rays = np.asarray(rays, np.float64)
        v0, e1, e2 = self.v0.astype(np.float64), self.e1.astype(np.float64), self.e2.astype(np.float64)
        nrm = np.cross(e1, e2)
        nlen = np.linalg.norm(nrm, axis=1)
        tri = np.full(len(rays), -1, np.int64)
        tb, mb, cb = np.full(len(rays), np.inf), np.zeros(len(rays)), np.zeros(len(rays))
        for a in range(0, len(rays), self.chunk):
            R = rays[a:a + self.chunk]
            o, d = R[:, None, 0:3], R[:, None, 4:7]
            with np.errstate(all="ignore"):
                p = np.cross(d, e2[None])
                det = (e1[None] * p).sum(-1)
                tv = o - v0[None]
                u = (tv * p).sum(-1) / det
                q = np.cross(tv, e1[None])
                v = (d * q).sum(-1) / det
                t = (e2[None] * q).sum(-1) / det
                marg = np.minimum(np.minimum(u, v), 1 - u - v)
                ok = (det != 0) & (marg >= -slack) & (t > R[:, None, 3]) & (t < R[:, None, 7]) & np.isfinite(t)
                ok &= (self.mask[None, :] & np.uint32(mask)) != 0
                ok &= np.isfinite(R).all(1)[:, None]
                tt = np.where(ok, t, np.inf)
                j = np.argmin(tt, 1)
                r = np.arange(len(j))
                hit = ok[r, j]
                dl = np.linalg.norm(R[:, 4:7], axis=1)
                cos = np.abs((R[:, 4:7] * nrm[j]).sum(1)) / (dl * nlen[j])
            tri[a:a + self.chunk] = np.where(hit, j, -1)
            tb[a:a + self.chunk] = np.where(hit, tt[r, j], np.inf)
            mb[a:a + self.chunk] = np.where(hit, marg[r, j], 0)
            cb[a:a + self.chunk] = np.where(hit, cos, 0)
        return tri, tb, mb, cb

    def exact_t(self, rays, tri):
        """float64 ray-plane distance of each ray to triangle tri[i] (no inside test)"""
        R = np.asarray(rays, np.float64)
        v0, e1, e2 = self.v0[tri].astype(np.float64), self.e1[tri].astype(np.float64), self.e2[tri].astype(np.float64)
        n = np.cross(e1, e2)
        with np.errstate(all="ignore"):
            return ((v0 - R[:, 0:3]) * n).sum(1) / (R[:, 4:7] * n).sum(1)

    def distance_to_triangle(self, points, tri):
        """float64 distance from each point to triangle tri[i] (the stored float32 triangle taken as exact)"""
        P = np.asarray(points, np.float64)
        a = self.v0[tri].astype(np.float64)
        b = a + self.e1[tri].astype(np.float64)
        c = a + self.e2[tri].astype(np.float64)
        return _point_tri_dist(P, a, b, c)


def _point_tri_dist(p, a, b, c):
    """Ericson, Real-Time Collision Detection 5.1.5 (closest point on triangle), vectorised; degenerate triangles fall back to the edges"""
    def seg(p, a, b):
        ab = b - a
        den = (ab * ab).sum(1)
        with np.errstate(all="ignore"):
            s = np.clip(np.where(den > 0, ((p - a) * ab).sum(1) / den, 0), 0, 1)
        return np.linalg.norm(p - (a + s[:, None] * ab), axis=1)
    dist = np.minimum(np.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(1)
    with np.errstate(all="ignore"):
        # inside test by barycentrics of the projection onto the plane
        w = p - a
        h = (w * n).sum(1) / nn
        proj = p - h[:, None] * n
        v0, v1, v2 = b - a, c - a, proj - a
        d00, d01, d11 = (v0 * v0).sum(1), (v0 * v1).sum(1), (v1 * v1).sum(1)
        d20, d21 = (v2 * v0).sum(1), (v2 * v1).sum(1)
        den = d00 * d11 - d01 * d01
        bv = (d11 * d20 - d01 * d21) / den
        bw = (d00 * d21 - d01 * d20) / den
        inside = (nn > 0) & (bv >= 0) & (bw >= 0) & (bv + bw <= 1)
        plane = np.abs(h) * np.sqrt(nn)
    return np.where(inside, np.minimum(plane, dist), dist)


# ---------------------------------------------------------------------------------------------------- ray families
def _rays(o, tmin, d, tmax):
    n = len(o)
    r = np.empty((n, 8), F)
    r[:, 0:3] = o
    r[:, 3] = np.broadcast_to(np.asarray(tmin, F), (n,))
    r[:, 4:7] = d
    r[:, 7] = np.broadcast_to(np.asarray(tmax, F), (n,))
    return r


def _normalize(d):
    d = np.asarray(d, F)
    ln = np.sqrt((d * d).sum(1, dtype=F)).astype(F)
    with np.errstate(all="ignore"):
        out = (d / np.where(ln > 0, ln, F(1))[:, None]).astype(F)
    return out


def _bounds(br):
    P = np.concatenate([br.v0, br.v0 + br.e1, br.v0 + br.e2]).astype(np.float64)
    return P.min(0), P.max(0)


CLUSTER_CELL = 1000.0     # triangles whose centroids share a cell of this size form one cluster (the seams scene: the geometry near the origin, the far instance)


def _cluster_bounds(br):
    """per triangle, (lo, hi) of the cluster it belongs to: random origins are drawn around the geometry a ray is meant for, so that a scene with
    one instance 1e4 away does not put nearly every origin thousands of units from everything else"""
    if getattr(br, "_cb", None) is None:
        P = np.stack([br.v0, br.v0 + br.e1, br.v0 + br.e2], 1).astype(np.float64)
        key = np.floor(P.mean(1) / CLUSTER_CELL).astype(np.int64)
        _, cid = np.unique(key, axis=0, return_inverse=True)
        cid = cid.reshape(-1)
        lo, hi = np.empty((len(P), 3)), np.empty((len(P), 3))
        for c in np.unique(cid):
            m = cid == c
            lo[m], hi[m] = P[m].min((0, 1)), P[m].max((0, 1))
        br._cb = (lo, hi)
    return br._cb


def _origins_around(br, rng, tri, pad_frac, pad_abs=0.0):
    """one uniform origin per ray in the bounds of triangle tri[i]'s cluster, grown by pad_frac x its extent + pad_abs"""
    lo, hi = _cluster_bounds(br)
    lo, hi = lo[tri], hi[tri]
    ext = np.maximum(hi - lo, 1e-3)
    return rng.uniform(lo - pad_frac * ext - pad_abs, hi + pad_frac * ext + pad_abs).astype(F)


def _random_tris(br, rng, n):
    return rng.integers(0, len(br.v0), n)


def _edge_targets(br, rng, n, vertex_frac=0.25):
    """points on edges (v0 + s e, float32) or exactly at vertices, and the triangle each belongs to (non-degenerate triangles)"""
    area = np.linalg.norm(np.cross(br.e1.astype(np.float64), br.e2.astype(np.float64)), axis=1)
    cand = np.nonzero(area > 0)[0]
    tri = cand[rng.integers(0, len(cand), n)]
    v0, e1, e2 = br.v0[tri], br.e1[tri], br.e2[tri]
    which = rng.integers(0, 3, n)
    s = rng.uniform(0, 1, n).astype(F)
    s = np.where(rng.uniform(size=n) < vertex_frac, rng.integers(0, 2, n).astype(F), s)
    base = np.where((which == 2)[:, None], (v0 + e1).astype(F), v0)
    edge = np.choose(which[:, None], [e1, e2, (e2 - e1).astype(F)]).astype(F)
    return (base + s[:, None] * edge).astype(F), tri


def fam_edge_random(br, rng, n):
    """rays from random origins around the scene aimed at points on triangle edges and at vertices"""
    P, tri = _edge_targets(br, rng, n)
    o = _origins_around(br, rng, tri, 0.25)
    return _rays(o, 0.0, _normalize(P - o), 3.0e38)


def fam_edge_near_axis(br, rng, n):
    """edge / vertex aimed rays whose direction lies within 1e-3 of +-x, +-y or +-z"""
    P, _ = _edge_targets(br, rng, n)
    ax = rng.integers(0, 3, n)
    sg = rng.choice([-1.0, 1.0], n)
    d = rng.uniform(-1e-3, 1e-3, (n, 3))
    d[np.arange(n), ax] = sg
    d = _normalize(d)
    back = rng.uniform(0.05, 3.0, n).astype(F)
    o = (P - back[:, None] * d).astype(F)
    return _rays(o, 0.0, d, 3.0e38)


def fam_edge_grazing(br, rng, n):
    """edge / vertex aimed rays nearly parallel to the face of the triangle they aim at (|cos| from 1e-1 down to 1e-6)"""
    P, tri = _edge_targets(br, rng, n)
    e1, e2 = br.e1[tri].astype(np.float64), br.e2[tri].astype(np.float64)
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = rng.uniform(0, 2 * np.pi, n)
    t1 = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    inplane = np.cos(a)[:, None] * t1 + np.sin(a)[:, None] * t2
    c = 10.0 ** rng.uniform(-6, -1, n) * rng.choice([-1.0, 1.0], n)
    d = _normalize(inplane + c[:, None] * nrm)
    back = rng.uniform(0.05, 3.0, n).astype(F)
    o = (P - back[:, None] * d).astype(F)
    return _rays(o, 0.0, d, 3.0e38)


def fam_axis_parallel(br, rng, n):
    """directions exactly +-x / +-y / +-z (the zero components +0 or -0) from origins of which one or two coordinates lie exactly on a
    vertex coordinate of the scene -- on box and triangle planes"""
    ax = rng.integers(0, 3, n)
    d = np.zeros((n, 3), F)
    d[rng.uniform(size=(n, 3)) < 0.5] = F(-0.0)
    d[np.arange(n), ax] = rng.choice([F(-1), F(1)], n)
    tri = _random_tris(br, rng, n)
    o = _origins_around(br, rng, tri, 0.0, 0.1)
    clo, chi = _cluster_bounds(br)
    lo, hi = clo[tri], chi[tri]
    # snap to a vertex coordinate of a triangle of the same cluster
    V = np.stack([br.v0, (br.v0 + br.e1).astype(F), (br.v0 + br.e2).astype(F)], 1)
    same = [np.nonzero((clo == clo[t]).all(1))[0] for t in tri]
    for k in range(3):
        snap = np.nonzero(rng.uniform(size=n) < 0.6)[0]
        for i in snap:
            o[i, k] = V[same[i][rng.integers(0, len(same[i]))], rng.integers(0, 3), k]
    # the origin along the ray's own axis: outside the scene half the time, on a plane (tmin = 0) otherwise
    far = rng.uniform(size=n) < 0.5
    r = np.arange(n)
    o[r[far], ax[far]] = np.where(d[r[far], ax[far]] > 0, lo[r[far], ax[far]] - 1.0, hi[r[far], ax[far]] + 1.0).astype(F)
    return _rays(o, 0.0, d, 3.0e38)


def fam_scaled(br, rng, n):
    """unnormalised directions (x 1e-3, x 1e3) and origins 1e4 away, aimed at edges and vertices"""
    P, tri = _edge_targets(br, rng, n)
    o = _origins_around(br, rng, tri, 0.0, 0.25)
    far = rng.uniform(size=n) < 1 / 3
    o[far] = (P[far] + _normalize(rng.normal(size=(far.sum(), 3))) * F(1e4)).astype(F)
    d = _normalize(P - o)
    k = rng.integers(0, 3, n)
    d = (d * np.array([1.0, 1e-3, 1e3], F)[k][:, None]).astype(F)
    return _rays(o, 0.0, d, 3.0e38)


def fam_near_axis_random(br, rng, n):
    """near-axis directions from random origins (not aimed): nearly parallel to the walls of axis-aligned geometry"""
    o = _origins_around(br, rng, _random_tris(br, rng, n), 0.0)
    ax = rng.integers(0, 3, n)
    d = rng.uniform(-1, 1, (n, 3)) * 10.0 ** rng.uniform(-7, -2, (n, 1))
    d[np.arange(n), ax] = rng.choice([-1.0, 1.0], n)
    return _rays(o, 0.0, _normalize(d), 3.0e38)


BASE_FAMILIES = {
    "edge_random": fam_edge_random,
    "edge_near_axis": fam_edge_near_axis,
    "edge_grazing": fam_edge_grazing,
    "axis_parallel": fam_axis_parallel,
    "scaled": fam_scaled,
    "near_axis_random": fam_near_axis_random,
}


def fam_t_edges(br, rng, n):
    """tmin / tmax placed at the brute-force hit t of edge-aimed rays: tmax = t (must miss that triangle), tmax = next float above t (must hit it),
    tmin = t (must skip it), shadow segments ending 0.1 % past the hit and 0.1 % short of it"""
    base = np.concatenate([fam_edge_near_axis(br, rng, n), fam_edge_random(br, rng, n)])
    h = br.closest(base)
    base = base[h[:, 3] != MISS][:n]
    t = br.closest(base)[:, 0].view(F)
    out = []
    a = base.copy(); a[:, 7] = t; out.append(a)
    a = base.copy(); a[:, 7] = np.nextafter(t, F(np.inf)); out.append(a)
    a = base.copy(); a[:, 3] = t; out.append(a)
    a = base.copy(); a[:, 3] = np.nextafter(t, F(-np.inf)); out.append(a)
    a = base.copy(); a[:, 7] = (t * F(1.001)).astype(F); out.append(a)
    a = base.copy(); a[:, 7] = (t * F(0.999)).astype(F); out.append(a)
    return np.concatenate(out)


def fam_t_ranges(br, rng, n):
    """tmin < 0 (hits behind the origin count), tmax <= tmin (nothing), tmin = -inf / tmax = +inf, and NaN / inf components (nothing hits a ray
    with a NaN anywhere)"""
    base = fam_edge_random(br, rng, n)
    m = len(base)
    out = []
    a = base.copy(); a[:, 4:7] = -a[:, 4:7]; a[:, 3] = F(-1e30); out.append(a)                         # aimed away, hits behind the origin
    a = base.copy(); a[:, 3] = F(-np.inf); a[:, 7] = F(np.inf); out.append(a)
    a = base.copy(); a[:, 3] = rng.uniform(-2, 2, m).astype(F); a[:, 7] = a[:, 3]; out.append(a)         # tmax == tmin
    a = base.copy(); a[:, 3] = rng.uniform(0, 2, m).astype(F); a[:, 7] = (a[:, 3] - rng.uniform(0, 1, m)).astype(F); out.append(a)   # tmax < tmin
    for col in range(8):
        a = base[: max(1, m // 8)].copy(); a[:, col] = F(np.nan); out.append(a)
    for col in (0, 1, 2, 4, 5, 6):
        a = base[: max(1, m // 8)].copy(); a[:, col] = rng.choice([F(np.inf), F(-np.inf)], len(a)); out.append(a)
    a = base[: max(1, m // 8)].copy(); a[:, 4:7] = 0; out.append(a)                                     # zero direction
    return np.concatenate(out)


FAMILIES = dict(BASE_FAMILIES, t_edges=fam_t_edges, t_ranges=fam_t_ranges)


def family_rays(name, br, seed, n):
    return FAMILIES[name](br, np.random.default_rng(seed), n).astype(F)


# ---------------------------------------------------------------------------------------------------- scenes
_IDENT_Q = np.rint((np.array([0, 0, 0, 1], np.float32) * np.float32(0.5) + np.float32(0.5)) * np.float32(65535.0)).astype(np.uint16)


def _build_scene(meshes):
    """meshes: [(positions (V, 3), indices (3T,), 3x4 object-to-world or None, instance mask)] -> scene_io.Scene, one instance per mesh"""
    sc = scene_io.Scene()
    sc.materials = np.array([scene_io.pack_material(base_color=(0.7, 0.7, 0.7, 1), roughness=1.0, double_sided=True)], dtype=wire.MATERIAL)
    verts, inds, insts, xf, masks, ntris = [], [], [], [], [], []
    vb = ib = 0
    for P, I, M, mask in meshes:
        P = np.asarray(P, np.float32).reshape(-1, 3)
        I = np.asarray(I, np.uint32).reshape(-1)
        v = np.zeros(len(P), wire.VERTEX)
        v["pos"] = P
        v["normal"] = scene_io.encode_octahedral(np.tile(np.float32([[0, 1, 0]]), (len(P), 1)), sse_order=False)
        inst = np.zeros((), wire.MESH_INSTANCE)
        inst["base_vtx_offset"], inst["base_idx_offset"] = vb, ib
        inst["rotation"] = inst["prev_rotation"] = _IDENT_Q
        inst["scale"] = scene_io.f32_to_f16_bits([1, 1, 1])
        inst["prev_scale"] = inst["scale"]
        inst["mat_idx"] = 0
        inst["base_emissive_tri_offset"] = 0xFFFFFFFF
        inst["base_color_tex"] = 0xFFFF
        inst["alpha_factor_cutoff"] = 255 | (128 << 8)
        verts.append(v); inds.append(I); insts.append(inst)
        xf.append(np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]) if M is None else np.asarray(M, np.float32).reshape(12))
        masks.append(mask); ntris.append(len(I) // 3)
        vb += len(P); ib += len(I)
    sc.vertices = np.concatenate(verts)
    sc.indices = np.concatenate(inds)
    sc.instances = np.array(insts, dtype=wire.MESH_INSTANCE)
    sc.instance_to_world = np.array(xf, np.float32)
    sc.instance_mask = np.array(masks, np.uint8)
    sc.instance_num_tris = np.array(ntris, np.uint32)
    sc.rho, sc.rho_dim = scene_io.load_rho_default()
    return sc


def _grid(nu, nv, corner, du, dv):
    """a tessellated quad: (nu + 1) x (nv + 1) shared vertices, 2 nu nv triangles"""
    corner, du, dv = (np.asarray(x, np.float32) for x in (corner, du, dv))
    P = np.array([corner + (F(i) / F(nu)) * du + (F(j) / F(nv)) * dv for j in range(nv + 1) for i in range(nu + 1)], np.float32)
    I = []
    for j in range(nv):
        for i in range(nu):
            a = j * (nu + 1) + i
            I += [a, a + 1, a + nu + 2, a, a + nu + 2, a + nu + 1]
    return P, np.array(I, np.uint32)


def _fan(center, radius, n, y):
    P = [np.float32([center[0], y, center[1]])]
    for k in range(n):
        a = 2 * np.pi * k / n
        P.append(np.float32([center[0] + radius * np.cos(a), y + 0.15 * np.sin(3 * a), center[1] + radius * np.sin(a)]))
    I = []
    for k in range(n):
        I += [0, 1 + k, 1 + (k + 1) % n]
    return np.array(P, np.float32), np.array(I, np.uint32)


def make_seams_scene():
    """Seams and corners: tessellated axis-aligned walls (shared edges and vertices, edges on one plane), a triangle fan around a shared
    vertex, a duplicated instance (exact t ties between two global indices), zero-area triangles, an instance translated to 1e4 (node
    quantisation far from the origin), a scaled and rotated instance and a non-opaque instance."""
    ns = wire.SUBGROUP_NON_EMISSIVE
    meshes = []
    floor = _grid(6, 6, (-1, 0, -1), (2, 0, 0), (0, 0, 2))
    meshes.append((*floor, None, ns))
    meshes.append((*_grid(5, 4, (-1, 0, 1), (2, 0, 0), (0, 2, 0)), None, ns))                 # back wall z = 1
    meshes.append((*_grid(4, 5, (-1, 0, -1), (0, 0, 2), (0, 2, 0)), None, ns))                # left wall x = -1
    meshes.append((*_grid(3, 3, (0.25, 0, -0.75), (0, 0, 0.5), (0, 0.75, 0)), None, ns | wire.SUBGROUP_EMISSIVE))   # interior panel x = 0.25
    fan = _fan((-0.3, 0.2), 0.45, 12, 0.6)
    meshes.append((*fan, None, ns))
    meshes.append((*fan, None, ns))                                                            # the duplicate: same triangles, larger indices
    degen = np.float32([[0.5, 0.3, 0.5], [0.7, 0.3, 0.5], [0.9, 0.3, 0.5],                    # collinear
                        [0.6, 0.4, 0.6], [0.6, 0.4, 0.6], [0.6, 0.4, 0.6],                    # a point
                        [0.4, 0.2, 0.4], [0.4, 0.2, 0.4], [0.8, 0.6, 0.2]])                   # two equal vertices
    meshes.append((degen, np.arange(9, dtype=np.uint32), None, ns))
    far = scene_io.trs_matrix((1.0e4, 3.0, -1.0e4), (0, 0, 0, 1), (1, 1, 1))
    meshes.append((*_grid(3, 3, (-0.5, 0, -0.5), (1, 0, 0), (0, 0, 1)), far, ns))
    ang = 0.7
    q = np.float32([np.sin(ang / 2) * 0.6, np.sin(ang / 2) * 0.8, 0.0, np.cos(ang / 2)])
    rot = scene_io.trs_matrix((0.35, 0.9, 0.1), q, (0.3, 1.7, 0.8))
    box = _box_mesh()
    meshes.append((*box, rot, ns))
    meshes.append((*_grid(2, 2, (-0.6, 1.2, -0.6), (0.8, 0, 0), (0, 0, 0.8)), None, ns | wire.INSTANCE_NON_OPAQUE))
    return _build_scene(meshes)


def _box_mesh():
    c = np.float32([[-0.5, -0.5, -0.5], [0.5, -0.5, -0.5], [0.5, 0.5, -0.5], [-0.5, 0.5, -0.5],
                    [-0.5, -0.5, 0.5], [0.5, -0.5, 0.5], [0.5, 0.5, 0.5], [-0.5, 0.5, 0.5]])
    quads = [(0, 1, 2, 3), (5, 4, 7, 6), (4, 0, 3, 7), (1, 5, 6, 2), (3, 2, 6, 7), (4, 5, 1, 0)]
    I = []
    for a, b, cc, d in quads:
        I += [a, b, cc, a, cc, d]
    return c, np.array(I, np.uint32)


def make_tiny_scene():
    """8 triangles: the whole-scene-leaf path (no nodes).  Shared edges, a duplicate and an axis-aligned pair."""
    ns = wire.SUBGROUP_NON_EMISSIVE
    quad = _grid(1, 1, (-1, 0, -1), (2, 0, 0), (0, 0, 2))
    wall = _grid(1, 1, (-1, 0, 1), (2, 0, 0), (0, 2, 0))
    fan = _fan((0.0, 0.0), 0.5, 3, 0.8)
    return _build_scene([(*quad, None, ns), (*wall, None, ns), (*fan, None, ns | wire.SUBGROUP_EMISSIVE), (fan[0], fan[1][:3], None, ns)])


def moved_seams_scene(sc):
    """the seams scene with its rotated instance moved and turned (a new 3x4 for a device refit / rebuild); returns a copy"""
    s2 = scene_io.Scene()
    for k, v in vars(sc).items():
        if k != "_desc":
            setattr(s2, k, v.copy() if isinstance(v, np.ndarray) else v)
    k = len(s2.instances) - 2
    ang = 1.3
    q = np.float32([0.0, np.sin(ang / 2), np.sin(ang / 2) * 0.2, np.cos(ang / 2)])
    q /= np.float32(np.sqrt(np.float32(np.dot(q, q))))
    s2.instance_to_world[k] = scene_io.trs_matrix((0.1, 0.7, -0.2), q, (0.3, 1.7, 0.8)).reshape(12)
    return s2, k


def cornell_scene():
    return scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_emissive.npz"))


SCENES = {
    "cornell": cornell_scene,
    "synthetic": lambda: scene_io.make_synthetic_scene(num_tris=3000, num_emissive=64, seed=3),
    "seams": make_seams_scene,
    "tiny": make_tiny_scene,
}


# ---------------------------------------------------------------------------------------------------- the claim of zr_intersect.h
# the condition: |o - v0| / |cos| <= COND_REACH x s and |cos| >= COND_MIN_COS, s = the hit triangle's largest |coordinate| (its pad is 2^-16 s)
COND_REACH = 64.0
COND_MIN_COS = 1e-3
# Outside the condition (measured over ~3 M rays of these families, both trees: at most 2.5 % behind on grazing rays, and 14 of 34 470
# rays losing their hit, the worst family):
CLOSEST_SLACK = 5e-2             # returned t - brute-force t <= CLOSEST_SLACK x |t| + 1e-3
OUTSIDE_LOSS = 2e-3              # rays whose brute-force hit the tree loses entirely (closest or any hit): <= OUTSIDE_LOSS x rays outside + 2


def in_condition(br, rays, tri):
    """rays whose brute-force hit triangle `tri` (-1: no hit) satisfies the stated condition of zr_intersect.h"""
    ok = tri >= 0
    k = np.where(ok, tri, 0)
    v0, e1, e2 = br.v0[k].astype(np.float64), br.e1[k].astype(np.float64), br.e2[k].astype(np.float64)
    P = np.stack([v0, v0 + e1, v0 + e2], 1)
    s = np.abs(P).max((1, 2))
    n = np.cross(e1, e2)
    d = rays[:, 4:7].astype(np.float64)
    with np.errstate(all="ignore"):
        cos = np.abs((n * d).sum(1)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d, axis=1))
        reach = np.linalg.norm(rays[:, 0:3].astype(np.float64) - v0, axis=1) / cos
    return ok & np.isfinite(rays).all(1) & (cos >= COND_MIN_COS) & (reach <= COND_REACH * s)


def check_against_brute(br, rays, got_closest, got_any, mask, label):
    """One batch of tree answers against brute force.  Inside the condition (and for every ray brute force calls a miss): equal bit for bit,
    closest and any hit.  Everywhere: any hit never reports an occlusion brute force does not see.  Outside the condition: a returned hit is
    one zr_ray_tri accepts (its t, its mask), at most CLOSEST_SLACK behind the brute-force hit; any hit is occluded whenever the same tree's
    closest hit found a triangle; and the rays whose brute-force hit is lost entirely -- closest hit a miss, or any hit unoccluded, a light
    leak -- are at most OUTSIDE_LOSS of the rays outside.  Returns (rays inside, rays outside, closest-hit losses, any-hit leaks)."""
    want = br.closest(rays, mask)
    want_any = br.any(rays, mask)
    tri = np.where(want[:, 3] != MISS, want[:, 3].astype(np.int64), -1)
    cond = in_condition(br, rays, tri) | (tri < 0)
    bad = np.nonzero(cond & (got_closest != want).any(1))[0]
    assert len(bad) == 0, f"{label}: {len(bad)} closest hits differ inside the condition, e.g. ray {rays[bad[0]].view(np.uint32)}: " \
                          f"brute {want[bad[0]]} tree {got_closest[bad[0]]}"
    leak = np.nonzero(cond & (want_any != got_any))[0]
    assert len(leak) == 0, f"{label}: {len(leak)} any-hit answers differ inside the condition, e.g. ray {rays[leak[0]].view(np.uint32)}"
    extra = np.nonzero((got_any == 1) & (want_any == 0))[0]
    assert len(extra) == 0, f"{label}: any hit reports {len(extra)} occlusions brute force does not see, e.g. ray {rays[extra[0]].view(np.uint32)}"
    out = np.nonzero(~cond)[0]
    lost = leaks = 0
    if len(out):
        g = got_closest[out]
        hit = g[:, 3] != MISS
        acc, t = br.accepts(rays[out][hit], g[hit, 3].astype(np.int64))
        assert acc.all(), f"{label}: the tree returned a hit zr_ray_tri does not accept"
        assert np.array_equal(t.view(np.uint32), g[hit, 0]), f"{label}: returned t is not zr_ray_tri's"
        assert np.all(br.mask[g[hit, 3]] & mask), f"{label}: returned a triangle outside the mask"
        tw = want[out][hit, 0].view(np.float32).astype(np.float64)
        tg = g[hit, 0].view(np.float32).astype(np.float64)
        assert np.all(tg - tw <= CLOSEST_SLACK * np.abs(tw) + 1e-3), f"{label}: a returned hit lies too far behind the brute-force hit"
        assert np.all(got_any[out][hit] == 1), f"{label}: any-hit says unoccluded where the tree's own closest hit found a triangle"
        # (every ray outside the condition has a brute-force hit: a brute-force miss counts as inside)
        lost = int((~hit).sum())
        leaks = int(((want_any[out] == 1) & (got_any[out] == 0)).sum())
        assert lost <= OUTSIDE_LOSS * len(out) + 2, f"{label}: {lost} of {len(out)} rays outside the condition lose their brute-force hit"
        assert leaks <= OUTSIDE_LOSS * len(out) + 2, f"{label}: {leaks} of {len(out)} any-hit rays outside the condition leak"
    return int(cond.sum()), len(out), lost, leaks
