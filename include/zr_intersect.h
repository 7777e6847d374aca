/*
 * zr_intersect.h -- the ray/triangle and ray/box arithmetic of the zetaray_amd C-ABI.
 *
 * In the reference, BVH traversal and ray/triangle intersection happen inside the D3D12 driver / RT hardware
 * (DXR 1.1 inline RayQuery: Source/ZetaRenderPass/Common/RayQuery.hlsli:42-53, 168-179, 317-331, 372-396;
 * GBuffer/GBufferRT_Inline.hlsl:72-95); their arithmetic is opaque and unpinned by any reference test.  Only the
 * semantics are defined: closest hit / any hit with TMin < t < TMax over world-space triangles.  This ABI pins the
 * arithmetic instead (SURVEY.md section 7 "Hard parts"): Moeller-Trumbore in the form below, no face culling, hit
 * accepted iff tmin < t < tmax, ties on t broken towards the smaller global triangle index.  Both the HIP kernels
 * and the CPU oracle call these two functions; everything around them (BVH layout, traversal order) is free,
 * because "closest hit with this tie-break" and "any hit" do not depend on traversal order -- nor on the tree, for rays within the
 * condition stated below (the box tests are conservative only that far).
 *
 * World-space triangles are stored as (v0, e1 = v1 - v0, e2 = v2 - v0), computed once on the host from the
 * instance's float 3x4 object-to-world matrix (row . (p, 1), summed left to right).
 */
#ifndef ZR_INTERSECT_H
#define ZR_INTERSECT_H

#include "zr_detmath.h"

/* returns 1 on hit and writes t, u (weight of v1), v (weight of v2) -- DXR barycentric convention */
ZR_HD int zr_ray_tri(float ox, float oy, float oz, float dx, float dy, float dz,
                     float v0x, float v0y, float v0z, float e1x, float e1y, float e1z,
                     float e2x, float e2y, float e2z, float tmin, float tmax,
                     float* t_out, float* u_out, float* v_out)
{
    /* p = d x e2 */
    float px = dy * e2z - dz * e2y;
    float py = dz * e2x - dx * e2z;
    float pz = dx * e2y - dy * e2x;
    float det = e1x * px + e1y * py + e1z * pz;
    if (det == 0.0f) return 0;
    float inv = 1.0f / det;
    float tx = ox - v0x, ty = oy - v0y, tz = oz - v0z;
    float u = (tx * px + ty * py + tz * pz) * inv;
    if (!(u >= 0.0f && u <= 1.0f)) return 0;
    /* q = tv x e1 */
    float qx = ty * e1z - tz * e1y;
    float qy = tz * e1x - tx * e1z;
    float qz = tx * e1y - ty * e1x;
    float v = (dx * qx + dy * qy + dz * qz) * inv;
    if (!(v >= 0.0f && (u + v) <= 1.0f)) return 0;
    float t = (e2x * qx + e2y * qy + e2z * qz) * inv;
    if (!(t > tmin && t < tmax)) return 0;
    *t_out = t; *u_out = u; *v_out = v;
    return 1;
}

/*
 * ---- What makes a box test conservative with respect to zr_ray_tri ----
 * zr_ray_tri is not exact: near an edge or vertex it accepts rays whose exact path passes slightly outside the triangle, and its t carries a
 * relative error.  Its error grows with the distance between ray origin and triangle and with 1 / |cos| (angle between ray and face).  So a box
 * that holds the triangle exactly is not enough; three things cover the error:
 *   1. every triangle's box is padded on every axis by ZR_TRI_PAD_REL x (the largest |coordinate| of the triangle's box) + ZR_TRI_PAD_ABS
 *      (zr_tri_bounds; every tree builder uses it: the host SAH build, the device LBVH and refit, and the oracle's BVH2).
 *      The absolute term matters for a coordinate of exactly 0.  The slab test clamps |1/d| to 1e30, so an origin that lies within a box's
 *      plane sees the slab end at (pad x 1e30) instead of at infinity.  A one-ulp pad at 0 is a denormal and would end the slab near t = 1e-15.
 *   2. the exit distance tf is widened by 3 ulp-ish of |tf| in either sign (zr_widen_far).  Scaling by (1 + eps) would shrink a negative tf.
 *   3. the traversal's entry-distance cull uses the same widening.
 * The stated condition, which tests/test_ray_queries_cpu.py and tests/test_ray_queries_gpu.py check: let v0 and s be the vertex 0 and the largest
 * |coordinate| of the triangle that brute force hits.  If |o - v0| / |cos| <= 2^6 x s and |cos| >= 1e-3 (cos between ray and face), then no
 * box test rejects a triangle that zr_ray_tri accepts.  So the closest hit with the index tie-break, and any hit, do not depend on the tree.
 * Outside the condition the answer MAY depend on the tree, and a query may miss a triangle that zr_ray_tri accepts: closest hit can return a
 * farther triangle or no hit at all, and any hit can report unoccluded (a light leak).  What still holds there: every hit returned is one
 * zr_ray_tri accepts, any hit never reports an occlusion that brute force does not see, and any hit is occluded whenever the same tree's
 * closest hit finds a triangle.  The tests also bound how often outside rays lose their hit (tests/raycheck.py OUTSIDE_LOSS, CLOSEST_SLACK).
 * Rays outside are far from the triangle they hit relative to its coordinates, or graze it: no build-time pad can cover an error that grows
 * with the ray's own origin distance / |cos|, and a larger pad costs traversal time (2^-12 instead of 2^-16 measured 0.6 % slower).
 */
#define ZR_TRI_PAD_REL 1.52587890625e-05f      /* 2^-16 (2^-12 measured 0.6 % slower on the Cornell ReSTIR PT frame) */
#define ZR_TRI_PAD_ABS 8.673617379884035e-19f  /* 2^-60 */
#define ZR_BOX_WIDEN 3.5762786865234375e-07f   /* 3 x 2^-23: fma(|tf|, w, tf) equals the old tf * (1 + 3 x 2^-23) for every tf >= 0 */

/* exit-distance widening of the box tests, symmetric in the sign of tf (one fma; |.| is a source modifier on the device) */
ZR_HD float zr_widen_far(float tf) { return __builtin_fmaf(__builtin_fabsf(tf), ZR_BOX_WIDEN, tf); }

/* padded box of one stored triangle (v0, e1, e2): what every BVH builder puts around a triangle (see above) */
ZR_HD void zr_tri_bounds(const float v0[3], const float e1[3], const float e2[3], float lo[3], float hi[3])
{
    float s = 0.0f;
    for (int r = 0; r < 3; r++)
    {
        const float a = v0[r], b = v0[r] + e1[r], c = v0[r] + e2[r];
        lo[r] = zr_min(a, zr_min(b, c)); hi[r] = zr_max(a, zr_max(b, c));
        s = zr_max(s, zr_max(zr_abs(lo[r]), zr_abs(hi[r])));
    }
    /* pad >= 2^-16 |coordinate| is >= 128 ulp of every coordinate, so rounding lo - pad / hi + pad to nearest keeps the box outward */
    const float pad = s * ZR_TRI_PAD_REL + ZR_TRI_PAD_ABS;
    for (int r = 0; r < 3; r++) { lo[r] = lo[r] - pad; hi[r] = hi[r] + pad; }
}

/* reciprocal direction for the slab test; |d| is clamped to 1e-30 so 0 * inf never produces a NaN */
ZR_HD float zr_safe_rcp_dir(float d)
{
    if (zr_abs(d) < 1e-30f) d = (zr_asuint(d) & 0x80000000u) ? -1e-30f : 1e-30f;
    return 1.0f / d;
}

/*
 * Slab test.  idx/idy/idz = zr_safe_rcp_dir(d).  The exit distance is widened by 3 ulp-ish of |tf| (zr_widen_far); together with the
 * padded triangle boxes (zr_tri_bounds) this never rejects a triangle zr_ray_tri accepts, within the condition stated above.
 * Returns 1 if [tmin, tmax] overlaps the box interval; writes the entry distance (for ordered traversal only).
 */
ZR_HD int zr_ray_box(float ox, float oy, float oz, float idx, float idy, float idz,
                     float bminx, float bminy, float bminz, float bmaxx, float bmaxy, float bmaxz,
                     float tmin, float tmax, float* t_entry)
{
    float t0x = (bminx - ox) * idx, t1x = (bmaxx - ox) * idx;
    float t0y = (bminy - oy) * idy, t1y = (bmaxy - oy) * idy;
    float t0z = (bminz - oz) * idz, t1z = (bmaxz - oz) * idz;
    /* NaN (0 * inf) compares false and drops out of min/max, which is the conservative choice here */
    float nx = zr_min(t0x, t1x), fx = zr_max(t0x, t1x);
    float ny = zr_min(t0y, t1y), fy = zr_max(t0y, t1y);
    float nz = zr_min(t0z, t1z), fz = zr_max(t0z, t1z);
    float tn = zr_max(zr_max(nx, ny), zr_max(nz, tmin));
    float tf = zr_min(zr_min(fx, fy), zr_min(fz, tmax));
    tf = zr_widen_far(tf);
    *t_entry = tn;
    return tn <= tf;
}

/*
 * The same test with the machine's own min / max (v_min_f32 / v_max_f32 on gfx950, which fuse to the three-operand
 * forms): what BVH traversal uses.  A box test only selects candidates -- closest hit with the index tie-break and any
 * hit do not depend on which conservative test produced them -- so unlike zr_ray_tri its arithmetic is not part of the
 * parity contract; it only has to never reject a box whose triangle zr_ray_tri would accept (same widening and condition as above).
 */
ZR_HD int zr_ray_box_native(float ox, float oy, float oz, float idx, float idy, float idz,
                            float bminx, float bminy, float bminz, float bmaxx, float bmaxy, float bmaxz,
                            float tmin, float tmax, float* t_entry)
{
    float t0x = (bminx - ox) * idx, t1x = (bmaxx - ox) * idx;
    float t0y = (bminy - oy) * idy, t1y = (bmaxy - oy) * idy;
    float t0z = (bminz - oz) * idz, t1z = (bmaxz - oz) * idz;
    float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t0x, t1x), __builtin_fminf(t0y, t1y)), __builtin_fmaxf(__builtin_fminf(t0z, t1z), tmin));
    float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t0x, t1x), __builtin_fmaxf(t0y, t1y)), __builtin_fminf(__builtin_fmaxf(t0z, t1z), tmax));
    tf = zr_widen_far(tf);
    *t_entry = tn;
    return tn <= tf;
}

#endif /* ZR_INTERSECT_H */
