/*
 * zr_skin.h -- linear blend skinning of glTF meshes, stated once for the host and the device.
 *
 * glTF 2.0 section 3.7.3: a skinned vertex is moved by the weighted sum of its (up to four) joint matrices, a joint matrix being the joint node's world
 * matrix times the joint's inverse bind matrix.  zr_scene_io.cpp (zrh_skin_pose, the host form, and the loader's check of its tables), zr_api.hip
 * (the setter's check), tests/skinmath and zr_tu_pose.hip (zr_scene_animate with a skin set) all compile these functions; under the arithmetic contract of zr_detmath.h (+ - * / sqrt fma, round to nearest
 * even, -ffp-contract=off) they give the same bytes.  Every fma below is written; nothing else is fused.
 *
 * Matrices are 3 x 4 row-major in the column-vector convention (zr_scene_desc.instance_to_world, the node matrices of zr_anim.h): M[4 r + c].
 *
 *   joint matrix   J = nodeWorld x inverse_bind: zran::ComposeWorld(inverse_bind, nodeWorld), i.e. zr_anim.h's Mul on the two matrices -- per entry
 *                  fma(a1, b1, a0 b0) + fma(a3, b3, a2 b2), three roundings on the longest path
 *   blend          M[e] = fma(w3, J3[e], fma(w2, J2[e], fma(w1, J1[e], w0 * J0[e]))) for each of the 12 entries: the sum in the order j = 0, 1, 2, 3,
 *                  four roundings.  A slot with weight 0 adds +-0 (its joint matrix is finite: the setter checks), so it may name any valid joint
 *   position       p' = M (p, 1) = zrsm::MulPoint: fma(1, M3, fma(z, M2, fma(y, M1, x * M0))) per row, four more roundings
 *   normal         n' = normalize(cof(M3) n), n = DecodeOct32(code), re-encoded with zrsm::EncodeOct32.  cof(M3), the cofactor matrix of the upper 3 x 3,
 *                  has the rows r1 x r2, r2 x r0, r0 x r1 (r_i the rows of M3; each cross product component a * b - c * d, two products and a
 *                  difference); it is det(M3) times the inverse transpose, so non-uniform scale is handled.  The dot products and the squared length
 *                  are fma(c2, n2, fma(c1, n1, c0 * n0)); normalize is v * (1 / sqrt(|v|^2)).
 *                  The caller guarantees det(M3) > 0 (like the "positive scale" guarantee of zr_anim.h).  With det <= 0 -- or a zero normal -- the two
 *                  code words are unspecified; nothing else is.
 *   tangent        t' = normalize(M3 t), t = DecodeOct32(code): rows fma(t2, M[4 r + 2], fma(t1, M[4 r + 1], t0 * M[4 r])), re-encoded
 *   uv             copied
 *   hit tables     the VtxDir entries (zr_hit_tables.h) of a posed vertex are DecodeOct32 of the STORED codes: DecodeOct32 below is, operation for
 *                  operation, zr::DecodeOct32 of zr_dev_math.h, the expression k_fill_vtx_normals evaluates and a hit would otherwise compute
 */
#ifndef ZR_SKIN_H
#define ZR_SKIN_H

#include "zr_detmath.h"
#include "zr_wire.h"
#include "zr_scene_math.h"
#include "zr_anim.h"
#include <stdio.h>
#include <vector>

namespace zrsk {

/* zr::DecodeOct32 (zr_dev_math.h; Math.hlsli:646-658) on the two code words */
ZR_HD void DecodeOct32(const uint16_t* e, float* n)
{
    const float ux = zr_fma(zr_div65535((float)e[0]), 2.0f, -1.0f), uy = zr_fma(zr_div65535((float)e[1]), 2.0f, -1.0f);
    const float z = 1.0f - zr_abs(ux) - zr_abs(uy);
    const float t = zr_saturate(-z);
    const float x = ux + ((ux >= 0.0f) ? -t : t), y = uy + ((uy >= 0.0f) ? -t : t);
    const float inv = 1.0f / zr_sqrt(x * x + y * y + z * z);
    n[0] = x * inv; n[1] = y * inv; n[2] = z * inv;
}

ZR_HD void JointMatrix(const float* nodeWorld, const float* inverseBind, float* J) { zran::ComposeWorld(inverseBind, nodeWorld, J); }

ZR_HD void Blend(const float* J0, const float* J1, const float* J2, const float* J3, const float* w, float* M)
{
    ZR_UNROLL
    for (int e = 0; e < 12; e++) M[e] = zr_fma(w[3], J3[e], zr_fma(w[2], J2[e], zr_fma(w[1], J1[e], w[0] * J0[e])));
}

ZR_HD float Dot3(const float* a, const float* b) { return zr_fma(a[2], b[2], zr_fma(a[1], b[1], a[0] * b[0])); }
ZR_HD void Normalize3(const float* v, float* out)
{
    const float inv = 1.0f / zr_sqrt(Dot3(v, v));
    ZR_UNROLL
    for (int k = 0; k < 3; k++) out[k] = v[k] * inv;
}
/* normalize(cof(M3) n) */
ZR_HD void Normal(const float* M, const float* n, float* out)
{
    float v[3];
    ZR_UNROLL
    for (int i = 0; i < 3; i++)
    {
        const float* a = M + 4 * ((i + 1) % 3);
        const float* b = M + 4 * ((i + 2) % 3);
        const float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        v[i] = Dot3(c, n);
    }
    Normalize3(v, out);
}
/* normalize(M3 t) */
ZR_HD void Tangent(const float* M, const float* t, float* out)
{
    float v[3];
    ZR_UNROLL
    for (int r = 0; r < 3; r++) v[r] = zr_fma(t[2], M[4 * r + 2], zr_fma(t[1], M[4 * r + 1], t[0] * M[4 * r]));
    Normalize3(v, out);
}

/* one vertex: the rest-pose record and the blended matrix give the posed record */
ZR_HD void PoseVertex(const zr_vertex& rest, const float* M, zr_vertex& out)
{
    float n[3], t[3], pn[3], pt[3];
    zrsm::MulPoint(M, rest.pos, out.pos);
    out.uv[0] = rest.uv[0]; out.uv[1] = rest.uv[1];
    DecodeOct32(rest.normal, n); Normal(M, n, pn); zrsm::EncodeOct32(pn, out.normal);
    DecodeOct32(rest.tangent, t); Tangent(M, t, pt); zrsm::EncodeOct32(pt, out.tangent);
}
/* ... from its influence record and the joint matrices (numJoints x 12 floats; every index in range: ValidateSkin) */
ZR_HD void SkinVertex(const zr_vertex& rest, const zr_skin_influence& f, const float* jointMatrices, zr_vertex& out)
{
    float M[12];
    Blend(jointMatrices + 12 * (size_t)f.joint[0], jointMatrices + 12 * (size_t)f.joint[1], jointMatrices + 12 * (size_t)f.joint[2],
        jointMatrices + 12 * (size_t)f.joint[3], f.weight, M);
    PoseVertex(rest, M, out);
}

/* ---- host side: the whole set.  nodeWorld: the node matrices of zran::EvalNodeWorlds; J: num_joints x 12 floats */
static inline void EvalJointMatrices(const zr_skin_desc& d, const float* nodeWorld, float* J)
{
    for (uint32_t j = 0; j < d.num_joints; j++) JointMatrix(nodeWorld + 12 * (size_t)d.joints[j].node, d.joints[j].inverse_bind, J + 12 * (size_t)j);
}
/* rest: the rest-pose records of the listed ranges, range after range; out: the posed ones in the same order */
static inline void SkinRanges(const zr_skin_desc& d, const float* J, const zr_vertex* rest, zr_vertex* out)
{
    size_t k = 0;
    for (uint32_t r = 0; r < d.num_ranges; r++)
        for (uint32_t v = 0; v < d.ranges[r].num_vertices; v++, k++) SkinVertex(rest[k], d.influences[d.ranges[r].first_influence + (size_t)v], J, out[k]);
}
/* What zr_scene_set_skinning refuses (ZR_ERR_INVALID_ARG): returns 0, or -1 with a message */
static inline int ValidateSkin(const zr_skin_desc& d, uint32_t animNodes, uint32_t sceneVertices, char* msg, size_t cap)
{
#define ZRSK_FAIL(...) do { snprintf(msg, cap, __VA_ARGS__); return -1; } while (0)
    if ((d.num_joints && !d.joints) || (d.num_ranges && !d.ranges) || (d.num_influences && !d.influences)) ZRSK_FAIL("null table with a non-zero count");
    if (d.num_joints > 65535u) ZRSK_FAIL("%u joints: an influence's 16-bit index reaches 65 535", d.num_joints);
    for (uint32_t j = 0; j < d.num_joints; j++)
    {
        if (d.joints[j].node >= animNodes) ZRSK_FAIL("joint %u: node %u, the animation has %u", j, d.joints[j].node, animNodes);
        for (int k = 0; k < 12; k++) if (!zran::Finite(d.joints[j].inverse_bind[k])) ZRSK_FAIL("joint %u: the inverse bind matrix is not finite", j);
    }
    std::vector<uint8_t> covered(sceneVertices, 0);
    for (uint32_t r = 0; r < d.num_ranges; r++)
    {
        const zr_skin_range& g = d.ranges[r];
        if ((uint64_t)g.first_vertex + g.num_vertices > sceneVertices) ZRSK_FAIL("range %u: vertices [%u, %llu), the scene has %u", r, g.first_vertex, (unsigned long long)g.first_vertex + g.num_vertices, sceneVertices);
        if ((uint64_t)g.first_influence + g.num_vertices > d.num_influences) ZRSK_FAIL("range %u: influences [%u, %llu), the table has %u", r, g.first_influence, (unsigned long long)g.first_influence + g.num_vertices, d.num_influences);
        for (uint32_t v = 0; v < g.num_vertices; v++)
        {
            if (covered[g.first_vertex + v]) ZRSK_FAIL("range %u overlaps an earlier range at vertex %u", r, g.first_vertex + v);
            covered[g.first_vertex + v] = 1;
        }
    }
    for (uint32_t i = 0; i < d.num_influences; i++)
        for (int k = 0; k < 4; k++)
        {
            if (d.influences[i].joint[k] >= d.num_joints) ZRSK_FAIL("influence %u: joint %u, the table has %u", i, d.influences[i].joint[k], d.num_joints);
            if (!zran::Finite(d.influences[i].weight[k])) ZRSK_FAIL("influence %u: a weight is not finite", i);
        }
#undef ZRSK_FAIL
    return 0;
}

} /* namespace zrsk */

#endif /* ZR_SKIN_H */
