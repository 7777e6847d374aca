/*
 * zr_scene_math.h -- the per-frame scene math of a dynamic scene, stated once for the host and the device.
 *
 * What TLAS::FillMeshInstanceData (RtAccelerationStructure.cpp:318-380) and SceneCore::UpdateEmissivePositions (SceneCore.cpp:913-955) compute
 * for an instance that moves: the decomposition of its world matrix into the quantised MeshInstance fields, and its EmissiveTriangle records
 * re-derived from the object-space ones.  zr_scene_io.cpp (zrh_scene_data_set_instance_world, the host form) and zr_tu_scene_update.hip
 * (zr_scene_move_instances, the device form) both compile these functions; the operation order is the reference's SSE code's, and under the
 * arithmetic contract of zr_detmath.h (+ - * / sqrt fma, round to nearest even, -ffp-contract=off) the two give the same bytes.
 */
#ifndef ZR_SCENE_MATH_H
#define ZR_SCENE_MATH_H

#include "zr_detmath.h"
#include "zr_wire.h"

namespace zrsm {

/* float -> integer-valued float, round to nearest even (cvtps_epi32 / v_rndne_f32) */
ZR_HD float RoundEven(float x) { return __builtin_rintf(x); }

/* Math::encode_octahedral (VectorFuncs.h:134-153) + unorm2::FromNormalized (Vector.h:626-647), in the SSE code's operation order:
   |x| + |z| first, then + |y| (hadd_float3); the fold's sign comes from the INPUT component (v >= 0, so -0.0 counts as positive);
   [-1, 1] -> [0, 1] is one fma; cvtps_epi32 rounds to nearest even */
ZR_HD void EncodeOct32(const float* n, uint16_t out[2])
{
    const float denom = (zr_abs(n[0]) + zr_abs(n[2])) + zr_abs(n[1]);
    const float p[2] = {n[0] / denom, n[1] / denom};
    ZR_UNROLL
    for (int k = 0; k < 2; k++)
    {
        const float sgn = n[k] >= 0.0f ? 1.0f : -1.0f;
        const float folded = (1.0f - zr_abs(p[1 - k])) * sgn;
        const float enc = n[2] <= 0.0f ? folded : p[k];
        out[k] = (uint16_t)RoundEven(zr_fma(enc, 0.5f, 0.5f) * 65535.0f);
    }
}

/* Row-vector 4 x 4 as the reference stores it: rows 0-2 = images of the basis vectors, row 3 = translation.  Only [i][0..2] is kept. */
struct Mat43 { float m[4][3]; };
/* 3 x 4 row-major, column-vector convention (zr_scene_desc.instance_to_world) -> reference layout */
ZR_HD Mat43 FromToWorld(const float* M)
{
    Mat43 r;
    ZR_UNROLL
    for (int i = 0; i < 3; i++) { ZR_UNROLL for (int j = 0; j < 3; j++) r.m[i][j] = M[4 * j + i]; }
    ZR_UNROLL
    for (int j = 0; j < 3; j++) r.m[3][j] = M[4 * j + 3];
    return r;
}

/* decomposeSRT, MatrixFuncs.h:562-610 + quaternionFromRotationMat1, :410-437 */
ZR_HD void DecomposeSRT(const Mat43& M, float s[3], float q[4], float t[3])
{
    ZR_UNROLL
    for (int j = 0; j < 3; j++) t[j] = M.m[3][j];
    float R[3][3];
    ZR_UNROLL
    for (int i = 0; i < 3; i++)
    {
        /* diagonal of M M^T through mul(): (m0 m0 + m1 m1) + (m2 m2 + 0 0) */
        const float s2 = zr_fma(M.m[i][1], M.m[i][1], M.m[i][0] * M.m[i][0]) + zr_fma(0.0f, 0.0f, M.m[i][2] * M.m[i][2]);
        s[i] = zr_sqrt(s2);
        const float inv = 1.0f / s[i];
        ZR_UNROLL
        for (int j = 0; j < 3; j++) R[i][j] = inv * M.m[i][j];
    }
    float tt[4];
    tt[0] = 1 + R[0][0] - R[1][1] - R[2][2];
    tt[1] = 1 - R[0][0] + R[1][1] - R[2][2];
    tt[2] = 1 - R[0][0] - R[1][1] + R[2][2];
    tt[3] = 1 + R[0][0] + R[1][1] + R[2][2];
    const float a = R[0][1] + R[1][0], b = R[2][0] + R[0][2], c = R[1][2] - R[2][1], d = R[1][2] + R[2][1], e = R[2][0] - R[0][2], f = R[0][1] - R[1][0];
    /* the row of the symmetric 4 x 4 that has the largest diagonal element: i = 0 / 1 / 2 when R00 / R11 / R22 dominates, 3 for the trace */
    const int i = (R[2][2] >= 0) * (2 + (R[0][0] >= -R[1][1])) + (R[2][2] < 0) * (R[1][1] >= R[0][0]);
    float row[4], ti;
    if (i == 0) { row[0] = tt[0]; row[1] = a; row[2] = b; row[3] = c; ti = tt[0]; }
    else if (i == 1) { row[0] = a; row[1] = tt[1]; row[2] = d; row[3] = e; ti = tt[1]; }
    else if (i == 2) { row[0] = b; row[1] = d; row[2] = tt[2]; row[3] = f; ti = tt[2]; }
    else { row[0] = c; row[1] = e; row[2] = f; row[3] = tt[3]; ti = tt[3]; }
    const float k = 0.5f / zr_sqrt(ti);
    ZR_UNROLL
    for (int j = 0; j < 4; j++) q[j] = row[j] * k;
    /* float4::normalize: _mm_dp_ps sums (x^2 + y^2) + (z^2 + w^2) */
    const float norm = zr_sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    const float inv = 1.0f / norm;
    ZR_UNROLL
    for (int j = 0; j < 4; j++) q[j] *= inv;
}
/* unorm4::FromNormalized (Vector.h:745-769): fma(v, 0.5, 0.5) * 65535, round to nearest even */
ZR_HD uint16_t Unorm16FromNormalized(float v) { return (uint16_t)RoundEven(zr_fma(v, 0.5f, 0.5f) * 65535.0f); }

/* ---- the MeshInstance record of a frame (TLAS::FillMeshInstanceData) */
/* a mesh at rest */
ZR_HD void FillMeshInstance(const float* toWorld, zr_mesh_instance& I)
{
    float s[3], q[4], t[3];
    DecomposeSRT(FromToWorld(toWorld), s, q, t);
    ZR_UNROLL
    for (int k = 0; k < 4; k++) I.rotation[k] = I.prev_rotation[k] = Unorm16FromNormalized(q[k]);
    ZR_UNROLL
    for (int k = 0; k < 3; k++) { I.scale[k] = I.prev_scale[k] = zr_f32_to_f16(s[k]); I.translation[k] = t[k]; I.d_translation[k] = zr_f32_to_f16(0.0f); }
}
/* an instance that does not move this frame: Prev* = current, dTranslation = 0 */
ZR_HD void InstanceBeginFrame(zr_mesh_instance& I)
{
    ZR_UNROLL
    for (int k = 0; k < 4; k++) I.prev_rotation[k] = I.rotation[k];
    ZR_UNROLL
    for (int k = 0; k < 3; k++) { I.prev_scale[k] = I.scale[k]; I.d_translation[k] = zr_f32_to_f16(0.0f); }
}
/* ... and one that moves, the !staticMesh branch (RtAccelerationStructure.cpp:318-380): current and previous S / R / T by decomposeSRT of the two
   world matrices, dTranslation = half3(t - t_prev) */
ZR_HD void InstanceSetWorld(zr_mesh_instance& I, const float* world, const float* prevWorld)
{
    float sc[3], q[4], t[3], sp[3], qp[4], tp[3];
    DecomposeSRT(FromToWorld(world), sc, q, t);
    DecomposeSRT(FromToWorld(prevWorld), sp, qp, tp);
    ZR_UNROLL
    for (int k = 0; k < 4; k++) { I.rotation[k] = Unorm16FromNormalized(q[k]); I.prev_rotation[k] = Unorm16FromNormalized(qp[k]); }
    ZR_UNROLL
    for (int k = 0; k < 3; k++)
    { I.scale[k] = zr_f32_to_f16(sc[k]); I.prev_scale[k] = zr_f32_to_f16(sp[k]); I.translation[k] = t[k]; I.d_translation[k] = zr_f32_to_f16(t[k] - tp[k]); }
}

/* ---- EmissiveTriangle records */
/* RT::EmissiveTriangle::StoreVertices (RtCommon.h:141-198): vertex 0 + the two edges as 16-bit octahedral directions and half lengths.
   A zero-length edge divides by zero: the bytes it yields are unspecified (the loader never produces one) */
ZR_HD void StoreEmissiveVertices(zr_emissive_triangle& e, const float* v0, const float* v1, const float* v2)
{
    float e0[3], e1[3];
    ZR_UNROLL
    for (int k = 0; k < 3; k++) { e.vtx0[k] = v0[k]; e0[k] = v1[k] - v0[k]; e1[k] = v2[k] - v0[k]; }
    const float l0 = zr_sqrt((e0[0] * e0[0] + e0[1] * e0[1]) + (e0[2] * e0[2] + 0.0f)), l1 = zr_sqrt((e1[0] * e1[0] + e1[1] * e1[1]) + (e1[2] * e1[2] + 0.0f));
    const float n0[3] = {e0[0] / l0, e0[1] / l0, e0[2] / l0}, n1[3] = {e1[0] / l1, e1[1] / l1, e1[2] / l1};
    EncodeOct32(n0, e.v0v1); EncodeOct32(n1, e.v0v2);
    e.edge_lengths[0] = zr_f32_to_f16(l0); e.edge_lengths[1] = zr_f32_to_f16(l1);
}
/* RT::EmissiveTriangle::DecodeVertices (RtCommon.h:200-234) with Math::decode_octahedral (VectorFuncs.h:155-174) and normalize (:64-70: dpps sums
   (x^2 + y^2) + (z^2 + 0)), in the SSE code's operation order */
ZR_HD void DecodeEmissiveVertices(const zr_emissive_triangle& e, float* v0, float* v1, float* v2)
{
    const uint16_t enc[4] = {e.v0v1[0], e.v0v1[1], e.v0v2[0], e.v0v2[1]};
    float u[4];
    ZR_UNROLL
    for (int k = 0; k < 4; k++) u[k] = zr_fma(zr_div65535((float)(int32_t)enc[k]), 2.0f, -1.0f);
    const float len[2] = {zr_f16_to_f32(e.edge_lengths[0]), zr_f16_to_f32(e.edge_lengths[1])};
    ZR_UNROLL
    for (int j = 0; j < 2; j++)
    {
        float* out = j == 0 ? v1 : v2;
        const float ux = u[2 * j], uy = u[2 * j + 1];
        const float z = 1.0f - (zr_abs(ux) + zr_abs(uy));
        const float nz = 0.0f - z, posT = nz < 0.0f ? 0.0f : (nz > 1.0f ? 1.0f : nz), negT = 0.0f - posT;      /* saturate(negate(z)), negate */
        const float dx = ux + (ux >= 0.0f ? negT : posT), dy = uy + (uy >= 0.0f ? negT : posT);
        const float n = zr_sqrt((dx * dx + dy * dy) + (z * z + 0.0f));
        const float d[3] = {dx / n, dy / n, z / n};
        ZR_UNROLL
        for (int k = 0; k < 3; k++) out[k] = zr_fma(d[k], len[j], e.vtx0[k]);
    }
    ZR_UNROLL
    for (int k = 0; k < 3; k++) v0[k] = e.vtx0[k];
}
/* mul(v_float4x4, __m128) (MatrixFuncs.h:93-112) of a point (w = 1) with a 3 x 4 object-to-world matrix (column-vector convention, zr_scene_desc) */
ZR_HD void MulPoint(const float* M, const float* v, float* out)
{
    ZR_UNROLL
    for (int r = 0; r < 3; r++) out[r] = zr_fma(1.0f, M[4 * r + 3], zr_fma(v[2], M[4 * r + 2], zr_fma(v[1], M[4 * r + 1], v[0] * M[4 * r])));
}
/* the emissive-triangle transform of SceneCore (SceneCore.cpp:196-236 on the first frame, UpdateEmissivePositions :913-955 for moving instances):
   decode the stored (object-space) triangle, transform its vertices, encode again -- every other field is kept */
ZR_HD void EmissiveToWorld(const zr_emissive_triangle& in, const float* M, zr_emissive_triangle& out)
{
    float v0[3], v1[3], v2[3], w0[3], w1[3], w2[3];
    DecodeEmissiveVertices(in, v0, v1, v2);
    MulPoint(M, v0, w0); MulPoint(M, v1, w1); MulPoint(M, v2, w2);
    out = in;
    StoreEmissiveVertices(out, w0, w1, w2);
}
/* a light triangle whose vertices were deformed (skinning, morph targets, zr_scene_update_vertices): p0..p2 are its object-space positions as the
   vertex buffer holds them.  The loader's geometry step (PackEmissiveTriangle: StoreVertices of the object-space triangle) followed by the moved-light
   rule above with the owner's matrix M -- the same functions in the same order; every non-geometric field of `rec` is kept in both records.  No
   identity-matrix shortcut: that belongs to the reference's first frame (SceneCore.cpp:196-236), UpdateEmissivePositions has none.  A zero-length
   edge: unspecified bytes, as in StoreEmissiveVertices */
ZR_HD void EmissiveFromVertices(const zr_emissive_triangle& rec, const float* p0, const float* p1, const float* p2, const float* M,
    zr_emissive_triangle& objectOut, zr_emissive_triangle& worldOut)
{
    objectOut = rec;
    StoreEmissiveVertices(objectOut, p0, p1, p2);
    EmissiveToWorld(objectOut, M, worldOut);
}

} /* namespace zrsm */

#endif /* ZR_SCENE_MATH_H */
