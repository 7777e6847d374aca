/*
 * zr_anim.h -- keyframe animation of instances, stated once for the host and the device.
 *
 * What SceneCore::UpdateAnimations (SceneCore.cpp:961-1027), FindInterval (Utility/Utility.h:81-102), Math::slerp (Math/Quaternion.h:83-119) with acos / sin /
 * lerp (Math/VectorFuncs.h:38-54, 177-280), affineTransformation (MatrixFuncs.h:488-503) and the world-transform propagation world = local x parent
 * (SceneCore.cpp:871-873) compute for an animated scene graph, restated as plain scalar code in the operation order of the reference's SSE code.
 * zr_scene_io.cpp (zrh_scene_data_animate, the loader, zrh_compose_world) and zr_tu_anim.hip (zr_scene_animate) both compile these functions; under the
 * arithmetic contract of zr_detmath.h (+ - * / sqrt fma floor, round to nearest even, -ffp-contract=off) the two give the same bits.
 *
 * Three deviations from the reference:
 *   1. Slerp's near-zero branch (cos(theta) > 1 - FLT_EPSILON) normalises the lerp with l * (1.0f / sqrt(dot(l, l))), the dot product in _mm_dp_ps order.  The
 *      reference's normalizeFast uses _mm_rsqrt_ps, a hardware approximation without a portable definition (relative error <= 1.5 * 2^-12).
 *   2. The reference applies an animation's start time T0 in its fast paths and in interpolatedT but searches the interval with the raw time; with T0 != 0
 *      its own assertions fail.  Here the local time is u = t - t0, and everything after that is the reference's code with t_start = 0.  For t0 = 0 the two
 *      are the same arithmetic.
 *   3. The interval index is the binary search's result clamped to num_keys - 2.  After the loop wrap u can round to the last key's time, where the
 *      reference reads the key after the animation's last one; the clamp makes the last interval the answer, and interpolatedT may then be >= 1.
 *
 * The caller guarantees: unit rotations, positive scales, strictly increasing key times (ValidateAnimation checks the last two and finiteness).
 */
#ifndef ZR_ANIM_H
#define ZR_ANIM_H

#include "zr_detmath.h"
#include "zr_wire.h"
#include "zr_scene_math.h"
#include <stdio.h>
#include <vector>

namespace zran {

using zrsm::Mat43;
using zrsm::FromToWorld;

/* Math/Common.h:25-27 */
static constexpr float kPi = 3.141592654f, kPiOver2 = 1.570796327f;

struct Srt { float s[3], q[4], t[3]; };

/* Math::acos (VectorFuncs.h:177-228; from DirectXMath): 7th-degree Horner polynomial in |x| times sqrt(max(0, 1 - |x|)), separate multiplies and adds */
ZR_HD float Acos(float v)
{
    const bool nonnegative = v >= 0.0f;
    const float x = zr_abs(v);
    const float oneM = 1.0f - x;
    const float root = zr_sqrt(oneM > 0.0f ? oneM : 0.0f);
    float t0 = -0.0012624911f * x;
    t0 = t0 + 0.0066700901f; t0 = t0 * x;
    t0 = t0 + -0.0170881256f; t0 = t0 * x;
    t0 = t0 + 0.0308918810f; t0 = t0 * x;
    t0 = t0 + -0.0501743046f; t0 = t0 * x;
    t0 = t0 + 0.0889789874f; t0 = t0 * x;
    t0 = t0 + -0.2145988016f; t0 = t0 * x;
    t0 = t0 + 1.5707963050f; t0 = t0 * root;
    return nonnegative ? t0 : kPi - t0;
}
/* Math::sin (VectorFuncs.h:232-280; from DirectXMath), -pi <= theta < pi: reflected into [-pi/2, pi/2], then the 11th-degree odd polynomial */
ZR_HD float Sin(float theta)
{
    const uint32_t sign = zr_asuint(theta) & 0x80000000u;
    const float c = zr_asfloat(zr_asuint(kPi) | sign);
    const float absx = zr_asfloat(zr_asuint(theta) & 0x7fffffffu);
    const float rflx = c - theta;
    const float x = absx <= kPiOver2 ? theta : rflx;
    const float x2 = x * x;
    float r = -2.3889859e-08f * x2;
    r = r + 2.7525562e-06f; r = r * x2;
    r = r + -0.00019840874f; r = r * x2;
    r = r + 0.0083333310f; r = r * x2;
    r = r + -0.16666667f; r = r * x2;
    r = r + 1.0f;
    return r * x;
}
/* Math::lerp (VectorFuncs.h:38-46): fma(t, v1, fma(-t, v0, v0)) */
ZR_HD float Lerp(float v0, float v1, float t) { return zr_fma(t, v1, zr_fma(-t, v0, v0)); }
ZR_HD void Lerp3(const float* a, const float* b, float t, float* out) { ZR_UNROLL for (int k = 0; k < 3; k++) out[k] = Lerp(a[k], b[k], t); }
ZR_HD void Lerp4(const float* a, const float* b, float t, float* out) { ZR_UNROLL for (int k = 0; k < 4; k++) out[k] = Lerp(a[k], b[k], t); }
/* _mm_dp_ps(a, b, 0xff): (x + y) + (z + w) */
ZR_HD float Dot4(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]); }

/* Math::slerp (Quaternion.h:83-119).  Returns 1 when the near-zero (lerp + normalise) branch was taken: deviation 1 */
ZR_HD int Slerp(const float* q1, const float* q2, float t, float* out)
{
    float cosTheta = Dot4(q1, q2);
    const bool sameHemisphere = cosTheta > 0.0f;
    if (!sameHemisphere) cosTheta = -cosTheta;
    if (cosTheta > 1.0f - 1.1920929e-07f)
    {
        float l[4]; Lerp4(q1, q2, t, l);
        const float inv = 1.0f / zr_sqrt(Dot4(l, l));
        ZR_UNROLL
        for (int k = 0; k < 4; k++) out[k] = l[k] * inv;
        return 1;
    }
    const float sinTheta = zr_sqrt(1.0f - cosTheta * cosTheta);
    const float theta = Acos(cosTheta);
    const float s1 = Sin((1.0f - t) * theta);
    float s2 = Sin(t * theta);
    if (!sameHemisphere) s2 = -s2;
    ZR_UNROLL
    for (int k = 0; k < 4; k++) out[k] = zr_fma(q2[k], s2, q1[k] * s1) / sinTheta;
    return 0;
}

ZR_HD void KeyTransform(const zr_keyframe& k, Srt& r)
{
    ZR_UNROLL
    for (int i = 0; i < 3; i++) { r.s[i] = k.scale[i]; r.t[i] = k.translation[i]; }
    ZR_UNROLL
    for (int i = 0; i < 4; i++) r.q[i] = k.rotation[i];
}
/* the interpolation of UpdateAnimations (SceneCore.cpp:1003-1020): scale and translation lerped, rotation slerped */
ZR_HD void Interpolate(const zr_keyframe& k1, const zr_keyframe& k2, float interpolatedT, Srt& r)
{
    Srt a, b; KeyTransform(k1, a); KeyTransform(k2, b);
    Lerp3(a.s, b.s, interpolatedT, r.s);
    Lerp3(a.t, b.t, interpolatedT, r.t);
    Slerp(a.q, b.q, interpolatedT, r.q);
}
/* SceneCore::UpdateAnimations for one animation: keys[0 .. numKeys), numKeys >= 2, at time t.  Deviations 2 and 3 */
ZR_HD void SampleAnimation(const zr_keyframe* keys, uint32_t numKeys, float t0, uint32_t loop, float t, Srt& r)
{
    float u = t - t0;
    const float ks = keys[0].time, ke = keys[numKeys - 1].time;
    if (u <= ks) { KeyTransform(keys[0], r); return; }
    if (!loop && u >= ke) { KeyTransform(keys[numKeys - 1], r); return; }
    if (u >= ke)
    {
        const float numLoops = zr_floor((u - ks) / (ke - ks));
        const float excess = numLoops * (ke - ks) + ks;
        u -= excess;
        u += ks;
    }
    /* FindInterval over [0, numKeys - 1] */
    int32_t beg = 0, end = (int32_t)numKeys - 1;
    while (beg != end)
    {
        const int32_t mid = 1 + ((beg + end - 1) >> 1);
        if (keys[mid].time > u) end = mid - 1;
        else beg = mid;
    }
    if (beg > (int32_t)numKeys - 2) beg = (int32_t)numKeys - 2;
    const float t1 = keys[beg].time, t2 = keys[beg + 1].time;
    const float interpolatedT = (u - t1) / (t2 - t1);
    Interpolate(keys[beg], keys[beg + 1], interpolatedT, r);
}

/* ---- matrices (Math/MatrixFuncs.h).  Mat43 (zr_scene_math.h): row-vector 4 x 4 as the reference stores it */
ZR_HD void ToToWorld(const Mat43& r, float* M)
{
    ZR_UNROLL
    for (int i = 0; i < 3; i++) { ZR_UNROLL for (int j = 0; j < 3; j++) M[4 * j + i] = r.m[i][j]; }
    ZR_UNROLL
    for (int j = 0; j < 3; j++) M[4 * j + 3] = r.m[3][j];
}
/* rotationMatFromQuat, MatrixFuncs.h:356-405 (operation order of the SSE code) */
ZR_HD void RotationMatFromQuat(const float q[4], float R[3][3])
{
    const float q1 = q[0], q2 = q[1], q3 = q[2], q4 = q[3];
    const float q1s = q1 * q1, q2s = q2 * q2, q3s = q3 * q3;
    const float d0 = zr_fma(q1s + q3s, -2.0f, 1.0f), d1 = zr_fma(q2s + q3s, -2.0f, 1.0f), d2 = zr_fma(q1s + q2s, -2.0f, 1.0f);
    const float q1q4 = (q1 * q4) * 2.0f, q2q4 = (q2 * q4) * 2.0f, q1q3 = (q3 * q1) * 2.0f, q3q4 = (q4 * q3) * 2.0f;
    const float q1q2 = (q1 * q2) * 2.0f, q2q3 = (q2 * q3) * 2.0f;
    R[0][0] = d1;          R[0][1] = q1q2 + q3q4; R[0][2] = q1q3 - q2q4;
    R[1][0] = q1q2 - q3q4; R[1][1] = d0;          R[1][2] = q2q3 + q1q4;
    R[2][0] = q1q3 + q2q4; R[2][1] = q2q3 - q1q4; R[2][2] = d2;
}
/* affineTransformation(vS, vQ, vT), MatrixFuncs.h:488-503 */
ZR_HD Mat43 AffineTransformation(const float s[3], const float q[4], const float t[3])
{
    float R[3][3]; RotationMatFromQuat(q, R);
    Mat43 r;
    ZR_UNROLL
    for (int i = 0; i < 3; i++) { ZR_UNROLL for (int j = 0; j < 3; j++) r.m[i][j] = s[i] * R[i][j]; }
    ZR_UNROLL
    for (int j = 0; j < 3; j++) r.m[3][j] = t[j];
    return r;
}
/* mul(M1, M2), MatrixFuncs.h:114-163, for affine matrices (column 3 = (0, 0, 0, 1)): (a0 b0 + a1 b1) + (a2 b2 + a3 b3), fused as the AVX code */
ZR_HD Mat43 Mul(const Mat43& A, const Mat43& B)
{
    Mat43 C;
    ZR_UNROLL
    for (int i = 0; i < 4; i++)
    {
        const float a3 = i == 3 ? 1.0f : 0.0f;
        ZR_UNROLL
        for (int j = 0; j < 3; j++)
        {
            const float c2 = zr_fma(A.m[i][1], B.m[1][j], A.m[i][0] * B.m[0][j]);
            const float c6 = zr_fma(a3, B.m[3][j], A.m[i][2] * B.m[2][j]);
            C.m[i][j] = c2 + c6;
        }
    }
    return C;
}
/* a node's local matrix and the propagation step, on 3 x 4 row-major matrices (the layout of zr_scene_desc.instance_to_world): what zrh_compose_world chains */
ZR_HD void LocalMatrix(const Srt& r, float* local) { ToToWorld(AffineTransformation(r.s, r.q, r.t), local); }
ZR_HD void ComposeWorld(const float* local, const float* parentWorld, float* world) { ToToWorld(Mul(FromToWorld(local), FromToWorld(parentWorld)), world); }

/* ---- a node of the dynamic closure (zr_anim_node, zr_wire.h) at time t */
ZR_HD void NodeLocal(const zr_anim_node& n, const zr_keyframe* keys, float t, float* local)
{
    Srt r;
    if (n.num_keys) SampleAnimation(keys + n.first_key, n.num_keys, n.t0, n.loop, t, r);
    else
    {
        ZR_UNROLL
        for (int i = 0; i < 3; i++) { r.s[i] = n.rest_scale[i]; r.t[i] = n.rest_translation[i]; }
        ZR_UNROLL
        for (int i = 0; i < 4; i++) r.q[i] = n.rest_rotation[i];
    }
    LocalMatrix(r, local);
}

/* ---- host side: the whole table in table order (a parent precedes its children, so this is the loader's recursion and the device's level-by-level
   launches in one loop).  nodeWorld: num_nodes x 12 floats */
static inline void EvalNodeWorlds(const zr_anim_desc& d, float t, float* nodeWorld)
{
    for (uint32_t i = 0; i < d.num_nodes; i++)
    {
        const zr_anim_node& n = d.nodes[i];
        float local[12];
        NodeLocal(n, d.keys, t, local);
        ComposeWorld(local, n.parent == ZR_ANIM_ROOT ? n.parent_world : nodeWorld + 12 * (size_t)n.parent, nodeWorld + 12 * (size_t)i);
    }
}
static inline bool Finite(float x) { return (zr_asuint(x) & 0x7f800000u) != 0x7f800000u; }
/* What zr_scene_set_animation and zrh_scene_data_set_animation refuse (ZR_ERR_INVALID_ARG): returns 0, or -1 with a message.  level[i] (num_nodes entries,
   may be null) receives each node's depth below its ZR_ANIM_ROOT ancestor */
static inline int ValidateAnimation(const zr_anim_desc& d, uint32_t sceneInstances, uint32_t* level, char* msg, size_t cap)
{
#define ZRAN_FAIL(...) do { snprintf(msg, cap, __VA_ARGS__); return -1; } while (0)
    if ((d.num_nodes && !d.nodes) || (d.num_keys && !d.keys) || (d.num_instances && (!d.instance_idx || !d.instance_node))) ZRAN_FAIL("null table with a non-zero count");
    for (uint32_t i = 0; i < d.num_nodes; i++)
    {
        const zr_anim_node& n = d.nodes[i];
        if (n.parent != ZR_ANIM_ROOT && n.parent >= i) ZRAN_FAIL("node %u: parent %u is not an earlier entry of the table", i, n.parent);
        if (n.num_keys == 1) ZRAN_FAIL("node %u: num_keys == 1 (0 = not animated, else >= 2)", i);
        if (n.num_keys && ((uint64_t)n.first_key + n.num_keys > d.num_keys)) ZRAN_FAIL("node %u: key range [%u, %llu) out of bounds, the table has %u keys", i, n.first_key, (unsigned long long)n.first_key + n.num_keys, d.num_keys);
        if (!Finite(n.t0)) ZRAN_FAIL("node %u: t0 is not finite", i);
        for (int k = 0; k < 3; k++) if (!Finite(n.rest_scale[k]) || !(n.rest_scale[k] > 0.0f)) ZRAN_FAIL("node %u: rest scale <= 0 or not finite", i);
        for (uint32_t k = 0; k < n.num_keys; k++)
        {
            const zr_keyframe& key = d.keys[n.first_key + k];
            if (!Finite(key.time)) ZRAN_FAIL("node %u: key %u: time is not finite", i, k);
            if (k && !(key.time > d.keys[n.first_key + k - 1].time)) ZRAN_FAIL("node %u: key times are not strictly increasing at key %u", i, k);
            for (int c = 0; c < 3; c++)
            {
                if (!Finite(key.scale[c]) || !Finite(key.translation[c])) ZRAN_FAIL("node %u: key %u is not finite", i, k);
                if (!(key.scale[c] > 0.0f)) ZRAN_FAIL("node %u: key %u: a scale <= 0", i, k);
            }
            for (int c = 0; c < 4; c++) if (!Finite(key.rotation[c])) ZRAN_FAIL("node %u: key %u is not finite", i, k);
        }
    }
        std::vector<uint32_t> depth(d.num_nodes);
    for (uint32_t i = 0; i < d.num_nodes; i++)
    {
        depth[i] = d.nodes[i].parent == ZR_ANIM_ROOT ? 0u : depth[d.nodes[i].parent] + 1u;
        if (depth[i] >= ZR_ANIM_MAX_LEVELS) ZRAN_FAIL("node %u: more than %u levels", i, ZR_ANIM_MAX_LEVELS);
    }
    std::vector<uint8_t> listed(sceneInstances, 0);
    for (uint32_t j = 0; j < d.num_instances; j++)
    {
        if (d.instance_idx[j] >= sceneInstances) ZRAN_FAIL("instance %u (entry %u of the list), the scene has %u", d.instance_idx[j], j, sceneInstances);
        if (d.instance_node[j] >= d.num_nodes) ZRAN_FAIL("entry %u of the list names node %u, the table has %u", j, d.instance_node[j], d.num_nodes);
        if (listed[d.instance_idx[j]]) ZRAN_FAIL("instance %u is listed twice", d.instance_idx[j]);
        listed[d.instance_idx[j]] = 1;
    }
    if (level) for (uint32_t i = 0; i < d.num_nodes; i++) level[i] = depth[i];
#undef ZRAN_FAIL
    return 0;
}

} /* namespace zran */

#endif /* ZR_ANIM_H */
