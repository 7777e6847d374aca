/*
 * zr_morph.h -- glTF morph targets (blend shapes), stated once for the host and the device.
 *
 * glTF 2.0 section 3.7.2.2: a morphed vertex is its rest attribute plus the weighted sum of its targets' deltas; the weights are the mesh's or the node's,
 * or sampled from an animation channel with the path `weights`.  zr_scene_io.cpp (zrh_morph_pose, the host form), zr_api.hip (the setter's check),
 * tests/morphmath and zr_tu_pose.hip (zr_scene_animate with a morph set) all compile these functions; under the arithmetic contract of zr_detmath.h
 * (+ - * / sqrt fma, round to nearest even, -ffp-contract=off) they give the same bytes.  Every fma below is written; nothing else is fused.
 *
 *   weights        SampleWeight: zran::SampleAnimation's control flow over a plain array of key times.  u = t - t0; u <= first key: the first key's
 *                  values; not looping and u >= last key: the last key's; else the loop wrap (floor((u - ks) / (ke - ks)) whole periods taken off),
 *                  FindInterval over [0, numKeys - 1] clamped to numKeys - 2, interpolatedT = (u - t1) / (t2 - t1), and
 *                  w_k = zran::Lerp(v[i][k], v[i + 1][k], interpolatedT) = fma(T, v1, fma(-T, v0, v0)).  The values are key-major: values[i * numTargets + k].
 *                  A track with num_keys == 0 yields its rest weights unchanged.  (tests/test_morph_cpu.py pins the flow to SampleAnimation's
 *                  translation.x bit for bit.)
 *   skip rule      a target whose weight is +0 or -0 is SKIPPED, on the host and on the device: this is part of the definition (fma(0, d, -0) is +0, so
 *                  applying it could change a byte), and it lets the device skip the loads -- weights are uniform over a range
 *   position       acc_c = rest.pos[c]; for each applied target k = 0 .. T - 1 in order that has POSITION deltas: acc_c = fma(w_k, d_k[c], acc_c)
 *   normal         acc = zrsk::DecodeOct32(rest.normal); the same fma chain over the applied targets that have NORMAL deltas; if at least one was
 *                  applied, out.normal = zrsm::EncodeOct32(zrsk::Normalize3(acc)), otherwise the rest code words are COPIED (decode + encode need not
 *                  round-trip; an untouched vertex keeps its bytes).  The caller guarantees acc != 0: with a zero-length sum the two code words are
 *                  unspecified; nothing else is (as zr_skin.h's det <= 0)
 *   tangent        as the normal, with the TANGENT deltas (xyz only; the vertex has no handedness word)
 *   uv             copied
 *   morph + skin   the morphed record, with its ENCODED words, is the rest record zrsk::PoseVertex takes: the host form of a range that is morphed and
 *                  skinned is MorphVertex, then zrsk::SkinVertex on its output.  The device fuses the two without a trip through memory, but through
 *                  the encode and the decode, so the bytes agree
 *   hit tables     the VtxDir entries (zr_hit_tables.h) of a posed vertex are zrsk::DecodeOct32 of the STORED codes, as in skinning
 *
 * Weights of a set live in one array, track after track: track i's start at the sum of num_targets of the tracks before it (WeightOffsets).
 */
#ifndef ZR_MORPH_H
#define ZR_MORPH_H

#include "zr_detmath.h"
#include "zr_wire.h"
#include "zr_scene_math.h"
#include "zr_anim.h"
#include "zr_skin.h"
#include <stdio.h>
#include <vector>

namespace zrmo {

/* weight k of a keyed track (numKeys >= 2) at time t: SampleAnimation's flow (zr_anim.h), restated over `times` */
ZR_HD float SampleWeight(const float* times, const float* values, uint32_t numKeys, uint32_t numTargets, float t0, uint32_t loop, float t, uint32_t k)
{
    float u = t - t0;
    const float ks = times[0], ke = times[numKeys - 1];
    if (u <= ks) return values[k];
    if (!loop && u >= ke) return values[(size_t)(numKeys - 1) * numTargets + k];
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
        if (times[mid] > u) end = mid - 1;
        else beg = mid;
    }
    if (beg > (int32_t)numKeys - 2) beg = (int32_t)numKeys - 2;
    const float t1 = times[beg], t2 = times[beg + 1];
    const float interpolatedT = (u - t1) / (t2 - t1);
    return zran::Lerp(values[(size_t)beg * numTargets + k], values[(size_t)(beg + 1) * numTargets + k], interpolatedT);
}
ZR_HD void SampleWeights(const float* times, const float* values, uint32_t numKeys, uint32_t numTargets, float t0, uint32_t loop, float t, float* out)
{
    for (uint32_t k = 0; k < numTargets; k++) out[k] = SampleWeight(times, values, numKeys, numTargets, t0, loop, t, k);
}
/* weight k of a track of a set: sampled, or its rest weight */
ZR_HD float TrackWeight(const zr_morph_track& tr, const float* times, const float* values, const float* restWeights, float t, uint32_t k)
{
    if (!tr.num_keys) return restWeights[(size_t)tr.first_rest + k];
    return SampleWeight(times + tr.first_key, values + tr.first_value, tr.num_keys, tr.num_targets, tr.t0, tr.loop, t, k);
}

/* acc += w d, component by component */
ZR_HD void AddDelta(float w, const float* d, float* acc)
{
    ZR_UNROLL
    for (int c = 0; c < 3; c++) acc[c] = zr_fma(w, d[c], acc[c]);
}
/* one vertex in three steps, so that the device form can schedule its loads (zr_tu_pose.hip issues two targets' loads before the first one's fmas) and
 * still compile this arithmetic: Begin, Apply for the targets k = 0 .. T - 1 in order, End */
struct Acc { float p[3], n[3], t[3]; bool anyN, anyT; };
ZR_HD void Begin(const zr_vertex& rest, Acc& a)
{
    a.p[0] = rest.pos[0]; a.p[1] = rest.pos[1]; a.p[2] = rest.pos[2];
    zrsk::DecodeOct32(rest.normal, a.n); zrsk::DecodeOct32(rest.tangent, a.t);
    a.anyN = a.anyT = false;
}
/* target m under weight w; dp / dn / dt: the vertex's POSITION / NORMAL / TANGENT delta triples, read only for an attribute m has and only if w != 0 */
ZR_HD void Apply(Acc& a, float w, const zr_morph_target& m, const float* dp, const float* dn, const float* dt)
{
    if (w == 0.0f) return;      /* +0 and -0: the skip rule */
    if (m.first_pos != ZR_MORPH_NONE) AddDelta(w, dp, a.p);
    if (m.first_nrm != ZR_MORPH_NONE) { AddDelta(w, dn, a.n); a.anyN = true; }
    if (m.first_tan != ZR_MORPH_NONE) { AddDelta(w, dt, a.t); a.anyT = true; }
}
ZR_HD void End(const zr_vertex& rest, const Acc& a, zr_vertex& out)
{
    out.pos[0] = a.p[0]; out.pos[1] = a.p[1]; out.pos[2] = a.p[2];
    out.uv[0] = rest.uv[0]; out.uv[1] = rest.uv[1];
    if (a.anyN) { float u[3]; zrsk::Normalize3(a.n, u); zrsm::EncodeOct32(u, out.normal); }
    else { out.normal[0] = rest.normal[0]; out.normal[1] = rest.normal[1]; }
    if (a.anyT) { float u[3]; zrsk::Normalize3(a.t, u); zrsm::EncodeOct32(u, out.tangent); }
    else { out.tangent[0] = rest.tangent[0]; out.tangent[1] = rest.tangent[1]; }
}
/* ... and in one: vertex v of a range with the targets targets[0 .. numTargets) under weights[0 .. numTargets); deltas: the pool of float triples */
ZR_HD void MorphVertex(const zr_vertex& rest, const zr_morph_target* targets, uint32_t numTargets, const float* weights, const float* deltas, uint32_t v, zr_vertex& out)
{
    Acc a;
    Begin(rest, a);
    for (uint32_t k = 0; k < numTargets; k++)
    {
        const zr_morph_target m = targets[k];
        /* (an address is formed only for an attribute the target has; Apply reads nothing else) */
        Apply(a, weights[k], m, m.first_pos != ZR_MORPH_NONE ? deltas + 3 * ((size_t)m.first_pos + v) : deltas,
            m.first_nrm != ZR_MORPH_NONE ? deltas + 3 * ((size_t)m.first_nrm + v) : deltas, m.first_tan != ZR_MORPH_NONE ? deltas + 3 * ((size_t)m.first_tan + v) : deltas);
    }
    End(rest, a, out);
}

/* ---- host side: the whole set */
/* offs[i]: where track i's weights start in the set's weight array; returns the array's length */
static inline uint32_t WeightOffsets(const zr_morph_desc& d, uint32_t* offs)
{
    uint32_t n = 0;
    for (uint32_t i = 0; i < d.num_tracks; i++) { offs[i] = n; n += d.tracks[i].num_targets; }
    return n;
}
/* W: the set's weights at time t, track after track */
static inline void EvalWeights(const zr_morph_desc& d, float t, float* W)
{
    size_t o = 0;
    for (uint32_t i = 0; i < d.num_tracks; i++)
        for (uint32_t k = 0; k < d.tracks[i].num_targets; k++) W[o++] = TrackWeight(d.tracks[i], d.times, d.values, d.rest_weights, t, k);
}
/* the skin range equal to morph range g, or -1 (ValidateMorph: a skin range that meets g equals it) */
static inline int64_t SkinRangeOf(const zr_morph_range& g, const zr_skin_desc* skin)
{
    if (skin) for (uint32_t r = 0; r < skin->num_ranges; r++)
        if (skin->ranges[r].first_vertex == g.first_vertex && skin->ranges[r].num_vertices == g.num_vertices && g.num_vertices) return r;
    return -1;
}
/* rest: the rest-pose records of the morph ranges, range after range; out: the posed ones in the same order.  With skin and J (its joint matrices,
 * zrsk::EvalJointMatrices) a range that is also a skin range goes on through zrsk::SkinVertex; with skin == null the ranges are morphed only */
static inline void MorphRanges(const zr_morph_desc& d, const float* W, const zr_skin_desc* skin, const float* J, const zr_vertex* rest, zr_vertex* out)
{
    std::vector<uint32_t> offs(d.num_tracks);
    WeightOffsets(d, offs.data());
    size_t k = 0;
    for (uint32_t r = 0; r < d.num_ranges; r++)
    {
        const zr_morph_range& g = d.ranges[r];
        const int64_t sr = SkinRangeOf(g, skin);
        for (uint32_t v = 0; v < g.num_vertices; v++, k++)
        {
            zr_vertex m;
            MorphVertex(rest[k], d.targets + g.first_target, g.num_targets, W + offs[g.track], d.deltas, v, m);
            if (sr >= 0) zrsk::SkinVertex(m, skin->influences[skin->ranges[sr].first_influence + (size_t)v], J, out[k]);
            else out[k] = m;
        }
    }
}
/* What zr_scene_set_morph refuses (ZR_ERR_INVALID_ARG): returns 0, or -1 with a message.  skin: the set the scene holds, or null */
static inline int ValidateMorph(const zr_morph_desc& d, const zr_skin_desc* skin, uint32_t sceneVertices, char* msg, size_t cap)
{
#define ZRMO_FAIL(...) do { snprintf(msg, cap, __VA_ARGS__); return -1; } while (0)
    if ((d.num_tracks && !d.tracks) || (d.num_targets && !d.targets) || (d.num_ranges && !d.ranges) || (d.num_times && !d.times) || (d.num_values && !d.values) ||
        (d.num_rest_weights && !d.rest_weights) || (d.num_deltas && !d.deltas)) ZRMO_FAIL("null table with a non-zero count");
    for (uint32_t i = 0; i < d.num_tracks; i++)
    {
        const zr_morph_track& tr = d.tracks[i];
        if (tr.num_keys == 1) ZRMO_FAIL("track %u: num_keys == 1 (0 keys, or at least 2)", i);
        if (!zran::Finite(tr.t0)) ZRMO_FAIL("track %u: t0 is not finite", i);
        if (!tr.num_keys)
        {
            if ((uint64_t)tr.first_rest + tr.num_targets > d.num_rest_weights) ZRMO_FAIL("track %u: rest weights [%u, %llu), the pool has %u", i, tr.first_rest, (unsigned long long)tr.first_rest + tr.num_targets, d.num_rest_weights);
            for (uint32_t k = 0; k < tr.num_targets; k++) if (!zran::Finite(d.rest_weights[tr.first_rest + k])) ZRMO_FAIL("track %u: a rest weight is not finite", i);
            continue;
        }
        if ((uint64_t)tr.first_key + tr.num_keys > d.num_times) ZRMO_FAIL("track %u: key times [%u, %llu), the pool has %u", i, tr.first_key, (unsigned long long)tr.first_key + tr.num_keys, d.num_times);
        if ((uint64_t)tr.first_value + (uint64_t)tr.num_keys * tr.num_targets > d.num_values) ZRMO_FAIL("track %u: values [%u, %llu), the pool has %u", i, tr.first_value, (unsigned long long)tr.first_value + (unsigned long long)tr.num_keys * tr.num_targets, d.num_values);
        for (uint32_t k = 0; k < tr.num_keys; k++)
        {
            const float tm = d.times[tr.first_key + k];
            if (!zran::Finite(tm)) ZRMO_FAIL("track %u: key %u: time is not finite", i, k);
            if (k && !(tm > d.times[tr.first_key + k - 1])) ZRMO_FAIL("track %u: key %u: times are not strictly increasing", i, k);
        }
        for (uint64_t k = 0; k < (uint64_t)tr.num_keys * tr.num_targets; k++) if (!zran::Finite(d.values[tr.first_value + k])) ZRMO_FAIL("track %u: a weight is not finite", i);
    }
    std::vector<uint8_t> covered(sceneVertices, 0);
    for (uint32_t r = 0; r < d.num_ranges; r++)
    {
        const zr_morph_range& g = d.ranges[r];
        if ((uint64_t)g.first_vertex + g.num_vertices > sceneVertices) ZRMO_FAIL("range %u: vertices [%u, %llu), the scene has %u", r, g.first_vertex, (unsigned long long)g.first_vertex + g.num_vertices, sceneVertices);
        if ((uint64_t)g.first_target + g.num_targets > d.num_targets) ZRMO_FAIL("range %u: targets [%u, %llu), the table has %u", r, g.first_target, (unsigned long long)g.first_target + g.num_targets, d.num_targets);
        if (g.track >= d.num_tracks) ZRMO_FAIL("range %u: track %u, the table has %u", r, g.track, d.num_tracks);
        if (g.num_targets != d.tracks[g.track].num_targets) ZRMO_FAIL("range %u: %u targets, its track %u has %u", r, g.num_targets, g.track, d.tracks[g.track].num_targets);
        for (uint32_t k = 0; k < g.num_targets; k++)
        {
            const zr_morph_target& m = d.targets[g.first_target + k];
            const uint32_t firsts[3] = {m.first_pos, m.first_nrm, m.first_tan};
            for (int a = 0; a < 3; a++)
                if (firsts[a] != ZR_MORPH_NONE && (uint64_t)firsts[a] + g.num_vertices > d.num_deltas)
                    ZRMO_FAIL("range %u: target %u: deltas [%u, %llu), the pool has %u", r, k, firsts[a], (unsigned long long)firsts[a] + g.num_vertices, d.num_deltas);
        }
        for (uint32_t v = 0; v < g.num_vertices; v++)
        {
            if (covered[g.first_vertex + v]) ZRMO_FAIL("range %u overlaps an earlier range at vertex %u", r, g.first_vertex + v);
            covered[g.first_vertex + v] = 1;
        }
        if (skin) for (uint32_t q = 0; q < skin->num_ranges; q++)
        {
            const zr_skin_range& o = skin->ranges[q];
            const uint64_t lo = g.first_vertex > o.first_vertex ? g.first_vertex : o.first_vertex;
            const uint64_t ga = (uint64_t)g.first_vertex + g.num_vertices, oa = (uint64_t)o.first_vertex + o.num_vertices, hi = ga < oa ? ga : oa;
            if (hi > lo && (g.first_vertex != o.first_vertex || g.num_vertices != o.num_vertices))
                ZRMO_FAIL("range %u meets skin range %u without being equal to it", r, q);
        }
    }
    for (uint64_t i = 0; i < 3 * (uint64_t)d.num_deltas; i++) if (!zran::Finite(d.deltas[i])) ZRMO_FAIL("delta %llu: a component is not finite", (unsigned long long)(i / 3));
#undef ZRMO_FAIL
    return 0;
}

} /* namespace zrmo */

#endif /* ZR_MORPH_H */
