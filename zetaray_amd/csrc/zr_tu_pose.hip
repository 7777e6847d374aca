// zr_tu_pose.hip -- the device form of skinning and of morph targets (zr_scene_set_skinning / zr_scene_set_morph + zr_scene_animate, include/zetaray_amd.h):
// between k_anim_compose's node matrices and the refit, the joint matrices are made (k_skin_joints), the weights of every track are sampled
// (k_morph_weights), and every vertex of a listed range (zr_pose.h) is posed from its rest record by k_pose_vertices, which also writes the vertex's entries
// of the hit tables (zr_hit_tables.h).  A range is morphed, skinned, or both in the same lane and without a trip through memory: the morphed record with
// its ENCODED words is the rest record zrsk::PoseVertex takes.  The arithmetic is include/zr_skin.h and include/zr_morph.h, the headers the host form
// compiles, so the records are the host's byte for byte.  No LDS, no scratch, no wave operations.
//
// k_pose_vertices is a stream: 28 bytes in, 28 + 16 (+ 16 with ZR_HIT_TANGENTS) out per vertex, plus 24 bytes of influence record where the range is
// skinned and 12 bytes for every delta array of a target that is APPLIED where it is morphed.  The record moves as 7 dwords each way, the influence
// record and the joint matrices as 8- and 16-byte words (zr_vtx_lane.h), the table entries as 16-byte words.  A block-cooperative form that moved a
// block's 7 168 record bytes through LDS as 16-byte words was measured against this one (profiles/r14_scene_skin.json): it was 7 %
// slower in a kernel trace and is not kept.  A range's weights and target records are read through addresses that do not depend on the lane, so the
// target loop and the zero-weight skip are wave-uniform: a skipped target costs no vector loads.  A delta triple is 12 bytes: each lane loads its three
// dwords, a wave's three loads cover 768 contiguous bytes, every line used whole.
#include "zr_pose.h"
#include "zr_vtx_lane.h"

namespace zr {

static constexpr uint32_t kBlock = 256;

// one lane per joint: J[j] = nodeWorld[node[j]] x inverseBind[j]
__global__ void __launch_bounds__(kBlock) k_skin_joints(float* J, const float* nodeWorld, const uint32_t* jointNode, const float* inverseBind, uint32_t n)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    float W[12], B[12], M[12];
    LoadMatrix(nodeWorld + 12 * (size_t)jointNode[j], W);
    LoadMatrix(inverseBind + 12 * (size_t)j, B);
    zrsk::JointMatrix(W, B, M);
    StoreMatrix(J + 12 * (size_t)j, M);
}

// one lane per (track, target): lane i belongs to the track whose weights contain place i of the weight array (trackOfWeight[i]; weightFirst[track]: where they start)
__global__ void __launch_bounds__(kBlock) k_morph_weights(float* weights, const zr_morph_track* tracks, const uint32_t* trackOfWeight, const uint32_t* weightFirst,
    const float* times, const float* values, const float* restWeights, float t, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t tr = trackOfWeight[i];
    weights[i] = zrmo::TrackWeight(tracks[tr], times, values, restWeights, t, i - weightFirst[tr]);
}

// the delta triples of vertex i under target m into d[0..3) POSITION, d[3..6) NORMAL, d[6..9) TANGENT -- only for an applied target (w != 0: wave-uniform)
// and an attribute it has; each a 12-byte load at a 12-byte stride across the wave
__device__ inline void LoadTargetDeltas(const float* __restrict__ deltas, const zr_morph_target& m, float w, uint32_t i, float d[9])
{
    ZR_UNROLL
    for (int c = 0; c < 9; c++) d[c] = 0.0f;
    if (w == 0.0f) return;
    const uint32_t firsts[3] = {m.first_pos, m.first_nrm, m.first_tan};
    ZR_UNROLL
    for (int a = 0; a < 3; a++)
        if (firsts[a] != ZR_MORPH_NONE)
        {
            const float* p = deltas + 3 * ((size_t)firsts[a] + i);
            d[3 * a] = p[0]; d[3 * a + 1] = p[1]; d[3 * a + 2] = p[2];
        }
}
// zrmo::MorphVertex with the target loop unrolled by two by hand: both targets' loads are issued before the first one's fmas (the rolled loop waited for
// each target's deltas before it read the next weight), the fmas in the order k, k + 1 as the header has them
__device__ inline void MorphLane(const zr_vertex& rest, const zr_morph_target* __restrict__ targets, uint32_t numTargets, const float* __restrict__ weights,
    const float* __restrict__ deltas, uint32_t i, zr_vertex& out)
{
    zrmo::Acc a;
    zrmo::Begin(rest, a);
    uint32_t k = 0;
    for (; k + 1 < numTargets; k += 2)
    {
        const float w0 = weights[k], w1 = weights[k + 1];
        const zr_morph_target m0 = targets[k], m1 = targets[k + 1];
        float d0[9], d1[9];
        LoadTargetDeltas(deltas, m0, w0, i, d0);
        LoadTargetDeltas(deltas, m1, w1, i, d1);
        zrmo::Apply(a, w0, m0, d0, d0 + 3, d0 + 6);
        zrmo::Apply(a, w1, m1, d1, d1 + 3, d1 + 6);
    }
    if (k < numTargets)
    {
        const float w0 = weights[k];
        const zr_morph_target m0 = targets[k];
        float d0[9];
        LoadTargetDeltas(deltas, m0, w0, i, d0);
        zrmo::Apply(a, w0, m0, d0, d0 + 3, d0 + 6);
    }
    zrmo::End(rest, a, out);
}

// one lane per vertex of one range.  rest: the range's rest records; vertices / vtxNormals / vtxTangents (null without ZR_HIT_TANGENTS): the scene's arrays,
// written at [firstVertex, firstVertex + count).  kMorph: targets / weights: the range's numTargets target records and weights; deltas: the pool.
// kSkin: influence record firstInfluence + i belongs to vertex i of the range, J: the joint matrices k_skin_joints wrote.  A range that is skinned only
// takes zrsk::PoseVertex alone (no pass through zrmo::Begin / End, whose decode and encode need not return the rest record's code words)
template <bool kMorph, bool kSkin>
__global__ void __launch_bounds__(kBlock) k_pose_vertices(zr_vertex* vertices, VtxDir* vtxNormals, VtxDir* vtxTangents, const zr_vertex* __restrict__ rest,
    const zr_morph_target* __restrict__ targets, const float* __restrict__ weights, uint32_t numTargets, const float* __restrict__ deltas,
    const zr_skin_influence* __restrict__ influences, const float* __restrict__ J, uint32_t firstVertex, uint32_t firstInfluence, uint32_t count)
{
    static_assert(kMorph || kSkin, "a listed range is morphed, skinned or both");
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    uint32_t in[kVtxDwords], out[kVtxDwords];
    ZR_UNROLL
    for (uint32_t k = 0; k < kVtxDwords; k++) in[k] = reinterpret_cast<const uint32_t*>(rest)[kVtxDwords * (size_t)i + k];
    zr_vertex posed = VertexOfDwords(in);
    if (kMorph)
    {
        const zr_vertex r = posed;
        MorphLane(r, targets, numTargets, weights, deltas, i, posed);
    }
    if (kSkin)
    {   // (the blend after the target loop: the twelve matrix entries live through the loop cost 15 VGPRs and two waves per SIMD)
        const zr_vertex r = posed;
        const zr_skin_influence f = LoadInfluence(influences, (size_t)firstInfluence + i);
        float M[12];
        BlendOfInfluence(f, J, M);
        zrsk::PoseVertex(r, M, posed);
    }
    DwordsOfVertex(posed, out);
    float n[3], t[3];
    zrsk::DecodeOct32(posed.normal, n); zrsk::DecodeOct32(posed.tangent, t);
    const size_t v = (size_t)firstVertex + i;
    ZR_UNROLL
    for (uint32_t k = 0; k < kVtxDwords; k++) reinterpret_cast<uint32_t*>(vertices)[kVtxDwords * v + k] = out[k];
    *reinterpret_cast<float4*>(vtxNormals + v) = make_float4(n[0], n[1], n[2], 0.0f);
    if (vtxTangents) *reinterpret_cast<float4*>(vtxTangents + v) = make_float4(t[0], t[1], t[2], 0.0f);
}

// the tables and ranges as zr_scene_set_skinning / zr_scene_set_morph validated and zr_api.hip laid them out (every index in range, no range empty)
hipError_t LaunchPose(hipStream_t st, float t, const PoseTables& T, const PoseRange* ranges, uint32_t numRanges, zr_vertex* vertices, VtxDir* normals, VtxDir* tangents)
{
    if (T.numJoints) hipLaunchKernelGGL(k_skin_joints, dim3((T.numJoints + kBlock - 1) / kBlock), dim3(kBlock), 0, st, T.J, T.nodeWorld, T.jointNode, T.inverseBind, T.numJoints);
    if (T.numWeights) hipLaunchKernelGGL(k_morph_weights, dim3((T.numWeights + kBlock - 1) / kBlock), dim3(kBlock), 0, st, T.weights, T.tracks, T.trackOfWeight, T.weightFirst,
        T.times, T.values, T.restWeights, t, T.numWeights);
    for (uint32_t r = 0; r < numRanges; r++)
    {
        const PoseRange& g = ranges[r];
        const auto kernel = g.kind == kPoseSkin ? k_pose_vertices<false, true> : g.kind == kPoseMorph ? k_pose_vertices<true, false> : k_pose_vertices<true, true>;
        hipLaunchKernelGGL(kernel, dim3((g.numVertices + kBlock - 1) / kBlock), dim3(kBlock), 0, st, vertices, normals, tangents, T.rest + g.restFirst, T.targets + g.firstTarget,
            T.weights + g.weightFirst, g.numTargets, T.deltas, T.influences, T.J, g.firstVertex, g.firstInfluence, g.numVertices);
    }
    return hipGetLastError();
}

} // namespace zr
