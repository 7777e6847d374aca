// zr_tu_skin.hip -- the device form of skinning (zr_scene_set_skinning + zr_scene_animate, include/zetaray_amd.h): between k_anim_compose's node matrices
// and the refit, the joint matrices are made (k_skin_joints) and every listed vertex is posed from its rest record (k_skin_vertices), which also writes
// the vertex's entries of the hit tables (zr_hit_tables.h).  The arithmetic is include/zr_skin.h, the header the host form compiles, so the records are
// the host's byte for byte.  No LDS, no scratch, no wave operations.
//
// k_skin_vertices is a stream: 28 + 24 bytes in, 28 + 16 (+ 16 with ZR_HIT_TANGENTS) out per vertex.  A zr_vertex is 28 bytes, so consecutive lanes'
// records are not 16-byte aligned: each lane loads and stores its record as 7 dwords (a wave's 64 records are 1 792 contiguous bytes, every cache line
// of which is used whole).  The influence record travels as one 8-byte and one 16-byte word, the joint matrices as 16-byte rows, the table entries as
// 16-byte words.  A block-cooperative form that moved a block's 7 168 bytes through LDS as 16-byte words, with the head and the tail of a window that
// starts off a 16-byte boundary handled dword by dword, was measured against this one (profiles/r14_scene_skin.json): it was 7 %
// slower in a kernel trace and is not kept.
#include <hip/hip_runtime.h>
#include "../../include/zr_skin.h"
#include "zr_hit_tables.h"
#include "zr_vtx_lane.h"

namespace zr {

static constexpr uint32_t kBlock = 256;
using SkinRange = zrsk::DeviceRange;

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

// the posed record and its two table entries from the rest record's dwords
__device__ inline void PoseLane(const uint32_t in[kVtxDwords], const zr_skin_influence& f, const float* J, uint32_t out[kVtxDwords], VtxDir& vn, VtxDir& vt)
{
    float J0[12], J1[12], J2[12], J3[12], M[12];
    LoadMatrix(J + 12 * (size_t)f.joint[0], J0); LoadMatrix(J + 12 * (size_t)f.joint[1], J1);
    LoadMatrix(J + 12 * (size_t)f.joint[2], J2); LoadMatrix(J + 12 * (size_t)f.joint[3], J3);
    zrsk::Blend(J0, J1, J2, J3, f.weight, M);
    const zr_vertex rest = VertexOfDwords(in);
    zr_vertex posed;
    zrsk::PoseVertex(rest, M, posed);
    DwordsOfVertex(posed, out);
    float n[3], t[3];
    zrsk::DecodeOct32(posed.normal, n); zrsk::DecodeOct32(posed.tangent, t);
    vn.x = n[0]; vn.y = n[1]; vn.z = n[2]; vn.w = 0.0f;
    vt.x = t[0]; vt.y = t[1]; vt.z = t[2]; vt.w = 0.0f;
}

// one lane per vertex of one range.  rest: the range's rest records; vertices / vtxNormals / vtxTangents (null without ZR_HIT_TANGENTS): the scene's arrays,
// written at [firstVertex, firstVertex + count); influence record firstInfluence + i belongs to vertex i of the range
__global__ void __launch_bounds__(kBlock) k_skin_vertices(zr_vertex* vertices, VtxDir* vtxNormals, VtxDir* vtxTangents, const zr_vertex* rest,
    const zr_skin_influence* influences, const float* J, uint32_t firstVertex, uint32_t firstInfluence, uint32_t count)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    uint32_t in[kVtxDwords], out[kVtxDwords];
    ZR_UNROLL
    for (uint32_t k = 0; k < kVtxDwords; k++) in[k] = reinterpret_cast<const uint32_t*>(rest)[kVtxDwords * (size_t)i + k];
    const zr_skin_influence f = LoadInfluence(influences, (size_t)firstInfluence + i);
    VtxDir vn, vt;
    PoseLane(in, f, J, out, vn, vt);
    const size_t v = (size_t)firstVertex + i;
    ZR_UNROLL
    for (uint32_t k = 0; k < kVtxDwords; k++) reinterpret_cast<uint32_t*>(vertices)[kVtxDwords * v + k] = out[k];
    *reinterpret_cast<float4*>(vtxNormals + v) = make_float4(vn.x, vn.y, vn.z, vn.w);
    if (vtxTangents) *reinterpret_cast<float4*>(vtxTangents + v) = make_float4(vt.x, vt.y, vt.z, vt.w);
}

// joints / ranges as zr_scene_set_skinning validated and laid them out (every index in range); nodeWorld: the animation's node matrices, written by the
// launches before these on `st`
hipError_t LaunchSkin(hipStream_t st, float* J, const float* nodeWorld, const uint32_t* jointNode, const float* inverseBind, uint32_t numJoints,
    const SkinRange* ranges, uint32_t numRanges, const zr_vertex* rest, const zr_skin_influence* influences, zr_vertex* vertices, VtxDir* vtxNormals, VtxDir* vtxTangents)
{
    if (numJoints) hipLaunchKernelGGL(k_skin_joints, dim3((numJoints + kBlock - 1) / kBlock), dim3(kBlock), 0, st, J, nodeWorld, jointNode, inverseBind, numJoints);
    for (uint32_t r = 0; r < numRanges; r++)
    {
        const SkinRange& g = ranges[r];
        if (g.numVertices)
            hipLaunchKernelGGL(k_skin_vertices, dim3((g.numVertices + kBlock - 1) / kBlock), dim3(kBlock), 0, st, vertices, vtxNormals, vtxTangents,
                rest + g.restFirst, influences, J, g.firstVertex, g.firstInfluence, g.numVertices);
    }
    return hipGetLastError();
}

} // namespace zr
