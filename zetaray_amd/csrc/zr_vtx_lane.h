// zr_vtx_lane.h -- how one lane moves a vertex record, an influence record and a joint matrix: what the kernels that pose vertices
// (zr_tu_pose.hip) move through.  A zr_vertex is 28 bytes, so consecutive lanes' records are not 16-byte aligned: each lane loads and stores its record as 7 dwords (a
// wave's 64 records are 1 792 contiguous bytes, every cache line of which is used whole).  The influence record travels as one 8-byte and one 16-byte
// word, the joint matrices as 16-byte rows.
#ifndef ZR_VTX_LANE_H
#define ZR_VTX_LANE_H

#include <hip/hip_runtime.h>
#include "../../include/zr_skin.h"

namespace zr {

static constexpr uint32_t kVtxDwords = 7;
static_assert(sizeof(zr_vertex) == 4 * kVtxDwords && sizeof(zr_skin_influence) == 24, "record sizes");

__device__ inline void LoadMatrix(const float* p, float M[12])
{
    ZR_UNROLL
    for (int k = 0; k < 3; k++) { const float4 r = reinterpret_cast<const float4*>(p)[k]; M[4 * k] = r.x; M[4 * k + 1] = r.y; M[4 * k + 2] = r.z; M[4 * k + 3] = r.w; }
}
__device__ inline void StoreMatrix(float* p, const float M[12])
{
    ZR_UNROLL
    for (int k = 0; k < 3; k++) reinterpret_cast<float4*>(p)[k] = make_float4(M[4 * k], M[4 * k + 1], M[4 * k + 2], M[4 * k + 3]);
}
__device__ inline zr_vertex VertexOfDwords(const uint32_t d[kVtxDwords])
{
    zr_vertex v;
    v.pos[0] = zr_asfloat(d[0]); v.pos[1] = zr_asfloat(d[1]); v.pos[2] = zr_asfloat(d[2]); v.uv[0] = zr_asfloat(d[3]); v.uv[1] = zr_asfloat(d[4]);
    v.normal[0] = (uint16_t)(d[5] & 0xffffu); v.normal[1] = (uint16_t)(d[5] >> 16); v.tangent[0] = (uint16_t)(d[6] & 0xffffu); v.tangent[1] = (uint16_t)(d[6] >> 16);
    return v;
}
__device__ inline void DwordsOfVertex(const zr_vertex& v, uint32_t d[kVtxDwords])
{
    d[0] = zr_asuint(v.pos[0]); d[1] = zr_asuint(v.pos[1]); d[2] = zr_asuint(v.pos[2]); d[3] = zr_asuint(v.uv[0]); d[4] = zr_asuint(v.uv[1]);
    d[5] = (uint32_t)v.normal[0] | ((uint32_t)v.normal[1] << 16); d[6] = (uint32_t)v.tangent[0] | ((uint32_t)v.tangent[1] << 16);
}
// the influence record `idx` of a 16-byte aligned table as one 8-byte and one 16-byte word (24 idx is a multiple of 8, and of 16 for an even idx)
__device__ inline zr_skin_influence LoadInfluence(const zr_skin_influence* table, size_t idx)
{
    const char* p = reinterpret_cast<const char*>(table + idx);
    uint32_t d[6];
    if (idx & 1) { const uint2 a = *reinterpret_cast<const uint2*>(p); const uint4 b = *reinterpret_cast<const uint4*>(p + 8); d[0] = a.x; d[1] = a.y; d[2] = b.x; d[3] = b.y; d[4] = b.z; d[5] = b.w; }
    else { const uint4 b = *reinterpret_cast<const uint4*>(p); const uint2 a = *reinterpret_cast<const uint2*>(p + 16); d[0] = b.x; d[1] = b.y; d[2] = b.z; d[3] = b.w; d[4] = a.x; d[5] = a.y; }
    zr_skin_influence f;
    f.joint[0] = (uint16_t)(d[0] & 0xffffu); f.joint[1] = (uint16_t)(d[0] >> 16); f.joint[2] = (uint16_t)(d[1] & 0xffffu); f.joint[3] = (uint16_t)(d[1] >> 16);
    ZR_UNROLL
    for (int k = 0; k < 4; k++) f.weight[k] = zr_asfloat(d[2 + k]);
    return f;
}
// the matrix a vertex's influence blends from the joint matrices J (16-byte rows)
__device__ inline void BlendOfInfluence(const zr_skin_influence& f, const float* J, float M[12])
{
    float J0[12], J1[12], J2[12], J3[12];
    LoadMatrix(J + 12 * (size_t)f.joint[0], J0); LoadMatrix(J + 12 * (size_t)f.joint[1], J1);
    LoadMatrix(J + 12 * (size_t)f.joint[2], J2); LoadMatrix(J + 12 * (size_t)f.joint[3], J3);
    zrsk::Blend(J0, J1, J2, J3, f.weight, M);
}

} // namespace zr

#endif // ZR_VTX_LANE_H
