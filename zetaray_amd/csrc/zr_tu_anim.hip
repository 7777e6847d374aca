// zr_tu_anim.hip -- the device form of keyframe animation (zr_scene_animate, include/zetaray_amd.h): one float, the time, becomes the frame's moved list
// [n x 12 floats | n indices] that zr::LaunchMoveInstances (zr_tu_scene_update.hip) consumes.  The arithmetic is include/zr_anim.h, the header the host
// path (zrh_scene_data_animate) compiles, so the matrices are the host's bit for bit.  Three per-element kernels bound by launch latency: no LDS, no wave
// operations, matrices travel as 16-byte words.
#include <hip/hip_runtime.h>
#include "../../include/zr_anim.h"

namespace zr {

static constexpr uint32_t kBlock = 256;

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

// one lane per animated node: nodeLocal[node] = AffineTransformation(SampleAnimation(its keys, t))
__global__ void __launch_bounds__(kBlock) k_anim_sample(float* nodeLocal, const zr_anim_node* nodes, const zr_keyframe* keys, const uint32_t* animated, uint32_t nAnimated, float t)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nAnimated) return;
    const uint32_t n = animated[j];
    const zr_anim_node* nd = nodes + n;
    zran::Srt r;
    zran::SampleAnimation(keys + nd->first_key, nd->num_keys, nd->t0, nd->loop, t, r);
    float L[12]; zran::LocalMatrix(r, L);
    StoreMatrix(nodeLocal + 12 * (size_t)n, L);
}

// one launch per level, top level first; one lane per node of the level: nodeWorld[n] = local x (the static matrix above a root | the parent's world of the
// launch before).  Per level, so that the products associate as in the loader's recursion (zrh_compose_world chained)
__global__ void __launch_bounds__(kBlock) k_anim_compose(float* nodeWorld, const float* nodeLocal, const zr_anim_node* nodes, const uint32_t* levelNodes, uint32_t cnt)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    const uint32_t n = levelNodes[j];
    const zr_anim_node* nd = nodes + n;
    const uint32_t parent = nd->parent;
    float L[12], P[12], W[12];
    LoadMatrix(nodeLocal + 12 * (size_t)n, L);
    if (parent == ZR_ANIM_ROOT)
    {   // (a 108-byte record: 4-byte aligned)
        ZR_UNROLL
        for (int k = 0; k < 12; k++) P[k] = nd->parent_world[k];
    }
    else LoadMatrix(nodeWorld + 12 * (size_t)parent, P);
    zran::ComposeWorld(L, P, W);
    StoreMatrix(nodeWorld + 12 * (size_t)n, W);
}

// one lane per listed instance: slot j of the moved list takes the world matrix of the node the instance hangs on
__global__ void __launch_bounds__(kBlock) k_anim_emit(float* movedXf, const float* nodeWorld, const uint32_t* instNode, uint32_t n)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    float M[12]; LoadMatrix(nodeWorld + 12 * (size_t)instNode[j], M);
    StoreMatrix(movedXf + 12 * (size_t)j, M);
}

// nodes / keys / animated / levelNodes / instNode: the tables zr_scene_set_animation validated and uploaded (every index in range); levelOffsets: host array of
// numLevels + 1 offsets into levelNodes; nodeLocal holds the non-animated nodes' local matrices already; moved: [nInst x 12 floats | nInst indices]
hipError_t LaunchAnimate(hipStream_t st, float t, const zr_anim_node* nodes, const zr_keyframe* keys, const uint32_t* animated, uint32_t nAnimated,
    const uint32_t* levelNodes, const uint32_t* levelOffsets, uint32_t numLevels, float* nodeLocal, float* nodeWorld, const uint32_t* instNode, uint32_t nInst, uint32_t* moved)
{
    if (nAnimated) hipLaunchKernelGGL(k_anim_sample, dim3((nAnimated + kBlock - 1) / kBlock), dim3(kBlock), 0, st, nodeLocal, nodes, keys, animated, nAnimated, t);
    for (uint32_t l = 0; l < numLevels; l++)
    {
        const uint32_t first = levelOffsets[l], cnt = levelOffsets[l + 1] - first;
        if (cnt) hipLaunchKernelGGL(k_anim_compose, dim3((cnt + kBlock - 1) / kBlock), dim3(kBlock), 0, st, nodeWorld, nodeLocal, nodes, levelNodes + first, cnt);
    }
    if (nInst) hipLaunchKernelGGL(k_anim_emit, dim3((nInst + kBlock - 1) / kBlock), dim3(kBlock), 0, st, reinterpret_cast<float*>(moved), nodeWorld, instNode, nInst);
    return hipGetLastError();
}

} // namespace zr
