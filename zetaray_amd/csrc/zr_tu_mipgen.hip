// zr_tu_mipgen.hip -- the device form of the mip generation (zr_scene_create_compressed with ZR_TEX_SRC_RAW_MIP0 sources, zr_mipgen_device;
// include/zetaray_amd.h): levels 1 .. of every texture of a call from its level 0, ONE launch per level, top down, all textures in the same launch.  A
// launch of level k reads what the launch of level k - 1 wrote on the same stream.  The arithmetic is include/zr_mipgen.h, the header the host loader
// compiles (zrh_mip_generate), so the chains are the host's byte for byte.
//   k_mipgen_level   one lane per destination texel.  A lane finds its texture by binary search of its item index in the level's job table (zrmg::Job,
//                    sorted by first item; 128 textures: 7 probes, all lanes of a wave but those at a texture boundary taking the same path through
//                    the same cached words).  Lanes follow the texels of a destination row, so with even widths a wave reads 2 x 512 (RGBA8) or
//                    2 x 256 (RG8) contiguous bytes and stores 256 / 128.  No wave operations; LDS holds the sRGB table only.
// A level is loaded and stored texel by texel: heap offsets are multiples of 4 only, so an RGBA8 texel is 4-byte aligned and no more, and an RG8 level
// can start on any even byte (a 5 x 3 RG8 level 0 is 30 bytes), so an RG8 texel is 2-byte aligned.
// The 16-bit sRGB table (zr_srgb16_table, a constant of this code object, 512 bytes) is read by per-lane index, about 60 times per sRGB texel (4 taps and
// 16 search probes per colour channel).  Each block copies it into LDS first: read from global memory through the vector cache, the same launches took
// twice the stream time (0.531 / 4.112 ms against 0.285 / 2.033 ms for 16 / 128 textures of 2048^2, measured with tools/mipgen_bench.py).
#include <hip/hip_runtime.h>
#include "../../include/zr_mipgen.h"

namespace zr {

static constexpr uint32_t kMipBlock = 256;
// every job's source and destination levels lie inside texels (the host checked); texels: 4-byte aligned
__global__ void __launch_bounds__(kMipBlock) k_mipgen_level(const zrmg::Job* jobs, uint32_t numJobs, uint32_t numItems, uint8_t* texels)
{
    // the 16-bit sRGB table, 512 bytes, staged in LDS by the block's 256 lanes: an sRGB texel looks it up about 60 times by per-lane index
    __shared__ uint16_t sL[256];
    sL[threadIdx.x] = zr_srgb16_table[threadIdx.x];
    __syncthreads();
    const uint64_t g64 = (uint64_t)blockIdx.x * kMipBlock + threadIdx.x;
    if (g64 >= numItems) return;
    const uint32_t g = (uint32_t)g64;
    const zrmg::Job job = jobs[zrmg::FindJob(jobs, numJobs, g)];
    const uint32_t local = g - job.first_item;
    const uint32_t y = local / job.dw, x = local - y * job.dw;
    const uint32_t p = zrmg::Texel(texels + job.src, job.sw, job.sh, job.format, x, y, sL);
    if (job.format == ZR_TEX_RG8) *reinterpret_cast<uint16_t*>(texels + job.dst + 2ull * local) = (uint16_t)p;
    else *reinterpret_cast<uint32_t*>(texels + job.dst + 4ull * local) = p;
}

// jobs: numJobs >= 1 records on the device of `st`, sorted by first_item, holding numItems destination texels in all.  Enqueues only
hipError_t LaunchMipLevel(hipStream_t st, const zrmg::Job* jobs, uint32_t numJobs, uint32_t numItems, uint8_t* texels)
{
    const uint32_t nb = (uint32_t)(((uint64_t)numItems + kMipBlock - 1) / kMipBlock);
    hipLaunchKernelGGL(k_mipgen_level, dim3(nb), dim3(kMipBlock), 0, st, jobs, numJobs, numItems, texels);
    return hipGetLastError();
}

} // namespace zr
