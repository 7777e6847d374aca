// zr_tu_jpeg.hip -- the device form of the JPEG decode behind the entropy decoder (zr_scene_create_compressed with ZR_TEX_SRC_JPEG_COEF sources,
// zr_jpeg_decode_device; include/zetaray_amd.h): every block and every level-0 texel of every JPEG texture of a call in one launch per kernel.  The
// arithmetic is include/zr_jpeg.h, the header the host loader compiles (zrh_jpeg_decode), so level 0 is the host's byte for byte.
//   k_jpeg_idct    one lane per 8 x 8 block.  A lane finds its component by binary search of its block index in the job table (zrjp::BlockJob, sorted by
//                  first block), reads its run of quantised coefficients (2 .. 128 bytes; the runs of a wave's blocks are contiguous), dequantises,
//                  transforms and stores eight rows of 8 bytes into the component's sample plane.  Lanes follow the blocks of a block row, so a wave
//                  stores 512 contiguous bytes per sample row.
//                  The 64 values stay in registers with constant indices through both passes.  The run cannot be scattered into such an array by its
//                  zigzag position (a computed index would put the array in scratch), so each lane owns a slot of LDS: 64 int16 zeroed, the run written
//                  to its natural positions, read back as 32 words with constant indices.  A slot is 33 words, not 32: word i of lane l then lies in bank
//                  (33 l + i) mod 32 = (l + i) mod 32, a different bank for each lane of a 32-lane half (the group within which ds_read_b32 and the
//                  writes conflict); at 32 words every lane would sit on bank i.  Slots are lane-private: no barrier.  One wave per work-group
//                  (8 448 B of LDS; 102 VGPRs, no scratch).
//   k_jpeg_texel   one lane per texel of level 0: y and the chroma taps from the planes (clamped to the component's real extent), the triangle filter,
//                  YCbCr -> RGB, the slot's channel map, one 4-byte (RGBA8) or 2-byte (RG8) store.  An RG8 level 0 can start on any even byte.
// The planes (u8, block-padded) live in a stream-ordered allocation between the two launches; the mip levels are then generated from level 0 as for a
// RAW_MIP0 source (zr_tu_mipgen.hip).
#include <hip/hip_runtime.h>
#include "../../include/zr_jpeg.h"

namespace zr {

static constexpr uint32_t kIdctBlock = 64, kIdctSlot = 33, kTexelBlock = 256;
typedef uint32_t __attribute__((may_alias)) SlotWord;      // a slot is written as int16 and read as words

// payload: 16-byte aligned; every job's record passed zrjp::CheckRecord and its plane lies inside planes (8-byte aligned)
__global__ void __launch_bounds__(kIdctBlock) k_jpeg_idct(const zrjp::BlockJob* jobs, uint32_t numJobs, uint32_t numBlocks, const uint8_t* payload, uint8_t* planes)
{
    __shared__ SlotWord slots[kIdctBlock * kIdctSlot];
    const uint64_t g64 = (uint64_t)blockIdx.x * kIdctBlock + threadIdx.x;
    if (g64 >= numBlocks) return;
    const uint32_t g = (uint32_t)g64;
    const zrjp::BlockJob* job = jobs + zrjp::FindFirst(jobs, numJobs, g, &zrjp::BlockJob::first_block);
    const uint32_t local = g - job->first_block, bw = job->bw;
    SlotWord* slot = slots + threadIdx.x * kIdctSlot;
    ZR_UNROLL
    for (uint32_t i = 0; i < 32u; i++) slot[i] = 0u;
    const uint32_t* cb = reinterpret_cast<const uint32_t*>(payload + job->coef_begin) + (job->comp_first + local);
    const uint32_t b0 = cb[0], n = cb[1] - b0;      // 1 .. 64
    const int16_t* run = reinterpret_cast<const int16_t*>(payload + job->coef) + b0;
    int16_t* slot16 = reinterpret_cast<int16_t*>(slot);
    for (uint32_t k = 0; k < n; k++) slot16[zrjp::ZZ[k]] = run[k];
    uint32_t v[64];
    ZR_UNROLL
    for (uint32_t i = 0; i < 32u; i++)
    {
        const uint32_t c = slot[i], q = job->q2[i];
        v[2u * i] = (uint32_t)(int32_t)(int16_t)(c & 0xffffu) * (q & 0xffffu);
        v[2u * i + 1u] = (uint32_t)((int32_t)c >> 16) * (q >> 16);
    }
    zrjp::Idct8x8(v);
    const uint32_t by = local / bw, bx = local - by * bw;
    uint8_t* o = planes + job->plane + (64ull * by * bw + 8ull * bx);
    ZR_UNROLL
    for (uint32_t r = 0; r < 8u; r++)
        *reinterpret_cast<uint2*>(o + 8ull * r * bw) = make_uint2(v[8u * r] | (v[8u * r + 1u] << 8) | (v[8u * r + 2u] << 16) | (v[8u * r + 3u] << 24),
                                                                  v[8u * r + 4u] | (v[8u * r + 5u] << 8) | (v[8u * r + 6u] << 16) | (v[8u * r + 7u] << 24));
}

// every job's planes were written by k_jpeg_idct on the same stream and its level 0 lies inside texels (the host checked); texels: 4-byte aligned
__global__ void __launch_bounds__(kTexelBlock) k_jpeg_texel(const zrjp::TexJob* jobs, uint32_t numJobs, uint32_t numItems, const uint8_t* planes, uint8_t* texels)
{
    const uint64_t g64 = (uint64_t)blockIdx.x * kTexelBlock + threadIdx.x;
    if (g64 >= numItems) return;
    const uint32_t g = (uint32_t)g64;
    const zrjp::TexJob job = jobs[zrjp::FindFirst(jobs, numJobs, g, &zrjp::TexJob::first_item)];
    const uint32_t local = g - job.first_item;
    const uint32_t y = local / job.w, x = local - y * job.w;
    const uint32_t p = zrjp::Texel(planes, job, x, y);
    if (job.map == (uint32_t)zrjp::kMapRgba) *reinterpret_cast<uint32_t*>(texels + job.dst + 4ull * local) = p;
    else *reinterpret_cast<uint16_t*>(texels + job.dst + 2ull * local) = (uint16_t)p;
}

// The two launches of a call.  blockJobs / texJobs: numBlockJobs / numTexJobs >= 1 records on the device of `st`, sorted by first_block / first_item,
// holding numBlocks blocks and numItems texels in all.  Enqueues only
hipError_t LaunchJpegDecode(hipStream_t st, const zrjp::BlockJob* blockJobs, uint32_t numBlockJobs, uint32_t numBlocks, const zrjp::TexJob* texJobs, uint32_t numTexJobs,
    uint32_t numItems, const uint8_t* payload, uint8_t* planes, uint8_t* texels)
{
    hipLaunchKernelGGL(k_jpeg_idct, dim3((uint32_t)(((uint64_t)numBlocks + kIdctBlock - 1) / kIdctBlock)), dim3(kIdctBlock), 0, st, blockJobs, numBlockJobs, numBlocks, payload, planes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_jpeg_texel, dim3((uint32_t)(((uint64_t)numItems + kTexelBlock - 1) / kTexelBlock)), dim3(kTexelBlock), 0, st, texJobs, numTexJobs, numItems, planes, texels);
    return hipGetLastError();
}

} // namespace zr
