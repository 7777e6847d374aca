// zr_tu_texdecode.hip -- the device form of the BC7 / BC5 decode (zr_scene_create_compressed, zr_bcn_decode_device; include/zetaray_amd.h): the blocks
// of every mip of every block-compressed texture of a scene become RGBA8 / RG8 texels in the texture heap in ONE launch.  The arithmetic is
// include/zr_bcn.h's lane form, the header tests/bcnmath compiles for the host, so the heap is the host decoder's byte for byte.
//   k_bcn_decode   one lane per 4 x 4 block.  A lane finds its mip by binary search of its block index in the job table (zrbc::Job, sorted by first
//                  block; a 2048^2 chain is 12 jobs, 128 textures 1 536: at most 11 probes, all lanes of a wave but those at a mip boundary taking
//                  the same path through the same cached words), loads its 16 bytes once, and stores four rows.  Lanes follow the blocks of a block
//                  row, so a wave's stores of one texel row are 64 x 16 (BC7) or 64 x 8 (BC5) contiguous bytes.
// A row is stored as wide as its address allows: heap offsets are multiples of 4 only and a mip's width need not be a multiple of 4, so an RGBA8 row
// of a block is 16-, 8- or 4-byte aligned; an RG8 mip can start on any even byte (517 x 13 RG8 is 13 442 bytes), so its rows are 8-, 4- or 2-byte
// aligned.  Blocks cut by the right or bottom edge store texel by texel and drop what lies outside.
// RAW textures of the same scene are not jobs: their chain is contiguous in the payload and in the heap, the host enqueues one copy per texture.
#include <hip/hip_runtime.h>
#include "../../include/zr_bcn.h"

namespace zr {

static constexpr uint32_t kBcnBlock = 256;

__device__ inline void StoreRowRgba(uint8_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if ((addr & 15u) == 0u) *reinterpret_cast<uint4*>(p) = make_uint4(a, b, c, d);
    else if ((addr & 7u) == 0u) { reinterpret_cast<uint2*>(p)[0] = make_uint2(a, b); reinterpret_cast<uint2*>(p)[1] = make_uint2(c, d); }
    else { uint32_t* q = reinterpret_cast<uint32_t*>(p); q[0] = a; q[1] = b; q[2] = c; q[3] = d; }
}
// four RG8 texels, each in the low 16 bits of its argument
__device__ inline void StoreRowRg(uint8_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    const uint32_t lo = a | (b << 16), hi = c | (d << 16);
    if ((addr & 7u) == 0u) *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
    else if ((addr & 3u) == 0u) { uint32_t* q = reinterpret_cast<uint32_t*>(p); q[0] = lo; q[1] = hi; }
    else { uint16_t* q = reinterpret_cast<uint16_t*>(p); q[0] = (uint16_t)a; q[1] = (uint16_t)b; q[2] = (uint16_t)c; q[3] = (uint16_t)d; }
}

// payload: 16-byte aligned; every job's blocks lie inside it and its mip inside texels (the host checked both); texels: 4-byte aligned
__global__ void __launch_bounds__(kBcnBlock) k_bcn_decode(const zrbc::Job* jobs, uint32_t numJobs, uint32_t numBlocks, const uint8_t* payload, uint8_t* texels)
{
    const uint64_t g64 = (uint64_t)blockIdx.x * kBcnBlock + threadIdx.x;
    if (g64 >= numBlocks) return;
    const uint32_t g = (uint32_t)g64;
    const zrbc::Job job = jobs[zrbc::FindJob(jobs, numJobs, g)];
    const uint32_t local = g - job.first_block, bw = (job.w + 3u) >> 2;
    const uint32_t by = local / bw, bx = local - by * bw;
    const uint4 raw = *reinterpret_cast<const uint4*>(payload + job.src + 16ull * local);
    const zrbc::Block b = {raw.x, raw.y, raw.z, raw.w};
    const uint32_t x0 = 4u * bx, y0 = 4u * by;
    const bool whole = x0 + 4u <= job.w && y0 + 4u <= job.h;
    if (job.encoding == zrbc::kSrcBc7)
    {
        zrbc::Bc7 s;
        zrbc::Bc7Begin(b, s);
        uint8_t* dst = texels + job.dst + 4ull * ((uint64_t)y0 * job.w + x0);
        ZR_UNROLL
        for (uint32_t r = 0; r < 4u; r++)
        {
            const uint32_t p0 = zrbc::Bc7Texel(s, 4u * r), p1 = zrbc::Bc7Texel(s, 4u * r + 1u), p2 = zrbc::Bc7Texel(s, 4u * r + 2u), p3 = zrbc::Bc7Texel(s, 4u * r + 3u);
            uint8_t* row = dst + 4ull * r * job.w;
            if (whole) StoreRowRgba(row, p0, p1, p2, p3);
            else if (y0 + r < job.h)
            {
                uint32_t* q = reinterpret_cast<uint32_t*>(row);
                q[0] = p0;
                if (x0 + 1u < job.w) q[1] = p1;
                if (x0 + 2u < job.w) q[2] = p2;
                if (x0 + 3u < job.w) q[3] = p3;
            }
        }
    }
    else
    {
        uint8_t* dst = texels + job.dst + 2ull * ((uint64_t)y0 * job.w + x0);
        ZR_UNROLL
        for (uint32_t r = 0; r < 4u; r++)
        {
            const uint32_t p0 = zrbc::Bc5Texel(b, 4u * r), p1 = zrbc::Bc5Texel(b, 4u * r + 1u), p2 = zrbc::Bc5Texel(b, 4u * r + 2u), p3 = zrbc::Bc5Texel(b, 4u * r + 3u);
            uint8_t* row = dst + 2ull * r * job.w;
            if (whole) StoreRowRg(row, p0, p1, p2, p3);
            else if (y0 + r < job.h)
            {
                uint16_t* q = reinterpret_cast<uint16_t*>(row);
                q[0] = (uint16_t)p0;
                if (x0 + 1u < job.w) q[1] = (uint16_t)p1;
                if (x0 + 2u < job.w) q[2] = (uint16_t)p2;
                if (x0 + 3u < job.w) q[3] = (uint16_t)p3;
            }
        }
    }
}

// jobs: numJobs >= 1 records on the device of `st`, sorted by first_block, holding numBlocks blocks in all.  Enqueues only
hipError_t LaunchBcnDecode(hipStream_t st, const zrbc::Job* jobs, uint32_t numJobs, uint32_t numBlocks, const uint8_t* payload, uint8_t* texels)
{
    const uint32_t nb = (uint32_t)(((uint64_t)numBlocks + kBcnBlock - 1) / kBcnBlock);
    hipLaunchKernelGGL(k_bcn_decode, dim3(nb), dim3(kBcnBlock), 0, st, jobs, numJobs, numBlocks, payload, texels);
    return hipGetLastError();
}

} // namespace zr
