// zr_api.hip -- HIP kernels (gfx950) and the C-ABI of libzetaray_amd.so (include/zetaray_amd.h).
//
// Kernel wrappers around the stage functions of zr_stages.h: pixel <-> lane mapping, wave-ballot stream compaction
// into the SoA path queues, ray counters, per-kernel hipEvent timing.  Host side: scene upload + BVH build, G-buffer
// planes, the pass objects mirroring the reference's RenderPass surface (citations in include/zetaray_amd.h).
// There is no CPU fallback in this library: without a usable HIP device every compute entry point fails loudly.
#include <hip/hip_runtime.h>
#include <immintrin.h>
#include <string>
#include <vector>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <new>
#include <mutex>
#include <unordered_map>
#include "zr_stages.h"
#include "zr_rpt.h"
#include "zr_rdi.h"
#include "zr_sdi.h"
#include "zr_rgi.h"
#include "zr_rgi_spatial.h"
#include "zr_bvh.h"
#include "zr_taa.h"
#include "zr_svgf.h"
#include "zr_post.h"
#include "zr_rpt_overlap.h"
#include "zr_pass_frame.h"
#include "../../include/zr_srgb_table.h"

// 512 x half2 spatial-search points (generated from zetaray_amd/assets/rpt_sample_set_f16.bin by the Makefile)
static const uint16_t kRptSampleSet[1024] = {
#include "zr_rpt_sample_set.inc"
};


// ------------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
static int Fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return Fail(ZR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// cross-stream ordering of the scene's buffers, the G-buffer's plane sets and the ReSTIR PT planes (zr_stream_order.h, zr_rpt_overlap.h) on HIP events
struct HipOrderBackend
{
    using Stream = hipStream_t; using Event = hipEvent_t;
    static int Create(Event* e) { HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming)); return ZR_OK; }
    static void Destroy(Event e) { (void)hipEventDestroy(e); }
    static int Record(Event e, Stream s) { HIP_TRY(hipEventRecord(e, s)); return ZR_OK; }
    static int Wait(Stream s, Event e) { HIP_TRY(hipStreamWaitEvent(s, e, 0)); return ZR_OK; }
};
using HipStreamOrder = zr::StreamOrder<HipOrderBackend>; using HipOrderPoints = zr::OrderPoints<HipOrderBackend>;

static int RequireDevice(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return Fail(ZR_ERR_NO_DEVICE, "no usable HIP device (hipGetDeviceCount: %s); libzetaray_amd has no CPU path", hipGetErrorString(e));
    if (device < 0 || device >= n) return Fail(ZR_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    return ZR_OK;
}

#include "zr_kernels.h"

// A/B switches of the measurement builds.  The product library has none: each reads as its default.  `make experiments` (-DZR_EXPERIMENTS ->
// libzetaray_amd_exp.so) turns them into environment variables read once per process.
#ifdef ZR_EXPERIMENTS
#define ZR_EXP_ENV(name) std::getenv(name)
#else
#define ZR_EXP_ENV(name) ((const char*)nullptr)
#endif
#include "zr_bvh_device.h"
#include "../../include/zr_anim.h"
#include <memory>
namespace zr { int DeviceProbeRun(int device, float min_ms, zr_device_probe* out, std::string& err); }      // zr_tu_probe.hip
namespace zr { hipError_t LaunchInscattering(hipStream_t s, const SceneView& sc, const zr_frame_constants& g, const InscatterParams& c, uint32_t* grid); }   // zr_tu_sky.hip
namespace zr { hipError_t LaunchDisplayView(hipStream_t s, int option, const GBuf& gb, uint32_t dw, uint32_t dh, float cameraNear, float roughnessTh, F4* out, uint32_t* outSrgb); }   // zr_tu_display.hip
namespace zr { hipError_t LaunchPickOutline(hipStream_t s, const zr_vertex* vertices, const uint32_t* indices, const zr_mesh_instance* instances, uint32_t inst, uint32_t numTris,
    const post::PickWvp& m, uint32_t dw, uint32_t dh, uint32_t rw, uint32_t rh, int4* tris, uint32_t* count, uint8_t* mask, F4* out, uint32_t* outSrgb); }   // zr_tu_display.hip
namespace zr { hipError_t LaunchMoveInstances(hipStream_t st, zr_mesh_instance* cur, const zr_mesh_instance* prev, float* toWorld, uint32_t n, uint32_t* slot,
    const uint32_t* moved, uint32_t nMoved, zr_emissive_triangle* emissives, const zr_emissive_triangle* object, const uint32_t* owner, uint32_t emFirst, uint32_t emEnd); }   // zr_tu_scene_update.hip
namespace zr { hipError_t LaunchAnimate(hipStream_t st, float t, const zr_anim_node* nodes, const zr_keyframe* keys, const uint32_t* animated, uint32_t nAnimated,
    const uint32_t* levelNodes, const uint32_t* levelOffsets, uint32_t numLevels, float* nodeLocal, float* nodeWorld, const uint32_t* instNode, uint32_t nInst, uint32_t* moved); }   // zr_tu_anim.hip
#include "zr_pose.h"      // zr_tu_pose.hip
namespace zr { hipError_t LaunchFillInstRecs(hipStream_t st, InstRec* recs, const zr_mesh_instance* instances, uint32_t n);      // zr_tu_scene_update.hip
               hipError_t LaunchFillVtxNormals(hipStream_t st, VtxDir* out, const zr_vertex* vertices, uint32_t n, bool tangent); }
namespace zr { size_t AliasScratchWords(uint32_t n);      // zr_tu_alias.hip
               hipError_t LaunchAliasBuild(hipStream_t st, const float* power, uint32_t n, zr_alias_entry* out, uint64_t* scratch); }
#include "zr_tex_plan.h"
namespace zr { hipError_t LaunchBcnDecode(hipStream_t st, const zrbc::Job* jobs, uint32_t numJobs, uint32_t numBlocks, const uint8_t* payload, uint8_t* texels); }   // zr_tu_texdecode.hip
namespace zr { hipError_t LaunchJpegDecode(hipStream_t st, const zrjp::BlockJob* blockJobs, uint32_t numBlockJobs, uint32_t numBlocks, const zrjp::TexJob* texJobs, uint32_t numTexJobs,
                   uint32_t numItems, const uint8_t* payload, uint8_t* planes, uint8_t* texels); }   // zr_tu_jpeg.hip
namespace zr { hipError_t LaunchMipLevel(hipStream_t st, const zrmg::Job* jobs, uint32_t numJobs, uint32_t numItems, uint8_t* texels); }   // zr_tu_mipgen.hip
// the ReSTIR PT kernels are compiled in zr_tu_rpt_[a-i].hip (see zr_kernels.h)
ZR_RPT_GROUPS_PRODUCT(extern template)
#ifdef ZR_EXPERIMENTS
ZR_RPT_GROUP_C(extern template)
#endif

// pickXY: x | y << 16 of the pixel to pick (render-target coordinates), 0xffffffff = none
__global__ void __launch_bounds__(kBlock) k_gbuffer(SceneView sc, zr_frame_constants g, GBuf gb, uint32_t tilesX, uint32_t pickXY, uint32_t* pick)
{
    uint32_t x, y; PixelOfThread(tilesX, gb.x0, gb.y0, &x, &y);
    if (x >= gb.x0 + gb.w || y >= gb.y0 + gb.h) return;
    ZR_TRAV_STACK(stack);
    GBufferPixel(sc, g, gb, x, y, stack, nullptr, (x | (y << 16)) == pickXY ? pick : nullptr);
}

// (PLAIN: the material-class permutation of the K9 stages, like K11's -- zr_rpt.h SetMaterialClass)
template<bool TEX, bool PLAIN>
__global__ void __launch_bounds__(kBlock) k_pt_init(SceneView sc, zr_frame_constants g, GBuf gb, PtParams prm, float* finalRGBA,
    F4* firstBOP, PathQueue out, uint32_t* outCount, uint32_t* outRays, uint32_t cap, uint32_t tilesX)
{
    sc.plain = PLAIN; gb.plain = PLAIN;
    uint32_t x, y; PixelOfThread(tilesX, gb.x0, gb.y0, &x, &y);
    PathOut po; po.alive = false;
    if (x < gb.x0 + gb.w && y < gb.y0 + gb.h) PtInitPixel(sc, g, gb, prm, x, y, finalRGBA, firstBOP, po, TEX);
    const uint32_t slot = AllocPathAndRaysBlock(outCount, out.rayList, cap, outRays, po.alive, po.alive && po.rayC_d.w >= 0, po.alive && po.rayM_d.w >= 0, po.alive && po.rayS_d.w >= 0);
    if (po.alive) WritePath(out, slot, po, TEX);
}

// trace stage, run-to-completion variant (default): grid-stride over the queue's compacted ray list
__global__ void __launch_bounds__(kBlock) k_trace_simple(SceneView sc, PathQueue q, const uint32_t* rayCount, uint32_t cap, unsigned long long* counters)
{
    const uint32_t nC = rayCount[0], nM = rayCount[kCounterStride], total = nC + nM + rayCount[2 * kCounterStride];
    ZR_TRAV_STACK(stack);
#ifdef ZR_NODE_CACHE_MORE
    ZR_NODE_CACHE_FILL(stack, sc, kBlock);
#endif
    for (uint32_t base = blockIdx.x * kBlock; base < total; base += gridDim.x * kBlock)
    {
        const uint32_t j = base + threadIdx.x;
        bool closest = false, shadow = false;
        if (j < total)
        {
            // one Traverse call site for the three ray types: a wave holds a mix of them
            uint32_t type, i;
            RayOfIndex(q.rayList, cap, nC, nM, j, type, i);
            F4 ro, rd;
            if (type == 0) { rd = q.rayC_d[i]; ro = q.rayC_o[i]; }
            else if (type == 1) { rd = q.rayM_d[i]; ro = q.rayM_o[i]; }
            else { rd = q.rayS_d[i]; ro = q.rayS_o[i]; }
            // S rays: segment to an emissive triangle (closest over NON_EMISSIVE) or sun / sky visibility (any hit over ALL)
            const uint32_t lightID = type == 2 ? q.sLightID[i] : 0u;
            const bool vis = type == 2 && lightID == kVisibilityRayID;
            const RawHit h = TraverseDyn(sc, xyz(ro), xyz(rd), ro.w, rd.w, (type == 2 && !vis) ? ZR_SUBGROUP_NON_EMISSIVE : ZR_SUBGROUP_ALL, stack, vis);
            if (type == 0) q.hitC[i] = PackRawHit(h);
            else if (type == 1) q.hitM[i] = PackRawHit(h);
            else q.visS[i] = SegmentVisible(sc, h, lightID);
            closest = type != 2; shadow = type == 2;
        }
        CountWave(&counters[0], closest);
        CountWave(&counters[1], shadow);
    }
}

// trace stage, persistent variant (ZR_TRACE_MODE=1).  Every lane owns one ray at a time; each iteration the wave votes
// for one phase -- refill idle lanes from the wave's chunk of ray slots, inner-node step, or one triangle test -- and runs
// the one most lanes are waiting for (the phases of Traverse, zr_dev_scene.h, plus the refill).  Waves take chunks of
// kTraceChunk entries of the compacted ray list from a global cursor.  Which lane traces which ray, and in which order,
// has no effect on the results.
static constexpr uint32_t kTraceChunk = 256;
static constexpr uint32_t kTraceRefillAt = 16;
__global__ void __launch_bounds__(kBlock) k_trace(SceneView sc, PathQueue q, const uint32_t* rayCount, uint32_t cap, uint32_t* cursor, unsigned long long* counters)
{
    const uint32_t nC = rayCount[0], nM = rayCount[kCounterStride], total = nC + nM + rayCount[2 * kCounterStride];
    ZR_TRAV_STACK(stack);
    const uint32_t lane = __lane_id();
    TravState st; TravLane L; L.triCur = 0; L.triEnd = 0; L.done = true;
    uint32_t slot = 0;                              // this lane's ray: list entry (slot | type << 30)
    bool laneAnyHit = false;
    uint32_t nClosest = 0, nShadow = 0;
    uint32_t chunkPos = 0, chunkEnd = 0;            // wave-uniform
    bool exhausted = false;                         // wave-uniform: the global cursor ran past `total`
    for (;;)
    {
        const bool atTri = L.triCur < L.triEnd;
        const bool atNode = !L.done && !atTri;
        const uint64_t mIdle = __ballot(L.done);
        const uint32_t nNode = (uint32_t)__popcll(__ballot(atNode)), nTri = (uint32_t)__popcll(__ballot(atTri)), nIdle = (uint32_t)__popcll(mIdle);
        const bool canRefill = !(exhausted && chunkPos == chunkEnd);
        if (nNode + nTri == 0 && !canRefill) break;
        if (canRefill && (nIdle >= kTraceRefillAt || nNode + nTri == 0))
        {
            if (chunkPos == chunkEnd)
            {
                uint32_t b = 0;
                if (lane == 0) b = atomicAdd(cursor, kTraceChunk);
                b = __builtin_amdgcn_readfirstlane(b);
                exhausted = b >= total;
                chunkPos = b < total ? b : total;
                chunkEnd = b + kTraceChunk < total ? b + kTraceChunk : total;
            }
            const uint32_t rank = (uint32_t)__popcll(mIdle & ((1ull << lane) - 1ull));
            const uint32_t j = chunkPos + rank;
            if (L.done && j < chunkEnd)
            {
                uint32_t type, i;
                RayOfIndex(q.rayList, cap, nC, nM, j, type, i);
                slot = i | (type << 30);
                F4 ro, rd;
                if (type == 0) { rd = q.rayC_d[i]; ro = q.rayC_o[i]; }
                else if (type == 1) { rd = q.rayM_d[i]; ro = q.rayM_o[i]; }
                else { rd = q.rayS_d[i]; ro = q.rayS_o[i]; }
                L.done = false;
                if (type == 2)
                {
                    laneAnyHit = q.sLightID[i] == kVisibilityRayID;
                    TravInit(sc, st, xyz(ro), xyz(rd), ro.w, rd.w, laneAnyHit ? ZR_SUBGROUP_ALL : ZR_SUBGROUP_NON_EMISSIVE, false, 0); nShadow++;
                }
                else { laneAnyHit = false; TravInit(sc, st, xyz(ro), xyz(rd), ro.w, rd.w, ZR_SUBGROUP_ALL, false, 0); nClosest++; }
                TravEnter(sc, st, L, st.cur);
            }
            chunkPos = chunkPos + nIdle < chunkEnd ? chunkPos + nIdle : chunkEnd;
            continue;
        }
        bool stepped = false;
        if (nNode >= nTri) { if (atNode) { TravNodePhase(sc, st, L, stack); stepped = true; } }
        else if (atTri) { TravTriPhase(sc, st, L, stack, laneAnyHit); stepped = true; }
        if (stepped && L.done)
        {
            // shadow segments run to the closest hit: visible iff it is the light's own triangle (TraceSegmentRay)
            const uint32_t type = slot >> 30, i = slot & 0x3fffffffu;
            if (type == 0) q.hitC[i] = PackRawHit(st.best);
            else if (type == 1) q.hitM[i] = PackRawHit(st.best);
            else q.visS[i] = SegmentVisible(sc, st.best, q.sLightID[i]);
        }
    }
    uint32_t a = nClosest, b = nShadow;
    for (int s = 1; s < 64; s <<= 1) { a += __shfl_xor(a, s); b += __shfl_xor(b, s); }
    if (lane == 0) { if (a) atomicAdd(&counters[0], (unsigned long long)a); if (b) atomicAdd(&counters[1], (unsigned long long)b); }
}

template<bool TEX>
__device__ __forceinline__ void PtShadeBody(const SceneView& sc, const zr_frame_constants& g, const PtParams& prm, const PathQueue& in, const uint32_t* inCount,
    const PathQueue& out, uint32_t* outCount, uint32_t* outRays, uint32_t cap, float* finalRGBA, const F4* firstBOP, uint32_t* groupMax)
{
    const uint32_t n = *inCount;
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock)
    {
        const uint32_t i = base + threadIdx.x;
        PathOut po; po.alive = false;
        if (i < n) PtShadePath(sc, g, prm, in, i, finalRGBA, firstBOP, groupMax, po, TEX);
        const uint32_t slot = AllocPathAndRaysBlock(outCount, out.rayList, cap, outRays, po.alive, po.alive && po.rayC_d.w >= 0, po.alive && po.rayM_d.w >= 0, po.alive && po.rayS_d.w >= 0);
        if (po.alive) WritePath(out, slot, po, TEX);
    }
}
template<bool PLAIN>
__global__ void __launch_bounds__(kBlock) k_pt_shade(SceneView sc, zr_frame_constants g, PtParams prm, PathQueue in, const uint32_t* inCount,
    PathQueue out, uint32_t* outCount, uint32_t* outRays, uint32_t cap, float* finalRGBA, const F4* firstBOP, uint32_t* groupMax)
{ sc.plain = PLAIN; PtShadeBody<false>(sc, g, prm, in, inCount, out, outCount, outRays, cap, finalRGBA, firstBOP, groupMax); }
// textured permutation: 258 VGPRs by default = 1 wave per SIMD; asking for 2 costs 2 registers and takes the atrium's shade
// stage from 8.6 to 5.6 ms per frame (the same request on the untextured kernel, 246 VGPRs, made it 10 % slower -- not applied)
#ifndef ZR_WAVES_PT_SHADE_TEX
#define ZR_WAVES_PT_SHADE_TEX ZR_WAVES_MIN(2)
#endif
__global__ void __launch_bounds__(kBlock) ZR_WAVES_PT_SHADE_TEX k_pt_shade_tex(SceneView sc, zr_frame_constants g, PtParams prm, PathQueue in, const uint32_t* inCount,
    PathQueue out, uint32_t* outCount, uint32_t* outRays, uint32_t cap, float* finalRGBA, const F4* firstBOP, uint32_t* groupMax)
{ sc.plain = 0; PtShadeBody<true>(sc, g, prm, in, inCount, out, outCount, outRays, cap, finalRGBA, firstBOP, groupMax); }

// Russian-roulette stage: finishes the vertices PtShadePath parked (only launched for rounds in which RR can trigger)
template<bool TEX>
__global__ void __launch_bounds__(kBlock) k_pt_rr(SceneView sc, PtParams prm, PathQueue q, const uint32_t* count, uint32_t* rays, uint32_t cap, const uint32_t* groupMax)
{
    sc.plain = 0;
    const uint32_t n = *count;
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock)
    {
        const uint32_t i = base + threadIdx.x;
        const bool cont = i < n && PtRussianRoulette(sc, prm, q, i, groupMax, TEX);
        AllocPathAndRaysBlock(nullptr, q.rayList, cap, rays, false, cont, false, false, true, i);
    }
}

// TAA: one thread per pixel; 9 signal + 9 depth reads from a 3 x 3 neighbourhood that the L2 serves after the first touch, 9 bilinear
// history fetches (36 half4 texels) around the reprojected position, one half4 store: HBM-bound (16 + 4 + 4 + 8 B read, 8 B written per
// pixel algorithmically)
#ifndef ZR_WAVES_TAA
#define ZR_WAVES_TAA
#endif
__global__ void __launch_bounds__(256) ZR_WAVES_TAA k_taa(taa::TaaFrame F)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < F.w * F.h) taa::TaaPixel(F, i % F.w, i / F.w);
}

// Denoise pass (zr_svgf.h): blocks of 32 x 8 pixels of the pass's planes (a window of the frame: the whole of it on one device, a tile + apron in
// the multi-GPU split), one thread per pixel.  The a-trous kernel is VALU-bound (r04: ~1.6 k VALU instructions per pixel in definition 1, SIMD VALU
// ~0.9 busy at 0.03 of the HBM roof): definition 2 of zr_svgf.h is what addresses that; the LDS tiles of the dense steps save the remaining tap latency.
__device__ __forceinline__ bool SvgfPixel(const svgf::Window& w, int* x, int* y)
{
    const int lx = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), ly = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    *x = w.ox + lx; *y = w.oy + ly;
    return lx < w.pw && ly < w.ph;
}
__global__ void __launch_bounds__(256) k_svgf_temporal(svgf::SvgfFrame F) { int x, y; if (SvgfPixel(F.win, &x, &y)) svgf::TemporalPixel(F, x, y); }
// POW: svgf_normal_power_log2 as a compile-time constant (7, the default: the squarings unroll) or -1 (read from the parameters)
template<int POW> __global__ void __launch_bounds__(256) k_svgf_variance(svgf::FilterFrame F) { int x, y; if (SvgfPixel(F.win, &x, &y)) svgf::VariancePixelT<POW>(F, x, y); }
// ROWLOOP: zr_svgf.h AtrousPixelT -- false = the 24 taps unrolled (held to 128 VGPRs: 4 waves per SIMD), true = a loop over the tap rows (8 waves)
template<int POW, bool ROWLOOP> __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_svgf_atrous(svgf::FilterFrame F)
{ int x, y; if (SvgfPixel(F.win, &x, &y)) { svgf::PlaneTaps t; t.srcP = (const U4*)F.src; t.guideZ = F.guideZ; t.win = F.win; svgf::AtrousPixelT<POW, ROWLOOP>(F, x, y, t); } }
// The same iteration with the block's (32 + 4 S) x (8 + 4 S) neighbourhood of both planes staged in LDS first (steps 1 and 2: 13.8 / 20.5 KB per block),
// so that the 25 taps + the 3 x 3 variance blur are ds_read_b128 instead of cache hits.  Same stage function, same results.  The default for
// steps 1 and 2 (RenderDenoise).  Tap positions arrive clamped into the planes, which keeps them inside the tile (a clamped position is nearer to the block
// than the unclamped one).
struct LdsTaps
{
    const ZR_LDS_AS F4* c; const ZR_LDS_AS F4* g; int x0, y0, tw;      // the tile holds the stage texels unpacked: (rgb, variance) and (n, z) in fp32
    __device__ __forceinline__ int RowBase(int y) const { return (y - y0) * tw - x0; }
    __device__ __forceinline__ void Load(int rb, int x, F4& gq, F4& q) const
    {
        const ZR_LDS_AS F4* a = c + rb + x; const ZR_LDS_AS F4* b = g + rb + x;
        q.x = a->x; q.y = a->y; q.z = a->z; q.w = a->w; gq.x = b->x; gq.y = b->y; gq.z = b->z; gq.w = b->w;
    }
    __device__ __forceinline__ float Var(int rb, int x) const { return (c + rb + x)->w; }
};
template<int S, int POW, bool ROWLOOP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_svgf_atrous_lds(svgf::FilterFrame F)
{
    constexpr int TW = 32 + 4 * S, TH = 8 + 4 * S;
    __shared__ F4 sC[TW * TH];
    __shared__ F4 sG[TW * TH];
    const svgf::Window& w = F.win;
    const int bx0 = w.ox + (int)(blockIdx.x * 32u) - 2 * S, by0 = w.oy + (int)(blockIdx.y * 8u) - 2 * S;
    for (int t = (int)threadIdx.x; t < TW * TH; t += 256)
    {
        const int gx = bx0 + t % TW, gy = by0 + t / TW;
        if (w.InPlanes(gx, gy)) { const size_t j = w.Idx(gx, gy); F4 gq, q; svgf::UnpackStage(((const U4*)F.src)[j], F.guideZ[j], gq, q); sC[t] = q; sG[t] = gq; }
    }
    __syncthreads();
    int x, y;
    if (!SvgfPixel(w, &x, &y)) return;
    LdsTaps taps; taps.c = (const ZR_LDS_AS F4*)sC; taps.g = (const ZR_LDS_AS F4*)sG; taps.x0 = bx0; taps.y0 = by0; taps.tw = TW;
    svgf::AtrousPixelT<POW, ROWLOOP>(F, x, y, taps);
}

// AutoExposure_Histogram.hlsl: per-block LDS histogram (256 bins = 256 threads), one global atomic per non-empty bin and block.
// in16 / in32: exactly one is non-null (RGBA16F plane, or RGBA32F read rounded to half).  HBM-bound: 8 (16) B read per pixel.
__global__ void __launch_bounds__(256) k_ae_histogram(const uint16_t* in16, const F4* in32, uint32_t n, post::AeParams prm, uint32_t* hist)
{
    __shared__ uint32_t bins[post::kHistBins];
    bins[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const V3 c = in16 ? post::LoadHalf3(in16, i) : post::HalfRounded(in32[i]);
        atomicAdd(&bins[post::AeBin(c, prm)], 1u);
    }
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(hist + threadIdx.x, bins[threadIdx.x]);
}
// AutoExposure_WeightedAvg.hlsl: one 256-thread group = 4 waves of 64; WaveActiveSum = the ABI's xor butterfly
__global__ void __launch_bounds__(256) k_ae_resolve(const uint32_t* hist, uint32_t numPixels, float dt, post::AeParams prm, float* exposure)
{
    const uint32_t gidx = threadIdx.x;
    float val = post::AeBinValue(gidx, gidx == 0 ? 0u : hist[gidx]);
    val = WaveSumButterfly(val);
    __shared__ float waveSum[4];
    if ((gidx & 63u) == 0) waveSum[gidx >> 6] = val;
    __syncthreads();
    float mean = gidx < 4 ? waveSum[gidx] : 0.0f;
    mean = WaveSumButterfly(mean);
    if (gidx == 0) post::AeResolve(mean, numPixels - hist[0], dt, prm, exposure);
}
// Display.hlsl mainPS: one thread per display pixel; point-clamp fetch of the render-resolution image
__global__ void __launch_bounds__(256) k_display(const uint16_t* in16, const F4* in32, uint32_t rw, uint32_t rh, uint32_t dw, uint32_t dh,
    const float* exposure, post::DisplayParams prm, post::Lut3D lut, F4* out, uint32_t* outSrgb)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dw * dh) return;
    const uint32_t x = i % dw, y = i / dw;
    const float u = ((float)x + 0.5f) / (float)dw, v = ((float)y + 0.5f) / (float)dh;
    int sx = (int)zr_floor(u * (float)rw), sy = (int)zr_floor(v * (float)rh);
    sx = sx < 0 ? 0 : (sx > (int)rw - 1 ? (int)rw - 1 : sx); sy = sy < 0 ? 0 : (sy > (int)rh - 1 ? (int)rh - 1 : sy);
    const size_t sp = (size_t)sy * rw + sx;
    // Texture2D<float4> on the composited texture: the stored (half) values
    const V3 c = in16 ? post::LoadHalf3(in16, sp) : post::HalfRounded(in32[sp]);
    const V3 d = post::DisplayPixel(c, (prm.autoExposure && exposure) ? exposure[0] : 1.0f, prm, lut);
    out[i] = f4(d, 1.0f);
    outSrgb[i] = post::LinearToSrgb8(d.x) | (post::LinearToSrgb8(d.y) << 8) | (post::LinearToSrgb8(d.z) << 16) | 0xff000000u;
}

// self-test of zr_detmath.h's half conversions (instruction path vs portable path), see zr_selftest_half_conversions
__global__ void __launch_bounds__(256) k_selftest_half(unsigned long long* bad)
{
    unsigned long long b0 = 0, b1 = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride)
    {
        const float f = zr_asfloat((uint32_t)i);
        if (zr_f32_to_f16(f) != zr_f32_to_f16_portable(f)) b0++;
        if (i < 65536u)
        {
            if (zr_asuint(zr_f16_to_f32((uint16_t)i)) != zr_asuint(zr_f16_to_f32_portable((uint16_t)i))) b1++;
            // the UNORM divisions by constant (zr_div255 / zr_div65535) against the IEEE division
            const float x = (float)(uint32_t)i;
            volatile float d255 = 255.0f, d65535 = 65535.0f;      // (volatile: keep real divisions)
            if (zr_asuint(zr_div255(x)) != zr_asuint(x / d255)) b1++;
            if (zr_asuint(zr_div65535(x)) != zr_asuint(x / d65535)) b1++;
        }
    }
    if (b0) atomicAdd(bad, b0);
    if (b1) atomicAdd(bad + 1, b1);
}

// Compositing: pure streaming kernel (2 + 16 + 16 B read, 16 B written per pixel)
__global__ void __launch_bounds__(256) k_composite(zr_frame_constants g, const uint16_t* mr, const F4* skyDI, const F4* emissiveDI, const F4* indirect, F4* out, uint32_t n,
    SkyLutView sky, uint32_t w)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = CompositePixel(g, mr[i], skyDI, emissiveDI, indirect, i, out[i], sky, i % w, i / w);
}
// Compositing with the inscattering voxel grid bound (zr_pass_bind_inscattering): + 4 B depth read and the grid's 8 texels per pixel
__global__ void __launch_bounds__(256) k_composite_inscattering(zr_frame_constants g, const uint16_t* mr, const float* depth, const F4* skyDI, const F4* emissiveDI,
    const F4* indirect, F4* out, uint32_t n, SkyLutView sky, uint32_t w, InscatterGridView grid)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F4 c = CompositePixel(g, mr[i], skyDI, emissiveDI, indirect, i, out[i], sky, i % w, i / w);
    out[i] = CompositeInscattering(g, mr[i], c, depth[i], grid, i % w, i / w);
}

// Firefly filter (FireflyFilter.hlsl): a 3 x 3 stencil over RGBA32F + depth.  A block filters a 64 x 16 pixel tile, 4 pixels per thread;
// colour and depth of the tile and its 1-pixel border are staged through LDS once (66 x 18 texels x 20 B = 23.8 KB, rows of 1 KB so the
// global loads coalesce and ~5 of them are in flight per thread), so every texel leaves HBM / L2 once per block instead of 9 times per
// pixel: 20 B read + 16 B written per pixel, HBM-bound.
static constexpr int kFfW = 64, kFfH = 16, kFfLW = kFfW + 2, kFfLH = kFfH + 2;
__global__ void __launch_bounds__(256) k_firefly(const F4* in, const float* depth, F4* out, uint32_t W, uint32_t H)
{
    __shared__ F4 sCol[kFfLW * kFfLH];
    __shared__ float sDep[kFfLW * kFfLH];
    const int bx = (int)blockIdx.x * kFfW, by = (int)blockIdx.y * kFfH;
    for (int t = threadIdx.x; t < kFfLW * kFfLH; t += 256)
    {
        const int lx = t % kFfLW, ly = t / kFfLW;
        const int gx = bx + lx - 1, gy = by + ly - 1;
        const bool inside = gx >= 0 && gy >= 0 && gx < (int)W && gy < (int)H;
        sCol[t] = inside ? in[(size_t)gy * W + gx] : f4(v3(0.0f), 0.0f);
        sDep[t] = inside ? depth[(size_t)gy * W + gx] : ZR_FLT_MAX;
    }
    __syncthreads();
    auto col = [&](int tx, int ty) { return xyz(sCol[ty * kFfLW + tx]); };
    auto dep = [&](int tx, int ty) { return sDep[ty * kFfLW + tx]; };
    for (int k = 0; k < 4; k++)
    {
        const int lx = threadIdx.x & 63, ly = (threadIdx.x >> 6) + 4 * k;
        const int x = bx + lx, y = by + ly;
        if (x >= (int)W || y >= (int)H) continue;
        const F4 c = sCol[(ly + 1) * kFfLW + lx + 1];
        V3 color = xyz(c);
        if (sDep[(ly + 1) * kFfLW + lx + 1] != ZR_FLT_MAX) color = FireflyClamp(col, dep, lx + 1, ly + 1, x, y, (int)W, (int)H, color);
        out[(size_t)y * W + x] = f4(color, c.w);
    }
}

__global__ void k_presample(SceneView sc, uint32_t total, uint32_t frameNum, uint32_t numEmissives, zr_presampled_tri* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) out[i] = PresampleEmissive(sc, i, frameNum, numEmissives);
}

__global__ void k_estimate_power(SceneView sc, uint32_t n, float* power)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) power[i] = EstimateTriPower(sc, sc.emissives[i]);
}

__device__ __forceinline__ float WaveSumButterfly(float v);
// K4 light voxel grid: one wave64 per voxel = the reference's 64-thread group; the group sums are wave reductions
__global__ void __launch_bounds__(64) k_build_lvg(SceneView sc, zr_frame_constants g, uint32_t dx, uint32_t dy, uint32_t dz, float ex, float ey, float ez,
    float offset_y, zr_voxel_sample* out)
{
    const uint32_t dim[3] = {dx, dy, dz};
    const int v[3] = {(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
    zr_voxel_sample r; float w_sum, target_z; uint32_t numLights;
    LvgThread(sc, g, dim, v3(ex, ey, ez), offset_y, v, threadIdx.x, r, w_sum, target_z, numLights);
    const float w_sum_group = WaveSumButterfly(w_sum);
    uint32_t n = numLights;
    for (int s = 1; s < 64; s <<= 1) n += __shfl_xor(n, s);
    LvgFinish(r, target_z, w_sum_group, n);
    out[(size_t)LvgFlatten(v, dim) * ZR_LVG_SAMPLES_PER_VOXEL + threadIdx.x] = r;
}

// K17 sky-view LUT: one thread per texel, 8 x 8 threads per group like the reference (ALU-bound: ~300 exp per texel)
__global__ void __launch_bounds__(64) k_sky_lut(zr_frame_constants g, uint32_t w, uint32_t h, uint32_t* out)
{
    const uint32_t x = blockIdx.x * 8 + (threadIdx.x & 7), y = blockIdx.y * 8 + (threadIdx.x >> 3);
    if (x < w && y < h) out[(size_t)y * w + x] = SkyViewLutTexel(g, x, y, w, h);
}

// generic ray-query kernels behind zr_trace_closest / zr_trace_any
__global__ void __launch_bounds__(kBlock) k_trace_rays(SceneView sc, const F4* rays, uint32_t n, uint32_t mask, U4* hits)
{
    ZR_TRAV_STACK(stack);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
        hits[i] = TraceClosestRay(sc, rays[2 * i], rays[2 * i + 1], mask, stack);
}
__global__ void __launch_bounds__(kBlock) k_trace_rays_any(SceneView sc, const F4* rays, uint32_t n, uint32_t mask, uint32_t* occ)
{
    ZR_TRAV_STACK(stack);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
    {
        const F4 ro = rays[2 * i], rd = rays[2 * i + 1];
        RawHit h = Traverse<true>(sc, xyz(ro), xyz(rd), ro.w, rd.w, mask, stack);
        occ[i] = h.tri != kInvalidTri ? 1u : 0u;
    }
}

// ------------------------------------------------------------------------------------------------ direct-lighting and ReSTIR GI kernels
// K5 - K8 and K10 are defined in zr_tu_di.hip (a translation unit of their own: zr_api.hip was the build's long pole); launched from here through their host stubs.
// threads per block (see kRptBlock in zr_kernels.h): one-wave blocks pay for the emissive DI kernels (K5 0.580 -> 0.568 ms
// Cornell, 5.42 -> 5.12 ms atrium; K6 0.258 -> 0.241 / 2.99 -> 2.61 ms), not for the sun + sky ones (K7 / K8 within +-0.6 %)
#include "zr_kernels_di.h"
// the spatial reuse stage of ReSTIR GI: defined in zr_tu_rgi_spatial.hip, launched by RenderReSTIR_GI
__global__ void k_rgi_spatial(rgi::GiFrame F, zr_frame_constants g, uint32_t tilesX, unsigned long long* counters, rgi::SpatialParams sp);
ZR_DI_GROUP(extern template, false)
ZR_DI_GROUP(extern template, true)
static const uint16_t kRdiSampleSet[64] = {
#include "zr_rdi_sample_set.inc"
};

// ------------------------------------------------------------------------------------------------ host objects
template<typename T> struct DevBuf
{
    T* p = nullptr; size_t n = 0;
    int Alloc(size_t count) { Free(); n = count; if (!count) return ZR_OK; hipError_t e = hipMalloc((void**)&p, count * sizeof(T)); if (e != hipSuccess) { p = nullptr; return Fail(ZR_ERR_OOM, "hipMalloc(%zu B) failed: %s", count * sizeof(T), hipGetErrorString(e)); } return ZR_OK; }
    // ... and clears it on the null stream (asynchronous to the host: see zr_pass_init)
    int AllocZero(size_t count) { int r = Alloc(count); if (r) return r; HIP_TRY(hipMemset(p, 0, count * sizeof(T))); return ZR_OK; }
    int Upload(const T* src, size_t count) { int r = Alloc(count); if (r) return r; if (count) HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice)); return ZR_OK; }
    void Free() { if (p) { (void)hipFree(p); p = nullptr; } n = 0; }
    void Swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }
    // at least `count` elements, the first `keep` of them kept (a blocking copy into a new allocation; nothing happens to a buffer that is large enough)
    int Grow(size_t count, size_t keep) { if (n >= count) return ZR_OK; DevBuf nb; int r = nb.Alloc(count); if (r) return r; if (keep && p) HIP_TRY(hipMemcpy(nb.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice)); Swap(nb); return ZR_OK; }
    ~DevBuf() { Free(); }
};
// What a trace binds that a frame's instance update replaces: the instance records and their decoded table (zr_hit_tables.h), the BVH4's nodes and triangle
// slots, the global (mesh, primitive) table.  A buffer's n is its CAPACITY; numNodes / numTris say how much of nodes / tris the tree in them uses.
struct AccelSet
{
    DevBuf<zr_mesh_instance> instances; DevBuf<InstRec> instRecs; DevBuf<Bvh4Node> nodes; DevBuf<BvhTri> tris; DevBuf<TriMeta> meta;
    uint32_t numNodes = 0, numTris = 0;
};
struct HaloPlane { void* base; size_t bpp; };
// A per-pixel device plane: PER_PIXEL elements of T for every pixel.  This declaration is the one statement of the plane's layout -- allocation, the
// clear, halo transfers and zr_pass_get_output all take its bytes per pixel from here.  Alloc / AllocZero count pixels; n goes on counting elements.
template<typename T, size_t PER_PIXEL = 1> struct Plane : DevBuf<T>
{
    static constexpr size_t bpp = sizeof(T) * PER_PIXEL;
    int Alloc(size_t pixels) { return DevBuf<T>::Alloc(pixels * PER_PIXEL); }
    int AllocZero(size_t pixels) { return DevBuf<T>::AllocZero(pixels * PER_PIXEL); }
    size_t Pixels() const { return this->n / PER_PIXEL; }
    HaloPlane Halo() const { return {this->p, bpp}; }
    void Output(void** dev, uint32_t* bytesPerPixel) const { *dev = this->p; if (bytesPerPixel) *bytesPerPixel = (uint32_t)bpp; }      // zr_pass_get_output
};
// ... and a set of planes (zr_pass::ResStorage / RBufStorage): S::Each(set, f) calls f on each plane in the set's order and stops at the first error
template<typename S> static int PlanesAllocZero(S& set, size_t pixels) { return S::Each(set, [&](auto& pl) { return pl.AllocZero(pixels); }); }
template<typename S> static int PlanesHalo(const S& set, HaloPlane* out) { int n = 0; S::Each(set, [&](const auto& pl) { out[n++] = pl.Halo(); return 0; }); return n; }
template<typename S> static void PlanesOutput(const S& set, int i, void** dev, uint32_t* bpp) { S::Each(set, [&](const auto& pl) { if (i-- == 0) pl.Output(dev, bpp); return 0; }); }

struct zr_scene
{
    int device = 0;
    DevBuf<zr_vertex> vertices; DevBuf<uint32_t> indices; DevBuf<zr_material> materials;
    DevBuf<zr_emissive_triangle> emissives; DevBuf<zr_alias_entry> alias;
    // The current and the previous acceleration structure + instance buffer (RT_SCENE_BVH_PREV / RT_FRAME_MESH_INSTANCES_PREV of the temporal passes):
    //  * they change roles in SceneFlip and nowhere else -- whole sets, capacities and counts with the pointers -- once per instance update of any form;
    //    `prev` is bound only while hasPrev (FrameViewPrev: before the first update, and after a rolled-back rebuild, the temporal passes bind `cur`)
    //  * `view` takes a set's buffers and counts through SceneBind only; view.numNodes / numTris are what kernels and zr_scene_bvh_info read,
    //    cur.numNodes / numTris the host's statement of the same values
    //  * refitReady: both sets hold the same topology (SceneDuplicate made `prev` a copy of `cur`, only refits followed), so the set that becomes current
    //    is refit in place; a rebuild or the install of a background tree clears it, and the next refit duplicates first
    AccelSet cur, prev; bool hasPrev = false, refitReady = false;
    // material class (SceneView::plain): host copy of the material table + "every material is an opaque uncoated non-metallic dielectric"; kept current by
    // zr_scene_create / zr_scene_update_materials on the calling thread, read by zr_pass_render when it picks a kernel permutation
    std::vector<zr_material> hMaterials; std::atomic<bool> plainMaterials{false};
    // identity of this scene for the G-buffers rendered from it (zr_gbuffer::sceneAt): never reused, unlike an address
    uint64_t uid = [] { static std::atomic<uint64_t> next{1}; return next.fetch_add(1); }();
    DevBuf<uint16_t> rho;
    DevBuf<zr_texture_desc> texDescs; DevBuf<uint8_t> texels; DevBuf<float> srgb;   // material texture heap (zr_texture.h)
    DevBuf<zr_presampled_tri> sampleSets; uint32_t numSampleSets = 0;      // K3 output, refreshed by every PRELIGHTING render
    DevBuf<zr_voxel_sample> lvg;                                           // K4 output, rebuilt by every PRELIGHTING render when use_lvg
    std::vector<zr_alias_entry> aliasHost;
    // dynamic instances (zr_scene_update_instances): host copies of what a BVH rebuild needs
    std::vector<zr_vertex> hVertices; std::vector<uint32_t> hIndices; std::vector<uint8_t> hMask; std::vector<uint32_t> hNumTris;
    // what hit reconstruction decodes from a vertex normal, stored once (zr_hit_tables.h; the instance records' table is part of each AccelSet)
    DevBuf<VtxDir> vtxNormals;
#if ZR_HIT_TANGENTS
    DevBuf<VtxDir> vtxTangents;
#endif
    // device refit of `cur`: node indices grouped by tree level (deepest level first) + the offsets of the groups, per-node float bounds, object-to-world matrices
    DevBuf<uint32_t> levelNodes; std::vector<uint32_t> levelOffsets, hLevelOrder; DevBuf<float> nodeBounds, toWorld;
    // device-side BVH build (zr_tu_bvh.hip): instance masks on the device, scratch buffers kept between builds
    DevBuf<uint8_t> dMask; DeviceBvhScratch bvhScratch; bool deviceBuilt = false;
    bool aliasStale = false;      // zr_scene_invalidate_alias_table_deferred: the old table stays bound until the rebuilt one has been uploaded
    // zr_scene_set_alias_build: ZR_ALIAS_BUILD_DEVICE builds the table in `alias` with the kernels of zr_tu_alias.hip on the PRELIGHTING render's stream.
    // aliasScratch: their scratch words, sized once per emissive count.  aliasOnDevice: the bound table was built there, so aliasHost is empty and
    // zr_scene_get_alias_table reads the device buffer back
    int aliasBuild = ZR_ALIAS_BUILD_HOST; DevBuf<uint64_t> aliasScratch; bool aliasOnDevice = false;
    // `view` is what kernels receive by value.  Passes of one dependency level may record concurrently from several host threads
    // (RenderGraph.cpp:442-541) while Sky / PreLighting publish scene-owned state (sky LUT, alias table, presampled sets, LVG):
    // every reader takes a private copy through FrameView() and every writer updates `view` under `mtx`.
    SceneView view{};
    mutable std::mutex mtx;
    int64_t maxTex[4] = {-1, -1, -1, -1};     // largest tex16 used per table (base colour, normal, metallic-roughness, emissive)
    uint32_t maxDepth = 0;
    // ---- stream-ordered updates (zr_scene_update_*_async; RtAccelerationStructure.cpp:708-789 records them on the frame's command list).
    // Host records travel through a ring of pinned staging buffers (a slot is reused only after its copy has run); `order` takes an update as a
    // write of the scene's buffers and a render as a read: renders on OTHER streams wait for the last update, and an update waits for the last
    // render of every other stream before it overwrites what those renders read (guarded by mtx).
    struct StageSlot { void* host = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool pending = false; };
    StageSlot stage[4]; int stageNext = 0;
    mutable HipOrderPoints points; mutable HipStreamOrder order;
    bool HasUpdate() const { return order.LastWriter(nullptr); }
    // ---- background SAH rebuild (zr_scene_set_background_rebuild; VERDICT r3 item 9, RtAccelerationStructure.cpp:708-789 rebuilds its TLAS every frame).
    // The device refit keeps the topology of the last build, and a tree built for where the instances WERE gets worse the further they move.  With this
    // on, an update that finds no build in flight snapshots the new transforms and starts the host's binned-SAH builder on a thread; the first update
    // after it has finished uploads the new topology into the buffer set that is about to become current and refits THAT to the transforms of the
    // update at hand.  No render waits, no result depends on the tree (include/zr_intersect.h's tie-break), the previous structure stays what it was.
    // What the build thread hands over is the TOPOLOGY only, packed in pinned memory by the thread itself: [4 child references per node | the scene
    // triangle each leaf slot holds | node ids level by level] -- 3.6 MB for the 380 k-triangle atrium, where whole node + triangle arrays are 24.8 MB.
    // Everything else in a node (origin, scales, quantised planes) and in a triangle slot (vertices, mask, ID) is recomputed on the device for the
    // transforms of the installing update (k_install_topology, then the refit kernels), so the installing update costs the host three async copies.
    struct Background
    {
        bool enabled = false; std::thread th; std::atomic<int> state{0};      // 0 idle, 1 building, 2 built
        std::vector<uint32_t> levelOffsets;
        uint32_t numNodes = 0, numTris = 0, stackNeed = 0, maxDepth = 0; bool packed = false;
        uint32_t* pkg = nullptr; size_t pkgCap = 0; hipEvent_t pkgCopied = nullptr; bool pkgInFlight = false;      // pkgCap in words
        std::vector<zr_mesh_instance> inst; std::vector<float> xf; std::vector<uint8_t> own;
        uint32_t refitsSince = 0; std::atomic<uint64_t> started{0}, installed{0};      // (atomic: zr_scene_background_rebuild_stats may read them from another thread)
        bool movedSinceBuild = false;      // a transform changed since the last build was started: updates that repeat the same matrices start no build
        double buildMs = 0, packMs = 0;
    } bg;
    DevBuf<uint32_t> bgDev;                      // device side of the package (children + slot triangles)
    // instances whose transform has ever changed: the background build gives each a subtree of its own (zr_bvh.h Build, ownSubtree)
    std::vector<float> hToWorld; std::vector<uint8_t> movedEver;
    // ---- the device form of the update (zr_scene_move_instances; kernels in zr_tu_scene_update.hip): the object-space light records and the instance that
    // carries each (zr_scene_set_object_emissives), the frame's moved list [n_moved x 12 floats | n_moved indices] and each instance's position in it
    // (0xffffffff between updates).  hInstances: the records as the host last stated them -- their static fields (mesh offsets, first light triangle)
    // are what the background builder and the dirty light range need when the caller hands over matrices only.  toWorldDev: `toWorld` holds hToWorld
    std::vector<zr_mesh_instance> hInstances; bool toWorldDev = false;
    DevBuf<zr_emissive_triangle> objectEmissives; DevBuf<uint32_t> emissiveOwner, movedDev, movedSlot;
    // ---- keyframe animation (zr_scene_set_animation / zr_scene_animate; kernels in zr_tu_anim.hip, arithmetic in include/zr_anim.h).  Host copies of the
    // tables (desc points into them), what set_animation derives once -- the animated nodes, the nodes grouped by level (top level first) and the groups'
    // offsets, the dirty light range of the listed instances -- and the device side: the tables, every node's local and world matrix (the non-animated
    // nodes' local matrices written at set time) and the scene-owned moved list [n x 12 floats | n indices] with its index half written at set time.
    // The host's view of the matrices (hToWorld) follows an animate LAZILY: lastT is kept, and SceneAnimSyncHost runs the header on the host for it at the
    // places that read hToWorld.
    struct Anim
    {
        std::vector<zr_anim_node> nodes; std::vector<zr_keyframe> keys; std::vector<uint32_t> instIdx, instNode, levelOffsets;
        zr_anim_desc desc{}; uint32_t nAnimated = 0, emFirst = 0, emEnd = 0;
        DevBuf<zr_anim_node> dNodes; DevBuf<zr_keyframe> dKeys; DevBuf<uint32_t> dAnimated, dLevelNodes, dInstNode, dMoved; DevBuf<float> dLocal, dWorld;
        float lastT = 0; bool hasT = false, hostStale = false;
    };
    std::unique_ptr<Anim> anim; std::mutex animMtx;
    // ---- skinned meshes (zr_scene_set_skinning; kernels in zr_tu_pose.hip, arithmetic in include/zr_skin.h): with a set, every zr_scene_animate also poses
    // the listed vertex ranges from their rest records.  What set_skinning lays out once: the joints' nodes and inverse bind matrices as two arrays (48-byte
    // matrices: 16-byte rows), the influences, and the joint matrices the frame's first kernel writes.  ranges: the caller's, which a later set_morph is
    // checked and laid out against
    struct Skin
    {
        std::vector<zr_skin_range> ranges; uint32_t numJoints = 0;
        DevBuf<uint32_t> dJointNode; DevBuf<float> dInverseBind, dJ; DevBuf<zr_skin_influence> dInfluences;
    };
    std::unique_ptr<Skin> skin;
    // ---- morph targets (zr_scene_set_morph; kernels in zr_tu_pose.hip, arithmetic in include/zr_morph.h): with a set, every zr_scene_animate also samples
    // the tracks' weights into dWeights (track after track) and poses the listed ranges.  What set_morph lays out once: the tables, each weight's track
    // and each track's first weight
    struct Morph
    {
        uint32_t numWeights = 0;
        DevBuf<zr_morph_track> dTracks; DevBuf<zr_morph_target> dTargets; DevBuf<uint32_t> dTrackOfWeight, dWeightFirst;
        DevBuf<float> dTimes, dValues, dRestWeights, dDeltas, dWeights;
    };
    std::unique_ptr<Morph> morph;
    // ---- what the two sets pose each frame (ScenePoseRebuild is the one writer): the ranges of both as one list (zr_pose.h) -- the skin-only ranges in the
    // skin set's order, then the morph set's in its order, a range both list once -- and the ranges' rest records, range after range, on the device and
    // (hRest, same layout) on the host: what a range goes back to when its set goes.  hVertices keeps the rest pose (only the background builder reads it: topology)
    // lights: the light triangles with a vertex in one of the ranges, by triangle index (zr::LightEntry; from hIndices and hInstances), which every
    // zr_scene_animate re-derives behind the instance kernels (k_refresh_emissives, listed form); hLightObject / hLightWorld: their object-space and world
    // records as the first set that listed them found them, entry after entry -- what they go back to with the rest vertices
    struct Pose
    {
        std::vector<zr::PoseRange> ranges; std::vector<zr_vertex> hRest; DevBuf<zr_vertex> dRest;
        std::vector<zr::LightEntry> lights; std::vector<zr_emissive_triangle> hLightObject, hLightWorld; DevBuf<zr::LightEntry> dLights;
        std::vector<uint32_t> lightOwner; std::vector<float> hLightXf;      // each entry's instance, and its matrix (12 floats) when the records were saved
    } pose;
    // zr_scene_update_vertices while a background build reads hVertices: the ranges wait here and reach hVertices once the builder's thread is done
    // (SceneFlushVertexCopies) -- the builder delivers topology, so the pose it saw does not matter, and the call does not wait for it
    std::vector<std::pair<uint32_t, std::vector<zr_vertex>>> hVertexPending;
    ~zr_scene()
    {
        if (bg.th.joinable()) bg.th.join();
        if (bg.pkg) (void)hipHostFree(bg.pkg);
        if (bg.pkgCopied) (void)hipEventDestroy(bg.pkgCopied);
        for (StageSlot& t : stage) { if (t.ev) (void)hipEventDestroy(t.ev); if (t.host) (void)hipHostFree(t.host); }
    }
};

// a pinned staging buffer of >= bytes whose previous transfer (if any) has completed; the caller fills it, enqueues its copy on `st`
// and calls StageCommit
static int StageAcquire(zr_scene* s, size_t bytes, zr_scene::StageSlot** out)
{
    zr_scene::StageSlot& t = s->stage[s->stageNext];
    s->stageNext = (s->stageNext + 1) % 4;
    if (t.pending) { HIP_TRY(hipEventSynchronize(t.ev)); t.pending = false; }      // only blocks when the host runs > 4 updates ahead of the device
    if (!t.ev) HIP_TRY(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
    if (t.cap < bytes)
    {
        if (t.host) { (void)hipHostFree(t.host); t.host = nullptr; t.cap = 0; }
        hipError_t e = hipHostMalloc(&t.host, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { t.host = nullptr; return Fail(ZR_ERR_OOM, "hipHostMalloc(%zu B) failed: %s", bytes, hipGetErrorString(e)); }
        t.cap = bytes;
    }
    *out = &t;
    return ZR_OK;
}
static int StageCommit(zr_scene::StageSlot* t, hipStream_t st) { HIP_TRY(hipEventRecord(t->ev, st)); t->pending = true; return ZR_OK; }
// an update on `st` must not overwrite what renders enqueued on other streams still read, and updates on different streams are ordered against
// each other (a render then only has to wait for the latest update: SceneAcquireForRender)
static int SceneWaitUsers(zr_scene* s, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(s->mtx);
    // the FIRST update of a scene: renders have not been marked yet (SceneReleaseAfterRender starts doing so once there has been an update, so
    // that static scenes pay nothing), and kernels of earlier frames on non-blocking streams may still read the buffers this update overwrites
    // in place -- wait for the device once.  (Not legal inside a stream capture: capture a scene's update path only after its first update.)
    if (!s->HasUpdate()) HIP_TRY(hipDeviceSynchronize());
    return s->order.AcquireWrite(s->points, st);
}
static int SceneMarkUpdatedLocked(zr_scene* s, hipStream_t st) { return s->order.MarkWritten(s->points, st); }      // (the caller holds mtx)
static int SceneMarkUpdated(zr_scene* s, hipStream_t st) { std::lock_guard<std::mutex> lock(s->mtx); return s->order.MarkWritten(s->points, st); }
// cur <-> prev: the only place the two sets change roles (the caller holds mtx, and has ordered `st` behind the readers of both: SceneWaitUsers)
static void SceneFlip(zr_scene* s)
{
    AccelSet &a = s->cur, &b = s->prev;
    a.instances.Swap(b.instances); a.instRecs.Swap(b.instRecs); a.nodes.Swap(b.nodes); a.tris.Swap(b.tris); a.meta.Swap(b.meta);
    std::swap(a.numNodes, b.numNodes); std::swap(a.numTris, b.numTris); s->hasPrev = true;
}
// ... and the only place a view takes a set's buffers and counts
static void SceneBind(SceneView& v, const AccelSet& a)
{
    v.instances = a.instances.p; v.instRecs = a.instRecs.p; v.nodes = a.nodes.p; v.tris = a.tris.p; v.triMeta = a.meta.p;
    v.numNodes = a.numNodes; v.numTris = a.numTris;
}
// a render on `st`: behind the last update if that ran on another stream ...
static int SceneAcquireForRender(const zr_scene* sc, hipStream_t st) { std::lock_guard<std::mutex> lock(sc->mtx); return sc->order.AcquireRead(sc->points, st); }
// ... and remembered as a reader of the scene's buffers (only once the scene has ever been updated: static scenes pay nothing)
static int SceneReleaseAfterRender(const zr_scene* sc, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(sc->mtx);
    return sc->HasUpdate() ? sc->order.MarkRead(sc->points, st) : ZR_OK;
}

// The scene as one launch sees it: a private copy of the scene's view with the texture descriptor-table offsets of THIS frame's
// constants (per-frame data in the reference, FrameConstants.h:31-34) -- nothing per-frame is latched on the shared scene.
#ifdef ZR_PROF
// measurement build only (scripts/gpu.sh prof): 8 kernels x 32 wave-cycle / event counters, read and cleared by zr_debug_prof_read
static unsigned long long* ProfBuffer()
{
    static unsigned long long* p = nullptr;
    if (!p) { (void)hipMalloc(&p, 256 * sizeof(unsigned long long)); (void)hipMemset(p, 0, 256 * sizeof(unsigned long long)); }
    return p;
}
extern "C" int zr_debug_prof_read(unsigned long long* out256)
{
    (void)hipDeviceSynchronize();
    if (hipMemcpy(out256, ProfBuffer(), 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    (void)hipMemset(ProfBuffer(), 0, 256 * sizeof(unsigned long long));
    return 0;
}
#endif
static SceneView FrameView(const zr_scene* sc, const zr_frame_constants* cb)
{
    std::lock_guard<std::mutex> lock(sc->mtx);
    SceneView v = sc->view;
#ifdef ZR_PROF
    v.prof = ProfBuffer();
#endif
    if (cb)
    {
        v.baseColorMapsOffset = cb->base_color_maps_desc_heap_offset; v.normalMapsOffset = cb->normal_maps_desc_heap_offset;
        v.mrMapsOffset = cb->metallic_roughness_maps_desc_heap_offset; v.emissiveMapsOffset = cb->emissive_maps_desc_heap_offset;
    }
    v.texFilter = ZR_TEX_FILTER_ANISOTROPIC_4X;      // the INDIRECT pass overrides it with its zr_params.tex_filter
    return v;
}
// ... and as the passes that bind the PREVIOUS acceleration structure and mesh-instance buffer see it (RT_SCENE_BVH_PREV /
// RT_FRAME_MESH_INSTANCES_PREV: CtT replay / reconnect of ReSTIR PT, the temporal shifts of the DI passes); == FrameView while nothing moved
static SceneView FrameViewPrev(const zr_scene* sc, const zr_frame_constants* cb)
{
    SceneView v = FrameView(sc, cb);
    std::lock_guard<std::mutex> lock(sc->mtx);
    if (sc->hasPrev) SceneBind(v, sc->prev);
    return v;
}

struct zr_gbuffer
{
    int device = 0; uint32_t w = 0, h = 0, x0 = 0, y0 = 0;
    // double-buffered like the reference's GBufferData (DefaultRendererImpl.h:80-130): every GBUFFER pass render flips
    // `cur`; the other set is the previous frame's G-buffer that the temporal passes of ReSTIR read
    // (a third set once the G-buffer is stream-tracked, zr_pass_set_frame_overlap: the GBUFFER render of frame N + 2 then runs while the temporal passes of
    // frame N + 1 still read the sets of frames N + 1 and N)
    DevBuf<uint8_t> planeSets[3][ZR_GB_COUNT];
    int cur = 0, numSets = 2; uint64_t numRendered = 0;
    // which object this is and which render filled each plane set (numRendered at the time; 0 = never): what a ReSTIR PT pass checks before a K12 sort it
    // put off reads these planes after the frame that rendered them (RptPendingSort).  uid: zr_gbuffer_create; g_liveGBuffers knows the ones that still exist
    uint64_t uid = 0, renderAt[3] = {0, 0, 0};
    int Next() const { return (cur + 1) % numSets; }
    int Prev() const { return (cur + numSets - 1) % numSets; }
    // the scene's material class (zr_scene::plainMaterials) at the time each plane set was rendered: the PLAIN kernel permutations take a pixel's flags as known,
    // so both the current and the previous frame's planes must come from a plain material table (a scene that BECAME plain renders one more frame with the general kernels)
    bool plainAt[3] = {true, true, true};
    // ... and WHICH scene rendered it (zr_scene::uid; 0 = never rendered by a GBUFFER pass): planes an engine filled itself through zr_gbuffer_device_plane, or
    // rendered from another scene than the lighting pass is given, carry flags the lighting pass cannot vouch for -- they run the general kernels
    uint64_t sceneAt[3] = {0, 0, 0};
    // stream tracking (zr_pass_set_frame_overlap): with the passes of a frame spread over two streams, a GBUFFER render must not overwrite a plane set
    // that a pass on another stream still reads, and a pass on another stream must not read a set before its GBUFFER render has finished: one tracker per plane set, acting only while `tracked`
    bool tracked = false;
    HipOrderPoints points; HipStreamOrder order[3];
    int AcquireRead(hipStream_t s) { return tracked ? order[cur].AcquireRead(points, s) : ZR_OK; }      // a pass on `s` is about to read the current planes
    int MarkRead(int set, hipStream_t s) { return tracked ? order[set].MarkRead(points, s) : ZR_OK; }    // `s` has finished reading plane set `set` at this point of its queue
    int AcquireWrite(int set, hipStream_t s) { return tracked ? order[set].AcquireWrite(points, s) : ZR_OK; }      // the GBUFFER pass on `s` is about to overwrite plane set `set`
    int MarkWritten(hipStream_t s) { return tracked ? order[cur].MarkWritten(points, s) : ZR_OK; }       // ... and has rendered the current one
    DevBuf<uint8_t>* Planes() { return planeSets[cur]; }
    const DevBuf<uint8_t>* Planes() const { return planeSets[cur]; }
    GBuf View() const { return ViewOf(cur); }
    GBuf PrevView() const { return ViewOf(Prev()); }
    GBuf ViewOf(int which) const
    {
        const DevBuf<uint8_t>* planes = planeSets[which];
        GBuf g; g.w = w; g.h = h; g.x0 = x0; g.y0 = y0;
        g.baseColor = (uint32_t*)planes[ZR_GB_BASE_COLOR].p; g.normal = (uint32_t*)planes[ZR_GB_NORMAL].p;
        g.mr = (uint16_t*)planes[ZR_GB_METALLIC_ROUGHNESS].p; g.motion = (uint32_t*)planes[ZR_GB_MOTION_VECTOR].p;
        g.emissive = (uint32_t*)planes[ZR_GB_EMISSIVE_COLOR].p; g.ior = (uint8_t*)planes[ZR_GB_IOR].p;
        g.coat = (uint16_t*)planes[ZR_GB_COAT].p; g.depth = (float*)planes[ZR_GB_DEPTH].p;
        g.triA = (uint32_t*)planes[ZR_GB_TRI_DIFF_GEO_A].p; g.triB = (uint32_t*)planes[ZR_GB_TRI_DIFF_GEO_B].p;
        return g;
    }
};

// the G-buffers that exist, by address, with their uids (an address can be handed out again)
static std::mutex g_liveGBuffersMtx;
static std::unordered_map<const zr_gbuffer*, uint64_t> g_liveGBuffers;
static uint64_t g_gbufferUid = 0;

struct QueueStorage
{
    DevBuf<U4> s0; DevBuf<F4> f[8]; DevBuf<F4> rays[6]; DevBuf<uint32_t> lightID; DevBuf<U4> hitC, hitM; DevBuf<uint32_t> visS, rayList;
    DevBuf<F4> t[8];      // ray-differential state, allocated by the first render of a textured scene
    int AllocTex(size_t cap)
    {
        int r;
        for (auto& b : t) if (b.n != cap && (r = b.Alloc(cap))) return r;
        return ZR_OK;
    }
    int Alloc(size_t cap)
    {
        int r;
        if ((r = s0.Alloc(cap))) return r;
        for (auto& b : f) if ((r = b.Alloc(cap))) return r;
        for (auto& b : rays) if ((r = b.Alloc(cap))) return r;
        if ((r = lightID.Alloc(cap))) return r;
        if ((r = hitC.Alloc(cap))) return r;
        if ((r = hitM.Alloc(cap))) return r;
        if ((r = visS.Alloc(cap))) return r;
        if ((r = rayList.Alloc(3 * cap))) return r;
        return ZR_OK;
    }
    PathQueue View() const
    {
        PathQueue q;
        q.s0 = s0.p; q.s1 = f[0].p; q.s2 = f[1].p; q.s3 = f[2].p; q.s4 = f[3].p; q.s5 = f[4].p; q.s6 = f[5].p; q.s7 = f[6].p; q.s8 = f[7].p;
        q.rayC_o = rays[0].p; q.rayC_d = rays[1].p; q.rayM_o = rays[2].p; q.rayM_d = rays[3].p; q.rayS_o = rays[4].p; q.rayS_d = rays[5].p;
        q.sLightID = lightID.p; q.hitC = hitC.p; q.hitM = hitM.p; q.visS = visS.p; q.rayList = rayList.p;
        for (int k = 0; k < 8; k++) q.t[k] = t[k].p;
        return q;
    }
};

static constexpr uint32_t kRptListWords = 12;      // replay work-list counts + cursors of the ReSTIR PT pass (layout: where the buffer is allocated)
// the node count from which K11 runs as k_rpt_pathtrace_w4 (4 waves per SIMD + the top 32 nodes of the tree in LDS).  Rounds 3 - 5: 16384 (1 MB of nodes = "does not fit
// the caches"; smaller scenes tied).  Round 6, re-measured on the collapsed trees (profiles/r06w_ab_k11_node_cache_small_scenes.txt): the cached build wins at every size --
// Cornell PLAIN K11 0.699 -> 0.679 ms (its 13 nodes are all in LDS), general Cornell 0.817 -> 0.803, sun + sky 0.899 -> 0.874, a 20 k-triangle scene 5.69 -> 5.26 -- so every
// scene that has a tree takes it; the other instantiation stays selectable (zr_debug_set_large_scene_nodes) and covered by the parity tests.
static constexpr uint32_t kLargeSceneNodes = 1;
static std::atomic<uint32_t> g_largeSceneNodes{kLargeSceneNodes};
static std::atomic<bool> g_materialClassKernels{true};      // zr_debug_set_material_class_kernels: plain scenes run the PLAIN kernel permutations
// the PLAIN kernel permutations apply: the scene's material table is of the plain class (and has no texture heap)
static bool PlainClass(const zr_scene* sc, const zr_gbuffer* gb)
{
    if (!sc->plainMaterials.load(std::memory_order_relaxed) || !g_materialClassKernels.load(std::memory_order_relaxed)) return false;
    const int c = gb->cur;
    if (!(gb->plainAt[c] && gb->sceneAt[c] == sc->uid)) return false;
    // the other set is the previous frame's G-buffer; nothing reads it before the second GBUFFER render (havePrevGBuffer)
    if (gb->numRendered >= 2 && !(gb->plainAt[gb->Prev()] && gb->sceneAt[gb->Prev()] == sc->uid)) return false;
    return true;
}
static constexpr int kMaxRounds = 16;
static constexpr int kMaxTimers = 64;
// ray-counter slots (pairs of u64 on the device): 0 = wavefront path tracer, 1.. = ReSTIR PT kernels in launch order
static constexpr int kCounterSlots = 16;
static const char* const kCounterNames[kCounterSlots] = {"trace", "rpt_pathtrace", "rpt_replay_ctt", "rpt_replay_ttc", "rpt_reconnect_temporal",
    "rpt_replay_cts", "rpt_replay_stc", "rpt_reconnect_spatial", "rdi_temporal", "rdi_spatial", "rgi", "sdi_temporal", "sdi_spatial", "rgi_spatial", "", ""};

struct zr_pass
{
    int kind = 0, device = 0, integrator = 0;
    bool initialized = false;
    uint32_t w = 0, h = 0;
    zr_params params{};
    // INDIRECT
    QueueStorage q[2];
    DevBuf<uint32_t> skyLut;                       // ZR_PASS_SKY: R11G11B10F texels
    // ZR_PASS_SKY: the inscattering voxel grid (Sky::SetInscatteringEnablement, zr_pass_set_inscattering), numVoxelsX x numVoxelsY x 128 R11G11B10F texels
    bool inscatterOn = false; InscatterParams inscatter{}; DevBuf<uint32_t> inscatterGrid;
    const zr_pass* inscatterSky = nullptr;         // ZR_PASS_COMPOSITING: the SKY pass whose grid is composited (zr_pass_bind_inscattering), read at render time
    Plane<float, 4> finalRGBA; Plane<F4> firstBOP; DevBuf<uint32_t> counts; DevBuf<unsigned long long> counters;
    DevBuf<uint32_t> groupMax;      // kMaxRounds x (8x8 groups of the tile): RR reduction keys
    zr_counters hostCounters{0, 0};
    // GBUFFER: GBufferRT::PickPixel (GBufferRT.h:36-46).  pickXY = x | y << 16, 0xffffffff = no pick pending; pickBuf[0] = the last picked mesh index
    uint32_t pickXY = 0xffffffffu; DevBuf<uint32_t> pickBuf; bool pickWritten = false;
    // INDIRECT / ReSTIR PT: two reservoir sets, two r-buffers, target, spatial neighbour, sample set.  A set states its planes once: their layouts in
    // the declaration, their order in Each (the order of zr_output and of a halo block), their kernel-side names in View; PlanesAllocZero / PlanesHalo /
    // PlanesOutput below go through Each
    struct ResStorage
    {
        Plane<uint32_t> A; Plane<float, 2> B; Plane<U4> C, D; Plane<uint16_t> E; Plane<float, 2> F; Plane<uint32_t, 2> G;
        template<typename S, typename Fn> static int Each(S& s, Fn f)
        { int r; if ((r = f(s.A)) || (r = f(s.B)) || (r = f(s.C)) || (r = f(s.D)) || (r = f(s.E)) || (r = f(s.F)) || (r = f(s.G))) return r; return ZR_OK; }
        rpt::ResPlanes View() const { rpt::ResPlanes v; v.A = A.p; v.B = B.p; v.C = C.p; v.D = D.p; v.E = E.p; v.F = F.p; v.G = G.p; return v; }
    } res[3];      // [2]: allocated by zr_pass_set_frame_overlap (the set K11 of the next frame writes while this frame's reuse passes read the other two)
    struct RBufStorage
    {
        Plane<uint16_t, 4> A; Plane<U4> B, C; Plane<uint16_t> D;
        template<typename S, typename Fn> static int Each(S& s, Fn f) { int r; if ((r = f(s.A)) || (r = f(s.B)) || (r = f(s.C)) || (r = f(s.D))) return r; return ZR_OK; }
        rpt::RBuf View() const { rpt::RBuf v; v.A = A.p; v.B = B.p; v.C = C.p; v.D = D.p; return v; }
    } rb[2];
    Plane<F4> rptTarget, rptTargetAlt; Plane<uint8_t, 2> rptNeighbor; DevBuf<uint16_t> rptSampleSet;
    // Frame overlap (zr_pass_set_frame_overlap): the roles of the three reservoir sets, the two target planes and the three FINAL planes, the mode, and
    // the cross-stream order of every stage's accesses to them (zr_rpt_overlap.h).  Without overlap the roles still hold currIdx and frameOpen; whether the pass has a history is hist.valid.
    zr::RptOverlap<HipOrderBackend> ov;
    Plane<float, 4> finalAlt, finalAlt2;      // FINAL rotates over three planes: K11 of frame N + 2 (which clears the pixels without a surface) may run while frame N's is still being consumed
    hipStream_t overlapStream = nullptr;      // "stream A" for callers without streams of their own
    const Plane<F4>& TargetPlane(int i) const { return i ? rptTargetAlt : rptTarget; }
    const Plane<float, 4>& FinalPlane(int i) const { return i == 0 ? finalRGBA : (i == 1 ? finalAlt : finalAlt2); }
    Plane<uint16_t> rptMap[2];      // K12 thread maps: [0] CtN, [1] NtC
    // A K12 sort that no kernel reads -- Sort_TtC of the temporal stage, Sort_CtS of a spatial round: their maps are outputs only -- is not launched by its
    // stage but kept here, with everything its launch needs, for whoever asks for the map (RptRunPendingSort below says when it runs and why its inputs still
    // stand then).  [0]: Sort_CtS into the CtN map, [1]: Sort_TtC into the NtC map.  live: the map plane does not hold the sort's result yet.
    struct RptPendingSort
    {
        bool live = false; int variant = 0;
        rpt::RptFrame F; zr_frame_constants cb; uint32_t sortTilesX = 0, numTiles = 0;      // the launch arguments of the stage that put it off
        hipStream_t stream = nullptr;                 // that stage's stream: where a consumer of the stage's outputs runs
        int set = 0;                                  // the reservoir set whose plane A it reads (index into res[])
        zr_gbuffer* gb = nullptr; uint64_t gbUid = 0, gbRenderAt = 0; int gbSet = 0;      // the G-buffer plane set whose flags and motion vectors it reads
    } rptPending[2];
    DevBuf<uint32_t> trip; DevBuf<unsigned long long> tripStats;      // ZR_K11=trip diagnostic
    DevBuf<uint32_t> carry[2], carryCount;                             // K11 with per-bounce compaction: path-state planes (ping-pong), alive counts
    DevBuf<uint32_t> costMap; bool costOn = false, costRays = false;      // rays per 32 x 32-px cell (zr_pass_enable_cost_map)
    DevBuf<uint32_t> rptLists, rptListCounts;      // 4 replay work lists (pixel ids) + their device-side counts
    // DI_EMISSIVE: two reservoir sets (A RGBA32_UINT, B RG32F), target (shared with DI_SKY), sample set
    struct DiStorage
    {
        Plane<U4> A; Plane<float, 2> B;
        template<typename S, typename Fn> static int Each(S& s, Fn f) { int r; if ((r = f(s.A)) || (r = f(s.B))) return r; return ZR_OK; }
        rdi::DiPlanes View() const { rdi::DiPlanes v; v.A = A.p; v.B = B.p; return v; }
    } di[2];
    Plane<F4> diTarget; DevBuf<uint16_t> diSampleSet;
    // DI_SKY: two sets of sun + sky DI reservoirs (A R8_UINT, B RG16_UINT, C RG32F)
    struct SkyStorage
    {
        Plane<uint8_t> A; Plane<uint16_t, 2> B; Plane<float, 2> C;
        template<typename S, typename Fn> static int Each(S& s, Fn f) { int r; if ((r = f(s.A)) || (r = f(s.B)) || (r = f(s.C))) return r; return ZR_OK; }
        sdi::SkyPlanes View() const { sdi::SkyPlanes v; v.A = A.p; v.B = B.p; v.C = C.p; return v; }
    } sky[2];
    // INDIRECT / ReSTIR GI: two reservoir sets (A RGBA32F, B RGBA16F, C RGBA32F)
    struct GiStorage
    {
        Plane<F4> A; Plane<uint16_t, 4> B; Plane<F4> C;
        template<typename S, typename Fn> static int Each(S& s, Fn f) { int r; if ((r = f(s.A)) || (r = f(s.B)) || (r = f(s.C))) return r; return ZR_OK; }
        rgi::GiPlanes View() const { rgi::GiPlanes v; v.A = A.p; v.B = B.p; v.C = C.p; return v; }
    } gi[2];
    // which of a pass's two sets is which, and whether the pass has a history at all (zr_pass_frame.h: who flips when, who rewinds on a reset)
    zr::PassHistory hist;
    bool doTemporal = false, doSpatial = false;      // ReSTIR PT: decided by the frame's CANDIDATES stage, held for its later stages
    const F4* compIn[4] = {nullptr, nullptr, nullptr, nullptr};     // COMPOSITING inputs (emissive DI, indirect, sky DI); [3] = TAA signal
    Plane<F4> svgfHist, svgfAccum, svgfPing, svgfPong; Plane<float, 2> svgfMoments[2]; Plane<float> svgfGuideFw; Plane<svgf::GuideN> svgfGuide; int svgfMomIdx = 0; const F4* svgfOut = nullptr; F4* svgfCur = nullptr; uint32_t svgfStepsDone = 0;      // DENOISE
    Plane<uint16_t, 4> taaOut[2]; int taaIdx = 0;            // TAA: ping-pong RGBA16F outputs; taaIdx = the one written last
    // AUTO_EXPOSURE / DISPLAY
    const uint16_t* postIn16 = nullptr; const F4* postIn32 = nullptr; const float* exposureIn = nullptr;
    DevBuf<uint32_t> aeHist; DevBuf<float> aeExposure;
    DevBuf<uint32_t> tonemapLut; uint32_t tonemapLutDim = 0; Plane<F4> displayOut; Plane<uint32_t> displaySrgb;
    int displayOption = ZR_DISPLAY_DEFAULT; float roughnessTh = 1.0f;      // DISPLAY: zr_pass_set_display_option (Display.cpp:69-73)
    // INDIRECT: zr_pass_set_rpt_debug_view (IndirectLighting.cpp:1543-1550); rptViewFrame = the view of the frame being rendered (latched by its first stage)
    int rptView = ZR_RPT_VIEW_NONE, rptViewFrame = ZR_RPT_VIEW_NONE;
    // INDIRECT: zr_pass_set_rgi_spatial (zr_rgi_spatial.h).  rgiSpatialFrame = the setting of the frame being rendered (latched by its first stage);
    // rgiScratch = the plane k_rgi's own radiance goes to while the spatial stage writes FINAL (allocated by the first frame that needs it)
    rgi::SpatialParams rgiSpatial{0u, rgi::kSpatialDefaultRadius}, rgiSpatialFrame{0u, rgi::kSpatialDefaultRadius}; Plane<float, 4> rgiScratch;
    std::vector<uint32_t> picks; DevBuf<uint8_t> pickMask; DevBuf<int4> pickTris; DevBuf<uint32_t> pickCount;     // DISPLAY: zr_pass_set_picked_instances
    uint32_t pickMaskW = 0, pickMaskH = 0;
    uint32_t own[4] = {0, 0, 0, 0};                // owned rect (global pixels); w == 0 -> the whole G-buffer rect
    // PRELIGHTING
    DevBuf<float> power;
    // deferred alias-table rebuild (zr_scene_invalidate_alias_table_deferred): K2's powers are read back into pinned memory behind an event
    float* powerHost = nullptr; size_t powerHostCap = 0; hipEvent_t powerEv = nullptr; bool powerPending = false;
    // timing
    bool timing = false;
    struct Timer { const char* name; hipEvent_t a, b; bool used; };
    std::vector<Timer> timers;
    int numTimers = 0;
    std::vector<std::string> timerNames; std::vector<float> timerMs; std::vector<uint32_t> timerLaunches;
};

// ------------------------------------------------------------------------------------------------ timing helpers
static void TimerBegin(zr_pass* p, hipStream_t s, const char* name)
{
    if (!p->timing) return;
    if (p->numTimers >= (int)p->timers.size())
    {
        zr_pass::Timer t; t.name = name; t.used = false;
        if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) return;
        p->timers.push_back(t);
    }
    zr_pass::Timer& t = p->timers[p->numTimers];
    t.name = name; t.used = true;
    (void)hipEventRecord(t.a, s);
}
static void TimerEnd(zr_pass* p, hipStream_t s)
{
    if (!p->timing) return;
    if (p->numTimers >= (int)p->timers.size()) return;
    (void)hipEventRecord(p->timers[p->numTimers].b, s);
    p->numTimers++;
}

// ------------------------------------------------------------------------------------------------ alias table (host)
// Math::KahanSum (Source/ZetaCore/Math/Common.cpp:72-139) with the reference's AVX2 lane structure.  `phase` floats of
// scalar head emulate a pointer that is `phase` floats short of 32-byte alignment (0 for the reference's allocations).
static float KahanSumAVX2(const float* data, int64_t N, int64_t phase)
{
    float sum = 0.0f, compensation = 0.0f;
    const int64_t start = phase < N ? phase : N;
    for (int64_t i = 0; i < start; i++)
    {
        volatile float corrected = data[i] - compensation;
        volatile float newSum = sum + corrected;
        compensation = (newSum - sum) - corrected;
        sum = newSum;
    }
    int64_t numSimd = (N - start);
    numSimd -= numSimd & 15;
    __m256 vSum = _mm256_setzero_ps(), vComp = _mm256_setzero_ps();
    for (int64_t c = start; c < start + numSimd; c += 16)
    {
        __m256 V1 = _mm256_loadu_ps(data + c), V2 = _mm256_loadu_ps(data + c + 8);
        __m256 vCurr = _mm256_add_ps(V1, V2);
        __m256 vCorrected = _mm256_sub_ps(vCurr, vComp);
        __m256 vNewSum = _mm256_add_ps(vSum, vCorrected);
        vComp = _mm256_sub_ps(vNewSum, vSum);
        vComp = _mm256_sub_ps(vComp, vCorrected);
        vSum = vNewSum;
    }
    alignas(32) float simdSum[8], simdComp[8];
    _mm256_store_ps(simdSum, vSum); _mm256_store_ps(simdComp, vComp);
    for (int i = 0; i < 8; i++)
    {
        volatile float corrected = simdSum[i] - compensation - simdComp[i];
        volatile float newSum = sum + corrected;
        compensation = (newSum - sum) - corrected;
        sum = newSum;
    }
    for (int64_t i = start + numSimd; i < N; i++)
    {
        volatile float corrected = data[i] - compensation;
        volatile float newSum = sum + corrected;
        compensation = (newSum - sum) - corrected;
        sum = newSum;
    }
    return sum;
}

// BuildAliasTable (Source/ZetaRenderPass/PreLighting/PreLighting.cpp:27-158): Vose's method with LIFO index stacks.
static void BuildAliasTableHost(std::vector<float>& probs, zr_alias_entry* table, uint32_t phase)
{
    const int64_t N = (int64_t)probs.size();
    const float oneDivN = 1.0f / (float)N;
    const float sum = KahanSumAVX2(probs.data(), N, phase);
    const float sumRcp = (float)N / sum;
    for (int64_t i = 0; i < N; i++) probs[i] *= sumRcp;
    for (int64_t i = 0; i < N; i++) { table[i].cached_p_orig = probs[i] * oneDivN; table[i].alias = 0xffffffffu; table[i].p_curr = 0.0f; }
    std::vector<uint32_t> larger, smaller;
    larger.reserve(N); smaller.reserve(N);
    for (int64_t i = 0; i < N; i++) (probs[i] < 1.0f ? smaller : larger).push_back((uint32_t)i);
    while (!smaller.empty() && !larger.empty())
    {
        const uint32_t si = smaller.back(); smaller.pop_back();
        const float sp = probs[si];
        const uint32_t li = larger.back();
        float lp = probs[li];
        table[si].alias = li; table[si].p_curr = sp;
        lp = (sp + lp) - 1.0f;
        probs[li] = lp;
        if (lp < 1.0f) { larger.pop_back(); smaller.push_back(li); }
    }
    for (; !larger.empty(); larger.pop_back()) { table[larger.back()].alias = larger.back(); table[larger.back()].p_curr = 1.0f; }
    for (; !smaller.empty(); smaller.pop_back()) { table[smaller.back()].alias = smaller.back(); table[smaller.back()].p_curr = 1.0f; }
    for (int64_t i = 0; i < N; i++) table[i].cached_p_alias = table[table[i].alias].cached_p_orig;
}

// ------------------------------------------------------------------------------------------------ C-ABI
// ---- device-side BVH refit (zr_scene_update_instances): the topology of the BVH4 stays, triangles are re-transformed and node boxes are
// recomputed bottom-up, one launch per tree level (deepest first; levels are a few dozen at most and the nodes of a level are independent).
// World-space triangles: the builder's expression (zr_bvh.h Build), so a refit scene traces the same triangles a rebuilt one would.
__global__ void __launch_bounds__(256) k_refit_tris(BvhTri* tris, uint32_t n, const TriMeta* meta, const zr_mesh_instance* instances, const float* toWorld,
    const zr_vertex* vertices, const uint32_t* indices)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    BvhTri t = tris[i];
    const TriMeta tm = meta[t.gidx];
    const zr_mesh_instance mi = instances[tm.mesh];
    const float* M = toWorld + 12 * (size_t)tm.mesh;
    float w[3][3];
    for (int k = 0; k < 3; k++)
    {
        const uint32_t vi = indices[mi.base_idx_offset + 3 * tm.prim + k] + mi.base_vtx_offset;
        const float* P = vertices[vi].pos;
        for (int r = 0; r < 3; r++) w[k][r] = M[4 * r + 0] * P[0] + M[4 * r + 1] * P[1] + M[4 * r + 2] * P[2] + M[4 * r + 3];
    }
    for (int r = 0; r < 3; r++) { t.v0[r] = w[0][r]; t.e1[r] = w[1][r] - w[0][r]; t.e2[r] = w[2][r] - w[0][r]; }
    tris[i] = t;
}
// A tree built in the background arrives as topology only (zr_scene::Background): child references per node, scene triangle per leaf slot.  The
// slot's constant words are the builder's (zr_bvh.h Build: mask of the instance, hashed triangle ID); vertices follow in k_refit_tris, boxes in k_refit_level.
__global__ void __launch_bounds__(256) k_install_topology(Bvh4Node* nodes, const uint32_t* children, uint32_t numNodes, BvhTri* tris, const uint32_t* slotTri, uint32_t numTris,
    const TriMeta* meta, const uint8_t* instanceMask)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < numNodes)
    {
        const uint4 c = ((const uint4*)children)[i];
        Bvh4Node N; N.ox = N.oy = N.oz = 0.0f; N.exps = 0; N.child[0] = c.x; N.child[1] = c.y; N.child[2] = c.z; N.child[3] = c.w;
        N.qlox = N.qloy = N.qloz = N.qhix = N.qhiy = N.qhiz = 0; N.pad0 = 0; N.pad1 = 0;
        nodes[i] = N;
    }
    if (i < numTris)
    {
        const uint32_t g = slotTri[i];
        const TriMeta tm = meta[g];
        BvhTri t; for (int r = 0; r < 3; r++) { t.v0[r] = 0.0f; t.e1[r] = 0.0f; t.e2[r] = 0.0f; }
        t.gidx = g; t.mask = instanceMask[tm.mesh]; t.id = TriID(tm.mesh, tm.prim);
        tris[i] = t;
    }
}
// bounds of leaf `c`: the union of its triangles' padded boxes (zr_intersect.h zr_tri_bounds, like the builder's)
__device__ __forceinline__ void LeafBounds(const BvhTri* tris, uint32_t c, float lo[3], float hi[3])
{
    const uint32_t first = (c & 0x7fffffffu) >> 3, count = (c & 7u) + 1u;
    for (int r = 0; r < 3; r++) { lo[r] = 3.402823466e+38f; hi[r] = -3.402823466e+38f; }
    for (uint32_t i = first; i < first + count; i++)
    {
        const BvhTri t = tris[i];
        float tlo[3], thi[3];
        zr_tri_bounds(t.v0, t.e1, t.e2, tlo, thi);
        for (int r = 0; r < 3; r++) { lo[r] = fminf(lo[r], tlo[r]); hi[r] = fmaxf(hi[r], thi[r]); }
    }
}
// one level: node = levelNodes[i]; its inner children were finished by the previous (deeper) launch.  Quantisation = BvhBuilder::Collapse:
// origin = the node's min corner, per-axis power-of-two scale whose 255 steps reach the max corner, child planes rounded outwards and verified
// against the traversal's decode expression fma(q, scale, origin).
__global__ void __launch_bounds__(64) k_refit_level(Bvh4Node* nodes, const uint32_t* levelNodes, uint32_t n, const BvhTri* tris, float* nodeBounds)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t ni = levelNodes[i];
    Bvh4Node N = nodes[ni];
    float clo[4][3], chi[4][3];
    for (int c = 0; c < 4; c++)
    {
        const uint32_t ref = N.child[c];
        if (ref == kEmptyChild) continue;
        if (ref & kLeafBit) LeafBounds(tris, ref, clo[c], chi[c]);
        else for (int r = 0; r < 3; r++) { clo[c][r] = nodeBounds[6 * (size_t)ref + r]; chi[c][r] = nodeBounds[6 * (size_t)ref + 3 + r]; }
    }
    float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
    for (int c = 0; c < 4; c++) if (N.child[c] != kEmptyChild) for (int r = 0; r < 3; r++) { lo[r] = fminf(lo[r], clo[c][r]); hi[r] = fmaxf(hi[r], chi[c][r]); }
    uint32_t ex[3], qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0};
    for (int r = 0; r < 3; r++)
    {
        int e = 1;
        const float ext = hi[r] - lo[r];
        if (ext > 0) { int ee; (void)frexpf(ext / 255.0f, &ee); e = max(1, min(254, ee + 126 - 1)); }
        while (e < 254 && !(fmaf(255.0f, zr_asfloat((uint32_t)e << 23), lo[r]) >= hi[r])) e++;
        ex[r] = (uint32_t)e;
        const float sc = zr_asfloat(ex[r] << 23);
        for (int c = 0; c < 4; c++)
        {
            if (N.child[c] == kEmptyChild) continue;
            int a = (int)floorf((clo[c][r] - lo[r]) / sc); a = max(0, min(255, a));
            while (a > 0 && fmaf((float)a, sc, lo[r]) > clo[c][r]) a--;
            int b = (int)ceilf((chi[c][r] - lo[r]) / sc); b = max(0, min(255, b));
            while (b < 255 && fmaf((float)b, sc, lo[r]) < chi[c][r]) b++;
            qlo[r] |= (uint32_t)a << (8 * c); qhi[r] |= (uint32_t)b << (8 * c);
        }
    }
    N.ox = lo[0]; N.oy = lo[1]; N.oz = lo[2]; N.exps = ex[0] | (ex[1] << 8) | (ex[2] << 16);
    N.qlox = qlo[0]; N.qloy = qlo[1]; N.qloz = qlo[2]; N.qhix = qhi[0]; N.qhiy = qhi[1]; N.qhiz = qhi[2];
    nodes[ni] = N;
    // what the parent sees: the box the quantised planes of the LARGEST child extent decode to would be looser; the exact union is enough,
    // because the parent quantises it outwards again
    for (int r = 0; r < 3; r++) { nodeBounds[6 * (size_t)ni + r] = lo[r]; nodeBounds[6 * (size_t)ni + 3 + r] = hi[r]; }
}

// ---- fused halo transfer: every plane x every rect in ONE launch (the per-plane hipMemcpy2DAsync path above costs planes x peers copies:
// 49 per exchange for ReSTIR PT on a 4 x 2 tile grid, each a few microseconds of launch latency for strips of a few hundred KB)
struct HaloJob
{
    struct Plane { char* base; uint32_t bpp; } planes[8];
    struct Rect { uint32_t first, w, h; uint32_t pad; uint64_t offset; } rects[ZR_HALO_MAX_RECTS];      // first = index of the rect's top-left pixel in the planes
    uint32_t numPlanes, numRects, pitch;      // pitch = plane width in pixels
    char* buf;
};
template<bool PACK> __global__ void __launch_bounds__(256) k_halo(HaloJob J)
{
    const HaloJob::Rect r = J.rects[blockIdx.y];
    const uint32_t n = r.w * r.h;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const size_t px = (size_t)r.first + (size_t)(i / r.w) * J.pitch + (i % r.w);
        char* cursor = J.buf + r.offset;
        for (uint32_t k = 0; k < J.numPlanes; k++)
        {
            const uint32_t bpp = J.planes[k].bpp;
            char* a = J.planes[k].base + px * bpp;      // in the plane
            char* b = cursor + (size_t)i * bpp;         // in the packed block (planes back to back, rows of the rect contiguous)
            char* dst = PACK ? b : a; const char* src = PACK ? a : b;
            switch (bpp)
            {
            case 16: *(uint4*)dst = *(const uint4*)src; break;
            case 8: *(uint2*)dst = *(const uint2*)src; break;
            case 4: *(uint32_t*)dst = *(const uint32_t*)src; break;
            case 2: *(uint16_t*)dst = *(const uint16_t*)src; break;
            default: *dst = *src; break;
            }
            cursor += (size_t)n * bpp;
        }
    }
}

extern "C" {

int zr_abi_version(void) { return ZR_ABI_VERSION; }
const char* zr_last_error(void) { return g_err.c_str(); }

int zr_device_count(int* count)
{
    if (!count) return Fail(ZR_ERR_INVALID_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = (e == hipSuccess) ? n : 0;
    return ZR_OK;
}

int zr_device_probe_run(int device, float min_ms, zr_device_probe* out)
{
    if (!out) return Fail(ZR_ERR_INVALID_ARG, "out is null");
    if (int r = RequireDevice(device)) return r;
    std::string err;
    if (zr::DeviceProbeRun(device, min_ms, out, err)) return Fail(ZR_ERR_HIP, "zr_device_probe_run: %s", err.c_str());
    return ZR_OK;
}

int zr_selftest_half_conversions(int device, uint64_t* m0, uint64_t* m1)
{
    if (!m0 || !m1) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    int r = RequireDevice(device);
    if (r) return r;
    DevBuf<unsigned long long> bad;
    if ((r = bad.Alloc(2))) return r;
    HIP_TRY(hipMemset(bad.p, 0, 2 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_selftest_half, dim3(256 * 64), dim3(256), 0, 0, bad.p);
    HIP_TRY(hipGetLastError());
    unsigned long long h[2];
    HIP_TRY(hipMemcpy(h, bad.p, sizeof(h), hipMemcpyDeviceToHost));
    *m0 = h[0]; *m1 = h[1];
    return ZR_OK;
}

int zr_params_default(zr_params* p)
{
    if (!p) return Fail(ZR_ERR_INVALID_ARG, "params is null");
    memset(p, 0, sizeof(*p));
    p->flags = ZR_IND_TEMPORAL_RESAMPLE | ZR_IND_SPATIAL_RESAMPLE | ZR_IND_RUSSIAN_ROULETTE | ZR_IND_BOILING_SUPPRESSION |
               ZR_IND_SORT_TEMPORAL | ZR_IND_SORT_SPATIAL;
    p->max_non_tr_bounces = 3; p->max_glossy_tr_bounces = 4; p->m_max_temporal = 10; p->m_max_spatial = 8;
    p->alpha_min = 0.175f * 0.175f; p->presampling = 0; p->num_sample_sets = 128; p->sample_set_size = 512;
    // light voxel grid: off; VOXEL_GRID_DIM (32, 8, 40), VOXEL_EXTENTS (0.6, 0.45, 0.6), y offset 0.1 (DefaultRendererImpl.h:42-43, 73-77)
    p->taa_blend_weight = 0.1f;      // TAA.h:72
    p->ae_min_lum = 5e-3f; p->ae_max_lum = 4.0f; p->ae_lum_map_exp = 0.5f; p->ae_adaptation_rate = 1.0f;      // AutoExposure.h:73-81
    p->tex_filter = ZR_TEX_FILTER_ANISOTROPIC_4X;      // IndirectLighting.h:243
    p->svgf_alpha = 0.2f; p->svgf_alpha_moments = 0.2f; p->svgf_sigma_l = 4.0f; p->svgf_sigma_z = 1.0f; p->svgf_normal_power_log2 = 7; p->svgf_iterations = 5;   // ZR_PASS_DENOISE (zr_svgf.h)
    p->num_spatial_passes = 1;        // IndirectLighting.h:392
    p->display_tonemapper = ZR_TONEMAP_NEUTRAL; p->display_auto_exposure = 1; p->display_saturation = 1.0f; p->display_agx_exp = 1.0f;   // Display.cpp:69-74
    p->use_lvg = 0; p->lvg_grid_dim = 32u | (8u << 10) | (40u << 20);
    p->lvg_extents[0] = 0.6f; p->lvg_extents[1] = 0.45f; p->lvg_extents[2] = 0.6f; p->lvg_offset_y = 0.1f;
    return ZR_OK;
}

int zr_alias_table_build(const float* power, uint32_t n, uint32_t align_phase, zr_alias_entry* out)
{
    if (!power || !out || n == 0) return Fail(ZR_ERR_INVALID_ARG, "zr_alias_table_build: null/empty input");
    std::vector<float> probs(power, power + n);
    BuildAliasTableHost(probs, out, align_phase);
    return ZR_OK;
}

// Tree levels of a BVH4 (root = node 0), deepest first: what the refit walks bottom-up
static void BvhLevels(const std::vector<Bvh4Node>& nodes, std::vector<uint32_t>& order, std::vector<uint32_t>& offsets)
{
    order.clear(); offsets.clear();
    if (nodes.empty()) return;
    std::vector<std::vector<uint32_t>> levels(1, std::vector<uint32_t>(1, 0u));
    for (size_t l = 0; l < levels.size(); l++)
    {
        std::vector<uint32_t> next;
        for (uint32_t ni : levels[l]) for (int c = 0; c < 4; c++) { const uint32_t r = nodes[ni].child[c]; if (r != kEmptyChild && !(r & kLeafBit)) next.push_back(r); }
        if (!next.empty()) levels.push_back(std::move(next));
    }
    for (size_t l = levels.size(); l-- > 0;) { offsets.push_back((uint32_t)order.size()); order.insert(order.end(), levels[l].begin(), levels[l].end()); }
    offsets.push_back((uint32_t)order.size());
}

// node boxes of the current set bottom-up: one k_refit_level launch per tree level (levelNodes / levelOffsets), deepest first
static void LaunchRefitLevels(zr_scene* s, hipStream_t st)
{
    for (size_t l = 0; l + 1 < s->levelOffsets.size(); l++)
    {
        const uint32_t first = s->levelOffsets[l], cnt = s->levelOffsets[l + 1] - first;
        hipLaunchKernelGGL(k_refit_level, dim3((cnt + 63) / 64), dim3(64), 0, st, s->cur.nodes.p, s->levelNodes.p + first, cnt, s->cur.tris.p, s->nodeBounds.p);
    }
}
// Builds the CURRENT acceleration structure on the device from the current set's instance buffer + the object-to-world matrices (both already
// on the device, or enqueued on `st`): LBVH topology (zr_tu_bvh.hip), then the level-by-level box computation + quantisation of the refit.
// Host-synchronous (the level structure comes back).  The node / triangle buffers are grown to the build's capacity on first use.  States the
// tree's counts in the set; binding the set to `view` is the caller's, once everything else of the update has succeeded too.
static int DeviceRebuild(zr_scene* s, hipStream_t st)
{
    AccelSet& a = s->cur;
    const uint32_t nt = (uint32_t)a.meta.n;
    int r;
    if (a.nodes.n < nt || a.tris.n < nt || s->nodeBounds.n < 6 * (size_t)nt)
    {
        HIP_TRY(hipDeviceSynchronize());
        if (a.nodes.n < nt && (r = a.nodes.Alloc(nt))) return r;
        if (a.tris.n < nt && (r = a.tris.Alloc(nt))) return r;
        if (s->nodeBounds.n < 6 * (size_t)nt && (r = s->nodeBounds.Alloc(6 * (size_t)nt))) return r;
    }
    if (!s->dMask.p && (r = s->dMask.Upload(s->hMask.data(), s->hMask.size()))) return r;
    DeviceBvhInputs in; in.numTris = nt; in.meta = a.meta.p; in.instances = a.instances.p; in.toWorld = s->toWorld.p; in.vertices = s->vertices.p;
    in.indices = s->indices.p; in.instanceMask = s->dMask.p;
    DeviceBvhOutputs out; out.tris = a.tris.p; out.nodes = a.nodes.p; out.nodeCap = (uint32_t)a.nodes.n;
    std::string err;
    if (DeviceBuildBvh4(st, s->bvhScratch, in, out, err)) return Fail(ZR_ERR_HIP, "device BVH build: %s", err.c_str());
    if (out.stackNeed + 1 > (uint32_t)kTravStack) return Fail(ZR_ERR_UNSUPPORTED, "device-built BVH has %u levels: needs %u traversal stack entries (limit %d); use the host builder", out.numLevels, out.stackNeed, kTravStack - 1);
    s->hLevelOrder = out.levelOrder; s->levelOffsets = out.levelOffsets;
    if (s->levelNodes.n < s->hLevelOrder.size()) { HIP_TRY(hipStreamSynchronize(st)); if ((r = s->levelNodes.Alloc(nt))) return r; }
    HIP_TRY(hipMemcpyAsync(s->levelNodes.p, s->hLevelOrder.data(), s->hLevelOrder.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    LaunchRefitLevels(s, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));          // hLevelOrder is pageable: its copy must have been staged and the kernels' errors seen
    a.numNodes = out.numNodes; a.numTris = nt;
    if (out.numLevels > s->maxDepth) s->maxDepth = out.numLevels;
    s->deviceBuilt = true;
    return ZR_OK;
}

// The current instance array has just been written on `st` (an upload, LaunchMoveInstances): its table of decoded records follows on the same stream
static int SceneFillInstRecs(zr_scene* s, hipStream_t st) { HIP_TRY(zr::LaunchFillInstRecs(st, s->cur.instRecs.p, s->cur.instances.p, (uint32_t)s->cur.instances.n)); return ZR_OK; }

// SceneView::plain: no material of the table is metallic, transmissive, thin-walled or coated (the fields GetMaterialData turns into those lobes, Material.h:268-427)
static bool MaterialsArePlain(const std::vector<zr_material>& m)
{
    const uint32_t lobes = (1u << ZR_MAT_METALLIC_BIT) | (1u << ZR_MAT_TRANSMISSIVE_BIT) | (1u << ZR_MAT_THIN_WALLED_BIT);
    for (const zr_material& x : m) if ((x.coat_color_flags & lobes) || ((x.base_color_tex_subsurf_coat_weight >> 24) & 0xffu)) return false;
    return !m.empty();
}
// Texture indices of created / updated records raise the per-table maxima that the descriptor-table bounds check of zr_pass_render relies on
static void RaiseMaxTex(zr_scene* s, int table, uint32_t tex) { if (tex != ZR_INVALID_TEX && (int64_t)tex > s->maxTex[table]) s->maxTex[table] = tex; }
// How zr_scene_update_instances makes the frame's tree (ZR_SCENE_UPDATE): the refit on the device (unset, "refit", "refit_sah"), a new LBVH on the device
// ("rebuild"), the host's binned-SAH builder ("rebuild_host").  The two rebuilds are host-synchronous, and the device forms of the update refuse them.
// "refit_sah" is the refit with the background rebuild on for every scene of the process; for one scene that is a flag (zr_scene_set_background_rebuild)
enum class UpdateMode { Refit, RebuildDevice, RebuildHost };
static UpdateMode SceneUpdateMode()
{
    const char* e = std::getenv("ZR_SCENE_UPDATE");
    return !e ? UpdateMode::Refit : !std::strcmp(e, "rebuild") ? UpdateMode::RebuildDevice : !std::strcmp(e, "rebuild_host") ? UpdateMode::RebuildHost : UpdateMode::Refit;
}
static bool BackgroundRebuildByDefault() { const char* e = std::getenv("ZR_SCENE_UPDATE"); return e && !std::strcmp(e, "refit_sah"); }
static int RefuseRebuildMode(const char* fn)
{
    const UpdateMode m = SceneUpdateMode();
    return m == UpdateMode::Refit ? ZR_OK : Fail(ZR_ERR_UNSUPPORTED, "%s: ZR_SCENE_UPDATE=%s is a host-synchronous path; the device form of the update needs the refit (default or refit_sah)",
        fn, m == UpdateMode::RebuildDevice ? "rebuild" : "rebuild_host");
}
// what the host's builder takes: the scene's host copies of the static arrays + the given instance records and matrices
static zr_scene_desc SceneBuilderDesc(const zr_scene* s, const zr_mesh_instance* instances, uint32_t n, const float* toWorld)
{
    zr_scene_desc d; memset(&d, 0, sizeof(d));
    d.vertices = s->hVertices.data(); d.num_vertices = (uint32_t)s->hVertices.size(); d.indices = s->hIndices.data(); d.num_indices = (uint32_t)s->hIndices.size();
    d.instances = instances; d.num_instances = n; d.instance_to_world = toWorld; d.instance_mask = s->hMask.data(); d.instance_num_tris = s->hNumTris.data();
    return d;
}
// zr::BuildTexturePlan (zr_tex_plan.h: everything a caller refuses about descs, sources and records, before anything is allocated), its refusal as this library's
static int PlanTextures(const char* fn, const zr_texture_desc* descs, const zr_texture_source* sources, uint32_t n, uint64_t payloadBytes, uint64_t texelBytes, const uint8_t* hostPayload,
    uint32_t accept, uint32_t stages, zr::TexturePlan& plan)
{
    std::string err;
    const int r = zr::BuildTexturePlan(descs, sources, n, payloadBytes, texelBytes, hostPayload, accept, stages, plan, err);
    return r ? Fail(r, "%s: %s", fn, err.c_str()) : ZR_OK;
}
// Enqueues on `st` whatever the plan holds, in this order: the block decode, the raw copies, the JPEG blocks and then their texels, the
// mip levels top down.  The job tables and the JPEG sample planes share one stream-ordered allocation, freed behind whatever was enqueued, on the error
// path too: nothing here waits for the stream's earlier work.  The tables are copied from the plan's pageable vectors, which the caller destroys on
// return: hipMemcpyAsync from pageable memory is synchronous towards the host buffer (the runtime has staged or sent it when it returns), so the
// vectors may go; it is no wait for earlier work of the stream
static int RunTexturePlan(const char* fn, hipStream_t st, const zr::TexturePlan& plan, const uint8_t* dPayload, uint8_t* dTexels)
{
    enum { kBlock, kJpegBlock, kJpegTex, kMip, kPlanes, kParts };
    const void* src[kParts] = {plan.blockJobs.data(), plan.jpegBlockJobs.data(), plan.jpegTexJobs.data(), plan.mipJobs.data(), nullptr};
    const size_t bytes[kParts] = {plan.blockJobs.size() * sizeof(zrbc::Job), plan.jpegBlockJobs.size() * sizeof(zrjp::BlockJob), plan.jpegTexJobs.size() * sizeof(zrjp::TexJob),
                                  plan.mipJobs.size() * sizeof(zrmg::Job), (size_t)plan.planeBytes};
    size_t at[kParts], total = 0;
    for (int k = 0; k < kParts; k++) { at[k] = total; total += (bytes[k] + 255u) & ~(size_t)255u; }      // (each part as aligned as an allocation of its own)
    uint8_t* mem = nullptr;
    hipError_t e = total ? hipMallocAsync((void**)&mem, total, st) : hipSuccess;
    for (int k = 0; k < kPlanes && e == hipSuccess; k++) if (bytes[k]) e = hipMemcpyAsync(mem + at[k], src[k], bytes[k], hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !plan.blockJobs.empty()) e = zr::LaunchBcnDecode(st, (const zrbc::Job*)(mem + at[kBlock]), (uint32_t)plan.blockJobs.size(), plan.numBlocks, dPayload, dTexels);
    for (const zr::TexturePlan::Copy& c : plan.copies) if (e == hipSuccess && c.bytes) e = hipMemcpyAsync(dTexels + c.dst, dPayload + c.src, c.bytes, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && !plan.jpegTexJobs.empty())
        e = zr::LaunchJpegDecode(st, (const zrjp::BlockJob*)(mem + at[kJpegBlock]), (uint32_t)plan.jpegBlockJobs.size(), (uint32_t)plan.jpegBlocks, (const zrjp::TexJob*)(mem + at[kJpegTex]),
                                 (uint32_t)plan.jpegTexJobs.size(), (uint32_t)plan.jpegItems, dPayload, mem + at[kPlanes], dTexels);
    for (const zr::TexturePlan::Level& lv : plan.levels)
        if (e == hipSuccess && lv.numItems) e = zr::LaunchMipLevel(st, (const zrmg::Job*)(mem + at[kMip]) + lv.firstJob, lv.numJobs, lv.numItems, dTexels);
    if (mem) { const hipError_t f = hipFreeAsync(mem, st); if (e == hipSuccess) e = f; }
    if (e != hipSuccess) return Fail(ZR_ERR_HIP, "%s: the texture decode could not be enqueued: %s", fn, hipGetErrorString(e));
    return ZR_OK;
}
// zero-fills what no chain of the plan covers in a heap of `bytes` bytes (the decode and the copies write every byte of a chain): the padding between
// chains, a few bytes each for a loader's heap, instead of the whole heap twice.  On the null stream
static int ClearHeapGaps(const zr::TexturePlan& plan, uint8_t* dTexels, uint64_t bytes)
{
    std::vector<std::pair<uint64_t, uint64_t>> c = plan.chains;
    std::sort(c.begin(), c.end());
    uint64_t at = 0;
    for (const auto& r : c)
    {
        if (r.first > at) HIP_TRY(hipMemset(dTexels + at, 0, r.first - at));
        if (r.second > at) at = r.second;
    }
    if (bytes > at) HIP_TRY(hipMemset(dTexels + at, 0, bytes - at));
    return ZR_OK;
}
// zr_scene_create (blocks == nullptr) and zr_scene_create_compressed: the same scene, the texel heap uploaded or decoded on the device
static int SceneCreate(const char* fn, int device, const zr_scene_desc* d, const zr_texture_blocks* blocks, zr_scene** out)
{
    if (!d || !out) return Fail(ZR_ERR_INVALID_ARG, "%s: null argument", fn);
    if (!d->vertices || !d->indices || !d->instances || !d->materials || !d->rho_lut || !d->instance_to_world || !d->instance_mask || !d->instance_num_tris)
        return Fail(ZR_ERR_INVALID_ARG, "%s: incomplete scene description", fn);
    zr::TexturePlan plan;
    if (blocks)
    {   // refused before the acceleration structure is built
        if (!blocks->sources || !blocks->payload) return Fail(ZR_ERR_INVALID_ARG, "%s: null sources / payload", fn);
        if (d->texels) return Fail(ZR_ERR_INVALID_ARG, "%s: desc->texels must be null: the heap is decoded from the blocks", fn);
        if (d->num_textures && !d->textures) return Fail(ZR_ERR_INVALID_ARG, "%s: num_textures > 0 without textures", fn);
        if (int pr = PlanTextures(fn, d->textures, blocks->sources, d->num_textures, blocks->payload_bytes, d->texel_bytes, blocks->payload, zr::kTexSrcAll, zr::kTexPlanAll, plan)) return pr;
    }
    DevBuf<uint8_t> payload;      // (live until the synchronize at the end)
    int r = RequireDevice(device);
    if (r) return r;
    std::unique_ptr<zr_scene> s(new (std::nothrow) zr_scene());      // (every early return below frees it)
    if (!s) return Fail(ZR_ERR_OOM, "out of host memory");
    s->device = device;
    // ZR_BVH_BUILD=device: the acceleration structure is built on the GPU (LBVH, zr_tu_bvh.hip) instead of by the host's binned-SAH builder
    uint64_t totalTris = 0;
    for (uint32_t i = 0; i < d->num_instances; i++) totalTris += d->instance_num_tris[i];
    const char* buildEnv = std::getenv("ZR_BVH_BUILD");
    const bool deviceBuild = buildEnv && !std::strcmp(buildEnv, "device") && totalTris > BvhBuilder::kTinyScene;
    BuiltBvh bvh;
    if (deviceBuild)
    {   // only the global-order (mesh, primitive) table is made on the host; geometry never passes through it
        bvh.meta.reserve((size_t)totalTris);
        for (uint32_t i = 0; i < d->num_instances; i++) for (uint32_t p = 0; p < d->instance_num_tris[i]; p++) { TriMeta m; m.mesh = i; m.prim = p; bvh.meta.push_back(m); }
    }
    else bvh = BvhBuilder().Build(*d);
    if (bvh.stackNeed + 1 > (uint32_t)kTravStack) return Fail(ZR_ERR_UNSUPPORTED, "BVH needs %u traversal stack entries (limit %d)", bvh.stackNeed, kTravStack - 1);
    s->maxDepth = bvh.maxDepth;
    AccelSet& a = s->cur;
    if ((r = s->vertices.Upload(d->vertices, d->num_vertices)) || (r = s->indices.Upload(d->indices, d->num_indices)) ||
        (r = a.instances.Upload(d->instances, d->num_instances)) || (r = s->materials.Upload(d->materials, d->num_materials)) ||
        (r = s->emissives.Upload(d->emissives, d->num_emissives)) || (r = a.nodes.Upload(bvh.nodes4.data(), bvh.nodes4.size())) ||
        (r = a.tris.Upload(bvh.tris.data(), bvh.tris.size())) || (r = a.meta.Upload(bvh.meta.data(), bvh.meta.size())) ||
        (r = s->rho.Upload(d->rho_lut, (size_t)d->rho_dim[0] * d->rho_dim[1] * d->rho_dim[2]))) return r;
    a.numNodes = (uint32_t)bvh.nodes4.size(); a.numTris = (uint32_t)bvh.tris.size();
    if (d->num_textures && blocks)
    {   // the blocks cross the bus once; the heap's padding is zero-filled, its chains decoded into, on the null stream like the uploads around it
        if ((r = s->texDescs.Upload(d->textures, d->num_textures)) || (r = payload.Upload(blocks->payload, blocks->payload_bytes)) ||
            (r = s->texels.Alloc(d->texel_bytes)) || (r = ClearHeapGaps(plan, s->texels.p, d->texel_bytes)) || (r = RunTexturePlan(fn, nullptr, plan, payload.p, s->texels.p))) return r;
    }
    else if (d->num_textures)
    {
        if (!d->textures || !d->texels) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_create: num_textures > 0 without textures / texels");
        for (uint32_t i = 0; i < d->num_textures; i++)
            if (!zr::TextureDescOk(d->textures[i], d->texel_bytes)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_create: texture %u is malformed or lies outside the texel blob", i);
        if ((r = s->texDescs.Upload(d->textures, d->num_textures)) || (r = s->texels.Upload(d->texels, d->texel_bytes))) return r;
    }
    if ((r = s->srgb.Upload(zr_srgb_to_linear_table, 256))) return r;
    // the decoded tables of zr_hit_tables.h, behind the uploads on the null stream (the synchronize below covers them)
    if ((r = a.instRecs.Alloc(d->num_instances)) || (r = s->vtxNormals.Alloc(d->num_vertices)) || (r = SceneFillInstRecs(s.get(), nullptr))) return r;
    { hipError_t e = zr::LaunchFillVtxNormals(nullptr, s->vtxNormals.p, s->vertices.p, d->num_vertices, false);
      if (e != hipSuccess) return Fail(ZR_ERR_HIP, "k_fill_vtx_normals failed: %s", hipGetErrorString(e)); }
    s->view.vtxNormals = s->vtxNormals.p;
#if ZR_HIT_TANGENTS
    if ((r = s->vtxTangents.Alloc(d->num_vertices))) return r;
    { hipError_t e = zr::LaunchFillVtxNormals(nullptr, s->vtxTangents.p, s->vertices.p, d->num_vertices, true);
      if (e != hipSuccess) return Fail(ZR_ERR_HIP, "k_fill_vtx_normals failed: %s", hipGetErrorString(e)); }
    s->view.vtxTangents = s->vtxTangents.p;
#endif
    SceneView& v = s->view;
    v.vertices = s->vertices.p; v.indices = s->indices.p; v.materials = s->materials.p;
    v.emissives = s->emissives.p; v.alias = nullptr; v.sampleSets = nullptr; v.sampleSetSize = 0;
    v.rho.data = s->rho.p; v.rho.dx = d->rho_dim[0]; v.rho.dy = d->rho_dim[1]; v.rho.dz = d->rho_dim[2];
    v.numEmissives = d->num_emissives;
    s->hMaterials.assign(d->materials, d->materials + d->num_materials);
    s->plainMaterials = MaterialsArePlain(s->hMaterials) && d->num_textures == 0;
    v.tex.descs = s->texDescs.p; v.tex.texels = s->texels.p; v.tex.srgb = s->srgb.p; v.tex.count = d->num_textures;
    // largest tex16 per descriptor table, so that zr_pass_render can reject frame constants whose table offsets would
    // send a texture fetch outside the heap
    for (uint32_t i = 0; i < d->num_materials; i++)
    {
        const zr_material& m = d->materials[i];
        const uint32_t t[4] = { m.base_color_tex_subsurf_coat_weight & 0xffffu, m.normal_tex_tr_depth & 0xffffu,
                                m.mr_tex_spec_roughness_coat_roughness & 0xffffu, m.emissive_tex_alpha_cutoff_coat_ior & 0xffffu };
        for (int k = 0; k < 4; k++) RaiseMaxTex(s.get(), k, t[k]);
    }
    for (uint32_t i = 0; i < d->num_instances; i++) RaiseMaxTex(s.get(), 0, d->instances[i].base_color_tex);
    for (uint32_t i = 0; i < d->num_emissives; i++) RaiseMaxTex(s.get(), 3, d->emissives[i].packed_b & 0xffffu);
    s->bg.enabled = BackgroundRebuildByDefault();
    s->hVertices.assign(d->vertices, d->vertices + d->num_vertices); s->hIndices.assign(d->indices, d->indices + d->num_indices);
    s->hMask.assign(d->instance_mask, d->instance_mask + d->num_instances); s->hNumTris.assign(d->instance_num_tris, d->instance_num_tris + d->num_instances);
    s->hToWorld.assign(d->instance_to_world, d->instance_to_world + 12 * (size_t)d->num_instances); s->movedEver.assign(d->num_instances, 0);
    s->hInstances.assign(d->instances, d->instances + d->num_instances);
    BvhLevels(bvh.nodes4, s->hLevelOrder, s->levelOffsets);
    if (!s->hLevelOrder.empty() && (r = s->levelNodes.Upload(s->hLevelOrder.data(), s->hLevelOrder.size()))) return r;
    if (deviceBuild)
    {
        if ((r = s->toWorld.Upload(d->instance_to_world, 12 * (size_t)d->num_instances)) || (r = DeviceRebuild(s.get(), nullptr))) return r;
        s->toWorldDev = true;
    }
    SceneBind(v, a);
    // uploads from pageable memory return once staged; renders on non-blocking streams must not start before the DMA has landed
    { hipError_t e = hipDeviceSynchronize(); if (e != hipSuccess) return Fail(ZR_ERR_HIP, "hipDeviceSynchronize failed: %s", hipGetErrorString(e)); }
    *out = s.release();
    return ZR_OK;
}
int zr_scene_create(int device, const zr_scene_desc* d, zr_scene** out) { return SceneCreate("zr_scene_create", device, d, nullptr, out); }
int zr_scene_create_compressed(int device, const zr_scene_desc* d, const zr_texture_blocks* blocks, zr_scene** out)
{
    if (!blocks) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_create_compressed: null blocks");
    return SceneCreate("zr_scene_create_compressed", device, d, blocks, out);
}
// the decode of zr_scene_create_compressed on caller buffers; enqueues only (RunTexturePlan)
int zr_bcn_decode_device(int device, void* stream, const zr_texture_desc* descs, const zr_texture_source* sources, uint32_t n, const void* d_payload, uint64_t payload_bytes,
    void* d_texels, uint64_t texel_bytes)
{
    const char* fn = "zr_bcn_decode_device";
    if (!descs || !sources || !d_payload || !d_texels || n == 0) return Fail(ZR_ERR_INVALID_ARG, "%s: null/empty input", fn);
    if (((uintptr_t)d_payload & 15u) || ((uintptr_t)d_texels & 3u)) return Fail(ZR_ERR_INVALID_ARG, "%s: d_payload must be 16-byte and d_texels 4-byte aligned", fn);
    zr::TexturePlan plan;
    if (int r = PlanTextures(fn, descs, sources, n, payload_bytes, texel_bytes, nullptr, zr::kTexSrcStored, zr::kTexPlanBlocks, plan)) return r;
    if (hipSetDevice(device) != hipSuccess) return Fail(ZR_ERR_NO_DEVICE, "%s: no usable HIP device %d", fn, device);
    return RunTexturePlan(fn, (hipStream_t)stream, plan, (const uint8_t*)d_payload, (uint8_t*)d_texels);
}
// level 0 of the JPEG_COEF sources of zr_scene_create_compressed on caller buffers.  The records are validated on the host like the scene path's, so the
// payload is read back first (a wait on the stream); the decode itself is enqueued only
int zr_jpeg_decode_device(int device, void* stream, const zr_texture_desc* descs, const zr_texture_source* sources, uint32_t n, const void* d_payload, uint64_t payload_bytes,
    void* d_texels, uint64_t texel_bytes)
{
    const char* fn = "zr_jpeg_decode_device";
    if (!descs || !sources || !d_payload || !d_texels || n == 0) return Fail(ZR_ERR_INVALID_ARG, "%s: null/empty input", fn);
    if (((uintptr_t)d_payload & 15u) || ((uintptr_t)d_texels & 3u)) return Fail(ZR_ERR_INVALID_ARG, "%s: d_payload must be 16-byte and d_texels 4-byte aligned", fn);
    bool any = false;
    for (uint32_t i = 0; i < n; i++) any = any || sources[i].encoding == ZR_TEX_SRC_JPEG_COEF;
    if (hipSetDevice(device) != hipSuccess) return Fail(ZR_ERR_NO_DEVICE, "%s: no usable HIP device %d", fn, device);
    hipStream_t st = (hipStream_t)stream;
    std::vector<uint8_t> host;
    if (any && payload_bytes)
    {
        host.resize(payload_bytes);
        HIP_TRY(hipMemcpyAsync(host.data(), d_payload, payload_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    zr::TexturePlan plan;
    if (int r = PlanTextures(fn, descs, sources, n, payload_bytes, texel_bytes, host.data(), zr::kTexSrcAll, zr::kTexPlanJpeg, plan)) return r;
    return RunTexturePlan(fn, st, plan, (const uint8_t*)d_payload, (uint8_t*)d_texels);
}
// the level launches of zr_scene_create_compressed on caller buffers; enqueues only, like zr_bcn_decode_device
int zr_mipgen_device(int device, void* stream, const zr_texture_desc* descs, uint32_t n, void* d_texels, uint64_t texel_bytes)
{
    const char* fn = "zr_mipgen_device";
    if (n == 0) return ZR_OK;
    if (!descs || !d_texels) return Fail(ZR_ERR_INVALID_ARG, "%s: null argument", fn);
    if ((uintptr_t)d_texels & 3u) return Fail(ZR_ERR_INVALID_ARG, "%s: d_texels must be 4-byte aligned", fn);
    zr::TexturePlan plan;
    if (int r = PlanTextures(fn, descs, nullptr, n, 0, texel_bytes, nullptr, 0u, zr::kTexPlanLevels, plan)) return r;
    if (plan.mipJobs.empty()) return ZR_OK;      // (chains of one level: nothing to enqueue, and the device is not looked at)
    if (hipSetDevice(device) != hipSuccess) return Fail(ZR_ERR_NO_DEVICE, "%s: no usable HIP device %d", fn, device);
    return RunTexturePlan(fn, (hipStream_t)stream, plan, nullptr, (uint8_t*)d_texels);
}
int zr_scene_get_texels(const zr_scene* s, void* stream, uint8_t* out, uint64_t first, uint64_t count)
{
    if (!s || (!out && count)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_texels: null argument");
    if (first > s->texels.n || count > s->texels.n - first) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_texels: [%llu, +%llu) exceeds the heap's %zu bytes", (unsigned long long)first, (unsigned long long)count, s->texels.n);
    if (!count) return ZR_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(out, s->texels.p + first, count, hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_scene_update_emissives_async(zr_scene* s, void* stream, const zr_emissive_triangle* triangles, uint32_t first, uint32_t count)
{
    if (!s || (!triangles && count)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_update_emissives: null argument");
    if ((uint64_t)first + count > s->emissives.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_update_emissives: [%u, %u) exceeds the scene's %zu emissive triangles", first, first + count, s->emissives.n);
    if (!count) return ZR_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    int r; zr_scene::StageSlot* t;
    if ((r = StageAcquire(s, (size_t)count * sizeof(zr_emissive_triangle), &t))) return r;
    memcpy(t->host, triangles, (size_t)count * sizeof(zr_emissive_triangle));
    for (uint32_t i = 0; i < count; i++) RaiseMaxTex(s, 3, triangles[i].packed_b & 0xffffu);
    if ((r = SceneWaitUsers(s, st))) return r;          // kernels of earlier frames on other streams may still sample the old records
    HIP_TRY(hipMemcpyAsync(s->emissives.p + first, t->host, (size_t)count * sizeof(zr_emissive_triangle), hipMemcpyHostToDevice, st));
    if ((r = StageCommit(t, st))) return r;
    return SceneMarkUpdated(s, st);
}
int zr_scene_update_materials_async(zr_scene* s, void* stream, const zr_material* materials, uint32_t first, uint32_t count)
{
    if (!s || (!materials && count)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_update_materials: null argument");
    if ((uint64_t)first + count > s->materials.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_update_materials: [%u, %u) exceeds the scene's %zu materials", first, first + count, s->materials.n);
    if (!count) return ZR_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    int r; zr_scene::StageSlot* t;
    if ((r = StageAcquire(s, (size_t)count * sizeof(zr_material), &t))) return r;
    memcpy(t->host, materials, (size_t)count * sizeof(zr_material));
    for (uint32_t i = 0; i < count; i++)
    {   // Material.h:268-427: base colour / normal / metallic-roughness / emissive texture ids (16 bits each)
        RaiseMaxTex(s, 0, materials[i].base_color_tex_subsurf_coat_weight & 0xffffu); RaiseMaxTex(s, 1, materials[i].normal_tex_tr_depth & 0xffffu);
        RaiseMaxTex(s, 2, materials[i].mr_tex_spec_roughness_coat_roughness & 0xffffu); RaiseMaxTex(s, 3, materials[i].emissive_tex_alpha_cutoff_coat_ior & 0xffffu);
    }
    if ((r = SceneWaitUsers(s, st))) return r;
    std::copy(materials, materials + count, s->hMaterials.begin() + first);
    s->plainMaterials = MaterialsArePlain(s->hMaterials) && s->view.tex.count == 0;
    HIP_TRY(hipMemcpyAsync(s->materials.p + first, t->host, (size_t)count * sizeof(zr_material), hipMemcpyHostToDevice, st));
    if ((r = StageCommit(t, st))) return r;
    return SceneMarkUpdated(s, st);
}
// the original host-synchronous entry points: the update on the null stream (r: what its _async form returned), then wait for it -- errors of the
// copies / refit kernels surface here.  (An empty range enqueues nothing and waits for nothing.)
static int ThenWait(int r) { if (r) return r; HIP_TRY(hipDeviceSynchronize()); return ZR_OK; }
int zr_scene_update_emissives(zr_scene* s, const zr_emissive_triangle* t, uint32_t first, uint32_t count) { const int r = zr_scene_update_emissives_async(s, nullptr, t, first, count); return count ? ThenWait(r) : r; }
int zr_scene_update_materials(zr_scene* s, const zr_material* m, uint32_t first, uint32_t count) { const int r = zr_scene_update_materials_async(s, nullptr, m, first, count); return count ? ThenWait(r) : r; }
int zr_scene_invalidate_alias_table(zr_scene* s)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_invalidate_alias_table: null argument");
    // kernels of earlier frames keep sampling the old table through the pointer they were launched with; the device buffer is only
    // rewritten by zr_scene_set_alias_table, which orders itself behind them
    std::lock_guard<std::mutex> lock(s->mtx);
    s->view.alias = nullptr; s->aliasHost.clear(); s->aliasOnDevice = false;
    return ZR_OK;
}
int zr_scene_set_alias_build(zr_scene* s, int mode)
{
    if (mode != ZR_ALIAS_BUILD_HOST && mode != ZR_ALIAS_BUILD_DEVICE) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_alias_build: mode %d is neither ZR_ALIAS_BUILD_HOST nor ZR_ALIAS_BUILD_DEVICE", mode);
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_alias_build: null argument");
    std::lock_guard<std::mutex> lock(s->mtx);
    s->aliasBuild = mode;
    return ZR_OK;
}
// The reference's steady-state behaviour (EmissiveTriangleAliasTable::Render, PreLighting.cpp:527-540: "fence hasn't passed, returning ..."): the
// old table keeps being sampled until the re-estimated powers have come back and the new table has been uploaded -- a frame or two later --
// and no render call ever waits for the device.  zr_scene_invalidate_alias_table is the deterministic form (new table in the very next frame).
int zr_scene_invalidate_alias_table_deferred(zr_scene* s)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_invalidate_alias_table_deferred: null argument");
    std::lock_guard<std::mutex> lock(s->mtx);
    if (s->view.alias) s->aliasStale = true;      // without a table there is nothing to keep: the next PRELIGHTING render builds one (first-frame path)
    return ZR_OK;
}
// One frame's instance update as the refit takes it, in one of three forms.  HostRecords: every record and matrix as the caller stated them, which the
// scene's host copies (hInstances / hToWorld) hold by then.  MovedMatrices: "instance idx[j] now has world matrix xf[j]" (zr_scene_move_instances_async),
// the records follow on the device.  Animated: the moved list is the scene's own, written on the device by zr::LaunchAnimate for time t -- nothing of it
// goes through the staging ring.  Both device forms carry the list's length and the range of light triangles its instances carry
enum class UpdateForm { HostRecords, MovedMatrices, Animated };
struct FrameUpdate { UpdateForm form; const uint32_t* idx; const float* xf; uint32_t nMoved, emFirst, emEnd; float t; };
// the range of light triangles the listed instances carry ([0, 0): none); a light that moves needs its object-space records first
static int SceneDirtyLights(const zr_scene* s, const char* fn, const uint32_t* idx, uint32_t count, uint32_t* first, uint32_t* end)
{
    *first = 0xffffffffu; *end = 0u;
    for (uint32_t j = 0; j < count; j++)
    {
        const uint32_t i = idx[j], b = s->hInstances[i].base_emissive_tri_offset;
        if (b == 0xffffffffu || !s->emissives.n) continue;
        if (!s->objectEmissives.p) return Fail(ZR_ERR_NOT_INITIALIZED, "%s: instance %u carries lights: call zr_scene_set_object_emissives first", fn, i);
        *first = std::min(*first, b); *end = std::max(*end, b + s->hNumTris[i]);
    }
    if (*end <= *first) *first = *end = 0;
    return ZR_OK;
}
// the host's matrices after zr_scene_animate: brought up to date for the time of the last one, where they are read
static void SceneAnimSyncHost(zr_scene* s)
{
    std::lock_guard<std::mutex> lock(s->animMtx);
    if (!s->anim || !s->anim->hostStale) return;
    zr_scene::Anim& A = *s->anim;
    std::vector<float> world(12 * (size_t)A.desc.num_nodes);
    zran::EvalNodeWorlds(A.desc, A.lastT, world.data());
    for (uint32_t j = 0; j < A.desc.num_instances; j++)
        std::memcpy(s->hToWorld.data() + 12 * (size_t)A.instIdx[j], world.data() + 12 * (size_t)A.instNode[j], 12 * sizeof(float));
    A.hostStale = false;
}

// ---- the steps of SceneRefitUpdate (below), in its order
// The frame's sizes and its layout in the staging slot, by form.  HostRecords: [n records | n matrices].  MovedMatrices: [seed | nMoved matrices |
// nMoved indices].  Animated: [seed].  seed = every matrix as the host has it, once -- while the device copy of the matrices is not current.
// (An animated frame without a seed stages nothing and takes no slot; every other form takes one as it always did, an empty moved list included.)
struct RefitFrame { uint32_t n; size_t instBytes, xfBytes, seedBytes, listBytes, stageBytes; bool takesSlot; };
static RefitFrame RefitFrameOf(const zr_scene* s, const FrameUpdate& u)
{
    RefitFrame F;
    F.n = (uint32_t)s->cur.instances.n; F.instBytes = (size_t)F.n * sizeof(zr_mesh_instance); F.xfBytes = 12 * (size_t)F.n * sizeof(float);
    const bool deviceForm = u.form != UpdateForm::HostRecords;
    F.seedBytes = deviceForm && (!s->toWorldDev || s->toWorld.n != 12 * (size_t)F.n) ? F.xfBytes : 0;
    F.listBytes = u.form == UpdateForm::MovedMatrices ? 13 * (size_t)u.nMoved * sizeof(uint32_t) : 0;
    F.stageBytes = deviceForm ? F.seedBytes + F.listBytes : F.instBytes + F.xfBytes;
    F.takesSlot = F.stageBytes || u.form != UpdateForm::Animated;
    return F;
}
// the vertex ranges zr_scene_update_vertices held back while a build was reading hVertices, in call order (the caller knows no build is running)
static void SceneFlushVertexCopies(zr_scene* s)
{
    for (const auto& p : s->hVertexPending) std::copy(p.second.begin(), p.second.end(), s->hVertices.begin() + p.first);
    s->hVertexPending.clear();
}
// background SAH rebuild: is a finished tree waiting to be installed by this update?  Its thread is joined either way; a tree that cannot be used
// (the scene changed shape under it, or it is too deep for the traversal stack) is dropped
static bool BgJoinFinished(zr_scene* s)
{
    zr_scene::Background& B = s->bg;
    if (!B.enabled || B.state.load(std::memory_order_acquire) != 2) return false;
    if (B.th.joinable()) B.th.join();
    const bool usable = B.packed && B.inst.size() == s->cur.instances.n && B.numTris == s->cur.numTris && B.stackNeed + 1 <= (uint32_t)kTravStack;
    if (!usable) B.state.store(0);
    return usable;
}
// ... and with it on, both sets must be able to hold any topology over these triangles (a BVH4 over nt triangles has < nt nodes): grown once,
// with their contents, behind a device-wide wait
static int BgGrowBuffers(zr_scene* s)
{
    AccelSet &a = s->cur, &b = s->prev;
    const size_t cap = a.numTris;
    if (a.nodes.n >= cap && !(s->refitReady && b.nodes.n < cap) && s->levelNodes.n >= cap && s->nodeBounds.n >= 6 * cap && s->bgDev.n >= 5 * cap && s->dMask.p) return ZR_OK;
    int r;
    HIP_TRY(hipDeviceSynchronize());
    if (!s->dMask.p && (r = s->dMask.Upload(s->hMask.data(), s->hMask.size()))) return r;
    if (s->bgDev.n < 5 * cap && (r = s->bgDev.Alloc(5 * cap))) return r;      // 4 child words per node (< cap nodes) + one word per triangle slot
    std::lock_guard<std::mutex> lock(s->mtx);
    if ((r = a.nodes.Grow(cap, a.numNodes)) || (b.nodes.p && (r = b.nodes.Grow(cap, s->refitReady || s->hasPrev ? b.numNodes : 0))) ||
        (r = s->levelNodes.Grow(cap, s->hLevelOrder.size())) || (r = s->nodeBounds.Grow(6 * cap, 0))) return r;
    SceneBind(s->view, a);
    return ZR_OK;
}
// the frame's input into a slot of the staging ring (RefitFrame: the layout)
static int RefitStage(zr_scene* s, const FrameUpdate& u, const RefitFrame& F, zr_scene::StageSlot** out)
{
    *out = nullptr;
    if (u.form == UpdateForm::Animated && F.seedBytes) SceneAnimSyncHost(s);      // (the seed takes hToWorld)
    if (!F.takesSlot) return ZR_OK;
    if (int r = StageAcquire(s, F.stageBytes, out)) return r;
    char* h = (char*)(*out)->host;
    if (u.form == UpdateForm::HostRecords) { memcpy(h, s->hInstances.data(), F.instBytes); memcpy(h + F.instBytes, s->hToWorld.data(), F.xfBytes); return ZR_OK; }
    if (F.seedBytes) memcpy(h, s->hToWorld.data(), F.xfBytes);
    const size_t matrixBytes = 12 * (size_t)u.nMoved * sizeof(float);
    if (u.form == UpdateForm::MovedMatrices) { memcpy(h + F.seedBytes, u.xf, matrixBytes); memcpy(h + F.seedBytes + matrixBytes, u.idx, (size_t)u.nMoved * sizeof(uint32_t)); }
    return ZR_OK;
}
// Both sets must hold the same tree before one is refit in place of the other: `prev` becomes a copy of `cur` on `st` (once, and again after a rebuild or an
// install).  Also sizes what only the refit needs: node bounds, device matrices.  The conditions decide when a hipMalloc / hipFree makes the device wait
static int SceneDuplicate(zr_scene* s, hipStream_t st)
{
    AccelSet &a = s->cur, &b = s->prev;
    const size_t n = a.instances.n, nn = a.numNodes, nt = a.numTris, nodeCap = s->bg.enabled ? std::max(nn, nt) : nn;
    int r;
    if ((b.instances.n != n && (r = b.instances.Alloc(n))) || (nodeCap && b.nodes.n < nodeCap && (r = b.nodes.Alloc(nodeCap))) ||
        (b.tris.n != nt && (r = b.tris.Alloc(nt))) || (b.meta.n != a.meta.n && (r = b.meta.Alloc(a.meta.n))) ||
        (nodeCap && s->nodeBounds.n < 6 * nodeCap && (r = s->nodeBounds.Alloc(6 * nodeCap))) || (s->toWorld.n != 12 * n && (r = s->toWorld.Alloc(12 * n)))) return r;
    HIP_TRY(hipMemcpyAsync(b.instances.p, a.instances.p, n * sizeof(zr_mesh_instance), hipMemcpyDeviceToDevice, st));
    if (b.instRecs.n != n && (r = b.instRecs.Alloc(n))) return r;
    HIP_TRY(hipMemcpyAsync(b.instRecs.p, a.instRecs.p, n * sizeof(InstRec), hipMemcpyDeviceToDevice, st));
    if (nn) HIP_TRY(hipMemcpyAsync(b.nodes.p, a.nodes.p, nn * sizeof(Bvh4Node), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.tris.p, a.tris.p, nt * sizeof(BvhTri), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.meta.p, a.meta.p, a.meta.n * sizeof(TriMeta), hipMemcpyDeviceToDevice, st));
    b.numNodes = a.numNodes; b.numTris = a.numTris;
    s->refitReady = true;
    return ZR_OK;
}
// what k_refresh_emissives reads and writes (zr_pose.h), from the set that is current
static zr::RefreshBuffers SceneRefreshBuffers(const zr_scene* s)
{
    return zr::RefreshBuffers{s->emissives.p, s->objectEmissives.p, s->emissiveOwner.p, s->toWorld.p, s->vertices.p, (uint32_t)s->vertices.n,
        s->cur.instances.p, s->indices.p, (uint32_t)s->indices.n};
}
// the frame's records and matrices into the set that has just become current: uploaded, or computed on the device from the previous set's records
// and the moved list (zr_tu_scene_update.hip; the animation writes its list first, zr_tu_anim.hip); then their decoded table
static int RefitWriteRecords(zr_scene* s, hipStream_t st, const FrameUpdate& u, const RefitFrame& F, const zr_scene::StageSlot* t)
{
    const char* h = t ? (const char*)t->host : nullptr;
    if (u.form == UpdateForm::HostRecords)
    {
        HIP_TRY(hipMemcpyAsync(s->cur.instances.p, h, F.instBytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s->toWorld.p, h + F.instBytes, F.xfBytes, hipMemcpyHostToDevice, st));
    }
    else
    {
        if (F.seedBytes) HIP_TRY(hipMemcpyAsync(s->toWorld.p, h, F.xfBytes, hipMemcpyHostToDevice, st));
        const uint32_t* movedList = s->movedDev.p;
        if (u.form == UpdateForm::Animated)
        {   // behind SceneWaitUsers: ordered after the previous update, whose kernels read the list this writes
            zr_scene::Anim& A = *s->anim;
            HIP_TRY(zr::LaunchAnimate(st, u.t, A.dNodes.p, A.dKeys.p, A.dAnimated.p, A.nAnimated, A.dLevelNodes.p, A.levelOffsets.data(),
                (uint32_t)A.levelOffsets.size() - 1, A.dLocal.p, A.dWorld.p, A.dInstNode.p, u.nMoved, A.dMoved.p));
            movedList = A.dMoved.p;
            if (s->skin || s->morph)
            {   // the node matrices are on the device: joint matrices and weights of time t, then the listed vertices and their hit-table entries, ahead of the refit that reads them
                zr::PoseTables T{};
                if (const zr_scene::Skin* K = s->skin.get())
                { T.J = K->dJ.p; T.nodeWorld = A.dWorld.p; T.jointNode = K->dJointNode.p; T.inverseBind = K->dInverseBind.p; T.numJoints = K->numJoints; T.influences = K->dInfluences.p; }
                if (const zr_scene::Morph* M = s->morph.get())
                {
                    T.weights = M->dWeights.p; T.numWeights = M->numWeights; T.tracks = M->dTracks.p; T.trackOfWeight = M->dTrackOfWeight.p; T.weightFirst = M->dWeightFirst.p;
                    T.times = M->dTimes.p; T.values = M->dValues.p; T.restWeights = M->dRestWeights.p; T.targets = M->dTargets.p; T.deltas = M->dDeltas.p;
                }
                T.rest = s->pose.dRest.p;
                VtxDir* tangents = nullptr;
#if ZR_HIT_TANGENTS
                tangents = s->vtxTangents.p;
#endif
                HIP_TRY(zr::LaunchPose(st, u.t, T, s->pose.ranges.data(), (uint32_t)s->pose.ranges.size(), s->vertices.p, s->vtxNormals.p, tangents));
            }
        }
        else if (u.nMoved) HIP_TRY(hipMemcpyAsync(s->movedDev.p, h + F.seedBytes, F.listBytes, hipMemcpyHostToDevice, st));
        HIP_TRY(zr::LaunchMoveInstances(st, s->cur.instances.p, s->prev.instances.p, s->toWorld.p, F.n, s->movedSlot.p, movedList, u.nMoved,
            s->emissives.p, s->objectEmissives.p, s->emissiveOwner.p, u.emFirst, u.emEnd));
        // deformed lights: the listed triangles from the vertices LaunchPose wrote and the matrices k_move_instances has just left in toWorld
        if (u.form == UpdateForm::Animated && (s->skin || s->morph) && !s->pose.lights.empty())
            HIP_TRY(zr::LaunchRefreshEmissives(st, SceneRefreshBuffers(s), s->pose.dLights.p, 0, (uint32_t)s->pose.lights.size()));
    }
    s->toWorldDev = true;
    return SceneFillInstRecs(s, st);
}
// The background build's topology goes into the set that has just become current (last frame's "previous": nobody needs it any more); its
// triangles and boxes are then computed for THIS update's transforms by the refit kernels, like any other frame's
static int BgInstall(zr_scene* s, hipStream_t st)
{
    zr_scene::Background& B = s->bg;
    AccelSet& a = s->cur;
    const size_t devWords = 4 * (size_t)B.numNodes + B.numTris;
    if (!B.pkgCopied) HIP_TRY(hipEventCreateWithFlags(&B.pkgCopied, hipEventDisableTiming));
    HIP_TRY(hipMemcpyAsync(s->bgDev.p, B.pkg, devWords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->levelNodes.p, B.pkg + devWords, (size_t)B.numNodes * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(B.pkgCopied, st)); B.pkgInFlight = true;      // the next build's thread waits for it before it overwrites the package
    hipLaunchKernelGGL(k_install_topology, dim3((uint32_t)((std::max<size_t>(B.numNodes, B.numTris) + 255) / 256)), dim3(256), 0, st,
        a.nodes.p, s->bgDev.p, B.numNodes, a.tris.p, s->bgDev.p + 4 * (size_t)B.numNodes, B.numTris, a.meta.p, s->dMask.p);
    s->hLevelOrder.assign(B.pkg + devWords, B.pkg + devWords + B.numNodes); s->levelOffsets = B.levelOffsets;
    a.numNodes = B.numNodes; s->deviceBuilt = false;
    if (B.maxDepth > s->maxDepth) s->maxDepth = B.maxDepth;
    s->refitReady = false;      // the two sets hold different topologies now: the next update duplicates this one first
    B.installed++; B.refitsSince = 0; B.state.store(0, std::memory_order_release);
    return ZR_OK;
}
// everything is enqueued: the host's view of the matrices follows.  HostRecords: zr_scene_update_instances_async did it from the caller's arrays up
// front.  Animated: lazily (SceneAnimSyncHost), from the time alone
static void RefitFollowOnHost(zr_scene* s, const FrameUpdate& u)
{
    if (u.form == UpdateForm::Animated)
    {
        std::lock_guard<std::mutex> lock(s->animMtx);
        zr_scene::Anim& A = *s->anim;
        if (!A.hasT || std::memcmp(&A.lastT, &u.t, sizeof(float))) s->bg.movedSinceBuild = true;
        A.lastT = u.t; A.hasT = true; A.hostStale = true;
    }
    else if (u.form == UpdateForm::MovedMatrices)
        for (uint32_t j = 0; j < u.nMoved; j++)
        {
            float* M = s->hToWorld.data() + 12 * (size_t)u.idx[j];
            if (std::memcmp(M, u.xf + 12 * (size_t)j, 12 * sizeof(float))) { s->movedEver[u.idx[j]] = 1; s->bg.movedSinceBuild = true; }
            std::memcpy(M, u.xf + 12 * (size_t)j, 12 * sizeof(float));
        }
}
// The background builder's thread: the host's binned-SAH build over the snapshot (bg.inst / bg.xf / bg.own), then the topology packed into pinned
// memory -- this thread's time, not the installing update's (zr_scene::Background: the package's layout)
static void BgBuildThread(zr_scene* s)
{
    zr_scene::Background& Q = s->bg;
    const auto t0 = std::chrono::steady_clock::now();
    BuiltBvh bvh = BvhBuilder().Build(SceneBuilderDesc(s, Q.inst.data(), (uint32_t)Q.inst.size(), Q.xf.data()), Q.own.empty() ? nullptr : Q.own.data());
    std::vector<uint32_t> levelOrder;
    BvhLevels(bvh.nodes4, levelOrder, Q.levelOffsets);
    const auto t1 = std::chrono::steady_clock::now();
    const size_t nn = bvh.nodes4.size(), nt = bvh.tris.size(), words = 5 * nn + nt;
    Q.packed = false;
    if (hipSetDevice(s->device) == hipSuccess)
    {
        if (Q.pkgInFlight) { (void)hipEventSynchronize(Q.pkgCopied); Q.pkgInFlight = false; }      // the previous package's copies have left the buffer
        if (Q.pkgCap < words)
        {
            if (Q.pkg) { (void)hipHostFree(Q.pkg); Q.pkg = nullptr; Q.pkgCap = 0; }
            void* h = nullptr;
            if (hipHostMalloc(&h, (words + words / 8) * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess) { Q.pkg = (uint32_t*)h; Q.pkgCap = words + words / 8; }
            else (void)hipGetLastError();
        }
        if (Q.pkg)
        {
            uint32_t* w = Q.pkg;
            for (size_t i = 0; i < nn; i++) for (int c = 0; c < 4; c++) *w++ = bvh.nodes4[i].child[c];
            for (size_t i = 0; i < nt; i++) *w++ = bvh.tris[i].gidx;
            std::memcpy(w, levelOrder.data(), nn * sizeof(uint32_t));
            Q.packed = true;
        }
    }
    Q.numNodes = (uint32_t)nn; Q.numTris = (uint32_t)nt; Q.stackNeed = bvh.stackNeed; Q.maxDepth = bvh.maxDepth;
    Q.buildMs = std::chrono::duration<double, std::milli>(t1 - t0).count();
    Q.packMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (ZR_EXP_ENV("ZR_BVH_TIMING"))
        std::fprintf(stderr, "[zr_scene] background tree: %zu nodes over %zu triangles, build %.1f ms, package (%.1f MB pinned) %.1f ms\n", nn, nt, Q.buildMs, words * 4e-6, Q.packMs);
    Q.state.store(2, std::memory_order_release);
}
// ... started on this update's transforms when none is in flight and something has moved since the last one was (host copies: hInstances, and
// hToWorld, which holds this update's matrices in every form)
static void BgStartBuild(zr_scene* s)
{
    zr_scene::Background& B = s->bg;
    if (!B.enabled || B.state.load(std::memory_order_acquire) != 0 || B.refitsSince < 1 || !B.movedSinceBuild || s->cur.meta.n <= BvhBuilder::kTinyScene) return;
    B.movedSinceBuild = false;
    if (B.th.joinable()) B.th.join();
    SceneFlushVertexCopies(s);
    SceneAnimSyncHost(s);
    B.inst = s->hInstances; B.xf = s->hToWorld;
    { const char* e = ZR_EXP_ENV("ZR_BVH_GROUP"); if (e && !std::strcmp(e, "0")) B.own.clear(); else B.own = s->movedEver; }
    B.state.store(1, std::memory_order_release); B.started++;
    B.th = std::thread(BgBuildThread, s);
}

// ---- refit on the device, stream-ordered: nothing below waits on the host (the staging ring aside, when the host runs far ahead, and the one-time growth
// of the buffers under the background rebuild).  The shared tail of the three forms of the update.  What is enqueued on `st` or waited for, in order:
//    1 StageAcquire (waits when the host is > 4 updates ahead)   6 SceneDuplicate's copies (first refit; after a rebuild / install)   11 the install's copies + k_install_topology
//    2 the memcpy into the slot                                  7 SceneFlip                                                         12 k_refit_tris
//    3 SceneWaitUsers (`st` behind readers on other streams)     8 the uploads, or LaunchAnimate + LaunchMoveInstances               13 k_refit_level, one launch per level
//    4 lock mtx (held to the end: a render sees all or nothing)  9 LaunchFillInstRecs                                                14 the `updated` event
//    5 the moved-slot memset (a scene's first device-form frame) 10 StageCommit                                                      15 the next background build's thread starts
static int SceneRefitUpdate(zr_scene* s, hipStream_t st, const FrameUpdate& u)
{
    int r;
    const bool install = BgJoinFinished(s);
    if (s->bg.enabled && (r = BgGrowBuffers(s))) return r;
    const RefitFrame F = RefitFrameOf(s, u);
    zr_scene::StageSlot* t;
    if ((r = RefitStage(s, u, F, &t))) return r;                                                    // 1, 2
    if ((r = SceneWaitUsers(s, st))) return r;                                                      // 3
    std::lock_guard<std::mutex> lock(s->mtx);                                                       // 4
    if (u.form != UpdateForm::HostRecords && (s->movedSlot.n != F.n || s->movedDev.n != 13 * (size_t)F.n))
    {   // once per scene: each instance's position in the frame's moved list, and the list; the slots start out as "did not move", in stream order
        if ((r = s->movedSlot.Alloc(F.n)) || (r = s->movedDev.Alloc(13 * (size_t)F.n))) return r;
        HIP_TRY(hipMemsetAsync(s->movedSlot.p, 0xff, (size_t)F.n * sizeof(uint32_t), st));         // 5
    }
    if (!s->refitReady && (r = SceneDuplicate(s, st))) return r;                                    // 6
    SceneFlip(s);                                                                                   // 7: both sets hold the same tree, counts included
    if ((r = RefitWriteRecords(s, st, u, F, t))) return r;                                          // 8, 9
    if (t && (r = StageCommit(t, st))) return r;                                                    // 10
    if (install) { if ((r = BgInstall(s, st))) return r; }                                          // 11
    else if (s->bg.enabled) s->bg.refitsSince++;
    const AccelSet& a = s->cur;
    hipLaunchKernelGGL(k_refit_tris, dim3((a.numTris + 255) / 256), dim3(256), 0, st, a.tris.p, a.numTris, a.meta.p, a.instances.p, s->toWorld.p, s->vertices.p, s->indices.p);   // 12
    LaunchRefitLevels(s, st);                                                                       // 13
    HIP_TRY(hipGetLastError());
    RefitFollowOnHost(s, u);
    SceneBind(s->view, s->cur);
    if ((r = SceneMarkUpdatedLocked(s, st))) return r;                                              // 14
    BgStartBuild(s);                                                                                // 15
    return ZR_OK;
}

// TLAS / instance-buffer update of a frame (RtAccelerationStructure.cpp:382-506, 708-787): the current instance buffer and acceleration
// structure become the previous ones, the new ones follow the new object-to-world matrices.  Default: a **refit on the device** -- the BVH4 built
// at zr_scene_create keeps its topology, k_refit_tris re-transforms the triangles and k_refit_level recomputes + re-quantises the node boxes
// level by level (what a D3D12 TLAS / BLAS update with ALLOW_UPDATE does); ZR_SCENE_UPDATE=rebuild / rebuild_host select a new tree per frame
// instead (UpdateMode; better trees after large motion, host-synchronous).  Results do not depend on the tree (zr_intersect.h).
int zr_scene_update_instances_async(zr_scene* s, void* stream, const zr_mesh_instance* instances, const float* instance_to_world, uint32_t n)
{
    if (!s || !instances || !instance_to_world) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_update_instances: null argument");
    if (n != s->cur.instances.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_update_instances: %u instances, the scene has %zu", n, s->cur.instances.n);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const UpdateMode mode = SceneUpdateMode();
    int r;
    SceneAnimSyncHost(s);
    for (uint32_t i = 0; i < n; i++) RaiseMaxTex(s, 0, instances[i].base_color_tex);
    for (uint32_t i = 0; i < n; i++)      // the reference's static -> dynamic conversion of an instance that starts to move (SceneCore.cpp:1038)
        if (std::memcmp(s->hToWorld.data() + 12 * (size_t)i, instance_to_world + 12 * (size_t)i, 12 * sizeof(float))) { s->movedEver[i] = 1; s->bg.movedSinceBuild = true; }
    std::memcpy(s->hToWorld.data(), instance_to_world, 12 * (size_t)n * sizeof(float));
    s->hInstances.assign(instances, instances + n);
    if (mode == UpdateMode::RebuildDevice && s->cur.meta.n > BvhBuilder::kTinyScene)
    {
        // ---- a NEW tree on the device (ZR_SCENE_UPDATE=rebuild): LBVH over the moved triangles, ~1 ms for the 380k-triangle atrium against 192 ms
        // for the host's binned-SAH rebuild (ZR_SCENE_UPDATE=rebuild_host); what the reference's per-frame TLAS rebuild is (RtAccelerationStructure.cpp:708-789)
        const size_t nt = s->cur.meta.n;
        HIP_TRY(hipDeviceSynchronize());           // buffers change roles and may be reallocated below: a host-synchronous path
        std::lock_guard<std::mutex> lock(s->mtx);
        AccelSet& b = s->prev;                     // the build's target, sized here, current from the flip on
        if ((b.instances.n != n && (r = b.instances.Alloc(n))) || (b.nodes.n < nt && (r = b.nodes.Alloc(nt))) ||
            (b.tris.n < nt && (r = b.tris.Alloc(nt))) || (b.meta.n != nt && (r = b.meta.Alloc(nt))) ||
            (s->toWorld.n != 12 * (size_t)n && (r = s->toWorld.Alloc(12 * (size_t)n)))) return r;
        if (!s->hasPrev && !s->refitReady) HIP_TRY(hipMemcpy(b.meta.p, s->cur.meta.p, nt * sizeof(TriMeta), hipMemcpyDeviceToDevice));
        if (b.instRecs.n != n && (r = b.instRecs.Alloc(n))) return r;
        SceneFlip(s);
        HIP_TRY(hipMemcpy(s->cur.instances.p, instances, (size_t)n * sizeof(zr_mesh_instance), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->toWorld.p, instance_to_world, 12 * (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        s->toWorldDev = true;
        // (the new records' table first, behind the blocking upload above and on the build's stream: a failure of either takes the roll-back below)
        if ((r = SceneFillInstRecs(s, st)) || (r = DeviceRebuild(s, st)))
        {
            // roll back: a build that fails (allocation, a tree deeper than the traversal stack) must leave the scene rendering as before the call.  A second flip
            // gives the sets their old roles and counts again (DeviceRebuild states a tree's counts only once it has succeeded); `view` has not been touched.  The
            // "previous" set was the build's target, so there is no previous structure any more (the CtT / temporal passes bind the current one, as in frame 1).
            (void)hipDeviceSynchronize();
            SceneFlip(s); s->hasPrev = false;
            return r;
        }
        SceneBind(s->view, s->cur);
        s->refitReady = false;      // the two sets no longer share a topology
        return ZR_OK;
    }
    if (mode != UpdateMode::Refit)
    {
        BuiltBvh bvh = BvhBuilder().Build(SceneBuilderDesc(s, instances, n, instance_to_world));
        if (bvh.stackNeed + 1 > (uint32_t)kTravStack) return Fail(ZR_ERR_UNSUPPORTED, "BVH needs %u traversal stack entries (limit %d)", bvh.stackNeed, kTravStack - 1);
        HIP_TRY(hipDeviceSynchronize());           // the host rebuild reallocates: a host-synchronous path by construction (ZR_SCENE_UPDATE=rebuild_host)
        std::lock_guard<std::mutex> lock(s->mtx);
        if (s->prev.instRecs.n != n && (r = s->prev.instRecs.Alloc(n))) return r;
        SceneFlip(s);
        // (a failing upload or fill returns with the roles already changed: this debug path has no roll-back, and the scene is not usable after an error from it)
        AccelSet& a = s->cur;
        if ((r = a.instances.Upload(instances, n)) || (r = a.nodes.Upload(bvh.nodes4.data(), bvh.nodes4.size())) ||
            (r = a.tris.Upload(bvh.tris.data(), bvh.tris.size())) || (r = a.meta.Upload(bvh.meta.data(), bvh.meta.size()))) return r;
        a.numNodes = (uint32_t)bvh.nodes4.size(); a.numTris = (uint32_t)bvh.tris.size();
        SceneBind(s->view, a);
        if ((r = SceneFillInstRecs(s, nullptr))) return r;
        HIP_TRY(hipStreamSynchronize(nullptr));      // host-synchronous like the uploads: renders on any stream may follow
        if (bvh.maxDepth > s->maxDepth) s->maxDepth = bvh.maxDepth;
        BvhLevels(bvh.nodes4, s->hLevelOrder, s->levelOffsets);
        if ((r = s->levelNodes.Upload(s->hLevelOrder.data(), s->hLevelOrder.size()))) return r;
        s->refitReady = false;      // the two sets no longer share a topology
        s->toWorldDev = false;      // ... and the device matrices were not touched
        return ZR_OK;
    }
    return SceneRefitUpdate(s, st, FrameUpdate{UpdateForm::HostRecords, nullptr, nullptr, 0, 0, 0, 0.0f});
}
// A tree built for where the instances are NOW, in the background, swapped in by a later zr_scene_update_instances(_async) (see zr_scene::Background).
int zr_scene_set_background_rebuild(zr_scene* s, int enable)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_background_rebuild: null scene");
    std::lock_guard<std::mutex> lock(s->mtx);
    s->bg.enabled = enable != 0;
    return ZR_OK;
}
int zr_scene_background_rebuild_stats(zr_scene* s, uint64_t* started, uint64_t* installed, int* building)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_background_rebuild_stats: null scene");
    if (started) *started = s->bg.started.load(std::memory_order_relaxed);
    if (installed) *installed = s->bg.installed.load(std::memory_order_relaxed);
    if (building) *building = s->bg.state.load(std::memory_order_acquire);
    return ZR_OK;
}
int zr_scene_update_instances(zr_scene* s, const zr_mesh_instance* instances, const float* to_world, uint32_t n) { return ThenWait(zr_scene_update_instances_async(s, nullptr, instances, to_world, n)); }

// ---- the device form of the frame's update: the caller says "instance i now has world matrix M", the records follow on the stream
int zr_scene_set_object_emissives(zr_scene* s, const zr_emissive_triangle* object_space, uint32_t n)
{
    if (!s || (!object_space && n)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_object_emissives: null argument");
    if (n != s->emissives.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_object_emissives: %u records, the scene has %zu emissive triangles", n, s->emissives.n);
    // a pose set that lists lights has saved their records and writes them every frame: new ones under it would be lost to the next animate or the next clear
    if (!s->pose.lights.empty()) return Fail(ZR_ERR_UNSUPPORTED, "zr_scene_set_object_emissives: a skin or morph set poses %zu light triangles of this scene: clear it first", s->pose.lights.size());
    // the instance that carries each light triangle, from the instances' first light triangle and triangle counts
    std::vector<uint32_t> owner(n, 0xffffffffu);
    for (size_t i = 0; i < s->hInstances.size(); i++)
    {
        const uint32_t b = s->hInstances[i].base_emissive_tri_offset;
        if (b == 0xffffffffu) continue;
        if ((uint64_t)b + s->hNumTris[i] > n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_object_emissives: instance %zu carries light triangles [%u, %llu), the scene has %u", i, b, (unsigned long long)b + s->hNumTris[i], n);
        std::fill(owner.begin() + b, owner.begin() + b + s->hNumTris[i], (uint32_t)i);
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());      // an update in flight may still read the records this call replaces
    int r;
    if ((r = s->objectEmissives.Upload(object_space, n)) || (r = s->emissiveOwner.Upload(owner.data(), n))) { s->objectEmissives.Free(); s->emissiveOwner.Free(); return r; }
    HIP_TRY(hipDeviceSynchronize());
    // k_move_emissives keeps every non-geometric field of the object-space record, its emissive texture index included: these records count for the
    // descriptor-table bounds check of zr_pass_render like the ones zr_scene_update_emissives hands over
    for (uint32_t i = 0; i < n; i++) RaiseMaxTex(s, 3, object_space[i].packed_b & 0xffffu);
    return ZR_OK;
}
int zr_scene_has_object_emissives(const zr_scene* s) { return s && s->objectEmissives.p ? 1 : 0; }
int zr_scene_move_instances_async(zr_scene* s, void* stream, const uint32_t* instance_idx, const float* world_3x4, uint32_t n_moved)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_move_instances: null scene");
    if (n_moved && (!instance_idx || !world_3x4)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_move_instances: null argument with %u moved instances", n_moved);
    if (int r = RefuseRebuildMode("zr_scene_move_instances")) return r;
    const uint32_t n = (uint32_t)s->cur.instances.n;
    FrameUpdate u{UpdateForm::MovedMatrices, instance_idx, world_3x4, n_moved, 0, 0, 0.0f};
    std::vector<uint8_t> listed(n, 0);      // (the list as a whole first, then what its instances carry)
    for (uint32_t j = 0; j < n_moved; j++)
    {
        const uint32_t i = instance_idx[j];
        if (i >= n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_move_instances: instance %u (entry %u of the list), the scene has %u", i, j, n);
        if (listed[i]) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_move_instances: instance %u is listed twice", i);
        listed[i] = 1;
    }
    if (int r = SceneDirtyLights(s, "zr_scene_move_instances", instance_idx, n_moved, &u.emFirst, &u.emEnd)) return r;
    HIP_TRY(hipSetDevice(s->device));
    SceneAnimSyncHost(s);      // (a frame moved by hand between animated ones: the host's matrices are compared and replaced per moved instance)
    return SceneRefitUpdate(s, (hipStream_t)stream, u);
}
// the hit-table entries of vertices [first, first + count) from the vertex buffer as it is on `st`
static int SceneFillVtxTables(zr_scene* s, hipStream_t st, uint32_t first, uint32_t count)
{
    hipError_t e = zr::LaunchFillVtxNormals(st, s->vtxNormals.p + first, s->vertices.p + first, count, false);
#if ZR_HIT_TANGENTS
    if (e == hipSuccess) e = zr::LaunchFillVtxNormals(st, s->vtxTangents.p + first, s->vertices.p + first, count, true);
#endif
    if (e != hipSuccess) return Fail(ZR_ERR_HIP, "k_fill_vtx_normals failed: %s", hipGetErrorString(e));
    return ZR_OK;
}
// ---- the vertices zr_scene_animate poses (zr_scene::Pose).  Every change of the skin set, the morph set, the range list and the rest records is this call.
// The skin set stays (keepSkin), or newSkin takes its place (null: none); newMorph takes the morph set's place (null: none) -- a morph set is laid out
// against the skin set and never outlives a change of it.  The descs have passed ValidateSkin / ValidateMorph, newMorph against the skin ranges that will
// hold.  Host-synchronous.  What can fail for want of memory happens before the scene is touched.
static int ScenePoseRebuild(zr_scene* s, bool keepSkin, const zr_skin_desc* newSkin, const zr_morph_desc* newMorph)
{
    if (!newSkin && !newMorph && !s->morph && (keepSkin || !s->skin)) return ZR_OK;      // nothing to lay out, nothing to drop
    const zr_scene::Pose& O = s->pose;
    // the range list: the skin ranges no morph range equals, then the morph ranges; a range with no vertices is not listed
    std::vector<zr_skin_range> skinRanges;
    if (newSkin) skinRanges.assign(newSkin->ranges, newSkin->ranges + newSkin->num_ranges);
    else if (keepSkin && s->skin) skinRanges = s->skin->ranges;
    zr_skin_desc skinDesc{};
    skinDesc.ranges = skinRanges.data(); skinDesc.num_ranges = (uint32_t)skinRanges.size();
    const uint32_t numMorphRanges = newMorph ? newMorph->num_ranges : 0;
    std::vector<uint32_t> weightFirst(newMorph ? newMorph->num_tracks : 0);
    const uint32_t numWeights = newMorph ? zrmo::WeightOffsets(*newMorph, weightFirst.data()) : 0;
    std::vector<int64_t> skinOf(numMorphRanges);
    std::vector<uint8_t> morphed(skinRanges.size(), 0);
    for (uint32_t i = 0; i < numMorphRanges; i++) if ((skinOf[i] = zrmo::SkinRangeOf(newMorph->ranges[i], &skinDesc)) >= 0) morphed[skinOf[i]] = 1;
    zr_scene::Pose P;
    auto list = [&P](zr::PoseRange g)
    {
        if (!g.numVertices) return;
        g.restFirst = (uint32_t)P.hRest.size();
        P.hRest.resize(P.hRest.size() + g.numVertices);
        P.ranges.push_back(g);
    };
    for (size_t q = 0; q < skinRanges.size(); q++)
        if (!morphed[q]) list(zr::PoseRange{skinRanges[q].first_vertex, skinRanges[q].num_vertices, 0, skinRanges[q].first_influence, 0, 0, 0, zr::kPoseSkin});
    for (uint32_t i = 0; i < numMorphRanges; i++)
    {
        const zr_morph_range& g = newMorph->ranges[i];
        const bool skinned = skinOf[i] >= 0;
        list(zr::PoseRange{g.first_vertex, g.num_vertices, 0, skinned ? skinRanges[skinOf[i]].first_influence : 0u, g.first_target, g.num_targets, weightFirst[g.track],
            skinned ? zr::kPoseSkin | zr::kPoseMorph : zr::kPoseMorph});
    }
    // the light list: every light triangle with a vertex in one of the new ranges, by triangle index (the host's index copy and instance records say which)
    auto inRanges = [](const std::vector<zr::PoseRange>& ranges, uint32_t kinds, uint32_t v)
    { for (const zr::PoseRange& g : ranges) if ((g.kind & kinds) && v >= g.firstVertex && v - g.firstVertex < g.numVertices) return true; return false; };
    const uint32_t anyKind = zr::kPoseSkin | zr::kPoseMorph;
    if (s->emissives.n && !P.ranges.empty())
        for (size_t i = 0; i < s->hInstances.size(); i++)
        {
            const zr_mesh_instance& I = s->hInstances[i];
            if (I.base_emissive_tri_offset == 0xffffffffu) continue;
            for (uint32_t t = 0; t < s->hNumTris[i]; t++)
            {
                const uint64_t at = (uint64_t)I.base_idx_offset + 3ull * t, k = (uint64_t)I.base_emissive_tri_offset + t;
                if (at + 3 > s->hIndices.size() || k >= s->emissives.n) break;
                const uint64_t v[3] = {(uint64_t)I.base_vtx_offset + s->hIndices[at], (uint64_t)I.base_vtx_offset + s->hIndices[at + 1], (uint64_t)I.base_vtx_offset + s->hIndices[at + 2]};
                if (v[0] >= s->vertices.n || v[1] >= s->vertices.n || v[2] >= s->vertices.n) continue;
                if (inRanges(P.ranges, anyKind, (uint32_t)v[0]) || inRanges(P.ranges, anyKind, (uint32_t)v[1]) || inRanges(P.ranges, anyKind, (uint32_t)v[2]))
                { P.lights.push_back(zr::LightEntry{(uint32_t)k, (uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]}); P.lightOwner.push_back((uint32_t)i); }
            }
        }
    if (!P.lights.empty() && !s->objectEmissives.p)
        return Fail(ZR_ERR_NOT_INITIALIZED, "%s: the ranges hold vertices of light triangle %u: call zr_scene_set_object_emissives first", newMorph ? "zr_scene_set_morph" : "zr_scene_set_skinning", P.lights[0].tri);
    {   // by triangle index, the owners with them
        std::vector<uint32_t> order(P.lights.size());
        for (uint32_t j = 0; j < order.size(); j++) order[j] = j;
        std::sort(order.begin(), order.end(), [&P](uint32_t a, uint32_t b) { return P.lights[a].tri < P.lights[b].tri; });
        std::vector<zr::LightEntry> lights(order.size()); std::vector<uint32_t> owner(order.size());
        for (size_t j = 0; j < order.size(); j++) { lights[j] = P.lights[order[j]]; owner[j] = P.lightOwner[order[j]]; }
        P.lights.swap(lights); P.lightOwner.swap(owner);
    }
    SceneAnimSyncHost(s);      // (the owners' matrices as they stand: saved with the records below, compared when the records go back)
    // the rest records: what the new ranges hold with the ranges listed until now back at rest (those may lie outside the new ones) -- the new ranges alone
    // are read back, and the old rest records laid over them where the two meet
    HIP_TRY(hipDeviceSynchronize());      // an animate in flight still reads the tables and writes the vertices; renders in flight read them
    if (!P.lights.empty())
    {   // ... and the listed lights' records likewise: read back over the span of the list, the records an earlier set saved laid over them
        const uint32_t lo = P.lights.front().tri, hi = P.lights.back().tri + 1;
        std::vector<zr_emissive_triangle> object(hi - lo), world(hi - lo);
        HIP_TRY(hipMemcpy(object.data(), s->objectEmissives.p + lo, (size_t)(hi - lo) * sizeof(zr_emissive_triangle), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(world.data(), s->emissives.p + lo, (size_t)(hi - lo) * sizeof(zr_emissive_triangle), hipMemcpyDeviceToHost));
        P.hLightObject.resize(P.lights.size()); P.hLightWorld.resize(P.lights.size()); P.hLightXf.resize(12 * P.lights.size());
        size_t q = 0;
        for (size_t j = 0; j < P.lights.size(); j++)
        {
            const uint32_t k = P.lights[j].tri;
            while (q < O.lights.size() && O.lights[q].tri < k) q++;
            const bool saved = q < O.lights.size() && O.lights[q].tri == k;
            P.hLightObject[j] = saved ? O.hLightObject[q] : object[k - lo];
            P.hLightWorld[j] = saved ? O.hLightWorld[q] : world[k - lo];
            std::memcpy(P.hLightXf.data() + 12 * j, saved ? O.hLightXf.data() + 12 * q : s->hToWorld.data() + 12 * (size_t)P.lightOwner[j], 12 * sizeof(float));
        }
    }
    for (const zr::PoseRange& g : P.ranges)
    {
        HIP_TRY(hipMemcpy(P.hRest.data() + g.restFirst, s->vertices.p + g.firstVertex, (size_t)g.numVertices * sizeof(zr_vertex), hipMemcpyDeviceToHost));
        for (const zr::PoseRange& o : O.ranges)
        {
            const uint64_t lo = std::max(g.firstVertex, o.firstVertex), hi = std::min((uint64_t)g.firstVertex + g.numVertices, (uint64_t)o.firstVertex + o.numVertices);
            if (hi > lo) std::copy(O.hRest.begin() + o.restFirst + (lo - o.firstVertex), O.hRest.begin() + o.restFirst + (hi - o.firstVertex), P.hRest.begin() + g.restFirst + (lo - g.firstVertex));
        }
    }
    int r;
    if ((r = P.dRest.Upload(P.hRest.data(), P.hRest.size())) || (!P.lights.empty() && (r = P.dLights.Upload(P.lights.data(), P.lights.size())))) return r;
    std::unique_ptr<zr_scene::Skin> K;
    if (newSkin)
    {
        K.reset(new zr_scene::Skin());
        K->ranges = skinRanges; K->numJoints = newSkin->num_joints;
        std::vector<uint32_t> jointNode(K->numJoints); std::vector<float> inverseBind(12 * (size_t)K->numJoints);
        for (uint32_t j = 0; j < K->numJoints; j++) { jointNode[j] = newSkin->joints[j].node; std::memcpy(inverseBind.data() + 12 * (size_t)j, newSkin->joints[j].inverse_bind, 12 * sizeof(float)); }
        if ((r = K->dJointNode.Upload(jointNode.data(), jointNode.size())) || (r = K->dInverseBind.Upload(inverseBind.data(), inverseBind.size())) ||
            (r = K->dJ.Alloc(inverseBind.size())) || (r = K->dInfluences.Upload(newSkin->influences, newSkin->num_influences))) return r;
    }
    std::unique_ptr<zr_scene::Morph> M;
    if (newMorph)
    {
        const zr_morph_desc* d = newMorph;
        M.reset(new zr_scene::Morph());
        M->numWeights = numWeights;
        std::vector<uint32_t> trackOfWeight;
        for (uint32_t i = 0; i < d->num_tracks; i++) trackOfWeight.insert(trackOfWeight.end(), d->tracks[i].num_targets, i);
        if ((r = M->dTracks.Upload(d->tracks, d->num_tracks)) || (r = M->dTargets.Upload(d->targets, d->num_targets)) ||
            (r = M->dTrackOfWeight.Upload(trackOfWeight.data(), trackOfWeight.size())) || (r = M->dWeightFirst.Upload(weightFirst.data(), weightFirst.size())) ||
            (r = M->dTimes.Upload(d->times, d->num_times)) || (r = M->dValues.Upload(d->values, d->num_values)) || (r = M->dRestWeights.Upload(d->rest_weights, d->num_rest_weights)) ||
            (r = M->dDeltas.Upload(d->deltas, 3 * (size_t)d->num_deltas)) || (r = M->dWeights.Alloc(M->numWeights))) return r;
    }
    // nothing of the scene has changed up to here.  The rest pose back into the ranges of a set that goes or is replaced, and their hit-table entries (a
    // skin-only range of a skin set that stays keeps its last pose: the next animate writes it)
    const uint32_t going = keepSkin ? zr::kPoseMorph : zr::kPoseSkin | zr::kPoseMorph;
    for (const zr::PoseRange& o : O.ranges)
    {
        if (!(o.kind & going)) continue;
        HIP_TRY(hipMemcpy(s->vertices.p + o.firstVertex, O.hRest.data() + o.restFirst, (size_t)o.numVertices * sizeof(zr_vertex), hipMemcpyHostToDevice));
        if ((r = SceneFillVtxTables(s, nullptr, o.firstVertex, o.numVertices))) return r;
    }
    // ... and the saved records of the lights with a vertex in such a range, both buffers, run of consecutive triangles after run
    for (size_t j = 0; j < O.lights.size();)
    {
        auto goes = [&](const zr::LightEntry& e) { return inRanges(O.ranges, going, e.v0) || inRanges(O.ranges, going, e.v1) || inRanges(O.ranges, going, e.v2); };
        if (!goes(O.lights[j])) { j++; continue; }
        size_t e = j + 1;
        while (e < O.lights.size() && O.lights[e].tri == O.lights[e - 1].tri + 1 && goes(O.lights[e])) e++;
        HIP_TRY(hipMemcpy(s->objectEmissives.p + O.lights[j].tri, O.hLightObject.data() + j, (e - j) * sizeof(zr_emissive_triangle), hipMemcpyHostToDevice));
        // the world record: the saved one while the owner stands where it stood when the record was saved (the very bytes, the loader's identity-matrix
        // shortcut among them); the moved-light rule on the saved object record where an animation has moved the owner since
        std::vector<zr_emissive_triangle> world(O.hLightWorld.begin() + j, O.hLightWorld.begin() + e);
        for (size_t q = j; q < e; q++)
        {
            const float* M = s->hToWorld.data() + 12 * (size_t)O.lightOwner[q];
            if (std::memcmp(M, O.hLightXf.data() + 12 * q, 12 * sizeof(float))) zrsm::EmissiveToWorld(O.hLightObject[q], M, world[q - j]);
        }
        HIP_TRY(hipMemcpy(s->emissives.p + O.lights[j].tri, world.data(), (e - j) * sizeof(zr_emissive_triangle), hipMemcpyHostToDevice));
        j = e;
    }
    HIP_TRY(hipDeviceSynchronize());
    if (!keepSkin) s->skin = std::move(K);
    s->morph = std::move(M);
    s->pose.ranges.swap(P.ranges); s->pose.hRest.swap(P.hRest); s->pose.dRest.Swap(P.dRest);
    s->pose.lights.swap(P.lights); s->pose.hLightObject.swap(P.hLightObject); s->pose.hLightWorld.swap(P.hLightWorld); s->pose.dLights.Swap(P.dLights);
    s->pose.lightOwner.swap(P.lightOwner); s->pose.hLightXf.swap(P.hLightXf);
    return ZR_OK;
}
// ---- keyframe animation: the tables once (zr_scene_set_animation), then one float per frame (zr_scene_animate_async)
int zr_scene_set_animation(zr_scene* s, const zr_anim_desc* d)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_animation: null scene");
    HIP_TRY(hipSetDevice(s->device));
    if (!d || (!d->num_nodes && !d->num_instances))
    {
        if (int r = ScenePoseRebuild(s, false, nullptr, nullptr)) return r;      // (a skin set and a morph set go with the animation they were set on: the joints are nodes of the table that goes)
        SceneAnimSyncHost(s);
        HIP_TRY(hipDeviceSynchronize());      // an animate in flight still reads the tables
        std::lock_guard<std::mutex> lock(s->animMtx);
        s->anim.reset();
        return ZR_OK;
    }
    const uint32_t n = (uint32_t)s->cur.instances.n;
    std::vector<uint32_t> level(d->num_nodes);
    char msg[256];
    if (zran::ValidateAnimation(*d, n, level.data(), msg, sizeof(msg))) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_animation: %s", msg);
    std::unique_ptr<zr_scene::Anim> A(new zr_scene::Anim());
    if (int r = SceneDirtyLights(s, "zr_scene_set_animation", d->instance_idx, d->num_instances, &A->emFirst, &A->emEnd)) return r;
    A->nodes.assign(d->nodes, d->nodes + d->num_nodes); A->keys.assign(d->keys, d->keys + d->num_keys);
    A->instIdx.assign(d->instance_idx, d->instance_idx + d->num_instances); A->instNode.assign(d->instance_node, d->instance_node + d->num_instances);
    A->desc.nodes = A->nodes.data(); A->desc.num_nodes = d->num_nodes; A->desc.keys = A->keys.data(); A->desc.num_keys = d->num_keys;
    A->desc.instance_idx = A->instIdx.data(); A->desc.instance_node = A->instNode.data(); A->desc.num_instances = d->num_instances;
    // the nodes grouped by level, top level first, table order within a level; the animated nodes; the local matrices of the others
    uint32_t numLevels = 0;
    for (uint32_t l : level) numLevels = std::max(numLevels, l + 1);
    A->levelOffsets.assign(numLevels + 1, 0);
    for (uint32_t l : level) A->levelOffsets[l + 1]++;
    for (uint32_t l = 0; l < numLevels; l++) A->levelOffsets[l + 1] += A->levelOffsets[l];
    std::vector<uint32_t> levelNodes(d->num_nodes), fill(A->levelOffsets.begin(), A->levelOffsets.end()), animatedNodes;
    std::vector<float> local(12 * (size_t)d->num_nodes, 0.0f);
    for (uint32_t i = 0; i < d->num_nodes; i++)
    {
        levelNodes[fill[level[i]]++] = i;
        if (A->nodes[i].num_keys) animatedNodes.push_back(i);
        else zran::NodeLocal(A->nodes[i], A->keys.data(), 0.0f, local.data() + 12 * (size_t)i);
    }
    A->nAnimated = (uint32_t)animatedNodes.size();
    std::vector<uint32_t> movedInit(13 * (size_t)d->num_instances, 0u);
    std::copy(A->instIdx.begin(), A->instIdx.end(), movedInit.begin() + 12 * (size_t)d->num_instances);
    int r;
    if ((r = A->dNodes.Upload(A->nodes.data(), A->nodes.size())) || (r = A->dKeys.Upload(A->keys.data(), A->keys.size())) ||
        (r = A->dAnimated.Upload(animatedNodes.data(), animatedNodes.size())) || (r = A->dLevelNodes.Upload(levelNodes.data(), levelNodes.size())) ||
        (r = A->dInstNode.Upload(A->instNode.data(), A->instNode.size())) || (r = A->dMoved.Upload(movedInit.data(), movedInit.size())) ||
        (r = A->dLocal.Upload(local.data(), local.size())) || (r = A->dWorld.Alloc(local.size()))) return r;
    // nothing of the scene has changed up to here.  The animation it replaces: its last frame reaches the host's matrices, its kernels finish
    SceneAnimSyncHost(s);
    HIP_TRY(hipDeviceSynchronize());
    if ((r = ScenePoseRebuild(s, false, nullptr, nullptr))) return r;      // a skin set and a morph set belong to the animation they were set on: the joints index the table this call replaces
    for (uint32_t i : A->instIdx) s->movedEver[i] = 1;      // the background builder gives each animated instance a subtree of its own
    std::lock_guard<std::mutex> lock(s->animMtx);
    s->anim = std::move(A);
    return ZR_OK;
}
int zr_scene_animate_async(zr_scene* s, void* stream, float t)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_animate: null scene");
    if (!s->anim) return Fail(ZR_ERR_NOT_INITIALIZED, "zr_scene_animate: no animation set (zr_scene_set_animation)");
    if (int r = RefuseRebuildMode("zr_scene_animate")) return r;
    HIP_TRY(hipSetDevice(s->device));
    return SceneRefitUpdate(s, (hipStream_t)stream, FrameUpdate{UpdateForm::Animated, nullptr, nullptr, s->anim->desc.num_instances, s->anim->emFirst, s->anim->emEnd, t});
}
int zr_scene_animate(zr_scene* s, float t) { return ThenWait(zr_scene_animate_async(s, nullptr, t)); }
int zr_scene_move_instances(zr_scene* s, const uint32_t* idx, const float* world_3x4, uint32_t n_moved) { return ThenWait(zr_scene_move_instances_async(s, nullptr, idx, world_3x4, n_moved)); }
int zr_scene_get_instances(const zr_scene* s, void* stream, int which, zr_mesh_instance* out, float* to_world_or_null, uint32_t n)
{
    if (!s || !out) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_instances: null argument");
    if (which != 0 && which != 1) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_instances: which = %d (0 current, 1 previous)", which);
    if (n != s->cur.instances.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_instances: %u instances, the scene has %zu", n, s->cur.instances.n);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    SceneAnimSyncHost(const_cast<zr_scene*>(s));
    const zr_mesh_instance* src; bool xfDev;
    { std::lock_guard<std::mutex> lock(s->mtx); src = (which == 1 && s->hasPrev ? s->prev : s->cur).instances.p; xfDev = s->toWorldDev && s->toWorld.n == 12 * (size_t)n; }
    HIP_TRY(hipMemcpy(out, src, (size_t)n * sizeof(zr_mesh_instance), hipMemcpyDeviceToHost));
    if (to_world_or_null)
    {   // the matrices live on the device from the first refit update on; before that the scene has only the host's
        if (xfDev) HIP_TRY(hipMemcpy(to_world_or_null, s->toWorld.p, 12 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        else std::memcpy(to_world_or_null, s->hToWorld.data(), 12 * (size_t)n * sizeof(float));
    }
    return ZR_OK;
}
int zr_scene_get_emissives(const zr_scene* s, void* stream, zr_emissive_triangle* out, uint32_t first, uint32_t count)
{
    if (!s || (!out && count)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_emissives: null argument");
    if ((uint64_t)first + count > s->emissives.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_emissives: [%u, %llu) exceeds the scene's %zu emissive triangles", first, (unsigned long long)first + count, s->emissives.n);
    if (!count) return ZR_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(out, s->emissives.p + first, (size_t)count * sizeof(zr_emissive_triangle), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_scene_has_skinning(const zr_scene* s) { return s && s->skin ? 1 : 0; }
// ---- deformed geometry: a vertex range replaced by the caller (the host form), or posed on the device by every zr_scene_animate (zr_scene_set_skinning)
int zr_scene_update_vertices_async(zr_scene* s, void* stream, uint32_t first, uint32_t count, const zr_vertex* vertices)
{
    if (!s || (!vertices && count)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_update_vertices: null argument");
    if ((uint64_t)first + count > s->vertices.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_update_vertices: [%u, %llu) exceeds the scene's %zu vertices", first, (unsigned long long)first + count, s->vertices.n);
    if (int r = RefuseRebuildMode("zr_scene_update_vertices")) return r;
    if (!count) return ZR_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    int r; zr_scene::StageSlot* t;
    if ((r = StageAcquire(s, (size_t)count * sizeof(zr_vertex), &t))) return r;
    memcpy(t->host, vertices, (size_t)count * sizeof(zr_vertex));
    if ((r = SceneWaitUsers(s, st))) return r;          // kernels of earlier frames on other streams may still read the old vertices
    HIP_TRY(hipMemcpyAsync(s->vertices.p + first, t->host, (size_t)count * sizeof(zr_vertex), hipMemcpyHostToDevice, st));
    if ((r = SceneFillVtxTables(s, st, first, count))) return r;
    if ((r = StageCommit(t, st))) return r;
    // the host's copy: a background build in flight reads it, so the range waits until its thread is done (no host wait here)
    if (s->bg.state.load(std::memory_order_acquire) == 1) s->hVertexPending.emplace_back(first, std::vector<zr_vertex>(vertices, vertices + count));
    else { SceneFlushVertexCopies(s); std::copy(vertices, vertices + count, s->hVertices.begin() + first); }
    s->bg.movedSinceBuild = true;
    return SceneMarkUpdated(s, st);
}
int zr_scene_update_vertices(zr_scene* s, uint32_t first, uint32_t count, const zr_vertex* v) { const int r = zr_scene_update_vertices_async(s, nullptr, first, count, v); return count ? ThenWait(r) : r; }
int zr_scene_get_vertices(const zr_scene* s, void* stream, zr_vertex* out, uint32_t first, uint32_t count)
{
    if (!s || (!out && count)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_vertices: null argument");
    if ((uint64_t)first + count > s->vertices.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_vertices: [%u, %llu) exceeds the scene's %zu vertices", first, (unsigned long long)first + count, s->vertices.n);
    if (!count) return ZR_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(out, s->vertices.p + first, (size_t)count * sizeof(zr_vertex), hipMemcpyDeviceToHost));
    return ZR_OK;
}
// ---- deformed lights, the range form: the caller has replaced vertices (zr_scene_update_vertices) and names the light triangles that use them
int zr_scene_refresh_emissives_async(zr_scene* s, void* stream, uint32_t first, uint32_t count)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_refresh_emissives: null scene");
    if ((uint64_t)first + count > s->emissives.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_refresh_emissives: [%u, %llu) exceeds the scene's %zu emissive triangles", first, (unsigned long long)first + count, s->emissives.n);
    if (s->emissives.n && !s->objectEmissives.p) return Fail(ZR_ERR_NOT_INITIALIZED, "zr_scene_refresh_emissives: call zr_scene_set_object_emissives first");
    if (int r = RefuseRebuildMode("zr_scene_refresh_emissives")) return r;
    if (!count) return ZR_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    int r;
    const size_t n = s->cur.instances.n, xfBytes = 12 * n * sizeof(float);
    const bool seed = !s->toWorldDev || s->toWorld.n != 12 * n;      // a scene no refit update has touched: the matrices are the host's alone
    zr_scene::StageSlot* t = nullptr;
    if (seed)
    {
        SceneAnimSyncHost(s);
        if ((r = StageAcquire(s, xfBytes, &t))) return r;
        memcpy(t->host, s->hToWorld.data(), xfBytes);
    }
    if ((r = SceneWaitUsers(s, st))) return r;          // renders of earlier frames on other streams may still sample the old records
    if (seed)
    {
        std::lock_guard<std::mutex> lock(s->mtx);
        if (s->toWorld.n != 12 * n && (r = s->toWorld.Alloc(12 * n))) return r;
        HIP_TRY(hipMemcpyAsync(s->toWorld.p, t->host, xfBytes, hipMemcpyHostToDevice, st));
        if ((r = StageCommit(t, st))) return r;
        s->toWorldDev = true;
    }
    hipError_t e = zr::LaunchRefreshEmissives(st, SceneRefreshBuffers(s), nullptr, first, count);
    if (e != hipSuccess) return Fail(ZR_ERR_HIP, "k_refresh_emissives failed: %s", hipGetErrorString(e));
    return SceneMarkUpdated(s, st);
}
int zr_scene_refresh_emissives(zr_scene* s, uint32_t first, uint32_t count) { const int r = zr_scene_refresh_emissives_async(s, nullptr, first, count); return count ? ThenWait(r) : r; }
int zr_scene_get_object_emissives(const zr_scene* s, void* stream, zr_emissive_triangle* out, uint32_t first, uint32_t count)
{
    if (!s || (!out && count)) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_object_emissives: null argument");
    if ((uint64_t)first + count > s->emissives.n) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_get_object_emissives: [%u, %llu) exceeds the scene's %zu emissive triangles", first, (unsigned long long)first + count, s->emissives.n);
    if (s->emissives.n && !s->objectEmissives.p) return Fail(ZR_ERR_NOT_INITIALIZED, "zr_scene_get_object_emissives: no object-space records (zr_scene_set_object_emissives)");
    if (!count) return ZR_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(out, s->objectEmissives.p + first, (size_t)count * sizeof(zr_emissive_triangle), hipMemcpyDeviceToHost));
    return ZR_OK;
}
int zr_scene_set_skinning(zr_scene* s, const zr_skin_desc* d)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_skinning: null scene");
    HIP_TRY(hipSetDevice(s->device));
    if (!d || (!d->num_joints && !d->num_ranges && !d->num_influences)) return ScenePoseRebuild(s, false, nullptr, nullptr);      // (a morph set is laid out against the skin set: it goes too)
    uint32_t animNodes = 0;
    {
        std::lock_guard<std::mutex> lock(s->animMtx);
        if (!s->anim) return Fail(ZR_ERR_NOT_INITIALIZED, "zr_scene_set_skinning: no animation set (zr_scene_set_animation): the joints are nodes of its table");
        animNodes = s->anim->desc.num_nodes;
    }
    char msg[256];
    if (zrsk::ValidateSkin(*d, animNodes, (uint32_t)s->vertices.n, msg, sizeof(msg))) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_skinning: %s", msg);
    return ScenePoseRebuild(s, false, d, nullptr);
}

// ---- morph targets: the tables once (zr_scene_set_morph), then every zr_scene_animate samples the weights and poses the ranges
int zr_scene_has_morph(const zr_scene* s) { return s && s->morph ? 1 : 0; }
int zr_scene_set_morph(zr_scene* s, const zr_morph_desc* d)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_morph: null scene");
    HIP_TRY(hipSetDevice(s->device));
    if (!d || (!d->num_tracks && !d->num_targets && !d->num_ranges)) return ScenePoseRebuild(s, true, nullptr, nullptr);
    {
        std::lock_guard<std::mutex> lock(s->animMtx);
        if (!s->anim) return Fail(ZR_ERR_NOT_INITIALIZED, "zr_scene_set_morph: no animation set (zr_scene_set_animation): zr_scene_animate owns the frame's time");
    }
    zr_skin_desc skinDesc{};      // the skin set's ranges: all the check needs of it
    if (s->skin) { skinDesc.ranges = s->skin->ranges.data(); skinDesc.num_ranges = (uint32_t)s->skin->ranges.size(); }
    char msg[256];
    if (zrmo::ValidateMorph(*d, s->skin ? &skinDesc : nullptr, (uint32_t)s->vertices.n, msg, sizeof(msg))) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_morph: %s", msg);
    return ScenePoseRebuild(s, true, nullptr, d);
}

int zr_wire_layout(char* buf, size_t cap)
{
    std::string s;
    char line[160];
#define ZR_L_SIZE(name, T) do { snprintf(line, sizeof(line), name " %zu\n", sizeof(T)); s += line; } while (0)
#define ZR_L_FIELD(name, T, f) do { snprintf(line, sizeof(line), name " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f)); s += line; } while (0)
    ZR_L_SIZE("Vertex", zr_vertex); ZR_L_FIELD("Vertex.Position", zr_vertex, pos); ZR_L_FIELD("Vertex.TexUV", zr_vertex, uv);
    ZR_L_FIELD("Vertex.Normal", zr_vertex, normal); ZR_L_FIELD("Vertex.Tangent", zr_vertex, tangent);
    ZR_L_SIZE("MeshInstance", zr_mesh_instance);
    ZR_L_FIELD("MeshInstance.BaseVtxOffset", zr_mesh_instance, base_vtx_offset); ZR_L_FIELD("MeshInstance.BaseIdxOffset", zr_mesh_instance, base_idx_offset);
    ZR_L_FIELD("MeshInstance.Rotation", zr_mesh_instance, rotation); ZR_L_FIELD("MeshInstance.Scale", zr_mesh_instance, scale);
    ZR_L_FIELD("MeshInstance.MatIdx", zr_mesh_instance, mat_idx); ZR_L_FIELD("MeshInstance.BaseEmissiveTriOffset", zr_mesh_instance, base_emissive_tri_offset);
    ZR_L_FIELD("MeshInstance.Translation", zr_mesh_instance, translation); ZR_L_FIELD("MeshInstance.PrevRotation", zr_mesh_instance, prev_rotation);
    ZR_L_FIELD("MeshInstance.PrevScale", zr_mesh_instance, prev_scale); ZR_L_FIELD("MeshInstance.dTranslation", zr_mesh_instance, d_translation);
    ZR_L_FIELD("MeshInstance.BaseColorTex", zr_mesh_instance, base_color_tex); ZR_L_FIELD("MeshInstance.AlphaFactor_Cutoff", zr_mesh_instance, alpha_factor_cutoff);
    ZR_L_SIZE("EmissiveTriangle", zr_emissive_triangle);
    ZR_L_FIELD("EmissiveTriangle.Vtx0", zr_emissive_triangle, vtx0); ZR_L_FIELD("EmissiveTriangle.V0V1", zr_emissive_triangle, v0v1);
    ZR_L_FIELD("EmissiveTriangle.V0V2", zr_emissive_triangle, v0v2); ZR_L_FIELD("EmissiveTriangle.EdgeLengths", zr_emissive_triangle, edge_lengths);
    ZR_L_FIELD("EmissiveTriangle.ID", zr_emissive_triangle, id); ZR_L_FIELD("EmissiveTriangle.PackedA", zr_emissive_triangle, packed_a);
    ZR_L_FIELD("EmissiveTriangle.PackedB", zr_emissive_triangle, packed_b); ZR_L_FIELD("EmissiveTriangle.UV0", zr_emissive_triangle, uv0);
    ZR_L_FIELD("EmissiveTriangle.UV1", zr_emissive_triangle, uv1); ZR_L_FIELD("EmissiveTriangle.UV2", zr_emissive_triangle, uv2);
    ZR_L_SIZE("EmissiveLumenAliasTableEntry", zr_alias_entry);
    ZR_L_FIELD("EmissiveLumenAliasTableEntry.CachedP_Orig", zr_alias_entry, cached_p_orig); ZR_L_FIELD("EmissiveLumenAliasTableEntry.CachedP_Alias", zr_alias_entry, cached_p_alias);
    ZR_L_FIELD("EmissiveLumenAliasTableEntry.P_Curr", zr_alias_entry, p_curr); ZR_L_FIELD("EmissiveLumenAliasTableEntry.Alias", zr_alias_entry, alias);
    ZR_L_SIZE("PresampledEmissiveTriangle", zr_presampled_tri);
    ZR_L_FIELD("PresampledEmissiveTriangle.pos", zr_presampled_tri, pos); ZR_L_FIELD("PresampledEmissiveTriangle.normal", zr_presampled_tri, normal);
    ZR_L_FIELD("PresampledEmissiveTriangle.pdf", zr_presampled_tri, pdf); ZR_L_FIELD("PresampledEmissiveTriangle.ID", zr_presampled_tri, id);
    ZR_L_FIELD("PresampledEmissiveTriangle.idx", zr_presampled_tri, idx); ZR_L_FIELD("PresampledEmissiveTriangle.bary", zr_presampled_tri, bary);
    ZR_L_FIELD("PresampledEmissiveTriangle.le", zr_presampled_tri, le); ZR_L_FIELD("PresampledEmissiveTriangle.twoSided", zr_presampled_tri, two_sided);
    ZR_L_SIZE("VoxelSample", zr_voxel_sample);
    ZR_L_FIELD("VoxelSample.pos", zr_voxel_sample, pos); ZR_L_FIELD("VoxelSample.normal", zr_voxel_sample, normal); ZR_L_FIELD("VoxelSample.pdf", zr_voxel_sample, pdf);
    ZR_L_FIELD("VoxelSample.ID", zr_voxel_sample, id); ZR_L_FIELD("VoxelSample.le", zr_voxel_sample, le); ZR_L_FIELD("VoxelSample.twoSided", zr_voxel_sample, two_sided);
    ZR_L_SIZE("Material", zr_material);
    ZR_L_FIELD("Material.BaseColorFactor", zr_material, base_color_factor); ZR_L_FIELD("Material.BaseColorTex_Subsurf_CoatWeight", zr_material, base_color_tex_subsurf_coat_weight);
    ZR_L_FIELD("Material.NormalTex_TrDepth", zr_material, normal_tex_tr_depth); ZR_L_FIELD("Material.MRTex_SpecRoughness_CoatRoughness", zr_material, mr_tex_spec_roughness_coat_roughness);
    ZR_L_FIELD("Material.EmissiveFactor_NormalScale", zr_material, emissive_factor_normal_scale); ZR_L_FIELD("Material.EmissiveStrength_IOR", zr_material, emissive_strength_ior);
    ZR_L_FIELD("Material.EmissiveTex_AlphaCutoff_CoatIOR", zr_material, emissive_tex_alpha_cutoff_coat_ior); ZR_L_FIELD("Material.CoatColor_Flags", zr_material, coat_color_flags);
    ZR_L_SIZE("cbFrameConstants", zr_frame_constants);
#define ZR_L_CB(ref, f) ZR_L_FIELD("cbFrameConstants." ref, zr_frame_constants, f)
    ZR_L_CB("CurrView", curr_view); ZR_L_CB("PrevView", prev_view); ZR_L_CB("CurrViewInv", curr_view_inv); ZR_L_CB("PrevViewInv", prev_view_inv);
    ZR_L_CB("CurrViewProj", curr_view_proj); ZR_L_CB("PrevViewProj", prev_view_proj); ZR_L_CB("CameraPos", camera_pos); ZR_L_CB("CameraNear", camera_near);
    ZR_L_CB("AspectRatio", aspect_ratio); ZR_L_CB("PixelSpreadAngle", pixel_spread_angle); ZR_L_CB("TanHalfFOV", tan_half_fov); ZR_L_CB("dt", dt);
    ZR_L_CB("FrameNum", frame_num); ZR_L_CB("CurrGBufferDescHeapOffset", curr_gbuffer_desc_heap_offset); ZR_L_CB("PrevGBufferDescHeapOffset", prev_gbuffer_desc_heap_offset);
    ZR_L_CB("BaseColorMapsDescHeapOffset", base_color_maps_desc_heap_offset); ZR_L_CB("NormalMapsDescHeapOffset", normal_maps_desc_heap_offset);
    ZR_L_CB("MetallicRoughnessMapsDescHeapOffset", metallic_roughness_maps_desc_heap_offset); ZR_L_CB("EmissiveMapsDescHeapOffset", emissive_maps_desc_heap_offset);
    ZR_L_CB("EnvMapDescHeapOffset", env_map_desc_heap_offset); ZR_L_CB("RenderWidth", render_width); ZR_L_CB("RenderHeight", render_height);
    ZR_L_CB("DisplayWidth", display_width); ZR_L_CB("DisplayHeight", display_height); ZR_L_CB("CurrCameraJitter", curr_camera_jitter); ZR_L_CB("PrevCameraJitter", prev_camera_jitter);
    ZR_L_CB("PlanetRadius", planet_radius); ZR_L_CB("SunCosAngularRadius", sun_cos_angular_radius); ZR_L_CB("SunSinAngularRadius", sun_sin_angular_radius); ZR_L_CB("pad", pad);
    ZR_L_CB("SunDir", sun_dir); ZR_L_CB("SunIlluminance", sun_illuminance); ZR_L_CB("RayleighSigmaSColor", rayleigh_sigma_s_color); ZR_L_CB("RayleighSigmaSScale", rayleigh_sigma_s_scale);
    ZR_L_CB("OzoneSigmaAColor", ozone_sigma_a_color); ZR_L_CB("OzoneSigmaAScale", ozone_sigma_a_scale); ZR_L_CB("MieSigmaS", mie_sigma_s); ZR_L_CB("MieSigmaA", mie_sigma_a);
    ZR_L_CB("AtmosphereAltitude", atmosphere_altitude); ZR_L_CB("g", g); ZR_L_CB("NumFramesCameraStatic", num_frames_camera_static); ZR_L_CB("CameraStatic", camera_static);
    ZR_L_CB("Accumulate", accumulate); ZR_L_CB("SunMoved", sun_moved); ZR_L_CB("CameraRayUVGradsScale", camera_ray_uv_grads_scale); ZR_L_CB("MipBias", mip_bias);
    ZR_L_CB("OneDivNumEmissiveTriangles", one_div_num_emissive_triangles); ZR_L_CB("NumEmissiveTriangles", num_emissive_triangles); ZR_L_CB("FocusDepth", focus_depth);
    ZR_L_CB("LensRadius", lens_radius); ZR_L_CB("DoF", dof); ZR_L_CB("pad2", pad2);
#undef ZR_L_CB
#undef ZR_L_FIELD
#undef ZR_L_SIZE
    if (!buf || s.size() + 1 > cap) return -(int)(s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}

int zr_scene_destroy(zr_scene* s) { delete s; return ZR_OK; }

int zr_scene_set_alias_table_async(zr_scene* s, void* stream, const zr_alias_entry* e, uint32_t n)
{
    if (!s || !e) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_set_alias_table: null argument");
    if (n != s->view.numEmissives) return Fail(ZR_ERR_INVALID_ARG, "alias table size %u != number of emissive triangles %u", n, s->view.numEmissives);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    int r; zr_scene::StageSlot* t;
    if (s->alias.n != n && (r = s->alias.Alloc(n))) return r;      // (re)allocation only when the light count changed: hipFree waits for the device
    if ((r = StageAcquire(s, (size_t)n * sizeof(zr_alias_entry), &t))) return r;
    memcpy(t->host, e, (size_t)n * sizeof(zr_alias_entry));
    if ((r = SceneWaitUsers(s, st))) return r;          // renders of earlier frames on other streams may still draw from the old table
    HIP_TRY(hipMemcpyAsync(s->alias.p, t->host, (size_t)n * sizeof(zr_alias_entry), hipMemcpyHostToDevice, st));
    if ((r = StageCommit(t, st))) return r;
    {
        std::lock_guard<std::mutex> lock(s->mtx);
        s->aliasHost.assign(e, e + n); s->aliasOnDevice = false;
        s->view.alias = s->alias.p;
    }
    return SceneMarkUpdated(s, st);
}
int zr_scene_set_alias_table(zr_scene* s, const zr_alias_entry* e, uint32_t n) { return ThenWait(zr_scene_set_alias_table_async(s, nullptr, e, n)); }

int zr_scene_get_alias_table(const zr_scene* s, zr_alias_entry* out, uint32_t n)
{
    if (!s || !out) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (s->aliasOnDevice)
    {   // a table built on the device has no host copy: a read-back for tests and tools, behind everything enqueued so far
        if (n != s->alias.n) return Fail(ZR_ERR_INVALID_ARG, "alias table has %zu entries", s->alias.n);
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, s->alias.p, n * sizeof(zr_alias_entry), hipMemcpyDeviceToHost));
        return ZR_OK;
    }
    if (n != s->aliasHost.size()) return Fail(ZR_ERR_INVALID_ARG, "alias table has %zu entries", s->aliasHost.size());
    memcpy(out, s->aliasHost.data(), n * sizeof(zr_alias_entry));
    return ZR_OK;
}
// the kernels of ZR_ALIAS_BUILD_DEVICE on caller buffers; waits for `stream` (the scratch words are the call's own)
int zr_alias_table_build_device(int device, void* stream, const float* d_power, uint32_t n, zr_alias_entry* d_out)
{
    if (!d_power || !d_out || n == 0) return Fail(ZR_ERR_INVALID_ARG, "zr_alias_table_build_device: null/empty input");
    if (hipSetDevice(device) != hipSuccess) return Fail(ZR_ERR_NO_DEVICE, "zr_alias_table_build_device: no usable HIP device %d", device);
    DevBuf<uint64_t> scratch;
    if (int r = scratch.Alloc(zr::AliasScratchWords(n))) return r;
    HIP_TRY(zr::LaunchAliasBuild((hipStream_t)stream, d_power, n, d_out, scratch.p));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return ZR_OK;
}

int zr_scene_get_light_voxel_grid(const zr_scene* s, void* stream, zr_voxel_sample* out, uint32_t n)
{
    if (!s || !out) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (!s->view.lvg) return Fail(ZR_ERR_NOT_INITIALIZED, "no light voxel grid: render the PRELIGHTING pass with use_lvg first");
    if (n != s->lvg.n) return Fail(ZR_ERR_INVALID_ARG, "the light voxel grid has %zu samples", s->lvg.n);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(out, s->lvg.p, (size_t)n * sizeof(zr_voxel_sample), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_scene_get_presampled_sets(const zr_scene* s, void* stream, zr_presampled_tri* out, uint32_t n)
{
    if (!s || !out) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (!s->view.sampleSets) return Fail(ZR_ERR_NOT_INITIALIZED, "no presampled light sets: render the PRELIGHTING pass with presampling first");
    if (n != s->sampleSets.n) return Fail(ZR_ERR_INVALID_ARG, "the presampled sets hold %zu samples", s->sampleSets.n);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(out, s->sampleSets.p, (size_t)n * sizeof(zr_presampled_tri), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_scene_bvh_info(const zr_scene* s, uint32_t* num_nodes, uint32_t* num_tris, uint32_t* max_depth)
{
    if (!s) return Fail(ZR_ERR_INVALID_ARG, "null scene");
    if (num_nodes) *num_nodes = s->view.numNodes;
    if (num_tris) *num_tris = s->view.numTris;
    if (max_depth) *max_depth = s->maxDepth;
    return ZR_OK;
}

int zr_gbuffer_create(int device, uint32_t w, uint32_t h, zr_gbuffer** out)
{
    if (!out || !w || !h) return Fail(ZR_ERR_INVALID_ARG, "zr_gbuffer_create: bad argument");
    int r = RequireDevice(device);
    if (r) return r;
    zr_gbuffer* g = new (std::nothrow) zr_gbuffer();
    if (!g) return Fail(ZR_ERR_OOM, "out of host memory");
    g->device = device; g->w = w; g->h = h;
    for (int k = 0; k < 2; k++)
    for (int i = 0; i < ZR_GB_COUNT; i++)
        if ((r = g->planeSets[k][i].AllocZero((size_t)w * h * ZR_GB_PLANE_BYTES[i]))) { delete g; return r; }
    { hipError_t e = hipDeviceSynchronize(); if (e != hipSuccess) { delete g; return Fail(ZR_ERR_HIP, "hipDeviceSynchronize failed: %s", hipGetErrorString(e)); } }   // see zr_pass_init
    { std::lock_guard<std::mutex> lk(g_liveGBuffersMtx); g->uid = ++g_gbufferUid; g_liveGBuffers[g] = g->uid; }
    *out = g;
    return ZR_OK;
}
int zr_gbuffer_destroy(zr_gbuffer* g)
{
    { std::lock_guard<std::mutex> lk(g_liveGBuffersMtx); g_liveGBuffers.erase(g); }
    delete g;
    return ZR_OK;
}
int zr_gbuffer_set_tile_origin(zr_gbuffer* g, uint32_t x0, uint32_t y0)
{
    if (!g) return Fail(ZR_ERR_INVALID_ARG, "null gbuffer");
    if ((x0 & 31u) || (y0 & 31u)) return Fail(ZR_ERR_INVALID_ARG, "tile origin must be 32-pixel aligned");
    g->x0 = x0; g->y0 = y0;
    return ZR_OK;
}

int zr_gbuffer_download(const zr_gbuffer* g, void* stream, zr_gbuffer_planes* hp)
{
    if (!g || !hp) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (hp->width != g->w || hp->height != g->h) return Fail(ZR_ERR_INVALID_ARG, "plane size mismatch");
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < ZR_GB_COUNT; i++)
        if (hp->plane[i]) HIP_TRY(hipMemcpy(hp->plane[i], g->Planes()[i].p, g->Planes()[i].n, hipMemcpyDeviceToHost));
    return ZR_OK;
}
int zr_gbuffer_device_plane(const zr_gbuffer* g, int plane, void** dev)
{
    if (!g || !dev || plane < 0 || plane >= ZR_GB_COUNT) return Fail(ZR_ERR_INVALID_ARG, "bad argument");
    *dev = g->Planes()[plane].p;
    return ZR_OK;
}

int zr_pass_create(int kind, int device, zr_pass** out)
{
    if (!out) return Fail(ZR_ERR_INVALID_ARG, "null out");
    if (kind < ZR_PASS_GBUFFER || kind > ZR_PASS_DENOISE) return Fail(ZR_ERR_INVALID_ARG, "unknown pass kind %d", kind);
    int r = RequireDevice(device);
    if (r) return r;
    zr_pass* p = new (std::nothrow) zr_pass();
    if (!p) return Fail(ZR_ERR_OOM, "out of host memory");
    p->kind = kind; p->device = device;
    zr_params_default(&p->params);
    if (kind == ZR_PASS_DI_SKY)
    {
        // SkyDI.cpp:81-82, SkyDI.h:86-92: M_max (Sky) 15 -> m_max_temporal, M_max (Sun) 3 -> m_max_spatial, Alpha_min = 0.35^2
        p->params.flags = ZR_IND_TEMPORAL_RESAMPLE | ZR_IND_SPATIAL_RESAMPLE;
        p->params.m_max_temporal = 15; p->params.m_max_spatial = 3; p->params.alpha_min = 0.35f * 0.35f;
    }
    if (kind == ZR_PASS_DI_EMISSIVE)
    {
        // DirectLighting.cpp:100-107, DirectLighting.h:93-98
        p->params.flags = ZR_IND_TEMPORAL_RESAMPLE | ZR_IND_SPATIAL_RESAMPLE | ZR_DI_STOCHASTIC_SPATIAL | ZR_DI_EXTRA_DISOCCLUSION_SAMPLING;
        p->params.m_max_temporal = 20; p->params.m_max_spatial = 20; p->params.alpha_min = 0.05f * 0.05f;
    }
    *out = p;
    return ZR_OK;
}

// the planes frame overlap adds to a ReSTIR PT pass (zr_pass_set_frame_overlap): a third reservoir set, a second target plane, a second and a third FINAL
// plane (FINAL rotates over three: zr_pass_get_output(ZR_OUT_FINAL) changes from frame to frame, callers re-query it).  All of them or none: after a
// failure part-way nothing stays allocated, so res[2].A.p != nullptr means "the overlap planes exist" (the guard of zr_pass_set_frame_overlap).
static int AllocOverlapPlanes(zr_pass* p)
{
    const size_t cap = (size_t)p->w * p->h;
    int r;
    if ((r = PlanesAllocZero(p->res[2], cap)) || (r = p->rptTargetAlt.AllocZero(cap)) || (r = p->finalAlt.AllocZero(cap)) || (r = p->finalAlt2.AllocZero(cap)))
    {
        zr_pass::ResStorage::Each(p->res[2], [](auto& pl) { pl.Free(); return 0; });
        p->rptTargetAlt.Free(); p->finalAlt.Free(); p->finalAlt2.Free();
        return r;
    }
    return ZR_OK;
}
static int AllocPass(zr_pass* p)
{
    int r;
    const size_t cap = (size_t)p->w * p->h;
    p->hist.Rewind();      // every kind that keeps a history starts over (zr_pass_init / zr_pass_resize)
    if (p->kind == ZR_PASS_SKY) { if ((r = p->skyLut.Alloc(cap))) return r; }
    if (p->kind == ZR_PASS_TAA)
    {
        for (auto& t : p->taaOut) if ((r = t.AllocZero(cap))) return r;
        p->taaIdx = 0;
    }
    if (p->kind == ZR_PASS_DENOISE)
    {
        if ((r = p->svgfHist.AllocZero(cap)) || (r = p->svgfAccum.Alloc(cap)) || (r = p->svgfPing.AllocZero(cap)) || (r = p->svgfPong.AllocZero(cap)) || (r = p->svgfGuide.Alloc(cap)) || (r = p->svgfGuideFw.Alloc(cap))) return r;
        for (auto& m : p->svgfMoments) if ((r = m.AllocZero(cap))) return r;
        p->svgfMomIdx = 0; p->svgfOut = p->svgfPing.p; p->svgfCur = p->svgfPing.p;
    }
    if (p->kind == ZR_PASS_AUTO_EXPOSURE)
    {
        if ((r = p->aeHist.AllocZero(post::kHistBins)) || (r = p->aeExposure.AllocZero(2))) return r;      // TEXTURE_FLAGS::INIT_TO_ZERO, AutoExposure.cpp:150-155
    }
    if (p->kind == ZR_PASS_DISPLAY)
    {
        if ((r = p->displayOut.AllocZero(cap)) || (r = p->displaySrgb.AllocZero(cap))) return r;
    }
    if (p->kind == ZR_PASS_COMPOSITING)
    {
        if ((r = p->firstBOP.AllocZero(cap))) return r;            // scratch plane of the firefly filter (composited, unfiltered)
        if ((r = p->finalRGBA.AllocZero(cap))) return r;
    }
    if (p->kind == ZR_PASS_DI_SKY)
    {
        if ((r = p->finalRGBA.AllocZero(cap))) return r;
        if ((r = p->counters.AllocZero(2 * kCounterSlots))) return r;
        for (auto& set : p->sky) if ((r = PlanesAllocZero(set, cap))) return r;
        if ((r = p->diTarget.AllocZero(cap))) return r;
    }
    if (p->kind == ZR_PASS_DI_EMISSIVE)
    {
        if ((r = p->finalRGBA.AllocZero(cap))) return r;
        if ((r = p->counters.AllocZero(2 * kCounterSlots))) return r;
        for (auto& set : p->di) if ((r = PlanesAllocZero(set, cap))) return r;
        if ((r = p->diTarget.AllocZero(cap))) return r;
        if ((r = p->diSampleSet.Upload(kRdiSampleSet, 64))) return r;
    }
    if (p->kind == ZR_PASS_INDIRECT)
    {
        if ((r = p->q[0].Alloc(cap))) return r;
        if ((r = p->q[1].Alloc(cap))) return r;
        if ((r = p->finalRGBA.AllocZero(cap))) return r;
        if ((r = p->firstBOP.Alloc(cap))) return r;
        if ((r = p->counts.Alloc(5 * (kMaxRounds + 2) * kCounterStride))) return r;   // per round: live paths, k_trace cursor, 3 ray counts
        if ((r = p->counters.AllocZero(2 * kCounterSlots))) return r;
        if ((r = p->groupMax.Alloc((size_t)kMaxRounds * ((p->w + 7) / 8) * ((p->h + 7) / 8)))) return r;
        if (p->integrator == ZR_INTEGRATOR_RESTIR_GI) for (auto& set : p->gi) if ((r = PlanesAllocZero(set, cap))) return r;
        if (p->integrator == ZR_INTEGRATOR_RESTIR_PT)
        {
            for (int k = 0; k < 2; k++)
                if ((r = PlanesAllocZero(p->res[k], cap)) || (r = PlanesAllocZero(p->rb[k], cap))) return r;
            if ((r = p->rptTarget.AllocZero(cap))) return r;
            if ((r = p->rptNeighbor.AllocZero(cap))) return r;
            for (auto& m : p->rptMap) if ((r = m.AllocZero(cap))) return r;
            for (auto& q : p->rptPending) q.live = false;      // (the planes it would read and write are gone)
            if ((r = p->costMap.AllocZero((size_t)((p->w + 31u) / 32u + 1u) * ((p->h + 31u) / 32u + 1u)))) return r;
            if ((r = p->rptSampleSet.Upload(kRptSampleSet, 1024))) return r;
            if ((r = p->rptLists.Alloc(4 * cap))) return r;
            p->ov.Reset();
            if (p->ov.overlap) { if ((r = AllocOverlapPlanes(p))) return r; }
            // word layout (kRptListWords): [0, 1] temporal counts, [2, 3] first spatial round, [4, 5] the temporal replays' cursors (counts + 4 / + 5 of
            // base 0: the only DYNAMIC replay), [6, 7] second spatial round, [8 .. 11] = base 6's cursor slots -- unused (the spatial replays split
            // their lists statically) but allocated and zeroed, so that no base ever reaches past the buffer
            if ((r = p->rptListCounts.Alloc(kRptListWords))) return r;
        }
    }
    return ZR_OK;
}

int zr_pass_init(zr_pass* p, uint32_t w, uint32_t h, int integrator)
{
    if (!p || !w || !h) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_init: bad argument");
    if (p->kind == ZR_PASS_INDIRECT && (integrator < ZR_INTEGRATOR_PATH_TRACING || integrator > ZR_INTEGRATOR_RESTIR_PT))
        return Fail(ZR_ERR_INVALID_ARG, "unknown integrator %d", integrator);
    HIP_TRY(hipSetDevice(p->device));
    p->w = w; p->h = h; p->integrator = integrator;
    int r = AllocPass(p);
    if (r) return r;
    // the clears above are null-stream work and asynchronous to the host; a first render on a non-blocking stream must not overtake them
    HIP_TRY(hipDeviceSynchronize());
    p->initialized = true;
    return ZR_OK;
}
int zr_pass_resize(zr_pass* p, uint32_t w, uint32_t h)
{
    if (!p) return Fail(ZR_ERR_INVALID_ARG, "null pass");
    if (!p->initialized) return Fail(ZR_ERR_NOT_INITIALIZED, "pass not initialised");
    return zr_pass_init(p, w, h, p->integrator);
}
int zr_pass_reset_temporal(zr_pass* p)
{
    if (!p) return Fail(ZR_ERR_INVALID_ARG, "null pass");
    if (!p->initialized) return Fail(ZR_ERR_NOT_INITIALIZED, "pass not initialised");
    HIP_TRY(hipSetDevice(p->device));
    if (p->kind == ZR_PASS_INDIRECT) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipMemset(p->finalRGBA.p, 0, p->finalRGBA.n * sizeof(float))); if (p->finalAlt.p) { HIP_TRY(hipMemset(p->finalAlt.p, 0, p->finalAlt.n * sizeof(float))); HIP_TRY(hipMemset(p->finalAlt2.p, 0, p->finalAlt2.n * sizeof(float))); } }
    p->hist.Invalidate();       // IndirectLighting::ResetTemporal -> RESET_TEMPORAL_TEXTURES next frame
    if (p->kind == ZR_PASS_DI_EMISSIVE || p->kind == ZR_PASS_DI_SKY) { HIP_TRY(hipMemset(p->finalRGBA.p, 0, p->finalRGBA.n * sizeof(float))); p->hist.Rewind(); }   // DirectLighting.cpp:159-164, SkyDI.cpp:128-133
    HIP_TRY(hipDeviceSynchronize());      // a host call between frames: renders on non-blocking streams must see the cleared plane
    return ZR_OK;
}
int zr_pass_set_params(zr_pass* p, const zr_params* prm)
{
    if (!p || !prm) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (p->kind == ZR_PASS_DI_EMISSIVE && (prm->m_max_temporal < 1 || prm->m_max_temporal > 30)) return Fail(ZR_ERR_INVALID_ARG, "DI M_max must be in 1..30");
    if (p->kind == ZR_PASS_DI_SKY && (prm->m_max_temporal < 1 || prm->m_max_temporal > 15 || prm->m_max_spatial < 1 || prm->m_max_spatial > 15))
        return Fail(ZR_ERR_INVALID_ARG, "sky DI M_max (sky = m_max_temporal, sun = m_max_spatial) must be in 1..15");
    if (prm->use_lvg)
    {
        const uint32_t dx = prm->lvg_grid_dim & 1023u, dy = (prm->lvg_grid_dim >> 10) & 1023u, dz = (prm->lvg_grid_dim >> 20) & 1023u;
        if (!prm->presampling) return Fail(ZR_ERR_INVALID_ARG, "the light voxel grid needs light presampling (IndirectLighting.h:93)");
        if (!dx || !dy || !dz || !(prm->lvg_extents[0] > 0) || !(prm->lvg_extents[1] > 0) || !(prm->lvg_extents[2] > 0))
            return Fail(ZR_ERR_INVALID_ARG, "light voxel grid: dimension / extents must be positive");
    }
    if (prm->max_non_tr_bounces < 1 || prm->max_non_tr_bounces > 15 || prm->max_glossy_tr_bounces < 1 || prm->max_glossy_tr_bounces > 15)
        return Fail(ZR_ERR_INVALID_ARG, "bounce counts must be in 1..15");
    // the reservoir caps travel in 4-bit fields of cb_ReSTIR_PT_*::Packed (IndirectLighting.cpp:1260-1270: "M_max (Temporal)" 1..15, "M_max (Spatial)" 1..12)
    if (p->kind == ZR_PASS_INDIRECT && (prm->m_max_temporal < 1 || prm->m_max_temporal > 15 || prm->m_max_spatial < 1 || prm->m_max_spatial > 15))
        return Fail(ZR_ERR_INVALID_ARG, "indirect lighting: M_max (temporal %u, spatial %u) must be in 1..15", prm->m_max_temporal, prm->m_max_spatial);
    if (p->kind == ZR_PASS_DENOISE && (prm->svgf_iterations > 8u || prm->svgf_normal_power_log2 > 16u))
        return Fail(ZR_ERR_INVALID_ARG, "DENOISE: svgf_iterations must be <= 8, svgf_normal_power_log2 <= 16");
    if (p->kind == ZR_PASS_INDIRECT && prm->num_spatial_passes > 2u) return Fail(ZR_ERR_INVALID_ARG, "ReSTIR PT: num_spatial_passes must be 0, 1 or 2 (IndirectLighting.cpp:1238-1240)");
    if (prm->presampling && (prm->num_sample_sets == 0 || prm->sample_set_size == 0 || prm->num_sample_sets > 65535 || prm->sample_set_size > 65535))
        return Fail(ZR_ERR_INVALID_ARG, "presampling needs 1..65535 sample sets of 1..65535 samples");
    if (prm->tex_filter >= ZR_TEX_FILTER_COUNT) return Fail(ZR_ERR_INVALID_ARG, "tex_filter must be a ZR_TEX_FILTER_* value");
    p->params = *prm;
    return ZR_OK;
}

static int RenderGBuffer(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb)
{
    if (!gb) return Fail(ZR_ERR_INVALID_ARG, "GBUFFER pass needs a gbuffer");
    if (gb->x0 + gb->w > cb->render_width || gb->y0 + gb->h > cb->render_height) return Fail(ZR_ERR_INVALID_ARG, "gbuffer tile lies outside the render target of the frame constants");
    const uint32_t tilesX = (gb->w + 15) / 16, tilesY = (gb->h + 15) / 16;
    if (int wr = gb->AcquireWrite(gb->Next(), s)) return wr;     // (tracked G-buffers: the set about to be overwritten may still be read on another stream)
    gb->cur = gb->Next(); gb->numRendered++;
    gb->plainAt[gb->cur] = sc->plainMaterials.load(std::memory_order_relaxed); gb->sceneAt[gb->cur] = sc->uid; gb->renderAt[gb->cur] = gb->numRendered;
    TimerBegin(p, s, "gbuffer");
    uint32_t pickXY = 0xffffffffu;
    if (p->pickXY != 0xffffffffu)
    {
        // a pending pick: only a G-buffer (tile) that holds the pixel writes
        if (!p->pickBuf.p) { int r = p->pickBuf.Alloc(1); if (r) return r; }
        const uint32_t px = p->pickXY & 0xffffu, py = p->pickXY >> 16;
        if (px >= gb->x0 && px < gb->x0 + gb->w && py >= gb->y0 && py < gb->y0 + gb->h) { pickXY = p->pickXY; p->pickWritten = true; }
    }
    hipLaunchKernelGGL(k_gbuffer, dim3(tilesX * tilesY), dim3(kBlock), 0, s, FrameView(sc, cb), *cb, gb->View(), tilesX, pickXY, p->pickBuf.p);
    TimerEnd(p, s);
    HIP_TRY(hipGetLastError());
    p->hostCounters.n_closest += (uint64_t)gb->w * gb->h;
    return gb->MarkWritten(s);
}

// GBufferRT::PickPixel / ClearPick / GetPickReadbackBuffer (GBufferRT.h:36-46): every GBUFFER render while a pick is pending writes the mesh index under
// the pixel (GBufferRT_Inline.hlsl:241-242: hitMeshIdx, UINT32_MAX on a miss)
int zr_pass_pick_pixel(zr_pass* p, uint32_t x, uint32_t y)
{
    if (!p || p->kind != ZR_PASS_GBUFFER) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_pick_pixel: needs a GBUFFER pass");
    if (x >= 0xffffu || y >= 0xffffu) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_pick_pixel: pixel (%u, %u) out of range", x, y);      // (UINT16_MAX is the reference's "no pick")
    p->pickXY = x | (y << 16); p->pickWritten = false;
    return ZR_OK;
}
int zr_pass_clear_pick(zr_pass* p)
{
    if (!p || p->kind != ZR_PASS_GBUFFER) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_clear_pick: needs a GBUFFER pass");
    p->pickXY = 0xffffffffu;
    return ZR_OK;
}
int zr_pass_read_pick(zr_pass* p, void* stream, uint32_t* mesh_idx)
{
    if (!p || p->kind != ZR_PASS_GBUFFER || !mesh_idx) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_read_pick: needs a GBUFFER pass and an output");
    if (!p->pickWritten) return Fail(ZR_ERR_NOT_INITIALIZED, "zr_pass_read_pick: no G-buffer has been rendered over the picked pixel since zr_pass_pick_pixel");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(mesh_idx, p->pickBuf.p, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return ZR_OK;
}

// Sky::Render (Sky.cpp:120-164): K17 (ZR_STAGE_TEMPORAL), then bind the LUT to the scene; then, with inscattering enabled, the voxel grid
// (ZR_STAGE_SPATIAL: a caller that keeps the LUT -- it does not depend on the camera -- renders the grid alone every frame)
static int RenderSky(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, zr_scene* sc, int stages)
{
    if (stages & ZR_STAGE_TEMPORAL)
    {
        TimerBegin(p, s, "sky_view_lut");
        hipLaunchKernelGGL(k_sky_lut, dim3((p->w + 7) / 8, (p->h + 7) / 8), dim3(64), 0, s, *cb, p->w, p->h, p->skyLut.p);
        TimerEnd(p, s);
        HIP_TRY(hipGetLastError());
        { std::lock_guard<std::mutex> lock(sc->mtx); sc->view.sky.data = p->skyLut.p; sc->view.sky.w = p->w; sc->view.sky.h = p->h; }
    }
    if (p->inscatterOn && (stages & ZR_STAGE_SPATIAL))
    {
        if (!(stages & ZR_STAGE_TEMPORAL)) p->numTimers = 0;      // the grid alone is this pass's whole frame
        TimerBegin(p, s, "inscattering");
        const hipError_t e = LaunchInscattering(s, FrameView(sc, cb), *cb, p->inscatter, p->inscatterGrid.p);
        TimerEnd(p, s);
        if (e != hipSuccess) return Fail(ZR_ERR_HIP, "inscattering launch failed: %s", hipGetErrorString(e));
    }
    return ZR_OK;
}

// K3: PreLighting::Render presampling branch (PreLighting.cpp:369-411): every frame, seeded by FrameNum
static int RenderPresample(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, zr_scene* sc)
{
    const uint32_t total = p->params.num_sample_sets * p->params.sample_set_size;
    if (sc->sampleSets.n != total) { int r = sc->sampleSets.Alloc(total); if (r) return r; }
    {
        std::lock_guard<std::mutex> lock(sc->mtx);
        sc->numSampleSets = p->params.num_sample_sets;
        sc->view.sampleSets = sc->sampleSets.p; sc->view.sampleSetSize = p->params.sample_set_size;
    }
    TimerBegin(p, s, "presample_emissives");
    hipLaunchKernelGGL(k_presample, dim3((total + 63) / 64), dim3(64), 0, s, FrameView(sc, cb), total, cb->frame_num, sc->view.numEmissives, sc->sampleSets.p);
    TimerEnd(p, s);
    HIP_TRY(hipGetLastError());
    return ZR_OK;
}

// K4: PreLighting::Render light-voxel-grid branch (PreLighting.cpp:405-428): every frame (the grid follows the camera)
static int RenderLVG(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, zr_scene* sc)
{
    const zr_params& ip = p->params;
    const uint32_t dx = ip.lvg_grid_dim & 1023u, dy = (ip.lvg_grid_dim >> 10) & 1023u, dz = (ip.lvg_grid_dim >> 20) & 1023u;
    const size_t total = (size_t)dx * dy * dz * ZR_LVG_SAMPLES_PER_VOXEL;
    if (sc->lvg.n != total) { int r = sc->lvg.Alloc(total); if (r) return r; }
    TimerBegin(p, s, "build_lvg");
    hipLaunchKernelGGL(k_build_lvg, dim3(dx, dy, dz), dim3(64), 0, s, FrameView(sc, cb), *cb, dx, dy, dz, ip.lvg_extents[0], ip.lvg_extents[1], ip.lvg_extents[2],
        ip.lvg_offset_y, sc->lvg.p);
    TimerEnd(p, s);
    HIP_TRY(hipGetLastError());
    std::lock_guard<std::mutex> lock(sc->mtx);
    sc->view.lvg = sc->lvg.p; sc->view.lvgDim[0] = dx; sc->view.lvgDim[1] = dy; sc->view.lvgDim[2] = dz;
    for (int a = 0; a < 3; a++) sc->view.lvgExtents[a] = ip.lvg_extents[a];
    sc->view.lvgOffsetY = ip.lvg_offset_y;
    return ZR_OK;
}

static int RenderPreLightingInner(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, zr_scene* sc);
static int RenderPreLighting(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, zr_scene* sc)
{
    int r = RenderPreLightingInner(p, s, cb, sc);
    if (r || !p->params.use_lvg || sc->view.numEmissives == 0) return r;
    return RenderLVG(p, s, cb, sc);
}
// ZR_ALIAS_BUILD_DEVICE, no table or a stale one (either invalidate form): K2, then the table of include/zr_alias.h built by zr_tu_alias.hip, both
// ENQUEUED on the pass stream into the scene's table buffer, ahead of K3 / K4 and of this frame's sampling kernels.  Nothing is read back, nothing
// waits, no host build: the frame that finds the table stale samples the new one.  Ordering against other streams is that of
// zr_scene_set_alias_table_async -- behind the renders that may still draw from the buffer, and an `updated` event behind the build.  (A table
// buffer of a new size has no readers; the allocation itself is the one of the host path, once per emissive count.)
static int RenderAliasTableDevice(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, zr_scene* sc)
{
    const uint32_t n = sc->view.numEmissives;
    int r;
    p->powerPending = false;      // a deferred host rebuild in flight when the mode changed is dropped: its powers must not feed a later host build
    if (p->power.n != n && (r = p->power.Alloc(n))) return r;
    const size_t words = zr::AliasScratchWords(n);
    if (sc->aliasScratch.n != words && (r = sc->aliasScratch.Alloc(words))) return r;
    if (sc->alias.n != n) { if ((r = sc->alias.Alloc(n))) return r; }
    else if ((r = SceneWaitUsers(sc, s))) return r;
    TimerBegin(p, s, "estimate_power");
    hipLaunchKernelGGL(k_estimate_power, dim3((n + 255) / 256), dim3(256), 0, s, FrameView(sc, cb), n, p->power.p);
    TimerEnd(p, s);
    HIP_TRY(hipGetLastError());
    TimerBegin(p, s, "alias_build");
    HIP_TRY(zr::LaunchAliasBuild(s, p->power.p, n, sc->alias.p, sc->aliasScratch.p));
    TimerEnd(p, s);
    {
        std::lock_guard<std::mutex> lock(sc->mtx);
        sc->aliasHost.clear(); sc->aliasOnDevice = true; sc->aliasStale = false;
        sc->view.alias = sc->alias.p;
        if ((r = SceneMarkUpdatedLocked(sc, s))) return r;
    }
    return p->params.presampling ? RenderPresample(p, s, cb, sc) : ZR_OK;
}
static int RenderPreLightingInner(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, zr_scene* sc)
{
    const uint32_t n = sc->view.numEmissives;
    if (n == 0) return ZR_OK;
    if (sc->aliasBuild == ZR_ALIAS_BUILD_DEVICE && (!sc->view.alias || sc->aliasStale)) return RenderAliasTableDevice(p, s, cb, sc);
    // the alias table is built once per emissive set (EmissiveTriangleAliasTable is only re-run when emissive materials change):
    // zr_scene_invalidate_alias_table or a new scene forces a rebuild
    if (sc->view.alias && sc->aliasStale)
    {
        // deferred rebuild: (1) nothing in flight -> estimate the powers and start their read-back; (2) read-back finished -> build on the host and
        // enqueue the upload; either way this call only enqueues, and the bound table stays valid for this frame's sampling
        int r;
        if (!p->powerPending)
        {
            if (p->power.n != n && (r = p->power.Alloc(n))) return r;
            if (p->powerHostCap < n) { if (p->powerHost) (void)hipHostFree(p->powerHost); p->powerHost = nullptr; HIP_TRY(hipHostMalloc((void**)&p->powerHost, n * sizeof(float), hipHostMallocDefault)); p->powerHostCap = n; }
            if (!p->powerEv) HIP_TRY(hipEventCreateWithFlags(&p->powerEv, hipEventDisableTiming));
            hipLaunchKernelGGL(k_estimate_power, dim3((n + 255) / 256), dim3(256), 0, s, FrameView(sc, cb), n, p->power.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(p->powerHost, p->power.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipEventRecord(p->powerEv, s));
            p->powerPending = true;
        }
        else if (hipEventQuery(p->powerEv) == hipSuccess)
        {
            std::vector<float> power(p->powerHost, p->powerHost + n);
            std::vector<zr_alias_entry> table(n);
            BuildAliasTableHost(power, table.data(), 0);
            if ((r = zr_scene_set_alias_table_async(sc, s, table.data(), n))) return r;
            p->powerPending = false;
            std::lock_guard<std::mutex> lock(sc->mtx);
            sc->aliasStale = false;
        }
        return p->params.presampling ? RenderPresample(p, s, cb, sc) : ZR_OK;
    }
    if (sc->view.alias) return p->params.presampling ? RenderPresample(p, s, cb, sc) : ZR_OK;
    int r = p->power.Alloc(n);
    if (r) return r;
    TimerBegin(p, s, "estimate_power");
    hipLaunchKernelGGL(k_estimate_power, dim3((n + 255) / 256), dim3(256), 0, s, FrameView(sc, cb), n, p->power.p);
    TimerEnd(p, s);
    HIP_TRY(hipGetLastError());
    // EmissiveTriangleAliasTable::Render (PreLighting.cpp:512-585): read back, build on the host, upload
    std::vector<float> power(n);
    HIP_TRY(hipMemcpyAsync(power.data(), p->power.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<zr_alias_entry> table(n);
    BuildAliasTableHost(power, table.data(), 0);
    if ((r = zr_scene_set_alias_table_async(sc, s, table.data(), n))) return r;      // the upload is ordered on the pass stream, ahead of the sampling kernels
    return p->params.presampling ? RenderPresample(p, s, cb, sc) : ZR_OK;
}

// The rect of the G-buffer tile this pass shades (zr_pass_set_owned_rect; width 0 = the whole tile), validated once for every
// pass with cross-pixel reuse: inside the tile (planes are indexed relative to the tile origin), 32-px aligned origin (thread
// groups / RNG group ids coincide with the single-device run) and -- on a proper sub-rect of the frame -- an apron of >= 16 px
// wherever the frame continues (spatial / temporal-candidate search radius: 15 px ReSTIR PT, 16 px DI / sky DI / GI).
static int ResolveOwnedRect(const zr_pass* p, const zr_gbuffer* gb, const zr_frame_constants* cb, uint32_t* ox0, uint32_t* oy0, uint32_t* ow, uint32_t* oh)
{
    const uint32_t x0 = p->own[2] ? p->own[0] : gb->x0, y0 = p->own[2] ? p->own[1] : gb->y0;
    const uint32_t w = p->own[2] ? p->own[2] : gb->w, h = p->own[2] ? p->own[3] : gb->h;
    if (w == 0 || h == 0) return Fail(ZR_ERR_INVALID_ARG, "owned rect is empty");
    if (x0 < gb->x0 || y0 < gb->y0 || (uint64_t)x0 + w > (uint64_t)gb->x0 + gb->w || (uint64_t)y0 + h > (uint64_t)gb->y0 + gb->h)
        return Fail(ZR_ERR_INVALID_ARG, "owned rect lies outside the G-buffer tile");
    if ((x0 & 31u) || (y0 & 31u)) return Fail(ZR_ERR_INVALID_ARG, "owned rect origin must be 32-pixel aligned");
    const bool wholeFrame = x0 == 0 && y0 == 0 && w == cb->render_width && h == cb->render_height;
    if (!wholeFrame)
    {
        auto apronOk = [&](uint32_t lo, uint32_t olo, uint32_t hi, uint32_t ohi, uint32_t frame) {
            return (olo == 0 || olo - lo >= 16) && (ohi == frame || hi - ohi >= 16); };
        if (!apronOk(gb->x0, x0, gb->x0 + gb->w, x0 + w, cb->render_width) || !apronOk(gb->y0, y0, gb->y0 + gb->h, y0 + h, cb->render_height))
            return Fail(ZR_ERR_INVALID_ARG, "a pass with cross-pixel reuse on a screen tile needs a G-buffer apron of >= 16 px around the owned rect (zr_pass_set_owned_rect)");
    }
    *ox0 = x0; *oy0 = y0; *ow = w; *oh = h;
    return ZR_OK;
}

// DirectLighting::Render (DirectLighting.cpp:166-296)
static int RenderDirectEmissive(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb, int stages)
{
    using namespace rdi;
    if (!gb) return Fail(ZR_ERR_INVALID_ARG, "DI_EMISSIVE pass needs a gbuffer");
    if (gb->w != p->w || gb->h != p->h) return Fail(ZR_ERR_INVALID_ARG, "gbuffer / pass size mismatch");
    if (gb->x0 + gb->w > cb->render_width || gb->y0 + gb->h > cb->render_height) return Fail(ZR_ERR_INVALID_ARG, "gbuffer tile outside the render target");
    if (sc->view.numEmissives == 0) return Fail(ZR_ERR_INVALID_ARG, "DI_EMISSIVE needs emissive triangles");
    if (!sc->view.alias) return Fail(ZR_ERR_NOT_INITIALIZED, "emissive alias table missing: render the PRELIGHTING pass first");
    if (cb->num_emissive_triangles != sc->view.numEmissives) return Fail(ZR_ERR_INVALID_ARG, "cbFrameConstants.NumEmissiveTriangles != scene");
    const zr_params& ip = p->params;
    if (ip.presampling && (!sc->view.sampleSets || sc->numSampleSets != ip.num_sample_sets || sc->view.sampleSetSize != ip.sample_set_size))
        return Fail(ZR_ERR_NOT_INITIALIZED, "presampled light sets missing or of another size: render the PRELIGHTING pass with the same presampling params first");
    DiFrame F;
    F.sc = FrameView(sc, cb); F.gb = gb->View(); F.gbPrev = gb->PrevView();
    F.scPrev = FrameViewPrev(sc, cb);
    if (int orc = ResolveOwnedRect(p, gb, cb, &F.ox0, &F.oy0, &F.ow, &F.oh)) return orc;
    F.cur = p->di[p->hist.Cur()].View(); F.prev = p->di[p->hist.Oth()].View();
    F.target = p->diTarget.p; F.finalRGBA = p->finalRGBA.p; F.sampleSet = p->diSampleSet.p;
    const DiParams& prm = F.prm = zr::DiParamsOf(ip, *cb, p->hist.valid, gb->numRendered >= 2);
    const bool hvs = prm.halfVec != 0;      // the half-vector copy shift has kernel instantiations of its own
    const uint32_t tilesX = (F.ow + 15) / 16, tilesY = (F.oh + 15) / 16;
    const dim3 grid(tilesX * tilesY), block(kBlock);
    const bool plainDi = PlainClass(sc, gb);
    if (stages & ZR_STAGE_TEMPORAL)
    {
        TimerBegin(p, s, "rdi_temporal");
        hipLaunchKernelGGL(hvs ? (plainDi ? k_rdi_temporal<true, true> : k_rdi_temporal<false, true>) : (plainDi ? k_rdi_temporal<true, false> : k_rdi_temporal<false, false>), dim3(grid.x * (256 / kDiBlock)), dim3(kDiBlock), 0, s, F, *cb, tilesX, p->counters.p + 2 * 8);
        TimerEnd(p, s);
    }
    if (!(stages & ZR_STAGE_SPATIAL)) { HIP_TRY(hipGetLastError()); return ZR_OK; }
    if (prm.doSpatial)
    {
        TimerBegin(p, s, "rdi_spatial");
        hipLaunchKernelGGL(hvs ? (plainDi ? k_rdi_spatial<true, true> : k_rdi_spatial<false, true>) : (plainDi ? k_rdi_spatial<true, false> : k_rdi_spatial<false, false>), dim3(grid.x * (256 / kDiBlock)), dim3(kDiBlock), 0, s, F, *cb, tilesX, p->counters.p + 2 * 9);
        TimerEnd(p, s);
    }
    HIP_TRY(hipGetLastError());
    p->hist.Flip();
    return ZR_OK;
}

// SkyDI::Render (SkyDI.cpp:135-259)
static int RenderDirectSky(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb, int stages)
{
    using namespace sdi;
    if (!gb) return Fail(ZR_ERR_INVALID_ARG, "DI_SKY pass needs a gbuffer");
    if (gb->w != p->w || gb->h != p->h) return Fail(ZR_ERR_INVALID_ARG, "gbuffer / pass size mismatch");
    if (gb->x0 + gb->w > cb->render_width || gb->y0 + gb->h > cb->render_height) return Fail(ZR_ERR_INVALID_ARG, "gbuffer tile outside the render target");
    if (!sc->view.sky.data) return Fail(ZR_ERR_NOT_INITIALIZED, "sky-view LUT missing: render a ZR_PASS_SKY pass first");
    const zr_params& ip = p->params;
    SkyFrame F;
    F.sc = FrameView(sc, cb); F.gb = gb->View(); F.gbPrev = gb->PrevView();
    F.scPrev = FrameViewPrev(sc, cb);
    if (int orc = ResolveOwnedRect(p, gb, cb, &F.ox0, &F.oy0, &F.ow, &F.oh)) return orc;
    F.cur = p->sky[p->hist.Cur()].View(); F.prev = p->sky[p->hist.Oth()].View();
    F.target = p->diTarget.p; F.finalRGBA = p->finalRGBA.p;
    const SkyParams& prm = F.prm = zr::SkyParamsOf(ip, *cb, p->hist.valid, gb->numRendered >= 2);
    const uint32_t tilesX = (F.ow + 15) / 16, tilesY = (F.oh + 15) / 16;
    const dim3 grid(tilesX * tilesY), block(kBlock);
    const bool plainDi = PlainClass(sc, gb);
    if (stages & ZR_STAGE_TEMPORAL)
    {
        TimerBegin(p, s, "sdi_temporal");
        hipLaunchKernelGGL(plainDi ? k_sdi_temporal<true> : k_sdi_temporal<false>, dim3(grid.x * (256 / kSdiBlock)), dim3(kSdiBlock), 0, s, F, *cb, tilesX, p->counters.p + 2 * 11);
        TimerEnd(p, s);
    }
    if (!(stages & ZR_STAGE_SPATIAL)) { HIP_TRY(hipGetLastError()); return ZR_OK; }
    if (prm.doSpatial)
    {
        TimerBegin(p, s, "sdi_spatial");
        hipLaunchKernelGGL(plainDi ? k_sdi_spatial<true> : k_sdi_spatial<false>, dim3(grid.x * (256 / kSdiBlock)), dim3(kSdiBlock), 0, s, F, *cb, tilesX, p->counters.p + 2 * 12);
        TimerEnd(p, s);
    }
    HIP_TRY(hipGetLastError());
    p->hist.Flip();
    return ZR_OK;
}

// IndirectLighting::RenderReSTIR_GI (IndirectLighting.cpp:277-368) + the Render() tail (:1006-1025).  ZR_STAGE_TEMPORAL: k_rgi (the reference's whole pass);
// ZR_STAGE_SPATIAL: k_rgi_spatial when zr_pass_set_rgi_spatial has switched it on (zr_rgi_spatial.h; no reference counterpart), else nothing.  The reservoir
// sets flip at the end of the TEMPORAL stage, so between the stages -- as after the frame -- the set k_rgi wrote is gi[hist.Oth()]: the set ZR_HALO_FINAL moves.
static int RenderReSTIR_GI(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb, int stages)
{
    using namespace rgi;
    const zr_params& ip = p->params;
    GiFrame F;
    F.sc = FrameView(sc, cb); F.gb = gb->View(); F.gbPrev = gb->PrevView();
    F.sc.texFilter = ip.tex_filter;
    if (int orc = ResolveOwnedRect(p, gb, cb, &F.ox0, &F.oy0, &F.ow, &F.oh)) return orc;
    GiParams& prm = F.prm = zr::GiParamsOf(ip, *cb, p->hist.valid, gb->numRendered >= 2, sc->view.tex.count != 0);
    const uint32_t tilesX = (F.ow + 15) / 16, tilesY = (F.oh + 15) / 16;
    if (stages & ZR_STAGE_TEMPORAL)
    {
        p->rgiSpatialFrame = p->rgiSpatial;
        const bool spatial = p->rgiSpatialFrame.numSamples != 0;
        F.cur = p->gi[p->hist.Cur()].View(); F.prev = p->gi[p->hist.Oth()].View();
        F.finalRGBA = p->finalRGBA.p;
        if (spatial)
        {   // FINAL gets one contribution per pixel and frame, from the spatial stage: k_rgi's own radiance is stored (never accumulated) in a scratch plane,
            // and it writes the set the spatial kernel reads every frame
            const size_t cap = (size_t)p->w * p->h;
            if (p->rgiScratch.Pixels() != cap) { int r; if ((r = p->rgiScratch.Alloc(cap))) return r; HIP_TRY(hipMemsetAsync(p->rgiScratch.p, 0, cap * p->rgiScratch.bpp, s)); }
            F.finalRGBA = p->rgiScratch.p; prm.accumulate = 0u; prm.writeReservoirs = 1u;
        }
        if (prm.useLVG && !sc->view.lvg) return Fail(ZR_ERR_NOT_INITIALIZED, "light voxel grid missing: render the PRELIGHTING pass with use_lvg first");
        TimerBegin(p, s, "rgi");
        hipLaunchKernelGGL(sc->view.tex.count ? k_rgi_tex : PlainClass(sc, gb) ? k_rgi<true> : k_rgi<false>, dim3(tilesX * tilesY * (256 / kRgiBlock)), dim3(kRgiBlock), 0, s, F, *cb, tilesX, p->counters.p + 2 * 10);
        TimerEnd(p, s);
        HIP_TRY(hipGetLastError());
        p->hist.Flip();
    }
    if ((stages & ZR_STAGE_SPATIAL) && p->rgiSpatialFrame.numSamples != 0)
    {
        if (!p->hist.valid) return Fail(ZR_ERR_NOT_INITIALIZED, "ReSTIR GI: ZR_STAGE_SPATIAL before the frame's ZR_STAGE_TEMPORAL");
        F.cur = F.prev = p->gi[p->hist.Oth()].View();      // the set this frame's k_rgi wrote
        F.finalRGBA = p->finalRGBA.p;
        prm.accumulate = (cb->accumulate && cb->camera_static) ? 1u : 0u;      // (the TEMPORAL stage above cleared it for k_rgi's scratch plane)
        prm.doTemporal = 0u; prm.writeReservoirs = 0u; prm.textured = 0u;
        TimerBegin(p, s, "rgi_spatial");
        hipLaunchKernelGGL(k_rgi_spatial, dim3(tilesX * tilesY), dim3(kBlock), 0, s, F, *cb, tilesX, p->counters.p + 2 * 13, p->rgiSpatialFrame);
        TimerEnd(p, s);
        HIP_TRY(hipGetLastError());
    }
    return ZR_OK;
}

// K11 is launched as one-wave blocks, and a wave lives for the whole path: a grid of a few thousand waves runs in ROUNDS of as many waves as are
// resident at once -- 3072 for the 3-wave build, 4096 for the 4-wave build.  A 480 x 544 tile of the 8-way screen split is 4080 waves: one round and
// a third of a second one at 3 waves per SIMD, exactly one at 4.  Measured per tile of the Cornell frame (scripts/gpu_r03_rounds.sh [rounds 1-4: git history up to 31e92fa; today scripts/gpu.sh ab]): the busiest
// 8-way tiles 0.365 -> 0.31 ms with the 4-wave build (slowest tile of the split 0.82 -> 0.76 ms); with two rounds or more the per-wave cost of the
// 4-wave build (the kernel is VALU-bound: a wave shares its SIMD with one more) eats the saving -- the 4-way split's tiles (8160 waves) get 4 - 17 %
// slower, the 2-way split's do not care -- so only the one-round case switches.
// frame overlap, carry mode: every plane of reservoir set `src` (+ its target plane) into `dst`, pixel by pixel (62 + 16 B read and written per pixel)
__global__ void __launch_bounds__(256) k_rpt_carry(rpt::ResPlanes dst, rpt::ResPlanes src, F4* tdst, const F4* tsrc, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    {
        dst.A[i] = src.A[i]; dst.B[2 * i] = src.B[2 * i]; dst.B[2 * i + 1] = src.B[2 * i + 1]; dst.C[i] = src.C[i]; dst.D[i] = src.D[i]; dst.E[i] = src.E[i];
        dst.F[2 * i] = src.F[2 * i]; dst.F[2 * i + 1] = src.F[2 * i + 1]; dst.G[2 * i] = src.G[2 * i]; dst.G[2 * i + 1] = src.G[2 * i + 1];
        tdst[i] = tsrc[i];
    }
}
static bool FewerRoundsAtFourWaves(uint32_t waves)
{
    static const bool off = [] { const char* e = ZR_EXP_ENV("ZR_K11_ROUNDS"); return e && !strcmp(e, "0"); }();      // (A/B switch)
    return !off && waves > 3072u && waves <= 4096u;
}

// ---- the K12 sorts a stage puts off (zr_pass::RptPendingSort).  A sorted map is a function of the G-buffer flags (and, Sort_TtC, the motion vectors) of
// the stage's frame, of plane A of ONE reservoir set -- Sort_TtC: the "previous" set of the temporal stage, Sort_CtS: the set the spatial round reads --
// and of doSpatial / the frame constants, which the record holds by value.  The stage only reads that set (zr_rpt_overlap.h: BeginTemporalReuse declares
// Oth() read, BeginSpatialRound declares Cur() read), so the sort gives the same map for as long as nobody writes the set or that G-buffer plane set.
// The record ends in one of three ways, whichever comes first:
//   * somebody asks for the map (zr_pass_get_output): launched there, on the stream of the stage that put it off, where that stage's consumers run;
//   * a stage is about to write the reservoir set it reads (RptSettleMaps, called by every stage ahead of its Begin...): launched there, on that stage's
//     stream.  Who writes which set: K11 the set that takes the "current" role (without overlap the very set the last spatial round read, or the previous
//     set of a frame without a spatial round; with overlap the free set, which a record outlives only when a frame ran no sort at all); a spatial round
//     the set the temporal stage read as "previous", and the second round the set the first one read;
//   * a later sort launch gives the map new contents (the spatial stage's Sort_StC replaces the temporal stage's TtC map, the next frame's Sort_CtT the
//     CtS map): dropped, nobody can see the map it would have written.  This is the frame's ordinary course: it launches neither.
// With frame overlap on, the launch is a reader of its set and of its G-buffer plane set under the stream-order trackers like any stage: behind their
// last writes, and marked, so that the next writer on another stream waits for it.  The G-buffer belongs to the caller: a record whose G-buffer has been
// destroyed, or whose plane set has been rendered again (possible only for a caller that renders G-buffers without rendering this pass), is dropped.
// The tile-split path moves reservoir sets only, never the maps (HaloPlanes), and never into a set a record reads: between the stages it addresses
// Cur() -- the records read Oth() there: the temporal stage's "previous" set, and after a round's flip the set that round read -- and after the frame
// Oth(), the set the last stage wrote, where the records read the other one.
// (the stages' own kernel instantiations, with the map that a stage left out in the place of the one it sorted: a launch of one map is numTiles blocks)
static void LaunchPendingSort(const zr_pass::RptPendingSort& q, uint16_t* map, hipStream_t s)
{
    uint16_t* const none = nullptr; uint32_t* const noList = nullptr;
    if (q.variant == rpt::RPT_SORT_TTC)
        hipLaunchKernelGGL((k_rpt_sort<rpt::RPT_SORT_CTT, rpt::RPT_SORT_TTC, true>), dim3(q.numTiles), dim3(256), 0, s, q.F, q.cb, q.sortTilesX, q.F.ox0 / 32u, q.F.oy0 / 32u, q.numTiles, none, map, 0u, noList, noList, noList);
    else
        hipLaunchKernelGGL((k_rpt_sort<rpt::RPT_SORT_STC, rpt::RPT_SORT_CTS, false>), dim3(q.numTiles), dim3(256), 0, s, q.F, q.cb, q.sortTilesX, q.F.ox0 / 32u, q.F.oy0 / 32u, q.numTiles, none, map, 0u, noList, noList, noList);
}
static int RptRunPendingSort(zr_pass* p, int idx, hipStream_t s)
{
    zr_pass::RptPendingSort& q = p->rptPending[idx];
    if (!q.live) return ZR_OK;
    q.live = false;
    {
        std::lock_guard<std::mutex> lk(g_liveGBuffersMtx);
        auto it = g_liveGBuffers.find(q.gb);
        if (it == g_liveGBuffers.end() || it->second != q.gbUid) return ZR_OK;
    }
    zr_gbuffer* gb = q.gb;
    if (gb->renderAt[q.gbSet] != q.gbRenderAt) return ZR_OK;
    const bool tracked = p->ov.overlap;
    if (tracked) { if (int r = p->ov.sets[q.set].AcquireRead(p->ov.points, s)) return r; }
    if (gb->tracked) { if (int r = gb->order[q.gbSet].AcquireRead(gb->points, s)) return r; }
    LaunchPendingSort(q, p->rptMap[idx].p, s);
    HIP_TRY(hipGetLastError());
    if (tracked) { if (int r = p->ov.sets[q.set].MarkRead(p->ov.points, s)) return r; }
    return gb->MarkRead(q.gbSet, s);
}
// a stage on stream s is about to write reservoir set `set`: the sorts that still have to read it run first
static int RptSettleMaps(zr_pass* p, hipStream_t s, int set)
{
    for (int i = 0; i < 2; i++) if (p->rptPending[i].live && p->rptPending[i].set == set) if (int r = RptRunPendingSort(p, i, s)) return r;
    return ZR_OK;
}
static void RptPutOffSort(zr_pass* p, int idx, int variant, const rpt::RptFrame& F, const zr_frame_constants& cb, uint32_t sortTilesX, uint32_t numTiles, hipStream_t s, int set, zr_gbuffer* gb)
{
    zr_pass::RptPendingSort& q = p->rptPending[idx];
    q.live = true; q.variant = variant; q.F = F; q.cb = cb; q.sortTilesX = sortTilesX; q.numTiles = numTiles; q.stream = s; q.set = set;
    q.gb = gb; q.gbUid = gb->uid; q.gbSet = gb->cur; q.gbRenderAt = gb->renderAt[gb->cur];
}

static int RenderReSTIR_PT(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb, int stages)
{
    using namespace rpt;
    // the TEMPORAL stage in its two halves (zetaray_amd.h): K11 alone / K12 - K14
    const bool stageCand = (stages & (ZR_STAGE_TEMPORAL | ZR_STAGE_CANDIDATES)) != 0, stageReuseT = (stages & (ZR_STAGE_TEMPORAL | ZR_STAGE_TEMPORAL_REUSE)) != 0;
    const zr::RptRoles& roles = p->ov.roles;      // which storage plays which role; every stage below asks, p->ov's Begin / End calls move them
    if (stageCand)
    {
        if (p->ov.overlap)
        {
            // two frames in flight need the G-buffer's third plane set and its stream tracking: both belong to the G-buffer handed to zr_pass_set_frame_overlap (a renderer
            // that replaces its G-buffer -- a resize -- hands the new one over again)
            if (!gb->tracked || gb->numSets < 3) return Fail(ZR_ERR_INVALID_ARG, "ReSTIR PT with frame overlap: this G-buffer is not the one given to zr_pass_set_frame_overlap (call it again with the new G-buffer)");
            if (roles.frameOpen) return Fail(ZR_ERR_INVALID_ARG, "ReSTIR PT with frame overlap: the previous frame's last stage has not been enqueued (stage order: CANDIDATES, TEMPORAL_REUSE, SPATIAL[, SPATIAL2])");
        }
        // K11 writes the set that takes the "current" role -- with overlap the free set, else Cur(): a K12 sort put off that reads it runs first (RptRunPendingSort)
        if (int sr = RptSettleMaps(p, s, p->ov.overlap ? roles.set[2] : roles.Cur())) return sr;
        // K11's accesses (with overlap: after the roles have moved on to this frame's).  Only host work lies between here and its launches.
        if (int br = p->ov.BeginCandidates(s, cb->accumulate && cb->camera_static)) return br;
    }
    RptFrame F;
    F.sc = FrameView(sc, cb); F.gb = gb->View(); F.gbPrev = gb->PrevView();
    F.scPrev = FrameViewPrev(sc, cb);
    F.sc.texFilter = F.scPrev.texFilter = p->params.tex_filter;
    if (int orc = ResolveOwnedRect(p, gb, cb, &F.ox0, &F.oy0, &F.ow, &F.oh)) return orc;
    F.rbCtN = p->rb[0].View(); F.rbNtC = p->rb[1].View(); F.tex.target = p->TargetPlane(roles.Target()).p; F.tex.neighbor = p->rptNeighbor.p;
    F.finalRGBA = p->FinalPlane(roles.Final()).p; F.sampleSet = p->rptSampleSet.p;
    F.mapCtN = p->rptMap[0].p; F.mapNtC = p->rptMap[1].p;
    F.costMap = p->costOn ? p->costMap.p : nullptr; F.costW = (p->w + 31u) / 32u + 1u; F.costMode = p->costRays ? 1u : 0u;
    F.trip = nullptr; F.tripStats = nullptr; F.tripStride = 0;
    F.carryOut = nullptr; F.carryIn = nullptr; F.carryCount = nullptr; F.carryCap = 0; F.carryBounce = 0;
    // K12 sorts whole 32 x 32 tiles: an owned rect may end inside one only where the render target ends
    if (((F.ox0 + F.ow) & 31u) && F.ox0 + F.ow != cb->render_width) return Fail(ZR_ERR_INVALID_ARG, "ReSTIR PT: the owned rect must end on a 32-pixel boundary or at the right edge of the render target");
    if (((F.oy0 + F.oh) & 31u) && F.oy0 + F.oh != cb->render_height) return Fail(ZR_ERR_INVALID_ARG, "ReSTIR PT: the owned rect must end on a 32-pixel boundary or at the bottom edge of the render target");
    const zr_params& ip = p->params;
    if (stageCand)
    {   // what the frame reuses is decided here and held (p->doTemporal, p->doSpatial) for its later stages
        p->rptViewFrame = p->rptView;
        const zr::ReuseFlags now = zr::ReuseFlagsOf(ip.flags, p->hist.valid, gb->numRendered >= 2, *cb);
        p->doTemporal = now.doTemporal != 0;
        p->doSpatial = now.doSpatial && ip.num_spatial_passes > 0;      // IndirectLighting.cpp:906
    }
    // m_numSpatialPasses (IndirectLighting.cpp:616-621, 1240): 0..2
    if (ip.num_spatial_passes > 2u) return Fail(ZR_ERR_INVALID_ARG, "ReSTIR PT: num_spatial_passes must be 0, 1 or 2");
    const uint32_t numSpatialPasses = ip.num_spatial_passes;
    RptParams& prm = F.prm = zr::RptParamsOf(ip, *cb, zr::ReuseFlagsLatched(p->doTemporal, p->doSpatial, p->hist.valid, *cb), sc->view.tex.count != 0);
    // the CtN map (current reservoirs bucketed by k) schedules the fused CtT + TtC kernel: 0.540 -> 0.495 ms Cornell, 3.27 -> 3.16 ms atrium at
    // 1080p; the NtC map does not pay (0.546 / 3.34).  ZR_TEMPORAL_MAP = 0 / 1 / 2 overrides (scripts/gpu_sortmap.sh [rounds 1-4: git history up to 31e92fa; today scripts/gpu.sh ab])
    static const uint32_t temporalMapEnv = [] { const char* e = ZR_EXP_ENV("ZR_TEMPORAL_MAP"); return e ? (uint32_t)atoi(e) : 1u; }();
    prm.temporalMap = prm.sortTemporal ? temporalMapEnv : 0u;
    // staged (tile-split) rendering with two rounds: ZR_STAGE_SPATIAL runs the first, ZR_STAGE_SPATIAL2 the second -- it reads the first round's outputs at
    // neighbouring pixels, so the host exchanges ZR_HALO_POST_TEMPORAL (= the set the next stage reads: res[roles.Cur()]) once more in between
    F.cur = p->res[roles.Cur()].View(); F.prev = p->res[roles.Oth()].View();
    const uint32_t tilesX = (F.ow + 15) / 16, tilesY = (F.oh + 15) / 16;
    const dim3 grid(tilesX * tilesY), block(kBlock);
    const dim3 gridRpt(tilesX * tilesY * (256 / kRptBlock)), blockRpt(kRptBlock);      // K11 (zr_kernels.h kRptBlock)
    const dim3 gridRecon(tilesX * tilesY * (256 / kReconBlock)), blockRecon(kReconBlock);      // K14 (zr_kernels.h kReconBlock)
    const dim3 gridStc(tilesX * tilesY * (256 / kStcBlock)), blockStc(kStcBlock);                // K16 (zr_kernels.h kStcBlock)
    const uint32_t sortTilesX = (F.ow + 31) / 32;
    const dim3 gridSort(sortTilesX * ((F.oh + 31) / 32));
    // work lists for the replay passes: [0] CtT, [1] TtC, [2] CtS, [3] StC (plane-local pixel ids, device-side counts)
    uint32_t* listCnt = p->rptListCounts.p;
    const size_t cap = (size_t)p->w * p->h;
    uint32_t* lists[4] = {p->rptLists.p, p->rptLists.p + cap, p->rptLists.p + 2 * cap, p->rptLists.p + 3 * cap};
    const dim3 gridList((uint32_t)std::min<size_t>((cap + kBlock - 1) / kBlock, 1024));
    const dim3 gridLight((tilesX * tilesY + kLightTilesPerBlock - 1u) / kLightTilesPerBlock), gridSearch((tilesX * tilesY + kSearchTilesPerBlock - 1u) / kSearchTilesPerBlock);      // k_rpt_light<0> / <1>: several tiles per block
    const dim3 gridReplay((uint32_t)std::min<size_t>((cap + kBlock - 1) / kBlock, kReplayPersistentBlocks));      // the temporal replays pull their work (zr_kernels.h)
    unsigned long long* ctr = p->counters.p;
#define RPT_TIMED(name, ...) do { TimerBegin(p, s, name); __VA_ARGS__; TimerEnd(p, s); } while (0)
    // the NEE_EMISSIVE permutation of a kernel (the reference compiles separate shaders, IndirectLighting.h:251-300)
    const bool emissiveVariant = prm.emissive != 0;
    // (zr_debug_set_large_scene_nodes: test hook, lets the parity tests run the large-scene kernel build on their small scenes)
    const uint32_t largeSceneNodes = g_largeSceneNodes.load(std::memory_order_relaxed);
    // ... and the TEXTURED permutation (this ABI's: untextured scenes carry no ray differentials)
    const bool texVariant = prm.textured != 0;
    // ... and the material-class permutation (zr_kernels.h PLAIN): scenes of opaque uncoated non-metallic dielectrics without a texture heap run kernels that have no code for the other lobes
    const bool plainVariant = PlainClass(sc, gb) && !texVariant;
#define RPT_LAUNCH_E(kern, ...) do { \
        if (plainVariant) { if (emissiveVariant) hipLaunchKernelGGL((kern<true, false, true>), __VA_ARGS__); else hipLaunchKernelGGL((kern<false, false, true>), __VA_ARGS__); } \
        else if (emissiveVariant) { if (texVariant) hipLaunchKernelGGL((kern<true, true, false>), __VA_ARGS__); else hipLaunchKernelGGL((kern<true, false, false>), __VA_ARGS__); } \
        else { if (texVariant) hipLaunchKernelGGL((kern<false, true, false>), __VA_ARGS__); else hipLaunchKernelGGL((kern<false, false, false>), __VA_ARGS__); } } while (0)
#define RPT_LAUNCH_PE(kern, PASS, ...) do { \
        if (emissiveVariant) { if (texVariant) hipLaunchKernelGGL((kern<PASS, true, true>), __VA_ARGS__); else hipLaunchKernelGGL((kern<PASS, true, false>), __VA_ARGS__); } \
        else { if (texVariant) hipLaunchKernelGGL((kern<PASS, false, true>), __VA_ARGS__); else hipLaunchKernelGGL((kern<PASS, false, false>), __VA_ARGS__); } } while (0)
    // a reconnection debug view: the VIEW instantiations of the three kernels that write FINAL (zr_kernels.h), general material class
    const uint32_t view = (uint32_t)p->rptViewFrame;
#define RPT_LAUNCH_VIEW(kern, ...) do { \
        if (emissiveVariant) { if (texVariant) hipLaunchKernelGGL((kern<true, true>), __VA_ARGS__, view); else hipLaunchKernelGGL((kern<true, false>), __VA_ARGS__, view); } \
        else { if (texVariant) hipLaunchKernelGGL((kern<false, true>), __VA_ARGS__, view); else hipLaunchKernelGGL((kern<false, false>), __VA_ARGS__, view); } } while (0)
    if (stageCand)
    {
        if (int ar = gb->AcquireRead(s)) return ar;
        if (roles.carryFrom >= 0)
        {
            // ZR_FRAME_OVERLAP_CARRY: K11 and the passes behind it update reservoir records in place (Reservoir.hlsli:283-456 writes the components a record's case
            // uses), so the bytes a record does NOT use are whatever the set held before -- in the plain order the set K11 wrote last frame, here the free set.
            // Copying the replaced set (and target plane) into the one that takes its place makes every byte of every plane equal to the plain order's.
            const size_t n = (size_t)p->w * p->h;
            RPT_TIMED("rpt_overlap_carry", hipLaunchKernelGGL(k_rpt_carry, dim3((uint32_t)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, F.cur, p->res[roles.carryFrom].View(), F.tex.target,
                (const F4*)p->TargetPlane(roles.OtherTarget()).p, n));
        }
        TimerBegin(p, s, "rpt_pathtrace");
        if (view != ZR_RPT_VIEW_NONE) RPT_LAUNCH_VIEW(k_rpt_pathtrace_view, gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1);
        else
        {
#ifdef ZR_EXPERIMENTS
        // (experiments build, zr_kernels_exp.h) ZR_K11=pool: K11 with block-pooled traces (k_rpt_pathtrace_coop; emissive untextured permutation);
        // compact: a kernel per bounce; trip: the alive-lane diagnostic; ZR_K11=inline: the megakernel
        static const int k11Mode = [] { const char* e = getenv("ZR_K11"); return e && !strcmp(e, "inline") ? 0 : (e && !strcmp(e, "pool") ? 1 : (e && !strcmp(e, "trip") ? 2 : (e && !strcmp(e, "compact") ? 3 : ZR_K11_DEFAULT))); }();
        static const bool park = [] { const char* e = getenv("ZR_K11_PARK"); return e ? atoi(e) != 0 : (ZR_K11_PARK_DEFAULT != 0); }();      // the 3-wave build with the reservoir's selected reconnection in LDS (zr_rpt.h RcPark)
        if (k11Mode == 1 && emissiveVariant && !texVariant)
        {
            const dim3 gridCoop(tilesX * tilesY), blockCoop(kCoopBlock);
            if (sc->view.numNodes >= largeSceneNodes) hipLaunchKernelGGL(k_rpt_pathtrace_coop_w4<false>, gridCoop, blockCoop, 0, s, F, *cb, tilesX, ctr + 2 * 1);
            else hipLaunchKernelGGL(k_rpt_pathtrace_coop<false>, gridCoop, blockCoop, 0, s, F, *cb, tilesX, ctr + 2 * 1);
        }
        else if (k11Mode == 3 && !texVariant)
        {   // a kernel per bounce, live paths compacted in between (zr_kernels.h: k_rpt_pt_first / k_rpt_pt_next)
            const size_t cap = (size_t)F.gb.w * F.gb.h;
            if (p->carry[0].n != cap * rpt::kPtCarryWords) { int rr; for (int k = 0; k < 2; k++) if ((rr = p->carry[k].Alloc(cap * rpt::kPtCarryWords))) return rr; if ((rr = p->carryCount.Alloc(16))) return rr; }
            HIP_TRY(hipMemsetAsync(p->carryCount.p, 0, 16 * sizeof(uint32_t), s));
            uint32_t maxB = prm.maxNonTrBounces > prm.maxGlossyTrBounces ? prm.maxNonTrBounces : prm.maxGlossyTrBounces;
            if (prm.russianRoulette && maxB > 3u) maxB = 3u;      // paths that go further are traced by whole tiles inside k_rpt_pt_first
            F.carryCap = cap; F.carryCount = p->carryCount.p; F.carryBounce = 0; F.carryOut = p->carry[0].p; F.carryIn = nullptr;
            if (emissiveVariant) hipLaunchKernelGGL(k_rpt_pt_first<true>, gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1);
            else hipLaunchKernelGGL(k_rpt_pt_first<false>, gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1);
            const dim3 gridNext((uint32_t)((cap + kRptBlock - 1) / kRptBlock));
            for (uint32_t b = 1; b + 1 <= maxB && b < 15u; b++)
            {
                F.carryBounce = b; F.carryIn = p->carry[(b - 1) & 1].p; F.carryOut = p->carry[b & 1].p;
                if (emissiveVariant) hipLaunchKernelGGL(k_rpt_pt_next<true>, gridNext, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1);
                else hipLaunchKernelGGL(k_rpt_pt_next<false>, gridNext, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1);
            }
        }
        else if (k11Mode == 2 && emissiveVariant && !texVariant)
        {   // diagnostic: the megakernel with a path-state round trip through SoA planes at every bounce boundary (zr_kernels.h)
            const size_t stride = (size_t)F.gb.w * F.gb.h;
            if (!p->trip.p) { int rr; if ((rr = p->trip.Alloc(stride * rpt::kPtCarryWords))) return rr; if ((rr = p->tripStats.Alloc(4))) return rr; HIP_TRY(hipMemsetAsync(p->tripStats.p, 0, 32, s)); }
            F.trip = p->trip.p; F.tripStats = p->tripStats.p; F.tripStride = stride;
            if (sc->view.numNodes >= largeSceneNodes) hipLaunchKernelGGL(k_rpt_pathtrace_trip_w4<false>, gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1);
            else hipLaunchKernelGGL(k_rpt_pathtrace_trip<false>, gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1);
        }
        else if (k11Mode == 0 && park && !texVariant && !(sc->view.numNodes >= largeSceneNodes || FewerRoundsAtFourWaves(gridRpt.x)))
        { if (emissiveVariant) hipLaunchKernelGGL(k_rpt_pathtrace_park<true>, gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); else hipLaunchKernelGGL(k_rpt_pathtrace_park<false>, gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); }
        else
#endif
        if (texVariant) { if (emissiveVariant) hipLaunchKernelGGL(k_rpt_pathtrace_tex<true>, gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); else hipLaunchKernelGGL(k_rpt_pathtrace_tex<false>, gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); }
        else if (sc->view.numNodes >= largeSceneNodes || FewerRoundsAtFourWaves(gridRpt.x))     // BVH beyond the caches, or a small grid: the 4-wave build of K11 (zr_kernels.h)
        {
            if (plainVariant) { if (emissiveVariant) hipLaunchKernelGGL((k_rpt_pathtrace_w4<true, true>), gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); else hipLaunchKernelGGL((k_rpt_pathtrace_w4<false, true>), gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); }
            else if (emissiveVariant) hipLaunchKernelGGL((k_rpt_pathtrace_w4<true, false>), gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); else hipLaunchKernelGGL((k_rpt_pathtrace_w4<false, false>), gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1);
        }
        else
        {
            if (plainVariant) { if (emissiveVariant) hipLaunchKernelGGL((k_rpt_pathtrace<true, true>), gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); else hipLaunchKernelGGL((k_rpt_pathtrace<false, true>), gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); }
            else if (emissiveVariant) hipLaunchKernelGGL((k_rpt_pathtrace<true, false>), gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1); else hipLaunchKernelGGL((k_rpt_pathtrace<false, false>), gridRpt, blockRpt, 0, s, F, *cb, tilesX, ctr + 2 * 1);
        }
        }
        TimerEnd(p, s);
        if (int er = p->ov.EndCandidates(s)) return er;
    }
    if (stageReuseT)
    {
        // behind K11 when that ran on another stream (it wrote the current set, the target and FINAL), and with it behind the GBUFFER render before it there
        hipStream_t k11;
        const bool behindK11 = p->ov.CandidatesStream(&k11) && k11 != s;      // (K11 read the same planes, behind their render)
        if (int br = p->ov.BeginTemporalReuse(s)) return br;
        if (!behindK11) if (int ar = gb->AcquireRead(s)) return ar;
        HIP_TRY(hipMemsetAsync(listCnt, 0, kRptListWords * sizeof(uint32_t), s));      // (the work lists are the reuse passes' alone: K11 of the next frame may already run)
        if (prm.doTemporal)
        {
            // K12 Sort_TtC / Sort_CtT (IndirectLighting.cpp:383-441: dispatched whether or not SORT_TEMPORAL is set).  The temporal reconnect
            // passes have no wave operations, so these two maps cannot change a result; they are outputs (ZR_OUT_RPT_THREAD_MAP_*), and the CtT map
            // schedules K14 (temporalMap).  Sort_CtT is launched here -- K14 rewrites the plane it buckets by, it cannot wait.  Sort_TtC is launched here only
            // when K14 is scheduled by its map (ZR_TEMPORAL_MAP=2); otherwise it is put off until somebody asks for the NtC map (RptRunPendingSort), which
            // the spatial stage's Sort_StC overwrites in the same frame.  The blocks behind the sort tiles classify the pixels into the two replay work
            // lists (k_rpt_light<0>'s work; once a launch of its own, timer "rpt_classify_temporal"): the launch reports as "rpt_sort_temporal".
            const bool sortTtCNow = prm.temporalMap == 2u;
            p->rptPending[0].live = false;      // (the CtN map gets new contents: a Sort_CtS still put off has nobody left to show it to)
            if (sortTtCNow) p->rptPending[1].live = false;
            else RptPutOffSort(p, 1, rpt::RPT_SORT_TTC, F, *cb, sortTilesX, gridSort.x, s, roles.Oth(), gb);
            RPT_TIMED("rpt_sort_temporal", hipLaunchKernelGGL((k_rpt_sort<rpt::RPT_SORT_CTT, rpt::RPT_SORT_TTC, true>), dim3(gridSort.x * (sortTtCNow ? 2u : 1u) + gridLight.x), dim3(256), 0, s, F, *cb,
                sortTilesX, F.ox0 / 32u, F.oy0 / 32u, gridSort.x, F.mapCtN, sortTtCNow ? F.mapNtC : (uint16_t*)nullptr, tilesX, lists[0], lists[1], listCnt + 0));
            RPT_TIMED("rpt_replay_temporal", RPT_LAUNCH_PE(k_rpt_replay, RPT_REPLAY_CTT, gridReplay, block, 0, s, F, *cb, lists[0], lists[1], listCnt + 0, ctr + 2 * 2));
            if (view != ZR_RPT_VIEW_NONE) RPT_TIMED("rpt_reconnect_temporal", RPT_LAUNCH_VIEW(k_rpt_temporal_view, gridRecon, blockRecon, 0, s, F, *cb, tilesX, ctr + 2 * 4));
            else RPT_TIMED("rpt_reconnect_temporal", RPT_LAUNCH_E(k_rpt_temporal, gridRecon, blockRecon, 0, s, F, *cb, tilesX, ctr + 2 * 4));
        }
        // nothing after this point reads the PREVIOUS frame's G-buffer, its final reservoirs or scene (the spatial passes read this frame's only)
        if (int er = p->ov.EndTemporalReuse(s)) return er;
        if (int mr = gb->MarkRead(gb->Prev(), s)) return mr;
    }
    for (uint32_t spass = 0; spass < numSpatialPasses && prm.doSpatial; spass++)
    {
        if (!(stages & (spass == 0 ? ZR_STAGE_SPATIAL : ZR_STAGE_SPATIAL2))) continue;
        // a round reads the current set and writes the other one, which then becomes "current" (IndirectLighting.cpp:609-612, 682-688: one flip per round)
        // K12 sorts put off: this round's Sort_StC gives the NtC map new contents and its Sort_CtS stands for the CtN map's -- what was put off before is dropped;
        // without SORT_SPATIAL the maps stay what they are, and a sort that reads the set this round writes runs first (RptRunPendingSort)
        if (prm.sortSpatial) { p->rptPending[0].live = false; p->rptPending[1].live = false; }
        else if (int sr = RptSettleMaps(p, s, roles.Oth())) return sr;
        if (int br = p->ov.BeginSpatialRound(s)) return br;
        F.cur = p->res[roles.Cur()].View(); F.prev = p->res[roles.Oth()].View();
        // replay work lists + their device-side counts of this round: {2, 3} for the first, {6, 7} for the second (zeroed at the start of the frame)
        uint32_t* const sCnt = listCnt + (spass == 0 ? 2 : 6);
#ifdef ZR_EXPERIMENTS
        // ZR_SEARCH=tile: the LDS-tiled K15 (k_rpt_light<2>), kept for the A/B of DESIGN's N3 row -- measured slower than the plain gathers
        static const bool searchTile = [] { const char* e = getenv("ZR_SEARCH"); return e && !strcmp(e, "tile"); }();
        if (searchTile) RPT_TIMED("rpt_spatial_search", hipLaunchKernelGGL(k_rpt_light<2>, grid, block, 0, s, F, *cb, tilesX, lists[2], lists[3], sCnt));
        else
#endif
        RPT_TIMED("rpt_spatial_search", hipLaunchKernelGGL(k_rpt_light<1>, gridSearch, block, 0, s, F, *cb, tilesX, lists[2], lists[3], sCnt));
        // K12 Sort_CtS / Sort_StC (IndirectLighting.cpp:690-742): the NtC map decides which pixels share a wave in Reconnect_StC, i.e. the
        // population of its boiling-suppression averages
        if (prm.sortSpatial)
        {
            // (Sort_StC alone: K16 reads its map.  The CtS map is an output only -- put off until somebody asks for it)
            RPT_TIMED("rpt_sort_spatial", hipLaunchKernelGGL((k_rpt_sort<rpt::RPT_SORT_STC, rpt::RPT_SORT_CTS, false>), gridSort, dim3(256), 0, s, F, *cb, sortTilesX, F.ox0 / 32u, F.oy0 / 32u, gridSort.x,
                F.mapNtC, (uint16_t*)nullptr, 0u, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr));
            RptPutOffSort(p, 0, rpt::RPT_SORT_CTS, F, *cb, sortTilesX, gridSort.x, s, roles.Cur(), gb);
        }
        RPT_TIMED("rpt_replay_spatial", RPT_LAUNCH_PE(k_rpt_replay, RPT_REPLAY_CTS, dim3(gridList.x * 2), block, 0, s, F, *cb, lists[2], lists[3], sCnt, ctr + 2 * 5));
        if (view != ZR_RPT_VIEW_NONE) RPT_TIMED("rpt_reconnect_spatial", RPT_LAUNCH_VIEW(k_rpt_stc_view, gridStc, blockStc, 0, s, F, *cb, tilesX, ctr + 2 * 7));
        else RPT_TIMED("rpt_reconnect_spatial", RPT_LAUNCH_E(k_rpt_stc, gridStc, blockStc, 0, s, F, *cb, tilesX, ctr + 2 * 7));
        // "Prepare for next iteration" (IndirectLighting.cpp:860-870: std::swap(inputs, outputs)) is the flip itself here: the next round starts from the set this one wrote
        if (int er = p->ov.EndSpatialRound(s)) return er;
    }
#undef RPT_TIMED
#undef RPT_LAUNCH_E
#undef RPT_LAUNCH_PE
#undef RPT_LAUNCH_VIEW
    HIP_TRY(hipGetLastError());
    // the frame ends with its last stage: the second round when there is one this frame, else ZR_STAGE_SPATIAL; Render() flips once more (:1018-1024)
    const bool lastStage = (prm.doSpatial && numSpatialPasses == 2u) ? (stages & ZR_STAGE_SPATIAL2) != 0 : (stages & ZR_STAGE_SPATIAL) != 0;
    if (lastStage && roles.frameOpen)
    {
        p->hist.valid = true;
        p->ov.CloseFrame();
        if (int mr = gb->MarkRead(gb->cur, s)) return mr;
    }
    return ZR_OK;
}

static int RenderIndirect(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb, int stages)
{
    if (!gb) return Fail(ZR_ERR_INVALID_ARG, "INDIRECT pass needs a gbuffer");
    if (gb->w != p->w || gb->h != p->h || gb->x0 + gb->w > cb->render_width || gb->y0 + gb->h > cb->render_height)
        return Fail(ZR_ERR_INVALID_ARG, "frame constants / gbuffer tile / pass size mismatch");
    if (sc->view.numEmissives == 0)
    {
        // NEE_EMISSIVE == 0 shader variants: sun + sky next-event estimation
        if (!sc->view.sky.data) return Fail(ZR_ERR_NOT_INITIALIZED, "sky-view LUT missing: render a ZR_PASS_SKY pass first");
    }
    else if (!sc->view.alias) return Fail(ZR_ERR_NOT_INITIALIZED, "emissive alias table missing: render the PRELIGHTING pass (or zr_scene_set_alias_table) first");
    if (cb->num_emissive_triangles != sc->view.numEmissives) return Fail(ZR_ERR_INVALID_ARG, "cbFrameConstants.NumEmissiveTriangles != scene");
    if (p->params.presampling && (!sc->view.sampleSets || sc->numSampleSets != p->params.num_sample_sets || sc->view.sampleSetSize != p->params.sample_set_size))
        return Fail(ZR_ERR_NOT_INITIALIZED, "presampled light sets missing or of another size: render the PRELIGHTING pass with the same presampling params first");
    if (p->integrator == ZR_INTEGRATOR_RESTIR_PT) return RenderReSTIR_PT(p, s, cb, sc, gb, stages);
    if (p->integrator == ZR_INTEGRATOR_RESTIR_GI) return RenderReSTIR_GI(p, s, cb, sc, gb, stages);
    if (!(stages & ZR_STAGE_TEMPORAL)) return ZR_OK;      // the path tracer renders in the first stage
    PtParams prm;
    prm.maxNonTrBounces = p->params.max_non_tr_bounces; prm.maxGlossyTrBounces = p->params.max_glossy_tr_bounces;
    prm.russianRoulette = (p->params.flags & ZR_IND_RUSSIAN_ROULETTE) ? 1u : 0u;
    prm.numSampleSets = p->params.presampling ? p->params.num_sample_sets : 0u;
    prm.accumulate = (cb->accumulate && cb->camera_static) ? 1u : 0u;
    prm.tileW = p->w; prm.groupsX = (p->w + 7) / 8;
    const uint32_t numGroups = prm.groupsX * ((p->h + 7) / 8);
    const uint32_t maxB = prm.maxNonTrBounces > prm.maxGlossyTrBounces ? prm.maxNonTrBounces : prm.maxGlossyTrBounces;
    const int rounds = (int)maxB + 1;
    if (rounds > kMaxRounds) return Fail(ZR_ERR_INVALID_ARG, "too many bounces");

    HIP_TRY(hipMemsetAsync(p->counts.p, 0, 5 * (kMaxRounds + 2) * kCounterStride * sizeof(uint32_t), s));
    // counter (kind, round): kind 0 = live paths, 1 = k_trace cursor, 2..4 = C / M / S rays
    auto Ctr = [&](int kind, int round) { return p->counts.p + ((size_t)round * 5 + kind) * kCounterStride; };
    // Russian roulette can only trigger once bounce >= 3, i.e. from round 2 on and only if some path may take >= 4 bounces
    const bool rrPossible = prm.russianRoulette && maxB >= 4;
    if (rrPossible) HIP_TRY(hipMemsetAsync(p->groupMax.p, 0, (size_t)rounds * numGroups * sizeof(uint32_t), s));
    const uint32_t tilesX = (p->w + 15) / 16, tilesY = (p->h + 15) / 16;
    const GBuf gbv = gb->View();
    SceneView scv = FrameView(sc, cb);
    scv.texFilter = p->params.tex_filter;
    const bool tex = scv.tex.count != 0;      // kernels carry ray differentials only when there is a texture heap
    const bool plainPt = PlainClass(sc, gb);
    if (tex) { int r; if ((r = p->q[0].AllocTex((size_t)p->w * p->h)) || (r = p->q[1].AllocTex((size_t)p->w * p->h))) return r; }
    TimerBegin(p, s, "pt_init");
    hipLaunchKernelGGL((tex ? k_pt_init<true, false> : plainPt ? k_pt_init<false, true> : k_pt_init<false, false>), dim3(tilesX * tilesY), dim3(kBlock), 0, s, scv, *cb, gbv, prm, p->finalRGBA.p, p->firstBOP.p,
        p->q[0].View(), Ctr(0, 0), Ctr(2, 0), (uint32_t)((size_t)p->w * p->h), tilesX);
    TimerEnd(p, s);
    const size_t cap = (size_t)p->w * p->h;
    const uint32_t gridShade = (uint32_t)std::min<size_t>((cap + kBlock - 1) / kBlock, 4096);
    const uint32_t gridTrace = (uint32_t)std::min<size_t>((3 * cap + kBlock - 1) / kBlock, 2048);    // persistent: 256 CUs x 8 blocks
    const uint32_t gridTraceSimple = (uint32_t)std::min<size_t>((3 * cap + kBlock - 1) / kBlock, 8192);
    static const int traceMode = [] { const char* e = ZR_EXP_ENV("ZR_TRACE_MODE"); return e ? atoi(e) : 0; }();
    for (int r = 0; r < rounds; r++)
    {
        const PathQueue qin = p->q[r & 1].View(), qout = p->q[(r + 1) & 1].View();
        TimerBegin(p, s, "trace");
        if (traceMode == 0) hipLaunchKernelGGL(k_trace_simple, dim3(gridTraceSimple), dim3(kBlock), 0, s, scv, qin, Ctr(2, r), (uint32_t)cap, p->counters.p);
        else hipLaunchKernelGGL(k_trace, dim3(gridTrace), dim3(kBlock), 0, s, scv, qin, Ctr(2, r), (uint32_t)cap, Ctr(1, r), p->counters.p);
        TimerEnd(p, s);
        TimerBegin(p, s, "pt_shade");
        hipLaunchKernelGGL(tex ? k_pt_shade_tex : plainPt ? k_pt_shade<true> : k_pt_shade<false>, dim3(gridShade), dim3(kBlock), 0, s, scv, *cb, prm, qin, Ctr(0, r), qout, Ctr(0, r + 1), Ctr(2, r + 1), (uint32_t)cap,
            p->finalRGBA.p, p->firstBOP.p, p->groupMax.p + (size_t)r * numGroups);
        TimerEnd(p, s);
        if (rrPossible && r >= 2)
        {
            TimerBegin(p, s, "pt_rr");
            hipLaunchKernelGGL(tex ? k_pt_rr<true> : k_pt_rr<false>, dim3(gridShade), dim3(kBlock), 0, s, scv, prm, qout, Ctr(0, r + 1), Ctr(2, r + 1), (uint32_t)cap, p->groupMax.p + (size_t)r * numGroups);
            TimerEnd(p, s);
        }
    }
    HIP_TRY(hipGetLastError());
    return ZR_OK;
}

int zr_pass_render(zr_pass* p, void* stream, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb)
{ return zr_pass_render_stage(p, stream, cb, sc, gb, ZR_STAGE_ALL | ZR_STAGE_SPATIAL2); }

int zr_pass_set_input(zr_pass* p, int which, const void* dev)
{
    if (p && p->kind == ZR_PASS_TAA && which == ZR_IN_TAA_SIGNAL) { p->compIn[3] = (const F4*)dev; return ZR_OK; }
    if (p && p->kind == ZR_PASS_DENOISE && which == ZR_IN_DENOISE_SIGNAL) { p->compIn[3] = (const F4*)dev; return ZR_OK; }
    if (p && (p->kind == ZR_PASS_AUTO_EXPOSURE || p->kind == ZR_PASS_DISPLAY))
    {
        if (which == ZR_IN_POST_SIGNAL_F16) { p->postIn16 = (const uint16_t*)dev; p->postIn32 = nullptr; return ZR_OK; }
        if (which == ZR_IN_POST_SIGNAL_F32) { p->postIn32 = (const F4*)dev; p->postIn16 = nullptr; return ZR_OK; }
        if (which == ZR_IN_DISPLAY_EXPOSURE && p->kind == ZR_PASS_DISPLAY) { p->exposureIn = (const float*)dev; return ZR_OK; }
        return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_input: bad input id for an AUTO_EXPOSURE / DISPLAY pass");
    }
    if (!p || p->kind != ZR_PASS_COMPOSITING || which < 0 || which > 2) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_input: not a COMPOSITING / TAA pass or bad input id");
    p->compIn[which] = (const F4*)dev;
    return ZR_OK;
}
// Sky::SetInscatteringEnablement + the "Inscattering" UI parameters (Sky.cpp:69-117, 210-223)
extern "C" int zr_pass_set_inscattering(zr_pass* p, int enable, uint32_t voxels_x, uint32_t voxels_y, float depth_map_exp, float near_z, float far_z)
{
    if (!p || p->kind != ZR_PASS_SKY) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_inscattering: needs a SKY pass");
    if (!p->initialized) return Fail(ZR_ERR_NOT_INITIALIZED, "zr_pass_set_inscattering: pass not initialised (zr_pass_init)");
    HIP_TRY(hipSetDevice(p->device));
    if (!enable)
    {
        p->inscatterOn = false; p->inscatterGrid.Free();      // m_voxelGrid.Reset()
        return ZR_OK;
    }
    if (voxels_x == 0 && voxels_y == 0) { voxels_x = ZR_INSCATTERING_VOXELS_X; voxels_y = ZR_INSCATTERING_VOXELS_Y; }     // Sky.h DefaultParamVals
    if (voxels_x == 0 || voxels_y == 0 || voxels_x > 4096 || voxels_y > 4096)
        return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_inscattering: voxel counts %u x %u outside 1..4096 (0 x 0 = the default)", voxels_x, voxels_y);
    if (!(depth_map_exp >= 1.0f && depth_map_exp <= 5.0f))
        return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_inscattering: depth_map_exp %g outside 1..5", (double)depth_map_exp);
    if (!(near_z >= 0.0f && near_z < far_z && far_z <= ZR_FLT_MAX))
        return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_inscattering: needs 0 <= near_z < far_z (got %g, %g)", (double)near_z, (double)far_z);
    const size_t n = (size_t)voxels_x * voxels_y * kInscatterSlices;
    if (!p->inscatterOn || p->inscatterGrid.n != n)
    {
        int r; if ((r = p->inscatterGrid.Alloc(n))) { p->inscatterOn = false; return r; }
        HIP_TRY(hipMemset(p->inscatterGrid.p, 0, n * sizeof(uint32_t)));
    }
    p->inscatter.numVoxelsX = voxels_x; p->inscatter.numVoxelsY = voxels_y;
    p->inscatter.depthMappingExp = depth_map_exp; p->inscatter.nearZ = near_z; p->inscatter.farZ = far_z;
    p->inscatterOn = true;
    return ZR_OK;
}
// Compositing::SetInscatteringEnablement + SetVoxelGridDepth / SetVoxelGridMappingExp + SHADER_IN_GPU_DESC::INSCATTERING, all read from `sky` at render time
extern "C" int zr_pass_bind_inscattering(zr_pass* p, const zr_pass* sky)
{
    if (!p || p->kind != ZR_PASS_COMPOSITING) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_bind_inscattering: needs a COMPOSITING pass");
    if (sky && sky->kind != ZR_PASS_SKY) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_bind_inscattering: the grid comes from a SKY pass");
    p->inscatterSky = sky;
    return ZR_OK;
}
extern "C" int zr_pass_set_tonemap_lut(zr_pass* p, const uint32_t* rgb9e5, uint32_t dim)
{
    if (!p || p->kind != ZR_PASS_DISPLAY || !rgb9e5 || dim == 0 || dim > 256) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_tonemap_lut: needs a DISPLAY pass and a dim^3 LUT");
    HIP_TRY(hipSetDevice(p->device));
    const size_t n = (size_t)dim * dim * dim;
    int r; if ((r = p->tonemapLut.Alloc(n))) return r;
    HIP_TRY(hipMemcpy(p->tonemapLut.p, rgb9e5, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    p->tonemapLutDim = dim;
    return ZR_OK;
}

extern "C" int zr_pass_set_display_option(zr_pass* p, int option, float roughness_th)
{
    if (!p || p->kind != ZR_PASS_DISPLAY) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_display_option: needs a DISPLAY pass");
    if (option < ZR_DISPLAY_DEFAULT || option >= ZR_DISPLAY_COUNT) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_display_option: unknown option %d", option);
    if (zr_isnan(roughness_th)) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_display_option: roughness_th is NaN");
    p->displayOption = option; p->roughnessTh = roughness_th;
    return ZR_OK;
}

extern "C" int zr_pass_set_rpt_debug_view(zr_pass* p, int view)
{
    if (!p || p->kind != ZR_PASS_INDIRECT) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_rpt_debug_view: needs an INDIRECT pass");
    if (view < ZR_RPT_VIEW_NONE || view >= ZR_RPT_VIEW_COUNT) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_rpt_debug_view: unknown view %d", view);
    p->rptView = view;      // read by ReSTIR PT only (the other integrators never look at it), from the next frame's first stage on
    return ZR_OK;
}

extern "C" int zr_pass_set_rgi_spatial(zr_pass* p, uint32_t num_samples, float radius_px)
{
    if (!p || p->kind != ZR_PASS_INDIRECT) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_rgi_spatial: needs an INDIRECT pass");
    if (num_samples > rgi::kSpatialMaxSamples) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_rgi_spatial: num_samples %u > %u", num_samples, rgi::kSpatialMaxSamples);
    if (!(radius_px >= 0.0f && radius_px <= rgi::kSpatialMaxRadius)) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_rgi_spatial: radius_px %g outside [0, %g] (0 = the default)", (double)radius_px, (double)rgi::kSpatialMaxRadius);
    // read by ReSTIR GI only (the other integrators never look at it), from the next frame's first stage on
    p->rgiSpatial.numSamples = num_samples; p->rgiSpatial.radius = radius_px == 0.0f ? rgi::kSpatialDefaultRadius : radius_px;
    return ZR_OK;
}

extern "C" int zr_pass_set_picked_instances(zr_pass* p, const uint32_t* mesh_idx, uint32_t n)
{
    if (!p || p->kind != ZR_PASS_DISPLAY) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_picked_instances: needs a DISPLAY pass");
    if (n && !mesh_idx) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_picked_instances: null indices");
    p->picks.assign(mesh_idx, mesh_idx + n);
    return ZR_OK;
}

static post::AeParams AeParamsOf(const zr_params& ip)
{ post::AeParams a; a.minLum = ip.ae_min_lum; a.lumRange = ip.ae_max_lum - ip.ae_min_lum; a.lumMapExp = ip.ae_lum_map_exp; a.adaptationRate = ip.ae_adaptation_rate; return a; }

// AutoExposure::Render (AutoExposure.cpp:100-143): clear the histogram, HISTOGRAM over the image, WEIGHTED_AVG in one group
static int RenderAutoExposure(zr_pass* p, hipStream_t s, const zr_frame_constants* cb)
{
    if (cb->render_width != p->w || cb->render_height != p->h) return Fail(ZR_ERR_INVALID_ARG, "AUTO_EXPOSURE: frame constants / pass size mismatch");
    if (!p->postIn16 && !p->postIn32) return Fail(ZR_ERR_NOT_INITIALIZED, "AUTO_EXPOSURE: no input bound (zr_pass_set_input(ZR_IN_POST_SIGNAL_*))");
    const uint32_t n = p->w * p->h;
    const post::AeParams prm = AeParamsOf(p->params);
    HIP_TRY(hipMemsetAsync(p->aeHist.p, 0, post::kHistBins * sizeof(uint32_t), s));
    TimerBegin(p, s, "ae_histogram");
    const uint32_t grid = std::min<uint32_t>((n + 255) / 256, 2048u);
    hipLaunchKernelGGL(k_ae_histogram, dim3(grid), dim3(256), 0, s, p->postIn16, p->postIn32, n, prm, p->aeHist.p);
    TimerEnd(p, s);
    TimerBegin(p, s, "ae_resolve");
    hipLaunchKernelGGL(k_ae_resolve, dim3(1), dim3(256), 0, s, p->aeHist.p, n, cb->dt, prm, p->aeExposure.p);
    TimerEnd(p, s);
    HIP_TRY(hipGetLastError());
    return ZR_OK;
}
// DisplayPass::Render (Display.cpp:188-260), the full-screen triangle of mainPS as one thread per display pixel
static int RenderPickOutlines(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc);
static int RenderDisplay(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc, const zr_gbuffer* gb)
{
    if (cb->display_width != p->w || cb->display_height != p->h) return Fail(ZR_ERR_INVALID_ARG, "DISPLAY: the pass size must be the display size of the frame constants");
    if (!p->postIn16 && !p->postIn32) return Fail(ZR_ERR_NOT_INITIALIZED, "DISPLAY: no input bound (zr_pass_set_input(ZR_IN_POST_SIGNAL_*))");
    const zr_params& ip = p->params;
    if (ip.display_tonemapper >= post::TM_COUNT) return Fail(ZR_ERR_INVALID_ARG, "DISPLAY: unknown tone mapper %u", ip.display_tonemapper);
    if (ip.display_tonemapper == ZR_TONEMAP_NEUTRAL && !p->tonemapLutDim) return Fail(ZR_ERR_NOT_INITIALIZED, "DISPLAY: the NEUTRAL tone mapper needs zr_pass_set_tonemap_lut");
    if (ip.display_auto_exposure && !p->exposureIn) return Fail(ZR_ERR_NOT_INITIALIZED, "DISPLAY: auto exposure is on but no exposure bound (ZR_IN_DISPLAY_EXPOSURE)");
    post::DisplayParams prm; prm.tonemapper = ip.display_tonemapper; prm.autoExposure = ip.display_auto_exposure; prm.saturation = ip.display_saturation; prm.agxExp = ip.display_agx_exp;
    post::Lut3D lut; lut.data = p->tonemapLut.p; lut.dim = p->tonemapLutDim;
    if (p->displayOption != ZR_DISPLAY_DEFAULT)
    {
        // the G-buffer debug views (Display.hlsl:77-168) read the current planes at render resolution
        if (!gb) return Fail(ZR_ERR_INVALID_ARG, "DISPLAY: display option %d needs the gbuffer", p->displayOption);
        if (gb->w != cb->render_width || gb->h != cb->render_height) return Fail(ZR_ERR_INVALID_ARG, "DISPLAY: gbuffer %ux%u is not the render size %ux%u", gb->w, gb->h, cb->render_width, cb->render_height);
        if (gb->x0 || gb->y0) return Fail(ZR_ERR_INVALID_ARG, "DISPLAY: display option %d needs a gbuffer with tile origin (0, 0)", p->displayOption);
        TimerBegin(p, s, "display_view");
        const hipError_t e = LaunchDisplayView(s, p->displayOption, gb->View(), p->w, p->h, cb->camera_near, p->roughnessTh, p->displayOut.p, p->displaySrgb.p);
        TimerEnd(p, s);
        HIP_TRY(e);
        return RenderPickOutlines(p, s, cb, sc);
    }
    const uint32_t n = p->w * p->h;
    TimerBegin(p, s, "display");
    hipLaunchKernelGGL(k_display, dim3((n + 255) / 256), dim3(256), 0, s, p->postIn16, p->postIn32, cb->render_width, cb->render_height, p->w, p->h,
        p->exposureIn, prm, lut, p->displayOut.p, p->displaySrgb.p);
    TimerEnd(p, s);
    HIP_TRY(hipGetLastError());
    return RenderPickOutlines(p, s, cb, sc);
}

// DisplayPass::DrawPicked (Display.cpp:293-400) for every pick, in order: WVP = mul(W, VP) on the host, the instance's triangles rasterised into the
// render-size R8 mask, then Sobel.hlsl over the display planes.  The host frustum cull of the reference is left out (an instance outside the frustum
// covers no pixel and outlines nothing either way).
static int RenderPickOutlines(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc)
{
    if (p->picks.empty()) return ZR_OK;
    const uint32_t rw = cb->render_width, rh = cb->render_height;
    if (p->w > 16384 || p->h > 16384 || rw > 16384 || rh > 16384) return Fail(ZR_ERR_INVALID_ARG, "DISPLAY: the picked-instance outline needs display and render sizes <= 16384");
    uint32_t maxTris = 0;
    for (uint32_t idx : p->picks)
    {
        if (idx >= sc->hNumTris.size()) return Fail(ZR_ERR_INVALID_ARG, "DISPLAY: picked instance %u is not an instance of the scene (%zu instances)", idx, sc->hNumTris.size());
        maxTris = std::max(maxTris, sc->hNumTris[idx]);
    }
    int r;
    if (p->pickMaskW != rw || p->pickMaskH != rh)
    {
        if ((r = p->pickMask.Alloc((size_t)rw * rh))) return r;
        p->pickMaskW = rw; p->pickMaskH = rh;
    }
    if (!p->pickCount.p && (r = p->pickCount.Alloc(1))) return r;
    if (p->pickTris.n < 14 * (size_t)maxTris + 2 && (r = p->pickTris.Alloc(14 * (size_t)maxTris + 2))) return r;
    SceneAnimSyncHost(const_cast<zr_scene*>(sc));
    for (uint32_t idx : p->picks)
    {
        // W: the 3x4 object-to-world matrix as the reference's float4x3 (row-vector convention); WVP[i][j] = ((W[i][0] VP[0][j] + W[i][1] VP[1][j]) + W[i][2] VP[2][j]) + W[i][3] VP[3][j]
        const float* M = sc->hToWorld.data() + 12 * (size_t)idx;
        float W[4][4];
        for (int i = 0; i < 4; i++) { for (int j = 0; j < 3; j++) W[i][j] = M[4 * j + i]; W[i][3] = i == 3 ? 1.0f : 0.0f; }
        post::PickWvp m;
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++)
        {
            const float* VP = cb->curr_view_proj;
            const float a = W[i][0] * VP[j], b = W[i][1] * VP[4 + j], c = W[i][2] * VP[8 + j], d = W[i][3] * VP[12 + j];
            m.m[4 * i + j] = ((a + b) + c) + d;
        }
        TimerBegin(p, s, "pick_outline");
        const hipError_t e = LaunchPickOutline(s, sc->vertices.p, sc->indices.p, sc->cur.instances.p, idx, sc->hNumTris[idx], m, p->w, p->h, rw, rh, p->pickTris.p,
            p->pickCount.p, p->pickMask.p, p->displayOut.p, p->displaySrgb.p);
        TimerEnd(p, s);
        HIP_TRY(e);
    }
    return ZR_OK;
}

// TAA::Render (TAA.cpp:75-118): reads the other output as history, then the roles swap
static int RenderTAA(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, zr_gbuffer* gb)
{
    if (!gb || gb->w != p->w || gb->h != p->h) return Fail(ZR_ERR_INVALID_ARG, "TAA needs a gbuffer of the pass size");
    if (cb->render_width != p->w || cb->render_height != p->h) return Fail(ZR_ERR_INVALID_ARG, "TAA: frame constants / pass size mismatch");
    if (!p->compIn[3]) return Fail(ZR_ERR_NOT_INITIALIZED, "TAA: no input bound (zr_pass_set_input(ZR_IN_TAA_SIGNAL))");
    const int curr = 1 - p->taaIdx;
    taa::TaaFrame F;
    F.signal = p->compIn[3]; F.depth = (const float*)gb->Planes()[ZR_GB_DEPTH].p; F.motion = (const uint32_t*)gb->Planes()[ZR_GB_MOTION_VECTOR].p;
    F.prevOut = p->taaOut[p->taaIdx].p; F.currOut = p->taaOut[curr].p; F.w = p->w; F.h = p->h;
    F.blendWeight = p->params.taa_blend_weight; F.temporalIsValid = p->hist.valid ? 1u : 0u;
    const uint32_t n = p->w * p->h;
    TimerBegin(p, s, "taa");
    hipLaunchKernelGGL(k_taa, dim3((n + 255) / 256), dim3(256), 0, s, F);
    TimerEnd(p, s);
    HIP_TRY(hipGetLastError());
    p->taaIdx = curr; p->hist.valid = true;
    return ZR_OK;
}

// Denoise pass: temporal accumulation -> variance estimate -> a-trous iterations (zr_svgf.h; no reference counterpart).
// `steps`: which of them this call runs (ZR_STAGE_DENOISE_*; zr_pass_render = all).  A device of the tile split runs them in groups with halo
// exchanges in between (zetaray_amd/tiling.py denoise_schedule): the planes then cover the tile + its apron, a window of the frame.
static int RenderDenoise(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, zr_gbuffer* gb, uint32_t steps)
{
    if (!gb || gb->w != p->w || gb->h != p->h) return Fail(ZR_ERR_INVALID_ARG, "DENOISE needs a gbuffer of the pass size");
    if (gb->x0 + gb->w > cb->render_width || gb->y0 + gb->h > cb->render_height) return Fail(ZR_ERR_INVALID_ARG, "DENOISE: the planes' window leaves the frame of the frame constants");
    if (!p->compIn[3]) return Fail(ZR_ERR_NOT_INITIALIZED, "DENOISE: no input signal (zr_pass_set_input(pass, ZR_IN_DENOISE_SIGNAL, rgba32f))");
    const zr_params& prm = p->params;
    if (prm.svgf_iterations > 8u || prm.svgf_normal_power_log2 > 16u) return Fail(ZR_ERR_INVALID_ARG, "DENOISE: svgf_iterations must be <= 8, svgf_normal_power_log2 <= 16");
    if (!(prm.svgf_sigma_z > 0.0f) || !(prm.svgf_sigma_l >= 0.0f) || !(prm.svgf_sigma_z < 1e30f) || !(prm.svgf_sigma_l < 1e30f)) return Fail(ZR_ERR_INVALID_ARG, "DENOISE: svgf_sigma_z must be positive, svgf_sigma_l non-negative, both finite");
    const GBuf cur = gb->View(), prev = gb->PrevView();
    svgf::SvgfParams sp; sp.alpha = prm.svgf_alpha; sp.alphaMoments = prm.svgf_alpha_moments; sp.sigmaL = prm.svgf_sigma_l; sp.sigmaZ = prm.svgf_sigma_z;
    sp.normalPowerLog2 = prm.svgf_normal_power_log2; sp.iterations = prm.svgf_iterations;
    svgf::Window win; win.ox = (int)gb->x0; win.oy = (int)gb->y0; win.pw = (int)p->w; win.ph = (int)p->h; win.W = (int)cb->render_width; win.H = (int)cb->render_height;
    const dim3 grid((p->w + 31u) / 32u, (p->h + 7u) / 8u), block(256);
    const bool pow7 = sp.normalPowerLog2 == 7u;
    const int mi = p->svgfMomIdx;      // histMoments = [mi], this frame's = [mi ^ 1]; flipped when the frame's last step has run
    if (steps & ZR_STAGE_DENOISE_TEMPORAL)
    {
        svgf::SvgfFrame T;
        T.signal = p->compIn[3]; T.depth = cur.depth; T.normal = cur.normal; T.motion = cur.motion; T.prevDepth = prev.depth; T.prevNormal = prev.normal;
        T.histColor = p->svgfHist.p; T.histMoments = p->svgfMoments[mi].p; T.accum = p->svgfAccum.p; T.moments = p->svgfMoments[mi ^ 1].p; T.guide = p->svgfGuide.p; T.guideFw = p->svgfGuideFw.p;
        T.win = win; T.temporalValid = (p->hist.valid && gb->numRendered >= 2) ? 1u : 0u; T.prm = sp;
        TimerBegin(p, s, "denoise_temporal");
        hipLaunchKernelGGL(k_svgf_temporal, grid, block, 0, s, T);
        TimerEnd(p, s);
        p->svgfStepsDone = 0;
    }
    svgf::FilterFrame V;
    V.src = p->svgfAccum.p; V.moments = p->svgfMoments[mi ^ 1].p; V.guide = p->svgfGuide.p; V.guideFw = p->svgfGuideFw.p; V.guideZ = cur.depth; V.dst = p->svgfPing.p; V.lenSrc = p->svgfAccum.p;
    V.history = sp.iterations == 0 ? p->svgfHist.p : nullptr; V.win = win; V.step = 1; V.prm = sp;
    V.dstPacked = sp.iterations != 0;      // the planes between two stages hold fp16 colour + normal (zr_svgf.h PackStage); the pass's last stage writes fp32
    if (steps & ZR_STAGE_DENOISE_VARIANCE)
    {
        TimerBegin(p, s, "denoise_variance");
        if (pow7) hipLaunchKernelGGL(k_svgf_variance<7>, grid, block, 0, s, V); else hipLaunchKernelGGL(k_svgf_variance<-1>, grid, block, 0, s, V);
        TimerEnd(p, s);
        p->svgfCur = p->svgfPing.p;
    }
    bool timing = false;
    for (uint32_t it = 0; it < sp.iterations; it++)
    {
        if (!(steps & ZR_STAGE_DENOISE_ATROUS(it))) continue;
        if (!timing) { TimerBegin(p, s, "denoise_atrous"); timing = true; }
        F4* src = p->svgfCur; F4* dst = src == p->svgfPing.p ? p->svgfPong.p : p->svgfPing.p;
        svgf::FilterFrame A = V;
        A.src = src; A.dst = dst; A.moments = nullptr; A.step = 1u << it; A.history = it == 0 ? p->svgfHist.p : nullptr; A.dstPacked = it + 1u != sp.iterations;
        // LDS-staged tiles for the dense iterations: steps 1, 2 and 4 (48 x 24 tile, 36.8 KB per block, for the last).  With definition 2 the iterations that
        // read their taps from the planes are L1-bound (800 B of taps per pixel through 64 B / clk / CU: 0.24 ms at 3840 x 2160 against 0.14 - 0.15 ms from
        // LDS, profiles/r04c_post_sqA.csv); steps 8 and 16 do not fit a tile.  ZR_DENOISE=plain: every iteration from the planes; ZR_DENOISE=lds2: steps 1 and 2 only
        static const int ldsSteps = [] { const char* e = ZR_EXP_ENV("ZR_DENOISE"); return e && !strcmp(e, "plain") ? 0 : (e && !strcmp(e, "lds2") ? 2 : 3); }();
        // the row-loop form of the tap stencil (zr_svgf.h AtrousPixelT) is the default: 5 iterations 0.978 ms against 1.006 ms for the fully unrolled form at
        // 3840 x 2160 (profiles/r04c_post_chain*.jsonl), a fifth of the code; ZR_DENOISE_TAPS=unroll selects the other
        static const bool rowLoop = [] { const char* e = ZR_EXP_ENV("ZR_DENOISE_TAPS"); return !(e && !strcmp(e, "unroll")); }();
#define ZR_SVGF_LAUNCH(K, ...) do { if (!pow7) hipLaunchKernelGGL((K<__VA_ARGS__ -1, true>), grid, block, 0, s, A); else if (rowLoop) hipLaunchKernelGGL((K<__VA_ARGS__ 7, true>), grid, block, 0, s, A); \
            else hipLaunchKernelGGL((K<__VA_ARGS__ 7, false>), grid, block, 0, s, A); } while (0)
        if (it == 0 && ldsSteps >= 1) ZR_SVGF_LAUNCH(k_svgf_atrous_lds, 1,);
        else if (it == 1 && ldsSteps >= 2) ZR_SVGF_LAUNCH(k_svgf_atrous_lds, 2,);
        else if (it == 2 && ldsSteps >= 3) ZR_SVGF_LAUNCH(k_svgf_atrous_lds, 4,);
        else ZR_SVGF_LAUNCH(k_svgf_atrous,);
#undef ZR_SVGF_LAUNCH
        p->svgfCur = dst;
    }
    if (timing) TimerEnd(p, s);
    HIP_TRY(hipGetLastError());
    // the frame is complete when its last step has run: the last a-trous iteration, or the variance stage when there are none
    const uint32_t last = sp.iterations ? ZR_STAGE_DENOISE_ATROUS(sp.iterations - 1u) : (uint32_t)ZR_STAGE_DENOISE_VARIANCE;
    if (steps & last) { p->svgfOut = p->svgfCur; p->svgfMomIdx = mi ^ 1; p->hist.valid = true; }
    return ZR_OK;
}

static int RenderCompositing(zr_pass* p, hipStream_t s, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb)
{
    if (!gb || gb->w != p->w || gb->h != p->h) return Fail(ZR_ERR_INVALID_ARG, "COMPOSITING needs a gbuffer of the pass size");
    if (const zr_pass* sky = p->inscatterSky)
    {
        if (!sky->inscatterOn) return Fail(ZR_ERR_INVALID_ARG, "COMPOSITING is bound to a SKY pass whose inscattering is disabled (zr_pass_set_inscattering)");
        if (sky->device != p->device) return Fail(ZR_ERR_INVALID_ARG, "COMPOSITING and the bound SKY pass live on different devices");
        // (the grid covers the whole screen; the N-way tile split of compositing with it is out of scope)
        if (gb->x0 || gb->y0) return Fail(ZR_ERR_INVALID_ARG, "compositing with inscattering on a tile of the split screen is not supported (gbuffer tile origin %u, %u)", gb->x0, gb->y0);
    }
    const uint32_t n = p->w * p->h;
    TimerBegin(p, s, "compositing");
    // with the firefly filter on (Compositing.cpp: m_filterFirefly) the composited image goes to a scratch plane and the filter writes FINAL
    const bool firefly = (p->params.flags & ZR_COMPOSIT_FIREFLY_FILTER) != 0;
    F4* composited = firefly ? p->firstBOP.p : (F4*)p->finalRGBA.p;
    if (const zr_pass* sky = p->inscatterSky)
    {
        // PostProcessor.cpp:123-136: the grid, its depth range and mapping exponent come from the sky pass as it is now
        const InscatterGridView grid = {sky->inscatterGrid.p, sky->inscatter.numVoxelsX, sky->inscatter.numVoxelsY, sky->inscatter.depthMappingExp,
                                        sky->inscatter.nearZ, sky->inscatter.farZ};
        hipLaunchKernelGGL(k_composite_inscattering, dim3((n + 255) / 256), dim3(256), 0, s, *cb, (const uint16_t*)gb->Planes()[ZR_GB_METALLIC_ROUGHNESS].p,
            (const float*)gb->Planes()[ZR_GB_DEPTH].p, p->compIn[ZR_IN_SKY_DI], p->compIn[ZR_IN_EMISSIVE_DI], p->compIn[ZR_IN_INDIRECT], composited, n,
            FrameView(sc, cb).sky, p->w, grid);
    }
    else
        hipLaunchKernelGGL(k_composite, dim3((n + 255) / 256), dim3(256), 0, s, *cb, (const uint16_t*)gb->Planes()[ZR_GB_METALLIC_ROUGHNESS].p, p->compIn[ZR_IN_SKY_DI],
            p->compIn[ZR_IN_EMISSIVE_DI], p->compIn[ZR_IN_INDIRECT], composited, n, FrameView(sc, cb).sky, p->w);
    TimerEnd(p, s);
    if (firefly)
    {
        TimerBegin(p, s, "firefly_filter");
        hipLaunchKernelGGL(k_firefly, dim3((p->w + kFfW - 1) / kFfW, (p->h + kFfH - 1) / kFfH), dim3(256), 0, s, composited, (const float*)gb->Planes()[ZR_GB_DEPTH].p,
            (F4*)p->finalRGBA.p, p->w, p->h);
        TimerEnd(p, s);
    }
    HIP_TRY(hipGetLastError());
    return ZR_OK;
}

int zr_device_synchronize(int device)
{
    if (int r = RequireDevice(device)) return r;
    HIP_TRY(hipDeviceSynchronize());
    return ZR_OK;
}
int zr_pass_set_frame_overlap(zr_pass* p, zr_gbuffer* gb, int enable)
{
    if (!p || !gb) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_frame_overlap: null argument");
    if (!p->initialized) return Fail(ZR_ERR_NOT_INITIALIZED, "pass not initialised");
    if (p->kind != ZR_PASS_INDIRECT || p->integrator != ZR_INTEGRATOR_RESTIR_PT) return Fail(ZR_ERR_UNSUPPORTED, "frame overlap is a mode of the ReSTIR PT pass");
    if (p->ov.roles.frameOpen) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_set_frame_overlap: call between frames (a frame's last stage has not been enqueued)");
    if (gb->device != p->device) return Fail(ZR_ERR_INVALID_ARG, "gbuffer / pass live on different devices");
    HIP_TRY(hipSetDevice(p->device));
    // (the K12 sorts put off run now, each on its stage's stream: the trackers they would order themselves by are about to forget everything)
    for (int i = 0; i < 2; i++) if (int r = RptRunPendingSort(p, i, p->rptPending[i].stream)) return r;
    HIP_TRY(hipDeviceSynchronize());      // (a host call between frames; the planes allocated below are cleared on the null stream)
    if (enable && !p->res[2].A.p) { if (int r = AllocOverlapPlanes(p)) return r; HIP_TRY(hipDeviceSynchronize()); }
    if (enable && !p->overlapStream) HIP_TRY(hipStreamCreateWithFlags(&p->overlapStream, hipStreamNonBlocking));
    // switching off keeps the plane roles as they stand (the set last written as FINAL stays the one the next frame reads); FINAL goes on in the plane it is in
    p->ov.SetMode(enable != 0, enable == ZR_FRAME_OVERLAP_CARRY);      // (behind the device synchronize above: no stage has a predecessor yet)
    if (enable && gb->numSets == 2)
    {   // the third plane set (never given back: the sets' roles rotate)
        for (int i = 0; i < ZR_GB_COUNT; i++)
            if (int r = gb->planeSets[2][i].AllocZero((size_t)gb->w * gb->h * ZR_GB_PLANE_BYTES[i])) return r;
        HIP_TRY(hipDeviceSynchronize());
        // sets 0 / 1 hold the last two frames and Prev() must go on naming the older of them for whatever pass renders before the next GBUFFER render.
        // cur = 1: Prev() stays 0, the next render takes the fresh set 2.  cur = 0: Prev() becomes 2, so the previous frame moves there from set 1 (with what
        // is known about it) and the next render takes the fresh planes, now in set 1.
        if (gb->cur == 0)
        {
            for (int i = 0; i < ZR_GB_COUNT; i++) gb->planeSets[1][i].Swap(gb->planeSets[2][i]);
            std::swap(gb->plainAt[1], gb->plainAt[2]); std::swap(gb->sceneAt[1], gb->sceneAt[2]); std::swap(gb->renderAt[1], gb->renderAt[2]);
        }
        gb->numSets = 3;
    }
    gb->tracked = enable != 0;
    if (!enable) { for (auto& o : gb->order) o.Reset(); gb->points.Reset(); }
    return ZR_OK;
}
int zr_pass_frame_overlap_stream(zr_pass* p, void** stream)
{
    if (!p || !stream) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (!p->overlapStream) return Fail(ZR_ERR_NOT_INITIALIZED, "frame overlap has never been enabled on this pass (zr_pass_set_frame_overlap)");
    *stream = (void*)p->overlapStream;
    return ZR_OK;
}
int zr_pass_set_owned_rect(zr_pass* p, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h)
{
    if (!p) return Fail(ZR_ERR_INVALID_ARG, "null pass");
    if ((w == 0) != (h == 0)) return Fail(ZR_ERR_INVALID_ARG, "owned rect: width and height must both be 0 (whole tile) or both be positive");
    if (w && ((x0 & 31u) || (y0 & 31u))) return Fail(ZR_ERR_INVALID_ARG, "owned rect origin must be 32-pixel aligned");
    if (w && p->initialized && (w > p->w || h > p->h)) return Fail(ZR_ERR_INVALID_ARG, "owned rect %ux%u larger than the pass %ux%u", w, h, p->w, p->h);
    p->own[0] = x0; p->own[1] = y0; p->own[2] = w; p->own[3] = h;
    return ZR_OK;
}

// ZR_HALO_DENOISE_INPUT: what the temporal step of a tile reads in its apron -- this frame's signal (the bound input plane: its owner shaded it, in the
// layout of the history; null while unbound) and the history the previous frame left (colour + length, moments)
static int DenoiseInputPlanes(const zr_pass* p, HaloPlane* planes)
{
    planes[0] = {(void*)p->compIn[3], p->svgfHist.bpp}; planes[1] = p->svgfHist.Halo(); planes[2] = p->svgfMoments[p->svgfMomIdx].Halo();
    return 3;
}
static size_t HaloBytes(const HaloPlane* planes, int n) { size_t b = 0; for (int i = 0; i < n; i++) b += planes[i].bpp; return b; }
// the planes a halo transfer of this pass moves, and their bytes per pixel
static int HaloPlanes(zr_pass* p, int which, HaloPlane* planes, size_t* bytesPerPixel)
{
    // which reservoir set a transfer addresses (zr_halo_set): between the stages of a frame the post-temporal set is Cur(); after the frame the set the
    // next frame reads as "previous" is Oth() -- of the overlap roles for ReSTIR PT, of the pass's history for the others
    const bool post = which == ZR_HALO_POST_TEMPORAL;
    const int set = post ? p->hist.Cur() : p->hist.Oth();
    int n = 0;
    if (p->kind == ZR_PASS_INDIRECT && p->integrator == ZR_INTEGRATOR_RESTIR_PT) n = PlanesHalo(p->res[post ? p->ov.roles.Cur() : p->ov.roles.Oth()], planes);
    else if (p->kind == ZR_PASS_INDIRECT && p->integrator == ZR_INTEGRATOR_RESTIR_GI) n = PlanesHalo(p->gi[set], planes);
    else if (p->kind == ZR_PASS_DI_EMISSIVE) n = PlanesHalo(p->di[set], planes);
    else if (p->kind == ZR_PASS_DI_SKY) n = PlanesHalo(p->sky[set], planes);
    else if (p->kind == ZR_PASS_DENOISE)
    {
        // ITER: the plane the next a-trous iteration reads (svgfPing or svgfPong)
        if (which == ZR_HALO_DENOISE_INPUT && p->compIn[3]) n = DenoiseInputPlanes(p, planes);
        else if (which == ZR_HALO_DENOISE_ITER) planes[n++] = {p->svgfCur, p->svgfPing.bpp};
    }
    *bytesPerPixel = HaloBytes(planes, n);
    return n;
}
int zr_pass_halo_bytes_per_pixel(zr_pass* p, uint32_t* bytes)
{
    if (!p || !bytes) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    HaloPlane pl[8]; size_t b = 0;
    if (p->initialized && p->kind == ZR_PASS_DENOISE) { *bytes = (uint32_t)HaloBytes(pl, DenoiseInputPlanes(p, pl)); return ZR_OK; }      // the larger of its two exchanges (_ITER moves one plane)
    if (!p->initialized || !HaloPlanes(p, ZR_HALO_FINAL, pl, &b)) return Fail(ZR_ERR_NOT_INITIALIZED, "pass has no reservoir planes to exchange (or is not initialised)");
    *bytes = (uint32_t)b;
    return ZR_OK;
}
static int HaloCopy(zr_pass* p, hipStream_t s, const zr_gbuffer* gb, int which, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* packed, size_t bytes, bool pack)
{
    if (!p || !gb || !packed) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    HaloPlane planes[8]; size_t bpp = 0;
    const int np = p->initialized ? HaloPlanes(p, which, planes, &bpp) : 0;
    if (!np) return Fail(ZR_ERR_NOT_INITIALIZED, "pass has no reservoir planes to exchange (or is not initialised)");
    if (x0 < gb->x0 || y0 < gb->y0 || x0 + w > gb->x0 + gb->w || y0 + h > gb->y0 + gb->h) return Fail(ZR_ERR_INVALID_ARG, "halo rect lies outside this device's planes");
    const size_t n = (size_t)w * h;
    if (bytes != n * bpp) return Fail(ZR_ERR_INVALID_ARG, "halo buffer must hold %zu bytes", n * bpp);
    if (!n) return ZR_OK;
    HIP_TRY(hipSetDevice(p->device));
    char* cursor = (char*)packed;
    const size_t first = (size_t)(y0 - gb->y0) * gb->w + (x0 - gb->x0);
    for (int i = 0; i < np; i++)
    {
        const HaloPlane& pl = planes[i];
        char* tile = (char*)pl.base + first * pl.bpp;
        if (pack) HIP_TRY(hipMemcpy2DAsync(cursor, w * pl.bpp, tile, gb->w * pl.bpp, w * pl.bpp, h, hipMemcpyDeviceToDevice, s));
        else HIP_TRY(hipMemcpy2DAsync(tile, gb->w * pl.bpp, cursor, w * pl.bpp, w * pl.bpp, h, hipMemcpyDeviceToDevice, s));
        cursor += n * pl.bpp;
    }
    return ZR_OK;
}
static int HaloAll(zr_pass* p, hipStream_t s, const zr_gbuffer* gb, int which, const zr_halo_rect* rects, uint32_t n, void* buf, size_t bytes, bool pack)
{
    if (!p || !gb || (n && (!rects || !buf))) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (n > ZR_HALO_MAX_RECTS) return Fail(ZR_ERR_INVALID_ARG, "at most %d rects per fused halo transfer", ZR_HALO_MAX_RECTS);
    HaloPlane planes[8]; size_t bpp = 0;
    const int np = p->initialized ? HaloPlanes(p, which, planes, &bpp) : 0;
    if (!np) return Fail(ZR_ERR_NOT_INITIALIZED, "pass has no reservoir planes to exchange (or is not initialised)");
    if (!n) return ZR_OK;
    HaloJob J; std::memset(&J, 0, sizeof(J));
    J.numPlanes = (uint32_t)np; J.numRects = n; J.pitch = gb->w; J.buf = (char*)buf;
    for (int i = 0; i < np; i++) { J.planes[i].base = (char*)planes[i].base; J.planes[i].bpp = (uint32_t)planes[i].bpp; }
    uint32_t maxPx = 0;
    for (uint32_t i = 0; i < n; i++)
    {
        const zr_halo_rect& r = rects[i];
        if (r.x0 < gb->x0 || r.y0 < gb->y0 || r.x0 + r.w > gb->x0 + gb->w || r.y0 + r.h > gb->y0 + gb->h) return Fail(ZR_ERR_INVALID_ARG, "halo rect %u lies outside this device's planes", i);
        const size_t blk = (size_t)r.w * r.h * bpp;
        if ((r.offset & 15u) || r.offset + blk > bytes) return Fail(ZR_ERR_INVALID_ARG, "halo rect %u: block [%llu, +%zu) must be 16-byte aligned and inside the %zu-byte buffer", i, (unsigned long long)r.offset, blk, bytes);
        // planes are copied with accesses of their own width: a block's plane sections start at sums of w * h * bpp_k (bpp 1 .. 16), which are
        // aligned for every plane when w * h is a multiple of 8 -- strips of 32-px aligned tiles with a 32-px apron always are
        if (((size_t)r.w * r.h) & 7u) return Fail(ZR_ERR_INVALID_ARG, "halo rect %u: w * h must be a multiple of 8 pixels", i);
        J.rects[i].first = (r.y0 - gb->y0) * gb->w + (r.x0 - gb->x0); J.rects[i].w = r.w; J.rects[i].h = r.h; J.rects[i].offset = r.offset;
        maxPx = std::max(maxPx, r.w * r.h);
    }
    HIP_TRY(hipSetDevice(p->device));
    const dim3 grid(std::min<uint32_t>((maxPx + 255) / 256, 1024u), n);
    if (pack) hipLaunchKernelGGL(k_halo<true>, grid, dim3(256), 0, s, J);
    else hipLaunchKernelGGL(k_halo<false>, grid, dim3(256), 0, s, J);
    HIP_TRY(hipGetLastError());
    return ZR_OK;
}
int zr_pass_halo_pack_all(zr_pass* p, void* stream, const zr_gbuffer* gb, int which, const zr_halo_rect* rects, uint32_t n, void* dev_buf, size_t bytes)
{ return HaloAll(p, (hipStream_t)stream, gb, which, rects, n, dev_buf, bytes, true); }
int zr_pass_halo_unpack_all(zr_pass* p, void* stream, const zr_gbuffer* gb, int which, const zr_halo_rect* rects, uint32_t n, const void* dev_buf, size_t bytes)
{ return HaloAll(p, (hipStream_t)stream, gb, which, rects, n, const_cast<void*>(dev_buf), bytes, false); }

int zr_pass_halo_pack(zr_pass* p, void* stream, const zr_gbuffer* gb, int which, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* dev_dst, size_t bytes)
{ return HaloCopy(p, (hipStream_t)stream, gb, which, x0, y0, w, h, dev_dst, bytes, true); }
int zr_pass_halo_unpack(zr_pass* p, void* stream, const zr_gbuffer* gb, int which, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const void* dev_src, size_t bytes)
{ return HaloCopy(p, (hipStream_t)stream, gb, which, x0, y0, w, h, const_cast<void*>(dev_src), bytes, false); }

static int RenderStageInner(zr_pass* p, void* stream, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb, int stages);
int zr_pass_render_stage(zr_pass* p, void* stream, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb, int stages)
{
    if (!p || !cb || !sc) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_render: null argument");
    // stream-ordered scene updates: wait (on the device) for an update enqueued on another stream, and leave an event behind this
    // render for the next update to wait for.  Both are no-ops until the scene has been updated once.
    HIP_TRY(hipSetDevice(p->device));
    int r = SceneAcquireForRender(sc, (hipStream_t)stream);
    if (r) return r;
    // tracked G-buffers (zr_pass_set_frame_overlap): the ReSTIR PT pass orders its stages itself, finer than a whole call; every other reader waits for
    // the planes' GBUFFER render when that ran on another stream and leaves an event behind its reads of both plane sets
    const bool rptPass = p->kind == ZR_PASS_INDIRECT && p->integrator == ZR_INTEGRATOR_RESTIR_PT;
    const bool trackedReader = gb && gb->tracked && p->kind != ZR_PASS_GBUFFER && !rptPass;
    if (trackedReader) { if ((r = gb->AcquireRead((hipStream_t)stream))) return r; }
    r = RenderStageInner(p, stream, cb, sc, gb, stages);
    if (r) return r;
    if (trackedReader) { if ((r = gb->MarkRead(gb->cur, (hipStream_t)stream)) || (r = gb->MarkRead(gb->Prev(), (hipStream_t)stream))) return r; }
    return SceneReleaseAfterRender(sc, (hipStream_t)stream);
}
static int RenderStageInner(zr_pass* p, void* stream, const zr_frame_constants* cb, const zr_scene* sc, zr_gbuffer* gb, int stages)
{
    if (!p || !cb || !sc) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_render: null argument");
    if (!(stages & (ZR_STAGE_ALL | ZR_STAGE_SPATIAL2 | ZR_STAGE_CANDIDATES | ZR_STAGE_TEMPORAL_REUSE | (p && p->kind == ZR_PASS_DENOISE ? ZR_STAGE_DENOISE_MASK : 0)))) return Fail(ZR_ERR_INVALID_ARG, "no stage selected");
    if (!p->initialized) return Fail(ZR_ERR_NOT_INITIALIZED, "pass not initialised (zr_pass_init)");
    if (sc->device != p->device || (gb && gb->device != p->device)) return Fail(ZR_ERR_INVALID_ARG, "scene / gbuffer / pass live on different devices");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    if ((stages & (ZR_STAGE_TEMPORAL | ZR_STAGE_CANDIDATES)) || (p->kind == ZR_PASS_DENOISE && (stages & (ZR_STAGE_SPATIAL | ZR_STAGE_DENOISE_TEMPORAL)))) p->numTimers = 0;      // timings accumulate over the stages of one frame
    {
        const uint32_t off[4] = { cb->base_color_maps_desc_heap_offset, cb->normal_maps_desc_heap_offset,
                                  cb->metallic_roughness_maps_desc_heap_offset, cb->emissive_maps_desc_heap_offset };
        for (int k = 0; k < 4; k++)
            if (sc->maxTex[k] >= 0 && (uint64_t)off[k] + (uint64_t)sc->maxTex[k] >= sc->view.tex.count)
                return Fail(ZR_ERR_INVALID_ARG, "texture table %d: offset %u + index %lld lies outside the scene's %u textures", k, off[k], (long long)sc->maxTex[k], sc->view.tex.count);
    }
    switch (p->kind)
    {
    case ZR_PASS_GBUFFER: return (stages & ZR_STAGE_TEMPORAL) ? RenderGBuffer(p, s, cb, sc, gb) : ZR_OK;
    case ZR_PASS_PRELIGHTING: return (stages & ZR_STAGE_TEMPORAL) ? RenderPreLighting(p, s, cb, const_cast<zr_scene*>(sc)) : ZR_OK;
    case ZR_PASS_INDIRECT: return RenderIndirect(p, s, cb, sc, gb, stages);
    case ZR_PASS_DI_EMISSIVE: return RenderDirectEmissive(p, s, cb, sc, gb, stages);
    case ZR_PASS_DI_SKY: return RenderDirectSky(p, s, cb, sc, gb, stages);
    case ZR_PASS_COMPOSITING: return (stages & ZR_STAGE_SPATIAL) ? RenderCompositing(p, s, cb, sc, gb) : ZR_OK;
    case ZR_PASS_SKY: return RenderSky(p, s, cb, const_cast<zr_scene*>(sc), stages);
    case ZR_PASS_TAA: return (stages & ZR_STAGE_SPATIAL) ? RenderTAA(p, s, cb, gb) : ZR_OK;
    case ZR_PASS_AUTO_EXPOSURE: return (stages & ZR_STAGE_SPATIAL) ? RenderAutoExposure(p, s, cb) : ZR_OK;
    case ZR_PASS_DISPLAY: return (stages & ZR_STAGE_SPATIAL) ? RenderDisplay(p, s, cb, sc, gb) : ZR_OK;
    case ZR_PASS_DENOISE:
    {   // ZR_STAGE_SPATIAL (what zr_pass_render passes): the whole pass; ZR_STAGE_DENOISE_* bits: the steps of a tile's schedule
        const uint32_t steps = ((uint32_t)stages & ZR_STAGE_DENOISE_MASK) | ((stages & ZR_STAGE_SPATIAL) ? (uint32_t)ZR_STAGE_DENOISE_MASK : 0u);
        return steps ? RenderDenoise(p, s, cb, gb, steps) : ZR_OK;
    }
    default: return Fail(ZR_ERR_UNSUPPORTED, "pass kind %d not implemented", p->kind);
    }
}

// The two K12 thread maps of a ReSTIR PT pass are complete when they are asked for, not before.  A stage launches the sort whose map one of its kernels
// reads (Sort_CtT, Sort_StC) and puts the other one off (Sort_TtC, Sort_CtS: zr_pass::RptPendingSort); asking for a map here launches the sort put off for it,
// on the stream of the stage it belongs to -- the stream a consumer of that stage's outputs runs on (zetaray_amd.h) -- so the plane holds what it has always
// held at this point: CtT / TtC after the temporal stage, CtS / StC after a spatial round, whatever the flags, the number of rounds and the overlap mode.
// RptRunPendingSort states why the sort's inputs still stand.  A renderer that never asks pays for neither map.
int zr_pass_get_output(const zr_pass* p, int which, void** dev, uint32_t* w, uint32_t* h, uint32_t* bpp)
{
    if (!p || !dev) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (!p->initialized) return Fail(ZR_ERR_NOT_INITIALIZED, "pass not initialised");
    if (p->kind == ZR_PASS_SKY && which == ZR_OUT_INSCATTERING)
    {
        if (!p->inscatterOn) return Fail(ZR_ERR_INVALID_ARG, "SKY pass: inscattering is disabled (zr_pass_set_inscattering)");
        *dev = p->inscatterGrid.p;
        if (w) *w = p->inscatter.numVoxelsX;
        if (h) *h = p->inscatter.numVoxelsY * kInscatterSlices;
        if (bpp) *bpp = 4;
        return ZR_OK;
    }
    if (p->kind == ZR_PASS_SKY)
    {
        if (which != ZR_OUT_SKY_LUT) return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
        *dev = p->skyLut.p;
        if (w) *w = p->w;
        if (h) *h = p->h;
        if (bpp) *bpp = 4;
        return ZR_OK;
    }
    if (p->kind == ZR_PASS_AUTO_EXPOSURE)
    {
        if (which == ZR_OUT_EXPOSURE) { *dev = p->aeExposure.p; if (w) *w = 1; if (h) *h = 1; if (bpp) *bpp = 8; return ZR_OK; }
        if (which == ZR_OUT_AE_HISTOGRAM) { *dev = p->aeHist.p; if (w) *w = post::kHistBins; if (h) *h = 1; if (bpp) *bpp = 4; return ZR_OK; }
        return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
    }
    if (p->kind == ZR_PASS_DISPLAY && which == ZR_OUT_PICK_MASK)
    {
        if (!p->pickMaskW) return Fail(ZR_ERR_INVALID_ARG, "DISPLAY: no picked instance has been rendered (zr_pass_set_picked_instances)");
        *dev = p->pickMask.p; if (w) *w = p->pickMaskW; if (h) *h = p->pickMaskH; if (bpp) *bpp = 1; return ZR_OK;
    }
    // every other output is a per-pixel plane of the pass's size.  Reservoir outputs name the set the last frame wrote: hist.Oth()
    const int last = p->hist.Oth();
    if (p->kind == ZR_PASS_DISPLAY)
    {
        if (which == ZR_OUT_DISPLAY) p->displayOut.Output(dev, bpp);
        else if (which == ZR_OUT_DISPLAY_SRGB8) p->displaySrgb.Output(dev, bpp);
        else return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
    }
    else if (p->kind == ZR_PASS_DENOISE)
    {
        if (which == ZR_OUT_DENOISED) { *dev = (void*)p->svgfOut; if (bpp) *bpp = (uint32_t)p->svgfPing.bpp; }      // svgfPing or svgfPong
        else if (which == ZR_OUT_DENOISE_HISTORY) p->svgfHist.Output(dev, bpp);
        else if (which == ZR_OUT_DENOISE_MOMENTS) p->svgfMoments[p->svgfMomIdx].Output(dev, bpp);
        else return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
    }
    else if (p->kind == ZR_PASS_TAA)
    {
        if (which != ZR_OUT_TAA) return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
        p->taaOut[p->taaIdx].Output(dev, bpp);
    }
    else if (p->kind == ZR_PASS_COMPOSITING)
    {
        if (which != ZR_OUT_FINAL) return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
        p->finalRGBA.Output(dev, bpp);
    }
    else if (p->kind == ZR_PASS_DI_SKY)
    {
        if (which == ZR_OUT_FINAL) p->finalRGBA.Output(dev, bpp);
        else if (which >= ZR_OUT_SDI_RESERVOIR_A && which <= ZR_OUT_SDI_RESERVOIR_C) PlanesOutput(p->sky[last], which - ZR_OUT_SDI_RESERVOIR_A, dev, bpp);
        else if (which == ZR_OUT_SDI_TARGET) p->diTarget.Output(dev, bpp);
        else return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
    }
    else if (p->kind == ZR_PASS_DI_EMISSIVE)
    {
        if (which == ZR_OUT_FINAL) p->finalRGBA.Output(dev, bpp);
        else if (which >= ZR_OUT_RDI_RESERVOIR_A && which <= ZR_OUT_RDI_RESERVOIR_B) PlanesOutput(p->di[last], which - ZR_OUT_RDI_RESERVOIR_A, dev, bpp);
        else if (which == ZR_OUT_RDI_TARGET) p->diTarget.Output(dev, bpp);
        else return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
    }
    else if (p->kind != ZR_PASS_INDIRECT) return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
    else if (which == ZR_OUT_FINAL) p->FinalPlane(p->ov.roles.finOut).Output(dev, bpp);
    else if (which >= ZR_OUT_RGI_RESERVOIR_A && which <= ZR_OUT_RGI_RESERVOIR_C && p->integrator == ZR_INTEGRATOR_RESTIR_GI)
        PlanesOutput(p->gi[last], which - ZR_OUT_RGI_RESERVOIR_A, dev, bpp);
    else if (which >= ZR_OUT_RPT_RBUF_CTN_A && which <= ZR_OUT_RPT_RBUF_NTC_D && p->integrator == ZR_INTEGRATOR_RESTIR_PT)
        PlanesOutput(p->rb[(which - ZR_OUT_RPT_RBUF_CTN_A) / 4], (which - ZR_OUT_RPT_RBUF_CTN_A) % 4, dev, bpp);
    else if ((which == ZR_OUT_RPT_THREAD_MAP_CTN || which == ZR_OUT_RPT_THREAD_MAP_NTC) && p->integrator == ZR_INTEGRATOR_RESTIR_PT)
    {
        const int idx = which - ZR_OUT_RPT_THREAD_MAP_CTN;
        if (p->rptPending[idx].live)
        {   // (the pass is const for what a caller can see of it: the plane gets the contents it is documented to have)
            HIP_TRY(hipSetDevice(p->device));
            if (int r = RptRunPendingSort(const_cast<zr_pass*>(p), idx, p->rptPending[idx].stream)) return r;
        }
        p->rptMap[idx].Output(dev, bpp);
    }
    else if (which >= ZR_OUT_RPT_RESERVOIR_A && which <= ZR_OUT_RPT_NEIGHBOR && p->integrator == ZR_INTEGRATOR_RESTIR_PT)
    {
        if (which <= ZR_OUT_RPT_RESERVOIR_G) PlanesOutput(p->res[p->ov.roles.Oth()], which - ZR_OUT_RPT_RESERVOIR_A, dev, bpp);      // the set the next frame reads as "previous"
        else if (which == ZR_OUT_RPT_TARGET) p->TargetPlane(p->ov.roles.Target()).Output(dev, bpp);
        else p->rptNeighbor.Output(dev, bpp);
    }
    else return Fail(ZR_ERR_INVALID_ARG, "pass has no such output");
    if (w) *w = p->w;
    if (h) *h = p->h;
    return ZR_OK;
}
int zr_pass_download_output(const zr_pass* p, int which, void* stream, void* dst, size_t bytes)
{
    void* dev = nullptr; uint32_t w, h, bpp;
    // (a thread map may be completed by the call below, on the stream of the stage it belongs to: the copy waits for that stream too)
    const bool isMap = p && p->initialized && p->kind == ZR_PASS_INDIRECT && p->integrator == ZR_INTEGRATOR_RESTIR_PT && (which == ZR_OUT_RPT_THREAD_MAP_CTN || which == ZR_OUT_RPT_THREAD_MAP_NTC);
    const bool sortRuns = isMap && p->rptPending[which - ZR_OUT_RPT_THREAD_MAP_CTN].live;
    const hipStream_t sortStream = sortRuns ? p->rptPending[which - ZR_OUT_RPT_THREAD_MAP_CTN].stream : nullptr;
    int r = zr_pass_get_output(p, which, &dev, &w, &h, &bpp);
    if (r) return r;
    if (!dst || bytes != (size_t)w * h * bpp) return Fail(ZR_ERR_INVALID_ARG, "destination must hold %zu bytes", (size_t)w * h * bpp);
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (sortRuns && sortStream != (hipStream_t)stream) HIP_TRY(hipStreamSynchronize(sortStream));
    HIP_TRY(hipMemcpy(dst, dev, bytes, hipMemcpyDeviceToHost));
    return ZR_OK;
}
// Cost map of a ReSTIR PT pass: wave lifetimes (shader cycles / 16) of K11 / K14 / K16 per 32 x 32-px cell of the pass's planes (cell (0, 0) at the
// plane origin) since the last reset -- the load signal of the cost-balanced screen split (zetaray_amd/tiling.py balanced_layout).  One atomic per wave while enabled.
int zr_pass_enable_cost_map(zr_pass* p, int enable)
{
    if (!p || !p->initialized) return Fail(ZR_ERR_NOT_INITIALIZED, "pass not initialised");
    if (p->kind != ZR_PASS_INDIRECT || p->integrator != ZR_INTEGRATOR_RESTIR_PT) return Fail(ZR_ERR_UNSUPPORTED, "the cost map is an output of the ReSTIR PT pass");
    p->costOn = enable != 0;
    p->costRays = enable == ZR_COST_MAP_RAYS;
    return ZR_OK;
}
int zr_scene_material_class(const zr_scene* s, uint32_t* out)
{
    if (!s || !out) return Fail(ZR_ERR_INVALID_ARG, "zr_scene_material_class: null argument");
    *out = s->plainMaterials.load() ? 1u : 0u;
    return ZR_OK;
}
int zr_debug_set_material_class_kernels(int enable) { g_materialClassKernels.store(enable != 0, std::memory_order_relaxed); return ZR_OK; }
int zr_debug_set_bvh_depth_cap(uint32_t levels) { DeviceBvhSetDepthCap(levels); return ZR_OK; }
int zr_debug_set_large_scene_nodes(uint32_t n) { g_largeSceneNodes.store(n ? n : kLargeSceneNodes, std::memory_order_relaxed); return ZR_OK; }
int zr_pass_debug_trip_stats(zr_pass* p, uint64_t out[3])
{
    if (!p || !out) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    out[0] = out[1] = out[2] = 0;
    if (!p->tripStats.p) return ZR_OK;
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long h[4];
    HIP_TRY(hipMemcpy(h, p->tripStats.p, 32, hipMemcpyDeviceToHost));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2];
    return ZR_OK;
}
int zr_pass_read_cost_map(zr_pass* p, void* stream, uint32_t* out, uint32_t cells_w, uint32_t cells_h, int reset)
{
    if (!p || !out || !p->initialized) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_read_cost_map: bad argument");
    const uint32_t cw = (p->w + 31u) / 32u + 1u, ch = (p->h + 31u) / 32u + 1u;
    if (!p->costMap.p || cells_w != cw || cells_h != ch) return Fail(ZR_ERR_INVALID_ARG, "the cost map is %u x %u cells", cw, ch);
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(out, p->costMap.p, (size_t)cw * ch * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (reset) HIP_TRY(hipMemsetAsync(p->costMap.p, 0, (size_t)cw * ch * 4, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return ZR_OK;
}
// K2's output of the last PRELIGHTING render that estimated powers, after waiting for `stream` (tests and tools)
int zr_pass_get_emissive_powers(zr_pass* p, void* stream, float* out, uint32_t n)
{
    if (!p || !out) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (p->kind != ZR_PASS_PRELIGHTING) return Fail(ZR_ERR_INVALID_ARG, "zr_pass_get_emissive_powers: not a PRELIGHTING pass");
    if (!p->power.p) return Fail(ZR_ERR_NOT_INITIALIZED, "no emissive powers: render the PRELIGHTING pass on a scene without a current alias table first");
    if (n != p->power.n) return Fail(ZR_ERR_INVALID_ARG, "the pass holds the powers of %zu emissive triangles", p->power.n);
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(out, p->power.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return ZR_OK;
}

// frame overlap: K11 may have run on another stream than the one the caller reads its counters on
static int SyncCandidates(zr_pass* p)
{
    hipStream_t k11;
    if (p->ov.CandidatesStream(&k11)) HIP_TRY(hipStreamSynchronize(k11));
    return ZR_OK;
}
int zr_pass_read_counters(zr_pass* p, void* stream, zr_counters* out, int reset)
{
    if (!p || !out) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    out->n_closest = p->hostCounters.n_closest; out->n_shadow = p->hostCounters.n_shadow;
    if ((p->kind == ZR_PASS_INDIRECT || p->kind == ZR_PASS_DI_EMISSIVE || p->kind == ZR_PASS_DI_SKY) && p->initialized)
    {
        unsigned long long c[2 * kCounterSlots];
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        if (int r = SyncCandidates(p)) return r;
        HIP_TRY(hipMemcpy(c, p->counters.p, sizeof(c), hipMemcpyDeviceToHost));
        for (int i = 0; i < kCounterSlots; i++) { out->n_closest += c[2 * i]; out->n_shadow += c[2 * i + 1]; }
        if (reset) { HIP_TRY(hipMemsetAsync(p->counters.p, 0, sizeof(c), (hipStream_t)stream)); HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); }
    }
    if (reset) { p->hostCounters.n_closest = 0; p->hostCounters.n_shadow = 0; }
    return ZR_OK;
}
int zr_pass_read_kernel_counters(zr_pass* p, void* stream, uint32_t max_entries, const char** names, uint64_t* closest, uint64_t* shadow,
    uint32_t* count)
{
    if (!p || !names || !closest || !shadow || !count) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if ((p->kind != ZR_PASS_INDIRECT && p->kind != ZR_PASS_DI_EMISSIVE && p->kind != ZR_PASS_DI_SKY) || !p->initialized) return Fail(ZR_ERR_NOT_INITIALIZED, "pass has no ray counters or is not initialised");
    HIP_TRY(hipSetDevice(p->device));
    unsigned long long c[2 * kCounterSlots];
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (int r = SyncCandidates(p)) return r;
    HIP_TRY(hipMemcpy(c, p->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    uint32_t n = 0;
    for (int i = 0; i < kCounterSlots && n < max_entries; i++)
    {
        if (!kCounterNames[i][0] || (c[2 * i] == 0 && c[2 * i + 1] == 0)) continue;
        names[n] = kCounterNames[i]; closest[n] = c[2 * i]; shadow[n] = c[2 * i + 1]; n++;
    }
    *count = n;
    return ZR_OK;
}
int zr_pass_enable_timing(zr_pass* p, int enable)
{
    if (!p) return Fail(ZR_ERR_INVALID_ARG, "null pass");
    p->timing = enable != 0;
    return ZR_OK;
}
int zr_pass_get_timings(zr_pass* p, uint32_t max_entries, const char** names, float* ms, uint32_t* launches, uint32_t* count)
{
    if (!p || !count) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    p->timerNames.clear(); p->timerMs.clear(); p->timerLaunches.clear();
    for (int i = 0; i < p->numTimers; i++)
    {
        zr_pass::Timer& t = p->timers[i];
        HIP_TRY(hipEventSynchronize(t.b));
        float dt = 0;
        HIP_TRY(hipEventElapsedTime(&dt, t.a, t.b));
        size_t k = 0;
        for (; k < p->timerNames.size(); k++) if (p->timerNames[k] == t.name) break;
        if (k == p->timerNames.size()) { p->timerNames.push_back(t.name); p->timerMs.push_back(0); p->timerLaunches.push_back(0); }
        p->timerMs[k] += dt; p->timerLaunches[k]++;
    }
    *count = (uint32_t)p->timerNames.size();
    for (uint32_t k = 0; k < *count && k < max_entries; k++)
    {
        if (names) names[k] = p->timerNames[k].c_str();
        if (ms) ms[k] = p->timerMs[k];
        if (launches) launches[k] = p->timerLaunches[k];
    }
    return ZR_OK;
}
int zr_pass_destroy(zr_pass* p)
{
    if (!p) return ZR_OK;
    (void)hipSetDevice(p->device);
    for (auto& t : p->timers) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    if (p->powerEv) (void)hipEventDestroy(p->powerEv);
    if (p->powerHost) (void)hipHostFree(p->powerHost);
    if (p->overlapStream) { (void)hipStreamSynchronize(p->overlapStream); (void)hipStreamDestroy(p->overlapStream); }
    delete p;
    return ZR_OK;
}

int zr_trace_closest(const zr_scene* sc, void* stream, const float* d_rays, uint32_t n, uint32_t mask, uint32_t* d_hits)
{
    if (!sc || !d_rays || !d_hits) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (n == 0) return ZR_OK;
    HIP_TRY(hipSetDevice(sc->device));
    const uint32_t grid = std::min<uint32_t>((n + kBlock - 1) / kBlock, 8192u);
    hipLaunchKernelGGL(k_trace_rays, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, FrameView(sc, nullptr), (const F4*)d_rays, n, mask, (U4*)d_hits);
    HIP_TRY(hipGetLastError());
    return ZR_OK;
}
int zr_trace_any(const zr_scene* sc, void* stream, const float* d_rays, uint32_t n, uint32_t mask, uint32_t* d_occ)
{
    if (!sc || !d_rays || !d_occ) return Fail(ZR_ERR_INVALID_ARG, "null argument");
    if (n == 0) return ZR_OK;
    HIP_TRY(hipSetDevice(sc->device));
    const uint32_t grid = std::min<uint32_t>((n + kBlock - 1) / kBlock, 8192u);
    hipLaunchKernelGGL(k_trace_rays_any, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, FrameView(sc, nullptr), (const F4*)d_rays, n, mask, d_occ);
    HIP_TRY(hipGetLastError());
    return ZR_OK;
}

} // extern "C"
