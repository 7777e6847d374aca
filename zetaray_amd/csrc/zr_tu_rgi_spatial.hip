// zr_tu_rgi_spatial.hip -- translation unit of libzetaray_amd.so holding k_rgi_spatial, the opt-in spatial reuse stage of ReSTIR GI
// (stage function + contract: zr_rgi_spatial.h; launch: zr_api.hip RenderReSTIR_GI).  General material class only: a PLAIN permutation
// is added when it is measured to pay.
#include "zr_kernels.h"
#include "zr_rgi_spatial.h"
// One thread per pixel of the owned rect, 16 x 16 tiles like k_rgi, 256-thread blocks: every wave does the same work (K14 / K16 keep 256 for that
// reason, zr_kernels.h kRptBlock).  Up to two 40-byte reservoir gathers and four visibility rays per pixel: latency-bound like the reconnect
// kernels, so it starts from their occupancy target (-DZR_WAVES_RGI_SPATIAL_N=n to measure another, 0 = the compiler's choice).
#ifndef ZR_WAVES_RGI_SPATIAL_N
#define ZR_WAVES_RGI_SPATIAL_N 4
#endif
#if ZR_WAVES_RGI_SPATIAL_N
#define ZR_WAVES_RGI_SPATIAL ZR_WAVES(ZR_WAVES_RGI_SPATIAL_N)
#else
#define ZR_WAVES_RGI_SPATIAL
#endif
__global__ void __launch_bounds__(kBlock) ZR_WAVES_RGI_SPATIAL k_rgi_spatial(rgi::GiFrame F, zr_frame_constants g, uint32_t tilesX, unsigned long long* counters, rgi::SpatialParams sp)
{
    F.prm.textured = 0u;
    F.sc.plain = false; F.gb.plain = false; F.gbPrev.plain = false;
    uint32_t x, y; PixelOfThreadB<kBlock>(tilesX, F.ox0, F.oy0, &x, &y);
    ZR_TRAV_STACK_B(stack, kBlock);
    uint32_t cnt[2] = {0u, 0u};
    rgi::SpatialResample(F, g, sp, x, y, stack, cnt);
    FlushRayCounters(counters, cnt);
}
