// zr_tu_sky.hip -- translation unit of libzetaray_amd.so holding the inscattering voxel grid of the sky pass (RP/Sky/Inscattering.hlsl):
// the kernel and its launch.  The per-voxel math is in zr_sky.h; zr_api.hip calls LaunchInscattering from the SKY pass's render.
#include "zr_kernels.h"

namespace {

constexpr int kInscatterBlock = (int)kInscatterSlices;      // the reference's group: 128 threads along z, one group per (x, y) column

// WavePrefixSum over the lane's 32-lane segment (Gidx & ~31; [WaveSize(32)] on a wave64), pinned in include/zetaray_amd.h (ZR_PASS_SKY): the values
// shifted up one lane (lane 0 of the segment = 0), then a Hillis-Steele inclusive scan with offsets 1, 2, 4, 8, 16 (a lane adds lane - s when lane >= s)
__device__ __forceinline__ float SegmentPrefixSum(float v, uint32_t l)
{
    float x = __shfl_up(v, 1u, 32);
    if (l == 0u) x = 0.0f;
#pragma unroll
    for (uint32_t s = 1u; s < 32u; s <<= 1)
    {
        const float t = __shfl_up(x, s, 32);
        if (l >= s) x = x + t;
    }
    return x;
}

// Inscattering.hlsl:115-205: block = column (blockIdx.x, blockIdx.y), thread = slice.  Two wave64s, each holding two of the shader's 32-lane waves.
// The visibility ray (:44-64) is an any-hit query over ZR_SUBGROUP_ALL with tmin = 0, tmax = FLT_MAX and RAY_FLAG_CULL_NON_OPAQUE.
__global__ void __launch_bounds__(kInscatterBlock) ZR_WAVES(8) k_inscattering(SceneView sc, zr_frame_constants g, InscatterParams c, uint32_t* grid)
{
    __shared__ V3 sWaveTr[kInscatterBlock / 32], sWaveLs[kInscatterBlock / 32];      // g_waveTr / g_waveLs (only 128 / 32 entries are used)
    ZR_TRAV_STACK_B(stack, kInscatterBlock);
    const uint32_t x = blockIdx.x, y = blockIdx.y, z = threadIdx.x;
    const uint32_t l = z & 31u;

    V3 rayDirVS, rayDirWS;
    InscatterRay(g, c, x, y, rayDirVS, rayDirWS);
    float ds;
    const V3 voxelPos = VoxelPosition(g, c, z, rayDirVS, rayDirWS, ds);
    const V3 sigma_s_rayleigh = v3p(g.rayleigh_sigma_s_color) * g.rayleigh_sigma_s_scale;
    const float sigma_t_mie = g.mie_sigma_a + g.mie_sigma_s;
    const V3 sigma_t_ozone = v3p(g.ozone_sigma_a_color) * g.ozone_sigma_a_scale;

    auto visibility = [&](V3 pos, V3 wi) -> float
    {
        const RawHit h = TraverseDyn<true>(sc, pos, wi, 0.0f, ZR_FLT_MAX, ZR_SUBGROUP_ALL, stack, /*anyHit*/ true);
        return h.tri != kInvalidTri ? 0.0f : 1.0f;
    };
    V3 density, LoTransmittance;
    ComputeVoxelData(g, voxelPos, sigma_s_rayleigh, sigma_t_mie, sigma_t_ozone, visibility, LoTransmittance, density);

    auto prefix = [&](V3 v) { return v3(SegmentPrefixSum(v.x, l), SegmentPrefixSum(v.y, l), SegmentPrefixSum(v.z, l)); };
    V3 tr, Ls;
    Integrate(g, rayDirWS, ds, sigma_s_rayleigh, g.mie_sigma_s, sigma_t_mie, sigma_t_ozone, LoTransmittance, density, prefix, tr, Ls);

    // :177-185: lane 31 of each segment publishes the segment's totals
    const uint32_t waveIdx = z >> 5;
    if (l == 31u) { sWaveTr[waveIdx] = tr; sWaveLs[waveIdx] = Ls; }
    __syncthreads();
    Ls = CombineSegments(Ls, sWaveTr, sWaveLs, waveIdx);
    grid[((size_t)z * c.numVoxelsY + y) * c.numVoxelsX + x] = InscatterTexel(g, Ls);
}

} // namespace

namespace zr {
// the grid is numVoxelsX x numVoxelsY x 128 R11G11B10_FLOAT texels, x fastest, then y, then the slice
hipError_t LaunchInscattering(hipStream_t s, const SceneView& sc, const zr_frame_constants& g, const InscatterParams& c, uint32_t* grid)
{
    hipLaunchKernelGGL(k_inscattering, dim3(c.numVoxelsX, c.numVoxelsY), dim3(kInscatterBlock), 0, s, sc, g, c, grid);
    return hipGetLastError();
}
} // namespace zr
