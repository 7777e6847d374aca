// zr_tu_alias.hip -- the device form of the emissive alias table (ZR_ALIAS_BUILD_DEVICE, zr_alias_table_build_device; include/zetaray_amd.h): the powers
// K2 left on the device become the table on the device, on one stream, with nothing read back.  The arithmetic is include/zr_alias.h, the header
// tests/aliasmath compiles for the host, so the table is the header's byte for byte whatever the launch shape: the one float sum runs in the header's
// order in a single wave, everything after it is integer.  Six launches:
//   k_alias_sum       1 wave    Math::KahanSum: 8 lanes x 16 floats per step is a serial recurrence (n / 16 dependent steps); the wave's 64 lanes stage
//                               the loads, 1024 floats at a time, through registers into LDS, lanes j, j + 8, ... all carry lane j's accumulator
//   k_alias_quantise  per light probs, cached_p_orig, w = fixed-point weight; per-block sums of w
//   k_alias_classify  per light S = sum of w, capacities, light / heavy; per-block (lights, deficit, excess)
//   k_alias_scan      per light the prefix sums D and E in class order, each light's rank in its class, the heavies' index list
//   k_alias_assign    per light alias and p_curr by binary search in E (a light) or D (a heavy)
//   k_alias_gather    per light cached_p_alias = cached_p_orig[alias]
// A block reads the per-block partials of ALL blocks before it (n / 256 words: 391 at 100 000 lights) instead of a third pass over them.
#include <hip/hip_runtime.h>
#include "../../include/zr_alias.h"

namespace zr {

static constexpr uint32_t kBlock = 256;
static constexpr uint32_t kSumChunk = 1024;      // floats staged per round of k_alias_sum: 16 per lane, 64 Kahan steps

// what zr::AliasScratchWords sizes, in 64-bit words: [hdr 4 | w n | D n | E n | rank n/2 | heavyIdx n/2 | blockW nb | blockAgg 3 nb]
struct AliasScratch
{
    float* sum; uint64_t* S; uint64_t* nL;
    uint64_t *w, *D, *E; uint32_t *rank, *heavyIdx; uint64_t *blockW, *blockAgg;
};
static uint32_t AliasBlocks(uint32_t n) { return (n + kBlock - 1) / kBlock; }
size_t AliasScratchWords(uint32_t n) { const size_t h = ((size_t)n + 1) / 2; return 4 + 3 * (size_t)n + 2 * h + 4 * (size_t)AliasBlocks(n); }
static AliasScratch Carve(uint64_t* p, uint32_t n)
{
    const size_t h = ((size_t)n + 1) / 2, nb = AliasBlocks(n);
    AliasScratch s;
    s.sum = reinterpret_cast<float*>(p); s.S = p + 1; s.nL = p + 2;
    s.w = p + 4; s.D = s.w + n; s.E = s.D + n;
    s.rank = reinterpret_cast<uint32_t*>(s.E + n); s.heavyIdx = reinterpret_cast<uint32_t*>(s.E + n + h);
    s.blockW = s.E + n + 2 * h; s.blockAgg = s.blockW + nb;
    return s;
}

struct U3 { uint64_t a, b, c; };
__device__ inline U3 Add(const U3& x, const U3& y) { return {x.a + y.a, x.b + y.b, x.c + y.c}; }
// inclusive scan of one U3 per thread over the block (Hillis-Steele in LDS); total = the last thread's value.  Every thread of the block calls it
__device__ inline U3 BlockScan(U3 v, U3* lds, U3* total)
{
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kBlock; off <<= 1)
    {
        U3 o = {0, 0, 0};
        if (t >= off) o = lds[t - off];
        __syncthreads();
        v = Add(v, o); lds[t] = v;
        __syncthreads();
    }
    *total = lds[kBlock - 1];
    __syncthreads();
    return v;
}
// the sum of one u64 per thread over the block, the same value in every thread: a butterfly within each wave, the waves' sums through LDS
__device__ inline uint64_t BlockSum(uint64_t v, uint64_t* lds)
{
    for (int off = 32; off; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t s = 0;
    ZR_UNROLL
    for (uint32_t k = 0; k < kBlock / 64; k++) s += lds[k];
    __syncthreads();
    return s;
}
__device__ inline U3 BlockSum3(const U3& v, uint64_t* lds) { return {BlockSum(v.a, lds), BlockSum(v.b, lds), BlockSum(v.c, lds)}; }
// the sum of p[0 .. cnt), or of the cnt triples at p, the same value in every thread
__device__ inline uint64_t BlockSumOf(const uint64_t* p, uint32_t cnt, uint64_t* lds)
{
    uint64_t v = 0;
    for (uint32_t k = threadIdx.x; k < cnt; k += kBlock) v += p[k];
    return BlockSum(v, lds);
}
__device__ inline U3 BlockSumOf3(const uint64_t* p, uint32_t cnt, uint64_t* lds)
{
    U3 v = {0, 0, 0};
    for (uint32_t k = threadIdx.x; k < cnt; k += kBlock) v = Add(v, U3{p[3 * (size_t)k], p[3 * (size_t)k + 1], p[3 * (size_t)k + 2]});
    return BlockSum3(v, lds);
}

__global__ void __launch_bounds__(64) k_alias_sum(const float* power, uint32_t n, float* sumOut)
{
    __shared__ float buf[kSumChunk];
    __shared__ float foldS[8], foldC[8];
    const uint32_t lane = threadIdx.x, j = lane & 7u;
    const uint32_t numSimd = zral::KahanNumSimd(n);
    float ls = 0.0f, lc = 0.0f;
    float r[kSumChunk / 64];
    ZR_UNROLL
    for (uint32_t m = 0; m < kSumChunk / 64; m++) { const uint32_t k = lane + 64 * m; r[m] = k < numSimd ? power[k] : 0.0f; }
    for (uint32_t base = 0; base < numSimd; base += kSumChunk)
    {
        ZR_UNROLL
        for (uint32_t m = 0; m < kSumChunk / 64; m++) buf[lane + 64 * m] = r[m];
        __syncthreads();
        // the next round's loads fly while this round's steps run
        ZR_UNROLL
        for (uint32_t m = 0; m < kSumChunk / 64; m++) { const uint32_t k = base + kSumChunk + lane + 64 * m; r[m] = k < numSimd ? power[k] : 0.0f; }
        const uint32_t cnt = numSimd - base < kSumChunk ? numSimd - base : kSumChunk;      // a multiple of 16
        // (unrolled: the LDS reads and the V1 + V2 adds of eight steps are issued ahead of the dependent chain, whose order stays the header's)
        _Pragma("unroll 8")
        for (uint32_t t = 0; t < cnt; t += 16) zral::KahanLaneStep(ls, lc, buf[t + j], buf[t + 8 + j]);
        __syncthreads();
    }
    if (lane < 8) { foldS[lane] = ls; foldC[lane] = lc; }
    __syncthreads();
    if (lane == 0)
    {
        float sum = 0.0f, comp = 0.0f;
        for (int k = 0; k < 8; k++) zral::KahanFoldStep(sum, comp, foldS[k], foldC[k]);
        for (uint32_t i = numSimd; i < n; i++) zral::KahanStep(sum, comp, power[i]);
        *sumOut = sum;
    }
}

__global__ void __launch_bounds__(kBlock) k_alias_quantise(const float* power, uint32_t n, const float* sum, zr_alias_entry* out, uint64_t* w, uint64_t* blockW)
{
    __shared__ uint64_t lds[kBlock / 64];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint64_t v = 0;
    if (i < n)
    {
        const float pw = power[i];
        const float p = zral::Prob(pw, zral::SumRcp(*sum, n));
        out[i].cached_p_orig = zral::CachedPOrig(p, n);
        v = zral::Quantise(pw, p, n);
        w[i] = v;
    }
    const uint64_t total = BlockSum(v, lds);
    if (threadIdx.x == 0) blockW[blockIdx.x] = total;
}

// (lights, deficit, excess) of light i
__device__ inline U3 Classify(uint64_t w, uint64_t cap) { return zral::IsLight(w, cap) ? U3{1, cap - w, 0} : U3{0, 0, w - cap}; }

__global__ void __launch_bounds__(kBlock) k_alias_classify(const uint64_t* w, uint32_t n, const uint64_t* blockW, uint32_t nb, uint64_t* blockAgg, uint64_t* S)
{
    __shared__ uint64_t lds[kBlock / 64];
    const uint64_t s = BlockSumOf(blockW, nb, lds);
    if (blockIdx.x == 0 && threadIdx.x == 0) *S = s;
    const zral::Capacity cap = zral::MakeCapacity(s, n);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    U3 v = {0, 0, 0};
    if (i < n) v = Classify(w[i], cap.At(i));
    const U3 total = BlockSum3(v, lds);
    if (threadIdx.x == 0) { blockAgg[3 * (size_t)blockIdx.x] = total.a; blockAgg[3 * (size_t)blockIdx.x + 1] = total.b; blockAgg[3 * (size_t)blockIdx.x + 2] = total.c; }
}

__global__ void __launch_bounds__(kBlock) k_alias_scan(const uint64_t* w, uint32_t n, const uint64_t* S, const uint64_t* blockAgg, uint64_t* D, uint64_t* E, uint32_t* rank,
    uint32_t* heavyIdx, uint64_t* nL)
{
    __shared__ U3 lds[kBlock];
    __shared__ uint64_t ldsSum[kBlock / 64];
    const U3 before = BlockSumOf3(blockAgg, blockIdx.x, ldsSum);
    const zral::Capacity cap = zral::MakeCapacity(*S, n);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    U3 v = {0, 0, 0};
    bool light = false;
    if (i < n) { v = Classify(w[i], cap.At(i)); light = v.a != 0; }
    U3 total;
    const U3 incl = Add(before, BlockScan(v, lds, &total));
    if (i < n)
    {
        // incl.a counts the lights among [0, i]: a light's rank is incl.a - 1, a heavy's i - incl.a; both < n, and the heavies' ranks are dense in [0, n - nL)
        if (light) { const uint32_t a = (uint32_t)incl.a - 1u; rank[i] = a; D[a] = incl.b; }
        else { const uint32_t k = i - (uint32_t)incl.a; rank[i] = k; E[k] = incl.c; heavyIdx[k] = i; }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *nL = before.a + total.a;
}

__global__ void __launch_bounds__(kBlock) k_alias_assign(const uint64_t* w, uint32_t n, const uint64_t* S, const uint64_t* nLp, const uint64_t* D, const uint64_t* E,
    const uint32_t* rank, const uint32_t* heavyIdx, zr_alias_entry* out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const zral::Capacity cap = zral::MakeCapacity(*S, n);
    const uint32_t nL = (uint32_t)*nLp;
    uint32_t alias; float pCurr;
    zral::Assign(i, w[i], cap.At(i), rank[i], D, nL, E, heavyIdx, n - nL, &alias, &pCurr);
    out[i].alias = alias < n ? alias : i;
    out[i].p_curr = pCurr;
}

__global__ void __launch_bounds__(kBlock) k_alias_gather(zr_alias_entry* out, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i].cached_p_alias = out[out[i].alias].cached_p_orig;
}

// power: n floats, out: n entries, scratch: AliasScratchWords(n) words, all on the device of `st`; n >= 1.  Enqueues only
hipError_t LaunchAliasBuild(hipStream_t st, const float* power, uint32_t n, zr_alias_entry* out, uint64_t* scratch)
{
    const AliasScratch s = Carve(scratch, n);
    const uint32_t nb = AliasBlocks(n);
    hipLaunchKernelGGL(k_alias_sum, dim3(1), dim3(64), 0, st, power, n, s.sum);
    hipLaunchKernelGGL(k_alias_quantise, dim3(nb), dim3(kBlock), 0, st, power, n, s.sum, out, s.w, s.blockW);
    hipLaunchKernelGGL(k_alias_classify, dim3(nb), dim3(kBlock), 0, st, s.w, n, s.blockW, nb, s.blockAgg, s.S);
    hipLaunchKernelGGL(k_alias_scan, dim3(nb), dim3(kBlock), 0, st, s.w, n, s.S, s.blockAgg, s.D, s.E, s.rank, s.heavyIdx, s.nL);
    hipLaunchKernelGGL(k_alias_assign, dim3(nb), dim3(kBlock), 0, st, s.w, n, s.S, s.nL, s.D, s.E, s.rank, s.heavyIdx, out);
    hipLaunchKernelGGL(k_alias_gather, dim3(nb), dim3(kBlock), 0, st, out, n);
    return hipGetLastError();
}

} // namespace zr
