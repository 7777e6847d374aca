/*
 * zr_alias.h -- the emissive alias table of ZR_ALIAS_BUILD_DEVICE, stated once for the host and the device.
 *
 * The reference builds its light-sampling table on the CPU with Vose's method over LIFO index stacks (BuildAliasTable, PreLighting.cpp:27-158; restated
 * as zr_alias_table_build).  Its residual chain is rounded sequentially, so no parallel build reproduces its bytes.  This header defines ANOTHER valid
 * table for the same powers -- this repository's, not the reference's -- whose every byte is a function of the powers alone: zr_tu_alias.hip compiles
 * these functions for the device, tests/aliasmath for the host, and under the arithmetic contract of zr_detmath.h the two give the same bytes, whatever
 * the launch shape.
 *
 * 1. Normalise -- the reference's arithmetic.
 *    sum = Math::KahanSum (Math/Common.cpp:72-139) in its AVX2 lane structure for a 32-byte aligned array: eight independent Kahan lanes, lane j taking
 *    data[c + j] + data[c + 8 + j] for c = 0, 16, 32, ... while 16 floats remain (KahanLaneStep), then the serial fold of the eight lanes into the scalar
 *    accumulator (KahanFoldStep), then the scalar tail (KahanStep).  sumRcp = (float)N / sum, probs[i] = power[i] * sumRcp,
 *    cached_p_orig[i] = probs[i] * (1.0f / N).  cached_p_orig is zr_alias_table_build's value in every bit: a consumer of the light pdf reads the
 *    reference's value in either mode.
 *
 * 2. Assign -- integer fixed point, so that every sum is associative.
 *    w[i] = Quantise(power[i], probs[i]): probs[i] * 2^32 rounded half up to an integer; a positive power gets at least 1 unit, a zero power exactly 0;
 *    clamped to N 2^33, twice what a guaranteed input can reach (probs[i] <= N (1 + 2^-22)), so the clamp never touches one.
 *    S = sum of w.  The buckets' capacities are C[i] = S / N + (i < S % N): integers that sum to S exactly, so the sweep below closes exactly and the
 *    common rounding error of sum and sumRcp cancels (the table represents w[i] / S).
 *    Light i is LIGHT when w[i] < C[i], else HEAVY.  In index order, the lights' deficits d = C - w have the inclusive prefix sums D[0 .. nL) and the
 *    heavies' excesses e = w - C the inclusive prefix sums E[0 .. nH); D[nL - 1] == E[nH - 1].
 *      - The a-th light (its exclusive prefix Dx = a ? D[a - 1] : 0) aliases to the FIRST heavy k with E[k] > Dx; p_curr = w / C.
 *      - The k-th heavy: c = the number of lights whose exclusive prefix is < E[k], Dc = c ? D[c - 1] : 0; it keeps r = C + E[k] - Dc units of its own
 *        (0 <= r <= C: Dc >= E[k] because the next light starts at Dc, Dc < E[k] + C because that light's deficit is <= its capacity); p_curr = r / C.
 *        With r == C it aliases to itself (p_curr == 1: the last heavy always, every light of an all-equal set), else to heavy k + 1, which exists
 *        because Dc > E[k] leaves supply behind k.
 *    The quotients are formed in double (both operands are < 2^53 for N < 2^20, so exact) and rounded to float once.  After the prefix sums every entry is
 *    independent of the others.  cached_p_alias[i] = cached_p_orig[alias[i]].
 *    (Capacities of exactly 2^32 with the residue N 2^32 - S added to one light would not do: that residue is N times the common rounding error of sum
 *    and sumRcp, up to N 2^8 units, and for all-equal powers whose probs round to 1 - 2^-24 it turns light 0 into the one heavy of the set.)
 *    Mass check: heavy k hands d to each of its lights and C[k-1] - r[k-1] to heavy k - 1 and keeps r[k]; these add up to C[k] + e[k] = w[k].
 *
 * Deviations from the reference: the assignment (2) is not Vose's; phase 0 of KahanSum only (the reference's allocations are 32-byte aligned).
 * Caller guarantee, as for the host build: powers finite and non-negative with a positive sum.  For any other input the bytes are unspecified, but every
 * alias is < n, nothing is written out of bounds and nothing loops: NaN quantises to 0 and +inf to the clamp, and where the sums of such weights wrap
 * around 2^64 (only outside the guarantee, whose S is about N 2^32) the counts, ranks and the heavies' index list -- all that ever indexes memory -- do
 * not depend on them, the two searches are bounded by the counts, and p_curr is a quotient r / C with r < C, or 1.
 * Byte equality host == device holds for the contract build; under -DZR_ARITH_FAST the divide differs in sumRcp, which (2) cancels up to rounding.
 */
#ifndef ZR_ALIAS_H
#define ZR_ALIAS_H

#include "zr_detmath.h"
#include "zr_wire.h"
#include <vector>

namespace zral {

/* ---- 1. Math::KahanSum */
ZR_HD void KahanStep(float& sum, float& comp, float v)
{
    const float corrected = v - comp;
    const float newSum = sum + corrected;
    comp = (newSum - sum) - corrected;
    sum = newSum;
}
/* one AVX2 step of one lane: vCurr = V1 + V2, then the Kahan update */
ZR_HD void KahanLaneStep(float& sum, float& comp, float v1, float v2) { KahanStep(sum, comp, v1 + v2); }
/* the fold of one lane's (sum, compensation) into the scalar accumulator: corrected = simdSum - compensation - simdComp */
ZR_HD void KahanFoldStep(float& sum, float& comp, float laneSum, float laneComp)
{
    const float corrected = laneSum - comp - laneComp;
    const float newSum = sum + corrected;
    comp = (newSum - sum) - corrected;
    sum = newSum;
}
/* floats covered by the eight lanes */
ZR_HD uint32_t KahanNumSimd(uint32_t n) { return n - (n & 15u); }
ZR_HD float KahanSum(const float* data, uint32_t n)
{
    float ls[8], lc[8];
    for (int j = 0; j < 8; j++) ls[j] = lc[j] = 0.0f;
    const uint32_t numSimd = KahanNumSimd(n);
    for (uint32_t c = 0; c < numSimd; c += 16)
        for (int j = 0; j < 8; j++) KahanLaneStep(ls[j], lc[j], data[c + j], data[c + 8 + j]);
    float sum = 0.0f, comp = 0.0f;
    for (int j = 0; j < 8; j++) KahanFoldStep(sum, comp, ls[j], lc[j]);
    for (uint32_t i = numSimd; i < n; i++) KahanStep(sum, comp, data[i]);
    return sum;
}
ZR_HD float SumRcp(float sum, uint32_t n) { return (float)n / sum; }
ZR_HD float Prob(float power, float sumRcp) { return power * sumRcp; }
ZR_HD float CachedPOrig(float prob, uint32_t n) { return prob * (1.0f / (float)n); }

/* ---- 2. fixed point */
ZR_HD uint64_t Quantise(float power, float prob, uint32_t n)
{
    const double cap = (double)((uint64_t)n << 33);
    const double d = (double)prob * 4294967296.0 + 0.5;
    uint64_t w = d > 0.0 ? (d < cap ? (uint64_t)d : (uint64_t)cap) : 0ull;      /* NaN -> 0 */
    if (w == 0 && power > 0.0f) w = 1;
    if (!(power > 0.0f)) w = 0;
    return w;
}
struct Capacity
{
    uint64_t base; uint32_t rem;      /* S / n, S % n */
    ZR_HDM uint64_t At(uint32_t i) const { return base + (i < rem ? 1u : 0u); }
};
ZR_HD Capacity MakeCapacity(uint64_t S, uint32_t n) { Capacity c; c.base = S / n; c.rem = (uint32_t)(S % n); return c; }
ZR_HD bool IsLight(uint64_t w, uint64_t cap) { return w < cap; }
ZR_HD float Ratio(uint64_t num, uint64_t den) { return (float)((double)num / (double)den); }

/* the first k in [0, nH) with E[k] > x; nH - 1 when there is none (outside the caller guarantee only) */
ZR_HD uint32_t FirstHeavyAbove(const uint64_t* E, uint32_t nH, uint64_t x)
{
    uint32_t lo = 0, hi = nH;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (E[mid] > x) hi = mid; else lo = mid + 1; }
    return lo < nH ? lo : nH - 1;
}
/* the number of lights a in [0, nL) whose exclusive prefix (a ? D[a - 1] : 0) is < x */
ZR_HD uint32_t LightsStartedBelow(const uint64_t* D, uint32_t nL, uint64_t x)
{
    uint32_t lo = 0, hi = nL;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((mid ? D[mid - 1] : 0ull) < x) lo = mid + 1; else hi = mid; }
    return lo;
}
/* entry of light i, the rank-th of its class.  heavyIdx[k]: the index of the k-th heavy */
ZR_HD void Assign(uint32_t i, uint64_t w, uint64_t cap, uint32_t rank, const uint64_t* D, uint32_t nL, const uint64_t* E, const uint32_t* heavyIdx, uint32_t nH,
    uint32_t* alias, float* pCurr)
{
    if (IsLight(w, cap))
    {
        const uint64_t Dx = rank ? D[rank - 1] : 0ull;
        *alias = nH ? heavyIdx[FirstHeavyAbove(E, nH, Dx)] : i;
        *pCurr = Ratio(w, cap);
        return;
    }
    const uint64_t Ek = E[rank];
    const uint32_t c = LightsStartedBelow(D, nL, Ek);
    const uint64_t Dc = c ? D[c - 1] : 0ull;
    const uint64_t have = cap + Ek;
    const uint64_t r = Dc <= Ek ? cap : (Dc < have ? have - Dc : 0ull);
    if (r >= cap || rank + 1 >= nH) { *alias = i; *pCurr = 1.0f; return; }
    *alias = heavyIdx[rank + 1];
    *pCurr = Ratio(r, cap);
}

/* ---- the whole build on the host, in index order */
static inline void Build(const float* power, uint32_t n, zr_alias_entry* out)
{
    if (n == 0) return;
    const float sumRcp = SumRcp(KahanSum(power, n), n);
    std::vector<uint64_t> w(n), D, E; std::vector<uint32_t> rank(n), heavyIdx;
    uint64_t S = 0;
    for (uint32_t i = 0; i < n; i++)
    {
        const float p = Prob(power[i], sumRcp);
        out[i].cached_p_orig = CachedPOrig(p, n);
        w[i] = Quantise(power[i], p, n); S += w[i];
    }
    const Capacity cap = MakeCapacity(S, n);
    uint64_t d = 0, e = 0;
    for (uint32_t i = 0; i < n; i++)
    {
        const uint64_t c = cap.At(i);
        if (IsLight(w[i], c)) { rank[i] = (uint32_t)D.size(); d += c - w[i]; D.push_back(d); }
        else { rank[i] = (uint32_t)E.size(); e += w[i] - c; E.push_back(e); heavyIdx.push_back(i); }
    }
    for (uint32_t i = 0; i < n; i++)
        Assign(i, w[i], cap.At(i), rank[i], D.data(), (uint32_t)D.size(), E.data(), heavyIdx.data(), (uint32_t)E.size(), &out[i].alias, &out[i].p_curr);
    for (uint32_t i = 0; i < n; i++) out[i].cached_p_alias = out[out[i].alias].cached_p_orig;
}

} /* namespace zral */

#endif /* ZR_ALIAS_H */
