// zr_rgi_spatial.h -- the spatial reuse stage of ReSTIR GI (k_rgi_spatial), opt-in through zr_pass_set_rgi_spatial.
//
// The reference has no live counterpart: ReSTIR_GI/PairwiseMIS.hlsli::SpatialResample is never included and its call site is commented
// out, so its ReSTIR GI is temporal-only and that is what k_rgi (zr_rgi.h) restates.  The dead code is this stage's design source (tap
// pattern, neighbour heuristics, pairwise MIS after Bitterli 2022); its arithmetic is DEFINED HERE and held to two checks: the kernel
// equals this same function run on the host bit for bit (tests/rgispatial), and the estimator's mean agrees with the K9 path tracer.
//
// Contract.  One thread per pixel of the owned rect, no wave operations: a pure function of the current G-buffer, the GI reservoir set
// k_rgi wrote this frame (planes A, B, C), the scene and the frame constants.  Nothing is written back to the reservoirs.
//  1. RNG.  Rng::Init(x, y, cb.frame_num ^ kSpatialSalt) with (x, y) the global pixel (tile origin added).  k_rgi seeds every stream of
//     its own with the plain frame number, so no stream is shared.
//  2. Taps.  The 8-point Hammersley table of PairwiseMIS.hlsli:144-154: start index rng.UniformUintBounded(8), rotated by
//     2 pi rng.Uniform() (drawn in this order), scaled by radius_px; tap pixel = rint(pixel + offset).  Up to 4 taps are examined in
//     order, stopping at num_samples accepted.
//  3. A tap is accepted when it lies inside the render rect (and inside this device's planes: beyond the apron behaves like the frame
//     border, as in the temporal search), is not the pixel itself, has a surface (depth != FLT_MAX, not flagged invalid), is not emissive,
//     |dot(n, pos_i - pos)| <= kMaxPlaneDist * z_view, dot(n_i, n) > 0 and |roughness_i - roughness| < 0.2 -- all from the CURRENT
//     G-buffer.  k = the number accepted.
//  4. Reservoirs.  The canonical r_c and every neighbour r_i are read back from the planes (PartialRead_Reuse + PartialRead_Rest), so Lo
//     is half precision for the canonical too.  A reservoir is valid when its ID != 0xffffffff.
//  5. Pairwise MIS, defensive form, with confidence weights M and the reconnection Jacobian J_{q->r} = JacobianReconnectionShift(n2, x1_r,
//     x1_q, x2).  p_s(y) = Luminance(Lo BSDF_s(wi) cos) at surface s; V = the pass's visibility segment from x1 to x2, traced only when
//     the untraced target's luminance exceeds 1e-5.
//       neighbour i valid:  t_i = Lo_i BSDF_c V(x1_c, y_i);  a_i = M_i p_i(y_i) / (M_i p_i(y_i) + (M_c / k) Lum(t_i) J_{i->c}), 0 unless the
//                           denominator is > 0;  w_i = a_i Lum(t_i) W_i J_{i->c};  p_i(y_i) is recomputed at the neighbour's surface without
//                           a trace.  (w_i, y_i, t_i) is streamed into the output reservoir.
//       canonical:          m_c = 1 + sum_i (1 - b_i),  b_i = M_i q_i / (M_i q_i + (M_c / k) p_c(y_c)),  q_i = Lum(Lo_c BSDF_i V(x1_i, y_c)) J_{c->i};
//                           b_i = 0 when r_i is invalid or the denominator is not > 0.  w_c = m_c p_c(y_c) W_c, streamed last.
//     Streaming: w_sum += w, one rng.Uniform() u per streamed sample, the sample is taken when u * w_sum < w (a NaN weight is skipped
//     without a draw).  W = w_sum / (p(selected) (k + 1)), 0 when that is NaN or p(selected) is 0.
//  6. FINAL gets li = target(selected) * W (NaN -> 0) through the pass's store-or-accumulate rule: exactly one contribution per pixel and
//     frame, because k_rgi's own radiance goes to a scratch plane while this stage is on.  Pixels without a shaded surface (invalid,
//     emissive) get what k_rgi gives them: 0 when storing, nothing when accumulating.  Pixels outside the owned rect are not touched.
//  7. While the stage is on k_rgi writes its reservoirs every frame (this kernel reads them).
//  8. The visibility rays count into n_shadow through a counter slot of their own ("rgi_spatial").
#pragma once
#include "zr_rgi.h"

namespace zr {
namespace rgi {

static constexpr uint32_t kSpatialSalt = 0x52475350u;      // "RGSP"
static constexpr uint32_t kSpatialMaxSamples = 2, kSpatialMaxTaps = 4;
static constexpr float kSpatialDefaultRadius = 16.0f, kSpatialMaxRadius = 64.0f, kSpatialMaxRoughDiff = 0.2f;

struct SpatialParams { uint32_t numSamples; float radius; };

// the G-buffer surface of a pixel, as k_rgi builds it (LoadPrimary)
struct SpatialSurface { V3 pos, normal; float roughness, z_view; Surface surface; };
ZR_HD SpatialSurface LoadSpatialSurface(const GiFrame& F, const zr_frame_constants& g, uint32_t x, uint32_t y, size_t px)
{
    Lane L; V2 lens; V3 origin;
    LoadPrimary(F, g, x, y, px, L, lens, origin);
    SpatialSurface s; s.pos = L.pos; s.normal = L.normal; s.roughness = L.roughness; s.z_view = L.z_view; s.surface = L.surface;
    return s;
}

// Lo BSDF_s(wi) cos of the sample at y seen from surface s, untraced; wi / t: the segment s -> y (t == 0: no segment, target 0)
ZR_HD V3 SpatialTarget(const SceneView& sc, const SpatialSurface& s, V3 y, V3 Lo, V3& wi, float& t)
{
    wi = y - s.pos;
    t = dot(wi, wi) == 0 ? 0.0f : length(wi);
    if (!(t > 0)) { wi = v3(0.0f); t = 0; return v3(0.0f); }
    wi = wi / t;
    Surface surface = s.surface;
    surface.SetWi(wi, s.normal);
    return Lo * Unified(sc.rho, surface).f;
}
// ... times V(s, y), traced only when the untraced target is bright enough to matter
ZR_HD V3 SpatialTargetVisible(const Globals& gl, const SpatialSurface& s, V3 y, V3 Lo, uint32_t ID)
{
    V3 wi; float t;
    V3 target = SpatialTarget(*gl.sc, s, y, Lo, wi, t);
    if (Luminance(target) > 1e-5f)
        target = target * (VisibilitySegmentApprox(gl, s.pos, wi, t, s.normal, ID, s.surface.Transmissive()) ? 1.0f : 0.0f);
    return target;
}

struct SpatialOut { V3 target; float w_sum; };
ZR_HD void SpatialStream(SpatialOut& o, float w, V3 target, Rng& rng)
{
    if (zr_isnan(w)) return;
    o.w_sum += w;
    if (rng.Uniform() * o.w_sum < w) o.target = target;
}

ZR_HD void SpatialResample(const GiFrame& F, const zr_frame_constants& g, const SpatialParams& sp, uint32_t x, uint32_t y, TravStack stack, uint32_t* cnt)
{
    if (!F.Owns(x, y)) return;
    const size_t px = Pix(F.gb, x, y);
    float* o = F.finalRGBA + 4 * px;
    {
        const GFlags flags = DecodeFlags(F.gb.mr[px]);
        if (flags.invalid || flags.emissive)
        {
            if (!F.prm.accumulate) { o[0] = 0; o[1] = 0; o[2] = 0; }
            return;
        }
    }
    const int W = (int)g.render_width, H = (int)g.render_height;
    const SpatialSurface c = LoadSpatialSurface(F, g, x, y, px);
    Rng rng = Rng::Init(x, y, g.frame_num ^ kSpatialSalt);

    // 2, 3: the taps
    const float kTapX[8] = {0.0f, -0.5f, 0.5f, -0.75f, 0.25f, -0.25f, 0.75f, -0.875f};
    const uint32_t start = rng.UniformUintBounded(8);
    const float theta = ZR_TWO_PI * rng.Uniform();
    float sinTheta, cosTheta; zr_sincos(theta, &sinTheta, &cosTheta);
    const uint32_t numSamples = sp.numSamples < kSpatialMaxSamples ? sp.numSamples : kSpatialMaxSamples;
    int tapX[kSpatialMaxSamples], tapY[kSpatialMaxSamples];
    uint32_t k = 0;
    for (uint32_t i = 0; i < kSpatialMaxTaps && k < numSamples; i++)
    {
        const uint32_t j = (start + i) & 7u;
        float ux = 0.0f;
        ZR_UNROLL for (uint32_t q = 0; q < 8; q++) ux = j == q ? kTapX[q] : ux;      // (selects, not an indexed table in scratch)
        const float uy = (2.0f * (float)j - 7.0f) / 9.0f;
        const float rx = (ux * cosTheta - uy * sinTheta) * sp.radius, ry = (ux * sinTheta + uy * cosTheta) * sp.radius;
        const int sx = zr_f2i_sat(__builtin_rintf((float)x + rx)), sy = zr_f2i_sat(__builtin_rintf((float)y + ry));
        if (sx < 0 || sy < 0 || sx >= W || sy >= H || !rpt::InPlanes(F.gb, sx, sy)) continue;
        if (sx == (int)x && sy == (int)y) continue;
        const size_t spx = Pix(F.gb, (uint32_t)sx, (uint32_t)sy);
        const GFlags fi = DecodeFlags(F.gb.mr[spx]);
        if (F.gb.depth[spx] == ZR_FLT_MAX || fi.invalid || fi.emissive) continue;
        const SpatialSurface n = LoadSpatialSurface(F, g, (uint32_t)sx, (uint32_t)sy, spx);
        bool ok = zr_abs(dot(c.normal, n.pos - c.pos)) <= kMaxPlaneDist * c.z_view;
        ok = ok && dot(n.normal, c.normal) > 0.0f;
        ok = ok && zr_abs(n.roughness - c.roughness) < kSpatialMaxRoughDiff;
        if (!ok) continue;
        if (k == 0) { tapX[0] = sx; tapY[0] = sy; } else { tapX[1] = sx; tapY[1] = sy; }
        k++;
    }

    Globals gl; gl.sc = &F.sc; gl.frame = &g; gl.emissive = g.num_emissive_triangles != 0; gl.numEmissives = g.num_emissive_triangles; gl.alpha_min = 0;
    gl.stack = stack; gl.cnt = cnt; gl.maxNumBounces = 0; gl.presampled = false; gl.sampleSetIdx = 0;

    // 4: the canonical reservoir, as the planes hold it
    Reservoir r_c = PartialRead_Reuse(F.cur, px);
    PartialRead_Rest(F.cur, px, r_c);
    const bool valid_c = r_c.ID != 0xffffffffu;
    V3 target_c = v3(0.0f);
    if (valid_c) { V3 wi; float t; target_c = SpatialTarget(F.sc, c, r_c.pos, r_c.Lo, wi, t); }
    const float p_c = Luminance(target_c);
    const float Mc_over_k = k ? (float)r_c.M / (float)k : 0.0f;

    // 5: pairwise MIS
    SpatialOut out; out.target = v3(0.0f); out.w_sum = 0.0f;
    float m_c = 1.0f;
    for (uint32_t i = 0; i < k; i++)
    {
        const int sx = i == 0 ? tapX[0] : tapX[1], sy = i == 0 ? tapY[0] : tapY[1];
        const size_t spx = Pix(F.gb, (uint32_t)sx, (uint32_t)sy);
        const SpatialSurface n = LoadSpatialSurface(F, g, (uint32_t)sx, (uint32_t)sy, spx);
        Reservoir r_i = PartialRead_Reuse(F.cur, spx);
        PartialRead_Rest(F.cur, spx, r_i);
        const bool valid_i = r_i.ID != 0xffffffffu;
        if (valid_i)
        {
            const V3 t_i = SpatialTargetVisible(gl, c, r_i.pos, r_i.Lo, r_i.ID);
            const float lum_t = Luminance(t_i);
            const float J_ic = JacobianReconnectionShift(r_i.normal, c.pos, n.pos, r_i.pos);
            V3 wi; float t;
            const float p_i = Luminance(SpatialTarget(F.sc, n, r_i.pos, r_i.Lo, wi, t));
            const float num = (float)r_i.M * p_i;
            const float den = num + Mc_over_k * lum_t * J_ic;
            const float a_i = den > 0 ? num / den : 0.0f;
            SpatialStream(out, a_i * lum_t * r_i.W * J_ic, t_i, rng);
        }
        float b_i = 0.0f;
        if (valid_i && valid_c)
        {
            const float J_ci = JacobianReconnectionShift(r_c.normal, n.pos, c.pos, r_c.pos);
            const float q_i = Luminance(SpatialTargetVisible(gl, n, r_c.pos, r_c.Lo, r_c.ID)) * J_ci;
            const float num = (float)r_i.M * q_i;
            const float den = num + Mc_over_k * p_c;
            b_i = den > 0 ? num / den : 0.0f;
        }
        m_c += 1.0f - b_i;
    }
    SpatialStream(out, m_c * p_c * r_c.W, target_c, rng);

    // 6: the frame's radiance
    const float p_sel = Luminance(out.target);
    float Wout = p_sel > 0 ? out.w_sum / (p_sel * (float)(k + 1u)) : 0.0f;
    Wout = zr_isnan(Wout) ? 0.0f : Wout;
    V3 li = out.target * Wout;
    li = any_nan(li) ? v3(0.0f) : li;
    if (F.prm.accumulate) { o[0] += li.x; o[1] += li.y; o[2] += li.z; }
    else { o[0] = li.x; o[1] = li.y; o[2] = li.z; }
}

} // namespace rgi
} // namespace zr
