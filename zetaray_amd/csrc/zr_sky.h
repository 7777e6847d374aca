// zr_sky.h -- the sky model on the device: atmosphere integrals, the sky-view LUT texel (K17) and the radiance lookups.
//
// Restates (device code; the CPU restatement used by the tests is oracle/zro_sky.h):
//   Source/ZetaRenderPass/Common/Volumetric.hlsli:34-229   phase functions, densities, EstimateTransmittance, EstimateLs
//   Source/ZetaRenderPass/Sky/SkyViewLUT.hlsl:19-63        K17: one thread per LUT texel, non-linear latitude, R11G11B10_FLOAT store
//   Source/ZetaRenderPass/Common/LightSource.hlsli:139-199 Le_Sun (6-step transmittance), Le_Sky (LUT lookup), Le_SkyWithSunDisk
//   Source/ZetaRenderPass/Sky/Inscattering.hlsl:32-204      the inscattering voxel grid's per-voxel math (kernel: zr_tu_sky.hip)
//   Source/ZetaRenderPass/Compositing/Compositing.hlsl:74-97 the grid's term in compositing
// Pinned where D3D leaves it open (include/zetaray_amd.h, ZR_PASS_SKY): the store rounds to R11G11B10_FLOAT to nearest even;
// g_samLinearWrap = fp32 bilinear, texel centres at (i + 0.5) / N, wrap addressing on both axes.
// K17 is ALU-bound by construction: 32 x (8 + 1) exp3 evaluations per texel, 4 bytes written.
#pragma once
#include "zr_dev_math.h"
#include "../../include/zr_wire.h"

namespace zr {

ZR_HD float RayleighPhaseFunction(float cosTheta) { return 0.0596831f * (1.0f + cosTheta * cosTheta); }
ZR_HD float SchlickPhaseFunction(float cosTheta, float g)
{
    float k = 1.55f * g - 0.55f * g * g * g;
    float denom = 1.0f - k * cosTheta;
    return ZR_ONE_OVER_4_PI * (1.0f - k * k) / (denom * denom);
}
// altitude in km: (Rayleigh, Mie, ozone) densities, Volumetric.hlsli:66-88
ZR_HD V3 AtmosphereDensity(float altitude)
{
    return v3(zr_exp(-zr_max(0.0f, altitude / 8.0f)), zr_exp(-zr_max(0.0f, altitude / 1.2f)),
        zr_max(0.0f, 1 - zr_abs(altitude - 25.0f) / 15.0f));
}
ZR_HD float IntersectRayAtmosphere(float radius, V3 rayOrigin, V3 rayDir)     // :101-112
{
    float mDotdir = dot(rayDir, rayOrigin);
    float delta = mDotdir * mDotdir - dot(rayOrigin, rayOrigin) + radius * radius;
    delta = zr_sqrt(delta);
    return -mDotdir + delta;
}
ZR_HD bool IntersectRayPlanet(float radius, V3 rayOrigin, V3 rayDir, float& t) // :114-132
{
    float mDotdir = dot(rayDir, rayOrigin);
    float delta = mDotdir * mDotdir - dot(rayOrigin, rayOrigin) + radius * radius;
    if (delta < 0.0f) { t = 0; return false; }
    delta = zr_sqrt(delta);
    t = zr_min(-mDotdir - delta, -mDotdir + delta);
    return t >= 0.0f;
}
ZR_HD V3 EstimateTransmittance(float planetRadius, V3 rayOrigin, V3 rayDir, float t, V3 sigma_t_rayleigh, float sigma_t_mie,
    V3 sigma_t_ozone, int numSteps)                                           // :137-170
{
    if (t <= 1e-5f) return v3(1.0f);
    const float stepSize = t / (float)numSteps;
    V3 pos = rayOrigin + 0.5f * stepSize * rayDir;
    V3 opticalThickness = v3(0.0f);
    for (int s = 0; s < numSteps; s++)
    {
        opticalThickness = opticalThickness + AtmosphereDensity(length(pos) - planetRadius);
        pos = pos + stepSize * rayDir;
    }
    opticalThickness = sigma_t_rayleigh * opticalThickness.x + v3(sigma_t_mie * opticalThickness.y) + sigma_t_ozone * opticalThickness.z;
    opticalThickness = opticalThickness * stepSize;
    return vexp(-opticalThickness);
}
ZR_HD V3 EstimateLs(float planetRadius, V3 rayOrigin, V3 rayDir, V3 lightDir, float atmosphereHeight, float g,
    V3 sigma_s_rayleigh, float sigma_s_mie, float sigma_t_mie, V3 sigma_t_ozone, int numSteps)   // :173-229
{
    float t = IntersectRayAtmosphere(planetRadius + atmosphereHeight, rayOrigin, rayDir);
    float tPlanet;
    if (IntersectRayPlanet(planetRadius, rayOrigin, rayDir, tPlanet)) t = tPlanet;
    const float stepSize = t / (float)numSteps;
    V3 pos = rayOrigin + 0.5f * stepSize * rayDir;
    V3 opticalThickness = v3(0.0f), LsRayleigh = v3(0.0f), LsMie = v3(0.0f);
    for (int s = 0; s < numSteps; s++)
    {
        V3 density = AtmosphereDensity(length(pos) - planetRadius);
        opticalThickness = opticalThickness + density * stepSize;
        V3 rayOriginToPosTr = vexp(-(sigma_s_rayleigh * opticalThickness.x + v3(sigma_t_mie * opticalThickness.y) + sigma_t_ozone * opticalThickness.z));
        const float posToAtmosphereDist = IntersectRayAtmosphere(planetRadius + atmosphereHeight, pos, -lightDir);
        V3 LoTranmittance = EstimateTransmittance(planetRadius, pos, -lightDir, posToAtmosphereDist, sigma_s_rayleigh, sigma_t_mie, sigma_t_ozone, 8);
        LsRayleigh = LsRayleigh + rayOriginToPosTr * density.x * LoTranmittance;
        LsMie = LsMie + rayOriginToPosTr * density.y * LoTranmittance;
        pos = pos + stepSize * rayDir;
    }
    const float cosTheta = dot(lightDir, -rayDir);
    V3 Ls = LsRayleigh * sigma_s_rayleigh * RayleighPhaseFunction(cosTheta);
    Ls = Ls + LsMie * sigma_s_mie * SchlickPhaseFunction(cosTheta, g);
    Ls = Ls * stepSize;
    return Ls;
}

// K17: texel (x, y) of a w x h sky-view LUT, SkyViewLUT.hlsl:19-63
ZR_HD uint32_t SkyViewLutTexel(const zr_frame_constants& g, uint32_t x, uint32_t y, uint32_t w, uint32_t h)
{
    float phi = ((float)x / (float)w);
    phi *= ZR_TWO_PI;
    float v = ((float)y / (float)h);
    float s = v >= 0.5f ? 1.0f : -1.0f;
    float a = v - 0.5f;
    float theta = a * a * ZR_TWO_PI * s + ZR_PI_OVER_2;
    float sinTheta = zr_sin(theta);
    V3 wdir = v3(1.0f * sinTheta * zr_cos(phi), 1.0f * zr_cos(theta), -1.0f * sinTheta * zr_sin(phi));   // Math::SphericalToCartesian
    const V3 sigma_s_rayleigh = v3p(g.rayleigh_sigma_s_color) * g.rayleigh_sigma_s_scale;
    const float sigma_t_mie = g.mie_sigma_a + g.mie_sigma_s;
    const V3 sigma_t_ozone = v3p(g.ozone_sigma_a_color) * g.ozone_sigma_a_scale;
    V3 rayOrigin = v3(0.0f, g.planet_radius + 0.2f, 0.0f);
    V3 Ls = EstimateLs(g.planet_radius, rayOrigin, wdir, v3p(g.sun_dir), g.atmosphere_altitude, g.g, sigma_s_rayleigh,
        g.mie_sigma_s, sigma_t_mie, sigma_t_ozone, 32);
    Ls = Ls * g.sun_illuminance;
    return PackR11G11B10F(v3(zr_max(Ls.x, 0.0f), zr_max(Ls.y, 0.0f), zr_max(Ls.z, 0.0f)));
}

struct SkyLutView { const uint32_t* data; uint32_t w, h; };

ZR_HD V3 Le_Sun(V3 pos, const zr_frame_constants& g)        // LightSource.hlsli:139-157
{
    const V3 sigma_t_rayleigh = v3p(g.rayleigh_sigma_s_color) * g.rayleigh_sigma_s_scale;
    const float sigma_t_mie = g.mie_sigma_a + g.mie_sigma_s;
    const V3 sigma_t_ozone = v3p(g.ozone_sigma_a_color) * g.ozone_sigma_a_scale;
    V3 temp = pos;
    temp.y += g.planet_radius;
    const float t = IntersectRayAtmosphere(g.planet_radius + g.atmosphere_altitude, temp, -v3p(g.sun_dir));
    const V3 tr = EstimateTransmittance(g.planet_radius, temp, -v3p(g.sun_dir), t, sigma_t_rayleigh, sigma_t_mie, sigma_t_ozone, 6);
    return tr * g.sun_illuminance;
}
ZR_HD V3 SkyTexel(const SkyLutView& lut, int x, int y)
{
    const uint32_t v = lut.data[(size_t)y * lut.w + x];
    return v3(zr_unpack_ufloat(v & 0x7ff, 6), zr_unpack_ufloat((v >> 11) & 0x7ff, 6), zr_unpack_ufloat(v >> 22, 5));
}
ZR_HD int WrapIndex(int i, int n) { int m = i % n; return m < 0 ? m + n : m; }
ZR_HD V3 SampleSkyLut(const SkyLutView& lut, V2 uv)
{
    const float x = uv.x * (float)lut.w - 0.5f, y = uv.y * (float)lut.h - 0.5f;
    const float fx = zr_floor(x), fy = zr_floor(y);
    const float tx = x - fx, ty = y - fy;
    const int x0 = WrapIndex((int)fx, (int)lut.w), x1 = WrapIndex((int)fx + 1, (int)lut.w);
    const int y0 = WrapIndex((int)fy, (int)lut.h), y1 = WrapIndex((int)fy + 1, (int)lut.h);
    const V3 a = SkyTexel(lut, x0, y0), b = SkyTexel(lut, x1, y0), c = SkyTexel(lut, x0, y1), d = SkyTexel(lut, x1, y1);
    const V3 r0 = v3(zr_lerp(a.x, b.x, tx), zr_lerp(a.y, b.y, tx), zr_lerp(a.z, b.z, tx));
    const V3 r1 = v3(zr_lerp(c.x, d.x, tx), zr_lerp(c.y, d.y, tx), zr_lerp(c.z, d.z, tx));
    return v3(zr_lerp(r0.x, r1.x, ty), zr_lerp(r0.y, r1.y, ty), zr_lerp(r0.z, r1.z, ty));
}
ZR_HD V3 Le_Sky(V3 wi, const SkyLutView& lut)                // LightSource.hlsli:159-174
{
    const V2 thetaPhi = SphericalFromCartesian(wi);
    V2 uv = v2(thetaPhi.y * ZR_ONE_OVER_2_PI, thetaPhi.x * ZR_ONE_OVER_PI);
    const float sn = thetaPhi.x >= ZR_PI_OVER_2 ? 1.0f : -1.0f;
    uv.y = zr_fma(0.5f, thetaPhi.x, -ZR_PI_OVER_4);
    uv.y = 0.5f + sn * zr_sqrt(zr_abs(uv.y) * ZR_ONE_OVER_PI);
    return SampleSkyLut(lut, uv);
}
// the target functor NEE_Sky hands to the lobe RIS (NEE.hlsli:68-84)
struct SkyIncidentRadiance { SkyLutView lut; ZR_HDM V3 operator()(V3 w) const { return Le_Sky(w, lut); } };

// Light::Le_SkyWithSunDisk, LightSource.hlsli:176-199: what a pixel without geometry shows -- the sun disk or the sky-view LUT along the
// pixel's pinhole camera ray (used by SkyDI, by the emissive DI pass and by Compositing for miss pixels)
ZR_HD V3 Le_SkyWithSunDisk(const SkyLutView& lut, const zr_frame_constants& g, uint32_t x, uint32_t y)
{
    V3 wc = GeneratePinholeCameraRay((int)x, (int)y, v2((float)g.render_width, (float)g.render_height), g.aspect_ratio, g.tan_half_fov,
        Row3(g.curr_view, 0), Row3(g.curr_view, 1), Row3(g.curr_view, 2), v2(g.curr_camera_jitter[0], g.curr_camera_jitter[1]));
    V3 rayOrigin = v3(0.0f, 1e-1f, 0.0f);
    rayOrigin.y += g.planet_radius;
    V3 wTemp = wc;
    wTemp.y = wTemp.y * g.sun_cos_angular_radius + zr_sqrt(1 - wc.y * wc.y) * g.sun_sin_angular_radius;
    float t;
    bool intersectedPlanet = IntersectRayPlanet(g.planet_radius, rayOrigin, wTemp, t);
    if (dot(-wc, v3p(g.sun_dir)) >= g.sun_cos_angular_radius && !intersectedPlanet) return v3(g.sun_illuminance);
    return Le_Sky(wc, lut);
}

// ------------------------------------------------------------------------------------------------ inscattering voxel grid (RP/Sky/Inscattering.hlsl)
// cbSky's voxel-grid fields (Sky_Common.h:13-29) + the slice count, INSCATTERING_THREAD_GROUP_SIZE_X
static constexpr uint32_t kInscatterSlices = 128;
struct InscatterParams { uint32_t numVoxelsX, numVoxelsY; float depthMappingExp, nearZ, farZ; };

// Inscattering.hlsl:32-42: start depth of slice z, exponentially distributed between VoxelGridNearZ and VoxelGridFarZ
ZR_HD float VoxelLinearDepth(const InscatterParams& c, uint32_t voxelZ)
{
    return c.nearZ + zr_pow((float)voxelZ / (float)kInscatterSlices, c.depthMappingExp) * (c.farZ - c.nearZ);
}
// :120-134: the view ray through the centre of column (x, y), in view space and in world space (both normalised)
ZR_HD void InscatterRay(const zr_frame_constants& g, const InscatterParams& c, uint32_t x, uint32_t y, V3& rayDirVS, V3& rayDirWS)
{
    const float u = ((float)x + 0.5f) / (float)c.numVoxelsX, v = ((float)y + 0.5f) / (float)c.numVoxelsY;
    float nx = zr_fma(u, 2.0f, -1.0f), ny = zr_fma(v, 2.0f, -1.0f);
    ny = -ny;
    nx *= g.aspect_ratio;
    nx *= g.tan_half_fov; ny *= g.tan_half_fov;
    const V3 dirV = v3(nx, ny, 1.0f);
    const V3 bx = Row3(g.curr_view, 0), by = Row3(g.curr_view, 1), bz = Row3(g.curr_view, 2);
    const V3 dirW = v3(zr_fma(dirV.x, bx.x, zr_fma(dirV.y, by.x, dirV.z * bz.x)), zr_fma(dirV.x, bx.y, zr_fma(dirV.y, by.y, dirV.z * bz.y)),
        zr_fma(dirV.x, bx.z, zr_fma(dirV.y, by.z, dirV.z * bz.z)));
    rayDirVS = normalize(dirV);
    rayDirWS = normalize(dirW);
}
// :145-152: slice thickness ds along the ray and the jittered sample position of voxel (x, y, z)
ZR_HD V3 VoxelPosition(const zr_frame_constants& g, const InscatterParams& c, uint32_t z, V3 rayDirVS, V3 rayDirWS, float& ds)
{
    const float currSliceStartLinearDepth = VoxelLinearDepth(c, z);
    const float nextSliceStartLinearDepth = VoxelLinearDepth(c, z + 1u);
    ds = (nextSliceStartLinearDepth - currSliceStartLinearDepth) / rayDirVS.z;
    const float sliceStartT = currSliceStartLinearDepth / rayDirVS.z;
    const float kHalton[8] = {0.5f, 0.25f, 0.75f, 0.125f, 0.625f, 0.375f, 0.875f, 0.0625f};      // :26
    const float offset = kHalton[g.frame_num & 7u];
    return v3p(g.camera_pos) + rayDirWS * (sliceStartT + offset * ds);
}
// :66-82.  `visibility(pos, wi)`: the any-hit shadow ray of :44-64 (1 = the sun is visible); the PlanetRadius shift is undone before it
template<class Visibility>
ZR_HD void ComputeVoxelData(const zr_frame_constants& g, V3 pos, V3 sigma_t_rayleigh, float sigma_t_mie, V3 sigma_t_ozone, const Visibility& visibility,
    V3& LoTransmittance, V3& density)
{
    pos.y += g.planet_radius;
    const float altitude = length(pos) - g.planet_radius;                                       // Volume::Altitude
    density = AtmosphereDensity(altitude);
    const float posToAtmosphereDist = IntersectRayAtmosphere(g.planet_radius + g.atmosphere_altitude, pos, -v3p(g.sun_dir));
    LoTransmittance = EstimateTransmittance(g.planet_radius, pos, -v3p(g.sun_dir), posToAtmosphereDist, sigma_t_rayleigh, sigma_t_mie, sigma_t_ozone, 8);
    pos.y -= g.planet_radius;
    const float isSunVisibleFromPos = visibility(pos, -v3p(g.sun_dir));
    LoTransmittance = LoTransmittance * isSunVisibleFromPos;
}
// :84-109.  `prefix(v)`: WavePrefixSum over the voxel's 32-lane segment (the scan order is pinned in include/zetaray_amd.h, ZR_PASS_SKY).
// waveStartToPosTr: transmittance from the segment's first slice to this one; Ls: in-scattered radiance over the same span
template<class PrefixSum>
ZR_HD void Integrate(const zr_frame_constants& g, V3 rayDir, float ds, V3 sigma_s_rayleigh, float sigma_s_mie, float sigma_t_mie, V3 sigma_t_ozone,
    V3 LoTransmittance, V3 density, const PrefixSum& prefix, V3& waveStartToPosTr, V3& Ls)
{
    const V3 sliceDensity = density * ds;
    const V3 opticalThickness = prefix(sliceDensity) + sliceDensity;
    waveStartToPosTr = vexp(-(sigma_s_rayleigh * opticalThickness.x + v3(sigma_t_mie * opticalThickness.y) + sigma_t_ozone * opticalThickness.z));
    const V3 common = waveStartToPosTr * LoTransmittance * ds;
    const V3 sliceLsRayleigh = common * density.x;
    const V3 sliceLsMie = common * density.y;
    const V3 LsRayleigh = prefix(sliceLsRayleigh) + sliceLsRayleigh;
    const V3 LsMie = prefix(sliceLsMie) + sliceLsMie;
    const float cosTheta = dot(v3p(g.sun_dir), -rayDir);
    const float phaseRayleigh = RayleighPhaseFunction(cosTheta);
    const float phaseMie = SchlickPhaseFunction(cosTheta, g.g);
    Ls = LsRayleigh * sigma_s_rayleigh * phaseRayleigh + LsMie * sigma_s_mie * phaseMie;
}
// :192-198: the segments before this one, serially: their in-scattering attenuated by the transmittance in front of them
ZR_HD V3 CombineSegments(V3 Ls, const V3* waveTr, const V3* waveLs, uint32_t waveIdx)
{
    V3 totalTr = v3(1.0f), prevLs = v3(0.0f);
    for (uint32_t w = 0; w < waveIdx; w++)
    {
        prevLs = prevLs + waveLs[w] * totalTr;
        totalTr = totalTr * waveTr[w];
    }
    return Ls * totalTr + prevLs;
}
// :202-204: max(Ls, 0) * SunIlluminance stored as half3 into the R11G11B10_FLOAT grid (f32 -> f16, then f16 -> R11G11B10, both to nearest even)
ZR_HD uint32_t InscatterTexel(const zr_frame_constants& g, V3 Ls)
{
    Ls = v3(zr_max(Ls.x, 0.0f), zr_max(Ls.y, 0.0f), zr_max(Ls.z, 0.0f));
    const V3 c = Ls * g.sun_illuminance;
    return PackR11G11B10F(v3(zr_round_f16(c.x), zr_round_f16(c.y), zr_round_f16(c.z)));
}

// Compositing.hlsl:74-97: the inscattering term of a pixel with view depth z_view.  Texture3D.SampleLevel(g_samLinearClamp, uvw, 0) is fp32
// trilinear, texel centres at (i + 0.5) / N, clamp addressing, R11G11B10 decoded exactly (coordinates are clamped to [-1, N] first: the same
// texels and weights under clamp addressing, and no float -> int overflow); the result is rounded to half (`half3 inscattering`).
struct InscatterGridView { const uint32_t* data; uint32_t nx, ny; float depthMappingExp, nearZ, farZ; };
ZR_HD V3 InscatterGridTexel(const InscatterGridView& v, int x, int y, int z)
{
    const uint32_t t = v.data[((size_t)z * v.ny + (size_t)y) * v.nx + (size_t)x];
    return v3(zr_unpack_ufloat(t & 0x7ff, 6), zr_unpack_ufloat((t >> 11) & 0x7ff, 6), zr_unpack_ufloat(t >> 22, 5));
}
ZR_HD void InscatterAxis(float u, int n, int& i0, int& i1, float& t)
{
    float x = u * (float)n - 0.5f;
    x = zr_min(zr_max(x, -1.0f), (float)n);
    const float f = zr_floor(x);
    t = x - f;
    const int i = (int)f;
    i0 = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    i1 = i + 1 < 0 ? 0 : (i + 1 > n - 1 ? n - 1 : i + 1);
}
ZR_HD V3 SampleInscatteringGrid(const InscatterGridView& v, float u, float w_, float p)
{
    int x0, x1, y0, y1, z0, z1; float tx, ty, tz;
    InscatterAxis(u, (int)v.nx, x0, x1, tx); InscatterAxis(w_, (int)v.ny, y0, y1, ty); InscatterAxis(p, (int)kInscatterSlices, z0, z1, tz);
    V3 r;
    for (int c = 0; c < 3; c++)
    {
        auto T = [&](int x, int y, int z) { const V3 t = InscatterGridTexel(v, x, y, z); return c == 0 ? t.x : (c == 1 ? t.y : t.z); };
        const float c00 = zr_lerp(T(x0, y0, z0), T(x1, y0, z0), tx);
        const float c10 = zr_lerp(T(x0, y1, z0), T(x1, y1, z0), tx);
        const float c01 = zr_lerp(T(x0, y0, z1), T(x1, y0, z1), tx);
        const float c11 = zr_lerp(T(x0, y1, z1), T(x1, y1, z1), tx);
        const float s = zr_lerp(zr_lerp(c00, c10, ty), zr_lerp(c01, c11, ty), tz);
        if (c == 0) r.x = s; else if (c == 1) r.y = s; else r.z = s;
    }
    return r;
}
// :78-96 for pixel (x, y): 0 where z_view <= 1e-4 (no inscattering added)
ZR_HD V3 InscatteringTerm(const zr_frame_constants& g, const InscatterGridView& v, float z_view, uint32_t x, uint32_t y)
{
    if (!(z_view > 1e-4f)) return v3(0.0f);
    const float u = ((float)x + 0.5f) / (float)g.render_width, w_ = ((float)y + 0.5f) / (float)g.render_height;
    const float p = zr_pow(zr_max(z_view - v.nearZ, 0.0f) / (v.farZ - v.nearZ), 1.0f / v.depthMappingExp);
    const V3 s = SampleInscatteringGrid(v, u, w_, p);
    return v3(zr_round_f16(s.x), zr_round_f16(s.y), zr_round_f16(s.z));
}

} // namespace zr
