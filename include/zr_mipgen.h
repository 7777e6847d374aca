/*
 * zr_mipgen.h -- the mip chain of a material texture, generated from its level 0: stated once for the host and the device.
 *
 * A glTF with PNG images carries level 0 only; the texture heap (zr_wire.h, zr_texture.h) holds full chains, which zr_texture.h filters with ray
 * differentials.  This header makes level m + 1 from the STORED BYTES of level m, per channel, by an exact area-weighted box over the sizes of
 * zr_tex_mip_of (max(1, n >> 1) per axis).  Integer arithmetic only, so the host (zrh_mip_generate of zetaray_amd/host/zr_scene_io.cpp), the device
 * (zr_tu_mipgen.hip) and either arithmetic build produce the same bytes.
 *
 * 1-D taps for a source extent n and destination texel x, with m = max(1, n >> 1):
 *   n == 1       taps {0}                  weights {1}                denominator 1
 *   n even       taps {2x, 2x + 1}         weights {1, 1}             denominator 2
 *   n odd >= 3   taps {2x, 2x + 1, 2x + 2} weights {m - x, m, x + 1}  denominator n
 * The odd case is the exact overlap of [x n / m, (x + 1) n / m) with the source texels, times m.  The 2-D weight is the product of the two 1-D
 * weights and D = Dx Dy.  Sums are 64-bit: D reaches 65535^2 and the values 65535.
 *
 *   UNORM channels (all of RGBA8, both of RG8, alpha of RGBA8_SRGB): out = (2 S + D) / (2 D) with S = sum w byte -- round half up.
 *   sRGB channels (r, g, b of RGBA8_SRGB) are averaged in linear light: S = sum w L[byte] with L = zr_srgb16_table (round(65535 linear(c)), strictly
 *   increasing), and the output is the code whose L is nearest to S / D, ties upward: the largest c with 2 S >= (L[c - 1] + L[c]) D, found in 8
 *   binary-search steps with integer compares.
 *
 * Stated deviations: nearest in linear space, not round(255 encode(mean)); colour is not weighted by alpha; normal-map x / y are averaged without
 * renormalisation (z is reconstructed at sampling time); the reference tool's (texconv) WIC filter is not reproduced.
 */
#ifndef ZR_MIPGEN_H
#define ZR_MIPGEN_H

#include "zr_detmath.h"
#include "zr_wire.h"
#include "zr_texture.h"
#include "zr_srgb16_table.h"
#include <stdint.h>
#include <string.h>

namespace zrmg {

/* the taps of one axis: source texels first .. first + count - 1 with weights w0, w1, w2 (those beyond count are 0) over `den` */
struct Taps { uint32_t first, count, w0, w1, w2, den; };
ZR_HD Taps Taps1(uint32_t n, uint32_t x)
{
    const bool one = n == 1u, odd = !one && (n & 1u);      /* (neither: even) */
    const uint32_t m = n >> 1;
    Taps t;
    t.first = 2u * x; t.count = one ? 1u : (odd ? 3u : 2u);
    t.w0 = odd ? m - x : 1u; t.w1 = one ? 0u : (odd ? m : 1u); t.w2 = odd ? x + 1u : 0u;
    t.den = one ? 1u : (odd ? n : 2u);
    return t;
}
ZR_HD uint32_t TapWeight(const Taps& t, uint32_t k) { return k == 0u ? t.w0 : (k == 1u ? t.w1 : t.w2); }

/* round half up of S / D */
ZR_HD uint32_t Unorm(uint64_t S, uint64_t D) { return (uint32_t)((2u * S + D) / (2u * D)); }
/* the sRGB code whose L is nearest to S / D, ties upward (L: zr_srgb16_table, or its copy on the device) */
ZR_HD uint32_t SrgbCode(const uint16_t* L, uint64_t S, uint64_t D)
{
    uint32_t c = 0u;
    ZR_UNROLL
    for (uint32_t step = 128u; step; step >>= 1)
    {
        const uint32_t k = c | step;
        if (2u * S >= (uint64_t)((uint32_t)L[k - 1u] + (uint32_t)L[k]) * D) c = k;
    }
    return c;
}

/* one texel of `format` at p: RGBA8 as r | g << 8 | b << 16 | a << 24 (p 4-byte aligned), RG8 as r | g << 8 (p 2-byte aligned) */
ZR_HD uint32_t LoadTexel(const uint8_t* p, bool rg)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return rg ? (uint32_t)*reinterpret_cast<const uint16_t*>(p) : *reinterpret_cast<const uint32_t*>(p);
#else
    return rg ? ((uint32_t)p[0] | ((uint32_t)p[1] << 8)) : ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
#endif
}

/* Texel (x, y) of the level below a source level of sw x sh texels at `src` (rows top-down, tightly packed), packed like LoadTexel.
   Both extents even -- every level of a power-of-two texture but its last ones -- is the 2 x 2 box: D = 4, 32-bit sums, the same integers. */
ZR_HD uint32_t Texel(const uint8_t* src, uint32_t sw, uint32_t sh, uint32_t format, uint32_t x, uint32_t y, const uint16_t* L)
{
    const bool rg = format == ZR_TEX_RG8, srgb = format == ZR_TEX_RGBA8_SRGB;
    const uint32_t bpp = rg ? 2u : 4u;
    if (!((sw | sh) & 1u))
    {
        const uint8_t* r0 = src + ((uint64_t)(2u * y) * sw + 2u * x) * bpp;
        const uint8_t* r1 = r0 + (uint64_t)sw * bpp;
        const uint32_t p0 = LoadTexel(r0, rg), p1 = LoadTexel(r0 + bpp, rg), p2 = LoadTexel(r1, rg), p3 = LoadTexel(r1 + bpp, rg);
        uint32_t out = 0u;
        ZR_UNROLL
        for (uint32_t ch = 0; ch < 4u; ch++)
        {
            if (rg && ch >= 2u) break;
            const uint32_t sh8 = 8u * ch;
            const uint32_t a = (p0 >> sh8) & 0xffu, b = (p1 >> sh8) & 0xffu, c = (p2 >> sh8) & 0xffu, d = (p3 >> sh8) & 0xffu;
            uint32_t v;
            if (srgb && ch < 3u) v = SrgbCode(L, (uint64_t)((uint32_t)L[a] + (uint32_t)L[b] + (uint32_t)L[c] + (uint32_t)L[d]), 4u);
            else v = (a + b + c + d + 2u) >> 2;      /* Unorm(S, 4) */
            out |= v << sh8;
        }
        return out;
    }
    const Taps tx = Taps1(sw, x), ty = Taps1(sh, y);
    const uint64_t D = (uint64_t)tx.den * ty.den;
    uint64_t S0 = 0u, S1 = 0u, S2 = 0u, S3 = 0u;
    ZR_UNROLL
    for (uint32_t j = 0; j < 3u; j++)      /* (unrolled with constant tap numbers: nothing is indexed at run time) */
    {
        if (j >= ty.count) break;
        const uint8_t* row = src + ((uint64_t)(ty.first + j) * sw + tx.first) * bpp;
        const uint64_t wy = TapWeight(ty, j);
        ZR_UNROLL
        for (uint32_t i = 0; i < 3u; i++)
        {
            if (i >= tx.count) break;
            const uint64_t w = wy * TapWeight(tx, i);
            const uint32_t p = LoadTexel(row + i * bpp, rg);
            const uint32_t r = p & 0xffu, g = (p >> 8) & 0xffu, b = (p >> 16) & 0xffu, a = p >> 24;
            if (srgb) { S0 += w * L[r]; S1 += w * L[g]; S2 += w * L[b]; }
            else { S0 += w * r; S1 += w * g; S2 += w * b; }
            S3 += w * a;
        }
    }
    if (rg) return Unorm(S0, D) | (Unorm(S1, D) << 8);
    if (srgb) return SrgbCode(L, S0, D) | (SrgbCode(L, S1, D) << 8) | (SrgbCode(L, S2, D) << 16) | (Unorm(S3, D) << 24);
    return Unorm(S0, D) | (Unorm(S1, D) << 8) | (Unorm(S2, D) << 16) | (Unorm(S3, D) << 24);
}

/* ------------------------------------------------------------------------------------------------ jobs (zr_tu_mipgen.hip) */
/* One level of one texture for the kernel, which is launched once per level for all textures of a call: `src` / `dst` bytes into the texel heap (the
   level above and the level written), their sizes, the texture's format, and the index of the level's first destination texel among all destination
   texels of the launch.  The jobs of a launch are sorted by first_item. */
struct Job { uint64_t src, dst; uint32_t sw, sh, dw, dh, format, first_item; };
/* the job that holds item `g`: the last one whose first_item is <= g (jobs[0].first_item == 0, n >= 1) */
ZR_HD uint32_t FindJob(const Job* jobs, uint32_t n, uint32_t g)
{
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (jobs[mid].first_item <= g) lo = mid; else hi = mid; }
    return lo;
}

/* ------------------------------------------------------------------------------------------------ the host form */
/* level m + 1 (at dst, max(1, sw >> 1) x max(1, sh >> 1) texels) from level m (at src) */
static inline void GenerateLevel(const uint8_t* src, uint32_t sw, uint32_t sh, uint32_t format, uint8_t* dst)
{
    const uint32_t dw = sw > 1u ? sw >> 1 : 1u, dh = sh > 1u ? sh >> 1 : 1u;
    for (uint32_t y = 0; y < dh; y++) for (uint32_t x = 0; x < dw; x++)
    {
        const uint32_t p = Texel(src, sw, sh, format, x, y, zr_srgb16_table);
        uint8_t* q = dst + ((size_t)y * dw + x) * (format == ZR_TEX_RG8 ? 2u : 4u);
        q[0] = (uint8_t)p; q[1] = (uint8_t)(p >> 8);
        if (format != ZR_TEX_RG8) { q[2] = (uint8_t)(p >> 16); q[3] = (uint8_t)(p >> 24); }
    }
}
/* levels 1 .. num_mips - 1 of the chain `d` names in `texels`, in place, from its level 0 */
static inline void GenerateChain(const zr_texture_desc* d, uint8_t* texels)
{
    for (uint32_t m = 1; m < d->num_mips; m++)
    {
        const zr_tex_mip s = zr_tex_mip_of(d, m - 1u), t = zr_tex_mip_of(d, m);
        GenerateLevel(texels + s.offset, s.w, s.h, d->format, texels + t.offset);
    }
}

} // namespace zrmg

#endif
