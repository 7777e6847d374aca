/*
 * zr_jpeg.h -- a baseline JPEG image from its entropy-decoded coefficients to the texels of level 0: stated once for the host and the device.
 *
 * Entropy decoding is sequential and stays in the host loader (zetaray_amd/host/zr_scene_io.cpp), which writes the RECORD below.  Everything behind
 * it -- dequantisation, the 8 x 8 inverse DCT, chroma upsampling, YCbCr -> RGB, the channel map of the slot -- is this header: integers only, every
 * sum and product 32-bit two's-complement wrap-around (computed in uint32_t, shifted arithmetically), so the host (zrh_jpeg_decode), the device
 * (zr_tu_jpeg.hip) and either arithmetic build produce the same bytes, and on files libjpeg writes those are libjpeg's (JDCT_ISLOW, fancy upsampling).
 *
 *   dequantise   c[k] * q[k] in zigzag position k, placed at the natural position ZZ[k]
 *   IDCT         the 13-bit fixed-point Loeffler form, columns then rows; DESCALE(x, n) = (x + (1 << (n - 1))) >> n with n = 11 after the columns and
 *                18 after the rows; then + 128, clamped to [0, 255]
 *   upsampling   the triangle filter over a component's REAL samples (ceil(w h_c / h_max) columns, rows likewise; the padding the MCU grid adds is
 *                never read, the edge sample is used instead).  Written with the far tap clamped to the real extent, which gives the edge cases:
 *                  2 x 1:  o[2i] = (3 s[i] + s[i-1] + 1) >> 2      o[2i+1] = (3 s[i] + s[i+1] + 2) >> 2
 *                  2 x 2:  cs[i] = 3 s[r][i] + s[r'][i] (r' the row above for the upper output row, below for the lower one, clamped)
 *                          o[2i] = (3 cs[i] + cs[i-1] + 8) >> 4    o[2i+1] = (3 cs[i] + cs[i+1] + 7) >> 4
 *                A chroma component of n <= 2 real columns (w <= 4) is not filtered at all, in either direction: o[2i] = o[2i+1] = s[y / v][i].  That is
 *                libjpeg's rule (it selects the triangle filter only for downsampled_width > 2), kept because its bytes are the reference.
 *   colour       cb -= 128, cr -= 128:  R = y + ((91881 cr + 32768) >> 16), G = y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *                B = y + ((116130 cb + 32768) >> 16), each clamped to [0, 255]; A = 255; one component gives (y, y, y, 255)
 *   channel map  RGBA8 as it is, or RG8 from the file's (R, G) (normal map) or (B, G) (metallic-roughness map)
 *
 * THE RECORD (ZR_TEX_SRC_JPEG_COEF; little endian; starts on a multiple of 16 bytes of the payload):
 *   Header (496 B)             magic, the record's bytes, w, h, the component count (1 or 3), the channel map, the block count B, and per component its
 *                              sampling, blocks per row and block rows (padded to whole MCUs), first block and quantisation table (zigzag order)
 *   uint32_t coef_begin[B + 1] in int16 units into the array below; coef_begin[0] == 0
 *   int16_t  coef[]            the blocks de-interleaved: per component, row-major.  A block stores its first n QUANTISED coefficients in zigzag order,
 *                              n = (index of its last non-zero coefficient) + 1, at least 1
 * CheckRecord states everything a reader relies on; what it accepts the kernels trust.
 */
#ifndef ZR_JPEG_H
#define ZR_JPEG_H

#include "zr_detmath.h"
#include "zr_wire.h"
#include <stdint.h>
#include <string.h>

namespace zrjp {

static const uint32_t kMagic = 0x47504a5au;      /* "ZJPG" */
enum { kMapRgba = 0, kMapRg = 1, kMapBg = 2 };
struct Comp { uint32_t hs, vs, bw, bh, first_block, pad; uint16_t q[64]; };
struct Header { uint32_t magic, pad0; uint64_t bytes; uint32_t w, h, ncomp, map, num_blocks, pad1; Comp comp[3]; };
static_assert(sizeof(Comp) == 152 && sizeof(Header) == 496, "the record header is 496 bytes");

/* natural position of zigzag position k */
static const uint8_t ZZ[64] = { 0,  1,  8, 16,  9,  2,  3, 10, 17, 24, 32, 25, 18, 11,  4,  5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,  6,  7, 14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

/* ------------------------------------------------------------------------------------------------ the inverse DCT */
template <int N> ZR_HD uint32_t Descale(uint32_t x) { return (uint32_t)((int32_t)(x + (1u << (N - 1))) >> N); }
/* one pass over eight values in place (int32 bits held in uint32_t), descaled by N bits */
template <int N> ZR_HD void IdctPass(uint32_t& v0, uint32_t& v1, uint32_t& v2, uint32_t& v3, uint32_t& v4, uint32_t& v5, uint32_t& v6, uint32_t& v7)
{
    uint32_t z1 = (v2 + v6) * 4433u;
    const uint32_t t2 = z1 - v6 * 15137u, t3 = z1 + v2 * 6270u;
    const uint32_t t0 = (v0 + v4) << 13, t1 = (v0 - v4) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a0 = v7, a1 = v5, a2 = v3, a3 = v1;
    z1 = a0 + a3;
    uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= 0u - 7373u; z2 *= 0u - 20995u; z3 *= 0u - 16069u; z4 *= 0u - 3196u;
    z3 += z5; z4 += z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    v0 = Descale<N>(t10 + a3); v7 = Descale<N>(t10 - a3);
    v1 = Descale<N>(t11 + a2); v6 = Descale<N>(t11 - a2);
    v2 = Descale<N>(t12 + a1); v5 = Descale<N>(t12 - a1);
    v3 = Descale<N>(t13 + a0); v4 = Descale<N>(t13 - a0);
}
ZR_HD uint32_t Clamp255(uint32_t x) { const int32_t v = (int32_t)x; return v < 0 ? 0u : (v > 255 ? 255u : (uint32_t)v); }
/* v: the 64 dequantised coefficients in natural order, in place -> the 64 samples (every index is a constant once unrolled) */
ZR_HD void Idct8x8(uint32_t* v)
{
    ZR_UNROLL
    for (uint32_t c = 0; c < 8u; c++) IdctPass<11>(v[c], v[8u + c], v[16u + c], v[24u + c], v[32u + c], v[40u + c], v[48u + c], v[56u + c]);
    ZR_UNROLL
    for (uint32_t r = 0; r < 8u; r++)
    {
        IdctPass<18>(v[8u * r], v[8u * r + 1u], v[8u * r + 2u], v[8u * r + 3u], v[8u * r + 4u], v[8u * r + 5u], v[8u * r + 6u], v[8u * r + 7u]);
        ZR_UNROLL
        for (uint32_t c = 0; c < 8u; c++) v[8u * r + c] = Clamp255(v[8u * r + c] + 128u);
    }
}

/* ------------------------------------------------------------------------------------------------ jobs (zr_tu_jpeg.hip, and the host form below) */
/* The blocks of one component of one image.  coef_begin / coef: bytes into the payload of the record's two arrays; plane: bytes into the sample planes
   of the component's plane, 8 bw bytes per row and 8 bh rows; comp_first: the component's first block in the record; first_block: among all blocks of a
   launch (jobs sorted by it); q2: the quantisation table in NATURAL order, entries 2 i and 2 i + 1 in the halves of word i */
struct BlockJob { uint64_t coef_begin, coef, plane; uint32_t bw, comp_first, first_block, pad; uint32_t q2[32]; };
/* The texels of one image.  dst: bytes into the texel heap of level 0; plane / stride: as above, per component; hs, vs: the luma sampling (chroma is
   1 x 1); first_item: among all texels of a launch (jobs sorted by it) */
struct TexJob { uint64_t dst, plane[3]; uint32_t stride[3], w, h, ncomp, hs, vs, map, first_item; };
template <typename J> ZR_HD uint32_t FindFirst(const J* jobs, uint32_t n, uint32_t g, uint32_t J::* key)
{
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (jobs[mid].*key <= g) lo = mid; else hi = mid; }
    return lo;
}

/* one chroma sample at full resolution for texel (x, y): p = the component's plane */
ZR_HD uint32_t Chroma(const uint8_t* p, uint32_t stride, const TexJob& t, uint32_t x, uint32_t y)
{
    if (t.hs == 1u) return p[(uint64_t)y * stride + x];
    const uint32_t n = (t.w + 1u) >> 1, i = x >> 1;
    if (n <= 2u) return p[(uint64_t)(t.vs == 2u ? y >> 1 : y) * stride + i];      /* libjpeg filters only components wider than 2 samples: replication */
    const uint32_t j = (x & 1u) ? (i + 1u < n ? i + 1u : i) : (i ? i - 1u : 0u);      /* the far tap, clamped to the real columns */
    if (t.vs == 1u)
    {
        const uint8_t* row = p + (uint64_t)y * stride;
        return (3u * row[i] + row[j] + ((x & 1u) ? 2u : 1u)) >> 2;
    }
    const uint32_t rows = (t.h + 1u) >> 1, r = y >> 1;
    const uint32_t r2 = (y & 1u) ? (r + 1u < rows ? r + 1u : r) : (r ? r - 1u : 0u);
    const uint8_t* near = p + (uint64_t)r * stride;
    const uint8_t* far = p + (uint64_t)r2 * stride;
    const uint32_t ci = 3u * near[i] + far[i], cj = 3u * near[j] + far[j];
    return (3u * ci + cj + ((x & 1u) ? 7u : 8u)) >> 4;
}
/* texel (x, y) of the image: r | g << 8 | b << 16 | 255 << 24 for kMapRgba, c0 | c1 << 8 for the RG maps */
ZR_HD uint32_t Texel(const uint8_t* planes, const TexJob& t, uint32_t x, uint32_t y)
{
    const uint32_t Y = planes[t.plane[0] + (uint64_t)y * t.stride[0] + x];
    uint32_t R = Y, G = Y, B = Y;
    if (t.ncomp == 3u)
    {
        const uint32_t cb = Chroma(planes + t.plane[1], t.stride[1], t, x, y) - 128u, cr = Chroma(planes + t.plane[2], t.stride[2], t, x, y) - 128u;
        R = Clamp255(Y + (uint32_t)((int32_t)(91881u * cr + 32768u) >> 16));
        G = Clamp255(Y + (uint32_t)((int32_t)((0u - 22554u) * cb + (0u - 46802u) * cr + 32768u) >> 16));
        B = Clamp255(Y + (uint32_t)((int32_t)(116130u * cb + 32768u) >> 16));
    }
    if (t.map == (uint32_t)kMapRgba) return R | (G << 8) | (B << 16) | 0xff000000u;
    return (t.map == (uint32_t)kMapRg ? R : B) | (G << 8);
}

/* ------------------------------------------------------------------------------------------------ the record, checked (host) */
static inline uint32_t CeilDiv(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }
/* Fills comp[].bw / bh / first_block and num_blocks of a header whose w, h, ncomp and sampling are set; false for a sampling this header does not read */
static inline bool LayoutComponents(Header& h)
{
    if (h.ncomp != 1u && h.ncomp != 3u) return false;
    const uint32_t hs = h.comp[0].hs, vs = h.comp[0].vs;
    if (h.ncomp == 1u ? (hs != 1u || vs != 1u) : !((hs == 1u && vs == 1u) || (hs == 2u && vs == 1u) || (hs == 2u && vs == 2u))) return false;
    for (uint32_t c = 1; c < h.ncomp; c++) if (h.comp[c].hs != 1u || h.comp[c].vs != 1u) return false;
    const uint32_t mx = CeilDiv(h.w, 8u * hs), my = CeilDiv(h.h, 8u * vs);
    uint32_t first = 0u;
    for (uint32_t c = 0; c < h.ncomp; c++)
    {
        h.comp[c].bw = mx * h.comp[c].hs; h.comp[c].bh = my * h.comp[c].vs; h.comp[c].first_block = first;
        first += h.comp[c].bw * h.comp[c].bh;      /* (at most 1.5 x 8192^2) */
    }
    h.num_blocks = first;
    return true;
}
/* null if the `avail` bytes at rec hold a whole, consistent record (copied to *out), else what is wrong with it */
static inline const char* CheckRecord(const uint8_t* rec, uint64_t avail, Header* out)
{
    Header h;
    if (avail < sizeof(Header)) return "the record ends beyond the payload";
    memcpy(&h, rec, sizeof(Header));
    if (h.magic != kMagic) return "wrong magic";
    if (h.bytes > avail) return "the record ends beyond the payload";
    if (h.w == 0u || h.h == 0u || h.w > 65535u || h.h > 65535u) return "dimensions outside [1, 65535]";
    if (h.map > (uint32_t)kMapBg) return "unknown channel map";
    Header want = h;
    if (!LayoutComponents(want)) return "unsupported component count or sampling";
    if (want.num_blocks != h.num_blocks) return "the block count does not follow from the size and the sampling";
    for (uint32_t c = 0; c < h.ncomp; c++)
        if (want.comp[c].bw != h.comp[c].bw || want.comp[c].bh != h.comp[c].bh || want.comp[c].first_block != h.comp[c].first_block) return "the block layout does not follow from the size and the sampling";
    const uint64_t table = sizeof(Header) + 4ull * ((uint64_t)h.num_blocks + 1u);
    if (table > h.bytes) return "coef_begin ends beyond the record";
    const uint8_t* cb = rec + sizeof(Header);
    uint32_t prev; memcpy(&prev, cb, 4);
    if (prev != 0u) return "coef_begin does not start at 0";
    for (uint32_t b = 1; b <= h.num_blocks; b++)
    {
        uint32_t at; memcpy(&at, cb + 4ull * b, 4);
        if (at <= prev || at - prev > 64u) return "coef_begin does not increase in steps of 1 .. 64";
        prev = at;
    }
    if (table + 2ull * prev > h.bytes) return "the coefficients end beyond the record";
    *out = h;
    return nullptr;
}
/* the bytes of the sample planes of a checked header (8 bw x 8 bh per component) */
static inline uint64_t PlaneBytes(const Header& h)
{
    uint64_t n = 0;
    for (uint32_t c = 0; c < h.ncomp; c++) n += 64ull * h.comp[c].bw * h.comp[c].bh;
    return n;
}
/* the jobs of a checked record that lies `at` bytes into the payload, its planes from `planeAt` on and its level 0 at `dst` of the heap */
static inline void MakeJobs(const Header& h, uint64_t at, uint64_t planeAt, uint64_t dst, uint32_t firstBlock, uint32_t firstItem, BlockJob* bj, TexJob* tj)
{
    memset(tj, 0, sizeof(TexJob));
    tj->dst = dst; tj->w = h.w; tj->h = h.h; tj->ncomp = h.ncomp; tj->hs = h.comp[0].hs; tj->vs = h.comp[0].vs; tj->map = h.map; tj->first_item = firstItem;
    for (uint32_t c = 0; c < h.ncomp; c++)
    {
        BlockJob& j = bj[c];
        memset(&j, 0, sizeof(BlockJob));
        j.coef_begin = at + sizeof(Header); j.coef = j.coef_begin + 4ull * ((uint64_t)h.num_blocks + 1u); j.plane = planeAt;
        j.bw = h.comp[c].bw; j.comp_first = h.comp[c].first_block; j.first_block = firstBlock + h.comp[c].first_block;
        for (uint32_t k = 0; k < 64u; k++) j.q2[ZZ[k] >> 1] |= (uint32_t)h.comp[c].q[k] << (16u * (ZZ[k] & 1u));
        tj->plane[c] = planeAt; tj->stride[c] = 8u * h.comp[c].bw;
        planeAt += 64ull * h.comp[c].bw * h.comp[c].bh;
    }
}

/* ------------------------------------------------------------------------------------------------ the host form */
/* block `local` of a job: its coefficient run dequantised to natural order, transformed, stored in the plane */
static inline void DecodeBlock(const uint8_t* payload, const BlockJob& j, uint32_t local, uint8_t* planes)
{
    uint32_t b0, b1;
    memcpy(&b0, payload + j.coef_begin + 4ull * (j.comp_first + local), 4); memcpy(&b1, payload + j.coef_begin + 4ull * (j.comp_first + local) + 4u, 4);
    uint32_t v[64] = {0};
    for (uint32_t k = 0; k < b1 - b0; k++)
    {
        int16_t c; memcpy(&c, payload + j.coef + 2ull * (b0 + k), 2);
        const uint32_t nat = ZZ[k];
        v[nat] = (uint32_t)(int32_t)c * ((j.q2[nat >> 1] >> (16u * (nat & 1u))) & 0xffffu);
    }
    Idct8x8(v);
    const uint32_t by = local / j.bw, bx = local - by * j.bw;
    uint8_t* o = planes + j.plane + (64ull * by * j.bw + 8ull * bx);
    for (uint32_t r = 0; r < 8u; r++) for (uint32_t c = 0; c < 8u; c++) o[8ull * r * j.bw + c] = (uint8_t)v[8u * r + c];
}
/* A checked record -> the w x h texels of its channel map at out (4 B / texel for kMapRgba, else 2).  planes: PlaneBytes(h) bytes of scratch */
static inline void DecodeRecord(const uint8_t* rec, const Header& h, uint8_t* planes, uint8_t* out)
{
    BlockJob bj[3]; TexJob tj;
    MakeJobs(h, 0u, 0u, 0u, 0u, 0u, bj, &tj);
    for (uint32_t c = 0; c < h.ncomp; c++) for (uint32_t b = 0; b < h.comp[c].bw * h.comp[c].bh; b++) DecodeBlock(rec, bj[c], b, planes);
    const bool rgba = h.map == (uint32_t)kMapRgba;
    for (uint32_t y = 0; y < h.h; y++) for (uint32_t x = 0; x < h.w; x++)
    {
        const uint32_t p = Texel(planes, tj, x, y);
        uint8_t* q = out + ((size_t)y * h.w + x) * (rgba ? 4u : 2u);
        q[0] = (uint8_t)p; q[1] = (uint8_t)(p >> 8);
        if (rgba) { q[2] = (uint8_t)(p >> 16); q[3] = (uint8_t)(p >> 24); }
    }
}

} // namespace zrjp

#endif
