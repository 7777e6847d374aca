/*
 * zr_bcn.h -- BC7 (BPTC) and BC5 block decompression, stated once for the host and the device.
 *
 * The material textures of a scene arrive as BC7 / BC5 .dds files (Assets.cpp + Tools/BCnCompressglTF of the reference); the texture heap the kernels
 * sample is uncompressed RGBA8 / RG8 (zr_wire.h, zr_texture.h).  This header turns the one into the other.  It holds the decoder twice:
 *
 *   Bc7Block / Bc4Block      the host loader's code (zrh_bc7_decode / zrh_bc5_decode / LoadDDS of zetaray_amd/host/zr_scene_io.cpp), a bit reader
 *                            that follows the D3D11 functional spec / Khronos data format spec 18.3 field by field.  Pinned to Pillow by
 *                            tests/test_scene_io.py.  Host only.
 *   Bc7Begin / Bc7Texel,     the same function of the 16 bytes written for a GPU lane (ZR_HD): zr_tu_texdecode.hip compiles it for the device,
 *   Bc5Texel                 tests/bcnmath for the host.  Integer arithmetic only, so host == device in every byte, in either arithmetic build.
 *
 * The lane form:
 *   - the block is four 32-bit words (little endian: word k = bytes 4k .. 4k + 3); a field of n <= 8 bits at bit position p is taken with two
 *     shifts from the words p / 32 and p / 32 + 1, which are SELECTED with compares, never indexed (Field)
 *   - per-mode constants are nibbles of one 32-bit immediate each (kNS .. kIB2), so the code is one path for the eight modes and lanes of different
 *     modes do not serialise.  After the mode's unary prefix come partition, rotation and index-selector bits, then, for N = 2 x subsets endpoints,
 *     field (endpoint e, channel c) of CB bits at  base + (c N + e) CB  for c = R, G, B, the alpha of endpoint e at  base + 3 N CB + e AB,
 *     the p-bits (one per endpoint, or one per subset in mode 1) behind them, then the indices
 *   - the at most six endpoints are held as packed RGBA words, expanded to 8 bits; a texel picks its pair with compares on its subset
 *   - the 2- and 3-subset partition tables are packed 2 bits per texel (kPart2 / kPart3, 64 words each); the anchor texels, whose index is one bit
 *     short, are three nibbles per partition (kAnchors).  Texel i's index starts at  ibase + i IB - (the number of anchors before i)
 *   - the interpolation weights are (64 i + (2^b - 1) / 2) / (2^b - 1), which is the specification's table for b = 2, 3, 4; the divisions by 3, 7
 *     and 15, and BC4's by 7 and 5, are multiplications by a 16-bit reciprocal, exact over the ranges they see (checked exhaustively by
 *     tools/make_bcn_goldens.py and, through the fixture, by tests/test_bcn_cpu.py)
 *   - no array is indexed at run time, so nothing goes to scratch memory
 *
 * Pinned here:
 *   - the reserved mode (byte 0 == 0) decodes to 16 texels of (0, 0, 0, 0)
 *   - a mip of w x h texels holds ceil(w / 4) x ceil(h / 4) blocks of 16 bytes in row-major order; texel (x, y) of block (bx, by) is texel
 *     (4 bx + x, 4 by + y) of the mip and texels of a partial block beyond w / h are dropped
 *   - BC5 is two BC4 blocks, red first; the texel is (r, g)
 *   - a texture's chain in a zr_texture_blocks payload (zetaray_amd.h) is its mips back to back in DDS order, mip m being
 *     max(1, w >> m) x max(1, h >> m) as in zr_texture_desc
 */
#ifndef ZR_BCN_H
#define ZR_BCN_H

#include "zr_detmath.h"
#include <stdint.h>
#include <string.h>

namespace zrbc {

/* ZR_TEX_SRC_* of zetaray_amd.h */
enum { kSrcRaw = 0, kSrcBc7 = 1, kSrcBc5 = 2 };

/* ------------------------------------------------------------------------------------------------ tables */
/* subset of texel i of partition p: (kPart[p] >> 2 i) & 3 */
ZR_HD uint32_t Part2(uint32_t p)
{
    static const uint32_t kPart2[64] = {
    0x50505050u,0x40404040u,0x54545454u,0x54505040u,0x50404000u,0x55545450u,0x55545040u,0x54504000u,
    0x50400000u,0x55555450u,0x55544000u,0x54400000u,0x55555440u,0x55550000u,0x55555500u,0x55000000u,
    0x55150100u,0x00004054u,0x15010000u,0x00405054u,0x00004050u,0x15050100u,0x05010000u,0x40505054u,
    0x00404050u,0x05010100u,0x14141414u,0x05141450u,0x01155440u,0x00555500u,0x15014054u,0x05414150u,
    0x44444444u,0x55005500u,0x11441144u,0x05055050u,0x05500550u,0x11114444u,0x41144114u,0x44111144u,
    0x15055054u,0x01055040u,0x05041050u,0x05455150u,0x14414114u,0x50050550u,0x41411414u,0x00141400u,
    0x00041504u,0x00105410u,0x10541000u,0x04150400u,0x50410514u,0x41051450u,0x05415014u,0x14054150u,
    0x41050514u,0x41505014u,0x40011554u,0x54150140u,0x50505500u,0x00555050u,0x15151010u,0x54540404u };
    return kPart2[p & 63u];
}
ZR_HD uint32_t Part3(uint32_t p)
{
    static const uint32_t kPart3[64] = {
    0xaa685050u,0x6a5a5040u,0x5a5a4200u,0x5450a0a8u,0xa5a50000u,0xa0a05050u,0x5555a0a0u,0x5a5a5050u,
    0xaa550000u,0xaa555500u,0xaaaa5500u,0x90909090u,0x94949494u,0xa4a4a4a4u,0xa9a59450u,0x2a0a4250u,
    0xa5945040u,0x0a425054u,0xa5a5a500u,0x55a0a0a0u,0xa8a85454u,0x6a6a4040u,0xa4a45000u,0x1a1a0500u,
    0x0050a4a4u,0xaaa59090u,0x14696914u,0x69691400u,0xa08585a0u,0xaa821414u,0x50a4a450u,0x6a5a0200u,
    0xa9a58000u,0x5090a0a8u,0xa8a09050u,0x24242424u,0x00aa5500u,0x24924924u,0x24499224u,0x50a50a50u,
    0x500aa550u,0xaaaa4444u,0x66660000u,0xa5a0a5a0u,0x50a050a0u,0x69286928u,0x44aaaa44u,0x66666600u,
    0xaa444444u,0x54a854a8u,0x95809580u,0x96969600u,0xa85454a8u,0x80959580u,0xaa141414u,0x96960000u,
    0xaaaa1414u,0xa05050a0u,0xa0a5a5a0u,0x96000000u,0x40804080u,0xa9a8a9a8u,0xaaaaaa44u,0x2a4a5254u };
    return kPart3[p & 63u];
}
/* anchor texels of partition p: bits 0-3 the second subset's of a 2-subset block, bits 4-7 / 8-11 the second / third subset's of a 3-subset block
   (texel 0 is always the first subset's) */
ZR_HD uint32_t Anchors(uint32_t p)
{
    static const uint16_t kAnchors[64] = {
    0xf3f,0x83f,0x8ff,0x3ff,0xf8f,0xf3f,0x3ff,0x8ff, 0xf8f,0xf8f,0xf6f,0xf6f,0xf6f,0xf5f,0xf3f,0x83f,
    0xf3f,0x832,0xf88,0x3f2,0xf32,0x838,0xf68,0x8af, 0x352,0xf88,0x682,0xa62,0xf88,0xf58,0xaf2,0x8f2,
    0xf8f,0x3ff,0xf36,0xa58,0xa62,0x8a8,0x98f,0xaff, 0x6f2,0xf38,0x8f2,0xf52,0x3f2,0x6ff,0x6ff,0x8f6,
    0xf36,0x3f2,0xf56,0xf58,0xf5f,0xf8f,0xf52,0xfa2, 0xf5f,0xfaf,0xf8f,0xfdf,0x3ff,0xfc2,0xf32,0x83f };
    return kAnchors[p & 63u];
}
/* per-mode constants, mode m in bits 4 m .. 4 m + 3: subsets, partition bits, rotation bits, index-selector bits, colour bits, alpha bits,
   a p-bit per endpoint, a p-bit per subset, index bits, secondary index bits */
static constexpr uint32_t kNS = 0x21112323u, kPB = 0x60006664u, kRB = 0x00220000u, kISB = 0x00010000u, kCB = 0x57757564u, kAB = 0x57860000u,
                      kEPB = 0x11001001u, kSPB = 0x00000010u, kIB = 0x24222233u, kIB2 = 0x00230000u;
ZR_HD uint32_t ModeParam(uint32_t table, uint32_t mode) { return (table >> (4u * mode)) & 15u; }

/* ------------------------------------------------------------------------------------------------ the host loader's decoder (host only) */
struct Bits { const uint8_t* p; uint32_t pos = 0; uint32_t Get(uint32_t n) { uint32_t v = 0; for (uint32_t i = 0; i < n; i++, pos++) v |= (uint32_t)((p[pos >> 3] >> (pos & 7)) & 1u) << i; return v; } };
static inline uint8_t Interp(uint32_t a, uint32_t b, uint32_t w) { return (uint8_t)((a * (64 - w) + b * w + 32) >> 6); }
static inline void Bc7Block(const uint8_t* blk, uint8_t out[16][4])
{
    static const uint8_t kW2[4] = {0, 21, 43, 64}, kW3[8] = {0, 9, 18, 27, 37, 46, 55, 64}, kW4[16] = {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64};
    uint32_t mode = 0; while (mode < 8 && !((blk[0] >> mode) & 1)) mode++;
    if (mode >= 8) { memset(out, 0, 64); return; }
    static const uint8_t NS[8] = {3, 2, 3, 2, 1, 1, 1, 2}, PB[8] = {4, 6, 6, 6, 0, 0, 0, 6}, RB[8] = {0, 0, 0, 0, 2, 2, 0, 0}, ISB[8] = {0, 0, 0, 0, 1, 0, 0, 0};
    static const uint8_t CB[8] = {4, 6, 5, 7, 5, 7, 7, 5}, AB[8] = {0, 0, 0, 0, 6, 8, 7, 5}, EPB[8] = {1, 0, 0, 1, 0, 0, 1, 1}, SPB[8] = {0, 1, 0, 0, 0, 0, 0, 0};
    static const uint8_t IB[8] = {3, 3, 2, 2, 2, 2, 4, 2}, IB2[8] = {0, 0, 0, 0, 3, 2, 0, 0};
    Bits bs{blk, mode + 1};
    const uint32_t ns = NS[mode], part = bs.Get(PB[mode]), rot = bs.Get(RB[mode]), isel = bs.Get(ISB[mode]);
    uint32_t ep[6][4];
    for (int c = 0; c < 3; c++) for (uint32_t e = 0; e < 2 * ns; e++) ep[e][c] = bs.Get(CB[mode]);
    for (uint32_t e = 0; e < 2 * ns; e++) ep[e][3] = AB[mode] ? bs.Get(AB[mode]) : 255u;
    uint32_t cbits = CB[mode], abits = AB[mode];
    if (EPB[mode]) { for (uint32_t e = 0; e < 2 * ns; e++) { const uint32_t pbit = bs.Get(1); for (int c = 0; c < 3; c++) ep[e][c] = (ep[e][c] << 1) | pbit; if (abits) ep[e][3] = (ep[e][3] << 1) | pbit; } cbits++; if (abits) abits++; }
    else if (SPB[mode]) { for (uint32_t s = 0; s < ns; s++) { const uint32_t pbit = bs.Get(1); for (uint32_t e = 2 * s; e < 2 * s + 2; e++) for (int c = 0; c < 3; c++) ep[e][c] = (ep[e][c] << 1) | pbit; } cbits++; }
    for (uint32_t e = 0; e < 2 * ns; e++)
    {
        for (int c = 0; c < 3; c++) { ep[e][c] <<= (8 - cbits); ep[e][c] |= ep[e][c] >> cbits; }
        if (abits) { ep[e][3] <<= (8 - abits); ep[e][3] |= ep[e][3] >> abits; }
    }
    const uint32_t an = Anchors(part);
    auto subsetOf = [&](int i) -> uint32_t { return ns == 1 ? 0u : (((ns == 2 ? Part2(part) : Part3(part)) >> (2 * i)) & 3u); };
    auto isAnchor = [&](int i) { if (i == 0) return true; if (ns == 2) return (uint32_t)i == (an & 15u); if (ns == 3) return (uint32_t)i == ((an >> 4) & 15u) || (uint32_t)i == ((an >> 8) & 15u); return false; };
    uint32_t idx[16], idx2[16];
    for (int i = 0; i < 16; i++) idx[i] = bs.Get(IB[mode] - (isAnchor(i) ? 1u : 0u));
    if (IB2[mode]) for (int i = 0; i < 16; i++) idx2[i] = bs.Get(IB2[mode] - (i == 0 ? 1u : 0u));
    auto weight = [](uint32_t bits, uint32_t i) -> uint32_t { return bits == 2 ? kW2[i] : (bits == 3 ? kW3[i] : kW4[i]); };
    for (int i = 0; i < 16; i++)
    {
        const uint32_t s = subsetOf(i);
        uint32_t cw, aw;
        if (IB2[mode]) { const uint32_t w1 = weight(IB[mode], idx[i]), w2 = weight(IB2[mode], idx2[i]); cw = isel ? w2 : w1; aw = isel ? w1 : w2; }
        else cw = aw = weight(IB[mode], idx[i]);
        uint8_t px[4];
        for (int c = 0; c < 3; c++) px[c] = Interp(ep[2 * s][c], ep[2 * s + 1][c], cw);
        px[3] = Interp(ep[2 * s][3], ep[2 * s + 1][3], aw);
        if (rot) { const uint8_t t = px[3]; px[3] = px[rot - 1]; px[rot - 1] = t; }
        memcpy(out[i], px, 4);
    }
}
static inline void Bc4Block(const uint8_t* b, uint8_t out[16])
{
    uint32_t r[8]; r[0] = b[0]; r[1] = b[1];
    if (r[0] > r[1]) for (int i = 1; i < 7; i++) r[1 + i] = ((7 - i) * r[0] + i * r[1]) / 7;
    else { for (int i = 1; i < 5; i++) r[1 + i] = ((5 - i) * r[0] + i * r[1]) / 5; r[6] = 0; r[7] = 255; }
    uint64_t bits = 0; for (int i = 0; i < 6; i++) bits |= (uint64_t)b[2 + i] << (8 * i);
    for (int i = 0; i < 16; i++) out[i] = (uint8_t)r[(bits >> (3 * i)) & 7];
}

/* ------------------------------------------------------------------------------------------------ the lane form */
struct Block { uint32_t w0, w1, w2, w3; };
/* n <= 8 bits at bit position pos of the block; n == 0 gives 0 at any pos <= 128 */
ZR_HD uint32_t Field(const Block& b, uint32_t pos, uint32_t n)
{
    /* the four words are read BEFORE the selects: the compiler turns a select between two loads into one load through a selected address, an indexed array */
    const uint32_t w0 = b.w0, w1 = b.w1, w2 = b.w2, w3 = b.w3;
    const uint32_t k = pos >> 5, s = pos & 31u;
    const uint32_t lo = k == 0u ? w0 : (k == 1u ? w1 : (k == 2u ? w2 : w3));
    const uint32_t hi = k == 0u ? w1 : (k == 1u ? w2 : (k == 2u ? w3 : 0u));
    return ((lo >> s) | ((hi << 1) << (31u - s))) & ((1u << n) - 1u);
}
/* a value of `bits` in [1, 8] bits to 8 bits by replicating its top bits */
ZR_HD uint32_t Expand(uint32_t v, uint32_t bits) { const uint32_t x = v << (8u - bits); return x | (x >> bits); }
/* the specification's weight table for `bits` index bits: 2, 3 or 4 */
ZR_HD uint32_t Weight(uint32_t bits, uint32_t idx)
{
    const uint32_t d = (1u << bits) - 1u, rcp = bits == 2u ? 21846u : (bits == 3u ? 9363u : 4370u);      /* ceil(2^16 / d) */
    return ((64u * idx + (d >> 1)) * rcp) >> 16;
}

struct Bc7
{
    Block b;
    uint32_t ep[6];      /* endpoint e as R | G << 8 | B << 16 | A << 24; only ever indexed with constants */
    uint32_t valid, subsets, a1, a2, ib, ib2, ibase, ibase2, isel, rot;
};
ZR_HD void Bc7Begin(const Block& b, Bc7& s)
{
    s.b = b;
    const uint32_t unary = (uint32_t)__builtin_ctz((b.w0 & 0xffu) | 0x100u);      /* 8: the reserved mode */
    s.valid = unary < 8u ? 1u : 0u;
    const uint32_t mode = unary & 7u;
    const uint32_t ns = ModeParam(kNS, mode), pb = ModeParam(kPB, mode), rb = ModeParam(kRB, mode), isb = ModeParam(kISB, mode);
    const uint32_t cb = ModeParam(kCB, mode), ab = ModeParam(kAB, mode), epb = ModeParam(kEPB, mode), spb = ModeParam(kSPB, mode);
    s.ib = ModeParam(kIB, mode); s.ib2 = ModeParam(kIB2, mode);
    uint32_t pos = mode + 1u;
    const uint32_t part = Field(b, pos, pb); pos += pb;
    s.rot = Field(b, pos, rb); pos += rb;
    s.isel = Field(b, pos, isb); pos += isb;
    const uint32_t ne = 2u * ns, apos = pos + 3u * ne * cb, ppos = apos + ne * ab, anyP = epb | spb;
    const uint32_t cbits = cb + anyP, abits = ab ? ab + epb : 0u;
    ZR_UNROLL
    for (uint32_t e = 0; e < 6u; e++)
    {
        uint32_t v = 0u;
        if (e < ne)
        {
            const uint32_t p = Field(b, ppos + (epb ? e : (e >> 1)), anyP);
            uint32_t r = Field(b, pos + e * cb, cb), g = Field(b, pos + (ne + e) * cb, cb), bl = Field(b, pos + (2u * ne + e) * cb, cb), a = Field(b, apos + e * ab, ab);
            if (anyP) { r = (r << 1) | p; g = (g << 1) | p; bl = (bl << 1) | p; a = (a << 1) | p; }
            a = abits ? Expand(a, abits) : 255u;
            v = Expand(r, cbits) | (Expand(g, cbits) << 8) | (Expand(bl, cbits) << 16) | (a << 24);
        }
        s.ep[e] = v;
    }
    s.ibase = ppos + (epb ? ne : (spb ? ns : 0u));
    s.ibase2 = s.ibase + 16u * s.ib - 1u;
    const uint32_t an = ns > 1u ? Anchors(part) : 0u;
    s.subsets = ns == 1u ? 0u : (ns == 2u ? Part2(part) : Part3(part));
    s.a1 = ns == 2u ? (an & 15u) : (ns == 3u ? ((an >> 4) & 15u) : 16u);      /* 16: none */
    s.a2 = ns == 3u ? ((an >> 8) & 15u) : 16u;
}
/* texel i = 4 y + x of the block, as R | G << 8 | B << 16 | A << 24 */
ZR_HD uint32_t Bc7Texel(const Bc7& s, uint32_t i)
{
    if (!s.valid) return 0u;
    const uint32_t sub = (s.subsets >> (2u * i)) & 3u;
    const uint32_t p0 = s.ep[0], p1 = s.ep[1], p2 = s.ep[2], p3 = s.ep[3], p4 = s.ep[4], p5 = s.ep[5];      /* read first, as in Field */
    const uint32_t e0 = sub == 0u ? p0 : (sub == 1u ? p2 : p4), e1 = sub == 0u ? p1 : (sub == 1u ? p3 : p5);
    const uint32_t anchor = (i == 0u || i == s.a1 || i == s.a2) ? 1u : 0u;
    const uint32_t before = (i > 0u ? 1u : 0u) + (i > s.a1 ? 1u : 0u) + (i > s.a2 ? 1u : 0u);
    uint32_t cw = Weight(s.ib, Field(s.b, s.ibase + i * s.ib - before, s.ib - anchor)), aw = cw;
    if (s.ib2)
    {
        const uint32_t w2 = Weight(s.ib2, Field(s.b, s.ibase2 + i * s.ib2 - (i > 0u ? 1u : 0u), s.ib2 - (i == 0u ? 1u : 0u)));
        if (s.isel) cw = w2; else aw = w2;
    }
    /* (a (64 - w) + b w + 32) >> 6 per channel; R and B share one multiply (each product is < 2^14) */
    const uint32_t rb = (((e0 & 0x00ff00ffu) * (64u - cw) + (e1 & 0x00ff00ffu) * cw + 0x00200020u) >> 6) & 0x00ff00ffu;
    const uint32_t g = (((e0 >> 8) & 0xffu) * (64u - cw) + ((e1 >> 8) & 0xffu) * cw + 32u) >> 6;
    const uint32_t a = ((e0 >> 24) * (64u - aw) + (e1 >> 24) * aw + 32u) >> 6;
    uint32_t px = rb | (g << 8) | (a << 24);
    if (s.rot)
    {   /* rotation 1 / 2 / 3: alpha changes places with R / G / B */
        const uint32_t sh = 8u * (s.rot - 1u), c = (px >> sh) & 0xffu;
        px = (px & 0x00ffffffu & ~(0xffu << sh)) | ((px >> 24) << sh) | (c << 24);
    }
    return px;
}
/* BC4: the 8-byte block as two words, texel i in [0, 16) */
ZR_HD uint32_t Bc4Texel(uint32_t lo, uint32_t hi, uint32_t i)
{
    const uint32_t r0 = lo & 0xffu, r1 = (lo >> 8) & 0xffu;
    const uint32_t k = (uint32_t)(((((uint64_t)hi << 32) | lo) >> (16u + 3u * i)) & 7u);
    if (k < 2u) return k ? r1 : r0;
    if (r0 > r1) return (((8u - k) * r0 + (k - 1u) * r1) * 9363u) >> 16;      /* / 7, exact below 1786 */
    if (k >= 6u) return k == 6u ? 0u : 255u;
    return (((6u - k) * r0 + (k - 1u) * r1) * 13108u) >> 16;                  /* / 5, exact below 1276 */
}
/* BC5: texel i as R | G << 8 */
ZR_HD uint32_t Bc5Texel(const Block& b, uint32_t i) { return Bc4Texel(b.w0, b.w1, i) | (Bc4Texel(b.w2, b.w3, i) << 8); }

/* ------------------------------------------------------------------------------------------------ mips and jobs */
ZR_HD uint32_t MipBlocks(uint32_t w, uint32_t h) { return ((w + 3u) >> 2) * ((h + 3u) >> 2); }
/* One mip of one texture for the decode kernel: `src` bytes into the payload (a multiple of 16), `dst` bytes into the texel heap, the mip's size, the
   index of its first block among all blocks of the launch, and its encoding (kSrcBc7 / kSrcBc5).  A table of jobs is sorted by first_block. */
struct Job { uint64_t src, dst; uint32_t w, h, first_block, encoding; };
/* the job that holds block `g`: the last one whose first_block is <= g (jobs[0].first_block == 0, n >= 1) */
ZR_HD uint32_t FindJob(const Job* jobs, uint32_t n, uint32_t g)
{
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (jobs[mid].first_block <= g) lo = mid; else hi = mid; }
    return lo;
}

/* ------------------------------------------------------------------------------------------------ the lane form on the host (tests/bcnmath) */
static inline Block LoadBlock(const uint8_t* p) { Block b; memcpy(&b, p, 16); return b; }      /* little-endian hosts */
static inline void DecodeMipLanes(uint32_t encoding, const uint8_t* blocks, uint32_t w, uint32_t h, uint8_t* out)
{
    const uint32_t bw = (w + 3u) / 4u, bh = (h + 3u) / 4u;
    for (uint32_t by = 0; by < bh; by++) for (uint32_t bx = 0; bx < bw; bx++)
    {
        const Block b = LoadBlock(blocks + 16u * ((size_t)by * bw + bx));
        Bc7 s{}; if (encoding == kSrcBc7) Bc7Begin(b, s);
        for (uint32_t i = 0; i < 16u; i++)
        {
            const uint32_t x = 4u * bx + (i & 3u), y = 4u * by + (i >> 2);
            if (x >= w || y >= h) continue;
            if (encoding == kSrcBc7) { const uint32_t px = Bc7Texel(s, i); memcpy(out + 4u * ((size_t)y * w + x), &px, 4); }
            else { const uint32_t px = Bc5Texel(b, i); out[2u * ((size_t)y * w + x)] = (uint8_t)px; out[2u * ((size_t)y * w + x) + 1u] = (uint8_t)(px >> 8); }
        }
    }
}

} // namespace zrbc

#endif
