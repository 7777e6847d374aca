// TEST-ONLY host compilation of include/zr_bcn.h: the lane form the decode kernel compiles (Bc7Begin / Bc7Texel / Bc5Texel), and the loader's own
// decoder next to it.  encoding: ZR_TEX_SRC_BC7 = 1, ZR_TEX_SRC_BC5 = 2; out: w x h texels, RGBA8 / RG8, rows top-down.
#include "../../include/zr_bcn.h"

extern "C" {
void zbc_decode_mip(uint32_t encoding, const uint8_t* blocks, uint32_t w, uint32_t h, uint8_t* out) { zrbc::DecodeMipLanes(encoding, blocks, w, h, out); }
// the fields the fixture generator reports coverage of: mode (8 = reserved), partition, rotation, index selector, and the p-bits as a mask
void zbc_bc7_fields(const uint8_t* blk, uint32_t* out5)
{
    const zrbc::Block b = zrbc::LoadBlock(blk);
    const uint32_t unary = (uint32_t)__builtin_ctz((b.w0 & 0xffu) | 0x100u), m = unary & 7u;
    uint32_t pos = m + 1u;
    const uint32_t pb = zrbc::ModeParam(zrbc::kPB, m), rb = zrbc::ModeParam(zrbc::kRB, m), isb = zrbc::ModeParam(zrbc::kISB, m);
    out5[0] = unary; out5[1] = zrbc::Field(b, pos, pb); pos += pb; out5[2] = zrbc::Field(b, pos, rb); pos += rb; out5[3] = zrbc::Field(b, pos, isb); pos += isb;
    const uint32_t ne = 2u * zrbc::ModeParam(zrbc::kNS, m), np = zrbc::ModeParam(zrbc::kEPB, m) ? ne : (zrbc::ModeParam(zrbc::kSPB, m) ? ne / 2u : 0u);
    out5[4] = zrbc::Field(b, pos + ne * (3u * zrbc::ModeParam(zrbc::kCB, m) + zrbc::ModeParam(zrbc::kAB, m)), np);
}
}
