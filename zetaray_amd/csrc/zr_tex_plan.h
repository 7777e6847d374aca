// What the texture sources of one call take to reach the texel heap: BuildTexturePlan validates untrusted descs, sources and JPEG records and lays out
// every job table the kernels of zr_tu_texdecode.hip, zr_tu_jpeg.hip and zr_tu_mipgen.hip then trust; RunTexturePlan (zr_api.hip) enqueues the plan.
// Host-only, under the rules of zr_stream_order.h (no HIP header): zr_api.hip and tests/hostexec compile these same lines, so every refusal and every
// table is tested on the CPU (tests/test_tex_plan_cpu.py).  The four callers (zr_api.hip) differ only in what they accept and which stages they ask for.
#pragma once
#include "../../include/zetaray_amd.h"
#include "../../include/zr_texture.h"
#include "../../include/zr_bcn.h"
#include "../../include/zr_mipgen.h"
#include "../../include/zr_jpeg.h"
#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace zr {

// the source encodings a caller accepts: whole stored chains (RAW, BC7, BC5), level 0 alone as texels (RAW_MIP0), level 0 alone as a JPEG record
enum : uint32_t { kTexSrcStored = 1u, kTexSrcMip0 = 2u, kTexSrcJpeg = 4u, kTexSrcAll = 7u };
// the stages a caller wants planned: the block decode and the raw copies, level 0 of the JPEG records, the generated levels
enum : uint32_t { kTexPlanBlocks = 1u, kTexPlanJpeg = 2u, kTexPlanLevels = 4u, kTexPlanAll = 7u };
// Everything one call enqueues, in the order it is enqueued
struct TexturePlan
{
    std::vector<zrbc::Job> blockJobs; uint32_t numBlocks = 0;      // one job per mip of every BC7 / BC5 chain, in texture order: one launch
    struct Copy { uint64_t src, dst, bytes; }; std::vector<Copy> copies;      // payload -> heap: one per RAW chain and per RAW_MIP0 level 0
    // one zrjp::BlockJob per component and one zrjp::TexJob per JPEG_COEF texture, in texture order (zr_tu_jpeg.hip), and the bytes of the sample planes
    std::vector<zrjp::BlockJob> jpegBlockJobs; std::vector<zrjp::TexJob> jpegTexJobs; uint64_t jpegBlocks = 0, jpegItems = 0, planeBytes = 0;
    // one zrmg::Job per generated level, grouped by level -- levels[k - 1] names the jobs of the launch that writes level k -- each group in texture order
    struct Level { uint32_t firstJob, numJobs, numItems; };
    std::vector<zrmg::Job> mipJobs; std::vector<Level> levels;
    // the bytes [first, second) of the heap each texture's chain fills, in texture order (everything else is what a caller sees as padding)
    std::vector<std::pair<uint64_t, uint64_t>> chains;
};
// is texture t one zr_scene_create accepts?  (its chain inside the texel blob, its offset a multiple of 4)
inline bool TextureDescOk(const zr_texture_desc& t, uint64_t texelBytes)
{
    const zr_tex_mip last = zr_tex_mip_of(&t, t.num_mips ? t.num_mips - 1u : 0u);
    const uint64_t end = last.offset + (uint64_t)last.w * last.h * (t.format == ZR_TEX_RG8 ? 2u : 4u);
    return t.num_mips && t.width && t.height && t.format <= ZR_TEX_RG8 && !(t.offset & 3u) && end <= texelBytes;
}
inline int TexRefuse(std::string& err, const char* fmt, ...)
{
    char buf[256]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    err = buf; return ZR_ERR_INVALID_ARG;
}
// ZR_OK and the plan, or ZR_ERR_INVALID_ARG and what is wrong in err (the plan is then half made: drop it).  Nothing is allocated on a device and no
// kernel has run when this returns, so a caller that refuses here leaves nothing behind.
// sources: one per desc (unused when accept == 0); hostPayload: the payload ON THE HOST, read for JPEG records only (null where none can be accepted).
// The sources of a stage that was not asked for are validated and counted all the same -- the stage only leaves its tables empty.  (The levels have
// nothing to validate but their texel count, which is checked where they are planned.)
inline int BuildTexturePlan(const zr_texture_desc* descs, const zr_texture_source* sources, uint32_t n, uint64_t payloadBytes, uint64_t texelBytes,
    const uint8_t* hostPayload, uint32_t accept, uint32_t stages, TexturePlan& plan, std::string& err)
{
    uint64_t blocks = 0;
    std::vector<uint32_t> generated;      // the textures whose levels below 0 are generated
    for (uint32_t i = 0; i < n; i++)
    {
        const zr_texture_desc& t = descs[i];
        if (!TextureDescOk(t, texelBytes)) return TexRefuse(err, "texture %u is malformed or lies outside the texel blob", i);
        const uint32_t bpp = t.format == ZR_TEX_RG8 ? 2u : 4u;
        bool level0Only = accept == 0u;
        if (accept)
        {
            const zr_texture_source& src = sources[i];
            const uint32_t kind = src.encoding <= ZR_TEX_SRC_BC5 ? kTexSrcStored : src.encoding == ZR_TEX_SRC_RAW_MIP0 ? kTexSrcMip0 : src.encoding == ZR_TEX_SRC_JPEG_COEF ? kTexSrcJpeg : 0u;
            const bool jpeg = kind == kTexSrcJpeg, mip0 = kind == kTexSrcMip0, raw = src.encoding == ZR_TEX_SRC_RAW || mip0;
            if (!(kind & accept)) return TexRefuse(err, "texture %u has the unknown source encoding %u", i, (unsigned)src.encoding);
            if (src.encoding == ZR_TEX_SRC_BC7 && t.format != ZR_TEX_RGBA8 && t.format != ZR_TEX_RGBA8_SRGB) return TexRefuse(err, "texture %u is BC7 but its format is not RGBA8 / RGBA8_SRGB", i);
            if (src.encoding == ZR_TEX_SRC_BC5 && t.format != ZR_TEX_RG8) return TexRefuse(err, "texture %u is BC5 but its format is not RG8", i);
            if (src.offset & (raw ? 3u : 15u)) return TexRefuse(err, "the source offset of texture %u is not a multiple of %u", i, raw ? 4u : 16u);
            if (src.offset > payloadBytes) return TexRefuse(err, "the %s of texture %u starts beyond the payload", jpeg ? "record" : "chain", i);
            level0Only = jpeg || mip0;
            if (jpeg)
            {   // the whole record is validated here, on the host, before anything is enqueued -- the kernels trust what this accepted
                zrjp::Header h;
                if (const char* why = zrjp::CheckRecord(hostPayload + src.offset, payloadBytes - src.offset, &h)) return TexRefuse(err, "the JPEG record of texture %u: %s", i, why);
                if (h.w != t.width || h.h != t.height) return TexRefuse(err, "the JPEG record of texture %u is %u x %u, its desc %u x %u", i, h.w, h.h, (unsigned)t.width, (unsigned)t.height);
                if ((h.map == (uint32_t)zrjp::kMapRgba) != (t.format != ZR_TEX_RG8)) return TexRefuse(err, "the channel map of the JPEG record of texture %u does not fit its format", i);
                if (plan.jpegBlocks + h.num_blocks > 0xffffffffull || plan.jpegItems + (uint64_t)h.w * h.h > 0xffffffffull) return TexRefuse(err, "more than 2^32 - 1 JPEG blocks or texels");
                if (stages & kTexPlanJpeg)
                {
                    zrjp::BlockJob bj[3]; zrjp::TexJob tj;
                    zrjp::MakeJobs(h, src.offset, plan.planeBytes, t.offset, (uint32_t)plan.jpegBlocks, (uint32_t)plan.jpegItems, bj, &tj);
                    plan.jpegBlockJobs.insert(plan.jpegBlockJobs.end(), bj, bj + h.ncomp); plan.jpegTexJobs.push_back(tj);
                    plan.planeBytes += zrjp::PlaneBytes(h);
                }
                plan.jpegBlocks += h.num_blocks; plan.jpegItems += (uint64_t)h.w * h.h;
            }
            else
            {
                uint64_t at = src.offset;      // (a chain is < 2^37 bytes, so `at` cannot wrap before it is compared)
                for (uint32_t m = 0; m < (mip0 ? 1u : t.num_mips); m++)      // (a RAW_MIP0 source ends with level 0)
                {
                    const zr_tex_mip mip = zr_tex_mip_of(&t, m);
                    if (raw) { at += (uint64_t)mip.w * mip.h * bpp; continue; }
                    zrbc::Job j; j.src = at; j.dst = mip.offset; j.w = mip.w; j.h = mip.h; j.first_block = (uint32_t)blocks; j.encoding = src.encoding;
                    const uint64_t nb = (uint64_t)((mip.w + 3u) >> 2) * ((mip.h + 3u) >> 2);
                    blocks += nb; at += 16u * nb;
                    if (blocks > 0xffffffffull) return TexRefuse(err, "more than 2^32 - 1 blocks");
                    if (stages & kTexPlanBlocks) plan.blockJobs.push_back(j);
                }
                if (at > payloadBytes) return TexRefuse(err, "the chain of texture %u ends beyond the payload (%llu > %llu bytes)", i, (unsigned long long)at, (unsigned long long)payloadBytes);
                if (raw && (stages & kTexPlanBlocks)) plan.copies.push_back({src.offset, t.offset, at - src.offset});
            }
        }
        if (level0Only) generated.push_back(i);
        const zr_tex_mip last = zr_tex_mip_of(&t, t.num_mips - 1u);
        plan.chains.push_back({t.offset, last.offset + (uint64_t)last.w * last.h * bpp});
    }
    plan.numBlocks = (stages & kTexPlanBlocks) ? (uint32_t)blocks : 0u;
    if (!(stages & kTexPlanLevels)) return ZR_OK;
    // the levels below 0, top down: level k of every chain that has one is read from its level k - 1, which the launch before wrote
    uint32_t maxMips = 0;
    for (uint32_t i : generated) if (descs[i].num_mips > maxMips) maxMips = descs[i].num_mips;
    for (uint32_t k = 1; k < maxMips; k++)
    {
        TexturePlan::Level lv = {(uint32_t)plan.mipJobs.size(), 0u, 0u};
        uint64_t items = 0;
        for (uint32_t i : generated)
        {
            const zr_texture_desc& t = descs[i];
            if (t.num_mips <= k) continue;
            const zr_tex_mip s = zr_tex_mip_of(&t, k - 1u), d = zr_tex_mip_of(&t, k);
            zrmg::Job j; j.src = s.offset; j.dst = d.offset; j.sw = s.w; j.sh = s.h; j.dw = d.w; j.dh = d.h; j.format = t.format; j.first_item = (uint32_t)items;
            items += (uint64_t)d.w * d.h;
            if (items > 0xffffffffull) return TexRefuse(err, "more than 2^32 - 1 texels in mip level %u", k);
            plan.mipJobs.push_back(j);
        }
        lv.numJobs = (uint32_t)plan.mipJobs.size() - lv.firstJob; lv.numItems = (uint32_t)items;
        plan.levels.push_back(lv);
    }
    return ZR_OK;
}
} // namespace zr
