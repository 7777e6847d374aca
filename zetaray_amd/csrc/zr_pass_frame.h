// The per-frame host state of the four ReSTIR passes (DI emissive, sky DI, ReSTIR GI, ReSTIR PT): the reuse flags, the copy of zr_params into a
// kernel's parameter struct, and which of a pass's two reservoir sets is which.  Host-only, under the rules of zr_stream_order.h: the render
// functions of zr_api.hip and the serial executor of tests/hostexec compile these same lines, so the CPU parity suites run the derivation the library ships.
#pragma once
#include "zr_rpt.h"
#include "zr_rdi.h"
#include "zr_sdi.h"
#include "zr_rgi.h"
namespace zr {
// What a frame reuses.  historyValid: the pass has rendered a frame since its last init / resize / reset; havePrevGBuffer: there is a previous frame's
// G-buffer to reproject into (the caller's to say: zr_gbuffer::numRendered >= 2 in the library, a non-null `prev` in tests/hostexec).
struct ReuseFlags { uint32_t accumulate, doTemporal, doSpatial, writeReservoirs; };
// ... with doTemporal / doSpatial already decided: ReSTIR PT decides them in its CANDIDATES stage and holds them for the stages that follow
inline ReuseFlags ReuseFlagsLatched(bool doTemporal, bool doSpatial, bool historyValid, const zr_frame_constants& cb)
{
    // (writeReservoirs: a frame without temporal reuse on a valid history leaves the reservoirs alone)
    return {(cb.accumulate && cb.camera_static) ? 1u : 0u, doTemporal ? 1u : 0u, doSpatial ? 1u : 0u, (doTemporal || !historyValid) ? 1u : 0u};
}
inline ReuseFlags ReuseFlagsOf(uint32_t flags, bool historyValid, bool havePrevGBuffer, const zr_frame_constants& cb)
{
    const bool doTemporal = historyValid && (flags & ZR_IND_TEMPORAL_RESAMPLE) && havePrevGBuffer;
    return ReuseFlagsLatched(doTemporal, doTemporal && (flags & ZR_IND_SPATIAL_RESAMPLE), historyValid, cb);
}

inline rdi::DiParams DiParamsOf(const zr_params& ip, const zr_frame_constants& cb, bool historyValid, bool havePrevGBuffer)
{
    const ReuseFlags f = ReuseFlagsOf(ip.flags, historyValid, havePrevGBuffer, cb);
    rdi::DiParams p;
    p.flags = ip.flags; p.M_max = ip.m_max_temporal; p.numSampleSets = ip.presampling ? ip.num_sample_sets : 0u;
    p.accumulate = f.accumulate; p.doTemporal = f.doTemporal; p.doSpatial = f.doSpatial; p.writeReservoirs = f.writeReservoirs;
    p.halfVec = (ip.flags & ZR_DI_HALF_VECTOR_COPY_SHIFT) ? 1u : 0u; p.alpha_min = ip.alpha_min;      // USE_HALF_VECTOR_COPY_SHIFT (ReSTIR_DI/Params.hlsli:12)
    return p;
}
inline sdi::SkyParams SkyParamsOf(const zr_params& ip, const zr_frame_constants& cb, bool historyValid, bool havePrevGBuffer)
{
    const ReuseFlags f = ReuseFlagsOf(ip.flags, historyValid, havePrevGBuffer, cb);
    sdi::SkyParams p;
    p.M_max_sky = ip.m_max_temporal; p.M_max_sun = ip.m_max_spatial; p.alpha_min = ip.alpha_min;
    p.accumulate = f.accumulate; p.doTemporal = f.doTemporal; p.doSpatial = f.doSpatial; p.writeReservoirs = f.writeReservoirs;
    return p;
}
// (k_rgi's frame; the library's spatial stage overrides accumulate / doTemporal / writeReservoirs / textured where it launches)
inline rgi::GiParams GiParamsOf(const zr_params& ip, const zr_frame_constants& cb, bool historyValid, bool havePrevGBuffer, bool textured)
{
    const ReuseFlags f = ReuseFlagsOf(ip.flags, historyValid, havePrevGBuffer, cb);
    rgi::GiParams p;
    p.flags = ip.flags; p.maxNonTrBounces = ip.max_non_tr_bounces; p.maxGlossyTrBounces = ip.max_glossy_tr_bounces;
    p.numSampleSets = ip.presampling ? ip.num_sample_sets : 0u; p.accumulate = f.accumulate; p.doTemporal = f.doTemporal; p.writeReservoirs = f.writeReservoirs;
    p.M_max = (float)ip.m_max_temporal; p.useLVG = (ip.use_lvg && ip.presampling) ? 1u : 0u; p.textured = textured ? 1u : 0u;
    return p;
}
// f: ReuseFlagsLatched of the pass's held doTemporal / doSpatial.  temporalMap 0: the library sets its choice where it calls.
inline rpt::RptParams RptParamsOf(const zr_params& ip, const zr_frame_constants& cb, const ReuseFlags& f, bool textured)
{
    rpt::RptParams p;
    p.maxNonTrBounces = ip.max_non_tr_bounces; p.maxGlossyTrBounces = ip.max_glossy_tr_bounces;
    p.russianRoulette = (ip.flags & ZR_IND_RUSSIAN_ROULETTE) ? 1u : 0u; p.boiling = (ip.flags & ZR_IND_BOILING_SUPPRESSION) ? 1u : 0u;
    p.numSampleSets = ip.presampling ? ip.num_sample_sets : 0u; p.alpha_min = ip.alpha_min;
    p.M_max_temporal = ip.m_max_temporal & 0xf; p.M_max_spatial = ip.m_max_spatial & 0xf;      // the reservoir caps travel in 4-bit fields of cb_ReSTIR_PT_*::Packed
    p.accumulate = f.accumulate; p.doTemporal = f.doTemporal; p.doSpatial = f.doSpatial; p.writeReservoirs = f.writeReservoirs;
    p.emissive = cb.num_emissive_triangles ? 1u : 0u; p.textured = textured ? 1u : 0u;
    p.sortTemporal = (ip.flags & ZR_IND_SORT_TEMPORAL) ? 1u : 0u; p.sortSpatial = (ip.flags & ZR_IND_SORT_SPATIAL) ? 1u : 0u; p.temporalMap = 0u;
    return p;
}

// The history of a pass: whether it has one and, for the passes with two reservoir sets, which set is which.  Set Cur() is the one the next frame's
// first stage writes (between the stages of a frame: the post-temporal set, ZR_HALO_POST_TEMPORAL); set Oth() is the one the last frame wrote -- what the
// next frame reads as "previous", what ZR_HALO_FINAL moves and what the pass's reservoir outputs name.
//   DI emissive, sky DI   Flip() when a call includes the SPATIAL stage (a TEMPORAL-only call neither flips nor validates); reset_temporal: Rewind()
//   ReSTIR GI             Flip() at the end of TEMPORAL, so its SPATIAL stage reads Oth() and refuses an invalid history; reset_temporal: Invalidate()
//   ReSTIR PT             its indices are RptRoles' (zr_rpt_overlap.h), which a reset leaves alone: `valid` only, set when the frame closes
//   TAA, DENOISE          ping-pong indices of their own ("written last", not "written next"): `valid` only
//   zr_pass_init / zr_pass_resize: Rewind() for all of them
struct PassHistory
{
    bool valid = false; int currIdx = 0;
    int Cur() const { return currIdx; }
    int Oth() const { return 1 - currIdx; }
    void Flip() { valid = true; currIdx = 1 - currIdx; }      // the frame's reservoirs are written
    void Invalidate() { valid = false; }
    void Rewind() { valid = false; currIdx = 0; }
};

} // namespace zr
