// ReSTIR PT frame overlap (zetaray_amd.h zr_pass_set_frame_overlap): which storage plays which role, and what each stage reads and writes.  Host-only,
// under the rules of zr_stream_order.h: RenderReSTIR_PT (zr_api.hip) runs it with the HIP backend, tests/hostexec with one that logs, so the CPU suite
// executes the rotation and the access lists the library uses (tests/test_stream_order_cpu.py).
#pragma once
#include <utility>
#include "zr_stream_order.h"

namespace zr {

// The roles.  set[0], set[1]: the two reservoir sets currIdx flips between; set[2]: the free one (frame overlap only).  tgt / fin: the target / FINAL
// plane of the frame whose CANDIDATES stage ran last; finOut: the FINAL plane of the last frame whose final stage has been enqueued.
struct RptRoles
{
    int set[3] = {0, 1, 2}, currIdx = 0, tgt = 0, fin = 0, finOut = 0;
    int carryFrom = -1;                 // carry mode: the set the open frame's K11 copies from (the one its set replaced); -1 otherwise
    int rounds = 0, closedRounds = 0;   // spatial rounds of the open frame / of the last closed one
    bool frameOpen = false;             // a frame's CANDIDATES stage has run, its last stage has not

    int Cur() const { return set[currIdx]; }
    int Oth() const { return set[1 - currIdx]; }
    int Target() const { return tgt; }
    int OtherTarget() const { return tgt ^ 1; }
    int Final() const { return fin; }

    void Reset() { *this = RptRoles(); }      // (zr_pass_init / zr_pass_resize; zr_pass_reset_temporal leaves the roles as they stand)
    // An overlapped frame's K11 runs beside the previous frame's reuse passes, which still read the two sets in play and that frame's target plane: it
    // writes the free set, which takes the "current" role (the set it replaces is free from here on), and the other target plane.  FINAL moves on to
    // the next of three planes, unless the frame accumulates: then it adds to the plane the frames before it wrote.
    void BeginCandidates(bool overlap, bool carry, bool accumulating)
    {
        carryFrom = -1; rounds = 0;
        if (!overlap) return;
        std::swap(set[currIdx], set[2]);
        tgt ^= 1;
        if (carry) carryFrom = set[2];
        if (!accumulating) fin = (fin + 1) % 3;
    }
    void EndCandidates() { frameOpen = true; }
    // a round reads Cur() and writes Oth(), which then becomes "current"
    void SpatialRound() { currIdx = 1 - currIdx; rounds++; }
    // the frame's last stage has been enqueued: one more flip, so that Oth() is the set the next frame reads as "previous"
    void CloseFrame() { currIdx = 1 - currIdx; frameOpen = false; finOut = fin; closedRounds = rounds; }
};

enum RptBuf { RPT_BUF_SET = 0, RPT_BUF_TARGET = 1, RPT_BUF_FINAL = 2 };
struct RptAccess { int buf, idx; bool write; };

// The roles plus one StreamOrder per buffer that two streams can touch: three reservoir sets, two target planes, three FINAL planes.  A stage calls
// Begin...(s) immediately before its launches -- which declares its accesses (acc[0 .. numAcc)) and, with overlap on, orders s behind what they
// conflict with -- and End...(s) immediately after them.  The lists are the kernels' arguments: F.cur, F.prev, F.tex.target, F.finalRGBA, carryFrom;
// they name what a stage MAY touch, whichever of its kernels a given frame launches (a frame without temporal resampling runs no reuse kernel, and
// the frame-level events this replaces were recorded all the same).  The G-buffer (F.gb, F.gbPrev) has its own trackers in zr_gbuffer.
//
// NOT tracked, because only the reuse stages (TEMPORAL_REUSE, SPATIAL, SPATIAL2) ever touch them: the replay work lists and their counts, the two
// r-buffers, the two thread maps, the spatial neighbour plane (K11 does not write it) and the sample set (read-only).  What makes that safe is the
// contract line of zr_pass_set_frame_overlap: "stream B is the same stream from frame to frame".
template<typename B> struct RptOverlap
{
    using Stream = typename B::Stream;
    RptRoles roles;
    bool overlap = false, carry = false;
    OrderPoints<B> points;      // one record per stage, shared by the buffers it marks
    StreamOrder<B> sets[3], target[2], fin[3];
    RptAccess acc[5]; int numAcc = 0;

    // forget the accesses so far (a mode switch or a re-initialisation, both behind a device synchronize): no stage has a predecessor yet
    void Forget() { for (auto& t : sets) t.Reset(); for (auto& t : target) t.Reset(); for (auto& t : fin) t.Reset(); points.Reset(); }
    void SetMode(bool on, bool carryMode) { overlap = on; carry = carryMode; Forget(); }
    void Reset() { roles.Reset(); Forget(); }

    // K11 writes the set that takes the "current" role, its target plane and its FINAL plane (an accumulating frame adds into FINAL); in carry mode
    // it first copies the replaced set and the other target plane into them
    int BeginCandidates(Stream s, bool accumulating)
    {
        roles.BeginCandidates(overlap, carry, accumulating);
        numAcc = 0;      // (what the carry reads was written last of all this stage touches: acquired first, it makes the other waits redundant)
        if (roles.carryFrom >= 0) { Declare(RPT_BUF_SET, roles.carryFrom, false); Declare(RPT_BUF_TARGET, roles.OtherTarget(), false); }
        Declare(RPT_BUF_SET, roles.Cur(), true); Declare(RPT_BUF_TARGET, roles.Target(), true); Declare(RPT_BUF_FINAL, roles.Final(), true);
        if (!overlap) return 0;
        // An accumulating frame adds into the FINAL plane of the frame before it.  That plane's readers are not the library's: "consumers of a
        // frame's outputs run on the stream of its last stage, behind it" (zetaray_amd.h).  So the plane's last write is taken to reach as far as
        // that stream's tail stands now, and acquiring the plane waits for the consumers too.  Accumulating frames therefore do not overlap.
        Stream w;
        if (accumulating && fin[roles.Final()].LastWriter(&w) && !(w == s)) if (int r = fin[roles.Final()].MarkWritten(points, w)) return r;
        // Kept from the frame-level events this replaces, not derived: in carry mode, after a frame with two spatial rounds, K11 goes behind that
        // frame's LAST stage (the last write of its FINAL plane).  The accesses above ask for less -- the copy reads the set that frame's FIRST round
        // wrote, and its second round only reads that set too -- so this wait protects no buffer of the library's; it keeps the overlap exactly as
        // wide as it was, for callers whose consumers may have come to rely on it.
        if (carry && roles.closedRounds == 2) if (int r = fin[roles.finOut].AcquireRead(points, s)) return r;
        return Acquire(s);
    }
    int EndCandidates(Stream s) { roles.EndCandidates(); return Mark(s); }
    // K12 - K14 read the "previous" set (and both G-buffer sets), and read and write the current set, the target and FINAL
    int BeginTemporalReuse(Stream s)
    {
        numAcc = 0;
        Declare(RPT_BUF_SET, roles.Oth(), false); Declare(RPT_BUF_SET, roles.Cur(), true); Declare(RPT_BUF_TARGET, roles.Target(), true); Declare(RPT_BUF_FINAL, roles.Final(), true);
        return Acquire(s);
    }
    int EndTemporalReuse(Stream s) { return Mark(s); }
    // K15 - K16 read the current set and the target, and write the other set and FINAL
    int BeginSpatialRound(Stream s)
    {
        numAcc = 0;
        Declare(RPT_BUF_SET, roles.Cur(), false); Declare(RPT_BUF_TARGET, roles.Target(), false); Declare(RPT_BUF_SET, roles.Oth(), true); Declare(RPT_BUF_FINAL, roles.Final(), true);
        return Acquire(s);
    }
    int EndSpatialRound(Stream s) { int r = Mark(s); roles.SpatialRound(); return r; }
    void CloseFrame() { roles.CloseFrame(); }
    // the stream that last wrote the target plane of the frame whose K11 ran last (K11 itself, or the temporal reuse behind it): the one to wait
    // for before the host reads K11's ray counters
    bool CandidatesStream(Stream* s) const { return target[roles.Target()].LastWriter(s); }

private:
    void Declare(int buf, int idx, bool write) { acc[numAcc++] = {buf, idx, write}; }
    StreamOrder<B>& Of(const RptAccess& a) { return a.buf == RPT_BUF_SET ? sets[a.idx] : (a.buf == RPT_BUF_TARGET ? target[a.idx] : fin[a.idx]); }
    int Acquire(Stream s)
    {
        if (!overlap) return 0;
        for (int i = 0; i < numAcc; i++) if (int r = acc[i].write ? Of(acc[i]).AcquireWrite(points, s) : Of(acc[i]).AcquireRead(points, s)) return r;
        return 0;
    }
    int Mark(Stream s)
    {
        if (!overlap) return 0;
        typename OrderPoints<B>::Point* at;
        if (int r = points.Record(s, &at)) return r;
        for (int i = 0; i < numAcc; i++) { if (acc[i].write) Of(acc[i]).MarkWritten(at); else Of(acc[i]).MarkRead(at); }
        return 0;
    }
};

} // namespace zr
