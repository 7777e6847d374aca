"""Cross-stream ordering on the CPU: zetaray_amd/csrc/zr_stream_order.h (one buffer's "last write + every stream's last read") and zr_rpt_overlap.h (the
ReSTIR PT roles and each stage's accesses), compiled by tests/hostexec with a backend that logs records and waits instead of calling HIP.

The model tests drive the stages in the host order of tests/overlapcheck.py drive -- GBUFFER and CANDIDATES on stream A; TEMPORAL_REUSE, the spatial rounds
and a consumer (the denoise pass: it reads the frame's FINAL and both G-buffer sets) on stream B -- and build happens-before from stream order plus the
logged waits.  zr_pass_reset_temporal touches neither the roles nor the trackers (it waits for the device, which only adds order), so a reset point shows
here as what it does to the frame after it: no temporal resampling, no spatial round.

"Kernel granularity": a stage that launches nothing (the closing call of a frame without a spatial round) counts as the last stage before it on its
stream that did launch; an event recorded there and one recorded at that stage are the same edge.
"""
import itertools

import pytest

from tests import overlapcheck as oc
from tests.hostexec import zhx

A, B = 0, 1
LAUNCHING = ("gbuffer", "candidates", "temporal_reuse", "spatial_round", "consumer")
BUF = ("set", "target", "final", "gbuffer")


# ------------------------------------------------------------------------------------------------ the log
class Op:
    def __init__(self, index, stage, stream):
        self.index, self.stage, self.stream = index, stage, stream
        self.waits, self.records, self.creates, self.destroys, self.accesses = [], [], [], [], []      # waits: the op (index) each waited event stood for
        self.roles = None


def run(ops):
    """-> [Op].  An event stands for the last launching op enqueued on the stream it was recorded on, at the time of the record."""
    out, point_of, last_launch = [], {}, {}
    cur = None
    for kind, a, b, c in zhx.stream_order_run(ops):
        if kind == "op":
            cur = Op(a, zhx.ORDER_STAGES[b], c)
            assert cur.index == len(out) and ops[a][0] == cur.stage
            out.append(cur)
            if cur.stage in LAUNCHING:
                last_launch[c] = cur.index
        elif kind == "create":
            cur.creates.append(a)
        elif kind == "destroy":
            (cur.destroys if cur is not None else []).append(a)
        elif kind == "record":
            point_of[a] = last_launch.get(b)
            cur.records.append((a, b))
        elif kind == "wait":
            assert a == cur.stream, "a wait is issued on the stream of the stage that needs it"
            cur.waits.append((b, point_of[b]))
        elif kind == "access":
            cur.accesses.append((BUF[a], b, bool(c)))
        elif kind == "roles":
            cur.roles = {"cur": a, "oth": b, "target": c}
        elif kind == "roles2":
            cur.roles.update(final=a, fin_out=b, frame_open=bool(c))
    return out


def lone(seq):
    """the type alone: [(op name, stream)] on one StreamOrder -> [Op]"""
    return run([(name, s, 0) for name, s in seq])


# ------------------------------------------------------------------------------------------------ the type alone
def test_same_stream_acquire_issues_no_wait():
    ops = lone([("mark_written", 3), ("acquire_read", 3), ("mark_read", 3), ("acquire_write", 3), ("mark_written", 3), ("acquire_write", 3)])
    assert all(not o.waits for o in ops)


def test_write_waits_for_each_other_streams_last_read_exactly_once():
    ops = lone([("mark_read", 1), ("mark_read", 2), ("mark_read", 1), ("mark_read", 3), ("acquire_write", 3), ("acquire_write", 3), ("acquire_read", 3)])
    assert [src for _, src in ops[4].waits] == [None, None] and sorted(e for e, _ in ops[4].waits) == sorted([ops[2].records[0][0], ops[1].records[0][0]]), \
        "one wait per OTHER stream that has read, for its LAST read; none for its own"
    assert not ops[5].waits and not ops[6].waits, "a stream that is behind a point does not wait for it again"


def test_write_also_waits_for_a_foreign_write():
    ops = lone([("mark_written", 1), ("mark_read", 2), ("acquire_write", 3)])
    assert sorted(e for e, _ in ops[2].waits) == sorted([ops[0].records[0][0], ops[1].records[0][0]])


def test_read_waits_for_the_last_foreign_write_only():
    ops = lone([("mark_written", 1), ("mark_read", 2), ("mark_written", 2), ("mark_read", 3), ("acquire_read", 1), ("acquire_read", 2)])
    assert [e for e, _ in ops[4].waits] == [ops[2].records[0][0]], "stream 1 waits for stream 2's write and for no read"
    assert not ops[5].waits, "the last write was stream 2's own"


def test_a_streams_own_write_covers_its_earlier_read():
    ops = lone([("mark_read", 1), ("mark_written", 1), ("acquire_write", 2)])
    assert [e for e, _ in ops[2].waits] == [ops[1].records[0][0]]


def test_reset_forgets():
    ops = lone([("mark_written", 1), ("mark_read", 2), ("reset", 0), ("acquire_write", 3), ("acquire_read", 3), ("mark_read", 2), ("acquire_write", 3)])
    assert not ops[3].waits and not ops[4].waits
    assert not ops[5].creates, "the events outlive a Reset"
    assert [e for e, _ in ops[6].waits] == [ops[5].records[0][0]]


def test_events_are_created_once_per_buffer_and_stream():
    frame = [("acquire_write", 1), ("mark_written", 1), ("acquire_read", 2), ("mark_read", 2), ("acquire_read", 3), ("mark_read", 3)]
    ops = lone(frame * 50)
    created = [e for o in ops for e in o.creates]
    assert len(created) <= 6 and all(not o.creates for o in ops[2 * len(frame):]), "a point nobody refers to is recorded again: nothing is created in the steady state"
    assert sorted(ops[-1].destroys) == sorted(created), "the destructor destroys what was created"


# ------------------------------------------------------------------------------------------------ the model
def frame_plan(case):
    """per frame (1-based): the spatial rounds it runs and whether it accumulates, by the rules of RenderReSTIR_PT: temporal resampling needs a valid
    history (not the first frame, not the one after a reset) and a previous G-buffer; spatial rounds need temporal resampling"""
    plan, valid = {}, False
    for f in range(1, case.frames + 1):
        if case.reset_at == f:
            valid = False
        do_temporal = bool(case.temporal and valid and f >= 2)
        kw = case.cb_kw(f)
        plan[f] = {"rounds": case.nsp if do_temporal else 0, "acc": bool(kw.get("accumulate") and kw.get("camera_static"))}
        valid = True
    return plan


def frame_ops(f, info, overlap=True):
    """one frame in drive's host order -> [(name, (stage, stream, flags))]"""
    a = A if overlap else B
    seq = [(("GB", f), ("gbuffer", a, 0)), (("K11", f), ("candidates", a, 1 if info["acc"] else 0)), (("REUSE", f), ("temporal_reuse", B, 0))]
    seq += [((f"SP{k + 1}", f), ("spatial_round", B, 0)) for k in range(info["rounds"])]
    seq += [(("CLOSE", f), ("close", B, 0)), (("CONSUMER", f), ("consumer", B, 0))]
    return seq


class Model:
    def __init__(self, case_name, mode):
        self.case, self.mode = oc.CASES[case_name], mode
        self.plan = frame_plan(self.case)
        seq = [(("MODE", 0), ("set_overlap", A, 2 if mode == "carry" else 1))]
        for f in range(1, self.case.frames + 1):
            seq += frame_ops(f, self.plan[f])
        self.at = {name: i for i, (name, _) in enumerate(seq)}
        self.ops = run([op for _, op in seq])
        self.name = {i: name for name, i in self.at.items()}
        # happens-before over the launching ops: stream order + the waits
        n = len(self.ops)
        succ = [set() for _ in range(n)]
        last = {}
        for o in self.ops:
            if o.stage in LAUNCHING:
                if o.stream in last:
                    succ[last[o.stream]].add(o.index)
                last[o.stream] = o.index
            for _, src in o.waits:
                if src is not None:
                    succ[src].add(o.index)
        self.before = [set() for _ in range(n)]      # before[j] = everything ordered before op j
        for j in range(n):      # (edges only go forward in host order)
            for i in range(j):
                if j in succ[i]:
                    self.before[j] |= self.before[i] | {i}

    def op(self, stage, f):
        return self.ops[self.at[(stage, f)]] if (stage, f) in self.at else None

    def last_stage(self, f):
        return ("REUSE", "SP1", "SP2")[self.plan[f]["rounds"]]

    def ordered(self, first, then):
        return first.index in self.before[then.index]

    def waited(self, o):
        """the latest op on the other stream that `o` itself waits for (None: no cross-stream wait)"""
        src = [s for _, s in o.waits if s is not None]
        assert all(self.ops[s].stream != o.stream for s in src), "a wait is never issued on the stream that recorded the event"
        return max(src) if src else None


MODELS = {}


def model(case_name, mode):
    if (case_name, mode) not in MODELS:
        MODELS[(case_name, mode)] = Model(case_name, mode)
    return MODELS[(case_name, mode)]


ALL = [(c, m) for c in oc.CASES for m in ("product", "carry")]


def test_the_cases_are_the_ones_the_gpu_tests_drive():
    assert sorted(oc.CASES) == ["acc_no_temporal", "acc_reset", "acc_starts", "moving", "two_rounds"]
    assert all(c.frames == 6 for c in oc.CASES.values())
    assert [frame_plan(oc.CASES["two_rounds"])[f]["rounds"] for f in range(1, 7)] == [0, 2, 2, 0, 2, 2]
    assert [frame_plan(oc.CASES["acc_starts"])[f]["acc"] for f in range(1, 7)] == [False, False, True, True, True, True]
    assert all(v["rounds"] == 0 and v["acc"] for v in frame_plan(oc.CASES["acc_no_temporal"]).values())


@pytest.mark.parametrize("case_name,mode", ALL)
def test_no_hazard(case_name, mode):
    """every pair of accesses to the same storage on different streams, of which at least one is a write, is ordered -- the consumer's read of FINAL against
    the next write of that plane included (the consumer's accesses are in the log like any stage's)"""
    m = model(case_name, mode)
    acc = [(o, buf, idx, wr) for o in m.ops for buf, idx, wr in o.accesses]
    pairs = 0
    for (o1, b1, i1, w1), (o2, b2, i2, w2) in itertools.combinations(acc, 2):
        if (b1, i1) == (b2, i2) and (w1 or w2) and o1.stream != o2.stream:
            pairs += 1
            assert m.ordered(o1, o2), f"{m.name[o1.index]} and {m.name[o2.index]} both touch {b1}[{i1}] unordered"
    assert pairs > 20
    final_reads = [(o, i) for o, b, i, w in acc if o.stage == "consumer" and b == "final"]
    assert len(final_reads) == m.case.frames
    for o, i in final_reads:
        nxt = [o2 for o2, b, i2, w in acc if b == "final" and i2 == i and w and o2.index > o.index and o2.stream != o.stream]
        assert all(m.ordered(o, o2) for o2 in nxt)


@pytest.mark.parametrize("case_name,mode", ALL)
def test_edges_are_the_parents(case_name, mode):
    """each stage's cross-stream waits, frame by frame, against the table of the frame-level events this replaced:
         GB(f)                      CONSUMER(f - 2): stream B's last read of the plane set it overwrites
         K11(f), product            LAST(f - 2)
         K11(f), carry              REUSE(f - 1); LAST(f - 1) if frame f - 1 ran two spatial rounds
         K11(f), accumulating       additionally stream B's tail at enqueue time: CONSUMER(f - 1)
         REUSE(f)                   K11(f)
         SP1(f), SP2(f)             nothing
         CONSUMER(f)                GB(f)"""
    m = model(case_name, mode)
    for f in range(1, m.case.frames + 1):
        def at(stage, g):
            return m.at[(stage, g)] if g >= 1 else None
        want = {"GB": at("CONSUMER", f - 2), "REUSE": at("K11", f), "SP1": None, "SP2": None, "CONSUMER": at("GB", f)}
        if m.plan[f]["acc"] and f >= 2:
            want["K11"] = at("CONSUMER", f - 1)
        elif mode == "product":
            want["K11"] = at(m.last_stage(f - 2), f - 2) if f >= 3 else None
        else:
            want["K11"] = at(m.last_stage(f - 1) if m.plan[f - 1]["rounds"] == 2 else "REUSE", f - 1) if f >= 2 else None
        for stage, w in want.items():
            o = m.op(stage, f)
            if o is None:
                continue
            got = m.waited(o)
            assert got == w, f"{stage}({f}) waits for {m.name.get(got)}, the table says {m.name.get(w)}"
        assert not m.op("CLOSE", f).waits


@pytest.mark.parametrize("case_name,mode", ALL)
def test_overlap_is_kept(case_name, mode):
    m = model(case_name, mode)
    checked = 0
    for f in range(1, m.case.frames):
        k11 = m.op("K11", f + 1)
        if not m.plan[f + 1]["acc"]:      # (an accumulating frame goes behind the previous frame's consumers: the table)
            if mode == "product":
                assert not m.ordered(m.op("REUSE", f), k11), f"K11({f + 1}) is ordered behind REUSE({f})"
                checked += 1
            elif m.plan[f]["rounds"] == 1:
                assert not m.ordered(m.op("SP1", f), k11), f"K11({f + 1}) is ordered behind SP1({f})"
                checked += 1
        if case_name in ("moving", "two_rounds"):
            for stage in ("REUSE", "SP1", "SP2", "CONSUMER"):
                o = m.op(stage, f)
                assert o is None or not m.ordered(o, m.op("GB", f + 1)), f"GB({f + 1}) is ordered behind {stage}({f})"
            checked += 1
    assert checked or case_name.startswith("acc_")


# ---- the roles.  The parent's rules, as RenderReSTIR_PT applied them inline:
#   CANDIDATES with overlap: swap(rptSet[currIdx], rptSet[2]); tgtIdx ^= 1; finIdx = (finIdx + 1) % 3 unless the frame accumulates
#   a stage runs with cur = rptSet[currIdx], prev = rptSet[1 - currIdx], target tgtIdx, FINAL finIdx
#   after each spatial round: currIdx = 1 - currIdx;  closing the frame: currIdx = 1 - currIdx, finOut = finIdx
class ParentRoles:
    def __init__(self):
        self.set, self.c, self.tgt, self.fin, self.fin_out = [0, 1, 2], 0, 0, 0, 0

    def now(self):
        return {"cur": self.set[self.c], "oth": self.set[1 - self.c], "target": self.tgt, "final": self.fin}

    def frame(self, rounds, acc, overlap):
        """-> the roles of CANDIDATES, TEMPORAL_REUSE and each round, then FINAL's output plane after the close"""
        if overlap:
            self.set[self.c], self.set[2] = self.set[2], self.set[self.c]
            self.tgt ^= 1
            if not acc:
                self.fin = (self.fin + 1) % 3
        out = [self.now(), self.now()]
        for _ in range(rounds):
            out.append(self.now())
            self.c = 1 - self.c
        self.c = 1 - self.c
        self.fin_out = self.fin
        return out, self.fin_out


def stage_roles(ops, at, f, rounds):
    got = [ops[at[(st, f)]].roles for st in ["K11", "REUSE"] + [f"SP{k + 1}" for k in range(rounds)]]
    return [{k: r[k] for k in ("cur", "oth", "target", "final")} for r in got], ops[at[("CLOSE", f)]].roles["fin_out"]


@pytest.mark.parametrize("case_name,mode", ALL)
def test_roles_follow_the_parents_rotation(case_name, mode):
    m = model(case_name, mode)
    parent = ParentRoles()
    for f in range(1, m.case.frames + 1):
        want = parent.frame(m.plan[f]["rounds"], m.plan[f]["acc"], True)
        assert stage_roles(m.ops, m.at, f, m.plan[f]["rounds"]) == want, f"frame {f}"
        assert m.op("K11", f).roles["frame_open"] is False and m.op("REUSE", f).roles["frame_open"] is True and m.op("CLOSE", f).roles["frame_open"] is False
        # the access lists name the storage the roles name
        k11 = m.op("K11", f)
        assert {("set", want[0][0]["cur"], True), ("target", want[0][0]["target"], True), ("final", want[0][0]["final"], True)} <= set(k11.accesses)
        assert (len([a for a in k11.accesses if a[0] != "gbuffer"]) == 5) == (mode == "carry")


def test_roles_of_the_moving_case_written_out():
    """`moving`: frames 1 and 4 (the first, the one after the reset) run no round, the others one.  (cur, prev, target, FINAL) of each frame's CANDIDATES
    stage, by hand from the rules above: [0 1 | 2] -> f1 swaps slot 0: [2 1 | 0], closes on slot 1; f2 swaps slot 1: [2 0 | 1], one round and the close
    leave slot 1; f3: [2 1 | 0]; f4: [2 0 | 1], no round, so the close moves to slot 0; f5 swaps slot 0: [1 0 | 2]; f6: [2 0 | 1]"""
    m = model("moving", "product")
    got = [tuple(m.op("K11", f).roles[k] for k in ("cur", "oth", "target", "final")) for f in range(1, 7)]
    assert got == [(2, 1, 1, 1), (0, 2, 0, 2), (1, 2, 1, 0), (0, 2, 0, 1), (1, 0, 1, 2), (2, 0, 0, 0)]


def test_roles_across_overlap_off_and_on():
    """frames 1 - 2 overlapped, 3 - 4 in the plain order on one stream (zr_pass_set_frame_overlap(0): the roles stay as they stand, nothing rotates, nothing is
    recorded or waited for), 5 - 6 overlapped again -- where no stage has a predecessor yet"""
    rounds = {1: 0, 2: 1, 3: 2, 4: 1, 5: 1, 6: 2}
    on = {1: True, 2: True, 3: False, 4: False, 5: True, 6: True}
    seq = [(("MODE", 0), ("set_overlap", A, 1))]
    for f in range(1, 7):
        if f == 3:
            seq.append((("MODE", 1), ("set_overlap", A, 0)))
        if f == 5:
            seq.append((("MODE", 2), ("set_overlap", A, 2)))
        seq += frame_ops(f, {"rounds": rounds[f], "acc": False}, overlap=on[f])
    at = {name: i for i, (name, _) in enumerate(seq)}
    ops = run([op for _, op in seq])
    parent = ParentRoles()
    for f in range(1, 7):
        assert stage_roles(ops, at, f, rounds[f]) == parent.frame(rounds[f], False, on[f]), f"frame {f}"
    for f in (3, 4):
        for st in ("GB", "K11", "REUSE", "SP1", "CLOSE", "CONSUMER"):
            o = ops[at[(st, f)]]
            assert not o.waits and not o.records, f"{st}({f}) with overlap off"
    assert not ops[at[("GB", 5)]].waits and not ops[at[("K11", 5)]].waits, "after the switch no stage has a predecessor yet"
    assert [s for _, s in ops[at[("REUSE", 5)]].waits if s is not None] and max(s for _, s in ops[at[("REUSE", 5)]].waits) == at[("K11", 5)]


def test_init_resets_the_roles():
    seq = [("set_overlap", A, 1)] + [op for f in (1, 2) for _, op in frame_ops(f, {"rounds": 1, "acc": False})] + [("init", A, 0)]
    seq += [op for _, op in frame_ops(3, {"rounds": 0, "acc": False})]
    ops = run(seq)
    k11 = [o for o in ops if o.stage == "candidates"][-1]
    assert (k11.roles["cur"], k11.roles["oth"], k11.roles["target"], k11.roles["final"]) == (2, 1, 1, 1) and not k11.waits
