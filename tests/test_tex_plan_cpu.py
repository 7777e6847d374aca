"""The texture planner of the library (zetaray_amd/csrc/zr_tex_plan.h: what zr_scene_create_compressed, zr_bcn_decode_device, zr_jpeg_decode_device and
zr_mipgen_device refuse about descs, sources and JPEG records, and every job table their kernels then trust) on the CPU, through tests/hostexec.  The
refusals restate, on the same inputs, what the three GPU tests test_refusals_leave_nothing_behind ask of the entry points; null and misaligned device
pointers are the entry points' own checks and stay there.  Expected tables come from scene_io.Scene._chain_layout and zjp.record_header, never from
the header under test."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_bcn_gpu as tbc
from tests import test_jpeg_gpu as tjp
from tests import test_mipgen_gpu as tmg
from tests.bcnmath import zbc
from tests.hostexec import zhx
from tests.jpegmath import zjp
from tests.mipmath import zmg
from zetaray_amd import scene_io, wire

OK, INVALID = 0, 1      # ZR_OK, ZR_ERR_INVALID_ARG
SCENE = (zhx.TEX_SRC_ALL, zhx.TEX_PLAN_ALL)                      # zr_scene_create_compressed
BCN = (zhx.TEX_SRC_STORED, zhx.TEX_PLAN_BLOCKS)                  # zr_bcn_decode_device
JPEG = (zhx.TEX_SRC_ALL, zhx.TEX_PLAN_JPEG)                      # zr_jpeg_decode_device
MIPGEN = (0, zhx.TEX_PLAN_LEVELS)                                # zr_mipgen_device


def _variant(sc, edit, select=SCENE):
    """the planner on copies of the scene's descs, sources and payload after `edit(descs, sources, desc, blocks, payload)` changed them; desc.texel_bytes
    and blocks.payload_bytes stand for the fields of zr_scene_desc and zr_texture_blocks the GPU tests edit"""
    descs, sources, payload = sc.textures.copy(), sc.texture_sources.copy(), np.ascontiguousarray(sc.texture_payload, np.uint8).copy()
    desc, blocks = SimpleNamespace(texel_bytes=sc.texel_heap_bytes), SimpleNamespace(payload_bytes=len(payload))
    edit(descs, sources, desc, blocks, payload)
    return zhx.tex_plan(descs, sources, blocks.payload_bytes, desc.texel_bytes, payload, *select)


def _refused(sc, edits, select=SCENE):
    code, msg, plan = _variant(sc, lambda d, s, desc, b, p: None, select)
    assert code == OK and msg == "", msg
    for name, edit in edits.items():
        code, msg, _ = _variant(sc, edit, select)
        assert code == INVALID and msg, name
    return plan


# ---- 1. every refusal of the three GPU suites
def test_refusals_of_the_bcn_suite():
    sc = tbc._textured_box(np.random.default_rng(5))
    edits = {
        "unknown encoding": lambda d, s, desc, b, p: s["encoding"].__setitem__(0, 3),
        "BC7 on RG8": lambda d, s, desc, b, p: s["encoding"].__setitem__(1, zbc.BC7),
        "BC5 on RGBA8": lambda d, s, desc, b, p: s["encoding"].__setitem__(0, zbc.BC5),
        "BC5 on RGBA8 (raw texture)": lambda d, s, desc, b, p: s["encoding"].__setitem__(2, zbc.BC5),
        "BCn offset not a multiple of 16": lambda d, s, desc, b, p: s["offset"].__setitem__(1, int(s["offset"][1]) + 8),
        "RAW offset not a multiple of 4": lambda d, s, desc, b, p: s["offset"].__setitem__(2, int(s["offset"][2]) + 2),
        "chain beyond the payload": lambda d, s, desc, b, p: setattr(b, "payload_bytes", int(s["offset"][2]) + 19),
        "chain starts beyond the payload": lambda d, s, desc, b, p: s["offset"].__setitem__(0, 1 << 40),
        "desc: no mips": lambda d, s, desc, b, p: d["num_mips"].__setitem__(0, 0),
        "desc: zero width": lambda d, s, desc, b, p: d["width"].__setitem__(1, 0),
        "desc: unknown format": lambda d, s, desc, b, p: d["format"].__setitem__(0, 3),
        "desc: offset not a multiple of 4": lambda d, s, desc, b, p: d["offset"].__setitem__(1, int(d["offset"][1]) + 2),
        "desc: outside the heap": lambda d, s, desc, b, p: setattr(desc, "texel_bytes", sc.texel_heap_bytes - 1),
    }
    _refused(sc, edits)
    _refused(sc, edits, BCN)      # "the stand-alone entry point refuses the same"
    assert "multiple of 16" in _variant(sc, edits["BCn offset not a multiple of 16"])[1] and "multiple of 4" in _variant(sc, edits["RAW offset not a multiple of 4"])[1]
    code, msg, _ = zhx.tex_plan(tbc._descs([(0, 4, 4, 1, wire.TEX_RG8)]), tbc._sources([(0, zbc.BC7)]), 16, 64, None, *BCN)
    assert code == INVALID and "BC7" in msg
    # more than 2^32 - 1 blocks, as the GPU suite asks: 16 textures of 65535^2 are 2^32 blocks
    n = 16
    code, msg, _ = zhx.tex_plan(tbc._descs([(0, 65535, 65535, 1, wire.TEX_RGBA8)] * n), tbc._sources([(0, zbc.BC7)] * n), 1 << 62, 1 << 62, None, *SCENE)
    assert code == INVALID and "2^32 - 1 blocks" in msg


def test_refusals_of_the_mipgen_suite():
    sc = tmg._mixed_box(np.random.default_rng(5))
    payload_end = len(sc.texture_payload)
    assert int(sc.texture_sources["encoding"][4]) == wire.TEX_SRC_RAW_MIP0 and int(sc.texture_sources["offset"][4]) + 64 == payload_end
    edits = {
        "encoding 3 is still unknown": lambda d, s, desc, b, p: s["encoding"].__setitem__(1, 3),
        "encoding 9": lambda d, s, desc, b, p: s["encoding"].__setitem__(1, 9),
        "RAW_MIP0 offset not a multiple of 4": lambda d, s, desc, b, p: s["offset"].__setitem__(3, int(s["offset"][3]) + 2),
        "level 0 ends beyond the payload": lambda d, s, desc, b, p: setattr(b, "payload_bytes", payload_end - 1),
        "level 0 starts beyond the payload": lambda d, s, desc, b, p: s["offset"].__setitem__(1, 1 << 40),
        "desc: zero height": lambda d, s, desc, b, p: d["height"].__setitem__(1, 0),
        "desc: unknown format": lambda d, s, desc, b, p: d["format"].__setitem__(3, 3),
        "desc: outside the heap": lambda d, s, desc, b, p: setattr(desc, "texel_bytes", int(d["offset"][4]) + 63),
        "RAW needs the whole chain in the payload": lambda d, s, desc, b, p: (s["encoding"].__setitem__(4, wire.TEX_SRC_RAW), d["num_mips"].__setitem__(4, 2)),
    }
    _refused(sc, edits)
    # the level-0 size is what the chain-end check uses: the last source may end exactly with the payload although its chain is longer
    assert _variant(sc, lambda d, s, desc, b, p: setattr(b, "payload_bytes", payload_end))[0] == OK
    # zr_mipgen_device: descs alone
    rows = [(0, 9, 7, 4, wire.TEX_RG8), (256, 8, 8, 4, wire.TEX_RGBA8_SRGB)]

    def run(rows, bytes_=1024):
        return zhx.tex_plan(zmg.descs(rows), None, 0, bytes_, None, *MIPGEN)[0]

    assert run([(0, 9, 7, 4, 3)]) == INVALID, "unknown format"
    assert run([(0, 0, 7, 1, wire.TEX_RG8)]) == INVALID and run([(0, 9, 0, 1, wire.TEX_RG8)]) == INVALID, "zero dimensions"
    assert run([(0, 9, 7, 0, wire.TEX_RG8)]) == INVALID and run([(2, 9, 7, 4, wire.TEX_RG8)]) == INVALID
    assert run(rows, bytes_=256 + zmg.chain_bytes(8, 8, 4, wire.TEX_RGBA8_SRGB) - 1) == INVALID, "a chain that ends beyond texel_bytes"
    assert run(rows, bytes_=256 + zmg.chain_bytes(8, 8, 4, wire.TEX_RGBA8_SRGB)) == OK


def test_refusals_of_the_jpeg_suite():
    sc = tjp._mixed_box(np.random.default_rng(5))
    _u32 = tjp._u32
    r0, r2 = int(sc.texture_sources["offset"][0]), int(sc.texture_sources["offset"][2])
    h0 = zjp.record_header(sc.texture_payload[r0:])
    B0 = int(h0["num_blocks"])
    assert int(h0["ncomp"]) == 3 and B0 == 36
    comp0 = r0 + 40      # the first component's entry of the record's header: hs, vs, bw, bh, first_block
    begin = r0 + 496
    edits = {
        "wrong magic": lambda d, s, desc, b, p: _u32(p, r0, 0x12345678),
        "the record ends beyond the payload": lambda d, s, desc, b, p: (p.__setitem__(slice(r0 + 8, r0 + 16), np.frombuffer(np.uint64(len(p) - r0 + 1).tobytes(), np.uint8))),
        "a header cut by the payload's end": lambda d, s, desc, b, p: (s["offset"].__setitem__(2, (len(p) - 100) // 16 * 16)),
        "the record starts beyond the payload": lambda d, s, desc, b, p: s["offset"].__setitem__(0, 1 << 40),
        "offset not a multiple of 16": lambda d, s, desc, b, p: s["offset"].__setitem__(0, r0 + 8),
        "w differs from the desc": lambda d, s, desc, b, p: d["width"].__setitem__(0, 34),
        "h differs from the desc": lambda d, s, desc, b, p: d["height"].__setitem__(2, 24),
        "an RGBA map on RG8": lambda d, s, desc, b, p: _u32(p, r2 + 28, wire.JPEG_MAP_RGBA),
        "an RG map on RGBA8": lambda d, s, desc, b, p: _u32(p, r0 + 28, wire.JPEG_MAP_BG),
        "unknown map": lambda d, s, desc, b, p: _u32(p, r0 + 28, 3),
        "4:1:1 sampling": lambda d, s, desc, b, p: _u32(p, comp0, 4),
        "4:4:0 sampling": lambda d, s, desc, b, p: (_u32(p, comp0, 1), _u32(p, comp0 + 4, 2)),
        "two components": lambda d, s, desc, b, p: _u32(p, r0 + 24, 2),
        "a block row more than the size gives": lambda d, s, desc, b, p: _u32(p, comp0 + 12, 5),
        "a block count that does not follow": lambda d, s, desc, b, p: _u32(p, r0 + 32, B0 + 1),
        "coef_begin does not start at 0": lambda d, s, desc, b, p: _u32(p, begin, 1),
        "coef_begin stands still": lambda d, s, desc, b, p: _u32(p, begin + 4 * 5, int(np.frombuffer(p[begin + 16:begin + 20].tobytes(), "<u4")[0])),
        "coef_begin steps by more than 64": lambda d, s, desc, b, p: [_u32(p, begin + 4 * k, int(np.frombuffer(p[begin + 4 * k:begin + 4 * k + 4].tobytes(), "<u4")[0]) + 64) for k in range(3, B0 + 1)],
        "coef_begin decreases": lambda d, s, desc, b, p: _u32(p, begin + 4 * 7, 2),
        "the coefficients end beyond the record": lambda d, s, desc, b, p: (p.__setitem__(slice(r0 + 8, r0 + 16), np.frombuffer(np.uint64(int(h0["bytes"]) - 2).tobytes(), np.uint8))),
        "encoding 3 is still unknown": lambda d, s, desc, b, p: s["encoding"].__setitem__(0, 3),
        "encoding 9 is still unknown": lambda d, s, desc, b, p: s["encoding"].__setitem__(0, 9),
        "encoding 17": lambda d, s, desc, b, p: s["encoding"].__setitem__(0, 17),
    }
    _refused(sc, edits)
    _refused(sc, edits, JPEG)      # "zr_jpeg_decode_device refuses the same"
    assert "wrong magic" in _variant(sc, edits["wrong magic"])[1] and "34 x 17" in _variant(sc, edits["w differs from the desc"])[1]
    # what the GPU suite asks of zr_jpeg_decode_device on one 33 x 17 record
    descs, sources, payload, nbytes, _ = tjp._call([(tjp.FILES["33x17_420_q90_noise"], wire.JPEG_MAP_RGBA, wire.TEX_RGBA8)])

    def run(descs=descs, pb=len(payload), tb=nbytes):
        return zhx.tex_plan(descs, sources, pb, tb, payload, *JPEG)[0]

    assert run() == OK
    assert run(pb=len(payload) - 17) == INVALID, "a record that ends beyond payload_bytes"
    assert run(tb=int(descs["offset"][0]) + 33 * 17 * 4 - 1) == INVALID, "a level 0 that ends beyond texel_bytes"
    d2 = descs.copy()
    d2["format"] = wire.TEX_RG8
    assert run(descs=d2) == INVALID


# ---- 2. the two 2^32 - 1 refusals at their exact seams.  The planner reads descs, sources and record headers, never texels or blocks, so no payload or
# heap of that size has to exist: on the CPU these cost nothing
def test_more_than_2_32_minus_1_blocks():
    per = zbc.mip_blocks(16384, 16384)
    assert per == 1 << 24

    def run(n):
        descs = tbc._descs([(0, 16384, 16384, 1, wire.TEX_RGBA8)] * n)
        return zhx.tex_plan(descs, tbc._sources([(0, zbc.BC7)] * n), 16 * per, 16384 * 16384 * 4, None, *BCN)      # (every texture names the same source offset)

    code, msg, plan = run(255)
    assert code == OK and plan["num_blocks"] == 255 * per and len(plan["block_jobs"]) == 255 and int(plan["block_jobs"]["first_block"][254]) == 254 * per
    code, msg, _ = run(256)
    assert code == INVALID and msg == "more than 2^32 - 1 blocks"


def test_more_than_2_32_minus_1_jpeg_texels():
    big = zjp.make_gray_record(np.zeros((256 * 256, 64)), 256, 256)      # one all-grey 2048 x 2048 record, named by every texture

    def run(n):
        d, s = np.zeros(n, wire.TEXTURE_DESC), np.zeros(n, wire.TEXTURE_SOURCE)
        d["width"], d["height"], d["num_mips"], d["format"] = 2048, 2048, 1, wire.TEX_RGBA8
        s["encoding"] = wire.TEX_SRC_JPEG_COEF
        return zhx.tex_plan(d, s, len(big), 2048 * 2048 * 4, big, *JPEG)

    code, msg, plan = run(1023)
    assert code == OK and plan["jpeg_items"] == 1023 << 22 and int(plan["jpeg_tex_jobs"]["first_item"][1022]) == 1022 << 22
    for n in (1024, 1025):      # (1024 of them are 2^32 texels exactly: one too many)
        code, msg, _ = run(n)
        assert code == INVALID and "2^32 - 1" in msg and "texels" in msg


# ---- 3. the job tables of one mixed call
def _expected_tables(sc):
    """every table of the plan of a scene's sources, from scene_io.Scene._chain_layout and the record headers"""
    want = {k: [] for k in ("block_jobs", "copies", "jpeg_block_jobs", "jpeg_tex_jobs", "chains")}
    blocks = jblocks = jitems = plane = 0
    level_offsets, generated = [], []
    for i, (t, s) in enumerate(zip(sc.textures, sc.texture_sources)):
        enc, at, to, fmt = int(s["encoding"]), int(s["offset"]), int(t["offset"]), int(t["format"])
        rec = zjp.record_header(sc.texture_payload[at:]) if enc == wire.TEX_SRC_JPEG_COEF else None
        layout = scene_io.Scene._chain_layout(int(t["width"]), int(t["height"]), int(t["num_mips"]), fmt, enc, int(rec["bytes"]) if rec is not None else 0)
        dst = [to + sum(l[3] for l in layout[:m]) for m in range(len(layout) + 1)]
        src = [at + sum(l[2] for l in layout[:m]) for m in range(len(layout) + 1)]
        level_offsets.append(dst)
        want["chains"].append((to, dst[-1]))
        if enc in (wire.TEX_SRC_BC7, wire.TEX_SRC_BC5):
            for m, (w, h, nsrc, _) in enumerate(layout):
                want["block_jobs"].append((src[m], dst[m], w, h, blocks, enc))
                blocks += nsrc // 16
        elif enc in (wire.TEX_SRC_RAW, wire.TEX_SRC_RAW_MIP0):
            want["copies"].append((at, to, src[-1] - at))
        else:
            ncomp, B = int(rec["ncomp"]), int(rec["num_blocks"])
            planes = []
            for c in rec["comp"][:ncomp]:
                nat = np.zeros(64, np.uint32)
                nat[zjp.ZZ] = c["q"]
                want["jpeg_block_jobs"].append((at + 496, at + 496 + 4 * (B + 1), plane, int(c["bw"]), int(c["first_block"]), jblocks + int(c["first_block"]), 0, nat[0::2] | (nat[1::2] << 16)))
                planes.append((plane, 8 * int(c["bw"])))
                plane += 64 * int(c["bw"]) * int(c["bh"])
            planes += [(0, 0)] * (3 - ncomp)
            want["jpeg_tex_jobs"].append((to, [p[0] for p in planes], [p[1] for p in planes], int(rec["w"]), int(rec["h"]), ncomp, int(rec["comp"][0]["hs"]), int(rec["comp"][0]["vs"]),
                                          int(rec["map"]), jitems))
            jblocks, jitems = jblocks + B, jitems + int(rec["w"]) * int(rec["h"])
        if enc in (wire.TEX_SRC_RAW_MIP0, wire.TEX_SRC_JPEG_COEF):
            generated.append((i, layout))
    want["mip_jobs"], want["levels"] = [], []
    for k in range(1, max([len(l) for _, l in generated] + [1])):
        first, items = len(want["mip_jobs"]), 0
        for i, layout in generated:
            if len(layout) > k:
                want["mip_jobs"].append((level_offsets[i][k - 1], level_offsets[i][k], layout[k - 1][0], layout[k - 1][1], layout[k][0], layout[k][1], int(sc.textures["format"][i]), items))
                items += layout[k][0] * layout[k][1]
        want["levels"].append((first, len(want["mip_jobs"]) - first, items))
    counts = {"num_blocks": blocks, "jpeg_blocks": jblocks, "jpeg_items": jitems, "plane_bytes": plane}
    return want, counts


def _assert_tables(plan, want, counts, names):
    for name in names:
        got = plan[name]
        assert len(got) == len(want[name]), (name, len(got), len(want[name]))
        for k, row in enumerate(want[name]):
            for field, value in zip(got.dtype.names, row):
                assert np.array_equal(got[field][k], np.asarray(value, got.dtype[field].base)), (name, k, field, got[field][k], value)
    for name, value in counts.items():
        assert plan[name] == value, (name, plan[name], value)


def test_job_tables_of_one_mixed_call():
    sc, order = zjp.five_encoding_box(np.random.default_rng(17))
    assert order != sorted(order) and list(np.argsort(sc.textures["offset"])) == order
    want, counts = _expected_tables(sc)
    assert [len(want[k]) for k in ("block_jobs", "copies", "jpeg_block_jobs", "jpeg_tex_jobs")] == [6, 2, 4, 2] and len(want["levels"]) == 5 and len(want["mip_jobs"]) == 2 + 1 + 5
    assert int(zjp.record_header(sc.texture_payload[int(sc.texture_sources["offset"][3]):])["comp"][0]["hs"]) == 2, "the 33 x 17 file is 4:2:0"
    code, msg, plan = zhx.tex_plan(sc.textures, sc.texture_sources, len(sc.texture_payload), sc.texel_heap_bytes, sc.texture_payload, *SCENE)
    assert code == OK, msg
    _assert_tables(plan, want, counts, ("block_jobs", "copies", "jpeg_block_jobs", "jpeg_tex_jobs", "mip_jobs", "levels", "chains"))
    # the chains cover the heap but for its padding, and no two of them overlap
    c = np.sort(plan["chains"], order="first")
    assert (c["first"][1:] >= c["end"][:-1]).all() and int(c["first"][0]) == 8 and int(c["end"][-1]) + 24 == sc.texel_heap_bytes


# ---- 4. what each caller's selection refuses and leaves alone
def test_selections_of_the_four_callers():
    sc, _ = zjp.five_encoding_box(np.random.default_rng(17))
    want, counts = _expected_tables(sc)
    args = (len(sc.texture_payload), sc.texel_heap_bytes, sc.texture_payload)
    # zr_bcn_decode_device: RAW_MIP0 and JPEG_COEF are unknown encodings, in texture order
    code, msg, _ = zhx.tex_plan(sc.textures, sc.texture_sources, *args, *BCN)
    assert code == INVALID and msg == "texture 0 has the unknown source encoding %u" % wire.TEX_SRC_RAW_MIP0
    code, msg, _ = zhx.tex_plan(sc.textures[1:], sc.texture_sources[1:], *args, *BCN)
    assert code == INVALID and msg == "texture 2 has the unknown source encoding %u" % wire.TEX_SRC_JPEG_COEF
    stored = [1, 2, 5]
    code, msg, plan = zhx.tex_plan(sc.textures[stored], sc.texture_sources[stored], *args, *BCN)
    assert code == OK, msg
    _assert_tables(plan, want, {"num_blocks": counts["num_blocks"]}, ("block_jobs",))
    assert [tuple(int(v) for v in r) for r in plan["copies"]] == [want["copies"][1]], "the RAW chain alone"
    assert [len(plan[k]) for k in ("jpeg_block_jobs", "jpeg_tex_jobs", "mip_jobs", "levels")] == [0, 0, 0, 0]
    # zr_jpeg_decode_device: plans the records alone ...
    code, msg, plan = zhx.tex_plan(sc.textures, sc.texture_sources, *args, *JPEG)
    assert code == OK, msg
    _assert_tables(plan, want, {k: counts[k] for k in ("jpeg_blocks", "jpeg_items", "plane_bytes")}, ("jpeg_block_jobs", "jpeg_tex_jobs", "chains"))
    assert [len(plan[k]) for k in ("block_jobs", "copies", "mip_jobs", "levels")] == [0, 0, 0, 0] and plan["num_blocks"] == 0
    # ... and validates the sources it plans nothing for: a BC7 source on an RG8 desc, a BC7 chain cut by the payload's end
    s2 = sc.texture_sources.copy()
    s2["encoding"][5] = wire.TEX_SRC_BC7
    code, msg, _ = zhx.tex_plan(sc.textures, s2, *args, *JPEG)
    assert code == INVALID and msg == "texture 5 is BC7 but its format is not RGBA8 / RGBA8_SRGB"
    cut = int(sc.texture_sources["offset"][2]) + 47
    code, msg, _ = zhx.tex_plan(sc.textures[:3], sc.texture_sources[:3], cut, sc.texel_heap_bytes, sc.texture_payload, *JPEG)
    assert code == INVALID and msg == "the chain of texture 2 ends beyond the payload (%d > %d bytes)" % (cut + 1, cut)
    # zr_mipgen_device: no sources, the levels of every texture
    code, msg, plan = zhx.tex_plan(sc.textures, None, 0, sc.texel_heap_bytes, None, *MIPGEN)
    assert code == OK, msg
    assert [len(plan[k]) for k in ("block_jobs", "copies", "jpeg_block_jobs", "jpeg_tex_jobs")] == [0, 0, 0, 0]
    every = sc
    mips = [int(m) for m in every.textures["num_mips"]]
    assert len(plan["levels"]) == max(mips) - 1 and len(plan["mip_jobs"]) == sum(m - 1 for m in mips)
    assert [int(l["num_jobs"]) for l in plan["levels"]] == [sum(1 for m in mips if m > k) for k in range(1, max(mips))]
    lv1 = plan["mip_jobs"][:len(mips)]
    assert [int(v) for v in lv1["src"]] == [int(o) for o in every.textures["offset"]], "level 1 of every texture, in texture order, from its level 0"
    assert [int(v) for v in lv1["first_item"]] == list(np.cumsum([0] + [max(1, int(t["width"]) >> 1) * max(1, int(t["height"]) >> 1) for t in every.textures[:-1]]))
