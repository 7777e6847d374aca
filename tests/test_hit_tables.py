"""The tables hit reconstruction reads on the device (zetaray_amd/csrc/zr_hit_tables.h): one decoded record per mesh instance, refilled behind every
scene update and swapped with the instance buffers, and one decoded normal per vertex.  The parity suite covers the arithmetic; these cases aim at
what only the tables can break -- a stale one, one bound to the wrong buffer set, a fill kernel that misses its tail.  Each runs ReSTIR PT (temporal
and spatial reuse on) at 96 x 64 on the 58-triangle Cornell box against the CPU oracle, which decodes per hit: G-buffer planes, FINAL, every
reservoir plane and the ray counters must be equal in every frame."""
import copy
import os

import numpy as np
import pytest

from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RPT_PLANES = ("A", "B", "C", "D", "E", "F", "G", "neighbor", "map_ctn", "map_ntc")
W, H = 96, 64


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


def _own(scene):
    """a copy whose per-frame arrays are this run's own (the fixtures are shared)"""
    sc = copy.copy(scene)
    sc.instances, sc.instance_to_world = scene.instances.copy(), scene.instance_to_world.copy()
    return sc


def _quat(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(ang / 2), [np.cos(ang / 2)]]).astype(np.float32)


def _advance(sc, moves):
    """the next frame's records in place: the begin-frame rule for every instance (Prev* = this frame's values, dTranslation = 0), then the new
    TRS of each (idx, t, q, s) in `moves` -- scene_io.move_instance for several instances at once.  Returns their object-to-world matrices."""
    scene_io.move_instance(sc, 0)
    inst, mats = sc.instances, []
    for idx, t, q, s in moves:
        t, q, s = np.asarray(t, np.float32), np.asarray(q, np.float32), np.asarray(s, np.float32)
        q = q / np.float32(np.sqrt(np.float32(np.dot(q, q))))
        old_t = inst["translation"][idx].copy()
        inst["rotation"][idx] = np.rint((q * np.float32(0.5) + np.float32(0.5)) * np.float32(65535.0)).astype(np.uint16)
        inst["scale"][idx] = scene_io.f32_to_f16_bits(s)
        inst["translation"][idx] = t
        inst["d_translation"][idx] = scene_io.f32_to_f16_bits(t - old_t)
        sc.instance_to_world[idx] = scene_io.trs_matrix(t, q, s).astype(np.float32).reshape(12)
        mats.append(sc.instance_to_world[idx].copy())
    return mats


def _run(api, scene, frames, moves_of_frame=None, via="update", overlap=False, cam=None):
    """`frames` frames against the oracle.  moves_of_frame(f) -> [(idx, t, q, s)] is the scene update issued before frame f >= 2 (an empty list: a frame
    in which nothing moves, still an update); None = no update is ever issued.  via "update": zr_scene_update_instances with records made on the
    host; "move": zr_scene_move_instances with the matrices alone -- the oracle then takes the records the device made of them."""
    from oracle import zro
    sc = _own(scene)
    prm = wire.default_params()
    r = api.Renderer(sc, W, H, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    if overlap:
        r.enable_frame_overlap(True, carry=True)
    osc = zro.OracleScene(sc, force_bvh=True)
    opt = zro.OracleRPT(osc, W, H)
    prev = None
    for f in range(1, frames + 1):
        if moves_of_frame is not None and f >= 2:
            moves = moves_of_frame(f)
            mats = _advance(sc, moves)
            if via == "update":
                r.scene.update_instances(sc.instances, sc.instance_to_world)
                osc.update_instances(sc.instances, sc.instance_to_world)
            else:
                r.move_instances([m[0] for m in moves], mats)
                inst, world = r.scene.download_instances(0)
                osc.update_instances(inst, world)
        cb = scene_io.make_frame_constants(W, H, frame_num=f, num_emissives=len(sc.emissives), **(cam or {}))
        if prev is not None:
            cb["prev_view"], cb["prev_view_inv"], cb["prev_camera_jitter"] = prev["curr_view"], prev["curr_view_inv"], prev["curr_camera_jitter"]
        prev = cb.copy()
        if len(sc.emissives) == 0:
            osc.sky_lut(cb, 256, 128)
        r.p_indirect.read_counters(reset=True)
        r.render_frame(cb)
        got = r.final()
        want = opt.render(cb, prm)
        planes, _ = r.gbuffer.download()
        oplanes, _ = osc.gbuffer(cb)
        for n, a, b in zip(wire.GB_PLANE_NAMES, planes, oplanes):
            assert np.array_equal(np.asarray(a).view(np.uint8).reshape(-1), np.asarray(b).view(np.uint8).reshape(-1)), f"frame {f}: G-buffer plane {n}"
        assert r.p_indirect.read_counters() == opt.counters, f"frame {f}: ray counters differ"
        mism = int((got.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())
        assert mism == 0, f"frame {f}: {mism} pixels of FINAL differ"
        for nm in RPT_PLANES:
            a, b = r.p_indirect.download_plane(nm), opt.plane(nm)
            if nm == "A":
                a, b = a & 0xffffff, b & 0xffffff
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"frame {f}: reservoir plane {nm} differs"
    return got


# instances of the Cornell box: 8 = the short box (A: moves every frame), 9 = the tall box (B: moves in frames 3 and 4 only); the room, its walls
# and the light (C) never move
BOX_A, BOX_B = 8, 9


def _three_mover_schedule(scene):
    tA, tB = scene.instances["translation"][BOX_A].copy(), scene.instances["translation"][BOX_B].copy()
    sB = scene.instances["scale"][BOX_B].view(np.float16).astype(np.float32)

    def moves(f):
        k = f - 1
        out = [(BOX_A, tA + np.float32([0.02 * k, 0.01 * k, -0.015 * k]), _quat((0.2, 1.0, 0.1), 0.3 + 0.11 * k),
                np.float32([0.297 * (1 + 0.05 * k), 0.297 * (1 - 0.04 * k), 0.297 * (1 + 0.02 * k)]))]
        if f in (3, 4):
            out.append((BOX_B, tB + np.float32([-0.03 * (f - 2), 0.0, 0.02 * (f - 2)]), _quat((0, 1, 0), -0.3 + 0.2 * (f - 2)),
                        sB * np.float32([1.0, 1.0 - 0.05 * (f - 2), 1.0 + 0.05 * (f - 2)])))
        return out
    return moves


@pytest.mark.parametrize("via", ["update", "move"])
def test_moving_instances_keep_both_tables_current(api, cornell_emissive, via):
    """six frames: A's rotation and non-uniform scale change every frame, B moves in frames 3 and 4 only, the rest never.  Frames 2 - 6 bind the
    previous set's table (CtT replay and reconnection), frame 5 is "moved last frame, not this one" for B, whose Prev* fields then change while its
    matrix does not.  Once through zr_scene_update_instances, once through zr_scene_move_instances."""
    got = _run(api, cornell_emissive, 6, _three_mover_schedule(cornell_emissive), via=via)
    assert got[..., :3].max() > 0


def _with_clutter(scene, total, own_vertices=False):
    """the Cornell box plus copies of its short box (the same index range; the same vertex range too unless own_vertices, which appends a copy of the
    box's 24 vertices per block) as small blocks in the room, up to `total` instances; the last one is mirrored (a negative scale component)"""
    sc = _own(scene)
    n0, extra = len(sc.instances), total - len(sc.instances)
    rng = np.random.default_rng(5)
    inst = np.concatenate([sc.instances, np.repeat(sc.instances[BOX_A:BOX_A + 1], extra)])
    world = np.concatenate([sc.instance_to_world, np.zeros((extra, 12), np.float32)])
    for k in range(extra):
        i = n0 + k
        t = np.float32([rng.uniform(-0.8, 0.8), rng.uniform(0.1, 1.8), rng.uniform(-0.8, 0.8)])
        q = _quat(rng.uniform(-1, 1, 3), rng.uniform(-3, 3))
        s = np.float32(rng.uniform(0.05, 0.12, 3))
        if k == extra - 1:
            s[0] = -s[0]
        inst["rotation"][i] = np.rint((q * np.float32(0.5) + np.float32(0.5)) * np.float32(65535.0)).astype(np.uint16)
        inst["prev_rotation"][i] = inst["rotation"][i]
        inst["scale"][i] = scene_io.f32_to_f16_bits(s)
        inst["prev_scale"][i] = inst["scale"][i]
        inst["translation"][i] = t
        inst["d_translation"][i] = 0
        world[i] = scene_io.trs_matrix(t, q, s).astype(np.float32).reshape(12)
    if own_vertices:
        v0, v1 = int(sc.instances["base_vtx_offset"][BOX_A]), int(sc.instances["base_vtx_offset"][BOX_A + 1])
        inst["base_vtx_offset"][n0:] = len(sc.vertices) + (v1 - v0) * np.arange(extra, dtype=np.uint32)
        sc.vertices = np.concatenate([scene.vertices] + [scene.vertices[v0:v1]] * extra)
    sc.instances, sc.instance_to_world = inst, world
    sc.instance_mask = np.concatenate([sc.instance_mask, np.repeat(sc.instance_mask[BOX_A:BOX_A + 1], extra)])
    sc.instance_num_tris = np.concatenate([sc.instance_num_tris, np.repeat(sc.instance_num_tris[BOX_A:BOX_A + 1], extra)])
    return sc


def _room_alone(sky_scene):
    """one instance: the 20-triangle room of the sun-and-sky Cornell box, with the vertices and indices it uses"""
    sc = copy.copy(sky_scene)
    assert sc.instances["base_vtx_offset"][0] == 0 and sc.instances["base_idx_offset"][0] == 0
    nv, ni = int(sc.instances["base_vtx_offset"][1]), int(sc.instances["base_idx_offset"][1])
    sc.vertices, sc.indices = sky_scene.vertices[:nv].copy(), sky_scene.indices[:ni].copy()
    sc.instances, sc.instance_to_world = sky_scene.instances[:1].copy(), sky_scene.instance_to_world[:1].copy()
    sc.instance_mask, sc.instance_num_tris = sky_scene.instance_mask[:1].copy(), sky_scene.instance_num_tris[:1].copy()
    return sc


@pytest.mark.parametrize("count", [1, 65, 300])
def test_edge_shapes(api, cornell_emissive, count):
    """the fill kernels' tails, block = 256 lanes: 1 instance (54 vertices) and 65 instances (130 vertices) are one partial block; 300 instances, each
    block with vertices of its own (7090), are a full block plus a tail of 44 instances, and 27 full blocks plus a tail of 178 vertices.  The last
    instance of the 65 and of the 300 has a negative scale component.  Three frames; the last instance gets a new rotation and non-uniform scale
    before frames 2 and 3, so the tables are filled at creation and refilled by an update."""
    if count == 1:
        sc = _room_alone(scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz")))
    else:
        sc = _with_clutter(cornell_emissive, count, own_vertices=count > 256)
    assert len(sc.instances) == count and len(sc.vertices) % 256 != 0 and (count <= 256 or (count % 256 != 0 and len(sc.vertices) > 256))
    last = count - 1
    t0 = sc.instances["translation"][last].copy()
    s0 = sc.instances["scale"][last].view(np.float16).astype(np.float32)

    def moves(f):
        k = f - 1
        return [(last, t0 + np.float32([0.01 * k, 0.0, -0.01 * k]), _quat((0.1, 1.0, 0.3), 0.07 * k), s0 * np.float32([1 + 0.03 * k, 1.0, 1 - 0.02 * k]))]
    _run(api, sc, 3, moves)


def test_no_update_ever_issued(api, cornell_emissive):
    """four frames under frame overlap without a scene update: the previous view binds the current tables, as it binds the current instances"""
    got = _run(api, cornell_emissive, 4, None, overlap=True)
    assert got[..., :3].max() > 0
