"""What the skinning tests share (tests/test_skin_cpu.py, tests/test_skin_gpu.py): a float64 restatement of include/zr_skin.h, the case tables of the CPU
checks, and the skinned scene of the GPU checks -- the Cornell box plus a tube whose joints are nodes of an animation table -- with its host form."""
import os

import numpy as np

from tests.animmath import zan
from tests.skinmath import zsk
from zetaray_amd import scene_io, wire

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F32, F64 = np.float32, np.float64
U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------------------------------------------- float64 restatement
def mat4(M12):
    """(..., 12) row-major 3 x 4 -> (..., 4, 4) float64 with the row (0, 0, 0, 1)"""
    M = np.asarray(M12, F64).reshape(-1, 3, 4)
    out = np.zeros((len(M), 4, 4))
    out[:, :3] = M
    out[:, 3, 3] = 1
    return out


def joint_matrix64(node_world, inverse_bind):
    """J = nodeWorld x inverseBind and the componentwise sum of |products| (the bound's magnitude)"""
    W, B = mat4(node_world), mat4(inverse_bind)
    return (W @ B)[:, :3].reshape(-1, 12), (np.abs(W) @ np.abs(B))[:, :3].reshape(-1, 12)


def blend64(J4, w):
    J4, w = np.asarray(J4, F64).reshape(-1, 4, 12), np.asarray(w, F64).reshape(-1, 4, 1)
    return (w * J4).sum(1), (np.abs(w) * np.abs(J4)).sum(1)


def position64(J4, w, p):
    """p' = sum_j w_j J_j (p, 1), and sum_j |w_j| (|J_j| (|x|, |y|, |z|, 1))"""
    J4, w = np.asarray(J4, F64).reshape(-1, 4, 3, 4), np.asarray(w, F64).reshape(-1, 4)
    ph = np.concatenate([np.asarray(p, F64).reshape(-1, 3), np.ones((len(w), 1))], 1)
    val = np.einsum("nj,njrc,nc->nr", w, J4, ph)
    mag = np.einsum("nj,njrc,nc->nr", np.abs(w), np.abs(J4), np.abs(ph))
    return val, mag


def cofactor64(M3):
    r0, r1, r2 = M3[:, 0], M3[:, 1], M3[:, 2]
    return np.stack([np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)], 1)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def normal64(M12, n):
    M3 = np.asarray(M12, F64).reshape(-1, 3, 4)[:, :, :3]
    return unit(np.einsum("nrc,nc->nr", cofactor64(M3), np.asarray(n, F64)))


def tangent64(M12, t):
    M3 = np.asarray(M12, F64).reshape(-1, 3, 4)[:, :, :3]
    return unit(np.einsum("nrc,nc->nr", M3, np.asarray(t, F64)))


def decode_oct64(codes):
    """Math.hlsli:646-658 on two UNORM16 code words, in float64"""
    c = np.asarray(codes, F64).reshape(-1, 2) / 65535.0 * 2 - 1
    z = 1 - np.abs(c[:, 0]) - np.abs(c[:, 1])
    t = np.clip(-z, 0, 1)
    x = c[:, 0] + np.where(c[:, 0] >= 0, -t, t)
    y = c[:, 1] + np.where(c[:, 1] >= 0, -t, t)
    return unit(np.stack([x, y, z], 1))


def encode_oct64(n):
    """Math.hlsli:638-644 in float64, rounded to the nearest UNORM16 code"""
    n = np.asarray(n, F64).reshape(-1, 3)
    p = n[:, :2] / np.abs(n).sum(1, keepdims=True)
    sgn = np.where(n[:, :2] >= 0, 1.0, -1.0)
    folded = (1 - np.abs(p[:, ::-1])) * sgn
    enc = np.where(n[:, 2:3] <= 0, folded, p)
    return np.rint((enc * 0.5 + 0.5) * 65535).astype(np.uint16)


def angle(a, b):
    a, b = unit(np.asarray(a, F64)), unit(np.asarray(b, F64))
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))


def round_trip_angle(n64):
    """A_q of a case: the largest angle the oct32 round trip of its float64 directions produces"""
    return float(angle(decode_oct64(encode_oct64(n64)), n64).max())


# ---------------------------------------------------------------------------------------------------------------- matrices
def trs12(t, axis, ang, s):
    """3 x 4 row-major T R(axis, ang) S in float32"""
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    M = np.zeros((3, 4))
    M[:, :3] = R * np.asarray(s, F64).reshape(1, 3)
    M[:, 3] = t
    return M.reshape(12).astype(F32)


def inverse12(M12):
    M = mat4(M12)[0]
    return np.linalg.inv(M)[:3].reshape(12).astype(F32)


def quat(axis, ang):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]]).astype(F32)


IDENTITY = F32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


# ---------------------------------------------------------------------------------------------------------------- the CPU case tables
def directions(rng, n):
    """unit directions on both hemispheres, with the fold lines (z = 0), the axes and the octant diagonals first"""
    special = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [-1, 1, 0], [1, -1, 0], [-1, -1, 0], [0.3, -0.954, 0],
               [1, 1, 1], [-1, -1, -1], [1, -1, -1], [0, 1, -1], [1, 0, -1], [1e-4, 1, -1e-4], [-0.6, 0.8, 1e-7], [-0.6, 0.8, -1e-7]]
    d = np.concatenate([np.asarray(special, F64), rng.normal(size=(n - len(special), 3))])
    return unit(d)


def joint_set(rng, nj, nonuniform):
    """nj joint matrices of a gently bent chain: rotations of at most 0.5 rad about nearby axes, scales in [0.8, 1.3] (one per axis when nonuniform),
    so that every convex blend keeps cond(M3) well below 4 and det > 0"""
    out = []
    for j in range(nj):
        s = rng.uniform(0.8, 1.3, 3) if nonuniform else np.full(3, rng.uniform(0.8, 1.3))
        out.append(trs12(rng.uniform(-1, 1, 3), [0.1 * rng.normal(), 0.1 * rng.normal(), 1.0], rng.uniform(-0.5, 0.5), s))
    return np.array(out, F32)


def influence_cases(rng, nj, n):
    """(joint (n, 4) uint16, weight (n, 4) float32): one weight of 1 with the idle slots naming joint 0 and the last joint, then two, three and four
    non-zero weights summing to 1 in float32 as the loader leaves them"""
    joint = rng.integers(0, nj, (n, 4)).astype(np.uint16)
    weight = np.zeros((n, 4), F32)
    for i in range(n):
        k = i % 5
        if k < 2:
            weight[i, 0] = 1
            joint[i, 1:] = 0 if k == 0 else nj - 1
        else:
            w = rng.uniform(0.05, 1, k).astype(F32)
            weight[i, :k] = w / w.sum(dtype=F32)
    return joint, weight


# ---------------------------------------------------------------------------------------------------------------- the GPU scene
TUBE_RINGS, TUBE_SEGS = 45, 24
TUBE_VERTS = TUBE_RINGS * TUBE_SEGS      # 1 080
TUBE_Y0, TUBE_Y1, TUBE_R = 0.25, 1.65, 0.13
TUBE_X, TUBE_Z = 0.05, -0.35


def tube(rng):
    """(vertices, indices): a closed-sided tube along +y with slightly perturbed normals and tangents on both hemispheres"""
    v = np.zeros(TUBE_VERTS, wire.VERTEX)
    ring, seg = np.divmod(np.arange(TUBE_VERTS), TUBE_SEGS)
    a = 2 * np.pi * seg / TUBE_SEGS
    y = TUBE_Y0 + (TUBE_Y1 - TUBE_Y0) * ring / (TUBE_RINGS - 1)
    n = np.stack([np.cos(a), 0.15 * np.sin(3 * a + ring), np.sin(a)], 1)
    v["pos"] = np.stack([TUBE_X + TUBE_R * np.cos(a), y, TUBE_Z + TUBE_R * np.sin(a)], 1).astype(F32)
    v["uv"] = np.stack([seg / TUBE_SEGS, ring / (TUBE_RINGS - 1)], 1).astype(F32)
    v["normal"] = zsk.encode(unit(n))
    v["tangent"] = zsk.encode(unit(np.stack([-np.sin(a), 0.1 * np.cos(ring), np.cos(a)], 1)))
    idx = []
    for r in range(TUBE_RINGS - 1):
        for s in range(TUBE_SEGS):
            p, q = r * TUBE_SEGS + s, r * TUBE_SEGS + (s + 1) % TUBE_SEGS
            idx += [p, q, p + TUBE_SEGS, q, q + TUBE_SEGS, p + TUBE_SEGS]
    return v, np.asarray(idx, np.uint32)


def skinned_cornell(extra_tubes=0):
    """tests/golden/cornell_emissive.npz + (1 + extra_tubes) tubes, each an instance of its own with an identity world matrix, as the loader lays a
    skinned node out.  Returns (scene, [first vertex of each tube])"""
    sc = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_emissive.npz"))
    rng = np.random.default_rng(23)
    firsts = []
    for k in range(1 + extra_tubes):
        v, idx = tube(rng)
        v["pos"][:, 0] += F32(0.45 * k)
        firsts.append(len(sc.vertices))
        inst = sc.instances[:1].copy()      # a wall: unit scale, no rotation, not emissive
        inst["base_vtx_offset"], inst["base_idx_offset"], inst["mat_idx"] = len(sc.vertices), len(sc.indices), 2 + k
        inst["translation"] = 0
        sc.vertices = np.concatenate([sc.vertices, v])
        sc.indices = np.concatenate([sc.indices, idx])
        sc.instances = np.concatenate([sc.instances, inst])
        sc.instance_to_world = np.concatenate([sc.instance_to_world, IDENTITY.reshape(1, 12)])
        sc.instance_mask = np.concatenate([sc.instance_mask, sc.instance_mask[:1]])
        sc.instance_num_tris = np.concatenate([sc.instance_num_tris, np.uint32([len(idx) // 3])])
    return sc, firsts


def joint_chain(nj, moving_instances=(), seed=3, x=TUBE_X):
    """an animation table of nj joints up the tube: joint 0 a static root, every other one animated -- a bend of at most 0.35 rad about z or x and a
    non-uniform scale in [0.85, 1.2] -- except the last, a static leaf on its animated parent (the closure rule).  Joint j hangs on joint j - 1 while
    the chain is shorter than ZR_ANIM_MAX_LEVELS, later ones on joint 0.  moving_instances: [(instance, rest TRS)] animated as instances of their own.
    Returns (AnimDesc, joints (SKIN_JOINT) with the inverse bind matrices of the rest pose)"""
    rng = np.random.default_rng(seed)
    nodes, keys, worlds = [], [], []
    for j in range(nj):
        n = np.zeros((), wire.ANIM_NODE)
        parent = wire.ANIM_ROOT if j == 0 else (j - 1 if j < 24 else 0)
        yj = TUBE_Y0 + (TUBE_Y1 - TUBE_Y0) * j / max(nj, 1)
        yp = 0.0 if j == 0 else TUBE_Y0 + (TUBE_Y1 - TUBE_Y0) * parent / max(nj, 1)
        rest_t = F32([x if j == 0 else 0.0, yj - yp, TUBE_Z if j == 0 else 0.0])
        n["parent"], n["parent_world"] = parent, IDENTITY
        n["rest_scale"], n["rest_rotation"], n["rest_translation"] = 1, (0, 0, 0, 1), rest_t
        if nj == 1 or (0 < j and (j < nj - 1 or nj == 2)):
            n["first_key"], n["num_keys"], n["loop"], n["t0"] = len(keys), 3, j % 2, 0.0
            for tm in (0.0, 0.5, 1.25):
                key = np.zeros((), wire.KEYFRAME)
                key["scale"] = rng.uniform(0.85, 1.2, 3)
                key["rotation"] = quat([1, 0, 0] if j % 2 else [0, 0, 1], rng.uniform(-0.35, 0.35) / max(1.0, nj / 8))
                key["translation"] = rest_t + rng.uniform(-0.02, 0.02, 3).astype(F32)
                key["time"] = tm
                keys.append(key)
        nodes.append(n)
    inst_idx, inst_node = [], []
    for i, (s, q, t) in moving_instances:
        n = np.zeros((), wire.ANIM_NODE)
        n["parent"], n["parent_world"], n["rest_scale"], n["rest_rotation"], n["rest_translation"] = wire.ANIM_ROOT, IDENTITY, s, q, t
        n["first_key"], n["num_keys"], n["loop"] = len(keys), 2, 1
        for tm, dy in ((0.0, 0.0), (1.0, 0.25)):
            key = np.zeros((), wire.KEYFRAME)
            key["scale"], key["rotation"], key["translation"], key["time"] = s, q, np.asarray(t, F32) + F32([0, dy, 0]), tm
            keys.append(key)
        inst_idx.append(i); inst_node.append(len(nodes))
        nodes.append(n)
    anim = wire.AnimDesc(np.array(nodes, wire.ANIM_NODE), np.array(keys, wire.KEYFRAME) if keys else np.zeros(0, wire.KEYFRAME), inst_idx, inst_node)
    rest_world = node_worlds(anim, -1.0)      # before every first key: the first keys' poses are the bind pose
    joints = np.zeros(nj, wire.SKIN_JOINT)
    joints["node"] = np.arange(nj)
    for j in range(nj):
        joints["inverse_bind"][j] = inverse12(rest_world[j])
    return anim, joints


def concat(a, ja, b, jb):
    """two joint chains in one table: (AnimDesc, joints) of `a` followed by `b`, b's node, key and joint-node indices shifted"""
    nb = b.nodes.copy()
    nb["parent"] = np.where(nb["parent"] == wire.ANIM_ROOT, wire.ANIM_ROOT, nb["parent"] + len(a.nodes))
    nb["first_key"] = np.where(nb["num_keys"] > 0, nb["first_key"] + len(a.keys), 0)
    jb = jb.copy()
    jb["node"] += len(a.nodes)
    anim = wire.AnimDesc(np.concatenate([a.nodes, nb]), np.concatenate([a.keys, b.keys]), np.concatenate([a.instance_idx, b.instance_idx]),
                         np.concatenate([a.instance_node, b.instance_node + len(a.nodes)]))
    return anim, np.concatenate([ja, jb])


def node_worlds(anim, t):
    d = anim.c_desc()
    out = np.zeros((len(anim.nodes), 12), F32)
    import ctypes as C
    zan.lib().zan_eval_node_worlds(C.addressof(d), float(t), out.ctypes.data)
    return out


def tube_influences(verts, nj, rng):
    """four influences per vertex by height: the joints around the vertex's ring, weights renormalised in float32; every fifth vertex has one weight of 1
    and idle slots naming joint 0 or the last joint"""
    f = np.zeros(len(verts), wire.SKIN_INFLUENCE)
    h = (verts["pos"][:, 1].astype(F64) - TUBE_Y0) / (TUBE_Y1 - TUBE_Y0) * nj
    for i in range(len(verts)):
        j0 = int(np.clip(np.floor(h[i]), 0, nj - 1))
        js = [j0, min(j0 + 1, nj - 1), max(j0 - 1, 0), min(j0 + 2, nj - 1)]
        if i % 5 == 0:
            f["joint"][i], f["weight"][i] = [j0, 0 if i % 2 else nj - 1, 0, nj - 1], [1, 0, 0, 0]
            continue
        fr = h[i] - np.floor(h[i])
        w = F32([1 - fr, fr, 0.15 * rng.random() * (i % 3 > 0), 0.1 * rng.random() * (i % 3 > 1)])
        f["joint"][i], f["weight"][i] = js, w / w.sum(dtype=F32)
    return f


def host_posed(anim, skin, rest, t):
    """the host form's vertices for time t: zr_anim.h's node matrices, then zr_skin.h on the rest records (range after range), both compiled for the host"""
    J = zsk.eval_joint_matrices(skin, node_worlds(anim, t))
    return zsk.skin_ranges(skin, J, rest)


def rest_of_ranges(skin, vertices):
    return np.concatenate([vertices[int(r["first_vertex"]):int(r["first_vertex"]) + int(r["num_vertices"])] for r in skin.ranges]) if len(skin.ranges) else vertices[:0]


def apply_host_form(scene, host, anim, skin, rest, t, stream=False):
    """the host sequence the device form is held to: zrh_scene_data_animate(t), zr_scene_update_vertices with the vertices zr_skin.h computes on the host,
    then the host-form emissive and instance updates"""
    posed = host_posed(anim, skin, rest, t)
    k = 0
    for r in skin.ranges:
        n = int(r["num_vertices"])
        if n:
            scene.update_vertices(int(r["first_vertex"]), posed[k:k + n], stream=stream)
        k += n
    host.apply(scene, t, stream=stream)
    return posed


# ---------------------------------------------------------------------------------------------------------------- the loader's fixture
SKIN_GLTF = os.path.join(ROOT, "tests", "golden", "skin_gltf")


def skinned_gltf(tmp_path, edit=None, name="cornell_skinned", blob_edit=None):
    """tests/golden/skin_gltf/cornell_skinned.gltf (tools/make_skin_gltf.py) laid out next to the animated Cornell fixture's files, as it references
    them; edit(gltf dict) changes the JSON first, blob_edit(bytearray) the tube's buffer"""
    import json
    from tests.animmath import cases as acases
    acases.cornell_animated(tmp_path)
    blob = bytearray(open(os.path.join(SKIN_GLTF, "skin_tube.bin"), "rb").read())
    if blob_edit is not None:
        blob = blob_edit(blob) or blob
    (tmp_path / "skin_tube.bin").write_bytes(bytes(blob))
    g = json.load(open(os.path.join(SKIN_GLTF, "cornell_skinned.gltf")))
    if edit is not None:
        edit(g)
    p = tmp_path / (name + ".gltf")
    p.write_text(json.dumps(g))
    return str(p)
