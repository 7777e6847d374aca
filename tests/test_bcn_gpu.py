"""The BC7 / BC5 decode on the GPU (zr_tu_texdecode.hip) against include/zr_bcn.h on the host (tests/bcnmath/libzbc.so) and the block fixture
(tests/golden/bcn_blocks.npz, texels of the host loader before the header existed), byte for byte: on caller buffers (zr_bcn_decode_device) and
through the scene path (zr_scene_create_compressed).  Expected bytes never come from the kernel."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.bcnmath import zbc
from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST_LIB = os.path.join(ROOT, "zetaray_amd", "libzetaray_amd_fast.so")
REF_GLTF = os.path.join(ROOT, "tests", "golden", "cornell_gltf")
FILL = 0xA5
ENC = {"bc7": zbc.BC7, "bc5": zbc.BC5}


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


@pytest.fixture(scope="module")
def fixture_blocks():
    z = np.load(os.path.join(ROOT, "tests", "golden", "bcn_blocks.npz"))
    return {k: np.ascontiguousarray(z[k]) for k in z.files}


def _descs(rows):
    """rows of (offset, w, h, mips, fmt) -> wire.TEXTURE_DESC"""
    d = np.zeros(len(rows), wire.TEXTURE_DESC)
    for i, (off, w, h, mips, fmt) in enumerate(rows):
        d["offset"][i], d["width"][i], d["height"][i], d["num_mips"][i], d["format"][i] = off, w, h, mips, fmt
    return d


def _sources(rows):
    s = np.zeros(len(rows), wire.TEXTURE_SOURCE)
    for i, (off, enc) in enumerate(rows):
        s["offset"][i], s["encoding"][i] = off, enc
    return s


def _chain(w, h, mips):
    return [(max(1, w >> m), max(1, h >> m)) for m in range(mips)]


def _full(w, h):
    return int(np.log2(max(w, h))) + 1


def _random_chain(rng, enc, w, h, mips):
    """(the blocks of the chain, the texels the header decodes them to, mip by mip)"""
    blocks, texels = [], []
    for mw, mh in _chain(w, h, mips):
        b = rng.integers(0, 256, (zbc.mip_blocks(mw, mh), 16), dtype=np.uint8)
        if enc == zbc.BC7:
            b[::7, 0] = 0       # reserved-mode blocks among them
        blocks.append(b.reshape(-1))
        texels.append(zbc.decode_mip(enc, b, mw, mh).reshape(-1))
    return np.concatenate(blocks), texels


# ---- 1. the fixture's blocks
@pytest.mark.parametrize("enc", ["bc7", "bc5"])
def test_decode_device_equals_the_fixture(api, fixture_blocks, enc):
    blocks, want = fixture_blocks[enc], fixture_blocks[enc + "_texels"]
    n, ch = len(blocks), want.shape[2]
    # the n blocks as one block row: a 4 n x 4 mip
    got = api.bcn_decode_device(_descs([(0, 4 * n, 4, 1, wire.TEX_RGBA8 if enc == "bc7" else wire.TEX_RG8)]), _sources([(0, ENC[enc])]), blocks.reshape(-1), 16 * n * ch)
    got = got.reshape(4, n, 4, ch).transpose(1, 0, 2, 3).reshape(n, 16, ch)
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert len(bad) == 0, (len(bad), bad[:8])


# ---- 2. single mips: partial blocks on either edge, a block row of 65 that crosses a wave, degenerate rows
SHAPES = [(1, 1), (2, 2), (3, 5), (4, 4), (5, 3), (7, 9), (64, 1), (1, 64), (258, 6)]


@pytest.mark.parametrize("enc", ["bc7", "bc5"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_single_mips(api, enc, shape):
    w, h = shape
    rng = np.random.default_rng(w * 1000 + h)
    blocks, (want,) = _random_chain(rng, ENC[enc], w, h, 1)
    fmt = wire.TEX_RGBA8 if enc == "bc7" else wire.TEX_RG8
    for off in (0, 16, 4):      # rows 16-byte aligned where the width allows, and offset by 4
        got = api.bcn_decode_device(_descs([(off, w, h, 1, fmt)]), _sources([(0, ENC[enc])]), blocks, off + len(want) + 32, fill=FILL)
        assert np.array_equal(got[off:off + len(want)], want), (off, int((got[off:off + len(want)] != want).sum()))
        assert (got[:off] == FILL).all() and (got[off + len(want):] == FILL).all()


def test_two_byte_aligned_destination(api):
    """258 x 6 again where its rows start on a byte that is 2 mod 4.  Only RG8 can: heap offsets are multiples of 4 and every RGBA8 mip is a multiple of
    4 bytes, but an RG8 mip of odd area is not -- 517 x 13 RG8 is 13 442 bytes, so its mip 1 (258 x 6) starts there.  BC7 gets the least alignment it can
    have, 4 (offset 4 in test_single_mips, and the odd widths there)"""
    rng = np.random.default_rng(258)
    blocks, want = _random_chain(rng, zbc.BC5, 517, 13, 2)
    assert len(want[0]) % 4 == 2
    total = len(want[0]) + len(want[1])
    got = api.bcn_decode_device(_descs([(4, 517, 13, 2, wire.TEX_RG8)]), _sources([(0, zbc.BC5)]), blocks, 4 + total + 30, fill=FILL)
    assert np.array_equal(got[4:4 + total], np.concatenate(want))
    assert (got[:4] == FILL).all() and (got[4 + total:] == FILL).all()


# ---- 3. five textures of mixed encodings in one call
def test_mixed_textures_in_one_call(api):
    rng = np.random.default_rng(3)
    spec = [(zbc.RAW, wire.TEX_RGBA8, 8, 8, 4), (zbc.BC7, wire.TEX_RGBA8, 37, 21, _full(37, 21)), (zbc.BC5, wire.TEX_RG8, 64, 64, _full(64, 64)),
            (zbc.BC5, wire.TEX_RG8, 1, 1, 1), (zbc.BC7, wire.TEX_RGBA8_SRGB, 16, 16, 3)]
    payload, descs, sources, want = [np.full(32, 0x11, np.uint8)], [], [], []      # (padding first: no chain starts at 0)
    heap = 12
    for enc, fmt, w, h, mips in spec:
        at = sum(len(p) for p in payload)
        if enc == zbc.RAW:
            texels = [rng.integers(0, 256, mw * mh * 4, dtype=np.uint8) for mw, mh in _chain(w, h, mips)]
            chain = np.concatenate(texels)
        else:
            chain, texels = _random_chain(rng, enc, w, h, mips)
        sources.append((at, enc))
        payload += [chain, np.full(-len(chain) % 16 + 16 * int(rng.integers(0, 3)), 0x22, np.uint8)]
        heap = (heap + 3) // 4 * 4
        descs.append((heap, w, h, mips, fmt))
        for t in texels:
            want.append((heap, t))
            heap += len(t)
        heap += int(rng.integers(1, 40))
    payload = np.concatenate(payload)
    got = api.bcn_decode_device(_descs(descs), _sources(sources), payload, heap + 64, fill=FILL)
    untouched = np.ones(len(got), bool)
    for k, (off, t) in enumerate(want):
        assert np.array_equal(got[off:off + len(t)], t), ("mip", k, off, len(t))
        untouched[off:off + len(t)] = False
    assert (got[untouched] == FILL).all(), np.nonzero(untouched & (got != FILL))[0][:8]
    assert untouched.sum() > 64


# ---- 4. the scene path
def _cornell_gltf(tmp_path, name):
    for f in (name + ".gltf", "cornell.bin"):
        shutil.copy(os.path.join(REF_GLTF, f), tmp_path / f)
    (tmp_path / "compressed").mkdir()
    with gzip.open(os.path.join(REF_GLTF, "compressed", "checkerboard.dds.gz"), "rb") as src:
        (tmp_path / "compressed" / "checkerboard.dds").write_bytes(src.read())
    return str(tmp_path / (name + ".gltf"))


def test_scene_path_on_the_cornell_gltf(api, tmp_path):
    path = _cornell_gltf(tmp_path, "cornell_emissive")
    dec, offs = scene_io.load_gltf_native(path)
    cmp_, offs2 = scene_io.load_gltf_native(path, textures="compressed")
    assert offs == offs2 and len(cmp_.texture_payload) and len(cmp_.texels) == 0 and len(dec.texels)
    w, h = 96, 54
    prm = wire.default_params()
    ra = api.Renderer(dec, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    rb = api.Renderer(cmp_, w, h, params=prm, integrator=api.INTEGRATOR_RESTIR_PT)
    heap = rb.scene.get_texels()
    assert len(heap) == len(dec.texels) and np.array_equal(heap, dec.texels)
    assert np.array_equal(ra.scene.get_texels(), dec.texels)
    assert np.array_equal(rb.scene.get_texels(first=1000, count=77), dec.texels[1000:1077])
    for f in (1, 2):
        cb = scene_io.make_frame_constants(w, h, frame_num=f, num_emissives=len(dec.emissives))
        scene_io.set_texture_heap_offsets(cb, offs)
        for r in (ra, rb):
            r.render_frame(cb)
        ga, gb = ra.gbuffer.download()[0], rb.gbuffer.download()[0]
        for k, (pa, pb) in enumerate(zip(ga, gb)):
            assert np.array_equal(np.asarray(pa).view(np.uint8), np.asarray(pb).view(np.uint8)), ("G-buffer plane", k, "frame", f)
        assert np.array_equal(ra.final().view(np.uint32), rb.final().view(np.uint32)), ("FINAL", f)
        ca, cb_ = ra.p_indirect.read_counters(), rb.p_indirect.read_counters()
        assert ca == cb_ and ca[0] > 0, (ca, cb_)


def _untextured(path):
    """the glTF at `path` without its images: <name>_plain.gltf beside it"""
    g = json.load(open(path))
    for k in ("images", "textures", "samplers"):
        g.pop(k, None)
    for m in g.get("materials", []):
        for k in ("normalTexture", "emissiveTexture", "occlusionTexture"):
            m.pop(k, None)
        for k in ("baseColorTexture", "metallicRoughnessTexture"):
            m.get("pbrMetallicRoughness", {}).pop(k, None)
    out = path[:-5] + "_plain.gltf"
    json.dump(g, open(out, "w"))
    return out


def test_cpp_mirror_creates_the_scene_either_way(api, tmp_path):
    """zrh_scene_create_from_gltf_ex (libzetaray_host.so) with and without ZRH_LOAD_KEEP_COMPRESSED: the same heap on the device, the same table
    offsets; and a glTF without textures, which has no blocks in either mode and must still become a scene"""
    import ctypes as C
    H = C.CDLL(os.path.join(ROOT, "zetaray_amd", "libzetaray_host.so"))
    H.zrh_scene_create_from_gltf_ex.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L = api.lib()
    path = _cornell_gltf(tmp_path, "cornell_emissive")
    dec, offs = scene_io.load_gltf_native(path)
    rho, rho_dim = scene_io.load_rho_default()
    rho = np.ascontiguousarray(rho, np.uint16)
    dims = (C.c_uint32 * 3)(*rho_dim)

    def create(p, flags):
        h, o = C.c_void_p(), (C.c_uint32 * 4)()
        assert H.zrh_scene_create_from_gltf_ex(0, os.fsencode(p), rho.ctypes.data, dims, flags, C.byref(h), o) == 0, (p, flags, L.zr_last_error())
        return h, list(o)

    for flags in (0, scene_io.LOAD_KEEP_COMPRESSED):
        h, o = create(path, flags)
        assert o == [offs["base_color"], offs["normal"], offs["metallic_roughness"], offs["emissive"]]
        heap = np.zeros(len(dec.texels), np.uint8)
        api._check(L.zr_scene_get_texels(h, None, heap.ctypes.data, 0, len(heap)))
        assert np.array_equal(heap, dec.texels), flags
        assert L.zr_scene_get_texels(h, None, heap.ctypes.data, 1, len(heap)) == 1      # one byte past the heap: ZR_ERR_INVALID_ARG
        L.zr_scene_destroy(h)
    plain = _untextured(path)
    assert len(scene_io.load_gltf_native(plain)[0].textures) == 0
    for flags in (0, scene_io.LOAD_KEEP_COMPRESSED):
        h, _ = create(plain, flags)
        assert L.zr_scene_get_texels(h, None, None, 0, 0) == 0 and L.zr_scene_get_texels(h, None, None, 0, 1) == 1
        L.zr_scene_destroy(h)


# ---- 5. refusals
def _textured_box(rng):
    """the untextured Cornell box with three maps in its heap: a BC7 sRGB 8 x 8 base colour map with its full chain, a BC5 8 x 4 map and a RAW RGBA8 2 x 2 one"""
    sc = scene_io.load_npz(os.path.join(ROOT, "tests", "golden", "cornell.npz"))
    for enc, fmt, w, h in ((zbc.BC7, wire.TEX_RGBA8_SRGB, 8, 8), (zbc.BC5, wire.TEX_RG8, 8, 4)):
        sc.add_texture_blocks(_random_chain(rng, enc, w, h, _full(w, h))[0], w, h, _full(w, h), fmt, enc)
    sc.add_texture_blocks(rng.integers(0, 256, 2 * 2 * 4 + 4, dtype=np.uint8), 2, 2, 2, wire.TEX_RGBA8, zbc.RAW)
    return sc


def test_refusals_leave_nothing_behind(api):
    import ctypes as C
    rng = np.random.default_rng(5)
    sc = _textured_box(rng)
    L = api.lib()
    SENTINEL = 0x5A5A5A5A

    def create(desc, blocks):
        h = C.c_void_p(SENTINEL)
        code = L.zr_scene_create_compressed(0, C.addressof(desc) if desc is not None else None, C.addressof(blocks) if blocks is not None else None, C.byref(h))
        if code == 0:
            L.zr_scene_destroy(h)
        else:
            assert h.value == SENTINEL, "*out was written"
        return code

    def variant(edit):
        """the scene's desc and blocks after `edit(descs, sources, desc, blocks)` changed copies of them"""
        descs, sources = sc.textures.copy(), sc.texture_sources.copy()
        desc, blocks = sc.desc(), sc.texture_blocks()
        desc.texels, desc.texel_bytes = None, sc.texel_heap_bytes
        desc.textures, blocks.sources = descs.ctypes.data, sources.ctypes.data
        keep = edit(descs, sources, desc, blocks)
        return create(desc, blocks), keep

    INVALID = 1      # ZR_ERR_INVALID_ARG
    assert variant(lambda d, s, desc, b: None)[0] == 0, L.zr_last_error()
    assert create(sc.desc(), None) == INVALID
    some = np.zeros(4, np.uint8)
    edits = {
        "null sources": lambda d, s, desc, b: setattr(b, "sources", None),
        "null payload": lambda d, s, desc, b: setattr(b, "payload", None),
        "texels given": lambda d, s, desc, b: setattr(desc, "texels", some.ctypes.data),
        "unknown encoding": lambda d, s, desc, b: s["encoding"].__setitem__(0, 3),
        "BC7 on RG8": lambda d, s, desc, b: s["encoding"].__setitem__(1, zbc.BC7),
        "BC5 on RGBA8": lambda d, s, desc, b: s["encoding"].__setitem__(0, zbc.BC5),
        "BC5 on RGBA8 (raw texture)": lambda d, s, desc, b: s["encoding"].__setitem__(2, zbc.BC5),
        "BCn offset not a multiple of 16": lambda d, s, desc, b: s["offset"].__setitem__(1, int(s["offset"][1]) + 8),
        "RAW offset not a multiple of 4": lambda d, s, desc, b: s["offset"].__setitem__(2, int(s["offset"][2]) + 2),
        "chain beyond the payload": lambda d, s, desc, b: setattr(b, "payload_bytes", int(s["offset"][2]) + 19),
        "chain starts beyond the payload": lambda d, s, desc, b: s["offset"].__setitem__(0, 1 << 40),
        "desc: no mips": lambda d, s, desc, b: d["num_mips"].__setitem__(0, 0),
        "desc: zero width": lambda d, s, desc, b: d["width"].__setitem__(1, 0),
        "desc: unknown format": lambda d, s, desc, b: d["format"].__setitem__(0, 3),
        "desc: offset not a multiple of 4": lambda d, s, desc, b: d["offset"].__setitem__(1, int(d["offset"][1]) + 2),
        "desc: outside the heap": lambda d, s, desc, b: setattr(desc, "texel_bytes", sc.texel_heap_bytes - 1),
    }
    for name, edit in edits.items():
        assert variant(edit)[0] == INVALID, name

    # more than 2^32 - 1 blocks: nothing is read before the count is refused, so the payload can be a stub.  16 textures of 65535^2 are 2^32 blocks
    n = 16
    descs = _descs([(0, 65535, 65535, 1, wire.TEX_RGBA8)] * n)
    sources = _sources([(0, zbc.BC7)] * n)
    desc, blocks = sc.desc(), sc.texture_blocks()
    desc.texels, desc.texel_bytes, desc.textures, desc.num_textures = None, 1 << 62, descs.ctypes.data, n
    blocks.sources, blocks.payload_bytes = sources.ctypes.data, 1 << 62
    assert 16 * zbc.mip_blocks(65535, 65535) > 0xFFFFFFFF >= 15 * zbc.mip_blocks(65535, 65535)
    assert create(desc, blocks) == INVALID and b"2^32" in L.zr_last_error()

    # the stand-alone entry point refuses the same, and zr_scene_create with texels still works
    with pytest.raises(api.ZetaRayError):
        api.bcn_decode_device(_descs([(0, 4, 4, 1, wire.TEX_RG8)]), _sources([(0, zbc.BC7)]), np.zeros(16, np.uint8), 64)
    dec = _textured_box(np.random.default_rng(5))
    dec.decode_textures()
    dec.texture_payload = np.zeros(0, np.uint8)
    s = api.Scene(dec)
    assert np.array_equal(s.get_texels(), dec.texels)
    s2 = api.Scene(sc)
    assert np.array_equal(s2.get_texels(), dec.texels)


# ---- 6. the tolerance-mode library decodes the same bytes
def test_fast_library_decodes_the_same_bytes():
    assert os.path.exists(FAST_LIB), "libzetaray_amd_fast.so is missing: __graft_entry__.build() builds it"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bcnmath", "fast_check.py")], env=dict(os.environ, ZETARAY_AMD_LIB=FAST_LIB),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep == {"lib": "libzetaray_amd_fast.so", "bc7_bad": 0, "bc5_bad": 0, "bc7": 2112, "bc5": 1040}
