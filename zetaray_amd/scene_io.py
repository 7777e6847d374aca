"""Scene ingestion: glTF -> wire-format arrays (caller side of the hot path).

Restates, for the feature subset the Cornell assets use (float3/float2/float4 accessors, u16/u32 indices, TRS
nodes, KHR_materials_emissive_strength / ior / transmission / clearcoat):
  Source/ZetaCore/Model/glTF.cpp:143-268   (attribute processing: RHS->LHS flip, CW winding)
  Source/ZetaCore/Model/glTF.cpp:523-643   (ProcessMaterials)
  Source/ZetaCore/Model/glTF.cpp:692-767   (ProcessEmissiveSubtree)
  Source/ZetaCore/Model/glTF.cpp:769-940   (ProcessNodeSubtree: TRS -> LHS)
  Source/ZetaCore/RayTracing/RtAccelerationStructure.cpp:318-380 (FillMeshInstanceData: quantised TRS)
  Source/ZetaCore/Scene/SceneCore.cpp:25-36,196-236 (emissive world transform + PCG3d ID)
  Source/ZetaCore/Core/Material.h:66-260   (Material packing)
This is host plumbing in Python (numpy); it produces the buffers handed to zr_scene_create and to the oracle, so it is
not part of the oracle<->HIP parity.  Texture images are not decoded (BC7) -- materials keep their factors only.
"""
import json
import os
import struct

import numpy as np

from . import wire

_COMP = {5120: "i1", 5121: "u1", 5122: "<i2", 5123: "<u2", 5125: "<u4", 5126: "<f4"}
_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def f32_to_f16_bits(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def pcg3d(x, y, z):
    """RNG::PCG3d, Source/ZetaRenderPass/Common/Sampling.hlsli:22-33."""
    M = 0xFFFFFFFF
    x = (x * 1664525 + 1013904223) & M
    y = (y * 1664525 + 1013904223) & M
    z = (z * 1664525 + 1013904223) & M
    x = (x + y * z) & M
    y = (y + z * x) & M
    z = (z + x * y) & M
    x ^= x >> 16
    y ^= y >> 16
    z ^= z >> 16
    x = (x + y * z) & M
    y = (y + z * x) & M
    z = (z + x * y) & M
    return x, y, z


def encode_octahedral(n, sse_order=True):
    """Math::encode_octahedral + unorm2::FromNormalized (VectorFuncs.h:134-153, Vector.h:626-647) in the SSE code's operation order: the
    L1 norm is (|x| + |z|) + |y| (hadd_float3), the fold's sign is taken from the input component (v >= 0), round to nearest even.
    sse_order=False: the plain left-to-right statement ((|x| + |y|) + |z|, sign of the projected component) that the procedural test scenes
    were generated with -- any valid encoding does for those, and keeping it keeps their committed goldens valid."""
    n = np.asarray(n, dtype=np.float32).reshape(-1, 3)
    if sse_order:
        denom = (np.abs(n[:, 0]) + np.abs(n[:, 2])) + np.abs(n[:, 1])
    else:
        denom = np.abs(n[:, 0]) + np.abs(n[:, 1]) + np.abs(n[:, 2])
    p = n[:, :2] / denom[:, None]
    sgn = (np.where(n[:, :2] >= 0, np.float32(1), np.float32(-1)) if sse_order else np.where(np.signbit(p), np.float32(-1), np.float32(1))).astype(np.float32)
    folded = (np.float32(1) - np.abs(p[:, ::-1])) * sgn
    enc = np.where((n[:, 2] <= 0)[:, None], folded, p).astype(np.float32)
    u = (enc * np.float32(0.5) + np.float32(0.5)) * np.float32(65535.0)
    return np.rint(u).astype(np.uint16)


def unorm8(f):
    f = np.clip(np.float32(f), 0, 1)
    return int(np.float32(f) * np.float32(255.0) + np.float32(0.5))


def rgb8(c):
    return unorm8(c[0]) | (unorm8(c[1]) << 8) | (unorm8(c[2]) << 16)


def pack_material(base_color=(1, 1, 1, 1), metallic=0.0, roughness=1.0, ior=1.5, transmission=0.0, subsurface=0.0,
                  coat_weight=0.0, coat_color=(0.8, 0.8, 0.8), coat_roughness=0.0, coat_ior=1.6,
                  emissive_factor=(0, 0, 0), emissive_strength=1.0, normal_scale=1.0, alpha_cutoff=0.5,
                  alpha_mode=0, double_sided=False, thin_walled=False, transmission_depth=0.0,
                  base_color_tex=0xFFFF, normal_tex=0xFFFF, mr_tex=0xFFFF, emissive_tex=0xFFFF):
    """Material packing, Source/ZetaCore/Core/Material.h:66-260 (setter semantics)."""
    m = np.zeros((), dtype=wire.MATERIAL)
    m["base_color_factor"] = rgb8(base_color) | (unorm8(base_color[3]) << 24)
    m["base_color_tex_subsurf_coat_weight"] = base_color_tex | (unorm8(subsurface) << 16) | (unorm8(coat_weight) << 24)
    m["normal_tex_tr_depth"] = normal_tex | (int(f32_to_f16_bits(transmission_depth)) << 16)
    m["mr_tex_spec_roughness_coat_roughness"] = mr_tex | (unorm8(roughness) << 16) | (unorm8(coat_roughness) << 24)
    m["emissive_factor_normal_scale"] = rgb8(emissive_factor) | (unorm8(normal_scale) << 24)
    ior_n = (np.float32(ior) - np.float32(1.0)) / np.float32(1.5)
    ior16 = int(np.clip(ior_n, 0, 1) * np.float32(65535.0) + np.float32(0.5))
    m["emissive_strength_ior"] = int(f32_to_f16_bits(emissive_strength)) | (ior16 << 16)
    cior_n = (np.float32(coat_ior) - np.float32(1.0)) / np.float32(1.5)
    m["emissive_tex_alpha_cutoff_coat_ior"] = emissive_tex | (unorm8(alpha_cutoff) << 16) | (unorm8(cior_n) << 24)
    flags = rgb8(coat_color)
    if metallic >= 0.9:
        flags |= 1 << 24
    if double_sided:
        flags |= 1 << 25
    if transmission >= 0.9:
        flags |= 1 << 26
    flags |= (alpha_mode & 3) << 27
    if thin_walled:
        flags |= 1 << 29
    m["coat_color_flags"] = flags
    return m


def quat_rotate(q, v):
    """Math::RotateVector (Math.hlsli:556-565), float32."""
    q = np.asarray(q, np.float32)
    v = np.asarray(v, np.float32)
    im = q[:3]
    t = np.cross(np.float32(2) * im, v).astype(np.float32)
    return (v + q[3] * t + np.cross(im, t)).astype(np.float32)


def trs_matrix(t, q, s):
    """float32 3x4 row-major object-to-world matrix for p' = R(S p) + T."""
    cols = [quat_rotate(q, np.array(e, np.float32) * np.float32(s[i])) for i, e in
            enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1)))]
    M = np.zeros((3, 4), np.float32)
    for i in range(3):
        M[:, i] = cols[i]
    M[:, 3] = np.asarray(t, np.float32)
    return M


class Scene:
    """Wire-format scene + the ctypes desc that points into it."""

    def __init__(self):
        self.vertices = np.zeros(0, wire.VERTEX)
        self.indices = np.zeros(0, np.uint32)
        self.instances = np.zeros(0, wire.MESH_INSTANCE)
        self.instance_to_world = np.zeros((0, 12), np.float32)
        self.instance_mask = np.zeros(0, np.uint8)
        self.instance_num_tris = np.zeros(0, np.uint32)
        self.materials = np.zeros(0, wire.MATERIAL)
        self.emissives = np.zeros(0, wire.EMISSIVE_TRI)
        self.rho = None
        self.rho_dim = (0, 0, 0)
        self.textures = np.zeros(0, wire.TEXTURE_DESC)     # material texture heap (include/zr_wire.h zr_texture_desc)
        self.texels = np.zeros(0, np.uint8)
        # block-compressed sources (add_texture_blocks, load_gltf_native(textures="compressed")): texture_sources[i] names the chain of textures[i] in
        # texture_payload, texel_heap_bytes is the size of the heap the chains decode to.  api.Scene hands them to zr_scene_create_compressed, which
        # decodes on the device; decode_textures() fills `texels` on the host for the oracle and the host executor
        self.texture_sources = np.zeros(0, wire.TEXTURE_SOURCE)
        self.texture_payload = np.zeros(0, np.uint8)
        self.texel_heap_bytes = 0
        self._desc = None

    @staticmethod
    def _chain_layout(width, height, num_mips, fmt, encoding, record_bytes=0):
        """(w, h, source bytes, texel bytes) of each mip of a chain; a TEX_SRC_RAW_MIP0 source holds level 0 alone, and so does a TEX_SRC_JPEG_COEF source,
        as a record of record_bytes bytes"""
        bpp = 2 if fmt == wire.TEX_RG8 else 4
        out = []
        for m in range(num_mips):
            w, h = max(1, width >> m), max(1, height >> m)
            if encoding == wire.TEX_SRC_JPEG_COEF:
                nsrc = record_bytes if m == 0 else 0
            elif encoding == wire.TEX_SRC_RAW_MIP0:
                nsrc = w * h * bpp if m == 0 else 0
            else:
                nsrc = w * h * bpp if encoding == wire.TEX_SRC_RAW else ((w + 3) // 4) * ((h + 3) // 4) * 16
            out.append((w, h, nsrc, w * h * bpp))
        return out

    def add_texture_blocks(self, blocks, width, height, num_mips, fmt, encoding):
        """Appends one texture from its stored chain -- BC7 / BC5 blocks (wire.TEX_SRC_BC7 needs an RGBA8 format, TEX_SRC_BC5 RG8), or uncompressed texels
        (TEX_SRC_RAW) -- mips back to back in DDS order, mip m of max(1, w >> m) x max(1, h >> m) texels -- or from its uncompressed level 0 alone
        (TEX_SRC_RAW_MIP0: levels 1 .. num_mips - 1 are generated, include/zr_mipgen.h), or from the coefficient record of a JPEG image (TEX_SRC_JPEG_COEF,
        pack_jpeg: level 0 is decoded by include/zr_jpeg.h, the other levels generated; an RGBA record needs an RGBA8 format, an RG record RG8).  Nothing is
        decoded.  Returns its heap index."""
        blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1)
        if len(self.textures) != len(self.texture_sources):
            raise ValueError("the scene already holds decoded textures: a heap is either all sources or all texels")
        if encoding not in (wire.TEX_SRC_RAW, wire.TEX_SRC_BC7, wire.TEX_SRC_BC5, wire.TEX_SRC_RAW_MIP0, wire.TEX_SRC_JPEG_COEF) or (encoding == wire.TEX_SRC_BC7 and fmt == wire.TEX_RG8) or \
                (encoding == wire.TEX_SRC_BC5 and fmt != wire.TEX_RG8):
            raise ValueError("encoding %r does not decode to format %r" % (encoding, fmt))
        layout = self._chain_layout(width, height, num_mips, fmt, encoding, len(blocks))
        if num_mips < 1 or len(blocks) != sum(l[2] for l in layout):
            raise ValueError("a %d x %d chain of %d mips is %d bytes, not %d" % (width, height, num_mips, sum(l[2] for l in layout), len(blocks)))
        src = np.zeros(1, wire.TEXTURE_SOURCE)
        src["offset"], src["encoding"] = (len(self.texture_payload) + 15) // 16 * 16, encoding
        self.texture_payload = np.concatenate([self.texture_payload, np.zeros(int(src["offset"][0]) - len(self.texture_payload), np.uint8), blocks])
        d = np.zeros(1, wire.TEXTURE_DESC)
        off = (self.texel_heap_bytes + 3) // 4 * 4
        d["offset"], d["width"], d["height"], d["num_mips"], d["format"] = off, width, height, num_mips, fmt
        self.texel_heap_bytes = off + sum(l[3] for l in layout)
        self.textures = np.concatenate([self.textures, d])
        self.texture_sources = np.concatenate([self.texture_sources, src])
        return len(self.textures) - 1

    def decode_textures(self):
        """Fills `texels` from the sources on the host, with the loader's decoder (zrh_bc7_decode / zrh_bc5_decode) and, for TEX_SRC_RAW_MIP0 sources, its
        mip generation (zrh_mip_generate); TEX_SRC_JPEG_COEF records are expanded by include/zr_jpeg.h (zrh_jpeg_expand) and their chains generated
        likewise: the heap zr_scene_create_compressed produces on the device.  The sources stay."""
        import ctypes as C
        L = _sceneio_lib()
        for f in (L.zrh_bc7_decode, L.zrh_bc5_decode):
            f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        self.texture_payload = np.ascontiguousarray(self.texture_payload, np.uint8)
        heap = np.zeros(self.texel_heap_bytes, np.uint8)
        for t, s in zip(self.textures, self.texture_sources):
            enc, at, to = int(s["encoding"]), int(s["offset"]), int(t["offset"])
            if enc == wire.TEX_SRC_JPEG_COEF:
                px = jpeg_expand(self.texture_payload[at:])
                if px.shape[:2] != (int(t["height"]), int(t["width"])) or px.shape[2] != (2 if int(t["format"]) == wire.TEX_RG8 else 4):
                    raise ValueError("a JPEG record of shape %r does not fit its texture desc" % (px.shape,))
                heap[to:to + px.size] = px.reshape(-1)
                continue
            for w, h, nsrc, ndst in self._chain_layout(int(t["width"]), int(t["height"]), int(t["num_mips"]), int(t["format"]), enc):
                if enc in (wire.TEX_SRC_RAW, wire.TEX_SRC_RAW_MIP0):
                    heap[to:to + nsrc] = self.texture_payload[at:at + nsrc]
                else:
                    (L.zrh_bc7_decode if enc == wire.TEX_SRC_BC7 else L.zrh_bc5_decode)(self.texture_payload.ctypes.data + at, w, h, heap.ctypes.data + to)
                at, to = at + nsrc, to + ndst
        gen = np.ascontiguousarray(self.textures[np.isin(self.texture_sources["encoding"], (wire.TEX_SRC_RAW_MIP0, wire.TEX_SRC_JPEG_COEF))])
        if len(gen):
            mip_generate(gen, heap)
        self.texels = heap

    def texture_blocks(self):
        """wire.TextureBlocks (zr_texture_blocks) over the sources and the payload; None for a scene without sources"""
        if len(self.texture_sources) == 0:
            return None
        self.texture_sources = np.ascontiguousarray(self.texture_sources)
        self.texture_payload = np.ascontiguousarray(self.texture_payload, np.uint8)
        b = wire.TextureBlocks()
        b.sources, b.payload, b.payload_bytes = self.texture_sources.ctypes.data, self.texture_payload.ctypes.data, len(self.texture_payload)
        return b

    def add_texture(self, image, fmt=wire.TEX_RGBA8_SRGB, mips=True):
        """Appends one texture (H x W x C uint8, C = 4 for RGBA8 formats, 2 for RG8) with its full mip chain and returns
        its index in the heap.  Mips are 2x2 box filtered on the stored bytes (round half up; an odd size drops its last
        row / column -- floor convention, as the reference's offline texconv does); the reference ships them inside the
        .dds (Tools/BCnCompressglTF), here they are the caller's data like any other texel."""
        if len(self.texture_sources):
            raise ValueError("the scene holds block-compressed texture sources: a heap is either all sources or all texels")
        img = np.ascontiguousarray(image, np.uint8)
        ch = 2 if fmt == wire.TEX_RG8 else 4
        assert img.ndim == 3 and img.shape[2] == ch
        chain = [img]
        while mips and (chain[-1].shape[0] > 1 or chain[-1].shape[1] > 1):
            a = chain[-1].astype(np.uint32)
            h, w = a.shape[0], a.shape[1]
            h2, w2 = max(1, h // 2), max(1, w // 2)
            ys = (np.arange(h2) * 2, np.minimum(np.arange(h2) * 2 + 1, h - 1))
            xs = (np.arange(w2) * 2, np.minimum(np.arange(w2) * 2 + 1, w - 1))
            acc = sum(a[np.ix_(yy, xx)] for yy in ys for xx in xs)
            chain.append(((acc + 2) // 4).astype(np.uint8))
        off = (len(self.texels) + 3) // 4 * 4
        blob = np.concatenate([m.reshape(-1) for m in chain])
        self.texels = np.concatenate([self.texels, np.zeros(off - len(self.texels), np.uint8), blob])
        d = np.zeros(1, wire.TEXTURE_DESC)
        d["offset"], d["width"], d["height"], d["num_mips"], d["format"] = off, img.shape[1], img.shape[0], len(chain), fmt
        self.textures = np.concatenate([self.textures, d])
        return len(self.textures) - 1

    @property
    def num_tris(self):
        return int(self.instance_num_tris.sum())

    def desc(self) -> wire.SceneDesc:
        for name in ("vertices", "indices", "instances", "instance_to_world", "instance_mask", "instance_num_tris",
                     "materials", "emissives", "rho", "textures", "texels"):
            setattr(self, name, np.ascontiguousarray(getattr(self, name)))
        d = wire.SceneDesc()
        d.vertices = self.vertices.ctypes.data
        d.num_vertices = len(self.vertices)
        d.indices = self.indices.ctypes.data
        d.num_indices = len(self.indices)
        d.instances = self.instances.ctypes.data
        d.num_instances = len(self.instances)
        d.instance_to_world = self.instance_to_world.ctypes.data
        d.instance_mask = self.instance_mask.ctypes.data
        d.instance_num_tris = self.instance_num_tris.ctypes.data
        d.materials = self.materials.ctypes.data
        d.num_materials = len(self.materials)
        d.emissives = self.emissives.ctypes.data if len(self.emissives) else None
        d.num_emissives = len(self.emissives)
        d.rho_lut = self.rho.ctypes.data
        d.rho_dim[0], d.rho_dim[1], d.rho_dim[2] = self.rho_dim
        d.textures = self.textures.ctypes.data if len(self.textures) else None
        d.num_textures = len(self.textures)
        d.texels = self.texels.ctypes.data if len(self.texels) else None
        d.texel_bytes = len(self.texels) if len(self.texels) or not len(self.texture_sources) else self.texel_heap_bytes
        self._desc = d
        return d


def load_rho_dds(path):
    """Assets/LUT/rho.dds: legacy DDS header (128 B), R16_UNORM volume 64 x 32 x 16 (BSDF.hlsli:279-296)."""
    raw = open(path, "rb").read()
    assert raw[:4] == b"DDS "
    h = struct.unpack("<31I", raw[4:128])
    height, width, depth = h[2], h[3], h[5]
    data = np.frombuffer(raw, dtype="<u2", offset=128, count=width * height * depth).copy()
    return data, (width, height, depth)


def default_rho_path():
    here = os.path.dirname(os.path.abspath(__file__))
    p = os.path.join(here, "assets", "rho_lut_u16.bin")
    return p


def load_rho_default():
    """The rho LUT travels with the package as raw R16 data (zetaray_amd/assets/rho_lut_u16.bin, 64 KiB)."""
    p = default_rho_path()
    data = np.fromfile(p, dtype="<u2")
    assert data.size == 64 * 32 * 16
    return data, (64, 32, 16)


def load_rpt_sample_set():
    """512 x half2 spatial-search points of ReSTIR PT (reference: ReSTIR_PT/SampleSet.hlsli), raw binary16 pairs."""
    p = os.path.join(os.path.dirname(default_rho_path()), "rpt_sample_set_f16.bin")
    data = np.fromfile(p, dtype="<u2")
    assert data.size == 1024
    return data


def load_rdi_sample_set():
    """32 x half2 spatial sample points of ReSTIR DI (reference: DirectLighting/Emissive/Resampling.hlsli k_samples)."""
    p = os.path.join(os.path.dirname(default_rho_path()), "rdi_sample_set_f16.bin")
    data = np.fromfile(p, dtype="<u2")
    assert data.size == 64
    return data


def _accessor(g, bins, idx):
    acc = g["accessors"][idx]
    bv = g["bufferViews"][acc["bufferView"]]
    buf = bins[bv["buffer"]]
    dt = np.dtype(_COMP[acc["componentType"]])
    nc = _NCOMP[acc["type"]]
    off = bv.get("byteOffset", 0) + acc.get("byteOffset", 0)
    stride = bv.get("byteStride", 0) or dt.itemsize * nc
    count = acc["count"]
    if stride == dt.itemsize * nc:
        a = np.frombuffer(buf, dtype=dt, offset=off, count=count * nc).reshape(count, nc)
    else:
        a = np.ndarray((count, nc), dtype=dt, buffer=buf, offset=off, strides=(stride, dt.itemsize))
    return np.array(a)


def load_gltf(path, rho=None) -> Scene:
    """glTF -> wire formats in Python (meshes, materials, node hierarchy).  It does not read "animations": an animated file loads as the still scene at
    its nodes' rest transforms; load_gltf_native reads them (sc.animation)."""
    g = json.load(open(path))
    base = os.path.dirname(path)
    bins = [open(os.path.join(base, b["uri"]), "rb").read() for b in g["buffers"]]

    sc = Scene()
    # ---- materials (index 0 = default material, glTF materials follow: EmissiveInstance.MaterialIdx = idx + 1) ----
    mats = [pack_material(metallic=0.0, roughness=0.3)]     # Material() defaults, Material.h:66-95
    for m in g.get("materials", []):
        pbr = m.get("pbrMetallicRoughness", {})
        ext = m.get("extensions", {})
        kw = dict(
            base_color=pbr.get("baseColorFactor", [1, 1, 1, 1]),
            metallic=pbr.get("metallicFactor", 1.0),
            roughness=pbr.get("roughnessFactor", 1.0),
            emissive_factor=m.get("emissiveFactor", [0, 0, 0]),
            emissive_strength=ext.get("KHR_materials_emissive_strength", {}).get("emissiveStrength", 1.0),
            ior=ext.get("KHR_materials_ior", {}).get("ior", 1.5),
            transmission=ext.get("KHR_materials_transmission", {}).get("transmissionFactor", 0.0),
            coat_weight=ext.get("KHR_materials_clearcoat", {}).get("clearcoatFactor", 0.0),
            coat_roughness=ext.get("KHR_materials_clearcoat", {}).get("clearcoatRoughnessFactor", 0.0),
            alpha_cutoff=m.get("alphaCutoff", 0.5),
            alpha_mode={"OPAQUE": 0, "MASK": 1, "BLEND": 2}[m.get("alphaMode", "OPAQUE")],
            double_sided=m.get("doubleSided", False),
        )
        mats.append(pack_material(**kw))
    sc.materials = np.array(mats, dtype=wire.MATERIAL)

    # ---- meshes: one entry per (mesh, primitive) ----
    verts, inds, mesh_info = [], [], {}
    vtx_off = idx_off = 0
    for mi, mesh in enumerate(g["meshes"]):
        for pi, prim in enumerate(mesh["primitives"]):
            at = prim["attributes"]
            pos = _accessor(g, bins, at["POSITION"]).astype(np.float32)
            nrm = _accessor(g, bins, at["NORMAL"]).astype(np.float32)
            v = np.zeros(len(pos), wire.VERTEX)
            v["pos"] = pos * np.array([1, 1, -1], np.float32)
            v["normal"] = encode_octahedral(nrm * np.array([1, 1, -1], np.float32))
            if "TEXCOORD_0" in at:
                v["uv"] = _accessor(g, bins, at["TEXCOORD_0"]).astype(np.float32)
                if "TANGENT" in at:
                    tan = _accessor(g, bins, at["TANGENT"]).astype(np.float32)[:, :3]
                    v["tangent"] = encode_octahedral(tan * np.array([1, 1, -1], np.float32))
            idx = _accessor(g, bins, prim["indices"]).astype(np.uint32).reshape(-1, 3)
            idx = idx[:, [0, 2, 1]].reshape(-1)          # clockwise ordering
            mesh_info[(mi, pi)] = dict(vtx=vtx_off, idx=idx_off, nidx=len(idx), mat=prim.get("material", -1))
            verts.append(v)
            inds.append(idx)
            vtx_off += len(v)
            idx_off += len(idx)
    sc.vertices = np.concatenate(verts)
    sc.indices = np.concatenate(inds)

    # ---- instances: scene nodes in order (flat hierarchy only; children are walked depth-first) ----
    insts, mats_w, masks, ntris, emissive_tris = [], [], [], [], []

    def is_emissive(matidx):
        if matidx < 0:
            return False
        m = g["materials"][matidx]
        ef = m.get("emissiveFactor", [0, 0, 0])
        return (ef[0] + ef[1] + ef[2]) > 0 or "emissiveTexture" in m

    def walk(nidx, parent):
        node = g["nodes"][nidx]
        assert "matrix" not in node, "matrix nodes not supported by this loader"
        s = np.array(node.get("scale", [1, 1, 1]), np.float32)
        t = np.array(node.get("translation", [0, 0, 0]), np.float32) * np.array([1, 1, -1], np.float32)
        r = np.array(node.get("rotation", [0, 0, 0, 1]), np.float32) * np.array([-1, -1, 1, 1], np.float32)
        local = np.vstack([trs_matrix(t, r, s), [0, 0, 0, 1]]).astype(np.float32)
        world = (parent @ local).astype(np.float32)
        if "mesh" in node:
            mi = node["mesh"]
            for pi in range(len(g["meshes"][mi]["primitives"])):
                info = mesh_info[(mi, pi)]
                inst = np.zeros((), wire.MESH_INSTANCE)
                inst["base_vtx_offset"] = info["vtx"]
                inst["base_idx_offset"] = info["idx"]
                # FillMeshInstanceData: decomposeSRT of the world matrix, then quantise.  Only un-parented TRS nodes
                # are exact here (the Cornell scenes); general hierarchies would need a polar decomposition.
                rq = r / np.float32(np.sqrt(np.float32(np.dot(r, r))))
                inst["rotation"] = np.rint((rq * np.float32(0.5) + np.float32(0.5)) * np.float32(65535.0)).astype(np.uint16)
                inst["scale"] = f32_to_f16_bits(s)
                inst["mat_idx"] = info["mat"] + 1
                inst["translation"] = world[:3, 3]
                inst["prev_rotation"] = inst["rotation"]
                inst["prev_scale"] = inst["scale"]
                inst["d_translation"] = f32_to_f16_bits([0, 0, 0])
                inst["base_color_tex"] = 0xFFFF
                matp = sc.materials[info["mat"] + 1]
                alpha = np.float32((int(matp["base_color_factor"]) >> 24) & 0xFF) / np.float32(255.0)
                cutoff = np.float32((int(matp["emissive_tex_alpha_cutoff_coat_ior"]) >> 16) & 0xFF) / np.float32(255.0)
                inst["alpha_factor_cutoff"] = unorm8(alpha) | (unorm8(cutoff) << 8)
                em = is_emissive(info["mat"])
                inst["base_emissive_tri_offset"] = 0xFFFFFFFF
                insts.append(inst)
                mats_w.append(world[:3, :].reshape(12))
                masks.append(wire.SUBGROUP_EMISSIVE if em else wire.SUBGROUP_NON_EMISSIVE)
                ntris.append(info["nidx"] // 3)
                if em:
                    emissive_tris.append((len(insts) - 1, info, world[:3, :]))
        for c in node.get("children", []):
            walk(c, world)

    scene_idx = g.get("scene", 0)
    for n in g["scenes"][scene_idx]["nodes"]:
        walk(n, np.eye(4, dtype=np.float32))

    sc.instances = np.array(insts, dtype=wire.MESH_INSTANCE)
    sc.instance_to_world = np.array(mats_w, dtype=np.float32)
    sc.instance_mask = np.array(masks, dtype=np.uint8)
    sc.instance_num_tris = np.array(ntris, dtype=np.uint32)

    # ---- emissive triangles (glTF.cpp:692-767 then SceneCore.cpp:196-236) ----
    ems = []
    for inst_idx, info, M in emissive_tris:
        sc.instances[inst_idx]["base_emissive_tri_offset"] = len(ems)
        matp = sc.materials[info["mat"] + 1]
        tri_idx = sc.indices[info["idx"]:info["idx"] + info["nidx"]].reshape(-1, 3)
        for prim, (i0, i1, i2) in enumerate(tri_idx):
            vs = [sc.vertices[info["vtx"] + i] for i in (i0, i1, i2)]
            # packed in OBJECT space at load, then decoded, transformed and re-encoded unless the instance sits at the identity
            # (glTF.cpp:692-767, SceneCore.cpp:196-236; emissive_to_world)
            pw = [v["pos"].astype(np.float32) for v in vs]
            ems.append(pack_emissive_triangle(
                pw[0], pw[1], pw[2], [v["uv"] for v in vs],
                factor_rgb8=int(matp["emissive_factor_normal_scale"]) & 0xFFFFFF,
                tex=int(matp["emissive_tex_alpha_cutoff_coat_ior"]) & 0xFFFF,
                strength_h=int(matp["emissive_strength_ior"]) & 0xFFFF,
                tri_id=pcg3d(inst_idx, 0, prim)[0],
                double_sided=bool(int(matp["coat_color_flags"]) & (1 << 25))))
    sc.emissives = np.array(ems, dtype=wire.EMISSIVE_TRI) if ems else np.zeros(0, wire.EMISSIVE_TRI)
    sc.emissives_initial = sc.emissives.copy()      # object space: what move_emissive_instance transforms
    for inst_idx, info, M in emissive_tris:
        M = np.ascontiguousarray(M, np.float32)
        if not np.array_equal(M, np.eye(3, 4, dtype=np.float32)):
            b, n = int(sc.instances[inst_idx]["base_emissive_tri_offset"]), info["nidx"] // 3
            sc.emissives[b:b + n] = emissive_to_world(sc.emissives_initial[b:b + n], M)

    if rho is None:
        sc.rho, sc.rho_dim = load_rho_default()
    else:
        sc.rho, sc.rho_dim = rho
    return sc


def emissive_to_world(tris, to_world_3x4):
    """SceneCore's emissive transform (SceneCore.cpp:196-236, UpdateEmissivePositions :913-955) through the C++ restatement pinned to the reference's
    own LoadVertices / mul / StoreVertices (tests/test_scene_io.py): decode -> transform -> re-encode each record of `tris`"""
    import ctypes as C
    L = _sceneio_lib()
    tris = np.ascontiguousarray(tris, wire.EMISSIVE_TRI)
    out = np.zeros_like(tris)
    M = np.ascontiguousarray(to_world_3x4, np.float32).reshape(12)
    for i in range(len(tris)):
        L.zrh_emissive_to_world(C.c_void_p(tris[i:i + 1].ctypes.data), C.c_void_p(M.ctypes.data), C.c_void_p(out[i:i + 1].ctypes.data))
    return out


def move_emissive_instance(sc, idx, **kw):
    """move_instance for an emissive instance: also re-derives its world-space EmissiveTriangle records from the object-space ones (needs
    sc.emissives_initial: the glTF loaders provide it).  Returns (instances, instance_to_world, first emissive triangle, the new records)."""
    inst, xw = move_instance(sc, idx, **kw)
    b, n = int(sc.instances[idx]["base_emissive_tri_offset"]), int(sc.instance_num_tris[idx])
    assert b != 0xFFFFFFFF, "not an emissive instance"
    sc.emissives[b:b + n] = emissive_to_world(sc.emissives_initial[b:b + n], sc.instance_to_world[idx])
    return inst, xw, b, sc.emissives[b:b + n]


def _sceneio_lib():
    """zetaray_amd/libzetaray_sceneio.so: the C++ scene ingestion (zetaray_amd/host/zr_scene_io.cpp; no HIP dependency)"""
    import ctypes as C
    global _SCENEIO
    if "_SCENEIO" not in globals() or _SCENEIO is None:
        L = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libzetaray_sceneio.so"))
        L.zrh_gltf_load.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.zrh_gltf_load_ex.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.zrh_scene_data_texture_blocks.restype = C.POINTER(wire.TextureBlocks)
        L.zrh_scene_data_texture_blocks.argtypes = [C.c_void_p]
        L.zrh_scene_io_last_error.restype = C.c_char_p
        L.zrh_scene_data_desc.restype = C.POINTER(wire.SceneDesc)
        L.zrh_scene_data_desc.argtypes = [C.c_void_p]
        L.zrh_scene_data_tex_offsets.argtypes = [C.c_void_p, C.c_void_p]
        L.zrh_scene_data_destroy.argtypes = [C.c_void_p]
        L.zrh_emissive_to_world.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _SCENEIO = L
    return _SCENEIO


LOAD_KEEP_COMPRESSED = 1      # ZRH_LOAD_KEEP_COMPRESSED
LOAD_JPEG = 2      # ZRH_LOAD_JPEG
LOAD_DEFORMED_LIGHTS = 4      # ZRH_LOAD_DEFORMED_LIGHTS


def emissive_from_vertices(rec, p0, p1, p2, to_world_3x4):
    """zrh_emissive_from_vertices: a light triangle whose vertices were deformed -- (object-space record, world record) from the record `rec` (a
    wire.EMISSIVE_TRI scalar or 1-element array; its non-geometric fields are kept), the three object-space positions and the owner's matrix"""
    import ctypes as C
    L = _sceneio_lib()
    L.zrh_emissive_from_vertices.argtypes = [C.c_void_p] * 7
    rec = np.ascontiguousarray(rec, wire.EMISSIVE_TRI).reshape(1)
    p = [np.ascontiguousarray(q, np.float32).reshape(3) for q in (p0, p1, p2)]
    M = np.ascontiguousarray(to_world_3x4, np.float32).reshape(12)
    obj, world = np.zeros(1, wire.EMISSIVE_TRI), np.zeros(1, wire.EMISSIVE_TRI)
    L.zrh_emissive_from_vertices(rec.ctypes.data, p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, M.ctypes.data, obj.ctypes.data, world.ctypes.data)
    return obj[0], world[0]


def refresh_emissives(sc, vertices, first, count):
    """zrh_scene_data_refresh_emissives on a Scene: light triangles [first, first + count) re-derived from `vertices` (the scene's whole vertex array with
    the pose in it; None: sc.vertices) and their owners' matrices.  Writes sc.emissives and sc.emissives_initial (the object-space records) in place and
    returns the dirty range (first, count) the host-form update uploads -- the host form of api.Scene.refresh_emissives"""
    import ctypes as C
    L = _sceneio_lib()
    vp = C.c_void_p
    L.zrh_scene_data_from_desc.argtypes = [vp] * 3
    L.zrh_scene_data_refresh_emissives.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.zrh_scene_data_dirty_emissives.argtypes = [vp] * 3
    L.zrh_scene_data_initial_emissives.restype = vp
    L.zrh_scene_data_initial_emissives.argtypes = [vp]
    desc = sc.desc()
    init = np.ascontiguousarray(sc.emissives_initial, wire.EMISSIVE_TRI)
    h = vp()
    if L.zrh_scene_data_from_desc(C.addressof(desc), init.ctypes.data if len(init) else None, C.byref(h)) != 0:
        raise ValueError(L.zrh_scene_io_last_error().decode())
    try:
        v = None if vertices is None else np.ascontiguousarray(vertices, wire.VERTEX).reshape(-1)
        if v is not None and len(v) != len(sc.vertices):
            raise ValueError(f"refresh_emissives: {len(v)} vertices, the scene has {len(sc.vertices)}")
        if L.zrh_scene_data_refresh_emissives(h, v.ctypes.data if v is not None else None, int(first), int(count)) != 0:
            raise ValueError(L.zrh_scene_io_last_error().decode())
        n = len(sc.emissives)
        d = L.zrh_scene_data_desc(h).contents
        if n:
            sc.emissives[:] = np.frombuffer(C.string_at(d.emissives, n * 48), wire.EMISSIVE_TRI)
            sc.emissives_initial[:] = np.frombuffer(C.string_at(L.zrh_scene_data_initial_emissives(h), n * 48), wire.EMISSIVE_TRI)
        f, c = C.c_uint32(), C.c_uint32()
        L.zrh_scene_data_dirty_emissives(h, C.byref(f), C.byref(c))
        return f.value, c.value
    finally:
        L.zrh_scene_data_destroy(h)


def skin_pose(anim, skin, rest, t):
    """zrh_skin_pose: the host form of skinning -- the rest records of skin's ranges (range after range; wire.VERTEX) posed for time t by include/zr_anim.h
    and include/zr_skin.h on the host; anim / skin: wire.AnimDesc / wire.SkinDesc"""
    import ctypes as C
    L = _sceneio_lib()
    L.zrh_skin_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    rest = np.ascontiguousarray(rest, wire.VERTEX).reshape(-1)
    if len(rest) != int(skin.ranges["num_vertices"].sum()):
        raise ValueError(f"skin_pose: {len(rest)} rest records, the ranges list {int(skin.ranges['num_vertices'].sum())} vertices")
    out = np.zeros(len(rest), wire.VERTEX)
    a, k = anim.c_desc(), skin.c_desc()
    if L.zrh_skin_pose(C.addressof(a), C.addressof(k), float(t), rest.ctypes.data if len(rest) else None, out.ctypes.data if len(rest) else None) != 0:
        raise ValueError(L.zrh_scene_io_last_error().decode())
    return out


def morph_pose(anim, skin, morph, rest, t):
    """zrh_morph_pose: the host form of morph targets -- the rest records of morph's ranges (range after range; wire.VERTEX) posed for time t by
    include/zr_morph.h on the host, and by include/zr_skin.h after it where a range is also a range of `skin`; anim / skin (or None) / morph:
    wire.AnimDesc / wire.SkinDesc / wire.MorphDesc"""
    import ctypes as C
    L = _sceneio_lib()
    L.zrh_morph_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    rest = np.ascontiguousarray(rest, wire.VERTEX).reshape(-1)
    if len(rest) != int(morph.ranges["num_vertices"].sum()):
        raise ValueError(f"morph_pose: {len(rest)} rest records, the ranges list {int(morph.ranges['num_vertices'].sum())} vertices")
    out = np.zeros(len(rest), wire.VERTEX)
    a, k, m = (anim.c_desc() if anim is not None else None), (skin.c_desc() if skin is not None else None), morph.c_desc()
    if L.zrh_morph_pose(C.addressof(a) if a is not None else None, C.addressof(k) if k is not None else None, C.addressof(m), float(t),
                        rest.ctypes.data if len(rest) else None, out.ctypes.data if len(rest) else None) != 0:
        raise ValueError(L.zrh_scene_io_last_error().decode())
    return out


def mip_generate(descs, texels):
    """zrh_mip_generate: levels 1 .. of the chains `descs` (wire.TEXTURE_DESC) names in `texels` (uint8, contiguous), in place, from their level 0"""
    import ctypes as C
    L = _sceneio_lib()
    L.zrh_mip_generate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    descs = np.ascontiguousarray(descs, wire.TEXTURE_DESC)
    assert texels.dtype == np.uint8 and texels.flags["C_CONTIGUOUS"]
    for t in descs:
        last = Scene._chain_layout(int(t["width"]), int(t["height"]), int(t["num_mips"]), int(t["format"]), wire.TEX_SRC_RAW)
        if int(t["offset"]) + sum(l[3] for l in last) > len(texels):
            raise ValueError("a chain ends beyond the %d texel bytes" % len(texels))
    if L.zrh_mip_generate(descs.ctypes.data, len(descs), texels.ctypes.data) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    return texels


def png_decode(data, name="<memory>"):
    """zrh_png_decode: the bytes of a PNG file -> (h, w, 4) uint8 RGBA"""
    import ctypes as C
    L = _sceneio_lib()
    L.zrh_png_decode.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    data = bytes(data)
    w, h = C.c_uint32(), C.c_uint32()
    if L.zrh_png_decode(os.fsencode(name), data, len(data), C.byref(w), C.byref(h), None, 0) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    out = np.zeros((h.value, w.value, 4), np.uint8)
    if L.zrh_png_decode(os.fsencode(name), data, len(data), C.byref(w), C.byref(h), out.ctypes.data, out.nbytes) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    return out


def decode_jpeg(data, name="<memory>"):
    """zrh_jpeg_decode: the bytes of a baseline JPEG file -> (h, w, 4) uint8 RGBA (alpha 255), through include/zr_jpeg.h"""
    import ctypes as C
    L = _sceneio_lib()
    L.zrh_jpeg_decode.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    data = bytes(data)
    w, h = C.c_uint32(), C.c_uint32()
    if L.zrh_jpeg_decode(os.fsencode(name), data, len(data), C.byref(w), C.byref(h), None, 0) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    out = np.zeros((h.value, w.value, 4), np.uint8)
    if L.zrh_jpeg_decode(os.fsencode(name), data, len(data), C.byref(w), C.byref(h), out.ctypes.data, out.nbytes) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    return out


def pack_jpeg(data, name="<memory>", channel_map=wire.JPEG_MAP_RGBA):
    """zrh_jpeg_pack: the entropy decode of a baseline JPEG file alone -> the record of include/zr_jpeg.h (uint8; what a wire.TEX_SRC_JPEG_COEF source names)"""
    import ctypes as C
    L = _sceneio_lib()
    L.zrh_jpeg_pack.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    data = bytes(data)
    n = C.c_size_t()
    if L.zrh_jpeg_pack(os.fsencode(name), data, len(data), channel_map, None, 0, C.byref(n)) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    out = np.zeros(n.value, np.uint8)
    if L.zrh_jpeg_pack(os.fsencode(name), data, len(data), channel_map, out.ctypes.data, out.nbytes, C.byref(n)) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    return out


def jpeg_expand(record):
    """zrh_jpeg_expand: a record of pack_jpeg (uint8; bytes behind its end are ignored) -> (h, w, 4) or (h, w, 2) uint8, by its channel map, on the host"""
    import ctypes as C
    L = _sceneio_lib()
    L.zrh_jpeg_expand.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    record = np.ascontiguousarray(record, np.uint8)
    w, h = C.c_uint32(), C.c_uint32()
    if L.zrh_jpeg_expand(record.ctypes.data, len(record), C.byref(w), C.byref(h), None, 0) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    ch = 4 if len(record) >= 32 and int(record[28:32].view("<u4")[0]) == wire.JPEG_MAP_RGBA else 2
    out = np.zeros((h.value, w.value, ch), np.uint8)
    if L.zrh_jpeg_expand(record.ctypes.data, len(record), C.byref(w), C.byref(h), out.ctypes.data, out.nbytes) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    return out


def load_gltf_native(path, rho=None, textures="decoded", jpeg=False, deformed_lights=False):
    """glTF -> wire formats through the C++ loader (MeshInstance quantisation by decomposeSRT of the world matrix, node hierarchies, matrix
    nodes, DDS material textures decoded to the texel heap, PNG ones with their mip chain generated by include/zr_mipgen.h).  Returns (Scene, texture-table offsets dict for set_texture_heap_offsets).
    A file with "animations" (LINEAR translation / rotation / scale channels) also gives sc.animation, a wire.AnimDesc over the dynamic closure of
    its node hierarchy (Scene.set_animation / Scene.animate in api.py), and sc.emissives_initial, the object-space light records; None without.
    A file with skinned nodes ("skins", JOINTS_0 / WEIGHTS_0) also gives sc.skinning, a wire.SkinDesc over the animation's node table (Scene.set_skinning,
    after Scene.set_animation); None without.
    A file with morph targets driven by a "weights" channel also gives sc.morph, a wire.MorphDesc (Scene.set_morph, after set_animation and set_skinning); None
    without.  Targets without a channel are applied once at load with their default weights.
    textures="compressed": the .dds payloads are not decoded (ZRH_LOAD_KEEP_COMPRESSED): sc.texels stays empty, sc.texture_sources / sc.texture_payload
    carry the blocks and api.Scene decodes them on the device (zr_scene_create_compressed); sc.decode_textures() makes the texels on the host.
    A .png image travels as its level 0 (wire.TEX_SRC_RAW_MIP0) and its other levels are generated on the device.
    jpeg=True (ZRH_LOAD_JPEG): .jpg / .jpeg images are read wherever a .png is (refused by name without it): decoded on the host through include/zr_jpeg.h, or
    with textures="compressed" entropy-decoded only and handed over as wire.TEX_SRC_JPEG_COEF records, which the same header turns into level 0 on the device.
    deformed_lights=True (ZRH_LOAD_DEFORMED_LIGHTS): a skinned or morphed primitive may carry an emissive material (refused by name without it); its light
    records come from the rest pose and follow the pose with every Scene.animate once the skin / morph set is on the device."""
    import ctypes as C
    if textures not in ("decoded", "compressed"):
        raise ValueError("textures must be 'decoded' or 'compressed', not %r" % (textures,))
    L = _sceneio_lib()
    rho_data, rho_dim = load_rho_default() if rho is None else rho
    rho_data = np.ascontiguousarray(rho_data, np.uint16)
    dims = (C.c_uint32 * 3)(*rho_dim)
    h = C.c_void_p()
    if L.zrh_gltf_load_ex(os.fsencode(path), rho_data.ctypes.data, dims, (LOAD_KEEP_COMPRESSED if textures == "compressed" else 0) | (LOAD_JPEG if jpeg else 0) | (LOAD_DEFORMED_LIGHTS if deformed_lights else 0), C.byref(h)) != 0:
        raise RuntimeError(L.zrh_scene_io_last_error().decode())
    try:
        d = L.zrh_scene_data_desc(h).contents

        def arr(ptr, n, dt):
            if not ptr or n == 0:
                return np.zeros(0, dt)
            dt = np.dtype(dt)
            return np.frombuffer(C.string_at(ptr, n * dt.itemsize), dt).copy()
        sc = Scene()
        sc.vertices = arr(d.vertices, d.num_vertices, wire.VERTEX)
        sc.indices = arr(d.indices, d.num_indices, np.uint32)
        sc.instances = arr(d.instances, d.num_instances, wire.MESH_INSTANCE)
        sc.instance_to_world = arr(d.instance_to_world, d.num_instances * 12, np.float32).reshape(-1, 12)
        sc.instance_mask = arr(d.instance_mask, d.num_instances, np.uint8)
        sc.instance_num_tris = arr(d.instance_num_tris, d.num_instances, np.uint32)
        sc.materials = arr(d.materials, d.num_materials, wire.MATERIAL)
        sc.emissives = arr(d.emissives, d.num_emissives, wire.EMISSIVE_TRI)
        sc.textures = arr(d.textures, d.num_textures, wire.TEXTURE_DESC)
        sc.texels = arr(d.texels, d.texel_bytes, np.uint8)
        tb = L.zrh_scene_data_texture_blocks(h)
        if tb:
            sc.texture_sources = arr(tb.contents.sources, d.num_textures, wire.TEXTURE_SOURCE)
            sc.texture_payload = arr(tb.contents.payload, tb.contents.payload_bytes, np.uint8)
            sc.texel_heap_bytes = int(d.texel_bytes)
        sc.rho, sc.rho_dim = rho_data, tuple(rho_dim)
        sc.animation = None
        L.zrh_scene_data_animation.argtypes = [C.c_void_p]
        L.zrh_scene_data_animation.restype = C.POINTER(wire.AnimDescC)
        a = L.zrh_scene_data_animation(h)
        if a:
            a = a.contents
            sc.animation = wire.AnimDesc(arr(a.nodes, a.num_nodes, wire.ANIM_NODE), arr(a.keys, a.num_keys, wire.KEYFRAME),
                                         arr(a.instance_idx, a.num_instances, np.uint32), arr(a.instance_node, a.num_instances, np.uint32))
            L.zrh_scene_data_initial_emissives.restype = C.c_void_p
            L.zrh_scene_data_initial_emissives.argtypes = [C.c_void_p]
            sc.emissives_initial = arr(L.zrh_scene_data_initial_emissives(h), d.num_emissives, wire.EMISSIVE_TRI)
        sc.skinning = None
        L.zrh_scene_data_skinning.argtypes = [C.c_void_p]
        L.zrh_scene_data_skinning.restype = C.POINTER(wire.SkinDescC)
        k = L.zrh_scene_data_skinning(h)
        if k:
            k = k.contents
            sc.skinning = wire.SkinDesc(arr(k.joints, k.num_joints, wire.SKIN_JOINT), arr(k.ranges, k.num_ranges, wire.SKIN_RANGE),
                                        arr(k.influences, k.num_influences, wire.SKIN_INFLUENCE))
        sc.morph = None
        L.zrh_scene_data_morph.argtypes = [C.c_void_p]
        L.zrh_scene_data_morph.restype = C.POINTER(wire.MorphDescC)
        m = L.zrh_scene_data_morph(h)
        if m:
            m = m.contents
            sc.morph = wire.MorphDesc(arr(m.tracks, m.num_tracks, wire.MORPH_TRACK), arr(m.targets, m.num_targets, wire.MORPH_TARGET), arr(m.ranges, m.num_ranges, wire.MORPH_RANGE),
                                      arr(m.times, m.num_times, np.dtype("<f4")), arr(m.values, m.num_values, np.dtype("<f4")),
                                      arr(m.rest_weights, m.num_rest_weights, np.dtype("<f4")), arr(m.deltas, 3 * m.num_deltas, np.dtype("<f4")))
        offs = (C.c_uint32 * 4)()
        L.zrh_scene_data_tex_offsets(h, offs)
        return sc, dict(base_color=offs[0], normal=offs[1], metallic_roughness=offs[2], emissive=offs[3])
    finally:
        L.zrh_scene_data_destroy(h)


def save_npz(sc: Scene, path):
    """Wire-format fixture (tests/golden/*.npz); the rho LUT is not stored (it ships in zetaray_amd/assets).  The fixture holds texels, not texture
    sources: a scene with block-compressed sources must have run decode_textures() first."""
    if len(sc.textures) and len(getattr(sc, "texture_sources", ())) and len(sc.texels) != sc.texel_heap_bytes:
        raise ValueError("save_npz: the scene's textures are block-compressed sources; call decode_textures() first")
    np.savez_compressed(path, vertices=sc.vertices, indices=sc.indices, instances=sc.instances,
                        instance_to_world=sc.instance_to_world, instance_mask=sc.instance_mask,
                        instance_num_tris=sc.instance_num_tris, materials=sc.materials, emissives=sc.emissives,
                        **({"textures": sc.textures, "texels": sc.texels} if len(sc.textures) else {}),
                        **({"emissives_initial": sc.emissives_initial} if getattr(sc, "emissives_initial", None) is not None else {}))


def load_npz(path) -> Scene:
    z = np.load(path)
    sc = Scene()
    sc.vertices = z["vertices"].astype(wire.VERTEX)
    sc.indices = z["indices"].astype(np.uint32)
    sc.instances = z["instances"].astype(wire.MESH_INSTANCE)
    sc.instance_to_world = z["instance_to_world"].astype(np.float32)
    sc.instance_mask = z["instance_mask"].astype(np.uint8)
    sc.instance_num_tris = z["instance_num_tris"].astype(np.uint32)
    sc.materials = z["materials"].astype(wire.MATERIAL)
    sc.emissives = z["emissives"].astype(wire.EMISSIVE_TRI)
    if "textures" in z.files:
        sc.textures, sc.texels = z["textures"].astype(wire.TEXTURE_DESC), z["texels"].astype(np.uint8)
    if "emissives_initial" in z.files:      # object-space records, for move_emissive_instance
        sc.emissives_initial = z["emissives_initial"].astype(wire.EMISSIVE_TRI)
    sc.rho, sc.rho_dim = load_rho_default()
    return sc


def pack_emissive_triangle(v0, v1, v2, uvs, factor_rgb8, tex, strength_h, tri_id, double_sided):
    """RT::EmissiveTriangle ctor + StoreVertices (RtCommon.h:73-166): normalised edges oct-encoded as UNORM16 with
    round-to-nearest, half edge lengths; ID patched to the PCG3d hash (SceneCore.cpp:229-235)."""
    e = np.zeros((), wire.EMISSIVE_TRI)
    v0, v1, v2 = (np.asarray(v, np.float32) for v in (v0, v1, v2))
    e["vtx0"] = v0
    e0, e1 = v1 - v0, v2 - v0
    l0 = np.float32(np.sqrt(np.float32(np.dot(e0, e0))))
    l1 = np.float32(np.sqrt(np.float32(np.dot(e1, e1))))
    e["v0v1"] = encode_octahedral(e0 / l0)[0]
    e["v0v2"] = encode_octahedral(e1 / l1)[0]
    e["edge_lengths"] = f32_to_f16_bits([l0, l1])
    e["id"] = tri_id
    e["packed_a"] = (factor_rgb8 & 0xFFFFFF) | (1 << 24) | ((1 << 25) if double_sided else 0) | ((strength_h & 0xF) << 28)
    e["packed_b"] = (tex & 0xFFFF) | (strength_h << 16)
    e["uv0"] = f32_to_f16_bits(uvs[0])
    e["uv1"] = f32_to_f16_bits(uvs[1])
    e["uv2"] = f32_to_f16_bits(uvs[2])
    return e


def make_frame_constants(width, height, frame_num=1, cam_pos=(0.0, 1.2, -4.043), view_dir=(0, 0, 1), up=(0, 1, 0),
                         vfov_deg=60.0, near=0.2, num_emissives=0, accumulate=0, camera_static=0,
                         num_frames_static=0, jitter=(0.0, 0.0)):
    """cbFrameConstants for a static pinhole camera.  Reference defaults: Win32App.cpp:1510-1511 (camera),
    DefaultRenderer.cpp:257-308 (sun / atmosphere), Camera.cpp:63-106 (lookToLH basis)."""
    cb = np.zeros((), wire.FRAME_CONSTANTS)
    eye = np.array(cam_pos, np.float32)
    z = np.array(view_dir, np.float32)
    z = z / np.float32(np.linalg.norm(z))
    x = np.cross(np.array(up, np.float32), z).astype(np.float32)
    x = x / np.float32(np.linalg.norm(x))
    y = np.cross(z, x).astype(np.float32)
    view = np.zeros((3, 4), np.float32)
    view[0, :3], view[1, :3], view[2, :3] = x, y, z
    view[:, 3] = [-np.dot(x, eye), -np.dot(y, eye), -np.dot(z, eye)]
    view_inv = np.zeros((3, 4), np.float32)
    view_inv[:, 0], view_inv[:, 1], view_inv[:, 2], view_inv[:, 3] = x, y, z, eye
    for k in ("curr_view", "prev_view"):
        cb[k] = view.reshape(12)
    for k in ("curr_view_inv", "prev_view_inv"):
        cb[k] = view_inv.reshape(12)
    cb["camera_pos"] = eye
    cb["camera_near"] = near
    cb["aspect_ratio"] = np.float32(width) / np.float32(height)
    tan_half = np.float32(np.tan(np.float32(0.5) * np.float32(np.deg2rad(vfov_deg))))
    cb["tan_half_fov"] = tan_half
    cb["pixel_spread_angle"] = np.float32(np.arctan(np.float32(2) * tan_half / np.float32(height)))
    cb["dt"] = 1.0 / 60.0
    cb["frame_num"] = frame_num
    cb["render_width"], cb["render_height"] = width, height
    cb["display_width"], cb["display_height"] = width, height
    cb["curr_camera_jitter"] = jitter
    cb["prev_camera_jitter"] = jitter
    cb["planet_radius"] = 6360.0
    ang = np.float32(np.deg2rad(0.5 * 0.526))
    cb["sun_cos_angular_radius"] = np.float32(np.cos(ang))
    cb["sun_sin_angular_radius"] = np.float32(np.sqrt(np.float32(1) - np.float32(np.cos(ang)) ** 2))
    sd = np.array([0.6565358, -0.0560669, 0.752208233], np.float32)
    sd = sd / np.float32(np.linalg.norm(sd))
    if num_emissives > 0:
        sd = np.array([0.0, 1.0, 0.0], np.float32)   # emissive scenes move the sun below the horizon (PathTracer.cpp:112-119)
    cb["sun_dir"] = sd
    cb["sun_illuminance"] = 20.0
    cb["atmosphere_altitude"] = 100.0
    cb["g"] = 0.8
    # atmosphere coefficients in 1/km, stored as unit colour + scale (DefaultRendererImpl.h:29-32, DefaultRenderer.cpp:289-306)
    def _normalize_and_store(v, ckey, skey):
        v = np.asarray(v, np.float32) * np.float32(1e-3)
        scale = np.float32(np.sqrt(np.float32(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])))
        cb[skey] = scale
        cb[ckey] = v * (np.float32(1.0) / scale)
    _normalize_and_store((5.802, 13.558, 33.1), "rayleigh_sigma_s_color", "rayleigh_sigma_s_scale")
    _normalize_and_store((0.65, 1.881, 0.085), "ozone_sigma_a_color", "ozone_sigma_a_scale")
    cb["mie_sigma_s"] = np.float32(3.996) * np.float32(1e-3)
    cb["mie_sigma_a"] = np.float32(4.4) * np.float32(1e-3)
    cb["num_frames_camera_static"] = num_frames_static
    cb["camera_static"] = camera_static
    cb["accumulate"] = accumulate
    cb["camera_ray_uv_grads_scale"] = 1.0
    cb["mip_bias"] = 0.0
    cb["num_emissive_triangles"] = num_emissives
    cb["one_div_num_emissive_triangles"] = (1.0 / num_emissives) if num_emissives else 0.0
    cb["focus_depth"] = 5.0
    cb["lens_radius"] = 0.0
    cb["dof"] = 0
    return cb


def _grid_tris(fn, nu, nv):
    """Tessellate the parametric surface fn(u, v) -> (..., 3), u, v in [0, 1], into 2 * nu * nv triangles (T, 3, 3)."""
    u, v = np.meshgrid(np.linspace(0, 1, nu + 1, dtype=np.float32), np.linspace(0, 1, nv + 1, dtype=np.float32), indexing="ij")
    Pg = fn(u, v).astype(np.float32)
    a, b, c, d = Pg[:-1, :-1], Pg[1:, :-1], Pg[1:, 1:], Pg[:-1, 1:]
    t1 = np.stack([a, b, d], axis=2).reshape(-1, 3, 3)
    t2 = np.stack([b, c, d], axis=2).reshape(-1, 3, 3)
    return np.concatenate([t1, t2]).astype(np.float32)


def _atrium_geometry(num_tris, num_emissive, room, rng):
    """Structured ("Sponza-class") content for make_synthetic_scene(layout="atrium"): displaced floor and wall, two rows of
    columns joined by arches, wavy curtains, statues -- coherent surfaces a SAH BVH handles like real architecture -- and
    `num_emissive` triangles in small spherical lanterns.  Returns ([8 arrays (T, 3, 3)], emissive (E, 3, 3))."""
    r = np.float32(room)
    budget = max(num_tris, 2048)
    s = (budget / 262144.0) ** 0.5            # linear tessellation scale

    def n(k):
        return max(2, int(round(k * s)))
    two_pi = np.float32(2 * np.pi)
    floor = _grid_tris(lambda u, v: np.stack([(2 * u - 1) * r * 0.98, -r + 0.03 + 0.02 * np.sin(40 * u) * np.cos(36 * v), (2 * v - 1) * r * 0.98], -1), n(160), n(160))
    wall = _grid_tris(lambda u, v: np.stack([(2 * u - 1) * r * 0.98, (2 * v - 1) * r * 0.98, r - 0.03 - 0.04 * np.cos(24 * u) * np.cos(24 * v)], -1), n(128), n(128))
    cols, arches = [], []
    zs = [-1.0, 0.5, 2.0, 3.5]
    for x0 in (-2.0, 2.0):
        for z0 in zs:
            cols.append(_grid_tris(lambda u, v, x0=x0, z0=z0: np.stack([x0 * r / 4 + (0.22 + 0.03 * np.cos(8 * two_pi * u)) * np.cos(two_pi * u) * r / 4,
                                                                  (2 * v - 1) * r * 0.97, z0 * r / 4 + (0.22 + 0.03 * np.cos(8 * two_pi * u)) * np.sin(two_pi * u) * r / 4], -1), n(48), n(96)))
        for za, zb in zip(zs[:-1], zs[1:]):
            zc, rad = 0.5 * (za + zb) * r / 4, 0.5 * (zb - za) * r / 4
            arches.append(_grid_tris(lambda u, v, x0=x0, zc=zc, rad=rad: np.stack([x0 * r / 4 + 0.08 * r / 4 * np.cos(two_pi * u),
                                                                            0.45 * r + (rad + 0.08 * r / 4 * np.sin(two_pi * u)) * np.sin(np.pi * v),
                                                                            zc - (rad + 0.08 * r / 4 * np.sin(two_pi * u)) * np.cos(np.pi * v)], -1), n(32), n(64)))
    curtains = []
    for x0, z0 in ((-3.2, -0.5), (-3.2, 2.2), (3.2, -0.5), (3.2, 2.2)):
        curtains.append(_grid_tris(lambda u, v, x0=x0, z0=z0: np.stack([x0 * r / 4 + 0.08 * np.sin(30 * u + 3 * v), (0.9 - 1.5 * v) * r * 0.9,
                                                                 z0 * r / 4 + (u - 0.5) * 2.2 * r / 4], -1), n(96), n(96)))
    statues = []
    for cx, cz, rad in ((-0.9, 1.2, 0.45), (0.9, 2.4, 0.35), (0.0, 3.0, 0.55)):
        def statue(u, v, cx=cx, cz=cz, rad=rad):
            w = np.float32(np.pi) * (0.02 + 0.96 * v)          # keep away from the poles: no degenerate triangles
            rr = rad * r / 4 * (1 + 0.15 * np.sin(12 * w)) * np.sin(w)
            return np.stack([cx * r / 4 + rr * np.cos(two_pi * u), -r + rad * r / 4 * (1.05 - np.cos(w)), cz * r / 4 + rr * np.sin(two_pi * u)], -1)
        statues.append(_grid_tris(statue, n(64), n(64)))
    groups = [floor, wall, np.concatenate(cols[:4]), np.concatenate(cols[4:]), np.concatenate(arches), np.concatenate(curtains[:2]),
              np.concatenate(curtains[2:]), np.concatenate(statues)]
    # lanterns: small lat-long spheres, 2 * a * b triangles each, on a jittered lattice in the upper part of the hall
    em = np.zeros((0, 3, 3), np.float32)
    if num_emissive > 0:
        a_, b_ = 10, 10
        per = 2 * a_ * b_
        count = max(1, (num_emissive + per - 1) // per)
        ctr = np.stack([rng.uniform(-0.85 * r, 0.85 * r, count), rng.uniform(-0.2 * r, 0.85 * r, count), rng.uniform(-0.6 * r, 0.9 * r, count)], 1).astype(np.float32)
        rad = rng.uniform(0.03, 0.07, count).astype(np.float32) * r / 4
        unit = _grid_tris(lambda u, v: np.stack([np.sin(np.pi * (0.02 + 0.96 * v)) * np.cos(two_pi * u), np.cos(np.pi * (0.02 + 0.96 * v)),
                                                 np.sin(np.pi * (0.02 + 0.96 * v)) * np.sin(two_pi * u)], -1), a_, b_)
        em = (ctr[:, None, None, :] + unit[None] * rad[:, None, None, None]).reshape(-1, 3, 3)[:num_emissive].astype(np.float32)
    return groups, em


def make_synthetic_scene(num_tris=262144, num_emissive=100000, seed=0x5EED, room=4.0, with_special_materials=True, layout="soup",
                         open_top=False) -> Scene:
    """Procedural Sponza-class stand-in for BASELINE config 4 (not in the reference):
    a box room, `num_tris` clutter triangles in 8 instances with different materials (diffuse, rough metal, coated,
    glossy; plus a few axis-aligned coplanar sheets that produce exact t ties) and `num_emissive` small double-sided
    emissive triangles with strengths log-uniform in [0.5, 50].  Deterministic in `seed` (numpy PCG64).
    layout="soup": uniformly random triangles (worst case for any BVH; used by the parity tests for its exact-t ties and
    material coverage).  layout="atrium": the same room, materials and light model, but structured geometry (displaced
    floor / wall, columns, arches, curtains, statues, lantern lights) -- what bench.py uses for BASELINE config 4."""
    rng = np.random.default_rng(seed)
    sc = Scene()
    mats = [pack_material(metallic=0.0, roughness=0.3),
            pack_material(base_color=(0.7, 0.7, 0.7, 1), metallic=0, roughness=1.0, double_sided=True)]
    palette = [dict(base_color=(0.63, 0.065, 0.05, 1), roughness=1.0), dict(base_color=(0.14, 0.45, 0.09, 1), roughness=0.8),
               dict(base_color=(0.2, 0.3, 0.8, 1), roughness=0.5), dict(base_color=(0.9, 0.8, 0.3, 1), roughness=0.35, metallic=1.0),
               dict(base_color=(0.8, 0.8, 0.8, 1), roughness=0.25), dict(base_color=(0.5, 0.2, 0.6, 1), roughness=0.6),
               dict(base_color=(0.7, 0.1, 0.1, 1), roughness=0.4, coat_weight=1.0, coat_roughness=0.1) if with_special_materials
               else dict(base_color=(0.7, 0.1, 0.1, 1), roughness=0.4),
               dict(base_color=(0.3, 0.6, 0.6, 1), roughness=0.15) if not with_special_materials
               else dict(base_color=(0.6, 0.9, 0.7, 1), roughness=0.2, transmission=1.0, ior=1.45, transmission_depth=0.75)]
    if with_special_materials:
        palette[2] = dict(base_color=(0.95, 0.95, 0.95, 1), roughness=0.0, transmission=1.0, ior=1.5)       # clear specular glass
        palette[5] = dict(base_color=(0.5, 0.2, 0.6, 1), roughness=0.6, subsurface=0.5, thin_walled=True)   # thin-walled diffuse transmission
    for p in palette:
        mats.append(pack_material(double_sided=True, **p))
    em_mat_idx = len(mats)
    mats.append(pack_material(base_color=(0.8, 0.8, 0.8, 1), roughness=1.0, double_sided=True, emissive_factor=(1.0, 0.85, 0.7),
                              emissive_strength=5.0))
    sc.materials = np.array(mats, dtype=wire.MATERIAL)

    verts, inds, insts, xforms, masks, ntris = [], [], [], [], [], []
    ident_q = np.rint((np.array([0, 0, 0, 1], np.float32) * np.float32(0.5) + np.float32(0.5)) * np.float32(65535.0)).astype(np.uint16)

    def add_instance(P, N, mat, mask):
        """P: (T, 3, 3) triangle vertices, N: (T, 3) face normals."""
        T = len(P)
        v = np.zeros(T * 3, wire.VERTEX)
        v["pos"] = P.reshape(-1, 3).astype(np.float32)
        v["normal"] = encode_octahedral(np.repeat(N, 3, axis=0), sse_order=False)
        v["uv"] = np.tile(np.array([[0, 0], [1, 0], [0, 1]], np.float32), (T, 1))
        inst = np.zeros((), wire.MESH_INSTANCE)
        inst["base_vtx_offset"] = sum(len(x) for x in verts)
        inst["base_idx_offset"] = sum(len(x) for x in inds)
        inst["rotation"] = ident_q
        inst["prev_rotation"] = ident_q
        inst["scale"] = f32_to_f16_bits([1, 1, 1])
        inst["prev_scale"] = inst["scale"]
        inst["mat_idx"] = mat
        inst["base_emissive_tri_offset"] = 0xFFFFFFFF
        inst["base_color_tex"] = 0xFFFF
        inst["alpha_factor_cutoff"] = 255 | (128 << 8)
        verts.append(v)
        inds.append(np.arange(T * 3, dtype=np.uint32))
        insts.append(inst)
        xforms.append(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32))
        masks.append(mask)
        ntris.append(T)
        return len(insts) - 1

    def face_normals(P):
        n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        ln = np.linalg.norm(n, axis=1, keepdims=True)
        return (n / np.maximum(ln, 1e-20)).astype(np.float32)

    # room: inward-facing box [-room, room]^3 (floor at -room)
    r = room
    c = np.array([[-r, -r, -r], [r, -r, -r], [r, r, -r], [-r, r, -r], [-r, -r, r], [r, -r, r], [r, r, r], [-r, r, r]], np.float32)
    quads = [(0, 1, 2, 3), (5, 4, 7, 6), (4, 0, 3, 7), (1, 5, 6, 2), (3, 2, 6, 7), (4, 5, 1, 0)]
    if open_top:        # no ceiling: sun and sky reach the clutter (sun / sky DI and NEE tests)
        quads = [q for q in quads if q != (3, 2, 6, 7)]
    P = np.array([[c[a], c[b], c[d]] for (a, b, cc, d) in quads] + [[c[b], c[cc], c[d]] for (a, b, cc, d) in quads], np.float32)
    add_instance(P, face_normals(P), 1, wire.SUBGROUP_NON_EMISSIVE)

    atrium_em = None
    if layout == "atrium":
        groups, atrium_em = _atrium_geometry(num_tris, num_emissive, room, rng)
        for k, P in enumerate(groups):
            add_instance(P, face_normals(P), 2 + k, wire.SUBGROUP_NON_EMISSIVE)
        num_emissive = len(atrium_em)
    # clutter
    per = max(1, num_tris // 8)
    size = np.float32(2.0 * room / max(2.0, (num_tris ** (1.0 / 3.0))))
    for k in range(8 if layout == "soup" else 0):
        ctr = rng.uniform(-0.9 * room, 0.9 * room, (per, 1, 3)).astype(np.float32)
        P = ctr + rng.normal(size=(per, 3, 3)).astype(np.float32) * size
        if k == 0 and per >= 16:
            # coplanar, overlapping, axis-aligned sheets -> exact ties on t for axis-parallel rays
            m = min(per // 2, 64)
            zs = np.float32(0.5)
            for j in range(m):
                P[j] = np.array([[-1, -1, zs], [1, -1, zs], [-1, 1, zs]], np.float32) * np.float32(0.5 + 0.01 * (j % 4))
        add_instance(P, face_normals(P), 2 + k, wire.SUBGROUP_NON_EMISSIVE)

    # emissive triangles
    if num_emissive > 0:
        ctr = rng.uniform(-0.85 * room, 0.85 * room, (num_emissive, 1, 3)).astype(np.float32)
        P = ctr + rng.normal(size=(num_emissive, 3, 3)).astype(np.float32) * (size * np.float32(0.5))
        if atrium_em is not None:
            P = atrium_em
        ei = add_instance(P, face_normals(P), em_mat_idx, wire.SUBGROUP_EMISSIVE)
        insts[ei]["base_emissive_tri_offset"] = 0
        strengths = np.exp(rng.uniform(np.log(0.5), np.log(50.0), num_emissive)).astype(np.float32)
        sh = f32_to_f16_bits(strengths)
        matp = sc.materials[em_mat_idx]
        ems = np.zeros(num_emissive, wire.EMISSIVE_TRI)
        e0, e1 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        l0 = np.sqrt((e0 * e0).sum(1, dtype=np.float32)).astype(np.float32)
        l1 = np.sqrt((e1 * e1).sum(1, dtype=np.float32)).astype(np.float32)
        ems["vtx0"] = P[:, 0]
        ems["v0v1"] = encode_octahedral(e0 / l0[:, None], sse_order=False)
        ems["v0v2"] = encode_octahedral(e1 / l1[:, None], sse_order=False)
        ems["edge_lengths"] = np.stack([f32_to_f16_bits(l0), f32_to_f16_bits(l1)], 1)
        M = 0xFFFFFFFF
        # vectorised PCG3d(geometryIndex = instance index, instanceID = 0, primIdx)
        x = np.full(num_emissive, ei, np.uint64)
        y = np.zeros(num_emissive, np.uint64)
        z = np.arange(num_emissive, dtype=np.uint64)
        x = (x * 1664525 + 1013904223) & M
        y = (y * 1664525 + 1013904223) & M
        z = (z * 1664525 + 1013904223) & M
        x = (x + y * z) & M
        y = (y + z * x) & M
        z = (z + x * y) & M
        x ^= x >> np.uint64(16)
        y ^= y >> np.uint64(16)
        z ^= z >> np.uint64(16)
        x = (x + y * z) & M
        ems["id"] = x.astype(np.uint32)
        fac = int(matp["emissive_factor_normal_scale"]) & 0xFFFFFF
        ems["packed_a"] = (fac | (1 << 24) | (1 << 25)) | ((sh.astype(np.uint32) & 0xF) << 28)
        ems["packed_b"] = 0xFFFF | (sh.astype(np.uint32) << 16)
        uvh = f32_to_f16_bits(np.array([[0, 0], [1, 0], [0, 1]], np.float32))
        ems["uv0"], ems["uv1"], ems["uv2"] = uvh[0], uvh[1], uvh[2]
        sc.emissives = ems

    sc.vertices = np.concatenate(verts)
    sc.indices = np.concatenate(inds)
    sc.instances = np.array(insts, dtype=wire.MESH_INSTANCE)
    sc.instance_to_world = np.array(xforms, np.float32)
    sc.instance_mask = np.array(masks, np.uint8)
    sc.instance_num_tris = np.array(ntris, np.uint32)
    sc.rho, sc.rho_dim = load_rho_default()
    return sc


def add_test_textures(sc: Scene, seed=7, non_opaque_instance=2):
    """Binds a small procedural texture set to a synthetic scene (tests / benches; not in the reference): two sRGB base
    colour maps (the second with a varying alpha channel), an RG8 normal map, a non-power-of-two RG8 metallic-roughness
    map and an sRGB emissive map.  Heap order [base0, base1, normal0, mr0, emissive0]; returns the four descriptor-table
    offsets to put into the frame constants: dict(base_color=0, normal=2, metallic_roughness=3, emissive=4).
    Material 1 (the room) gets base0 + normal0 + mr0, every third clutter material base1, the emissive material and all
    emissive triangles emissive0; instance `non_opaque_instance` becomes alpha tested (ZR_INSTANCE_NON_OPAQUE, cutoff 0.5)
    against base1.  UVs are scaled so that several mip levels are exercised and per-vertex tangents are filled in."""
    rng = np.random.default_rng(seed)
    def smooth(h, w, c):
        a = rng.uniform(0, 1, (h // 4 + 1, w // 4 + 1, c))
        a = np.kron(a, np.ones((4, 4, 1)))[:h, :w]
        a = 0.75 * a + 0.25 * rng.uniform(0, 1, (h, w, c))
        return np.clip(np.rint(a * 255), 0, 255).astype(np.uint8)
    base0 = smooth(32, 64, 4); base0[..., 3] = 255
    base1 = smooth(32, 32, 4)
    yy, xx = np.mgrid[0:32, 0:32]
    base1[..., 3] = np.where(((xx // 4) + (yy // 4)) % 2 == 0, 255, rng.integers(0, 120, (32, 32))).astype(np.uint8)
    nrm = np.clip(128 + rng.normal(0, 30, (32, 32, 2)), 0, 255).astype(np.uint8)
    mr = smooth(12, 24, 2)
    em = smooth(8, 8, 4)
    t_base0 = sc.add_texture(base0, wire.TEX_RGBA8_SRGB)
    t_base1 = sc.add_texture(base1, wire.TEX_RGBA8_SRGB)
    t_nrm = sc.add_texture(nrm, wire.TEX_RG8)
    t_mr = sc.add_texture(mr, wire.TEX_RG8)
    t_em = sc.add_texture(em, wire.TEX_RGBA8_SRGB)
    offs = dict(base_color=t_base0, normal=t_nrm, metallic_roughness=t_mr, emissive=t_em)

    mats = sc.materials.copy()
    def set_tex(i, field, tex):
        mats[field][i] = (int(mats[field][i]) & 0xFFFF0000) | tex
    set_tex(1, "base_color_tex_subsurf_coat_weight", 0)
    set_tex(1, "normal_tex_tr_depth", 0)
    set_tex(1, "mr_tex_spec_roughness_coat_roughness", 0)
    mats["emissive_factor_normal_scale"][1] = (int(mats["emissive_factor_normal_scale"][1]) & 0x00FFFFFF) | (200 << 24)   # normal scale
    for i in range(2, len(mats) - 1, 3):
        set_tex(i, "base_color_tex_subsurf_coat_weight", 1)
    set_tex(len(mats) - 1, "emissive_tex_alpha_cutoff_coat_ior", 0)
    sc.materials = mats
    if len(sc.emissives):
        ems = sc.emissives.copy()
        ems["packed_b"] = (ems["packed_b"] & np.uint32(0xFFFF0000)) | np.uint32(0)
        sc.emissives = ems
    inst = sc.instances.copy()
    masks = sc.instance_mask.copy()
    k = non_opaque_instance
    if k is not None and k < len(inst):
        inst["base_color_tex"][k] = 1
        inst["alpha_factor_cutoff"][k] = 255 | (128 << 8)
        masks[k] |= wire.INSTANCE_NON_OPAQUE
    sc.instances, sc.instance_mask = inst, masks
    # UV scale per instance + tangents (non-indexed synthetic meshes: 3 vertices per triangle)
    v = sc.vertices.copy()
    for i in range(len(inst)):
        b, n = int(inst["base_vtx_offset"][i]), int(sc.instance_num_tris[i]) * 3
        v["uv"][b:b + n] *= np.float32(6.0 if i == 0 else 1.5)
        P = v["pos"][b:b + n].reshape(-1, 3, 3)
        t = P[:, 1] - P[:, 0]
        t = t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-20)
        v["tangent"][b:b + n] = encode_octahedral(np.repeat(t.astype(np.float32), 3, axis=0), sse_order=False)
    sc.vertices = v
    return offs


def set_texture_heap_offsets(cb, offs):
    """Writes add_test_textures' table offsets into frame constants (FrameConstants.h:31-34)."""
    cb["base_color_maps_desc_heap_offset"] = offs["base_color"]
    cb["normal_maps_desc_heap_offset"] = offs["normal"]
    cb["metallic_roughness_maps_desc_heap_offset"] = offs["metallic_roughness"]
    cb["emissive_maps_desc_heap_offset"] = offs["emissive"]
    return cb


def move_instance(sc: Scene, idx, translation=None, rotation=None, scale=None, xform_of=None):
    """Next frame of an animated scene, in place: instance `idx` gets a new TRS (glTF-convention-free: already in the renderer's space),
    every instance's Prev* fields take the values it had this frame -- what TLAS::FillMeshInstanceData does per frame
    (RtAccelerationStructure.cpp:318-380: PrevRotation / PrevScale = last frame's, dTranslation = half(T - T_prev)).
    `xform_of[i]` remembers the unquantised (t, q, s) of instance i between calls.  Returns (instances, instance_to_world)."""
    if xform_of is None:
        xform_of = {}
    inst = sc.instances
    old_t = inst["translation"].copy()
    inst["prev_rotation"] = inst["rotation"]
    inst["prev_scale"] = inst["scale"]
    inst["d_translation"] = 0            # half +0.0
    if translation is not None or rotation is not None or scale is not None:
        if idx not in xform_of:      # start from the instance's own (quantised) rotation and scale
            q_init = inst["rotation"][idx].astype(np.float32) / np.float32(65535.0) * np.float32(2.0) - np.float32(1.0)
            s_init = inst["scale"][idx].view(np.float16).astype(np.float32)
            xform_of[idx] = (inst["translation"][idx].copy(), q_init, s_init)
        t0, q0, s0 = xform_of[idx]
        t = np.asarray(translation if translation is not None else t0, np.float32)
        q = np.asarray(rotation if rotation is not None else q0, np.float32)
        q = q / np.float32(np.sqrt(np.float32(np.dot(q, q))))
        s = np.asarray(scale if scale is not None else s0, np.float32)
        xform_of[idx] = (t, q, s)
        inst["rotation"][idx] = np.rint((q * np.float32(0.5) + np.float32(0.5)) * np.float32(65535.0)).astype(np.uint16)
        inst["scale"][idx] = f32_to_f16_bits(s)
        inst["translation"][idx] = t
        inst["d_translation"][idx] = f32_to_f16_bits(t - old_t[idx])
        sc.instance_to_world[idx] = trs_matrix(t, q, s).astype(np.float32).reshape(12)
    return sc.instances, sc.instance_to_world
