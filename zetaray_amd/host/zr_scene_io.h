// zr_scene_io.h -- scene ingestion on the host, in C++: glTF 2.0 -> the wire formats of include/zr_wire.h.
//
// Mirrors the caller side of the hot path in the reference:
//   Source/ZetaCore/Model/glTF.cpp:270-431   mesh primitives: positions / normals / tangents / UVs, RH -> LH (z flip, winding swap)
//   Source/ZetaCore/Model/glTF.cpp:523-643   materials (pbrMetallicRoughness + KHR_materials_emissive_strength / ior / transmission / clearcoat)
//   Source/ZetaCore/Model/glTF.cpp:692-767   emissive instances and triangles (RT::EmissiveTriangle, RtCommon.h:73-190)
//   Source/ZetaCore/Scene/SceneCore.cpp:196-236, 860-900   emissive triangle IDs (PCG3d hash), world = local x parent
//   Source/ZetaCore/RayTracing/RtAccelerationStructure.cpp:318-380   MeshInstance quantisation: decomposeSRT (Math/MatrixFuncs.h:562-610) of
//       the world matrix -> unorm4 rotation, half3 scale, float3 translation
//   Assets.cpp / Tools/BCnCompressglTF       DDS material textures; here BC7 / BC5 / RGBA8 DDS files are decoded once at load to the texel
//       heap of zr_scene_desc (zr_wire.h: the ABI takes decoded texels and defines the filtering), by include/zr_bcn.h -- or kept as blocks
//       for zr_scene_create_compressed, which runs the same header on the device (ZRH_LOAD_KEEP_COMPRESSED)
// No HIP dependency: the library loads on machines without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/zr_wire.h"
#include "../../include/zetaray_amd.h"      // zr_texture_source / zr_texture_blocks (declarations only: this library links no HIP)

extern "C" {
typedef struct zrh_scene_data zrh_scene_data;      // owns every array its zr_scene_desc points to

// Loads <path>.gltf (+ its external .bin buffers and .dds images).  rho_lut / rho_dim: the GGX reflectance LUT to attach (Assets/LUT/rho.dds
// payload; copied).  Returns 0 and a handle, or -1 (zrh_scene_io_last_error()).
int zrh_gltf_load(const char* path, const uint16_t* rho_lut, const uint32_t* rho_dim3, zrh_scene_data** out);
// ... with flags.  ZRH_LOAD_KEEP_COMPRESSED: the .dds payloads are not decoded.  A BC7 file bound as a base colour / emissive map and a BC5 file bound
// as a normal / metallic-roughness map keep their blocks (the whole mip chain as the file stores it, copied 16-byte aligned into one payload); any other
// file is decoded as in the default mode and carried as a RAW chain.  zr_scene_desc.texels is then null and texel_bytes the size of the heap the chains
// decode to -- the desc zr_scene_create_compressed takes together with zrh_scene_data_texture_blocks (null in the default mode, and for a file
// without textures, whose desc zr_scene_create takes in either mode).  The zr_texture_desc
// records, and the heap once decoded (include/zr_bcn.h), equal the default mode's in every byte.
// A .png image (what stock glTF files carry; a file may mix .dds and .png) is level 0 alone: RGBA8 in a base colour / emissive slot (RGBA8_SRGB), the
// file's (R, G) in a normal slot and its (B, G) in a metallic-roughness slot (RG8; the reference converter's -swizzle bg), with
// num_mips = 1 + floor(log2(max(w, h))).  The default mode generates the chain here, by include/zr_mipgen.h; ZRH_LOAD_KEEP_COMPRESSED hands level 0 over
// as a ZR_TEX_SRC_RAW_MIP0 source and the same header runs on the device.  .jpg / .jpeg images are refused without ZRH_LOAD_JPEG (below).
// ZRH_LOAD_JPEG: a .jpg / .jpeg image is read wherever a .png is (without the flag it is refused by name, as before): baseline / extended sequential
// Huffman files of 8 bits, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0 (zrh_jpeg_decode below), same slots, same chain.  The default mode decodes it here through
// include/zr_jpeg.h; with ZRH_LOAD_KEEP_COMPRESSED only the entropy decode runs here and the record of quantised coefficients travels as a
// ZR_TEX_SRC_JPEG_COEF source, which the same header turns into level 0 on the device.  A file may mix .dds, .png and .jpg.
// ZRH_LOAD_DEFORMED_LIGHTS: a skinned or morphed primitive may carry an emissive material (without the flag it is refused by name, as before).  Its light
// records come from the rest pose, as for any mesh; zrh_scene_animate (zr_host.h) re-derives them each frame on either of its paths (zrh_scene_data_refresh_emissives
// below; zr_scene_refresh_emissives, include/zetaray_amd.h).  A file without such a primitive loads to the same bytes with and without the flag.
enum { ZRH_LOAD_KEEP_COMPRESSED = 1u, ZRH_LOAD_JPEG = 2u, ZRH_LOAD_DEFORMED_LIGHTS = 4u };
int zrh_gltf_load_ex(const char* path, const uint16_t* rho_lut, const uint32_t* rho_dim3, uint32_t flags, zrh_scene_data** out);
const zr_texture_blocks* zrh_scene_data_texture_blocks(const zrh_scene_data* s);
const char* zrh_scene_io_last_error(void);
const zr_scene_desc* zrh_scene_data_desc(const zrh_scene_data* s);
// the four descriptor-table offsets for cbFrameConstants (base colour, normal, metallic-roughness, emissive maps) of the scene's texture heap
void zrh_scene_data_tex_offsets(const zrh_scene_data* s, uint32_t* out4);
void zrh_scene_data_destroy(zrh_scene_data* s);

// ---- per-frame maintenance of a loaded scene (SceneCore::Update + TLAS::FillMeshInstanceData for dynamic instances, RtAccelerationStructure.cpp:318-380;
// SceneCore::UpdateEmissivePositions, SceneCore.cpp:913-955).  Per frame: begin_frame (this frame's matrices become the previous ones, every record
// turns static: Prev* = current, dTranslation = 0), set_instance_world for each instance that moves (current + previous S / R / T by decomposeSRT,
// dTranslation = half3(t - t_prev); the EmissiveTriangle records of a light-carrying instance re-derived from the object-space ones), then hand
// zrh_scene_data_desc's instances / instance_to_world and the dirty emissive range to zr_scene_update_emissives / zr_scene_update_instances
// (zrh_scene_apply_updates in zr_host.h does both calls).
void zrh_scene_data_begin_frame(zrh_scene_data* s);
int zrh_scene_data_set_instance_world(zrh_scene_data* s, uint32_t instance, const float* world_3x4);
void zrh_scene_data_dirty_emissives(const zrh_scene_data* s, uint32_t* first, uint32_t* count);
// ... or, for the device form of the update (zr_scene_move_instances, include/zetaray_amd.h), which instances set_instance_world named since
// begin_frame -- each once, in the order they were first named -- and their current matrices (n x 12 floats; valid until the next call on `s`).
// zrh_scene_data_set_device_records(s, 1) makes zrh_scene_apply_updates (zr_host.h) hand over exactly that instead of records.  The host's own
// records are maintained either way (set_instance_world still runs the record math: the device form saves the upload, and a caller that wants
// to save the host math too calls zr_scene_move_instances itself and keeps no zrh_scene_data records)
uint32_t zrh_scene_data_moved(const zrh_scene_data* s, const uint32_t** idx, const float** world_3x4);
void zrh_scene_data_set_device_records(zrh_scene_data* s, int on);
int zrh_scene_data_device_records(const zrh_scene_data* s);
// ---- keyframe animation (include/zr_anim.h; zr_keyframe / zr_anim_node / zr_anim_desc: include/zr_wire.h).  set_animation deep-copies `desc` (null or
// empty clears) and refuses what zr_scene_set_animation refuses as invalid (-1, zrh_scene_io_last_error(), nothing changed); zrh_scene_data_animation
// returns the scene's copy, null when there is none.  zrh_scene_data_animate(s, t) is the HOST PATH of a frame's animation: the header on the host for
// time t, then zrh_scene_data_set_instance_world for each listed instance in list order (the caller runs zrh_scene_data_begin_frame first, as for any
// frame) -- the definition zr_scene_animate (zetaray_amd.h) is held to, byte for byte.
int zrh_scene_data_set_animation(zrh_scene_data* s, const zr_anim_desc* desc);
const zr_anim_desc* zrh_scene_data_animation(const zrh_scene_data* s);
int zrh_scene_data_animate(zrh_scene_data* s, float t);
// ---- skinned meshes.  zrh_gltf_load reads "skins", JOINTS_0 (unsigned bytes / shorts) and WEIGHTS_0 (floats, normalised unsigned bytes / shorts;
// renormalised to sum 1 in float32).  A node with a mesh and a skin: every primitive gets a vertex range of its own (a copy: nothing is shared with
// another node that uses the mesh), the instance's world matrix is the identity (glTF ignores a skinned node's own transform) and the instance is not
// listed in the animation.  The joints of a used skin and their ancestors join the dynamic closure; the inverse bind matrices take the node matrices'
// handedness rule.  zrh_scene_data_skinning returns the tables (zr_scene_set_skinning takes them after zr_scene_set_animation), null for a file
// without a skinned node.  Refused by name and reason: a skin whose joints are not nodes of the file (or not in the scene's hierarchy), JOINTS_0
// without WEIGHTS_0 or the other way round, JOINTS_1 / WEIGHTS_1, a joint index >= the skin's joint count, weights without a positive finite sum, a
// skinned primitive with an emissive material (without ZRH_LOAD_DEFORMED_LIGHTS), a skin in a file with no animation
const zr_skin_desc* zrh_scene_data_skinning(const zrh_scene_data* s);
// ... and for a scene that did not come from a file: a deep copy of `desc` (null or empty clears), after zrh_scene_data_set_animation, refused (-1) for what
// zr_scene_set_skinning refuses as invalid; zrh_scene_data_set_animation clears a skin, as zr_scene_set_animation does.
// zrh_scene_data_skin_pose(s, t) is the HOST FORM of a frame's skinning: zrh_skin_pose (below) on this scene's tables and on its vertices, which keep the
// rest pose; returns the posed records of the ranges, range after range (valid until the next call), null without a skin.
// zrh_scene_data_set_device_skinning: which of the two zrh_scene_animate (zr_host.h) takes for the skin: 0 (default) the host form, handed over with
// zr_scene_update_vertices_async; 1 zr_scene_set_skinning once, then the time alone (it takes effect together with zrh_scene_data_set_device_animation)
int zrh_scene_data_set_skinning(zrh_scene_data* s, const zr_skin_desc* desc);
const zr_vertex* zrh_scene_data_skin_pose(zrh_scene_data* s, float t);
void zrh_scene_data_set_device_skinning(zrh_scene_data* s, int on);
int zrh_scene_data_device_skinning(const zrh_scene_data* s);
// ---- morph targets.  zrh_gltf_load reads a primitive's "targets" (POSITION / NORMAL / TANGENT deltas as float VEC3, or as normalised bytes / shorts; dense
// or SPARSE accessors -- sparse.indices / sparse.values over a bufferView or over zeros; z negated like the vertices' z), "weights" of the mesh and of the
// node (the node's override the mesh's) and animation channels with the path "weights" (LINEAR; a SCALAR output of keys x targets).  A node whose
// weights a channel drives: every primitive gets a vertex range of its own (the skin's copy, where the node is skinned too: one range listed in both
// tables), the node joins the dynamic closure even when no transform of it is animated, and zrh_scene_data_morph returns the tables (zr_scene_set_morph
// takes them after zr_scene_set_animation and zr_scene_set_skinning); nodes that share a mesh share its deltas.  Targets WITHOUT a weights channel: the
// default weights are applied once at load by zrmo::MorphVertex (to a copy of the node's own) and no morph set is made for them.
// Refused by name and reason: primitives of one mesh with different target counts, a weights array whose length is not the target count, a target
// accessor shorter than POSITION, a CUBICSPLINE or STEP weights sampler, a weights channel on a node whose mesh has no targets, a sparse index out of
// range, a morphed primitive with an emissive material without ZRH_LOAD_DEFORMED_LIGHTS (a deformed light would keep shining from its rest pose).
// zrh_scene_data_set_morph replaces the tables (a deep copy; null or empty: clears) after the checks of zr_scene_set_morph; zrh_scene_data_set_animation and
// _set_skinning clear them, as the device scene's calls do.  zrh_scene_data_morph_pose(s, t) is the HOST FORM of a frame's morphing: zrh_morph_pose (below)
// on this scene's tables and vertices, which keep the rest pose; returns the posed records of the ranges, range after range (valid until the next call).
// zrh_scene_data_set_device_morph: which of the two zrh_scene_animate (zr_host.h) takes: 0 (default) the host form, 1 zr_scene_set_morph once
const zr_morph_desc* zrh_scene_data_morph(const zrh_scene_data* s);
int zrh_scene_data_set_morph(zrh_scene_data* s, const zr_morph_desc* desc);
const zr_vertex* zrh_scene_data_morph_pose(zrh_scene_data* s, float t);
void zrh_scene_data_set_device_morph(zrh_scene_data* s, int on);
int zrh_scene_data_device_morph(const zrh_scene_data* s);
// which of the two zrh_scene_animate (zr_host.h) takes: 0 (default) the host path above, 1 zr_scene_animate_async
void zrh_scene_data_set_device_animation(zrh_scene_data* s, int on);
int zrh_scene_data_device_animation(const zrh_scene_data* s);
// the per-frame maintenance above for a scene that did not come from zrh_gltf_load: a deep copy of `desc`; object_space_emissives = desc->num_emissives
// object-space light records (null: instances that carry lights keep their records when they move)
int zrh_scene_data_from_desc(const zr_scene_desc* desc, const zr_emissive_triangle* object_space_emissives, zrh_scene_data** out);

// ---- building blocks, exported for the parity pins (tests/test_scene_io.py) ----
// decomposeSRT + quaternionFromRotationMat1 of a 3 x 4 row-major object-to-world matrix (column-vector convention, zr_scene_desc.instance_to_world)
void zrh_decompose_srt(const float* to_world_3x4, float* scale3, float* quat4, float* translation3);
// affineTransformation(s, q, t) x parent (both 3 x 4 row-major, column-vector convention; parent may be null = identity)
void zrh_compose_world(const float* scale3, const float* quat4, const float* translation3, const float* parent_3x4, float* out_3x4);
// the HOST FORM of skinning (include/zr_skin.h; zr_skin_desc: include/zr_wire.h), the definition zr_scene_animate on a scene with a skin set is held to byte
// for byte: the node matrices of `anim` at time t (include/zr_anim.h), the joint matrices, then every listed vertex.  rest / out: the records of the
// ranges, range after range; the caller hands `out` to zr_scene_update_vertices range by range.  -1 (zrh_scene_io_last_error()) for tables
// zr_scene_set_skinning would refuse
int zrh_skin_pose(const zr_anim_desc* anim, const zr_skin_desc* skin, float t, const zr_vertex* rest, zr_vertex* out);
// the HOST FORM of morph targets (include/zr_morph.h; zr_morph_desc: include/zr_wire.h), the definition zr_scene_animate on a scene with a morph set is held
// to byte for byte: rest = the rest-pose records of morph's ranges, range after range; out = the posed ones in the same order, for time t.  The weights are
// sampled, every vertex is morphed, and with `skin` (else null; then anim may be null too) a range that is also a range of the skin goes on through
// zr_skin.h with the node matrices of time t: MorphVertex, then SkinVertex.  Returns -1 with zrh_scene_io_last_error() for tables zr_scene_set_morph would refuse
int zrh_morph_pose(const zr_anim_desc* anim, const zr_skin_desc* skin_or_null, const zr_morph_desc* morph, float t, const zr_vertex* rest, zr_vertex* out);
// TLAS::FillMeshInstanceData for a static instance: rotation / scale / translation (+ prev_* = current, d_translation = 0)
void zrh_fill_mesh_instance(const float* to_world_3x4, zr_mesh_instance* inst);
// RT::EmissiveTriangle(v0, v1, v2, uv0..2, factor RGB8, texture, half strength bits, id, double sided)
void zrh_pack_emissive_triangle(const float* v0, const float* v1, const float* v2, const float* uv6, uint32_t factor_rgb8, uint32_t tex,
                                uint16_t strength_half, uint32_t id, int double_sided, zr_emissive_triangle* out);
// SceneCore's emissive transform (SceneCore.cpp:196-236, UpdateEmissivePositions :913-955): decode the triangle's vertices (16-bit octahedral edge
// directions, half lengths), transform them by the 3 x 4 object-to-world matrix, encode again; every other field is kept.  Per frame, for a moving
// emissive instance: out[t] = zrh_emissive_to_world(initial[t], new matrix) for its triangles, then zr_scene_update_emissives (zetaray_amd.h)
void zrh_emissive_to_world(const zr_emissive_triangle* in, const float* to_world_3x4, zr_emissive_triangle* out);
// A light triangle whose vertices were deformed (zrsm::EmissiveFromVertices, include/zr_scene_math.h -- the rule k_refresh_emissives compiles): the
// object-space record takes the three object-space positions p0..p2 (the loader's geometry step), the world record is zrh_emissive_to_world of that;
// every non-geometric field of `rec` is kept in both.  No identity-matrix shortcut.  Caller guarantee: no zero-length edge
void zrh_emissive_from_vertices(const zr_emissive_triangle* rec, const float* p0, const float* p1, const float* p2, const float* to_world_3x4,
                                zr_emissive_triangle* object_out, zr_emissive_triangle* world_out);
// ... over a scene's light triangles [first_tri, first_tri + count): each from its owner's index and vertex offsets, the scene's indices and `vertices`
// (the scene's WHOLE vertex array with the pose in it; null: the scene's own), with the owner's current matrix.  Writes the world records
// (zr_scene_desc.emissives) AND the object-space records (zrh_scene_data_initial_emissives: a later zrh_scene_data_set_instance_world starts from the
// posed shape), skips a triangle no instance carries, and adds the triangles to the dirty range zrh_scene_data_dirty_emissives reports, so the host-form
// update uploads them.  The HOST FORM zr_scene_refresh_emissives and the pose sets of zr_scene_animate are held to, byte for byte.  -1
// (zrh_scene_io_last_error()) for a range past the scene's emissive triangles or a scene without object-space records
int zrh_scene_data_refresh_emissives(zrh_scene_data* s, const zr_vertex* vertices, uint32_t first_tri, uint32_t count);
// the light triangles with a vertex in a range of the scene's skin or morph tables, ascending (valid until the next call): what zr_scene_set_skinning /
// zr_scene_set_morph list on the device, and what the host path of zrh_scene_animate refreshes
uint32_t zrh_scene_data_pose_lights(zrh_scene_data* s, const uint32_t** tris);
// the object-space records of the scene's emissive triangles as loaded (same order as zr_scene_desc.emissives; ID already hashed)
const zr_emissive_triangle* zrh_scene_data_initial_emissives(const zrh_scene_data* s);
// BC7 / BC5 block decompression: w x h texels (multiples of 4 not required) -> RGBA8 / RG8 rows top-down
int zrh_bc7_decode(const uint8_t* blocks, uint32_t w, uint32_t h, uint8_t* rgba8);
int zrh_bc5_decode(const uint8_t* blocks, uint32_t w, uint32_t h, uint8_t* rg8);
// A PNG file in memory -> *w x *h RGBA8 texels, rows top-down (rgba8 null: the size alone; else capacity >= 4 w h bytes).  Bit depth 8, and 16 keeping
// the high byte; colour types 0, 2, 3 (with tRNS), 4 and 6 (grey becomes r = g = b, a missing alpha 255); the five row filters.  Inflate, Adler-32 and
// CRC-32 are the loader's own: no link dependency.  -1 with a message that starts with `name` (zrh_scene_io_last_error()) for an interlaced file, a bit
// depth below 8, a bad CRC or Adler-32, truncated data, and dimensions outside [1, 65535].
int zrh_png_decode(const char* name, const uint8_t* data, size_t bytes, uint32_t* w, uint32_t* h, uint8_t* rgba8, size_t capacity);
// A JPEG file in memory -> *w x *h RGBA8 texels, rows top-down, alpha 255 (rgba8 null: the size alone; else capacity >= 4 w h bytes): the entropy decode
// of zrh_jpeg_pack, then include/zr_jpeg.h (13-bit integer IDCT, triangle-filter chroma upsampling, 16-bit fixed-point YCbCr -> RGB) -- on files libjpeg
// wrote, libjpeg's bytes.  Reads SOF0 / SOF1 with Huffman coding, 8 bits, 1 or 3 components (4:4:4, 4:2:2, 4:2:0; grey gives r = g = b), one scan, 8- and
// 16-bit DQT, DRI / RSTn; APPn / COM are skipped.  -1 with a message that starts with `name` for progressive, arithmetic-coded, lossless / hierarchical,
// 12-bit, 4-component, Adobe-RGB and multi-scan files, any other sampling, a Huffman code that is not in the table, a coefficient index past 63, a bad or
// missing restart marker, data that ends early, and a header that promises more blocks than the bytes can hold.
int zrh_jpeg_decode(const char* name, const uint8_t* data, size_t bytes, uint32_t* w, uint32_t* h, uint8_t* rgba8, size_t capacity);
// The entropy decode alone: the record of include/zr_jpeg.h (what a ZR_TEX_SRC_JPEG_COEF source names) with channel_map 0 = RGBA8, 1 = RG8 from the
// file's (R, G), 2 = RG8 from its (B, G).  record null: *record_bytes alone (a multiple of 16); else capacity >= *record_bytes.  Refuses what
// zrh_jpeg_decode refuses.
int zrh_jpeg_pack(const char* name, const uint8_t* data, size_t bytes, uint32_t channel_map, uint8_t* record, size_t capacity, size_t* record_bytes);
// A record -> the w x h texels of its channel map (4 or 2 bytes each) on the host, by the header the kernels compile; the record is checked like a
// ZR_TEX_SRC_JPEG_COEF source (zrjp::CheckRecord).  texels null: the size alone
int zrh_jpeg_expand(const uint8_t* record, size_t bytes, uint32_t* w, uint32_t* h, uint8_t* texels, size_t capacity);
// levels 1 .. num_mips - 1 of the n chains `descs` names in `texels`, in place, from their level 0: include/zr_mipgen.h on the host, the bytes
// zr_mipgen_device and zr_scene_create_compressed (ZR_TEX_SRC_RAW_MIP0) produce on the device
int zrh_mip_generate(const zr_texture_desc* descs, uint32_t n, uint8_t* texels);
}
