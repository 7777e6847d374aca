// zr_tu_scene_update.hip -- the device form of a frame's scene update (zr_scene_move_instances, include/zetaray_amd.h): the MeshInstance records
// and the EmissiveTriangle records of the instances that moved, computed on the device from their new world matrices by the same functions the
// host form compiles (include/zr_scene_math.h), byte for byte.  Two per-element streams bound by HBM and launch latency: no LDS (`make resources` reports 0 bytes for each kernel), no wave operations.
// k_refresh_emissives: the records of light triangles whose VERTICES changed (pose sets, zr_scene_refresh_emissives), by the same header.
#include <hip/hip_runtime.h>
#include <cstddef>
#include "../../include/zr_scene_math.h"
#include "zr_hit_tables.h"
#include "zr_pose.h"

namespace zr {

static constexpr uint32_t kNone = 0xffffffffu;      // slot of an instance that did not move / owner of a triangle no instance carries
static constexpr uint32_t kBlock = 256;

// records travel as 16-byte words (64 B MeshInstance, 48 B EmissiveTriangle: both 16-byte aligned in a hipMalloc'ed array)
template<typename T> __device__ inline T LoadRecord(const T* p)
{
    static_assert(sizeof(T) % 16 == 0, "record size");
    uint4 w[sizeof(T) / 16];
    ZR_UNROLL
    for (uint32_t k = 0; k < sizeof(T) / 16; k++) w[k] = reinterpret_cast<const uint4*>(p)[k];
    T t; __builtin_memcpy(&t, w, sizeof(T));
    return t;
}
template<typename T> __device__ inline void StoreRecord(T* p, const T& v)
{
    uint4 w[sizeof(T) / 16]; __builtin_memcpy(w, &v, sizeof(T));
    ZR_UNROLL
    for (uint32_t k = 0; k < sizeof(T) / 16; k++) reinterpret_cast<uint4*>(p)[k] = w[k];
}
// the MeshInstance record field by field from its four 16-byte words and back: a byte copy between the words and the struct leaves the compiler a 6-byte
// private array (a uint16[3] field it carries through unchanged), which it parks in LDS
static_assert(sizeof(zr_mesh_instance) == 64 && offsetof(zr_mesh_instance, rotation) == 8 && offsetof(zr_mesh_instance, scale) == 16 &&
    offsetof(zr_mesh_instance, mat_idx) == 22 && offsetof(zr_mesh_instance, base_emissive_tri_offset) == 24 && offsetof(zr_mesh_instance, translation) == 28 &&
    offsetof(zr_mesh_instance, prev_rotation) == 40 && offsetof(zr_mesh_instance, prev_scale) == 48 && offsetof(zr_mesh_instance, d_translation) == 54 &&
    offsetof(zr_mesh_instance, base_color_tex) == 60 && offsetof(zr_mesh_instance, alpha_factor_cutoff) == 62, "MeshInstance layout");
__device__ inline uint16_t Lo16(uint32_t w) { return (uint16_t)(w & 0xffffu); }
__device__ inline uint16_t Hi16(uint32_t w) { return (uint16_t)(w >> 16); }
__device__ inline uint32_t Pack16(uint16_t lo, uint16_t hi) { return (uint32_t)lo | ((uint32_t)hi << 16); }
__device__ inline zr_mesh_instance LoadInstance(const zr_mesh_instance* p)
{
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1], c = reinterpret_cast<const uint4*>(p)[2], d = reinterpret_cast<const uint4*>(p)[3];
    zr_mesh_instance I;
    I.base_vtx_offset = a.x; I.base_idx_offset = a.y;
    I.rotation[0] = Lo16(a.z); I.rotation[1] = Hi16(a.z); I.rotation[2] = Lo16(a.w); I.rotation[3] = Hi16(a.w);
    I.scale[0] = Lo16(b.x); I.scale[1] = Hi16(b.x); I.scale[2] = Lo16(b.y); I.mat_idx = Hi16(b.y);
    I.base_emissive_tri_offset = b.z;
    I.translation[0] = zr_asfloat(b.w); I.translation[1] = zr_asfloat(c.x); I.translation[2] = zr_asfloat(c.y);
    I.prev_rotation[0] = Lo16(c.z); I.prev_rotation[1] = Hi16(c.z); I.prev_rotation[2] = Lo16(c.w); I.prev_rotation[3] = Hi16(c.w);
    I.prev_scale[0] = Lo16(d.x); I.prev_scale[1] = Hi16(d.x); I.prev_scale[2] = Lo16(d.y);
    I.d_translation[0] = Hi16(d.y); I.d_translation[1] = Lo16(d.z); I.d_translation[2] = Hi16(d.z);
    I.base_color_tex = Lo16(d.w); I.alpha_factor_cutoff = Hi16(d.w);
    return I;
}
__device__ inline void StoreInstance(zr_mesh_instance* p, const zr_mesh_instance& I)
{
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(I.base_vtx_offset, I.base_idx_offset, Pack16(I.rotation[0], I.rotation[1]), Pack16(I.rotation[2], I.rotation[3]));
    q[1] = make_uint4(Pack16(I.scale[0], I.scale[1]), Pack16(I.scale[2], I.mat_idx), I.base_emissive_tri_offset, zr_asuint(I.translation[0]));
    q[2] = make_uint4(zr_asuint(I.translation[1]), zr_asuint(I.translation[2]), Pack16(I.prev_rotation[0], I.prev_rotation[1]), Pack16(I.prev_rotation[2], I.prev_rotation[3]));
    q[3] = make_uint4(Pack16(I.prev_scale[0], I.prev_scale[1]), Pack16(I.prev_scale[2], I.d_translation[0]), Pack16(I.d_translation[1], I.d_translation[2]),
        Pack16(I.base_color_tex, I.alpha_factor_cutoff));
}
__device__ inline void LoadMatrix(const float* p, float M[12])
{
    ZR_UNROLL
    for (int k = 0; k < 3; k++) { const float4 r = reinterpret_cast<const float4*>(p)[k]; M[4 * k] = r.x; M[4 * k + 1] = r.y; M[4 * k + 2] = r.z; M[4 * k + 3] = r.w; }
}

// slot[i] = position of instance i in the frame's moved list; every other entry holds kNone (k_move_instances puts it back)
__global__ void __launch_bounds__(kBlock) k_mark_moved(uint32_t* slot, const uint32_t* movedIdx, uint32_t nMoved)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j < nMoved) slot[movedIdx[j]] = j;
}

// one lane per light triangle of [first, end): emissives[k] = EmissiveToWorld(object[k], new matrix of the owner) where the owner moved
__global__ void __launch_bounds__(kBlock) k_move_emissives(zr_emissive_triangle* emissives, const zr_emissive_triangle* object, const uint32_t* owner,
    const uint32_t* slot, const float* movedXf, uint32_t first, uint32_t end)
{
    const uint32_t k = first + blockIdx.x * kBlock + threadIdx.x;
    if (k >= end) return;
    const uint32_t o = owner[k];
    if (o == kNone) return;
    const uint32_t j = slot[o];
    if (j == kNone) return;
    float M[12]; LoadMatrix(movedXf + 12 * (size_t)j, M);
    const zr_emissive_triangle in = LoadRecord(object + k);
    zr_emissive_triangle out;
    zrsm::EmissiveToWorld(in, M, out);
    StoreRecord(emissives + k, out);
}

// one lane per light triangle whose vertices were deformed: object[k] and emissives[k] = EmissiveFromVertices(object[k], the triangle's three positions in
// the vertex buffer, the owner's row of toWorld) -- behind k_move_instances of the same frame, so the row is this frame's whether the owner moved or not.
// kListed: entry j of `list` names the triangle and its absolute vertex indices.  Else: triangle first + j, indices from the owner's record (first light
// triangle, index and vertex offsets: words 0, 1 and 6 of the 64-byte record) and the index buffer.  The loads that do not depend on each other (entry ->
// owner -> matrix; entry -> three positions; entry -> record) are issued together; no LDS, no wave operations
template<bool kListed>
__global__ void __launch_bounds__(kBlock) k_refresh_emissives(RefreshBuffers B, const LightEntry* list, uint32_t first, uint32_t count)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= count) return;
    uint32_t k, v[3];
    uint32_t o;
    if constexpr (kListed)
    {
        const uint4 e = *reinterpret_cast<const uint4*>(list + j);
        k = e.x; v[0] = e.y; v[1] = e.z; v[2] = e.w;
        o = B.owner[k];
        if (o == kNone) return;
    }
    else
    {
        k = first + j;
        o = B.owner[k];
        if (o == kNone) return;
        const uint4 a = reinterpret_cast<const uint4*>(B.instances + o)[0], b = reinterpret_cast<const uint4*>(B.instances + o)[1];
        const uint64_t i = (uint64_t)a.y + 3ull * (k - b.z);      // a.x base_vtx_offset, a.y base_idx_offset, b.z base_emissive_tri_offset
        if (i + 3 > B.numIndices) return;
        ZR_UNROLL
        for (int c = 0; c < 3; c++) v[c] = a.x + B.indices[i + c];
    }
    if (v[0] >= B.numVertices || v[1] >= B.numVertices || v[2] >= B.numVertices) return;
    float p[3][3];
    ZR_UNROLL
    for (int c = 0; c < 3; c++) { ZR_UNROLL for (int r = 0; r < 3; r++) p[c][r] = B.vertices[v[c]].pos[r]; }
    float M[12]; LoadMatrix(B.toWorld + 12 * (size_t)o, M);
    const zr_emissive_triangle rec = LoadRecord(B.object + k);
    zr_emissive_triangle obj, world;
    zrsm::EmissiveFromVertices(rec, p[0], p[1], p[2], M, obj, world);
    StoreRecord(B.object + k, obj);
    StoreRecord(B.emissives + k, world);
}
hipError_t LaunchRefreshEmissives(hipStream_t st, const RefreshBuffers& B, const LightEntry* list, uint32_t first, uint32_t count)
{
    if (!count) return hipSuccess;
    const dim3 grid((count + kBlock - 1) / kBlock), block(kBlock);
    if (list) hipLaunchKernelGGL(k_refresh_emissives<true>, grid, block, 0, st, B, list, 0u, count);
    else hipLaunchKernelGGL(k_refresh_emissives<false>, grid, block, 0, st, B, nullptr, first, count);
    return hipGetLastError();
}

// one lane per instance: the record of the buffer that becomes previous -> the begin-frame rule -> (moved: the set_instance_world rule from the new
// matrix and the matrix the instance had, whose row of toWorld is replaced) -> the buffer that becomes current
__global__ void __launch_bounds__(kBlock) k_move_instances(zr_mesh_instance* cur, const zr_mesh_instance* prev, float* toWorld, uint32_t* slot,
    const float* movedXf, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    zr_mesh_instance I = LoadInstance(prev + i);
    const uint32_t j = slot[i];
    if (j == kNone) zrsm::InstanceBeginFrame(I);
    else
    {   // (the set-world rule writes every field the begin-frame rule does)
        float M[12], P[12];
        LoadMatrix(movedXf + 12 * (size_t)j, M); LoadMatrix(toWorld + 12 * (size_t)i, P);
        zrsm::InstanceSetWorld(I, M, P);
        ZR_UNROLL
        for (int k = 0; k < 3; k++) reinterpret_cast<float4*>(toWorld + 12 * (size_t)i)[k] = make_float4(M[4 * k], M[4 * k + 1], M[4 * k + 2], M[4 * k + 3]);
        slot[i] = kNone;
    }
    StoreInstance(cur + i, I);
}

// ---- the tables of zr_hit_tables.h: what hit reconstruction decodes from an instance record / a vertex, stored once.  MakeInstRec and DecodeOct32 are
// the inline functions the per-hit code calls, compiled with the library's flags, so the stored bits are the bits a hit would compute
// one lane per instance
__global__ void __launch_bounds__(kBlock) k_fill_inst_recs(InstRec* recs, const zr_mesh_instance* instances, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const zr_mesh_instance I = LoadInstance(instances + i);
    StoreRecord(recs + i, MakeInstRec(I));
}
// one lane per vertex; tangent: decode vertex.tangent instead of vertex.normal (-DZR_HIT_TANGENTS builds)
__global__ void __launch_bounds__(kBlock) k_fill_vtx_normals(VtxDir* out, const zr_vertex* vertices, uint32_t n, bool tangent)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t w = *reinterpret_cast<const uint32_t*>(tangent ? vertices[i].tangent : vertices[i].normal);      // (4-byte aligned: offsets 20 / 24 of a 28-byte record)
    const uint16_t e[2] = { Lo16(w), Hi16(w) };
    const V3 d = DecodeOct32(e);
    VtxDir r; r.x = d.x; r.y = d.y; r.z = d.z; r.w = 0.0f;
    out[i] = r;
}
hipError_t LaunchFillInstRecs(hipStream_t st, InstRec* recs, const zr_mesh_instance* instances, uint32_t n)
{
    if (n) hipLaunchKernelGGL(k_fill_inst_recs, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, recs, instances, n);
    return hipGetLastError();
}
hipError_t LaunchFillVtxNormals(hipStream_t st, VtxDir* out, const zr_vertex* vertices, uint32_t n, bool tangent)
{
    if (n) hipLaunchKernelGGL(k_fill_vtx_normals, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, out, vertices, n, tangent);
    return hipGetLastError();
}

// moved: [nMoved x 12 floats | nMoved instance indices] in device memory, every index < n and listed once (checked by the caller);
// [emFirst, emEnd) within the scene's light triangles, empty when no moved instance carries lights
hipError_t LaunchMoveInstances(hipStream_t st, zr_mesh_instance* cur, const zr_mesh_instance* prev, float* toWorld, uint32_t n, uint32_t* slot,
    const uint32_t* moved, uint32_t nMoved, zr_emissive_triangle* emissives, const zr_emissive_triangle* object, const uint32_t* owner, uint32_t emFirst, uint32_t emEnd)
{
    const float* movedXf = reinterpret_cast<const float*>(moved);
    const uint32_t* movedIdx = moved + 12 * (size_t)nMoved;
    if (nMoved) hipLaunchKernelGGL(k_mark_moved, dim3((nMoved + kBlock - 1) / kBlock), dim3(kBlock), 0, st, slot, movedIdx, nMoved);
    if (emEnd > emFirst)
        hipLaunchKernelGGL(k_move_emissives, dim3((emEnd - emFirst + kBlock - 1) / kBlock), dim3(kBlock), 0, st, emissives, object, owner, slot, movedXf, emFirst, emEnd);
    if (n) hipLaunchKernelGGL(k_move_instances, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, cur, prev, toWorld, slot, movedXf, n);
    return hipGetLastError();
}

} // namespace zr
