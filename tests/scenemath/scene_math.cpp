// TEST-ONLY: include/zr_scene_math.h compiled for the host on its own, so that tests/test_scene_math_cpu.py can hold the header's functions -- the
// ones the device kernels of zr_tu_scene_update.hip compile -- against the host library (zrh_*, zetaray_amd/host/zr_scene_io.cpp) and the reference.
#include "../../include/zr_scene_math.h"

extern "C" {

void zsm_decompose_srt(const float* M, float* s, float* q, float* t) { zrsm::DecomposeSRT(zrsm::FromToWorld(M), s, q, t); }
void zsm_fill_mesh_instance(const float* M, zr_mesh_instance* I) { zrsm::FillMeshInstance(M, *I); }
void zsm_unorm16(const float* v, uint16_t* out, uint32_t n) { for (uint32_t i = 0; i < n; i++) out[i] = zrsm::Unorm16FromNormalized(v[i]); }
void zsm_emissive_to_world(const zr_emissive_triangle* in, const float* M, zr_emissive_triangle* out) { zr_emissive_triangle t; zrsm::EmissiveToWorld(*in, M, t); *out = t; }
void zsm_decode_emissive_vertices(const zr_emissive_triangle* e, float* v9) { zrsm::DecodeEmissiveVertices(*e, v9, v9 + 3, v9 + 6); }
void zsm_mul_point(const float* M, const float* v, float* out) { zrsm::MulPoint(M, v, out); }
// what k_move_instances does to one record: the begin-frame rule, then (moved) the set_instance_world rule
void zsm_move_instance(zr_mesh_instance* I, const float* world_or_null, const float* prevWorld)
{
    zrsm::InstanceBeginFrame(*I);
    if (world_or_null) zrsm::InstanceSetWorld(*I, world_or_null, prevWorld);
}

}
