// TEST-ONLY: include/zr_anim.h compiled for the host on its own, so that tests/test_anim_cpu.py can hold the header's functions -- the ones the device
// kernels of zr_tu_anim.hip compile -- against the reference's recorded slerp, float64, and the host library (zrh_*, zetaray_amd/host/zr_scene_io.cpp).
#include "../../include/zr_anim.h"

extern "C" {

// returns the near-zero flag per case
void zan_slerp(const float* q1, const float* q2, const float* t, float* out, uint8_t* nearZero, uint32_t n)
{ for (uint32_t i = 0; i < n; i++) nearZero[i] = (uint8_t)zran::Slerp(q1 + 4 * i, q2 + 4 * i, t[i], out + 4 * i); }
float zan_acos(float x) { return zran::Acos(x); }
float zan_sin(float x) { return zran::Sin(x); }
// srt10: scale[3] rotation[4] translation[3]
static void Store(const zran::Srt& r, float* srt10) { for (int k = 0; k < 3; k++) { srt10[k] = r.s[k]; srt10[7 + k] = r.t[k]; } for (int k = 0; k < 4; k++) srt10[3 + k] = r.q[k]; }
void zan_interpolate(const zr_keyframe* k1, const zr_keyframe* k2, float interpolatedT, float* srt10) { zran::Srt r; zran::Interpolate(*k1, *k2, interpolatedT, r); Store(r, srt10); }
void zan_sample(const zr_keyframe* keys, uint32_t numKeys, float t0, uint32_t loop, float t, float* srt10) { zran::Srt r; zran::SampleAnimation(keys, numKeys, t0, loop, t, r); Store(r, srt10); }
void zan_local_matrix(const float* srt10, float* out12) { zran::Srt r; for (int k = 0; k < 3; k++) { r.s[k] = srt10[k]; r.t[k] = srt10[7 + k]; } for (int k = 0; k < 4; k++) r.q[k] = srt10[3 + k]; zran::LocalMatrix(r, out12); }
void zan_compose_world(const float* local12, const float* parent12, float* out12) { zran::ComposeWorld(local12, parent12, out12); }
void zan_eval_node_worlds(const zr_anim_desc* d, float t, float* nodeWorld) { zran::EvalNodeWorlds(*d, t, nodeWorld); }
int zan_validate(const zr_anim_desc* d, uint32_t sceneInstances, uint32_t* level, char* msg, uint32_t cap) { return zran::ValidateAnimation(*d, sceneInstances, level, msg, cap); }

}
