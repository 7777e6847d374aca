// TEST-ONLY: include/zr_morph.h compiled for the host on its own, so that tests/test_morph_cpu.py can hold the header's functions -- the ones the device
// kernels of zr_tu_pose.hip compile -- against a float64 restatement, and tests/test_morph_gpu.py can pose vertices for the host form.
#include "../../include/zr_morph.h"

extern "C" {

void zmo_sample_weights(const float* times, const float* values, uint32_t numKeys, uint32_t numTargets, float t0, uint32_t loop, float t, float* out)
{ zrmo::SampleWeights(times, values, numKeys, numTargets, t0, loop, t, out); }
// translation.x of zran::SampleAnimation over keys[0 .. numKeys): what SampleWeights' flow is pinned to
float zmo_sample_animation_tx(const zr_keyframe* keys, uint32_t numKeys, float t0, uint32_t loop, float t)
{ zran::Srt r; zran::SampleAnimation(keys, numKeys, t0, loop, t, r); return r.t[0]; }
// n vertices of one range: vertex i reads triple first_* + i of every target
void zmo_morph_vertices(const zr_vertex* rest, const zr_morph_target* targets, uint32_t numTargets, const float* weights, const float* deltas, zr_vertex* out, uint32_t n)
{ for (uint32_t i = 0; i < n; i++) zrmo::MorphVertex(rest[i], targets, numTargets, weights, deltas, i, out[i]); }
uint32_t zmo_num_weights(const zr_morph_desc* d) { std::vector<uint32_t> offs(d->num_tracks); return zrmo::WeightOffsets(*d, offs.data()); }
void zmo_eval_weights(const zr_morph_desc* d, float t, float* W) { zrmo::EvalWeights(*d, t, W); }
void zmo_morph_ranges(const zr_morph_desc* d, const float* W, const zr_skin_desc* skin, const float* J, const zr_vertex* rest, zr_vertex* out) { zrmo::MorphRanges(*d, W, skin, J, rest, out); }
int zmo_validate(const zr_morph_desc* d, const zr_skin_desc* skin, uint32_t sceneVertices, char* msg, uint32_t cap) { return zrmo::ValidateMorph(*d, skin, sceneVertices, msg, cap); }

}
