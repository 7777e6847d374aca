// TEST-ONLY: include/zr_skin.h compiled for the host on its own, so that tests/test_skin_cpu.py can hold the header's functions -- the ones the device
// kernels of zr_tu_pose.hip compile -- against a float64 restatement stage by stage, and tests/test_skin_gpu.py can pose vertices for the host form.
#include "../../include/zr_skin.h"

extern "C" {

void zsk_joint_matrix(const float* nodeWorld, const float* inverseBind, float* J, uint32_t n)
{ for (uint32_t i = 0; i < n; i++) zrsk::JointMatrix(nodeWorld + 12 * (size_t)i, inverseBind + 12 * (size_t)i, J + 12 * (size_t)i); }
// J4: n x 4 x 12, w: n x 4, M: n x 12
void zsk_blend(const float* J4, const float* w, float* M, uint32_t n)
{ for (uint32_t i = 0; i < n; i++) { const float* J = J4 + 48 * (size_t)i; zrsk::Blend(J, J + 12, J + 24, J + 36, w + 4 * (size_t)i, M + 12 * (size_t)i); } }
void zsk_position(const float* M, const float* p, float* out, uint32_t n) { for (uint32_t i = 0; i < n; i++) zrsm::MulPoint(M + 12 * (size_t)i, p + 3 * (size_t)i, out + 3 * (size_t)i); }
void zsk_decode(const uint16_t* codes, float* out, uint32_t n) { for (uint32_t i = 0; i < n; i++) zrsk::DecodeOct32(codes + 2 * (size_t)i, out + 3 * (size_t)i); }
void zsk_encode(const float* dirs, uint16_t* codes, uint32_t n) { for (uint32_t i = 0; i < n; i++) zrsm::EncodeOct32(dirs + 3 * (size_t)i, codes + 2 * (size_t)i); }
void zsk_normal(const float* M, const float* nrm, float* out, uint32_t n) { for (uint32_t i = 0; i < n; i++) zrsk::Normal(M + 12 * (size_t)i, nrm + 3 * (size_t)i, out + 3 * (size_t)i); }
void zsk_tangent(const float* M, const float* t, float* out, uint32_t n) { for (uint32_t i = 0; i < n; i++) zrsk::Tangent(M + 12 * (size_t)i, t + 3 * (size_t)i, out + 3 * (size_t)i); }
void zsk_pose_vertex(const zr_vertex* rest, const float* M, zr_vertex* out, uint32_t n) { for (uint32_t i = 0; i < n; i++) zrsk::PoseVertex(rest[i], M + 12 * (size_t)i, out[i]); }
void zsk_eval_joint_matrices(const zr_skin_desc* d, const float* nodeWorld, float* J) { zrsk::EvalJointMatrices(*d, nodeWorld, J); }
void zsk_skin_ranges(const zr_skin_desc* d, const float* J, const zr_vertex* rest, zr_vertex* out) { zrsk::SkinRanges(*d, J, rest, out); }
int zsk_validate(const zr_skin_desc* d, uint32_t animNodes, uint32_t sceneVertices, char* msg, uint32_t cap) { return zrsk::ValidateSkin(*d, animNodes, sceneVertices, msg, cap); }

}
