// zr_pose.h -- what zr_scene_animate poses each frame, stated once for zr_api.hip (which lays it out) and zr_tu_pose.hip (which launches it): the vertex
// ranges of the skin set (zr_scene_set_skinning) and of the morph set (zr_scene_set_morph) as ONE list, with ONE buffer of rest records behind it.
#ifndef ZR_POSE_H
#define ZR_POSE_H

#include <hip/hip_runtime.h>
#include "../../include/zr_skin.h"
#include "../../include/zr_morph.h"
#include "zr_hit_tables.h"

namespace zr {

// a range's kind: which set lists it.  A range both list (the two are then equal, zrmo::ValidateMorph) is ONE range of kind kPoseSkin | kPoseMorph
enum : uint32_t { kPoseSkin = 1, kPoseMorph = 2 };
// vertices [firstVertex, firstVertex + numVertices), never empty and never overlapping another range's.  restFirst: where its rest records start in the
// rest buffer.  kPoseSkin: influence record firstInfluence + i belongs to vertex i.  kPoseMorph: its numTargets target records start at firstTarget, its
// track's weights at weightFirst of the weight array.  The fields of a set that does not list the range are 0
struct PoseRange { uint32_t firstVertex, numVertices, restFirst, firstInfluence, firstTarget, numTargets, weightFirst, kind; };

// the device tables of a frame; the half of a set that is absent is null / 0
struct PoseTables
{
    // skin: J = nodeWorld[jointNode[j]] x inverseBind[j], written by the frame's k_skin_joints; nodeWorld: the animation's node matrices
    float* J; const float* nodeWorld; const uint32_t* jointNode; const float* inverseBind; uint32_t numJoints; const zr_skin_influence* influences;
    // morph: weights, written by the frame's k_morph_weights track after track; trackOfWeight / weightFirst: each weight's track, each track's first weight
    float* weights; uint32_t numWeights; const zr_morph_track* tracks; const uint32_t* trackOfWeight; const uint32_t* weightFirst;
    const float* times; const float* values; const float* restWeights; const zr_morph_target* targets; const float* deltas;
    const zr_vertex* rest;
};

// zr_tu_pose.hip.  On `st`, behind the launches that write nodeWorld: k_skin_joints (with joints), k_morph_weights (with weights), then one
// k_pose_vertices launch per range in list order.  tangents: null without ZR_HIT_TANGENTS
hipError_t LaunchPose(hipStream_t st, float t, const PoseTables& T, const PoseRange* ranges, uint32_t numRanges, zr_vertex* vertices, VtxDir* normals, VtxDir* tangents);

// ---- deformed lights: a light triangle with a vertex in one of the ranges, as the host lists it when the range list is made (ScenePoseRebuild): the
// triangle's index among the scene's light triangles and its three ABSOLUTE vertex indices -- instance -> index -> vertex resolved once, so the frame's
// kernel does one 16-byte load and three gathers
struct LightEntry { uint32_t tri, v0, v1, v2; };
static_assert(sizeof(LightEntry) == 16, "LightEntry travels as one 16-byte word");
// zr_tu_scene_update.hip: k_refresh_emissives, zrsm::EmissiveFromVertices per light triangle -- object[k] and emissives[k] from the vertex buffer and the
// owner's row of toWorld as they stand on `st`.  list != null: the LISTED form over list[0 .. count).  list == null: the RANGE form over light triangles
// [first, first + count), indices from the owner's record and the index buffer; a triangle without an owner is skipped.  A triangle whose indices reach
// past numIndices / numVertices is skipped too (nothing is read or written out of bounds)
struct RefreshBuffers
{
    zr_emissive_triangle* emissives; zr_emissive_triangle* object; const uint32_t* owner; const float* toWorld; const zr_vertex* vertices; uint32_t numVertices;
    const zr_mesh_instance* instances; const uint32_t* indices; uint32_t numIndices;
};
hipError_t LaunchRefreshEmissives(hipStream_t st, const RefreshBuffers& B, const LightEntry* list, uint32_t first, uint32_t count);

} // namespace zr

#endif // ZR_POSE_H
