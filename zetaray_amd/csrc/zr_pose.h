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

} // namespace zr

#endif // ZR_POSE_H
