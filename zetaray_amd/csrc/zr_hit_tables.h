// zr_hit_tables.h -- what hit reconstruction needs from an instance record and from a vertex, decoded once instead of per hit.
//
// FillHit (zr_dev_scene.h), the hit reconstruction of k_gbuffer (zr_stages.h) and MoveXk (zr_rpt.h) used to decode, for every hit in every lane,
// the instance's two quaternions (4 UNORM16 decodes + a normalize each), its two half3 scales and their reciprocals (six IEEE divisions), and the
// three vertex normals (an oct decode + a normalize each): 5 of FillHit's 6 square roots and 8 of its 9 divisions.  None of it depends on the hit.
// Device code reads them from two tables instead:
//   InstRec, one per mesh instance (96 B), refreshed by k_fill_inst_recs (zr_tu_scene_update.hip) behind everything that writes an instance array;
//   one float4 per vertex = DecodeOct32(vertex.normal), filled by k_fill_vtx_normals when the vertex buffer is uploaded (it is never written again).
// The tables hold the values of the very expressions they replace, computed by the same inline functions under the same compiler flags, so the
// bits a kernel sees do not change.  Host code (tests/hostexec, the oracle) keeps the per-hit decode: the tables exist on the device only.
// -DZR_HIT_TABLES=0 (make variant NAME=nohit EXTRA=-DZR_HIT_TABLES=0) compiles the per-hit decode into the kernels again, for A/B runs.
#pragma once
#include "zr_dev_math.h"

#ifndef ZR_HIT_TABLES
#define ZR_HIT_TABLES 1
#endif
// -DZR_HIT_TANGENTS=1 adds a second per-vertex array, DecodeOct32(vertex.tangent), which only k_gbuffer reads (every translation unit must be compiled with it:
// SceneView carries the pointer).  Off: measured on its own, profiles/r07_hit_tables_ab.txt
#ifndef ZR_HIT_TANGENTS
#define ZR_HIT_TANGENTS 0
#endif
// -DZR_HIT_VTX_NORMALS=0 keeps the instance records and decodes the vertex normals per hit again (the table is still filled), for A/B runs
#ifndef ZR_HIT_VTX_NORMALS
#define ZR_HIT_VTX_NORMALS 1
#endif
// kernels read the tables; everything compiled for the host decodes per hit
#if ZR_HIT_TABLES && defined(__HIP_DEVICE_COMPILE__)
#define ZR_HIT_TABLES_DEV 1
#else
#define ZR_HIT_TABLES_DEV 0
#endif
#define ZR_HIT_TANGENTS_DEV (ZR_HIT_TABLES_DEV && ZR_HIT_TANGENTS)
#define ZR_HIT_VTX_NORMALS_DEV (ZR_HIT_TABLES_DEV && ZR_HIT_VTX_NORMALS)

namespace zr {

// one frame's transform of an instance: 48 B = three 16-byte words.  q = normalize(DecodeNormalized4(rotation)), s = the half3 scale as floats,
// sInv = (1 / s.x, 1 / s.y, 1 / s.z).  d0 / d1 carry the record's d_translation (see InstRec)
struct InstXform { float q[4]; float sInv[3]; float d0; float s[3]; float d1; };
// curr from rotation / scale, prev from prev_rotation / prev_scale; d_translation as floats = (curr.d0, curr.d1, prev.d0); prev.d1 is padding
struct alignas(16) InstRec { InstXform curr, prev; };
static_assert(sizeof(InstRec) == 96, "InstRec layout");

ZR_HD InstXform MakeInstXform(const uint16_t* rotation, const uint16_t* scale)
{
    const V4 q = normalize(DecodeNormalized4(rotation));
    const V3 s = v3(zr_f16_to_f32(scale[0]), zr_f16_to_f32(scale[1]), zr_f16_to_f32(scale[2]));
    const V3 sInv = v3(1.0f / s.x, 1.0f / s.y, 1.0f / s.z);
    InstXform X;
    X.q[0] = q.x; X.q[1] = q.y; X.q[2] = q.z; X.q[3] = q.w;
    X.sInv[0] = sInv.x; X.sInv[1] = sInv.y; X.sInv[2] = sInv.z;
    X.s[0] = s.x; X.s[1] = s.y; X.s[2] = s.z;
    X.d0 = 0; X.d1 = 0;
    return X;
}
ZR_HD InstRec MakeInstRec(const zr_mesh_instance& md)
{
    InstRec R;
    R.curr = MakeInstXform(md.rotation, md.scale);
    R.prev = MakeInstXform(md.prev_rotation, md.prev_scale);
    R.curr.d0 = zr_f16_to_f32(md.d_translation[0]); R.curr.d1 = zr_f16_to_f32(md.d_translation[1]); R.prev.d0 = zr_f16_to_f32(md.d_translation[2]);
    return R;
}
ZR_HD V4 XformQ(const InstXform& X) { return v4(X.q[0], X.q[1], X.q[2], X.q[3]); }
ZR_HD V3 XformScale(const InstXform& X) { return v3p(X.s); }
ZR_HD V3 XformScaleInv(const InstXform& X) { return v3p(X.sInv); }
ZR_HD V3 RecDT(const InstRec& R) { return v3(R.curr.d0, R.curr.d1, R.prev.d0); }

// InverseTransformTRS (zr_dev_math.h) with the reciprocal scale it computes handed in: t * (1 / scale), the same product
ZR_HD V3 InverseTransformTRS_SInv(V3 pos, V3 tr, V4 rot, V3 scaleInv)
{
    V3 t = pos - tr;
    t = RotateVector(t, v4(-rot.x, -rot.y, -rot.z, rot.w));
    return t * scaleInv;
}

// one decoded unit vector per vertex at 16-byte stride (w unused)
struct alignas(16) VtxDir { float x, y, z, w; };

} // namespace zr
