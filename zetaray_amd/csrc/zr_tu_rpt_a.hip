// zr_tu_rpt_a.hip -- translation unit of libzetaray_amd.so holding the untextured K11 ReSTIR PT path-tracing kernels (ZR_RPT_GROUP_A, zr_kernels.h)
// Compiled with the per-hit decode of instance transforms and vertex normals: with the hit tables (zr_hit_tables.h) the general K11 ran 3.9 % slower on the
// 380 k-triangle atrium (7.19 -> 7.47 ms, frame 14.36 -> 14.62 ms, profiles/r07_hit_tables_ab.txt).  -DZR_HIT_TABLES_K11_GENERAL=1 gives it the tables for an A/B.
#ifndef ZR_HIT_TABLES_K11_GENERAL
#define ZR_HIT_TABLES_K11_GENERAL 0
#endif
#if !ZR_HIT_TABLES_K11_GENERAL      // (this wins over a -DZR_HIT_TABLES=1 on the command line: the switch above is the way to turn the tables on here)
#undef ZR_HIT_TABLES
#define ZR_HIT_TABLES 0
#endif
#include "zr_kernels.h"
ZR_RPT_GROUP_A(template)
