// zr_tu_rpt_j.hip -- translation unit of libzetaray_amd.so holding the material-class permutation of K16 (PLAIN = true) (ZR_RPT_GROUP_J, zr_kernels.h)
// Compiled with the per-hit decode of instance transforms and vertex normals: with the hit tables (zr_hit_tables.h) this kernel spills four more VGPRs and
// ran 1.5 % slower (profiles/r07_hit_tables_ab.txt), while K1, K11 and K14 gained.  -DZR_HIT_TABLES_STC_PLAIN=1 gives it the tables for an A/B.
#ifndef ZR_HIT_TABLES_STC_PLAIN
#define ZR_HIT_TABLES_STC_PLAIN 0
#endif
#if !ZR_HIT_TABLES_STC_PLAIN      // (this wins over a -DZR_HIT_TABLES=1 on the command line: the switch above is the way to turn the tables on here)
#undef ZR_HIT_TABLES
#define ZR_HIT_TABLES 0
#endif
#include "zr_kernels.h"
ZR_RPT_GROUP_J(template)
