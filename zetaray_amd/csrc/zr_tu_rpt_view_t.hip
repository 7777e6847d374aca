// zr_tu_rpt_view_t.hip -- translation unit of libzetaray_amd.so holding the reconnection-debug-view instantiations of K14 (k_rpt_temporal_view) (ZR_RPT_GROUP_VT, zr_kernels.h)
#include "zr_kernels.h"
ZR_RPT_GROUP_VT(template)
