// zr_tu_rpt_view_s.hip -- translation unit of libzetaray_amd.so holding the reconnection-debug-view instantiations of K16 (k_rpt_stc_view) (ZR_RPT_GROUP_VS, zr_kernels.h)
#include "zr_kernels.h"
ZR_RPT_GROUP_VS(template)
