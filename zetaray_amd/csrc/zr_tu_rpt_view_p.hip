// zr_tu_rpt_view_p.hip -- translation unit of libzetaray_amd.so holding the reconnection-debug-view instantiations of K11 (k_rpt_pathtrace_view) (ZR_RPT_GROUP_VP, zr_kernels.h)
#include "zr_kernels.h"
ZR_RPT_GROUP_VP(template)
