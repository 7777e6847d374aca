// tests/rptview -- TEST-ONLY host entry to rpt::DebugColor (zetaray_amd/csrc/zr_rpt.h), the stage function the reconnection debug views draw with:
// the same ZR_HD function the VIEW kernels inline, compiled with g++ so that the `-m "not gpu"` suite can hold it to the colour table of
// include/zetaray_amd.h class by class.  Never linked into, or loaded by, the product.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../zetaray_amd/csrc/zr_rpt.h"

// the reconnection record's fields DebugColor reads; `rgb` holds the radiance on entry and the view's colour (or the radiance, untouched) on return
extern "C" void zrv_debug_color(uint32_t view, uint32_t k, uint32_t lobe_k_min_1, uint32_t lobe_k, uint32_t lt_k, uint32_t lt_k_plus_1, float* rgb)
{
    zr::rpt::Reconnection rc = zr::rpt::InitReconnection();
    rc.k = k; rc.lobe_k_min_1 = lobe_k_min_1; rc.lobe_k = lobe_k; rc.lt_k = lt_k; rc.lt_k_plus_1 = lt_k_plus_1;
    zr::V3 c = zr::v3(rgb[0], rgb[1], rgb[2]);
    zr::rpt::DebugColor(rc, view, c);
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
}
