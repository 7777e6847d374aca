// TEST-ONLY: see Makefile.  zdr_shader_display = the reference's Display.hlsl mainPS over a ZrDispatch (oracle/ref_hlsl/ref_dispatch.h);
// zdr_linear_to_srgb8 = the R8G8B8A8_UNORM_SRGB store of include/zetaray_amd.h ZR_OUT_DISPLAY_SRGB8 (IEC 61966-2-1 OETF, then
// (uint)fma(x, 255, 0.5); alpha stored as UNORM8), in the ABI's arithmetic (include/zr_detmath.h).
#include <cstdint>
#include <cstddef>
#include "../../include/zr_detmath.h"

extern "C" void zrefp_shader_display(const void* dispatch);

static uint32_t Unorm8(float c) { return (uint32_t)zr_fma(zr_saturate(c), 255.0f, 0.5f); }
static uint32_t Srgb8(float c)
{
    c = zr_isnan(c) ? 0.0f : zr_saturate(c);
    const float e = c <= 0.0031308f ? 12.92f * c : 1.055f * zr_pow(c, 1.0f / 2.4f) - 0.055f;
    return Unorm8(e);
}

extern "C" {
__attribute__((visibility("default"))) void zdr_shader_display(const void* dispatch) { zrefp_shader_display(dispatch); }

__attribute__((visibility("default"))) void zdr_linear_to_srgb8(const float* rgba, size_t n, uint8_t* out)
{
    for (size_t i = 0; i < n; i++)
    {
        for (int k = 0; k < 3; k++) out[4 * i + k] = (uint8_t)Srgb8(rgba[4 * i + k]);
        out[4 * i + 3] = (uint8_t)Unorm8(zr_isnan(rgba[4 * i + 3]) ? 0.0f : rgba[4 * i + 3]);
    }
}
}
