// TEST-ONLY: include/zr_alias.h compiled for the host on its own, so that tests/test_alias_device_{cpu,gpu}.py can hold the header's table -- the one the
// kernels of zr_tu_alias.hip build -- against the host Vose build (zr_alias_table_build), float64, and the device.
#include "../../include/zr_alias.h"

extern "C" {

void zal_build(const float* power, uint32_t n, zr_alias_entry* out) { zral::Build(power, n, out); }
float zal_kahan_sum(const float* power, uint32_t n) { return zral::KahanSum(power, n); }
// the fixed-point weights the table represents (w[i] / sum of w), for the tests' statement of the quantisation
void zal_weights(const float* power, uint32_t n, uint64_t* w)
{
    const float sumRcp = zral::SumRcp(zral::KahanSum(power, n), n);
    for (uint32_t i = 0; i < n; i++) w[i] = zral::Quantise(power[i], zral::Prob(power[i], sumRcp), n);
}

}
