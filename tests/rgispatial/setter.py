"""The argument checks of zr_pass_set_rgi_spatial that need a pass, hence a device (TEST-ONLY; shared by tests/test_rgi_spatial_cpu.py, which runs them
when a device happens to be present, and tests/test_rgi_spatial_gpu.py)."""
import pytest

from zetaray_amd import api


def check_setter_arguments():
    """every argument error is ZR_ERR_INVALID_ARG; another pass kind is one; another integrator stores the value"""
    gi = api.Pass(api.PASS_INDIRECT, 64, 64, api.INTEGRATOR_RESTIR_GI)
    for ok in ((0, 0.0), (1, 0.0), (2, 64.0), (2, 0.5), (0, 16.0)):
        gi.set_rgi_spatial(*ok)
    for bad in ((3, 0.0), (0xffffffff, 16.0), (1, -1.0), (1, 64.5), (1, float("nan")), (1, float("inf")), (1, -float("inf"))):
        with pytest.raises(api.ZetaRayError) as e:
            gi.set_rgi_spatial(*bad)
        assert e.value.code == 1, bad
    for kind in (api.PASS_GBUFFER, api.PASS_DI_EMISSIVE, api.PASS_COMPOSITING):
        with pytest.raises(api.ZetaRayError) as e:
            api.Pass(kind, 64, 64).set_rgi_spatial(1, 0.0)
        assert e.value.code == 1
    # another integrator stores the value
    for integ in (api.INTEGRATOR_RESTIR_PT, api.INTEGRATOR_PATH_TRACING):
        api.Pass(api.PASS_INDIRECT, 64, 64, integ).set_rgi_spatial(2, 8.0)
