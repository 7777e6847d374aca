"""The layout of every per-pixel plane a pass serves, through the C-ABI: pointer, size and bytes per pixel of each output, the bytes per pixel
of each halo exchange, and that the planes come up cleared -- after init, after frame overlap adds its planes and after a resize.  Nothing is
rendered."""
import numpy as np
import pytest

from zetaray_amd import wire

pytestmark = pytest.mark.gpu

W, H = 64, 32      # not square (a swapped width / height shows), a multiple of 32 (ReSTIR PT owned rects) and of 8 pixels (fused halo transfers)
ZR_ERR_INVALID_ARG, ZR_ERR_NOT_INITIALIZED = 1, 6
FINAL = ("final", 0, np.float32, 4)      # ZR_OUT_FINAL: RGBA32F


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


def _named(api, *names):
    tables = {**api.RPT_OUTPUTS, **api.RPT_OUTPUTS_EXTRA}
    return [(n,) + tables[n] for n in names]


def _cases(api):
    """(label, kind, integrator, [(name, id, dtype, channels)], halo bytes per pixel or None).  Every output is pass-sized except AUTO_EXPOSURE's, which
    are listed below.  "sky_lut" and the inscattering grid need a SKY pass and are not cleared at init: left out."""
    PT, GI, RPT = api.INTEGRATOR_PATH_TRACING, api.INTEGRATOR_RESTIR_GI, api.INTEGRATOR_RESTIR_PT
    rpt = ["A", "B", "C", "D", "E", "F", "G", "target", "neighbor", "map_ctn", "map_ntc"] + [f"{s}_{c}" for s in ("ctn", "ntc") for c in "ABCD"]
    return [
        ("indirect_pt", api.PASS_INDIRECT, PT, [FINAL], None),
        ("indirect_rgi", api.PASS_INDIRECT, GI, [FINAL] + _named(api, "gi_A", "gi_B", "gi_C"), 40),
        ("indirect_rpt", api.PASS_INDIRECT, RPT, [FINAL] + _named(api, *rpt), 62),
        ("di_emissive", api.PASS_DI_EMISSIVE, PT, [FINAL] + _named(api, "di_A", "di_B", "di_target"), 24),
        ("di_sky", api.PASS_DI_SKY, PT, [FINAL] + _named(api, "sdi_A", "sdi_B", "sdi_C", "sdi_target"), 13),
        ("compositing", api.PASS_COMPOSITING, PT, [FINAL], None),
        ("denoise", api.PASS_DENOISE, PT, _named(api, "denoised", "denoise_history", "denoise_moments"), 40),
        ("taa", api.PASS_TAA, PT, _named(api, "taa"), None),
        # the outputs of these two are not in api's tables: the literal values of zr_pass_get_output
        ("display", api.PASS_DISPLAY, PT, [("display", api.OUT_DISPLAY, np.float32, 4), ("display_srgb8", api.OUT_DISPLAY_SRGB8, np.uint8, 4)], None),
        ("auto_exposure", api.PASS_AUTO_EXPOSURE, PT, [("exposure", api.OUT_EXPOSURE, np.float32, 2), ("ae_histogram", api.OUT_AE_HISTOGRAM, np.uint32, 1)], None),
    ]


# AUTO_EXPOSURE's outputs are not per-pixel: (w, h) of each
FIXED_SIZE = {"exposure": (1, 1), "ae_histogram": (256, 1)}
# ZR_OUT_PICK_MASK on a DISPLAY pass is served once a picked instance has been rendered; before that it has an error text of its own
NOT_PROBED = {"display": {wire.OUT_PICK_MASK}}


def _check_outputs(p, outputs, w, h, when):
    for name, which, dt, ch in outputs:
        dev, ow, oh, bpp = p.output_ptr(which)
        print(f"{when}: {name}: ptr {'set' if dev else 'NULL'}, {ow} x {oh}, {bpp} B per pixel")
        assert dev, f"{when}: {name}: null pointer"
        assert (ow, oh) == FIXED_SIZE.get(name, (w, h)), f"{when}: {name}: {ow} x {oh}"
        assert bpp == np.dtype(dt).itemsize * ch, f"{when}: {name}: {bpp} B per pixel"
        got = p.download_raw(which, dt, (oh, ow, ch))
        assert not got.view(np.uint8).any(), f"{when}: {name}: not cleared"


def test_plane_layouts_and_clears(api):
    cases = _cases(api)
    all_ids = {o[1] for c in cases for o in c[3]} | {api.OUT_SKY_LUT, wire.OUT_INSCATTERING, wire.OUT_PICK_MASK}
    for label, kind, integrator, outputs, halo in cases:
        p = api.Pass(kind, W, H, integrator)
        gb = None
        try:
            _check_outputs(p, outputs, W, H, f"{label} after init")
            for which in sorted(all_ids - {o[1] for o in outputs} - NOT_PROBED.get(label, set())):
                with pytest.raises(api.ZetaRayError, match="pass has no such output") as e:
                    p.output_ptr(which)
                assert e.value.code == ZR_ERR_INVALID_ARG, (label, which)
            if halo is not None:
                assert p.halo_bytes_per_pixel() == halo, label
            if label == "indirect_pt":
                with pytest.raises(api.ZetaRayError, match="pass has no reservoir planes to exchange") as e:
                    p.halo_bytes_per_pixel()
                assert e.value.code == ZR_ERR_NOT_INITIALIZED
            if label == "indirect_rpt":
                gb = api.GBuffer(W, H)
                p.set_frame_overlap(gb, 1)
                _check_outputs(p, outputs, W, H, f"{label} after set_frame_overlap")
                assert p.halo_bytes_per_pixel() == halo
            p.resize(H, W)
            _check_outputs(p, outputs, H, W, f"{label} after resize to {H} x {W}")
            p.resize(W, H)
            _check_outputs(p, outputs, W, H, f"{label} after resize back")
            if halo is not None:
                assert p.halo_bytes_per_pixel() == halo, label
        finally:
            p.close()
            if gb is not None:
                gb.close()
