"""Which reservoir set a two-set pass names after each call, through the C-ABI, for DI emissive, sky DI, ReSTIR GI and ReSTIR PT without frame
overlap: zr_pass_get_output of reservoir plane A is the set the last frame wrote, so its device POINTER tells when a pass flips its sets, and what
zr_pass_reset_temporal and zr_pass_resize do to them.  X is the pointer right after init, Y the other set's.  Contents matter once only: a
ZR_HALO_FINAL block must hold the same set the output names."""
import numpy as np
import pytest

from zetaray_amd import scene_io, wire

pytestmark = pytest.mark.gpu

W, H = 64, 32      # two 32 x 32 tiles: the halo rect below is the second one
RECT = (32, 0, 32, 32)
# case -> (reservoir plane A in api.RPT_OUTPUTS / RPT_OUTPUTS_EXTRA, spatial rounds of a ReSTIR PT frame that has a history)
CASES = {"di": ("di_A", 0), "sky": ("sdi_A", 0), "gi": ("gi_A", 0), "rpt_no_spatial": ("A", 0), "rpt": ("A", 1)}


@pytest.fixture(scope="module")
def api():
    from zetaray_amd import api
    assert api.device_count() >= 1, "no HIP device visible"
    return api


class _Rig:
    def __init__(self, api, scene, case):
        self.api, self.case, self.scene_host = api, case, scene
        self.plane, self.rounds = CASES[case]
        prm = wire.default_params()
        prm.num_spatial_passes = self.rounds
        integ = {"gi": api.INTEGRATOR_RESTIR_GI, "rpt": api.INTEGRATOR_RESTIR_PT, "rpt_no_spatial": api.INTEGRATOR_RESTIR_PT}.get(case, api.INTEGRATOR_PATH_TRACING)
        self.r = api.Renderer(scene, W, H, params=prm, integrator=integ)
        if case == "di":
            self.p = self.r.enable_direct(wire.default_params_di())
        elif case == "sky":
            self.p = self.r.enable_sky_direct(wire.default_params_sky_di())
        else:
            self.p = self.r.p_indirect
        self.which = {**api.RPT_OUTPUTS, **api.RPT_OUTPUTS_EXTRA}[self.plane][0]
        self.frames = 0

    def front(self):
        """what a frame renders before the pass under test: [sky LUT,] G-buffer, PreLighting"""
        self.frames += 1
        cb = scene_io.make_frame_constants(W, H, frame_num=self.frames, num_emissives=len(self.scene_host.emissives))
        self.r.render_sky(cb)
        self.r.p_gbuffer.render(cb, self.r.scene, self.r.gbuffer)
        self.r.p_prelight.render(cb, self.r.scene)
        return cb

    def frame(self):
        self.p.render(self.front(), self.r.scene, self.r.gbuffer)

    def stage(self, cb, stages):
        self.p.render_stage(cb, self.r.scene, self.r.gbuffer, stages)

    def ptr(self):
        return self.p.output_ptr(self.which)[0]

    def flips(self, history):
        """set flips of one whole frame: one per frame; ReSTIR PT one more per spatial round, and it runs its rounds only on a history"""
        return 1 + (self.rounds if history else 0)


def _after(ptr, X, Y, flips):
    return ptr if flips % 2 == 0 else (Y if ptr == X else X)


@pytest.mark.parametrize("case", list(CASES))
def test_reservoir_set_sequence(api, cornell_emissive, case):
    import torch
    g = _Rig(api, cornell_emissive, case)
    p = g.p
    X = g.ptr()
    g.frame()
    Y = g.ptr()
    print(f"{case}: X {X:#x}, Y {Y:#x}")
    assert X and Y and Y != X, "the first frame (no history: one flip) must name the other set"
    # whole frames: Y, X, Y -- ReSTIR PT with one spatial round flips twice per frame once it has a history, so it stays at Y
    want = Y
    for f in (2, 3):
        g.frame()
        want = _after(want, X, Y, g.flips(True))
        print(f"{case}: frame {f}: {g.ptr():#x}, want {want:#x}")
        assert g.ptr() == want, f"frame {f}"
    if g.rounds == 0:
        assert want == Y

    # a ZR_HALO_FINAL block names the set the output names: its first plane section is the rect of plane A
    _, dt, ch = {**api.RPT_OUTPUTS, **api.RPT_OUTPUTS_EXTRA}[g.plane]
    bpp = p.halo_bytes_per_pixel()
    buf = torch.zeros(RECT[2] * RECT[3] * bpp, dtype=torch.uint8, device="cuda")
    p.halo_pack(g.r.gbuffer, api.HALO_FINAL, RECT, buf.data_ptr(), buf.numel())
    torch.cuda.synchronize()
    a = np.ascontiguousarray(p.download_plane(g.plane)[RECT[1]:RECT[1] + RECT[3], RECT[0]:RECT[0] + RECT[2]])
    assert a.dtype == np.dtype(dt) and a.shape[2] == ch
    got = buf[:a.nbytes].cpu().numpy()
    print(f"{case}: halo block {buf.numel()} B, plane A section {a.nbytes} B, {int((a.view(np.uint8) != 0).sum())} non-zero bytes")
    assert np.array_equal(got, a.view(np.uint8).reshape(-1)), "ZR_HALO_FINAL does not move the set ZR_OUT_*_RESERVOIR_A names"
    if case != "sky":      # (the closed box shows little sky: its one-byte records may all be empty)
        assert a.view(np.uint8).any()

    # one frame stage by stage
    if case == "gi":
        p.set_rgi_spatial(1)
    cb = g.front()
    g.stage(cb, api.STAGE_TEMPORAL)
    if case == "gi":      # flips at the end of TEMPORAL; its SPATIAL stage reads the set that wrote and flips nothing
        want = _after(want, X, Y, 1)
        assert g.ptr() == want, "GI: the TEMPORAL stage flips"
        g.stage(cb, api.STAGE_SPATIAL)
        assert g.ptr() == want, "GI: the SPATIAL stage does not flip"
        p.set_rgi_spatial(0)
    else:                 # DI / sky DI / ReSTIR PT: the frame ends with its SPATIAL stage
        assert g.ptr() == want, "a TEMPORAL-only call must leave the sets alone"
        g.stage(cb, api.STAGE_SPATIAL)
        want = _after(want, X, Y, g.flips(True))
        assert g.ptr() == want, "the SPATIAL stage ends the frame"

    # resize there and back: the init state, whatever the state before (here: an odd number of flips since init)
    if g.ptr() == X:
        g.frame()
        want = _after(want, X, Y, g.flips(True))
        assert g.ptr() == want
    assert g.ptr() == Y
    p.resize(H, W)
    p.resize(W, H)
    X2 = g.ptr()
    g.frame()
    Y2 = g.ptr()
    print(f"{case}: after resize X {X2:#x}, Y {Y2:#x}")
    assert X2 and Y2 and Y2 != X2, "after a resize the first frame has no history: one flip"
    if {X2, Y2} == {X, Y}:      # the allocator handed the same two blocks back: then the pointers themselves show the rewind
        assert X2 == X, "resize must rewind to the init set"

    # reset_temporal after one frame: DI and sky DI rewind to the init set, GI only drops its history, ReSTIR PT leaves its roles alone
    p.reset_temporal()
    want = X2 if case in ("di", "sky") else Y2
    assert g.ptr() == want, "reset_temporal"
    g.frame()      # ... and the next frame has no history: one flip
    assert g.ptr() == _after(want, X2, Y2, g.flips(False)), "the frame after reset_temporal"
    torch.cuda.synchronize()
