"""TEST-ONLY harness: the reference's Display.hlsl mainPS (`zrefp_shader_display`, compiled by the oracle's recipe into
oracle/_ref/obj/post_display.o and reached through tests/displayref) on a full G-buffer, for any DisplayOption.  A ctypes mirror of hlsl::TexStorage / hlsl::DescriptorHeap (oracle/ref_hlsl/hlsl_resources.h) and ZrDispatch
(oracle/ref_hlsl/ref_dispatch.h) binds the ten planes at SLOT_GBUF_CURR with kGBufFormats (oracle/ref_hlsl/ref_pass_common.h), the input
image, the exposure texel and the tone-mapping LUT, as DisplayPass::Render does (Display.cpp:188-260).  Also the R8G8B8A8_UNORM_SRGB
store (zetaray_amd.h ZR_OUT_DISPLAY_SRGB8) of the views' float4 output."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISPLAY_OBJ = os.path.join(ROOT, "oracle", "_ref", "obj", "post_display.o")
_DIR = os.path.join(ROOT, "tests", "displayref")

# hlsl_resources.h enum TexFormat (pinned by tests/test_display_views_cpu.py)
FMT = dict(FMT_R8_UNORM=4, FMT_RG8_UNORM=5, FMT_RGBA8_UNORM=6, FMT_RGBA16_UINT=9, FMT_RG16_UNORM=11, FMT_RG16_SNORM=12, FMT_RGBA16_FLOAT=15,
           FMT_RGBA32_UINT=18, FMT_R32_FLOAT=19, FMT_RG32_UINT=17, FMT_RG32_FLOAT=20, FMT_R11G11B10_FLOAT=22, FMT_R9G9B9E5=23)
# ref_pass_common.h kGBufFormats, in ZR_GB_* order
GBUF_FORMATS = ["FMT_RGBA8_UNORM", "FMT_RG16_UNORM", "FMT_RG8_UNORM", "FMT_RG16_SNORM", "FMT_R11G11B10_FLOAT", "FMT_R8_UNORM",
                "FMT_RGBA16_UINT", "FMT_R32_FLOAT", "FMT_RGBA32_UINT", "FMT_RG32_UINT"]
SLOT_GBUF_CURR, SLOT_PASS = 16, 80
POST_INPUT, POST_EXPOSURE, POST_LUT = SLOT_PASS, SLOT_PASS + 1, SLOT_PASS + 2
HEAP_SIZE = 8192


class TexStorage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("readData", C.c_void_p), ("w", C.c_uint32), ("h", C.c_uint32), ("d", C.c_uint32), ("fmt", C.c_int),
                ("heap", C.c_void_p), ("heapIdx", C.c_uint32)]


class DescriptorHeap(C.Structure):
    _fields_ = [("table", TexStorage * HEAP_SIZE)]


class ZrDispatch(C.Structure):
    _fields_ = [("scene", C.c_void_p), ("prev_scene", C.c_void_p), ("use_prev_scene", C.c_int), ("heap", C.c_void_p), ("frame_cb", C.c_void_p),
                ("local_cb", C.c_void_p), ("local_cb_bytes", C.c_uint32), ("groups_x", C.c_uint32), ("groups_y", C.c_uint32), ("root_uav", C.c_void_p),
                ("buf", C.c_void_p * 4), ("buf_count", C.c_uint32 * 4), ("groups_z", C.c_uint32)]


class CbDisplayPass(C.Structure):      # Display_Common.h:32-46
    _fields_ = [("DisplayOption", C.c_uint16), ("Tonemapper", C.c_uint16), ("AutoExposure", C.c_uint16), ("pad", C.c_uint16),
                ("InputDescHeapIdx", C.c_uint32), ("ExposureDescHeapIdx", C.c_uint32), ("LUTDescHeapIdx", C.c_uint32),
                ("Saturation", C.c_float), ("AgXExp", C.c_float), ("RoughnessTh", C.c_float)]


def available():
    return os.path.exists(DISPLAY_OBJ)


_L = None


def _lib():
    global _L
    if _L is None:
        import fcntl
        with open(os.path.join(_DIR, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-s", "-C", _DIR, "libzdr.so"])
            L = C.CDLL(os.path.join(_DIR, "libzdr.so"))
        L.zdr_shader_display.argtypes = [C.c_void_p]
        L.zdr_linear_to_srgb8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        _L = L
    return _L


def shader_display(image, gb_arrays, params, cb, option, roughness_th=1.0, exposure2=None, lut=None):
    """mainPS over cb's display size.  image: (rh, rw, 4) RGBA16F bits (uint16) or RGBA32F (read rounded to half, as the HIP pass does);
    gb_arrays: the ten G-buffer planes (wire.alloc_gbuffer_planes / GBuffer.download order).  Returns (dh, dw, 4) float32."""
    a = np.ascontiguousarray(image)
    if a.dtype == np.float32:
        a = np.ascontiguousarray(a.astype(np.float16).view(np.uint16))
    assert a.dtype == np.uint16 and a.ndim == 3 and a.shape[2] == 4
    rh, rw = a.shape[:2]
    keep = [a]
    heap = DescriptorHeap()

    def bind(slot, arr, w, h, fmt, d=1):
        arr = np.ascontiguousarray(arr)
        keep.append(arr)
        t = heap.table[slot]
        t.data, t.w, t.h, t.d, t.fmt = arr.ctypes.data, w, h, d, FMT[fmt]

    bind(POST_INPUT, a, rw, rh, "FMT_RGBA16_FLOAT")
    for k, (plane, fmt) in enumerate(zip(gb_arrays, GBUF_FORMATS)):
        assert plane.shape[0] == rh and plane.shape[1] == rw, (k, plane.shape, (rh, rw))
        bind(SLOT_GBUF_CURR + k, plane, rw, rh, fmt)
    if exposure2 is not None:
        bind(POST_EXPOSURE, np.array(exposure2, np.float32).reshape(2), 1, 1, "FMT_RG32_FLOAT")
    if lut is not None:
        l = np.ascontiguousarray(lut, np.uint32)
        dim = int(round(l.size ** (1.0 / 3.0)))
        bind(POST_LUT, l, dim, dim, "FMT_R9G9B9E5", d=dim)
    L = CbDisplayPass(DisplayOption=int(option), Tonemapper=int(params.display_tonemapper), AutoExposure=int(params.display_auto_exposure),
                      InputDescHeapIdx=POST_INPUT, ExposureDescHeapIdx=POST_EXPOSURE, LUTDescHeapIdx=POST_LUT,
                      Saturation=params.display_saturation, AgXExp=params.display_agx_exp, RoughnessTh=float(np.float32(roughness_th)))
    g = np.ascontiguousarray(cb).copy()
    g["curr_gbuffer_desc_heap_offset"] = SLOT_GBUF_CURR
    dw, dh = int(np.asarray(g["display_width"]).reshape(-1)[0]), int(np.asarray(g["display_height"]).reshape(-1)[0])
    out = np.zeros((dh, dw, 4), np.float32)
    d = ZrDispatch(heap=C.addressof(heap), frame_cb=g.ctypes.data, local_cb=C.addressof(L), local_cb_bytes=C.sizeof(L), root_uav=out.ctypes.data)
    _lib().zdr_shader_display(C.byref(d))
    return out


def linear_to_srgb8(rgba):
    """(h, w, 4) float32 -> (h, w, 4) uint8 as the back buffer stores it"""
    a = np.ascontiguousarray(rgba, np.float32)
    out = np.zeros(a.shape, np.uint8)
    _lib().zdr_linear_to_srgb8(a.ctypes.data, a.size // 4, out.ctypes.data)
    return out
