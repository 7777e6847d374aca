"""Writes tests/golden/jpeg_cases.npz: JPEG files written by Pillow (libjpeg-turbo) and Pillow's decode of each -- the fixture of tests/test_jpeg_cpu.py,
tests/test_jpeg_gpu.py, tests/jpegmath/host_check.cpp and tools/jpeg_decode_bench.py.  Run where Pillow is installed:
    python tools/make_jpeg_goldens.py
names[i] names file i, f_<i> holds its bytes and d_<i> Pillow's (h, w, 3) RGB decode (absent for the files the loader must refuse)."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (7, 5), (8, 8), (9, 9), (16, 16), (17, 23), (33, 17), (2, 40)]      # (w, h)
MODES = [("L", None, "gray"), ("RGB", 0, "444"), ("RGB", 1, "422"), ("RGB", 2, "420")]
QUALITY = [30, 90, 100]


def content(rng, kind, w, h):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 5 + 40) % 256, (xx + yy * 9) % 256], axis=2).astype(np.uint8)


def encode(img, mode, subsampling, **kw):
    b = io.BytesIO()
    im = Image.fromarray(img).convert(mode)
    if subsampling is not None:
        kw["subsampling"] = subsampling
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def main():
    rng = np.random.default_rng(13)
    cases = []      # (name, bytes, decodable)
    k = 0
    for w, h in SIZES:
        for mode, ss, tag in MODES:
            q, kind = QUALITY[k % 3], ("noise", "smooth")[(k // 3) % 2]
            cases.append(("%dx%d_%s_q%d_%s" % (w, h, tag, q, kind), encode(content(rng, kind, w, h), mode, ss, quality=q), True))
            k += 1
    # the files the Cornell glTF of the tests names, whatever the cycle above gave their sizes
    for (w, h), (mode, ss, tag), q, kind in (((33, 17), MODES[3], 90, "noise"), ((16, 16), MODES[1], 100, "smooth"), ((7, 5), MODES[2], 90, "noise")):
        name = "%dx%d_%s_q%d_%s" % (w, h, tag, q, kind)
        if name not in [c[0] for c in cases]:
            cases.append((name, encode(content(rng, kind, w, h), mode, ss, quality=q), True))
    noise = content(rng, "noise", 33, 17)
    cases.append(("33x17_420_optimize", encode(noise, "RGB", 2, quality=90, optimize=True), True))
    cases.append(("17x23_gray_optimize", encode(content(rng, "smooth", 17, 23), "L", None, quality=30, optimize=True), True))
    cases.append(("33x17_420_restart_blocks", encode(noise, "RGB", 2, quality=90, restart_marker_blocks=1), True))
    cases.append(("17x23_444_restart_blocks", encode(content(rng, "noise", 17, 23), "RGB", 0, quality=30, restart_marker_blocks=1), True))
    cases.append(("33x17_422_restart_rows", encode(noise, "RGB", 1, quality=100, restart_marker_rows=1), True))
    cases.append(("17x23_gray_restart_rows", encode(content(rng, "noise", 17, 23), "L", None, quality=90, restart_marker_rows=1), True))
    qt = [list(map(int, rng.integers(1, 64, 64))), list(map(int, rng.integers(1, 256, 64)))]
    cases.append(("16x16_420_qtables", encode(content(rng, "noise", 16, 16), "RGB", 2, qtables=qt), True))
    # chroma components of one and of two samples per row: libjpeg does not filter those
    cases.append(("4x5_420_q90_noise", encode(content(rng, "noise", 4, 5), "RGB", 2, quality=90), True))
    cases.append(("3x3_422_q90_noise", encode(content(rng, "noise", 3, 3), "RGB", 1, quality=90), True))
    # what the measurement tiles (tools/jpeg_decode_bench.py)
    yy, xx = np.mgrid[0:64, 0:64] / 64.0
    photo = np.stack([128 + 90 * np.sin(5.1 * xx + 2.0 * yy), 128 + 80 * np.cos(3.3 * yy - 1.7 * xx) * np.sin(9.0 * xx), 60 + 150 * xx * yy], axis=2)
    photo = (photo + rng.integers(-4, 5, (64, 64, 3))).clip(0, 255).astype(np.uint8)      # low frequencies and a little grain, like a photograph
    # (one restart interval per MCU row of the tile -- 4 MCUs of 16 x 16, 8 of 8 x 8 -- so that the tool can repeat the intervals to any multiple of 64)
    cases.append(("64x64_420_q90_bench", encode(photo, "RGB", 2, quality=90, restart_marker_blocks=4), True))
    cases.append(("64x64_gray_q90_bench", encode(photo, "L", None, quality=90, restart_marker_blocks=8), True))
    # refused
    cases.append(("16x16_progressive", encode(noise[:16, :16], "RGB", 2, quality=90, progressive=True), False))
    b = io.BytesIO()
    Image.fromarray(np.concatenate([noise[:16, :16], noise[:16, :16, :1]], axis=2), "CMYK").save(b, "JPEG", quality=90)
    cases.append(("16x16_cmyk", b.getvalue(), False))

    out = {"names": np.array([c[0] for c in cases])}
    for i, (name, data, ok) in enumerate(cases):
        out["f_%d" % i] = np.frombuffer(data, np.uint8)
        if ok:
            out["d_%d" % i] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    path = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print("%d files, %d bytes of JPEG, %s: %d bytes" % (len(cases), sum(len(c[1]) for c in cases), path, os.path.getsize(path)))


if __name__ == "__main__":
    sys.exit(main())
