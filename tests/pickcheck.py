"""TEST-ONLY numpy restatement of the picked-instance outline (zetaray_amd.h zr_pass_set_picked_instances): the WVP product, the raster contract
(transform, homogeneous clipping with the 16 w guard band, viewport, 16.8 snapping, fan triangulation, top-left int64 edge functions) and
Sobel.hlsl's outline test.  Every fp32 operation is written out one at a time, in the contract's order, so the mask is bit-exact."""
import numpy as np

F = np.float32
G = F(16.0)
OUTLINE_RGBA = np.array([0.913098693, 0.332451582, 0.048171822, 1.0], np.float32)


def view_proj(cb):
    """CurrViewProj = mul(view, proj) (DefaultRenderer.cpp:72-79) for the frame constants' camera: lookToLH view (cb.curr_view, 3x4, column
    convention) and the infinite reverse-Z projection of Camera.cpp:206 (MatrixFuncs.h perspectiveReverseZ), row-vector convention, row-major"""
    v = np.asarray(cb["curr_view"], np.float32).reshape(3, 4)
    V = np.zeros((4, 4), np.float32)
    V[:3, :3] = v[:, :3].T
    V[3, :3] = v[:, 3]
    V[3, 3] = 1
    t = F(1) / F(cb["tan_half_fov"])
    P = np.zeros((4, 4), np.float32)
    P[0, 0], P[1, 1], P[2, 3], P[3, 2] = t / F(cb["aspect_ratio"]), t, 1, F(cb["camera_near"])
    return (V.astype(np.float64) @ P.astype(np.float64)).astype(np.float32).reshape(16)


def wvp(to_world_3x4, vp16):
    M = np.asarray(to_world_3x4, np.float32).reshape(3, 4)
    W = np.zeros((4, 4), np.float32)
    W[:, :3] = M.T
    W[3, 3] = 1
    VP = np.asarray(vp16, np.float32).reshape(4, 4)
    out = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            a, b, c, d = W[i, 0] * VP[0, j], W[i, 1] * VP[1, j], W[i, 2] * VP[2, j], W[i, 3] * VP[3, j]
            out[i, j] = ((a + b) + c) + d
    return out


def _dist(v, plane):
    x, y, z, w = v
    return [z, w - z, x + G * w, G * w - x, y + G * w, G * w - y][plane]


def _clip(poly):
    for plane in range(6):
        out = []
        n = len(poly)
        for i in range(n):
            a, b = poly[i], poly[(i + 1) % n]
            da, db = _dist(a, plane), _dist(b, plane)
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                s = da / (da - db)
                out.append(np.array([a[j] + s * (b[j] - a[j]) for j in range(4)], np.float32))
        poly = out
        if not poly:
            break
    return poly


def _top_left(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


def _edge_in(ax, ay, bx, by, px, py):
    e = (np.int64(bx - ax) * (py - ay)) - (np.int64(by - ay) * (px - ax))
    return (e > 0) | ((e == 0) & _top_left(bx - ax, by - ay))


def raster_mask(tris_obj, m, display, render):
    """tris_obj: (n, 3, 3) float32 object-space positions; m: 4x4 WVP; display = (dw, dh) viewport; render = (rw, rh) mask.  Returns (rh, rw) uint8."""
    dw, dh = display
    rw, rh = render
    mask = np.zeros((rh, rw), bool)
    t = np.asarray(tris_obj, np.float32)
    # clip_j = ((x m0j + y m1j) + z m2j) + m3j
    clip = ((t[..., 0:1] * m[0] + t[..., 1:2] * m[1]) + t[..., 2:3] * m[2]) + m[3]          # (n, 3, 4)
    x, y, z, w = clip[..., 0], clip[..., 1], clip[..., 2], clip[..., 3]
    all_in = ((z >= 0) & (w - z >= 0) & (x + G * w >= 0) & (G * w - x >= 0) & (y + G * w >= 0) & (G * w - y >= 0)).all(axis=1)
    for tri, inside in zip(clip, all_in):
        poly = list(tri) if inside else _clip(list(tri))
        if len(poly) < 3 or any(not (v[3] > 0) for v in poly):
            continue
        q = []
        for v in poly:
            ix, iy = v[0] / v[3], v[1] / v[3]
            sx, sy = (ix * F(0.5) + F(0.5)) * F(dw), (F(0.5) - iy * F(0.5)) * F(dh)
            q.append((int(np.rint(sx * F(256))), int(np.rint(sy * F(256)))))
        for i in range(1, len(q) - 1):
            (ax, ay), (bx, by), (cx, cy) = q[0], q[i], q[i + 1]
            area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            if area == 0:
                continue
            if area < 0:
                bx, by, cx, cy = cx, cy, bx, by
            x0 = max(-((128 - min(ax, bx, cx)) // 256), 0)
            x1 = min((max(ax, bx, cx) - 128) // 256, rw - 1)
            y0 = max(-((128 - min(ay, by, cy)) // 256), 0)
            y1 = min((max(ay, by, cy) - 128) // 256, rh - 1)
            if x0 > x1 or y0 > y1:
                continue
            py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
            px, py = px * 256 + 128, py * 256 + 128
            cov = _edge_in(ax, ay, bx, by, px, py) & _edge_in(bx, by, cx, cy, px, py) & _edge_in(cx, cy, ax, ay, px, py)
            mask[y0:y1 + 1, x0:x1 + 1] |= cov
    return mask.astype(np.uint8) * np.uint8(255)


def outline(mask, display):
    """Sobel.hlsl mainPS over the display: CheckNeighborHood within the mask's (render) size, then Luminance(|grad|) > 0 with out-of-range loads = 0"""
    dw, dh = display
    rh, rw = mask.shape
    m = np.zeros((dh + 2, dw + 2), np.int32)
    h, w = min(rh, dh + 1), min(rw, dw + 1)
    m[1:h + 1, 1:w + 1] = mask[:h, :w] != 0
    at = lambda dx, dy: m[1 + dy:1 + dy + dh, 1 + dx:1 + dx + dw]       # noqa: E731
    near = np.zeros((dh, dw), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near |= at(dx, dy) > 0
    gx = -at(-1, -1) - 2 * at(-1, 0) - at(-1, 1) + at(1, -1) + 2 * at(1, 0) + at(1, 1)
    gy = at(-1, -1) + 2 * at(0, -1) + at(1, -1) - at(-1, 1) - 2 * at(0, 1) - at(1, 1)
    g = np.sqrt((gx * gx + gy * gy).astype(np.float32))
    lum = F(0.2126) * g + F(0.7152) * g + F(0.0722) * g
    return near & (lum > 0)


def apply_outlines(rgba, srgb, outlines, srgb_word):
    """the display planes after the outline pass: `outlines` = list of (dh, dw) bool, one per pick"""
    rgba, srgb = rgba.copy(), srgb.copy()
    for o in outlines:
        rgba[o] = OUTLINE_RGBA
        srgb.view(np.uint32)[..., 0][o] = srgb_word
    return rgba, srgb
