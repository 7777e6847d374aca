// zr_tu_display.hip -- translation unit of libzetaray_amd.so holding the G-buffer debug views of the display pass (RP/Display/Display.hlsl:41-171,
// DisplayOption::BASE_COLOR .. DEPTH) and the picked-instance outline (DrawPicked.hlsl + Sobel.hlsl): the kernels and their launches.  zr_api.hip
// calls LaunchDisplayView from the DISPLAY pass's render when a view other than DEFAULT is set (DEFAULT stays k_display), then LaunchPickOutline
// once per picked instance.
#include <hip/hip_runtime.h>
#include "zr_stages.h"
#include "zr_post.h"

using namespace zr;

namespace {

// DisplayOption, Display_Common.h:6-19 (= enum zr_display_option)
enum : int { V_DEFAULT, V_BASE_COLOR, V_NORMAL, V_METALNESS_ROUGHNESS, V_COAT_WEIGHT, V_COAT_COLOR, V_ROUGHNESS_TH, V_EMISSIVE, V_TRANSMISSION, V_DEPTH, V_COUNT };

// GBuffer::DecodeMetallic, GBuffers.hlsli:68-82: (uint)mad(encoded, 255, 0.5) of the RG8_UNORM .x
__device__ __forceinline__ uint32_t MetallicFlags(uint16_t mr) { return (uint32_t)zr_fma(zr_div255((float)(mr & 0xffu)), 255.0f, 0.5f); }
constexpr uint32_t kFlagTransmissive = 1u << 0, kFlagEmissive = 1u << 1, kFlagCoated = 1u << 5, kFlagMetallic = 1u << 7;

// mainPS, Display.hlsl:41-171, for one non-DEFAULT option.  Every view overwrites the tone-mapped colour of :55-75, so the tone mapping is not
// computed (it has no other effect).  G-buffer planes are point-clamp sampled at the display UV like the input image of k_display; the COAT
// views load g_coat at the display pixel itself (g_coat[psin.PosSS.xy]), 0 outside the render-size plane.
template<int OPTION>
__global__ void __launch_bounds__(256) k_display_view(GBuf gb, uint32_t dw, uint32_t dh, float cameraNear, float roughnessTh, F4* out, uint32_t* outSrgb)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dw * dh) return;
    const uint32_t x = i % dw, y = i / dw;
    const uint32_t rw = gb.w, rh = gb.h;
    const float u = ((float)x + 0.5f) / (float)dw, v = ((float)y + 0.5f) / (float)dh;
    int sx = (int)zr_floor(u * (float)rw), sy = (int)zr_floor(v * (float)rh);
    sx = sx < 0 ? 0 : (sx > (int)rw - 1 ? (int)rw - 1 : sx); sy = sy < 0 ? 0 : (sy > (int)rh - 1 ? (int)rh - 1 : sy);
    const size_t sp = (size_t)sy * rw + sx;

    // :51-53: a miss shows as float4(0) in every view
    const float z = gb.depth[sp];
    if (z == ZR_FLT_MAX) { out[i] = f4(0.0f, 0.0f, 0.0f, 0.0f); outSrgb[i] = 0u; return; }

    V3 d;
    if (OPTION == V_DEPTH) d = v3(cameraNear / z);                                                         // :77-81
    else if (OPTION == V_NORMAL) d = DecodeOct32u(gb.normal[sp]) * 0.5f + v3(0.5f);                          // :82-88
    else if (OPTION == V_BASE_COLOR)                                                                       // :89-94
    {
        const uint32_t c = gb.baseColor[sp];
        d = v3(zr_div255((float)(c & 0xffu)), zr_div255((float)((c >> 8) & 0xffu)), zr_div255((float)((c >> 16) & 0xffu)));
    }
    else if (OPTION == V_METALNESS_ROUGHNESS)                                                              // :95-104
    {
        const uint16_t mr = gb.mr[sp];
        d = v3((MetallicFlags(mr) & kFlagMetallic) ? 1.0f : 0.0f, zr_div255((float)(mr >> 8)), 0.0f);
    }
    else if (OPTION == V_COAT_WEIGHT || OPTION == V_COAT_COLOR)                                            // :105-138
    {
        d = v3(0.0f);
        if (MetallicFlags(gb.mr[sp]) & kFlagCoated)
        {
            // GBuffer::UnpackCoat, GBuffers.hlsli:107-120, of .xyz
            uint32_t px = 0, py = 0;
            if (x < rw && y < rh) { const size_t cp = 4 * ((size_t)y * rw + x); px = gb.coat[cp]; py = gb.coat[cp + 1]; }
            if (OPTION == V_COAT_WEIGHT) d = v3(zr_div255((float)((py >> 8) & 0xffu)));
            else d = UnpackRGB8(px | ((py & 0xffu) << 16));
        }
    }
    else if (OPTION == V_ROUGHNESS_TH)                                                                     // :139-145
    {
        const float r = zr_div255((float)(gb.mr[sp] >> 8));
        d = (r >= roughnessTh ? 1.0f : 0.0f) * v3(0.26f, 0.014f, 0.021f);
    }
    else if (OPTION == V_EMISSIVE)                                                                         // :146-159
    {
        if (MetallicFlags(gb.mr[sp]) & kFlagEmissive)
        {
            const uint32_t e = gb.emissive[sp];
            d = v3(zr_unpack_ufloat(e & 0x7ffu, 6), zr_unpack_ufloat((e >> 11) & 0x7ffu, 6), zr_unpack_ufloat(e >> 22, 5));
        }
        else
        {
            const uint32_t c = gb.baseColor[sp];
            d = v3(zr_div255((float)(c & 0xffu)), zr_div255((float)((c >> 8) & 0xffu)), zr_div255((float)((c >> 16) & 0xffu))) * 0.005f;
        }
    }
    else                                                                                                   // :160-168, TRANSMISSION
    {
        const bool tr = (MetallicFlags(gb.mr[sp]) & kFlagTransmissive) != 0;
        d = v3(tr ? 1.0f : 0.0f, tr ? 0.0f : 1.0f, 0.0f);
    }
    out[i] = f4(d, 1.0f);
    outSrgb[i] = post::LinearToSrgb8(d.x) | (post::LinearToSrgb8(d.y) << 8) | (post::LinearToSrgb8(d.z) << 16) | 0xff000000u;
}

template<int OPTION>
void Launch(hipStream_t s, const GBuf& gb, uint32_t dw, uint32_t dh, float cameraNear, float roughnessTh, F4* out, uint32_t* outSrgb)
{
    const uint32_t n = dw * dh;
    hipLaunchKernelGGL(k_display_view<OPTION>, dim3((n + 255) / 256), dim3(256), 0, s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb);
}

// ---------------------------------------------------------------- picked-instance outline (DrawPicked.hlsl + Sobel.hlsl, Display.cpp:293-400)
// The raster contract is stated in include/zetaray_amd.h (zr_pass_set_picked_instances); tests/pickcheck.py restates it in numpy.
constexpr float kGuardBand = 16.0f;     // |x|, |y| <= 16 w after clipping: snapped coordinates stay below 2^26, edge functions below 2^54
constexpr int kMaxPoly = 9;             // a triangle clipped by 6 planes
constexpr int kPickTile = 32;           // coverage tile: 32 x 32 pixels, 256 threads x 4 rows

__device__ __forceinline__ int FloorDiv256(int v) { return v >= 0 ? v / 256 : -((-v + 255) / 256); }

// one lane per triangle: vertex transform, homogeneous clipping, viewport, 16.8 snapping, fan triangulation, bounding box; the triangles that
// can cover a mask pixel are appended to `out` (two int4: x0 y0 x1 y1 | x2 y2 bx0 | by0 << 16, bx1 | by1 << 16), one atomic per wave
__global__ void __launch_bounds__(256) k_pick_setup(const zr_vertex* vertices, const uint32_t* indices, const zr_mesh_instance* instances, uint32_t inst,
    uint32_t numTris, post::PickWvp m, uint32_t dw, uint32_t dh, uint32_t rw, uint32_t rh, int4* out, uint32_t* count)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    int4 rec[2 * (kMaxPoly - 2)];
    int nOut = 0;
    if (t < numTris)
    {
        const zr_mesh_instance mi = instances[inst];
        float P[kMaxPoly][4], Q[kMaxPoly][4];
        int n = 3;
        for (int k = 0; k < 3; k++)
        {
            const zr_vertex& v = vertices[indices[mi.base_idx_offset + 3 * t + k] + mi.base_vtx_offset];
            for (int j = 0; j < 4; j++) P[k][j] = v.pos[0] * m.m[j] + v.pos[1] * m.m[4 + j] + v.pos[2] * m.m[8 + j] + m.m[12 + j];
        }
        // Sutherland-Hodgman against z >= 0, z <= w, x >= -G w, x <= G w, y >= -G w, y <= G w, in this order
        for (int plane = 0; plane < 6 && n > 0; plane++)
        {
            auto dist = [&](const float* v) -> float
            {
                switch (plane)
                {
                case 0: return v[2];
                case 1: return v[3] - v[2];
                case 2: return v[0] + kGuardBand * v[3];
                case 3: return kGuardBand * v[3] - v[0];
                case 4: return v[1] + kGuardBand * v[3];
                default: return kGuardBand * v[3] - v[1];
                }
            };
            int nq = 0;
            for (int i = 0; i < n; i++)
            {
                const float* a = P[i]; const float* b = P[i + 1 < n ? i + 1 : 0];
                const float da = dist(a), db = dist(b);
                if (da >= 0.0f) { for (int j = 0; j < 4; j++) Q[nq][j] = a[j]; nq++; }
                if ((da >= 0.0f) != (db >= 0.0f))
                {
                    const float s = da / (da - db);
                    for (int j = 0; j < 4; j++) Q[nq][j] = a[j] + s * (b[j] - a[j]);
                    nq++;
                }
            }
            n = nq;
            for (int i = 0; i < n; i++) for (int j = 0; j < 4; j++) P[i][j] = Q[i][j];
        }
        int qx[kMaxPoly], qy[kMaxPoly];
        bool ok = n >= 3;
        for (int i = 0; i < n && ok; i++)
        {
            if (!(P[i][3] > 0.0f)) { ok = false; break; }
            const float ix = P[i][0] / P[i][3], iy = P[i][1] / P[i][3];
            const float sx = (ix * 0.5f + 0.5f) * (float)dw, sy = (0.5f - iy * 0.5f) * (float)dh;
            qx[i] = (int)rintf(sx * 256.0f); qy[i] = (int)rintf(sy * 256.0f);
        }
        for (int i = 1; ok && i + 1 < n; i++)
        {
            int ax = qx[0], ay = qy[0], bx = qx[i], by = qy[i], cx = qx[i + 1], cy = qy[i + 1];
            const long long area = (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
            if (area == 0) continue;
            if (area < 0) { int tx = bx, ty = by; bx = cx; by = cy; cx = tx; cy = ty; }
            int x0 = FloorDiv256(min(ax, min(bx, cx)) - 128 + 255), x1 = FloorDiv256(max(ax, max(bx, cx)) - 128);
            int y0 = FloorDiv256(min(ay, min(by, cy)) - 128 + 255), y1 = FloorDiv256(max(ay, max(by, cy)) - 128);
            x0 = max(x0, 0); y0 = max(y0, 0); x1 = min(x1, (int)rw - 1); y1 = min(y1, (int)rh - 1);
            if (x0 > x1 || y0 > y1) continue;
            rec[2 * nOut] = make_int4(ax, ay, bx, by);
            rec[2 * nOut + 1] = make_int4(cx, cy, x0 | (y0 << 16), x1 | (y1 << 16));
            nOut++;
        }
    }
    // wave-wide exclusive scan of nOut, one atomic per wave
    const uint32_t lane = threadIdx.x & 63u;
    int incl = nOut;
    for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d, 64); if ((int)lane >= d) incl += v; }
    const int total = __shfl(incl, 63, 64);
    uint32_t base = 0;
    if (lane == 63u && total > 0) base = atomicAdd(count, (uint32_t)total);
    base = __shfl(base, 63, 64);
    const uint32_t first = base + (uint32_t)(incl - nOut);
    for (int k = 0; k < nOut; k++) { out[2 * (first + k)] = rec[2 * k]; out[2 * (first + k) + 1] = rec[2 * k + 1]; }
}

__device__ __forceinline__ bool TopLeft(int dx, int dy) { return dy < 0 || (dy == 0 && dx > 0); }
__device__ __forceinline__ bool EdgeIn(int ax, int ay, int bx, int by, int px, int py)
{
    const long long e = (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
    return e > 0 || (e == 0 && TopLeft(bx - ax, by - ay));
}

// one block per 32 x 32 tile of the mask: the triangles whose boxes meet the tile are staged in LDS 256 at a time, then every thread tests its
// four pixel centres against them.  Writes every mask pixel of the tile (255 covered, 0 not): the mask needs no separate clear.
__global__ void __launch_bounds__(256) k_pick_cover(const int4* tris, const uint32_t* count, uint32_t rw, uint32_t rh, uint8_t* mask)
{
    __shared__ int4 sTri[2 * 256];
    __shared__ uint32_t sN;
    const int tx0 = blockIdx.x * kPickTile, ty0 = blockIdx.y * kPickTile;
    const int lx = threadIdx.x % kPickTile, ly = threadIdx.x / kPickTile;
    const int px = tx0 + lx;
    bool cov[4] = {false, false, false, false};
    const uint32_t n = *count;
    for (uint32_t c = 0; c < n; c += 256)
    {
        if (threadIdx.x == 0) sN = 0;
        __syncthreads();
        const uint32_t i = c + threadIdx.x;
        if (i < n)
        {
            const int4 a = tris[2 * i], b = tris[2 * i + 1];
            const int bx0 = b.z & 0xffff, by0 = (uint32_t)b.z >> 16, bx1 = b.w & 0xffff, by1 = (uint32_t)b.w >> 16;
            if (bx0 < tx0 + kPickTile && bx1 >= tx0 && by0 < ty0 + kPickTile && by1 >= ty0)
            {
                const uint32_t slot = atomicAdd(&sN, 1u);
                sTri[2 * slot] = a; sTri[2 * slot + 1] = b;
            }
        }
        __syncthreads();
        const uint32_t m = sN;
        for (uint32_t k = 0; k < m; k++)
        {
            const int4 a = sTri[2 * k], b = sTri[2 * k + 1];
            for (int r = 0; r < 4; r++)
            {
                const int cx = px * 256 + 128, cy = (ty0 + ly + 8 * r) * 256 + 128;
                cov[r] = cov[r] || (EdgeIn(a.x, a.y, a.z, a.w, cx, cy) && EdgeIn(a.z, a.w, b.x, b.y, cx, cy) && EdgeIn(b.x, b.y, a.x, a.y, cx, cy));
            }
        }
        __syncthreads();
    }
    for (int r = 0; r < 4; r++)
    {
        const int py = ty0 + ly + 8 * r;
        if (px < (int)rw && py < (int)rh) mask[(size_t)py * rw + px] = cov[r] ? 255 : 0;
    }
}

// Sobel.hlsl mainPS over the display: CheckNeighborHood within the render size, then the Sobel gradient with out-of-range mask loads = 0.  The mask holds
// 0 / 1, so the gradients are small integers, exact in fp32, and Luminance(sqrt(gx^2 + gy^2)) > 0 exactly when (gx, gy) != 0: computed in integers.
__global__ void __launch_bounds__(256) k_pick_outline(const uint8_t* mask, uint32_t rw, uint32_t rh, uint32_t dw, uint32_t dh, F4* out, uint32_t* outSrgb, uint32_t srgb)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dw * dh) return;
    const int x = (int)(i % dw), y = (int)(i / dw);
    auto m = [&](int u, int v) -> int { return (u >= 0 && v >= 0 && u < (int)rw && v < (int)rh && mask[(size_t)v * rw + u]) ? 1 : 0; };
    bool near = false;
    for (int a = -1; a <= 1; a++) for (int b = -1; b <= 1; b++) near = near || m(x + a, y + b);
    if (!near) return;
    const int gx = -m(x - 1, y - 1) - 2 * m(x - 1, y) - m(x - 1, y + 1) + m(x + 1, y - 1) + 2 * m(x + 1, y) + m(x + 1, y + 1);
    const int gy = m(x - 1, y - 1) + 2 * m(x, y - 1) + m(x + 1, y - 1) - m(x - 1, y + 1) - 2 * m(x, y + 1) - m(x + 1, y + 1);
    if (gx == 0 && gy == 0) return;
    out[i] = f4(0.913098693f, 0.332451582f, 0.048171822f, 1.0f);
    outSrgb[i] = srgb;
}

} // namespace

namespace zr {
// one pick: setup -> coverage (the render-size mask) -> outline into the display planes.  tris: 2 x 7 int4 per triangle; count: 1 uint32
hipError_t LaunchPickOutline(hipStream_t s, const zr_vertex* vertices, const uint32_t* indices, const zr_mesh_instance* instances, uint32_t inst, uint32_t numTris,
    const post::PickWvp& m, uint32_t dw, uint32_t dh, uint32_t rw, uint32_t rh, int4* tris, uint32_t* count, uint8_t* mask, F4* out, uint32_t* outSrgb)
{
    hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (numTris) hipLaunchKernelGGL(k_pick_setup, dim3((numTris + 255) / 256), dim3(256), 0, s, vertices, indices, instances, inst, numTris, m, dw, dh, rw, rh, tris, count);
    hipLaunchKernelGGL(k_pick_cover, dim3((rw + kPickTile - 1) / kPickTile, (rh + kPickTile - 1) / kPickTile), dim3(256), 0, s, tris, count, rw, rh, mask);
    const uint32_t srgb = post::LinearToSrgb8(0.913098693f) | (post::LinearToSrgb8(0.332451582f) << 8) | (post::LinearToSrgb8(0.048171822f) << 16) | 0xff000000u;
    hipLaunchKernelGGL(k_pick_outline, dim3((dw * dh + 255) / 256), dim3(256), 0, s, mask, rw, rh, dw, dh, out, outSrgb, srgb);
    return hipGetLastError();
}

// option: 1 .. 9 (ZR_DISPLAY_BASE_COLOR .. ZR_DISPLAY_DEPTH); gb: the current planes at render size, tile origin 0
hipError_t LaunchDisplayView(hipStream_t s, int option, const GBuf& gb, uint32_t dw, uint32_t dh, float cameraNear, float roughnessTh, F4* out, uint32_t* outSrgb)
{
    switch (option)
    {
    case V_BASE_COLOR: Launch<V_BASE_COLOR>(s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb); break;
    case V_NORMAL: Launch<V_NORMAL>(s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb); break;
    case V_METALNESS_ROUGHNESS: Launch<V_METALNESS_ROUGHNESS>(s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb); break;
    case V_COAT_WEIGHT: Launch<V_COAT_WEIGHT>(s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb); break;
    case V_COAT_COLOR: Launch<V_COAT_COLOR>(s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb); break;
    case V_ROUGHNESS_TH: Launch<V_ROUGHNESS_TH>(s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb); break;
    case V_EMISSIVE: Launch<V_EMISSIVE>(s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb); break;
    case V_TRANSMISSION: Launch<V_TRANSMISSION>(s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb); break;
    case V_DEPTH: Launch<V_DEPTH>(s, gb, dw, dh, cameraNear, roughnessTh, out, outSrgb); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
} // namespace zr
