// bmfr_upsample.hip -- guided upsampling (bmfr_upsample_output, include/bmfr.h):
// one kernel from the context's filtered_accumulated at W x H and a renderer's
// display-resolution guides to a surface at Wd x Hd.  No reference counterpart;
// the formulas are the ones the header documents, each line one f32 operation
// (-ffp-contract=off, correctly rounded division and square root).
//
// Shape: a work-group of 64 x 4 threads takes a display tile of 64 x 4 pixels,
// one pixel per thread, and walks down the frame in steps of gridDim.y tiles.
// A wave is 64 consecutive pixels of one display row: its guide loads and its
// surface store are consecutive elements (4 .. 12 bytes per lane), and its four
// taps of the three low-resolution planes fall into at most 65 consecutive
// pixels of two rows, which the work-group's other waves and its neighbours
// share through the vector cache and the L2 (DESIGN.md "Guided upsampling").
// Every tap is loaded -- its address is clamped into the plane -- and a tap of
// weight 0 is left out of the sums by a select.  Low-resolution addresses are
// the plane's base plus a 32-bit byte offset (bmfr_create bounds planes at
// 4 GiB); display-resolution offsets are 64-bit.  The surface format is a
// template parameter; source, guided / unguided, the guide formats, bgr and
// flip_y are wave-uniform run-time switches.  No LDS.
#include "../../include/bmfr.h"
#include "bmfr_pixel_io.h"
#include "bmfr_powr.h"
#include "bmfr_upsample.h"

namespace bmfr {
namespace {

constexpr int kTileW = 64, kTileH = 4;

// Pixel i (byte offset i * 12, or i * 6 of a half3 plane) of a frame plane as f32.
__device__ __forceinline__ void ld_frame(const void* base, bool half, uint32_t i, float (&c)[3]) {
    uint32_t e[3];
    if (half) {
        ld_elems<_Float16, 1, false>(base, i, e);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = half_to_float(e[k]);
    } else {
        ld_elems<float, 1, false>(base, i, e);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = __uint_as_float(e[k]);
    }
}

// Display pixel (X, Y), inside the frame.
template <int FMT>
__device__ __forceinline__ void upsample_pixel(const UpsampleArgs& a, int X, int Y) {
    const size_t di = (size_t)Y * (size_t)a.Wd + (size_t)X;  // flat display pixel
    const bool guided = a.normals != nullptr;

    // 1. footprint
    const float u = ((float)X + 0.5f) * a.rx - 0.5f, v = ((float)Y + 0.5f) * a.ry - 0.5f;
    const float x0 = __builtin_floorf(u), y0 = __builtin_floorf(v);
    const float fx = u - x0, fy = v - y0;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const int ix = (int)x0, iy = (int)y0;  // -1 .. W - 1, -1 .. H - 1
    const int xs[2] = {min(max(ix, 0), a.W - 1), min(max(ix + 1, 0), a.W - 1)};
    const int ys[2] = {min(max(iy, 0), a.H - 1), min(max(iy + 1, 0), a.H - 1)};
    const float w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
    uint32_t tap[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) tap[k] = (uint32_t)ys[k >> 1] * (uint32_t)a.W + (uint32_t)xs[k & 1];

    // 2. display guides
    float A[3];
    ld_channels(a.albedo, a.albedo_fmt, di, A);
    float N[3] = {}, P[3] = {};
    if (guided) {
        if (a.normal_fmt == BMFR_FORMAT_OCT_SNORM16X2) {
            uint32_t wd;
            ld_bytes<4, 4>(a.normals, di * 4u, &wd);
            oct_decode(wd, N);
        } else {
            ld_channels(a.normals, a.normal_fmt, di, N);
        }
        if (a.positions) {
            ld_channels(a.positions, BMFR_FORMAT_F32X3, di, P);
        } else {
            uint32_t wd;
            ld_bytes<4, 4>(a.depth, di * 4u, &wd);
            position_from_depth(a.m, __uint_as_float(wd), (float)X, (float)Y, a.jx, a.jy1, (float)a.Wd, (float)a.Hd, P);
        }
    }

    // 3., 4. tap test and sums: over the accepted taps, and over every tap of weight > 0
    // (-0 + t = t for every t, -0 included: a sum begins with its first term)
    float sw = -0.0f, sc[3] = {-0.0f, -0.0f, -0.0f};
    float tw = -0.0f, tc[3] = {-0.0f, -0.0f, -0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float e[3];
        ld_frame(a.acc, false, tap[k], e);
        const bool live = w[k] > 0.0f;
        bool ok = live;
        if (guided) {
            float n[3], p[3];
            ld_frame(a.f_normals, a.frame_half != 0, tap[k], n);
            ld_frame(a.f_positions, a.frame_half != 0, tap[k], p);
            const float dpx = p[0] - P[0], dpy = p[1] - P[1], dpz = p[2] - P[2];
            const float d = (dpx * N[0] + dpy * N[1]) + dpz * N[2];
            const float dnx = n[0] - N[0], dny = n[1] - N[1], dnz = n[2] - N[2];
            const float q = (dnx * dnx + dny * dny) + dnz * dnz;
            ok = live && d * d < a.plane_limit_sq && q < a.normal_limit_sq;
        }
        const float t[3] = {w[k] * e[0], w[k] * e[1], w[k] * e[2]};
        const float sw1 = sw + w[k], tw1 = tw + w[k];
        sw = ok ? sw1 : sw;
        tw = live ? tw1 : tw;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float s1 = sc[c] + t[c], t1 = tc[c] + t[c];
            sc[c] = ok ? s1 : sc[c];
            tc[c] = live ? t1 : tc[c];
        }
    }
    const bool fell = !(sw > 0.0f);  // guided only: unguided sums are the same two
    if (fell && guided && a.stats) atomicAdd(a.stats, 1u);

    // 6. source value
    float val[3];
    const float den = fell ? tw : sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float e = (fell ? tc[c] : sc[c]) / den;
        val[c] = A[c] * e;
    }
    if (a.tonemapped) {
#pragma unroll
        for (int c = 0; c < 3; ++c) val[c] = gamma_clamped(val[c]);
    }
    if (a.surf.bgr) {
        const float t = val[0];
        val[0] = val[2];
        val[2] = t;
    }
    st_surface<FMT>(surface_pixel<FMT>(a.surf, X, Y), val, a.surf.alpha);
}

template <int FMT>
__global__ __launch_bounds__(kTileW * kTileH) void upsample_kernel(const UpsampleArgs a) {
    const int X = blockIdx.x * kTileW + threadIdx.x;
    if (X >= a.Wd) return;
    for (int Y = blockIdx.y * kTileH + threadIdx.y; Y < a.Hd; Y += gridDim.y * kTileH) upsample_pixel<FMT>(a, X, Y);
}

}  // namespace

hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t st) {
    if (a.Wd <= 0 || a.Hd <= 0) return hipErrorInvalidValue;
    const int rows = (a.Hd + kTileH - 1) / kTileH;
    const dim3 grid((a.Wd + kTileW - 1) / kTileW, rows < 65535 ? rows : 65535);
    const bool listed = dispatch_surface_format(a.surf.format, [&](auto fmt) {
        hipLaunchKernelGGL(upsample_kernel<decltype(fmt)::value>, grid, dim3(kTileW, kTileH), 0, st, a);
    });
    if (!listed) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace bmfr
