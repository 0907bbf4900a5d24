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
#include "bmfr_powr.h"
#include "bmfr_upsample.h"

namespace bmfr {
namespace {

constexpr int kTileW = 64, kTileH = 4;

// bytes per pixel / natural alignment of a surface format
template <int FMT>
constexpr int kBpp = FMT == BMFR_FORMAT_F32X3 ? 12 : FMT == BMFR_FORMAT_F16X4 ? 8 : FMT == BMFR_FORMAT_UNORM8X3 ? 3 : 4;
template <int FMT>
constexpr int kNatural = FMT == BMFR_FORMAT_F16X4 ? 8 : FMT == BMFR_FORMAT_UNORM8X3 ? 1 : 4;

// BYTES at p into / out of 32-bit words (the last word may be partial).
template <int BYTES, int ALIGN>
__device__ __forceinline__ void ld_bytes(const void* base, size_t off, uint32_t* w) {
    const char* p = reinterpret_cast<const char*>(base) + off;
    __builtin_memcpy(w, __builtin_assume_aligned(p, ALIGN), BYTES);
}
template <int BYTES, int ALIGN>
__device__ __forceinline__ void st_bytes(char* p, const uint32_t* w) {
    __builtin_memcpy(__builtin_assume_aligned(p, ALIGN), w, BYTES);
}
__device__ __forceinline__ float half_to_float(uint32_t bits) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}
__device__ __forceinline__ uint32_t float_to_half(float v) {
    return __builtin_bit_cast(uint16_t, (_Float16)v);  // round to nearest even; overflow -> inf
}
// c = v > 0 ? (v < 1 ? v : 1) : 0;  q = (uint)floorf(c * scale + 0.5f)
__device__ __forceinline__ uint32_t unorm(float v, float scale) {
    const float c = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
    return (uint32_t)__builtin_floorf(c * scale + 0.5f);
}

// Pixel i of a three-channel guide plane (F32X3, F16X4, UNORM8X4) as f32.
__device__ __forceinline__ void ld_channels(const void* base, int fmt, size_t i, float (&c)[3]) {
    if (fmt == BMFR_FORMAT_F32X3) {
        uint32_t w[3];
        ld_bytes<12, 4>(base, i * 12u, w);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = __uint_as_float(w[k]);
    } else if (fmt == BMFR_FORMAT_F16X4) {
        uint32_t w[2];
        ld_bytes<8, 8>(base, i * 8u, w);
        c[0] = half_to_float(w[0] & 0xffffu);
        c[1] = half_to_float(w[0] >> 16);
        c[2] = half_to_float(w[1] & 0xffffu);
    } else {  // BMFR_FORMAT_UNORM8X4
        uint32_t w;
        ld_bytes<4, 4>(base, i * 4u, &w);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (float)((w >> (8 * k)) & 255u) / 255.0f;
    }
}

// One octahedral snorm16 component.
__device__ __forceinline__ float snorm16(uint32_t bits) {
    const float e = (float)(int16_t)(uint16_t)bits / 32767.0f;
    return e < -1.0f ? -1.0f : e;
}

// Pixel i (byte offset i * 12, or i * 6 of a half3 plane) of a frame plane as f32.
__device__ __forceinline__ void ld_frame(const void* base, bool half, uint32_t i, float (&c)[3]) {
    if (half) {
        uint32_t w[2] = {};
        ld_bytes<6, 2>(base, i * 6u, w);
        c[0] = half_to_float(w[0] & 0xffffu);
        c[1] = half_to_float(w[0] >> 16);
        c[2] = half_to_float(w[1] & 0xffffu);
    } else {
        uint32_t w[3];
        ld_bytes<12, 4>(base, i * 12u, w);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = __uint_as_float(w[k]);
    }
}

// One pixel's source value into the surface at p (bmfr_resolve.hip's encoding).
template <int FMT>
__device__ __forceinline__ void st_pixel(const float (&v)[3], float alpha, char* p) {
    uint32_t o[(kBpp<FMT> + 3) / 4] = {};
    if constexpr (FMT == BMFR_FORMAT_F32X3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = __float_as_uint(v[k]);
    } else if constexpr (FMT == BMFR_FORMAT_F16X4) {
        o[0] = float_to_half(v[0]) | (float_to_half(v[1]) << 16);
        o[1] = float_to_half(v[2]) | (float_to_half(alpha) << 16);
    } else if constexpr (FMT == BMFR_FORMAT_UNORM8X4) {
        o[0] = unorm(v[0], 255.0f) | (unorm(v[1], 255.0f) << 8) | (unorm(v[2], 255.0f) << 16) |
               (unorm(alpha, 255.0f) << 24);
    } else if constexpr (FMT == BMFR_FORMAT_UNORM10X3A2) {
        o[0] = unorm(v[0], 1023.0f) | (unorm(v[1], 1023.0f) << 10) | (unorm(v[2], 1023.0f) << 20) |
               (unorm(alpha, 3.0f) << 30);
    } else {  // BMFR_FORMAT_UNORM8X3
        o[0] = unorm(v[0], 255.0f) | (unorm(v[1], 255.0f) << 8) | (unorm(v[2], 255.0f) << 16);
    }
    st_bytes<kBpp<FMT>, kNatural<FMT>>(p, o);
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
            const float ex = snorm16(wd & 0xffffu), ey = snorm16(wd >> 16);
            const float ax = __builtin_fabsf(ex), ay = __builtin_fabsf(ey);
            const float z = (1.0f - ax) - ay;
            float ox = ex, oy = ey;
            if (z < 0.0f) {
                ox = (1.0f - ay) * (ex >= 0.0f ? 1.0f : -1.0f);
                oy = (1.0f - ax) * (ey >= 0.0f ? 1.0f : -1.0f);
            }
            const float len = __builtin_sqrtf((ox * ox + oy * oy) + z * z);
            N[0] = ox / len;
            N[1] = oy / len;
            N[2] = z / len;
        } else {
            ld_channels(a.normals, a.normal_fmt, di, N);
        }
        if (a.positions) {
            ld_channels(a.positions, BMFR_FORMAT_F32X3, di, P);
        } else {
            uint32_t wd;
            ld_bytes<4, 4>(a.depth, di * 4u, &wd);
            const float depth = __uint_as_float(wd);
            const float sx = (float)X + a.jx, sy = (float)Y + a.jy1;
            const float nx = (sx / (float)a.Wd) * 2.0f - 1.0f, ny = (sy / (float)a.Hd) * 2.0f - 1.0f;
            float h[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = ((a.m[i] * nx + a.m[4 + i] * ny) + a.m[8 + i] * depth) + a.m[12 + i];
#pragma unroll
            for (int i = 0; i < 3; ++i) P[i] = h[i] / h[3];
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
    if (a.bgr) {
        const float t = val[0];
        val[0] = val[2];
        val[2] = t;
    }
    char* p = reinterpret_cast<char*>(a.dst) + (long long)(a.dy0 + Y * a.dy_step) * a.pitch +
              (long long)(a.dx0 + X) * kBpp<FMT>;
    st_pixel<FMT>(val, a.alpha, p);
}

template <int FMT>
__global__ __launch_bounds__(kTileW * kTileH) void upsample_kernel(const UpsampleArgs a) {
    const int X = blockIdx.x * kTileW + threadIdx.x;
    if (X >= a.Wd) return;
    for (int Y = blockIdx.y * kTileH + threadIdx.y; Y < a.Hd; Y += gridDim.y * kTileH) upsample_pixel<FMT>(a, X, Y);
}

template <int FMT>
void launch(const UpsampleArgs& a, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(upsample_kernel<FMT>, grid, dim3(kTileW, kTileH), 0, st, a);
}

}  // namespace

hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t st) {
    if (a.Wd <= 0 || a.Hd <= 0) return hipErrorInvalidValue;
    const int rows = (a.Hd + kTileH - 1) / kTileH;
    const dim3 grid((a.Wd + kTileW - 1) / kTileW, rows < 65535 ? rows : 65535);
    switch (a.format) {
    case BMFR_FORMAT_F32X3: launch<BMFR_FORMAT_F32X3>(a, grid, st); break;
    case BMFR_FORMAT_F16X4: launch<BMFR_FORMAT_F16X4>(a, grid, st); break;
    case BMFR_FORMAT_UNORM8X4: launch<BMFR_FORMAT_UNORM8X4>(a, grid, st); break;
    case BMFR_FORMAT_UNORM8X3: launch<BMFR_FORMAT_UNORM8X3>(a, grid, st); break;
    case BMFR_FORMAT_UNORM10X3A2: launch<BMFR_FORMAT_UNORM10X3A2>(a, grid, st); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace bmfr
