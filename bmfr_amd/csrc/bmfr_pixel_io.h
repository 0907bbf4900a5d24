// bmfr_pixel_io.h -- the one place a bmfr_format (include/bmfr.h) is decoded
// or encoded on the device: raw access, element and G-buffer decoders, the
// surface encoder and the surface placement the edge stages share
// (bmfr_prepare.hip, bmfr_firefly.hip, bmfr_resolve.hip, bmfr_upsample.hip,
// bmfr_display_taa.hip).  Each arithmetic line is one f32 operation
// (-ffp-contract=off, correctly rounded / and sqrt) in the order and grouping
// the public header documents and tests/*_np.py restate.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/bmfr.h"

namespace bmfr {

// ---------------------------------------------------------------- raw access
// BYTES at base + off into / out of 32-bit words (the last word may be
// partial).  OFF is the caller's offset type: a 32-bit byte offset from a base
// in SGPRs (planes bmfr_create bounds at 4 GiB), or a 64-bit one.  ALIGN is
// what the address is a multiple of, the element's alignment at least: global
// accesses of gfx950 take any address, so an access is as wide as BYTES allow.
template <int BYTES, int ALIGN, class OFF>
__device__ __forceinline__ void ld_bytes(const void* base, OFF off, uint32_t* w) {
    const char* p = reinterpret_cast<const char*>(base) + off;
    __builtin_memcpy(w, __builtin_assume_aligned(p, ALIGN), BYTES);
}
template <int BYTES, int ALIGN, class OFF>
__device__ __forceinline__ void st_bytes(void* base, OFF off, const uint32_t* w) {
    char* p = reinterpret_cast<char*>(base) + off;
    __builtin_memcpy(__builtin_assume_aligned(p, ALIGN), w, BYTES);
}

// Alignment of an access of BYTES at a group's (WIDE) or a pixel's offset;
// NATURAL: the element's own alignment.
template <int BYTES, bool WIDE, int NATURAL>
constexpr int kAlign = !WIDE ? NATURAL : (BYTES % 16 == 0 ? 16 : (BYTES % 8 == 0 ? 8 : NATURAL));

// ------------------------------------------------------------------ elements
// 16-bit element k of packed words.
__device__ __forceinline__ uint32_t u16_at(const uint32_t* w, int k) { return (w[k >> 1] >> (16 * (k & 1))) & 0xffffu; }
__device__ __forceinline__ float half_to_float(uint32_t bits) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}
__device__ __forceinline__ uint32_t float_to_half(float v) {
    return __builtin_bit_cast(uint16_t, (_Float16)v);  // round to nearest even; overflow -> inf
}

// One element's bits (f32, or half in the low 16) <-> f32.
template <class T>
__device__ __forceinline__ uint32_t encode(float v) {
    if constexpr (sizeof(T) == 4) return __float_as_uint(v);
    else return float_to_half(v);
}
template <class T>
__device__ __forceinline__ float decode(uint32_t bits) {
    if constexpr (sizeof(T) == 4) return __uint_as_float(bits);
    else return half_to_float(bits);
}

// Pixels of a float3 / half3 plane a thread takes with 16-byte accesses (48 B).
template <class T>
constexpr int kGroup = sizeof(T) == 4 ? 4 : 8;

// N pixels of a float3 / half3 plane from pixel `first`, as element bits
// (e[N * 3]); WIDE: the run is a group, 16-byte aligned.
template <class T, int N, bool WIDE>
__device__ __forceinline__ void ld_elems(const void* base, uint32_t first, uint32_t* e) {
    constexpr int BYTES = N * 3 * (int)sizeof(T);
    uint32_t w[(BYTES + 3) / 4] = {};
    ld_bytes<BYTES, kAlign<BYTES, WIDE, (int)sizeof(T)>>(base, first * (uint32_t)(3 * sizeof(T)), w);
#pragma unroll
    for (int i = 0; i < N * 3; ++i) e[i] = sizeof(T) == 4 ? w[i] : u16_at(w, i);
}
template <class T, int N, bool WIDE>
__device__ __forceinline__ void st_elems(void* base, uint32_t first, const uint32_t* e) {
    constexpr int BYTES = N * 3 * (int)sizeof(T);
    uint32_t w[(BYTES + 3) / 4] = {};
#pragma unroll
    for (int i = 0; i < N * 3; ++i) {
        if constexpr (sizeof(T) == 4) w[i] = e[i];
        else w[i >> 1] |= e[i] << (16 * (i & 1));
    }
    st_bytes<BYTES, kAlign<BYTES, WIDE, (int)sizeof(T)>>(base, first * (uint32_t)(3 * sizeof(T)), w);
}

// ------------------------------------------------------------------ decoders
// N pixels from pixel `first` of a three-channel G-buffer plane (F32X3, F16X4,
// UNORM8X4) as f32.
template <int N, bool WIDE, class OFF>
__device__ __forceinline__ void ld_channels(const void* base, int fmt, OFF first, float (&c)[N][3]) {
    if (fmt == BMFR_FORMAT_F32X3) {
        uint32_t w[N * 3];
        ld_bytes<N * 12, kAlign<N * 12, WIDE, 4>>(base, first * 12u, w);
#pragma unroll
        for (int i = 0; i < N * 3; ++i) c[i / 3][i % 3] = __uint_as_float(w[i]);
    } else if (fmt == BMFR_FORMAT_F16X4) {
        uint32_t w[N * 2];
        ld_bytes<N * 8, kAlign<N * 8, WIDE, 8>>(base, first * 8u, w);
#pragma unroll
        for (int i = 0; i < N * 3; ++i) c[i / 3][i % 3] = half_to_float(u16_at(w, 4 * (i / 3) + i % 3));
    } else {  // BMFR_FORMAT_UNORM8X4
        uint32_t w[N];
        ld_bytes<N * 4, kAlign<N * 4, WIDE, 4>>(base, first * 4u, w);
#pragma unroll
        for (int i = 0; i < N * 3; ++i) c[i / 3][i % 3] = (float)((w[i / 3] >> (8 * (i % 3))) & 255u) / 255.0f;
    }
}
// Pixel i alone.
template <class OFF>
__device__ __forceinline__ void ld_channels(const void* base, int fmt, OFF i, float (&c)[3]) {
    ld_channels<1, false>(base, fmt, i, reinterpret_cast<float(&)[1][3]>(c));
}

// One octahedral snorm16 component.
__device__ __forceinline__ float snorm16(uint32_t bits) {
    const float e = (float)(int16_t)(uint16_t)bits / 32767.0f;
    return e < -1.0f ? -1.0f : e;
}
// The unit normal of an OCT_SNORM16X2 word.
__device__ __forceinline__ void oct_decode(uint32_t word, float (&n)[3]) {
    const float ex = snorm16(word & 0xffffu), ey = snorm16(word >> 16);
    const float ax = __builtin_fabsf(ex), ay = __builtin_fabsf(ey);
    const float z = (1.0f - ax) - ay;
    float ox = ex, oy = ey;
    if (z < 0.0f) {
        ox = (1.0f - ay) * (ex >= 0.0f ? 1.0f : -1.0f);
        oy = (1.0f - ax) * (ey >= 0.0f ? 1.0f : -1.0f);
    }
    const float len = __builtin_sqrtf((ox * ox + oy * oy) + z * z);
    n[0] = ox / len;
    n[1] = oy / len;
    n[2] = z / len;
}

// World position of pixel (fx, fy) of an fW x fH frame from its depth:
// m = inv_view_proj, column-major; jx, jy1 = pixel_offset[0], 1 - pixel_offset[1].
__device__ __forceinline__ void position_from_depth(const float (&m)[16], float depth, float fx, float fy, float jx,
                                                    float jy1, float fW, float fH, float (&pos)[3]) {
    const float sx = fx + jx, sy = fy + jy1;
    const float nx = (sx / fW) * 2.0f - 1.0f, ny = (sy / fH) * 2.0f - 1.0f;
    float h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = ((m[i] * nx + m[4 + i] * ny) + m[8 + i] * depth) + m[12 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pos[i] = h[i] / h[3];
}

// N pixels' motion vectors from pixel `first` of an F32X2 / F16X2 plane (a
// pixel's F32X2 entry is 4-byte aligned: bmfr_display_taa asks no more).
template <int N, bool WIDE, class OFF>
__device__ __forceinline__ void ld_motion(const void* base, int fmt, OFF first, float (&mv)[N][2]) {
    if (fmt == BMFR_FORMAT_F32X2) {
        uint32_t w[N * 2];
        ld_bytes<N * 8, kAlign<N * 8, WIDE, 4>>(base, first * 8u, w);
#pragma unroll
        for (int i = 0; i < N * 2; ++i) mv[i / 2][i % 2] = __uint_as_float(w[i]);
    } else {  // BMFR_FORMAT_F16X2
        uint32_t w[N];
        ld_bytes<N * 4, kAlign<N * 4, WIDE, 4>>(base, first * 4u, w);
#pragma unroll
        for (int i = 0; i < N * 2; ++i) mv[i / 2][i % 2] = half_to_float(u16_at(w, i));
    }
}
// Pixel i alone.
template <class OFF>
__device__ __forceinline__ void ld_motion(const void* base, int fmt, OFF i, float (&mv)[2]) {
    ld_motion<1, false>(base, fmt, i, reinterpret_cast<float(&)[1][2]>(mv));
}

// prev_pixel of pixel (fx, fy) from its motion vector: motion_scale, and with
// motion_at_pixel_centre (`centre`) the pixel's centre and the jitter.
__device__ __forceinline__ void previous_position(float mvx, float mvy, float mscale_x, float mscale_y, bool centre,
                                                  float fx, float fy, float jx, float jy1, float& pfx, float& pfy) {
    const float mx = mvx * mscale_x, my = mvy * mscale_y;
    if (centre) {
        pfx = ((fx + 0.5f) - mx) - jx;
        pfy = ((fy + 0.5f) - my) - jy1;
    } else {
        pfx = fx - mx;
        pfy = fy - my;
    }
}

// ------------------------------------------------------------------- surface
// bytes per pixel / natural alignment of a surface format
template <int FMT>
constexpr int kBpp = FMT == BMFR_FORMAT_F32X3 ? 12 : FMT == BMFR_FORMAT_F16X4 ? 8 : FMT == BMFR_FORMAT_UNORM8X3 ? 3 : 4;
template <int FMT>
constexpr int kNatural = FMT == BMFR_FORMAT_F16X4 ? 8 : FMT == BMFR_FORMAT_UNORM8X3 ? 1 : 4;

// c = v > 0 ? (v < 1 ? v : 1) : 0;  q = (uint)floorf(c * scale + 0.5f)
__device__ __forceinline__ uint32_t unorm(float v, float scale) {
    const float c = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
    return (uint32_t)__builtin_floorf(c * scale + 0.5f);
}

// N consecutive pixels' values (in the surface's channel order) and the
// surface's alpha as the N * kBpp<FMT> bytes of the surface, in words.
template <int FMT, int N>
__device__ __forceinline__ void encode_surface(const float (&v)[N][3], float alpha, uint32_t (&o)[(N * kBpp<FMT> + 3) / 4]) {
#pragma unroll
    for (int i = 0; i < (N * kBpp<FMT> + 3) / 4; ++i) o[i] = 0;
    if constexpr (FMT == BMFR_FORMAT_F32X3) {
#pragma unroll
        for (int i = 0; i < N * 3; ++i) o[i] = __float_as_uint(v[i / 3][i % 3]);
    } else if constexpr (FMT == BMFR_FORMAT_F16X4) {
        const uint32_t ha = float_to_half(alpha);
#pragma unroll
        for (int q = 0; q < N; ++q) {
            o[2 * q] = float_to_half(v[q][0]) | (float_to_half(v[q][1]) << 16);
            o[2 * q + 1] = float_to_half(v[q][2]) | (ha << 16);
        }
    } else if constexpr (FMT == BMFR_FORMAT_UNORM8X4) {
        const uint32_t qa = unorm(alpha, 255.0f) << 24;
#pragma unroll
        for (int q = 0; q < N; ++q)
            o[q] = unorm(v[q][0], 255.0f) | (unorm(v[q][1], 255.0f) << 8) | (unorm(v[q][2], 255.0f) << 16) | qa;
    } else if constexpr (FMT == BMFR_FORMAT_UNORM10X3A2) {
        const uint32_t qa = unorm(alpha, 3.0f) << 30;
#pragma unroll
        for (int q = 0; q < N; ++q)
            o[q] = unorm(v[q][0], 1023.0f) | (unorm(v[q][1], 1023.0f) << 10) | (unorm(v[q][2], 1023.0f) << 20) | qa;
    } else {  // BMFR_FORMAT_UNORM8X3
#pragma unroll
        for (int i = 0; i < N * 3; ++i) o[i >> 2] |= unorm(v[i / 3][i % 3], 255.0f) << (8 * (i & 3));
    }
}
// ... stored at p, a multiple of the element's alignment only: the store is as
// wide as the pixels (16 B stores for 16 / 32 / 48 B, one 12 B store for four
// UNORM8X3 pixels) wherever it lands.
template <int FMT, int N>
__device__ __forceinline__ void st_surface(char* p, const float (&v)[N][3], float alpha) {
    uint32_t o[(N * kBpp<FMT> + 3) / 4];
    encode_surface<FMT, N>(v, alpha, o);
    st_bytes<N * kBpp<FMT>, kNatural<FMT>>(p, 0u, o);
}
// One pixel.
template <int FMT>
__device__ __forceinline__ void st_surface(char* p, const float (&v)[3], float alpha) {
    st_surface<FMT, 1>(p, reinterpret_cast<const float(&)[1][3]>(v), alpha);
}

// Where a stage's W x H rectangle lies in a bmfr_surface (include/bmfr.h);
// filled and bounds-checked by the C ABI.
struct SurfaceDst {
    void* dst;        // surface pixel (0, 0); null: no surface (bmfr_display_taa)
    long long pitch;  // bytes between surface rows
    float alpha;
    int format;       // bmfr_format of the surface
    int bgr;
    int dx0, dy0;     // surface pixel of the rectangle's pixel (0, 0)
    int dy_step;      // +1, or -1 with flip_y: surface row of rectangle row Y is dy0 + Y * dy_step
};

// The surface address of the rectangle's pixel (X, Y).
template <int FMT>
__device__ __forceinline__ char* surface_pixel(const SurfaceDst& s, int X, int Y) {
    return reinterpret_cast<char*>(s.dst) + (long long)(s.dy0 + Y * s.dy_step) * s.pitch +
           (long long)(s.dx0 + X) * kBpp<FMT>;
}

// f(std::integral_constant<int, FMT>) for the surface format `format`; false
// (and no call) for a format no surface has.
template <class F>
bool dispatch_surface_format(int format, F&& f) {
    switch (format) {
    case BMFR_FORMAT_F32X3: f(std::integral_constant<int, BMFR_FORMAT_F32X3>{}); return true;
    case BMFR_FORMAT_F16X4: f(std::integral_constant<int, BMFR_FORMAT_F16X4>{}); return true;
    case BMFR_FORMAT_UNORM8X4: f(std::integral_constant<int, BMFR_FORMAT_UNORM8X4>{}); return true;
    case BMFR_FORMAT_UNORM8X3: f(std::integral_constant<int, BMFR_FORMAT_UNORM8X3>{}); return true;
    case BMFR_FORMAT_UNORM10X3A2: f(std::integral_constant<int, BMFR_FORMAT_UNORM10X3A2>{}); return true;
    default: return false;
    }
}

}  // namespace bmfr
