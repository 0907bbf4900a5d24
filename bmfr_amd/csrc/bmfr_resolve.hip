// bmfr_resolve.hip -- the output back end (bmfr_resolve_output, include/bmfr.h):
// one streaming kernel from the context's state planes to a renderer's
// surface.  No reference counterpart (the reference reads the float3 result
// back and quantises on the CPU); the formulas are the ones the header
// documents, each line one f32 operation (-ffp-contract=off).
//
// Shape: a 2-D launch, blockIdx.y over the tile's rows.  Within a row a thread
// takes four consecutive pixels whose SOURCE group is 16-byte aligned (flat
// region pixel index = 0 mod 4: three 16-byte loads of the float3 plane, and
// three more -- or 24 bytes, 8-byte aligned, of a half3 plane -- of the albedo) and
// stores them as 16 / 32 / 48 / 12 bytes at the destination's own alignment.
// The pixels before the row's first and after its last whole group, or every
// pixel when a source plane is not 16-byte aligned, go one per thread with
// element-sized accesses.  Source addresses are the plane's base plus a 32-bit
// byte offset (bmfr_create bounds planes at 4 GiB); the destination offset is
// 64-bit (row * pitch).  The surface format is a template parameter; source,
// bgr and flip_y are wave-uniform run-time switches.  No LDS.
#include "../../include/bmfr.h"
#include "bmfr_resolve.h"

namespace bmfr {
namespace {

constexpr int kResolveThreads = 256;
constexpr int kGroup = 4;

// bytes per pixel / natural alignment of a surface format
template <int FMT>
constexpr int kBpp = FMT == BMFR_FORMAT_F32X3 ? 12 : FMT == BMFR_FORMAT_F16X4 ? 8 : FMT == BMFR_FORMAT_UNORM8X3 ? 3 : 4;
template <int FMT>
constexpr int kNatural = FMT == BMFR_FORMAT_F16X4 ? 8 : FMT == BMFR_FORMAT_UNORM8X3 ? 1 : 4;

// BYTES at base + off into 32-bit words (the last word may be partial).
template <int BYTES, int ALIGN>
__device__ __forceinline__ void ld_bytes(const void* base, uint32_t off, uint32_t* w) {
    const char* p = reinterpret_cast<const char*>(base) + off;
    __builtin_memcpy(w, __builtin_assume_aligned(p, ALIGN), BYTES);
}
// BYTES at p, a multiple of the element's alignment only: global accesses of
// gfx950 take any address, so the group's store is as wide as the group (16 B
// stores for 16 / 32 / 48 B, one 12 B store for UNORM8X3) wherever it lands.
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

// N consecutive pixels of a row: flat region pixel index `first`, surface address p.
template <int FMT, int N, bool WIDE>
__device__ __forceinline__ void resolve_pixels(const ResolveArgs& a, uint32_t first, char* p) {
    float v[N][3];
    {
        uint32_t w[N * 3];
        ld_bytes<N * 12, WIDE ? 16 : 4>(a.src, first * 12u, w);
#pragma unroll
        for (int i = 0; i < N * 3; ++i) v[i / 3][i % 3] = __uint_as_float(w[i]);
    }
    if (a.albedo) {  // BMFR_RESOLVE_HDR: v = a * f
        float al[N][3];
        if (a.albedo_half) {
            uint32_t w[(N * 6 + 3) / 4] = {};
            ld_bytes<N * 6, WIDE ? 8 : 2>(a.albedo, first * 6u, w);
#pragma unroll
            for (int i = 0; i < N * 3; ++i) al[i / 3][i % 3] = half_to_float((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
        } else {
            uint32_t w[N * 3];
            ld_bytes<N * 12, WIDE ? 16 : 4>(a.albedo, first * 12u, w);
#pragma unroll
            for (int i = 0; i < N * 3; ++i) al[i / 3][i % 3] = __uint_as_float(w[i]);
        }
#pragma unroll
        for (int i = 0; i < N * 3; ++i) v[i / 3][i % 3] = al[i / 3][i % 3] * v[i / 3][i % 3];
    }
    if (a.bgr) {
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const float t = v[q][0];
            v[q][0] = v[q][2];
            v[q][2] = t;
        }
    }

    constexpr int BYTES = N * kBpp<FMT>;
    uint32_t o[(BYTES + 3) / 4] = {};
    if constexpr (FMT == BMFR_FORMAT_F32X3) {
#pragma unroll
        for (int i = 0; i < N * 3; ++i) o[i] = __float_as_uint(v[i / 3][i % 3]);
    } else if constexpr (FMT == BMFR_FORMAT_F16X4) {
        const uint32_t ha = float_to_half(a.alpha);
#pragma unroll
        for (int q = 0; q < N; ++q) {
            o[2 * q] = float_to_half(v[q][0]) | (float_to_half(v[q][1]) << 16);
            o[2 * q + 1] = float_to_half(v[q][2]) | (ha << 16);
        }
    } else if constexpr (FMT == BMFR_FORMAT_UNORM8X4) {
        const uint32_t qa = unorm(a.alpha, 255.0f) << 24;
#pragma unroll
        for (int q = 0; q < N; ++q)
            o[q] = unorm(v[q][0], 255.0f) | (unorm(v[q][1], 255.0f) << 8) | (unorm(v[q][2], 255.0f) << 16) | qa;
    } else if constexpr (FMT == BMFR_FORMAT_UNORM10X3A2) {
        const uint32_t qa = unorm(a.alpha, 3.0f) << 30;
#pragma unroll
        for (int q = 0; q < N; ++q)
            o[q] = unorm(v[q][0], 1023.0f) | (unorm(v[q][1], 1023.0f) << 10) | (unorm(v[q][2], 1023.0f) << 20) | qa;
    } else {  // BMFR_FORMAT_UNORM8X3
#pragma unroll
        for (int i = 0; i < N * 3; ++i) o[i >> 2] |= unorm(v[i / 3][i % 3], 255.0f) << (8 * (i & 3));
    }
    st_bytes<BYTES, kNatural<FMT>>(p, o);
}

template <int FMT>
__global__ __launch_bounds__(kResolveThreads) void resolve_kernel(const ResolveArgs a) {
    const uint32_t t = blockIdx.x * (uint32_t)kResolveThreads + threadIdx.x;
    const uint32_t tw = (uint32_t)a.tw;
    for (int r = blockIdx.y; r < a.th; r += gridDim.y) {
        const uint32_t s0 = (uint32_t)(a.sy0 + r) * (uint32_t)a.rw + (uint32_t)a.sx0;  // the row's first source pixel
        uint32_t head = a.wide ? (0u - s0) & (kGroup - 1u) : tw;  // pixels before the first aligned group
        head = head < tw ? head : tw;
        const uint32_t groups = (tw - head) / kGroup;
        char* row = reinterpret_cast<char*>(a.dst) + (long long)(a.dy0 + r * a.dy_step) * a.pitch +
                    (long long)a.dx0 * kBpp<FMT>;
        if (t < groups) {
            const uint32_t x = head + t * kGroup;
            resolve_pixels<FMT, kGroup, true>(a, s0 + x, row + (size_t)x * kBpp<FMT>);
        } else if (t - groups < tw - groups * kGroup) {  // the row's head, then its tail
            const uint32_t k = t - groups;
            const uint32_t x = k < head ? k : k + groups * kGroup;
            resolve_pixels<FMT, 1, false>(a, s0 + x, row + (size_t)x * kBpp<FMT>);
        }
    }
}

template <int FMT>
void launch(const ResolveArgs& a, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(resolve_kernel<FMT>, grid, dim3(kResolveThreads), 0, st, a);
}

}  // namespace

hipError_t launch_resolve(ResolveArgs a, hipStream_t st) {
    if (a.tw <= 0 || a.th <= 0) return hipSuccess;
    a.wide = (reinterpret_cast<uintptr_t>(a.src) & 15u) == 0 && (reinterpret_cast<uintptr_t>(a.albedo) & 15u) == 0;
    // threads of a row: its groups and at most 3 + 3 single pixels, or every pixel
    const uint32_t slots = a.wide ? (uint32_t)a.tw / kGroup + 2 * (kGroup - 1) : (uint32_t)a.tw;
    const dim3 grid((slots + kResolveThreads - 1) / kResolveThreads, a.th < 65535 ? a.th : 65535);
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
