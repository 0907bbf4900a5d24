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
#include "bmfr_pixel_io.h"
#include "bmfr_resolve.h"

namespace bmfr {
namespace {

constexpr int kResolveThreads = 256;
constexpr int kSrcGroup = kGroup<float>;  // pixels of a group of the f32x3 source plane

// N consecutive pixels of a row: flat region pixel index `first`, surface address p.
template <int FMT, int N, bool WIDE>
__device__ __forceinline__ void resolve_pixels(const ResolveArgs& a, uint32_t first, char* p) {
    float v[N][3];
    {
        uint32_t w[N * 3];
        ld_bytes<N * 12, kAlign<N * 12, WIDE, 4>>(a.src, first * 12u, w);
#pragma unroll
        for (int i = 0; i < N * 3; ++i) v[i / 3][i % 3] = __uint_as_float(w[i]);
    }
    if (a.albedo) {  // BMFR_RESOLVE_HDR: v = a * f
        float al[N][3];
        if (a.albedo_half) {
            uint32_t w[(N * 6 + 3) / 4] = {};
            ld_bytes<N * 6, kAlign<N * 6, WIDE, 2>>(a.albedo, first * 6u, w);
#pragma unroll
            for (int i = 0; i < N * 3; ++i) al[i / 3][i % 3] = half_to_float(u16_at(w, i));
        } else {
            uint32_t w[N * 3];
            ld_bytes<N * 12, kAlign<N * 12, WIDE, 4>>(a.albedo, first * 12u, w);
#pragma unroll
            for (int i = 0; i < N * 3; ++i) al[i / 3][i % 3] = __uint_as_float(w[i]);
        }
#pragma unroll
        for (int i = 0; i < N * 3; ++i) v[i / 3][i % 3] = al[i / 3][i % 3] * v[i / 3][i % 3];
    }
    if (a.surf.bgr) {
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const float t = v[q][0];
            v[q][0] = v[q][2];
            v[q][2] = t;
        }
    }
    st_surface<FMT, N>(p, v, a.surf.alpha);
}

template <int FMT>
__global__ __launch_bounds__(kResolveThreads) void resolve_kernel(const ResolveArgs a) {
    const uint32_t t = blockIdx.x * (uint32_t)kResolveThreads + threadIdx.x;
    const uint32_t tw = (uint32_t)a.tw;
    for (int r = blockIdx.y; r < a.th; r += gridDim.y) {
        const uint32_t s0 = (uint32_t)(a.sy0 + r) * (uint32_t)a.rw + (uint32_t)a.sx0;  // the row's first source pixel
        uint32_t head = a.wide ? (0u - s0) & (kSrcGroup - 1u) : tw;  // pixels before the first aligned group
        head = head < tw ? head : tw;
        const uint32_t groups = (tw - head) / kSrcGroup;
        char* row = surface_pixel<FMT>(a.surf, 0, r);
        if (t < groups) {
            const uint32_t x = head + t * kSrcGroup;
            resolve_pixels<FMT, kSrcGroup, true>(a, s0 + x, row + (size_t)x * kBpp<FMT>);
        } else if (t - groups < tw - groups * kSrcGroup) {  // the row's head, then its tail
            const uint32_t k = t - groups;
            const uint32_t x = k < head ? k : k + groups * kSrcGroup;
            resolve_pixels<FMT, 1, false>(a, s0 + x, row + (size_t)x * kBpp<FMT>);
        }
    }
}

}  // namespace

hipError_t launch_resolve(ResolveArgs a, hipStream_t st) {
    if (a.tw <= 0 || a.th <= 0) return hipSuccess;
    a.wide = (reinterpret_cast<uintptr_t>(a.src) & 15u) == 0 && (reinterpret_cast<uintptr_t>(a.albedo) & 15u) == 0;
    // threads of a row: its groups and at most 3 + 3 single pixels, or every pixel
    const uint32_t slots = a.wide ? (uint32_t)a.tw / kSrcGroup + 2 * (kSrcGroup - 1) : (uint32_t)a.tw;
    const dim3 grid((slots + kResolveThreads - 1) / kResolveThreads, a.th < 65535 ? a.th : 65535);
    const bool listed = dispatch_surface_format(a.surf.format, [&](auto fmt) {
        hipLaunchKernelGGL(resolve_kernel<decltype(fmt)::value>, grid, dim3(kResolveThreads), 0, st, a);
    });
    if (!listed) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace bmfr
