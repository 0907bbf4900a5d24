// bmfr_prepare.hip -- the G-buffer front end (bmfr_prepare_frame, include/bmfr.h):
// one streaming kernel from a renderer's buffers to the planes
// bmfr_process_frame reads.  No reference counterpart (the reference's dataset
// already holds those planes); the formulas are the ones the header documents,
// each line one f32 operation (-ffp-contract=off, correctly rounded / and sqrt).
//
// Shape: planes are contiguous (row stride = region width), so the kernel
// indexes them flat.  A thread takes a group of consecutive pixels -- 4 for
// float3 outputs (48 B), 8 for half3 (48 B) -- so that every plane access of a
// group is a run of 16-byte loads or stores (8 bytes for a group's 4 ids); the
// pixels past the last whole group, or every pixel when a plane is not
// 16-byte aligned, go one per thread with element-sized accesses.  Addresses
// are the plane's base (a kernel argument, in SGPRs) plus a 32-bit byte offset
// (bmfr_create bounds planes at 4 GiB).  Input formats are wave-uniform
// run-time switches; the output element type is a template parameter.  No LDS.
#include "../../include/bmfr.h"
#include "bmfr_pixel_io.h"
#include "bmfr_prepare.h"

namespace bmfr {
namespace {

constexpr int kPrepareThreads = 256;

// N pixels' f32 values into a float3 / half3 plane from pixel `first`.
template <class OUT, int N, bool WIDE>
__device__ __forceinline__ void st_float3(void* base, uint32_t first, const float (&v)[N][3]) {
    uint32_t e[N * 3];
#pragma unroll
    for (int i = 0; i < N * 3; ++i) e[i] = encode<OUT>(v[i / 3][i % 3]);
    st_elems<OUT, N, WIDE>(base, first, e);
}

// N consecutive pixels from flat region index `first`.
template <class OUT, int N, bool WIDE>
__device__ __forceinline__ void prepare_pixels(const PrepareArgs& a, uint32_t first) {
    // image coordinates of the pixels, as f32
    float fx[N], fy[N];
    {
        const uint32_t rw = (uint32_t)a.rw;
        uint32_t y = first / rw, x = first - y * rw;
#pragma unroll
        for (int p = 0; p < N; ++p) {
            fx[p] = (float)(a.rx + (int)x);
            fy[p] = (float)(a.ry + (int)y);
            if (++x == rw) {
                x = 0;
                ++y;
            }
        }
    }

    // demodulation
    if (a.o_noisy || a.o_albedo) {
        float alb[N][3];
        ld_channels<N, WIDE>(a.albedo, a.albedo_fmt, first, alb);
        if (a.o_albedo) st_float3<OUT, N, WIDE>(a.o_albedo, first, alb);
        if (a.o_noisy) {
            float rad[N][3];
            ld_channels<N, WIDE>(a.radiance, a.radiance_fmt, first, rad);
#pragma unroll
            for (int i = 0; i < N * 3; ++i) {
                const float al = alb[i / 3][i % 3];
                const float d = al > a.albedo_floor ? al : a.albedo_floor;
                rad[i / 3][i % 3] = rad[i / 3][i % 3] / d;
            }
            st_float3<OUT, N, WIDE>(a.o_noisy, first, rad);
        }
    }

    // normals
    if (a.o_normals) {
        float nrm[N][3];
        if (a.normal_fmt == BMFR_FORMAT_OCT_SNORM16X2) {
            uint32_t w[N];
            ld_bytes<N * 4, kAlign<N * 4, WIDE, 4>>(a.normals, first * 4u, w);
#pragma unroll
            for (int p = 0; p < N; ++p) oct_decode(w[p], nrm[p]);
        } else {
            ld_channels<N, WIDE>(a.normals, a.normal_fmt, first, nrm);
        }
        st_float3<OUT, N, WIDE>(a.o_normals, first, nrm);
    }

    // positions: given, or from depth
    if (a.o_positions) {
        float pos[N][3];
        if (a.positions) {
            ld_channels<N, WIDE>(a.positions, BMFR_FORMAT_F32X3, first, pos);
        } else {
            uint32_t w[N];
            ld_bytes<N * 4, kAlign<N * 4, WIDE, 4>>(a.depth, first * 4u, w);
            const float fW = (float)a.W, fH = (float)a.H;
#pragma unroll
            for (int p = 0; p < N; ++p)
                position_from_depth(a.m, __uint_as_float(w[p]), fx[p], fy[p], a.jx, a.jy1, fW, fH, pos[p]);
        }
        st_float3<OUT, N, WIDE>(a.o_positions, first, pos);
    }

    // motion vectors -> prev_pixel
    if (a.o_prev_pixel) {
        float mv[N][2];
        ld_motion<N, WIDE>(a.motion, a.motion_fmt, first, mv);
        uint32_t o[N * 2];
#pragma unroll
        for (int p = 0; p < N; ++p) {
            float pfx, pfy;
            previous_position(mv[p][0], mv[p][1], a.mscale_x, a.mscale_y, a.motion_centre != 0, fx[p], fy[p], a.jx,
                              a.jy1, pfx, pfy);
            o[2 * p] = __float_as_uint(pfx);
            o[2 * p + 1] = __float_as_uint(pfy);
        }
        st_bytes<N * 8, kAlign<N * 8, WIDE, 8>>(a.o_prev_pixel, first * 8u, o);
    }

    // the previous frame's planes, moved by each pixel's object transform
    if (a.o_prev_positions || a.o_prev_normals) {
        uint32_t ep[N * 3], en[N * 3];
        if (a.o_prev_positions) ld_elems<OUT, N, WIDE>(a.prev_positions, first, ep);
        if (a.o_prev_normals) ld_elems<OUT, N, WIDE>(a.prev_normals, first, en);
        if (a.n_objects > 0) {
            uint32_t idw[(N * 2 + 3) / 4] = {};
            ld_bytes<N * 2, kAlign<N * 2, WIDE, 2>>(a.prev_id, first * 2u, idw);
#pragma unroll
            for (int p = 0; p < N; ++p) {
                const uint32_t id = u16_at(idw, p);
                const bool moves = id < (uint32_t)a.n_objects;
                // the object's 3x4 after its id (entry 0 stands in for ids past the table: not used)
                uint32_t mw[12];
                ld_bytes<48, WIDE ? 16 : 4>(a.transforms, (moves ? id : 0u) * 48u, mw);
                float M[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) M[i] = __uint_as_float(mw[i]);
                if (a.o_prev_positions) {
                    const float x = decode<OUT>(ep[3 * p]), y = decode<OUT>(ep[3 * p + 1]), z = decode<OUT>(ep[3 * p + 2]);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float r = ((M[4 * i] * x + M[4 * i + 1] * y) + M[4 * i + 2] * z) + M[4 * i + 3];
                        ep[3 * p + i] = moves ? encode<OUT>(r) : ep[3 * p + i];
                    }
                }
                if (a.o_prev_normals) {
                    const float x = decode<OUT>(en[3 * p]), y = decode<OUT>(en[3 * p + 1]), z = decode<OUT>(en[3 * p + 2]);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float r = (M[4 * i] * x + M[4 * i + 1] * y) + M[4 * i + 2] * z;
                        en[3 * p + i] = moves ? encode<OUT>(r) : en[3 * p + i];
                    }
                }
            }
        }
        if (a.o_prev_positions) st_elems<OUT, N, WIDE>(a.o_prev_positions, first, ep);
        if (a.o_prev_normals) st_elems<OUT, N, WIDE>(a.o_prev_normals, first, en);
    }
}

template <class OUT>
__global__ __launch_bounds__(kPrepareThreads) void prepare_kernel(const PrepareArgs a) {
    constexpr int G = kGroup<OUT>;
    const uint32_t t = blockIdx.x * (uint32_t)kPrepareThreads + threadIdx.x;
    if (t < a.groups) {
        prepare_pixels<OUT, G, true>(a, t * G);
    } else {
        const uint32_t i = a.groups * G + (t - a.groups);
        if (i < a.n) prepare_pixels<OUT, 1, false>(a, i);
    }
}

}  // namespace

hipError_t launch_prepare(PrepareArgs a, bool half_out, hipStream_t st) {
    const void* planes[] = {a.radiance, a.albedo, a.normals, a.positions, a.depth, a.motion, a.prev_positions,
                            a.prev_normals, a.prev_id, a.transforms, a.o_noisy, a.o_normals, a.o_positions,
                            a.o_albedo, a.o_prev_pixel, a.o_prev_positions, a.o_prev_normals};
    bool aligned = true;
    for (const void* p : planes) aligned = aligned && (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
    const bool any = a.o_noisy || a.o_normals || a.o_positions || a.o_albedo || a.o_prev_pixel ||
                     a.o_prev_positions || a.o_prev_normals;
    if (a.n == 0 || !any) return hipSuccess;
    const uint32_t G = half_out ? kGroup<_Float16> : kGroup<float>;
    a.groups = aligned ? a.n / G : 0;
    const uint32_t threads = a.groups + (a.n - a.groups * G);
    const dim3 grid((threads + kPrepareThreads - 1) / kPrepareThreads), block(kPrepareThreads);
    if (half_out) hipLaunchKernelGGL(prepare_kernel<_Float16>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(prepare_kernel<float>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace bmfr
