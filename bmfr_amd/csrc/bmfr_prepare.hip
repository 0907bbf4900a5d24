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
#include "bmfr_prepare.h"

namespace bmfr {
namespace {

constexpr int kPrepareThreads = 256;
template <class OUT>
constexpr int kGroup = sizeof(OUT) == 4 ? 4 : 8;

// Alignment of an access of BYTES at a group's (WIDE) or a pixel's offset;
// NATURAL: the element's own alignment.
template <int BYTES, bool WIDE, int NATURAL>
constexpr int kAlign = !WIDE ? NATURAL : (BYTES % 16 == 0 ? 16 : (BYTES % 8 == 0 ? 8 : NATURAL));

// BYTES at base + off into / out of 32-bit words (the last word may be partial).
template <int BYTES, int ALIGN>
__device__ __forceinline__ void ld_bytes(const void* base, uint32_t off, uint32_t* w) {
    const char* p = reinterpret_cast<const char*>(base) + off;
    __builtin_memcpy(w, __builtin_assume_aligned(p, ALIGN), BYTES);
}
template <int BYTES, int ALIGN>
__device__ __forceinline__ void st_bytes(void* base, uint32_t off, const uint32_t* w) {
    char* p = reinterpret_cast<char*>(base) + off;
    __builtin_memcpy(__builtin_assume_aligned(p, ALIGN), w, BYTES);
}

// 16-bit element k of packed words.
__device__ __forceinline__ uint32_t u16_at(const uint32_t* w, int k) { return (w[k >> 1] >> (16 * (k & 1))) & 0xffffu; }
__device__ __forceinline__ float half_to_float(uint32_t bits) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}

// One output element's bits (f32, or half in the low 16) <-> f32.
template <class OUT>
__device__ __forceinline__ uint32_t encode(float v) {
    if constexpr (sizeof(OUT) == 4) return __float_as_uint(v);
    else return __builtin_bit_cast(uint16_t, (_Float16)v);
}
template <class OUT>
__device__ __forceinline__ float decode(uint32_t bits) {
    if constexpr (sizeof(OUT) == 4) return __uint_as_float(bits);
    else return half_to_float(bits);
}

// N pixels of a float3 / half3 plane from pixel `first`, as element bits.
template <class OUT, int N, bool WIDE>
__device__ __forceinline__ void ld_elems(const void* base, uint32_t first, uint32_t (&e)[N * 3]) {
    constexpr int BYTES = N * 3 * (int)sizeof(OUT);
    uint32_t w[(BYTES + 3) / 4] = {};
    ld_bytes<BYTES, kAlign<BYTES, WIDE, (int)sizeof(OUT)>>(base, first * (3u * sizeof(OUT)), w);
#pragma unroll
    for (int i = 0; i < N * 3; ++i) e[i] = sizeof(OUT) == 4 ? w[i] : u16_at(w, i);
}
template <class OUT, int N, bool WIDE>
__device__ __forceinline__ void st_elems(void* base, uint32_t first, const uint32_t (&e)[N * 3]) {
    constexpr int BYTES = N * 3 * (int)sizeof(OUT);
    uint32_t w[(BYTES + 3) / 4] = {};
#pragma unroll
    for (int i = 0; i < N * 3; ++i) {
        if constexpr (sizeof(OUT) == 4) w[i] = e[i];
        else w[i >> 1] |= e[i] << (16 * (i & 1));
    }
    st_bytes<BYTES, kAlign<BYTES, WIDE, (int)sizeof(OUT)>>(base, first * (3u * sizeof(OUT)), w);
}
template <class OUT, int N, bool WIDE>
__device__ __forceinline__ void st_float3(void* base, uint32_t first, const float (&v)[N][3]) {
    uint32_t e[N * 3];
#pragma unroll
    for (int i = 0; i < N * 3; ++i) e[i] = encode<OUT>(v[i / 3][i % 3]);
    st_elems<OUT, N, WIDE>(base, first, e);
}

// N pixels of a three-channel G-buffer plane (F32X3, F16X4, UNORM8X4) as f32.
template <int N, bool WIDE>
__device__ __forceinline__ void ld_channels(const void* base, int fmt, uint32_t first, float (&c)[N][3]) {
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

// One octahedral snorm16 component.
__device__ __forceinline__ float snorm16(uint32_t bits) {
    const float e = (float)(int16_t)(uint16_t)bits / 32767.0f;
    return e < -1.0f ? -1.0f : e;
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
            for (int p = 0; p < N; ++p) {
                const float ex = snorm16(w[p] & 0xffffu), ey = snorm16(w[p] >> 16);
                const float ax = __builtin_fabsf(ex), ay = __builtin_fabsf(ey);
                const float z = (1.0f - ax) - ay;
                float ox = ex, oy = ey;
                if (z < 0.0f) {
                    ox = (1.0f - ay) * (ex >= 0.0f ? 1.0f : -1.0f);
                    oy = (1.0f - ax) * (ey >= 0.0f ? 1.0f : -1.0f);
                }
                const float len = __builtin_sqrtf((ox * ox + oy * oy) + z * z);
                nrm[p][0] = ox / len;
                nrm[p][1] = oy / len;
                nrm[p][2] = z / len;
            }
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
            for (int p = 0; p < N; ++p) {
                const float depth = __uint_as_float(w[p]);
                const float sx = fx[p] + a.jx, sy = fy[p] + a.jy1;
                const float nx = (sx / fW) * 2.0f - 1.0f, ny = (sy / fH) * 2.0f - 1.0f;
                float h[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) h[i] = ((a.m[i] * nx + a.m[4 + i] * ny) + a.m[8 + i] * depth) + a.m[12 + i];
#pragma unroll
                for (int i = 0; i < 3; ++i) pos[p][i] = h[i] / h[3];
            }
        }
        st_float3<OUT, N, WIDE>(a.o_positions, first, pos);
    }

    // motion vectors -> prev_pixel
    if (a.o_prev_pixel) {
        float mv[N][2];
        if (a.motion_fmt == BMFR_FORMAT_F32X2) {
            uint32_t w[N * 2];
            ld_bytes<N * 8, kAlign<N * 8, WIDE, 8>>(a.motion, first * 8u, w);
#pragma unroll
            for (int i = 0; i < N * 2; ++i) mv[i / 2][i % 2] = __uint_as_float(w[i]);
        } else {  // BMFR_FORMAT_F16X2
            uint32_t w[N];
            ld_bytes<N * 4, kAlign<N * 4, WIDE, 4>>(a.motion, first * 4u, w);
#pragma unroll
            for (int i = 0; i < N * 2; ++i) mv[i / 2][i % 2] = half_to_float(u16_at(w, i));
        }
        uint32_t o[N * 2];
#pragma unroll
        for (int p = 0; p < N; ++p) {
            const float mx = mv[p][0] * a.mscale_x, my = mv[p][1] * a.mscale_y;
            float pfx, pfy;
            if (a.motion_centre) {
                pfx = ((fx[p] + 0.5f) - mx) - a.jx;
                pfy = ((fy[p] + 0.5f) - my) - a.jy1;
            } else {
                pfx = fx[p] - mx;
                pfy = fy[p] - my;
            }
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
