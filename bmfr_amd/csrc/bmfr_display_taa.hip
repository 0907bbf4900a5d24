// bmfr_display_taa.hip -- temporal anti-aliasing at display resolution
// (bmfr_display_taa, include/bmfr.h): the reference's TAA (bmfr.cl:860-974) on
// planes the caller owns, one kernel from `current`, `history` and a
// display-resolution prev_pixel (or motion) plane to `result` and, optionally,
// a surface.  The arithmetic is K2's (bmfr_kernels.h taa_offscreen,
// taa_history, taa_clamp_tail), restated on plain arguments: each line one f32
// operation (-ffp-contract=off, correctly rounded division), the YCoCg dot
// products the reference's fma chains.
//
// Shape: a work-group of 64 x 4 threads takes a display tile of 64 x 16 pixels
// and walks down the frame in steps of gridDim.y tiles.  A thread owns one
// column of kRows consecutive rows.  For each row it forms, once, the row's
// partial bounds -- min / max in YCoCg over the pixels (X - 1, X, X + 1) --
// and the centre's YCoCg; the box of pixel (X, Y) is the min / max of the
// three rows' partial bounds, its cross that of the middle row's and the upper
// and lower centres (exact in any grouping: taa_clamp_tail's comment), so a
// row loaded once serves three pixels: 3 (kRows + 2) / kRows loads of
// `current` per pixel instead of 9.  A wave is 64 consecutive pixels of a row:
// its loads and stores are consecutive elements, and the neighbours' columns
// and the history taps come through the vector cache.  A pixel that fails the
// off-screen test returns its own colour before the taps (a divergent branch
// that saves their loads); of a pixel that passes it every tap is loaded -- its
// address is clamped into the plane -- and left out of the sums by the
// reference's conditions.  The surface format is a template parameter; the
// plane formats, the motion convention, bgr and flip_y are wave-uniform
// run-time switches.  No LDS.
#include "../../include/bmfr.h"
#include "bmfr_display_taa.h"
#include "bmfr_pixel_io.h"

namespace bmfr {
namespace {

constexpr int kTileW = 64, kWaves = 4, kRows = 4;  // a tile is kTileW x (kWaves * kRows)
constexpr int kNoSurface = -1;

struct f3 {
    float x, y, z;
};

// Pixel (x, y), inside the plane, of an F32X3 / F16X4 plane as f32.
__device__ __forceinline__ f3 ld_plane(const void* base, long long pitch, int fmt, int x, int y) {
    const char* row = reinterpret_cast<const char*>(base) + (long long)y * pitch;
    if (fmt == BMFR_FORMAT_F32X3) {
        uint32_t w[3];
        ld_bytes<12, 4>(row, (long long)x * 12, w);
        return f3{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
    }
    uint32_t w[2];
    ld_bytes<8, 8>(row, (long long)x * 8, w);
    return f3{half_to_float(w[0] & 0xffffu), half_to_float(w[0] >> 16), half_to_float(w[1] & 0xffffu)};
}

// `result`: the bits of v, or (half)v with 4th component (half)1.
__device__ __forceinline__ void st_plane(void* base, long long pitch, int fmt, int x, int y, f3 v) {
    char* row = reinterpret_cast<char*>(base) + (long long)y * pitch;
    if (fmt == BMFR_FORMAT_F32X3) {
        const uint32_t w[3] = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z)};
        st_bytes<12, 4>(row, (long long)x * 12, w);
    } else {
        const uint32_t w[2] = {float_to_half(v.x) | (float_to_half(v.y) << 16), float_to_half(v.z) | (0x3c00u << 16)};
        st_bytes<8, 8>(row, (long long)x * 8, w);
    }
}

// RGB <-> YCoCg, bmfr.cl:184-198: dot(), an fma chain (the coefficients are
// powers of two, so every product is exact short of overflow and underflow).
__device__ __forceinline__ float dot3(f3 a, float bx, float by, float bz) {
    return __builtin_fmaf(a.z, bz, __builtin_fmaf(a.y, by, a.x * bx));
}
__device__ __forceinline__ f3 rgb_to_ycocg(f3 c) {
    return f3{dot3(c, 1.f, 2.f, 1.f), dot3(c, 2.f, 0.f, -2.f), dot3(c, -1.f, 2.f, -1.f)};
}
__device__ __forceinline__ f3 ycocg_to_rgb(f3 c) {
    return f3{dot3(c, 0.25f, 0.25f, -0.25f), dot3(c, 0.25f, 0.f, 0.25f), dot3(c, 0.25f, -0.25f, -0.25f)};
}

// min / max that ignore a NaN operand (v_min_f32 / v_max_f32; -0 < +0).
__device__ __forceinline__ f3 min3(f3 a, f3 b) {
    return f3{__builtin_fminf(a.x, b.x), __builtin_fminf(a.y, b.y), __builtin_fminf(a.z, b.z)};
}
__device__ __forceinline__ f3 max3(f3 a, f3 b) {
    return f3{__builtin_fmaxf(a.x, b.x), __builtin_fmaxf(a.y, b.y), __builtin_fmaxf(a.z, b.z)};
}

constexpr f3 kPosInf{__builtin_inff(), __builtin_inff(), __builtin_inff()};
constexpr f3 kNegInf{-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};

// What row y contributes to the pixels of column X in rows y - 1, y, y + 1:
// the centre's colour, its YCoCg as a min and as a max operand, and the bounds
// over (X - 1, X, X + 1).  Neighbours outside the image do not take part; a
// row outside the image contributes +inf / -inf, which leaves every bound as
// it is (bmfr.cl:897-920 skips those neighbours).
struct Row {
    f3 me, clo, chi, lo, hi;
};
__device__ __forceinline__ Row load_row(const DisplayTaaArgs& a, int X, int y) {
    Row r{f3{0.f, 0.f, 0.f}, kPosInf, kNegInf, kPosInf, kNegInf};
    if (y < 0 || y >= a.Hd) return r;  // wave-uniform: a wave is one row
    const bool left = X > 0, right = X + 1 < a.Wd;
    r.me = ld_plane(a.current, a.current_pitch, a.current_fmt, X, y);
    const f3 l = rgb_to_ycocg(ld_plane(a.current, a.current_pitch, a.current_fmt, left ? X - 1 : X, y));
    const f3 q = rgb_to_ycocg(ld_plane(a.current, a.current_pitch, a.current_fmt, right ? X + 1 : X, y));
    const f3 c = rgb_to_ycocg(r.me);
    r.clo = min3(kPosInf, c);
    r.chi = max3(kNegInf, c);
    r.lo = min3(min3(r.clo, left ? l : kPosInf), right ? q : kPosInf);
    r.hi = max3(max3(r.chi, left ? l : kNegInf), right ? q : kNegInf);
    return r;
}

// (pfx, pfy) of display pixel (X, Y): the prev_pixel entry, or bmfr_prepare_frame's motion rule.
__device__ __forceinline__ void ld_previous_position(const DisplayTaaArgs& a, int X, int Y, float& pfx, float& pfy) {
    const long long i = (long long)Y * a.Wd + X;
    if (a.prev_pixel) {
        uint32_t w[2];
        ld_bytes<8, 4>(a.prev_pixel, i * 8, w);
        pfx = __uint_as_float(w[0]);
        pfy = __uint_as_float(w[1]);
        return;
    }
    float mv[2];
    ld_motion(a.motion, a.motion_fmt, i, mv);
    previous_position(mv[0], mv[1], a.mscale[0], a.mscale[1], a.motion_centre != 0, (float)X, (float)Y, a.jx, a.jy1,
                      pfx, pfy);
}

// Rules 2-6 for display pixel (X, Y) given its three rows (a call with history).
__device__ __forceinline__ f3 taa_pixel(const DisplayTaaArgs& a, int X, int Y, const Row& up, const Row& mid,
                                        const Row& dn) {
    const int W = a.Wd, H = a.Hd;
    const f3 me = mid.me;
    float pfx, pfy;
    ld_previous_position(a, X, Y, pfx, pfy);
    const float flx = __builtin_floorf(pfx), fly = __builtin_floorf(pfy);
    // bmfr.cl:884-890, compared as floats (a NaN compares false and goes on, as in K2)
    if (flx < -1.f || fly < -1.f || flx >= (float)W || fly >= (float)H) return me;
    // bmfr.cl:897-920
    const f3 mnb = min3(min3(up.lo, mid.lo), dn.lo), mxb = max3(max3(up.hi, mid.hi), dn.hi);
    const f3 mnc = min3(min3(up.clo, mid.lo), dn.clo), mxc = max3(max3(up.chi, mid.hi), dn.chi);
    // bmfr.cl:925-966: in the int range whatever pf is
    const int ix = (int)__builtin_fminf(__builtin_fmaxf(flx, -2.f), (float)W + 1.f);
    const int iy = (int)__builtin_fminf(__builtin_fmaxf(fly, -2.f), (float)H + 1.f);
    const float fx = pfx - flx, fy = pfy - fly;
    const float omx = 1.f - fx, omy = 1.f - fy;
    const float tw[4] = {omx * omy, fx * omy, omx * fy, fx * fy};
    f3 pc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        pc[i] = ld_plane(a.history, a.history_pitch, a.history_fmt, min(max(ix + (i & 1), 0), W - 1),
                         min(max(iy + (i >> 1), 0), H - 1));
    f3 prev{0.f, 0.f, 0.f};
    float total = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool okx = (i & 1) ? (ix < W - 1) : (ix >= 0);
        const bool oky = (i >> 1) ? (iy < H - 1) : (iy >= 0);
        if (okx && oky) {
            prev.x = prev.x + tw[i] * pc[i].x;
            prev.y = prev.y + tw[i] * pc[i].y;
            prev.z = prev.z + tw[i] * pc[i].z;
            total = total + tw[i];
        }
    }
    prev = f3{prev.x / total, prev.y / total, prev.z / total};
    const f3 py = rgb_to_ycocg(prev);
    // bmfr.cl:922-973
    const f3 lo{(mnb.x + mnc.x) / 2.f, (mnb.y + mnc.y) / 2.f, (mnb.z + mnc.z) / 2.f};
    const f3 hi{(mxb.x + mxc.x) / 2.f, (mxb.y + mxc.y) / 2.f, (mxb.z + mxc.z) / 2.f};
    const f3 cl{__builtin_fminf(__builtin_fmaxf(py.x, lo.x), hi.x), __builtin_fminf(__builtin_fmaxf(py.y, lo.y), hi.y),
                __builtin_fminf(__builtin_fmaxf(py.z, lo.z), hi.z)};
    const f3 pr = ycocg_to_rgb(cl);
    return f3{a.blend_a * me.x + a.blend_b * pr.x, a.blend_a * me.y + a.blend_b * pr.y,
              a.blend_a * me.z + a.blend_b * pr.z};
}

// Rule 7: v into `result` and, FMT != kNoSurface, into the surface.
template <int FMT>
__device__ __forceinline__ void store(const DisplayTaaArgs& a, int X, int Y, f3 v) {
    st_plane(a.result, a.result_pitch, a.result_fmt, X, Y, v);
    if constexpr (FMT != kNoSurface) {
        const float val[3] = {a.surf.bgr ? v.z : v.x, v.y, a.surf.bgr ? v.x : v.z};
        st_surface<FMT>(surface_pixel<FMT>(a.surf, X, Y), val, a.surf.alpha);
    }
}

template <int FMT>
__global__ __launch_bounds__(kTileW * kWaves) void display_taa_kernel(const DisplayTaaArgs a) {
    const int X = blockIdx.x * kTileW + threadIdx.x;
    if (X >= a.Wd) return;
    const int step = gridDim.y * kWaves * kRows;
    // 64-bit: the last step past a frame near 2^31 rows must not wrap
    for (long long first = (long long)(blockIdx.y * kWaves + threadIdx.y) * kRows; first < a.Hd; first += step) {
        const int Y0 = (int)first;
        if (!a.history) {  // reset, or no history: result = current
            for (int r = 0; r < kRows && r < a.Hd - Y0; ++r)
                store<FMT>(a, X, Y0 + r, ld_plane(a.current, a.current_pitch, a.current_fmt, X, Y0 + r));
            continue;
        }
        Row up = load_row(a, X, Y0 - 1), mid = load_row(a, X, Y0);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (r >= a.Hd - Y0) break;
            const int Y = Y0 + r;
            const Row dn = load_row(a, X, Y + 1);
            store<FMT>(a, X, Y, taa_pixel(a, X, Y, up, mid, dn));
            up = mid;
            mid = dn;
        }
    }
}

}  // namespace

hipError_t launch_display_taa(const DisplayTaaArgs& a, hipStream_t st) {
    if (a.Wd <= 0 || a.Hd <= 0) return hipErrorInvalidValue;
    const int tile_h = kWaves * kRows;
    const int rows = (int)(((long long)a.Hd + tile_h - 1) / tile_h);
    const dim3 grid((unsigned)(((long long)a.Wd + kTileW - 1) / kTileW), rows < 65535 ? rows : 65535);
    const dim3 block(kTileW, kWaves);
    if (!a.surf.dst) {
        hipLaunchKernelGGL(display_taa_kernel<kNoSurface>, grid, block, 0, st, a);
        return hipGetLastError();
    }
    const bool listed = dispatch_surface_format(a.surf.format, [&](auto fmt) {
        hipLaunchKernelGGL(display_taa_kernel<decltype(fmt)::value>, grid, block, 0, st, a);
    });
    if (!listed) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace bmfr
