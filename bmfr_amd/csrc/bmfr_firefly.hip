// bmfr_firefly.hip -- the firefly pre-filter (bmfr_suppress_fireflies,
// include/bmfr.h): one stencil kernel over the noisy plane, ahead of the block
// fit.  No reference counterpart (the reference's dataset is clean); the rules
// are the ones the header documents, each line one f32 operation
// (-ffp-contract=off, correctly rounded division).
//
// Shape: a 256-thread work-group takes tiles of 16 rows of 16 groups, one after
// the other down its column of the plane (about 2048 work-groups per launch,
// the same number of tiles each, give or take one); a thread owns one
// group of consecutive pixels of a row -- 4 for float3 (48 B), 8 for half3
// (48 B) -- and keeps their element bits in registers from the load to the
// store.  A row's groups start where the flat pixel index is a multiple of the
// group (column shift(y) = -(y * rw) mod group), so that a group inside the row
// is a run of 16-byte loads and stores whatever the region's width; a group
// cut by the row's ends, or every group when a plane is not 16-byte aligned,
// goes pixel by pixel with element-sized accesses.  The filter needs only the
// luminance of neighbours: the work-group stages Y of its pixels (from the
// registers) and of the ring around them (element-sized loads, issued ahead of
// the group's own so that both are in flight together; L2 hits) in
// LDS, NaN standing for "no pixel here", and every thread reads its
// (2r + 1) x (group + 2r) window from there.  Addresses are the plane's base
// plus a 32-bit byte offset (bmfr_create bounds planes at 4 GiB).  The radius
// and the element type are template parameters.  The two counters are kept in
// registers over the work-group's tiles, summed in LDS and added to `stats`
// with one atomic each per work-group: all of a launch's atomics land on one
// line, and with one work-group per tile (8235 at 3840x2160) they took as long
// as the pixels (profiles/firefly_bench.txt).
#include <algorithm>

#include "../../include/bmfr.h"
#include "bmfr_firefly.h"
#include "bmfr_pixel_io.h"

namespace bmfr {
namespace {

constexpr int kFireflyThreads = 256;
constexpr int kCols = 16, kRows = 16;  // groups per tile row, tile rows
constexpr int kMaxGroups = 2048;       // work-groups of a launch, about: 8 per CU

__device__ __forceinline__ bool finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }  // false for NaN
// Y of a pixel's element bits
template <class T>
__device__ __forceinline__ float luminance(const uint32_t* e) {
    return (0.2126f * decode<T>(e[0]) + 0.7152f * decode<T>(e[1])) + 0.0722f * decode<T>(e[2]);
}

template <class T, int R>
__global__ __launch_bounds__(kFireflyThreads) void firefly_kernel(const FireflyArgs a) {
    constexpr int G = kGroup<T>;
    constexpr int TW = kCols * G;            // pixels a tile row owns
    constexpr int LW = TW + (G - 1) + 2 * R;  // staged columns: every shift of the owned run, and the ring
    constexpr int LH = kRows + 2 * R;
    constexpr int E = LW - TW;                // staged columns of a tile row its threads do not own
    constexpr uint32_t kNoPixel = sizeof(T) == 4 ? 0x7fc00000u : 0x7e00u;  // NaN: never a neighbour
    __shared__ float sY[LH][LW];
    __shared__ uint32_t sCount[2];

    const int tx = threadIdx.x & (kCols - 1), ty = threadIdx.x / kCols;
    const int X0 = (int)blockIdx.x * TW - G;  // image column of staged column R (the first group is the rows' heads)
    const uint32_t rw = (uint32_t)a.rw;
    // first column of row y whose flat pixel index is a multiple of the group
    auto shift = [&](int y) { return a.wide ? (int)((0u - (uint32_t)y * rw) & (uint32_t)(G - 1)) : 0; };
    auto inside = [&](int x, int y) { return x >= 0 && x < a.rw && y >= 0 && y < a.rh; };

    if (threadIdx.x < 2) sCount[threadIdx.x] = 0;
    uint32_t clamped = 0, replaced = 0;

    // the work-group's tiles: every gridDim.y-th of its column (Y0 is the same in all its threads)
    for (int Y0 = (int)blockIdx.y * kRows; Y0 < a.rh; Y0 += (int)gridDim.y * kRows) {
        // the ring: R rows above and below the tile, and beside each tile row the
        // E columns left and right of its owned run; its loads go out first, so
        // that they are in flight together with the group's
        constexpr int kAbove = 2 * R * LW, kRing = kAbove + kRows * E;
        constexpr int kTurns = (kRing + kFireflyThreads - 1) / kFireflyThreads;
        uint32_t q[kTurns][3];
        int at[kTurns];  // staged index, -1: none
#pragma unroll
        for (int t = 0; t < kTurns; ++t) {
            const int k = (int)threadIdx.x + t * kFireflyThreads;
            int lx, ly;
            if (k < kAbove) {
                const int r = k / LW;
                lx = k - r * LW;
                ly = r < R ? r : r + kRows;
            } else {
                const int r = (k - kAbove) / E, i = (k - kAbove) - r * E;
                const int lead = shift(Y0 + r) + R;  // staged columns before the row's owned run
                lx = i < lead ? i : i + TW;
                ly = r + R;
            }
            const int gx = X0 + lx - R, gy = Y0 + ly - R;
            at[t] = k < kRing ? ly * LW + lx : -1;
            q[t][0] = q[t][1] = q[t][2] = kNoPixel;
            if (k < kRing && inside(gx, gy)) ld_elems<T, 1, false>(a.noisy, (uint32_t)gy * rw + (uint32_t)gx, q[t]);
        }

        // this thread's group: element bits in registers, Y into LDS
        const int y = Y0 + ty;
        const int lx0 = shift(y) + tx * G;  // staged column of the group's first pixel, less R
        const int x0 = X0 + lx0;
        const uint32_t first = (uint32_t)y * rw + (uint32_t)x0;
        const bool whole = a.wide && y < a.rh && x0 >= 0 && x0 + G <= a.rw;
        uint32_t e[G * 3];
        if (whole) {
            ld_elems<T, G, true>(a.noisy, first, e);
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                e[3 * j] = e[3 * j + 1] = e[3 * j + 2] = kNoPixel;
                if (inside(x0 + j, y)) ld_elems<T, 1, false>(a.noisy, first + j, e + 3 * j);
            }
        }
        float Y[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            Y[j] = luminance<T>(e + 3 * j);
            sY[ty + R][lx0 + j + R] = Y[j];
        }
#pragma unroll
        for (int t = 0; t < kTurns; ++t)
            if (at[t] >= 0) (&sY[0][0])[at[t]] = luminance<T>(q[t]);
        __syncthreads();

        // the window of the group, column by column (finite Y, or -inf): the
        // maximum over its rows, and over its rows without the group's own
        float all[G + 2 * R], others[G + 2 * R];
#pragma unroll
        for (int i = 0; i < G + 2 * R; ++i) {
            float own = -__builtin_inff();
            others[i] = -__builtin_inff();
#pragma unroll
            for (int dy = 0; dy <= 2 * R; ++dy) {
                float v = sY[ty + dy][lx0 + i];
                v = finite(v) ? v : -__builtin_inff();
                if (dy == R) own = v;
                else others[i] = v > others[i] ? v : others[i];
            }
            all[i] = own > others[i] ? own : others[i];
        }
        __syncthreads();  // the next tile's Y goes into the same LDS

#pragma unroll
        for (int j = 0; j < G; ++j) {
            const float c0 = decode<T>(e[3 * j]), c1 = decode<T>(e[3 * j + 1]), c2 = decode<T>(e[3 * j + 2]);
            const bool here = whole || inside(x0 + j, y);
            float m = others[j + R];  // no finite Y is -inf: still -inf means no neighbour
#pragma unroll
            for (int dx = 0; dx <= 2 * R; ++dx)
                if (dx != R) m = all[j + dx] > m ? all[j + dx] : m;
            if (!(finite(c0) && finite(c1) && finite(c2))) {
                if (here && a.replace_nonfinite) {
                    e[3 * j] = e[3 * j + 1] = e[3 * j + 2] = 0;
                    ++replaced;
                }
            } else if (m > -__builtin_inff()) {
                float limit = a.threshold * m;
                if (!(limit > a.floor)) limit = a.floor;
                if (here && Y[j] > limit) {
                    const float s = limit / Y[j];
                    e[3 * j] = encode<T>(c0 * s);
                    e[3 * j + 1] = encode<T>(c1 * s);
                    e[3 * j + 2] = encode<T>(c2 * s);
                    ++clamped;
                }
            }
        }

        if (whole) {
            st_elems<T, G, true>(a.out, first, e);
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (inside(x0 + j, y)) st_elems<T, 1, false>(a.out, first + j, e + 3 * j);
        }
    }

    if (a.stats) {  // the same in every thread
        if (clamped) atomicAdd(&sCount[0], clamped);
        if (replaced) atomicAdd(&sCount[1], replaced);
        __syncthreads();
        if (threadIdx.x < 2 && sCount[threadIdx.x]) atomicAdd(a.stats + threadIdx.x, sCount[threadIdx.x]);
    }
}

template <class T, int R>
void launch(const FireflyArgs& a, hipStream_t st) {
    constexpr int TW = kCols * kGroup<T>;
    // columns -G .. rw - 1: the first group of a row holds the pixels before its first aligned one
    const int across = (a.rw + kGroup<T> + TW - 1) / TW, down = (a.rh + kRows - 1) / kRows;
    // about kMaxGroups work-groups, each with `turns` tiles of its column (the last ones may have one fewer)
    const int rows = std::max(kMaxGroups / across, 1);
    const int turns = (down + rows - 1) / rows;
    const dim3 grid(across, (down + turns - 1) / turns);
    hipLaunchKernelGGL((firefly_kernel<T, R>), grid, dim3(kFireflyThreads), 0, st, a);
}

}  // namespace

hipError_t launch_firefly(FireflyArgs a, bool half, int radius, hipStream_t st) {
    if (a.rw <= 0 || a.rh <= 0) return hipSuccess;
    if (radius != 1 && radius != 2) return hipErrorInvalidValue;
    a.wide = ((reinterpret_cast<uintptr_t>(a.noisy) | reinterpret_cast<uintptr_t>(a.out)) & 15u) == 0;
    if (half) radius == 1 ? launch<_Float16, 1>(a, st) : launch<_Float16, 2>(a, st);
    else radius == 1 ? launch<float, 1>(a, st) : launch<float, 2>(a, st);
    return hipGetLastError();
}

}  // namespace bmfr
