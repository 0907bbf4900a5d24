// bmfr_firefly.h -- host-side launcher of bmfr_firefly.hip (bmfr_suppress_fireflies).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmfr {

// Kernel arguments of the firefly pre-filter (include/bmfr.h,
// bmfr_firefly_params): validated by the C ABI.
struct FireflyArgs {
    const void* noisy;  // the region's noisy plane, float3 or half3, row stride rw
    void* out;          // same layout; never overlaps noisy
    uint32_t* stats;    // {clamped, replaced}, added to; nullable
    float threshold, floor;
    int replace_nonfinite;
    int rw, rh;         // region size, pixels
    int wide;           // groups of pixels with 16-byte accesses (set by the launcher)
};

// One launch; half: half3 planes; radius 1 or 2.  An empty region launches nothing.
hipError_t launch_firefly(FireflyArgs a, bool half, int radius, hipStream_t st);

}  // namespace bmfr
