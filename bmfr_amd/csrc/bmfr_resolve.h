// bmfr_resolve.h -- host-side launcher of bmfr_resolve.hip (bmfr_resolve_output).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmfr_pixel_io.h"

namespace bmfr {

// Kernel arguments of the output back end (include/bmfr.h, bmfr_surface):
// validated by the C ABI, which maps the context's tile into the surface.
struct ResolveArgs {
    const float* src;    // the region's result or filtered_accumulated plane, f32x3, row stride rw
    const void* albedo;  // BMFR_RESOLVE_HDR: the region's albedo plane (f32x3, or half3: albedo_half); else null
    SurfaceDst surf;     // the tile in the surface: rectangle row r is tile row r
    int albedo_half;
    int rw;              // region row stride, pixels
    int sx0, sy0;        // the tile's first pixel, region coordinates
    int tw, th;          // tile size
    int wide;            // groups of 4 pixels with 16-byte source loads (set by the launcher)
};

// One launch.  An empty tile launches nothing.
hipError_t launch_resolve(ResolveArgs a, hipStream_t st);

}  // namespace bmfr
