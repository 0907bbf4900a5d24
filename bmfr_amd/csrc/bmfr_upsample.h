// bmfr_upsample.h -- host-side launcher of bmfr_upsample.hip (bmfr_upsample_output).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmfr_pixel_io.h"

namespace bmfr {

// Kernel arguments of the guided upsampler (include/bmfr.h, bmfr_upsample_guides /
// bmfr_surface): validated by the C ABI, which maps the Wd x Hd frame into the surface.
struct UpsampleArgs {
    const float* acc;        // filtered_accumulated of the last frame, f32x3, W x H
    const void* f_normals;   // the frame's normals / positions (f32x3, or half3: frame_half); guided only
    const void* f_positions;
    const void* albedo;      // display-resolution guides, Wd x Hd
    const void* normals;     // null: unguided
    const float* positions;  // guided: this or depth
    const float* depth;
    uint32_t* stats;         // nullable
    SurfaceDst surf;         // the Wd x Hd frame in the surface
    float m[16];             // inv_view_proj, column-major
    float jx, jy1;           // pixel_offset[0], 1.0f - pixel_offset[1]
    float rx, ry;            // float(W) / float(Wd), float(H) / float(Hd)
    float plane_limit_sq, normal_limit_sq;
    int albedo_fmt, normal_fmt;
    int frame_half, tonemapped;
    int W, H, Wd, Hd;
};

// One launch.
hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t st);

}  // namespace bmfr
