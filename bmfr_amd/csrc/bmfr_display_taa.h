// bmfr_display_taa.h -- host-side launcher of bmfr_display_taa.hip (bmfr_display_taa).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmfr_pixel_io.h"

namespace bmfr {

// Kernel arguments of the display-resolution TAA (include/bmfr.h, bmfr_display_taa_args /
// bmfr_surface): validated by the C ABI, which maps the Wd x Hd frame into the surface.
struct DisplayTaaArgs {
    const void* current;     // display-resolution planes, Wd x Hd, rows *_pitch bytes apart
    const void* history;     // null: no history (or reset): result = current
    void* result;
    const float* prev_pixel; // with history: this (f32x2, stride Wd) or motion
    const void* motion;
    long long current_pitch, history_pitch, result_pitch;
    SurfaceDst surf;         // the Wd x Hd frame in the surface; surf.dst null: no surface
    float mscale[2];         // motion_scale
    float jx, jy1;           // pixel_offset[0], 1.0f - pixel_offset[1]
    float blend_a, blend_b;  // blend_alpha, 1.0f - blend_alpha
    int current_fmt, history_fmt, result_fmt;  // BMFR_FORMAT_F32X3 | BMFR_FORMAT_F16X4
    int motion_fmt, motion_centre;
    int Wd, Hd;
};

// One launch.
hipError_t launch_display_taa(const DisplayTaaArgs& a, hipStream_t st);

}  // namespace bmfr
