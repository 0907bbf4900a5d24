// bmfr_prepare.h -- host-side launcher of bmfr_prepare.hip (bmfr_prepare_frame).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmfr {

// Kernel arguments of the G-buffer front end (include/bmfr.h, bmfr_gbuffer /
// bmfr_prepared): validated by the C ABI, which leaves an output null unless
// every input it needs is there.
struct PrepareArgs {
    const void* radiance;
    const void* albedo;
    const void* normals;
    const float* positions;
    const float* depth;
    const void* motion;
    const void* prev_positions;
    const void* prev_normals;
    const uint16_t* prev_id;
    const float* transforms;
    void* o_noisy;
    void* o_normals;
    void* o_positions;
    void* o_albedo;
    float* o_prev_pixel;
    void* o_prev_positions;
    void* o_prev_normals;
    float m[16];  // inv_view_proj, column-major
    float albedo_floor, mscale_x, mscale_y;
    float jx, jy1;  // pixel_offset[0], 1.0f - pixel_offset[1]
    int radiance_fmt, albedo_fmt, normal_fmt, motion_fmt;  // bmfr_format
    int motion_centre, n_objects;
    int rx, ry, rw;  // region origin (image coordinates) and row stride
    int W, H;        // whole frame
    uint32_t n;       // pixels of the region
    uint32_t groups;  // threads that take a whole group of pixels with wide accesses (set by the launcher)
};

// One launch; half_out: the outputs (and prev_positions / prev_normals) are
// half3 planes.  n == 0 or no output: launches nothing.
hipError_t launch_prepare(PrepareArgs a, bool half_out, hipStream_t st);

}  // namespace bmfr
