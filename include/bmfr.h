/* bmfr.h -- C ABI of libbmfr, the MI355X-native BMFR denoiser.
 *
 * This is the drop-in boundary for the reference's hot path, the per-frame
 * pipeline of /root/reference/opencl/bmfr.cl driven by tasks() in
 * /root/reference/opencl/bmfr.cpp.  The reference has no plugin API: its
 * boundary is (a) the JIT `-D` option set of bmfr.cpp:205-232, mirrored here
 * by bmfr_config, and (b) the five OpenCL kernel signatures with the argument
 * binding of bmfr.cpp:349-383,429-476, mirrored by the five stage entry
 * points below with the same argument roles and buffer layouts.  On top,
 * bmfr_process_frame runs one whole frame (the loop body of
 * bmfr.cpp:417-485) through the fused MI355X kernels.
 *
 * Conventions
 *  - Plain C: pointers, sizes and a status code.  No exceptions cross the ABI
 *    (the reference maps cl::Error to a return code, bmfr.cpp:558-578).
 *  - All buffer pointers are device pointers (hipMalloc / torch tensors).
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *  - Layouts (bmfr.cpp:315-347): float3 images are interleaved RGB f32 with
 *    row stride image_width; u8 planes (spp, accept) and float2 prev-pixel
 *    planes likewise; tmp_data is [block][feature][32*32] (bmfr.cl:455-464)
 *    in IEEE half (use_half_precision_in_tmp_data = 1) or f32; weights are
 *    [block][B-3][3] f32; mins_maxs are [block][FEATURES_SCALED][2] f32.
 *  - A context is not thread-safe; contexts are independent (one per GPU).
 */
#ifndef BMFR_H
#define BMFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMFR_VERSION_MAJOR 0
#define BMFR_VERSION_MINOR 3

#define BMFR_BLOCK_EDGE_LENGTH 32 /* bmfr.cpp:104; other sizes unsupported, as upstream */
#define BMFR_MAX_FEATURES 16      /* NOT_SCALED + SCALED feature buffers */
#define BMFR_MAX_AUX_FEATURES 4   /* caller-supplied feature planes (BMFR_FEATURE_AUX0..3) */

typedef enum bmfr_status {
    BMFR_OK = 0,
    BMFR_ERROR_INVALID_ARGUMENT = 1,
    BMFR_ERROR_UNSUPPORTED = 2,     /* e.g. a feature count with no compiled kernel */
    BMFR_ERROR_OUT_OF_MEMORY = 3,
    BMFR_ERROR_HIP = 4,             /* a HIP runtime call failed (see bmfr_last_hip_error) */
    BMFR_ERROR_NO_DEVICE = 5,
    BMFR_ERROR_HALO_EXCEEDED = 6,   /* tiled context: a frame reprojected past the exchanged halo
                                       (see tile_halo, bmfr_halo_status) */
    BMFR_ERROR_SYNC_TIMEOUT = 7     /* a fused kernel's bounded wait for another work-group gave up
                                       (see bmfr_frame_status): that frame's output is not valid */
} bmfr_status;

/* Feature buffer monomials.  The reference pastes C expressions into the
 * kernels (NOT_SCALED_FEATURE_BUFFERS / SCALED_FEATURE_BUFFERS, bmfr.cpp:65-77
 * -> FEATURE_BUFFERS, bmfr.cl:448-453,727-729); this ABI names them.  Any
 * other expression enters as a plane the caller evaluates:
 * BMFR_FEATURE_AUXk is bmfr_aux_inputs.aux[k] (see there). */
typedef enum bmfr_feature {
    BMFR_FEATURE_ONE = 0, /* "1.f" */
    BMFR_FEATURE_NORMAL_X, BMFR_FEATURE_NORMAL_Y, BMFR_FEATURE_NORMAL_Z,
    BMFR_FEATURE_POSITION_X, BMFR_FEATURE_POSITION_Y, BMFR_FEATURE_POSITION_Z,
    BMFR_FEATURE_POSITION_X2, BMFR_FEATURE_POSITION_Y2, BMFR_FEATURE_POSITION_Z2,
    BMFR_FEATURE_POSITION_X3, BMFR_FEATURE_POSITION_Y3, BMFR_FEATURE_POSITION_Z3,
    BMFR_FEATURE_AUX0, BMFR_FEATURE_AUX1, BMFR_FEATURE_AUX2, BMFR_FEATURE_AUX3, /* 13..16: aux[0..3] */
    BMFR_FEATURE_COUNT_
} bmfr_feature;

/* The reference's #define surface (bmfr.cpp:32-118, forwarded as -D at
 * bmfr.cpp:205-232).  Fill with bmfr_config_default() and override. */
typedef struct bmfr_config {
    int image_width;                     /* IMAGE_WIDTH  (bmfr.cpp:39) */
    int image_height;                    /* IMAGE_HEIGHT (bmfr.cpp:40) */
    int features_not_scaled;             /* FEATURES_NOT_SCALED (bmfr.cpp:195-196) */
    int features_scaled;                 /* FEATURES_SCALED     (bmfr.cpp:198-199) */
    int feature_buffers[BMFR_MAX_FEATURES]; /* FEATURE_BUFFERS: not-scaled then scaled */
    double noise_amount;                 /* NOISE_AMOUNT 1e-2 (a double, bmfr.cpp:58) */
    float blend_alpha;                   /* BLEND_ALPHA 0.2f        (bmfr.cpp:60) */
    float second_blend_alpha;            /* SECOND_BLEND_ALPHA 0.1f (bmfr.cpp:61) */
    float taa_blend_alpha;               /* TAA_BLEND_ALPHA 0.2f    (bmfr.cpp:62) */
    double position_limit_squared;       /* camera_matrices.h value; used as the
                                            kernel sees it: float(%g text), bmfr.cpp:226 */
    double normal_limit_squared;         /* idem, bmfr.cpp:227 */
    int use_half_precision_in_tmp_data;  /* USE_HALF_PRECISION_IN_TMP_DATA 1 (bmfr.cpp:88) */
    /* Spatial tile of a larger frame (multi-GPU sharding);
     * 0/0/0/0 = whole image.  image_width/height stay the WHOLE frame: block
     * grid, mirroring at the borders and reprojection are the whole frame's,
     * so a tile's output equals the same pixels of the untiled output.  The
     * context's buffers then cover the tile's REGION = the tile grown by
     * tile_halo pixels on each side, clipped to the frame (bmfr_sizes
     * region_*): every plane passed to bmfr_process_frame and every state
     * plane holds that region with row stride region_width.  Before each
     * frame > 0 the caller refreshes the region's halo ring of the state
     * planes (noisy_accumulated, spp, filtered_accumulated, result of
     * bmfr_state(previous = 0)) from the neighbouring tiles, which own those
     * pixels -- at least the parts bmfr_halo_need names for that frame.  Exact for scene motion below tile_halo - 34 pixels per frame
     * (32: blocks reaching past the tile, 2: TAA + bilinear taps); the
     * reference reprojects to any pixel (bmfr.cl:343-356), so the kernels
     * check it: a frame whose reprojection taps reach past the state that
     * is valid for them (the tile before the halo exchange, the region after
     * it) makes bmfr_halo_status -- and every later bmfr_process_frame* call
     * until frame_number 0 starts a new sequence -- return
     * BMFR_ERROR_HALO_EXCEEDED instead of diverging silently from the
     * untiled frame.  Canonical feature lists, fused path only (the stage API
     * rejects tiled contexts). */
    int tile_x, tile_y, tile_width, tile_height;
    int tile_halo;
    /* Input planes of bmfr_process_frame (noisy, normals, positions, albedo
     * and the previous normals / positions) in IEEE half, interleaved RGB
     * (6 bytes per pixel), instead of f32: the .exr files' own HALF channels
     * kept as they are (the reference converts them to FLOAT on load,
     * bmfr.cpp:157-159).  Values are widened exactly to f32 on load, so the
     * output equals the f32 path's on the widened planes bit for bit.
     * Canonical feature lists, fused path only (stage API: unsupported). */
    int input_half;
    /* powr(x, 0.454545f) of the tone map (bmfr.cl:854), whose rounding
     * OpenCL leaves to the device: 0 (default) = correctly rounded, equal to
     * the CPU oracle's (float)pow for every input, ~20 instructions;
     * 1 = the device library's __ocml_powr_f32, i.e. what the reference
     * kernel compiled for gfx950 computes (one in four results 1 ulp from
     * the correctly rounded one), ~130 instructions. */
    int library_powr;
    /* Householder trailing update of the fitter (bmfr.cl:606-655), each
     * element's t - 2 u dot / |u|^2: 0 (default) = upstream's roundings (u * c,
     * then / |u|^2, then the subtraction; the output equals the reference's
     * strict build bit for bit); 1 = one fused multiply-add on the block-wide
     * factor 2 dot / |u|^2, the wave-wide sums, minima and maxima as
     * butterflies, the noise added in f32 and the pivot's square root,
     * reciprocals and feature scaling at hardware precision (half tmp_data;
     * the f32 tmp_data K1 fuses the update only) -- no longer
     * bit-exact: TAA output within 1.2e-5 relative L2 of the reference's
     * strict build and 1.6e-5 of its default build at 3840x2160 (3.0e-5 at
     * B = 16; the two reference builds differ by ~1.2e-5), ~15 % less K1
     * time.  Applies to the fused K1 (canonical feature lists, half
     * or f32 tmp_data, every frame API); the stage fitter (bmfr_fitter) and
     * the arbitrary-feature-list K1 run the exact update. */
    int fast_fit;
} bmfr_config;

/* Sizes derived from a config (bmfr.cpp:104-118, 316-343). */
typedef struct bmfr_sizes {
    int buffer_count;       /* BUFFER_COUNT = not_scaled + scaled + 3 */
    int r_edge;             /* R_EDGE = BUFFER_COUNT - 2 */
    int workset_width, workset_height;                           /* WORKSET_* */
    int workset_with_margins_width, workset_with_margins_height; /* WORKSET_WITH_MARGINS_* */
    int blocks;             /* fitter work-groups, FITTER_GLOBAL / 256 */
    size_t tmp_data_bytes;  /* in_buffer, bmfr.cpp:322-324 */
    size_t weights_bytes;   /* bmfr.cpp:338-339 */
    size_t mins_maxs_bytes; /* sized from FEATURES_SCALED (bmfr.cpp:340 assumes 6) */
    size_t image_bytes;     /* one float3 plane, W*H*3*4 */
    /* Buffer region of the context (the whole frame unless tiled): pixels
     * [region_x, region_x + region_width) x [region_y, region_y + region_height). */
    int region_x, region_y, region_width, region_height;
    size_t region_bytes;    /* one float3 plane of the region */
    /* Kernel launches of an untiled bmfr_process_frame on the fused path
     * (canonical feature lists; profiling off): 1 (K1 blocks, then the TAA
     * tiles on completion flags) for frames below 4096 K1 blocks (`blocks`),
     * 2 (K1, then K2) from there -- measured faster at 4K / 8K, slower at
     * 1080p. */
    int frame_launches;
} bmfr_sizes;

typedef struct bmfr_ctx bmfr_ctx;

void bmfr_config_default(bmfr_config *cfg, int image_width, int image_height);
bmfr_status bmfr_config_sizes(const bmfr_config *cfg, bmfr_sizes *out);
const char *bmfr_status_string(bmfr_status s);
int bmfr_last_hip_error(void);
/* Identity of the compiled library: SHA-256 (hex) of the sources it was built
 * from, followed by "+<flags>" for a variant build.  No reference counterpart
 * (the reference JIT-compiles bmfr.cl at start-up, bmfr.cpp:234-243, so its
 * binary is always its source); here it ties a shipped binary to its tree. */
const char *bmfr_build_id(void);

/* Replaces clutils::CLEnv + the addContext/addQueue/addProgram calls
 * (bmfr.cpp:183-243): binds a HIP device and selects the kernels. */
bmfr_status bmfr_create(const bmfr_config *cfg, int hip_device, bmfr_ctx **out);
bmfr_status bmfr_destroy(bmfr_ctx *ctx);
bmfr_status bmfr_get_sizes(const bmfr_ctx *ctx, bmfr_sizes *out);

/* ---- Stage API: one entry per reference kernel, same argument roles ---- */

/* accumulate_noisy_data, bmfr.cl:290-308 (args bound at bmfr.cpp:351-352,429-447).
 * current_noisy is in/out like the reference.  Margin work-items read the
 * colours current_noisy held before the call (race-free form of
 * bmfr.cl:316-322 vs 478-481). */
bmfr_status bmfr_accumulate_noisy_data(bmfr_ctx *ctx, void *stream,
    float *out_prev_frame_pixel, uint8_t *accept_bools,
    const float *current_normals, const float *previous_normals,
    const float *current_positions, const float *previous_positions,
    float *current_noisy, const float *previous_noisy,
    const uint8_t *previous_spp, uint8_t *current_spp, void *tmp_data,
    const float prev_frame_camera_matrix[16], const float pixel_offset[2],
    int frame_number);

/* fitter, bmfr.cl:490-501 (args bound at bmfr.cpp:363-367,449-453).  The LDS
 * scratch arguments of the OpenCL kernel are internal here. */
bmfr_status bmfr_fitter(bmfr_ctx *ctx, void *stream, float *weights, float *mins_maxs,
    void *tmp_data, int frame_number);

/* weighted_sum, bmfr.cl:703-710 (bmfr.cpp:370-372,455-461).  current_noisy is
 * accepted for signature parity; the reference uses it only for debugging. */
bmfr_status bmfr_weighted_sum(bmfr_ctx *ctx, void *stream, const float *weights,
    const float *mins_maxs, float *output, const float *current_normals,
    const float *current_positions, const float *current_noisy, int frame_number);

/* accumulate_filtered_data, bmfr.cl:761-770 (bmfr.cpp:375-379,463-469). */
bmfr_status bmfr_accumulate_filtered_data(bmfr_ctx *ctx, void *stream,
    const float *filtered_frame, const float *in_prev_frame_pixel,
    const uint8_t *accept_bools, const float *albedo, float *tone_mapped_frame,
    const uint8_t *current_spp, const float *accumulated_prev_frame,
    float *accumulated_frame, int frame_number);

/* taa, bmfr.cl:860-865 (bmfr.cpp:382-383,471-476). */
bmfr_status bmfr_taa(bmfr_ctx *ctx, void *stream, const float *in_prev_frame_pixel,
    const float *new_frame, float *result_frame, const float *prev_frame,
    int frame_number);

/* ---- Frame API: the loop body of bmfr.cpp:417-485 on fused kernels ---- */

/* One frame's inputs (the four planes uploaded at bmfr.cpp:420-427) plus the
 * previous frame's normals/positions (the Double_buffer halves the reference
 * keeps, bmfr.cpp:316-319).  Temporal state (accumulated noisy colour, spp,
 * accumulated filtered colour, TAA output) lives in the context and is
 * double-buffered and swapped per frame like bmfr.cpp:482-484. */
typedef struct bmfr_frame_inputs {  /* float3 planes, or half3 with input_half */
    const void *noisy;           /* 1-spp colour (demodulated) */
    const void *normals;         /* shading normals */
    const void *positions;       /* world positions */
    const void *albedo;
    const void *prev_normals;    /* previous frame's normals (ignored at frame 0) */
    const void *prev_positions;  /* previous frame's positions (ignored at frame 0) */
    const float *prev_pixel;     /* optional per-pixel previous-frame pixel positions, see below (ignored at frame 0) */
} bmfr_frame_inputs;

/* prev_pixel: where each pixel was in the previous frame, for content the one
 * camera matrix cannot describe (moving or skinned objects, camera cuts, a
 * renderer with its own motion vectors).  NULL (a zero-initialised struct
 * that fills the first six members): the library projects `positions` through
 * prev_frame_camera_matrix, as the reference does (bmfr.cl:343-358).
 *
 * Layout: a float2 plane, always f32 -- also with input_half (half cannot
 * hold a 4K pixel coordinate with sub-pixel precision) --, W x H entries, or
 * the region (bmfr_sizes.region_*) with row stride region_width for a tiled
 * context.  Entry [y][x] = (pfx, pfy) is the previous-frame position of
 * pixel (x, y), in the coordinates of the value the library itself stores in
 * bmfr_state_view.prev_frame_pixel:
 *     pfx = u * W - jx,      pfy = v * H - (1 - jy),
 * with (u, v) in [0, 1]^2 the previous frame's screen position of the
 * pixel's surface point (u to the right, v in the direction of increasing
 * row index) and (jx, jy) = pixel_offset, the CURRENT frame's jitter.
 * Integer values are previous-frame pixel indices: (pfx, pfy) = (x, y)
 * means "was exactly at pixel (x, y)"; the four bilinear taps are
 * (floor(pfx) + {0,1}, floor(pfy) + {0,1}).
 *
 * From a renderer's screen-space motion vector (mx, my), in pixels, pointing
 * from the previous to the current screen position of a surface point: if
 * that point is seen at screen position (sx, sy) now (pixels, sx = u * W),
 * it was at (sx - mx, sy - my), so  pfx = sx - mx - jx,  pfy = sy - my -
 * (1 - jy).  Where (sx, sy) is depends on where the renderer samples pixel
 * (x, y):
 *   - at the jittered position this library assumes, (x + jx, y + 1 - jy)
 *     (the inverse of bmfr.cl:343-355): the jitter cancels,
 *         pfx = x - mx,  pfy = y - my;
 *   - at the pixel centre (x + 0.5, y + 0.5), unjittered vectors:
 *         pfx = x + 0.5 - mx - jx,  pfy = y + 0.5 - my - (1 - jy)
 *     (with the offset (0.5, 0.5) the two agree).
 * A static point under a static camera has (mx, my) = 0 and maps to itself.
 * Vectors in NDC units scale by W / 2 and H / 2 first; negate my if the
 * renderer's v grows against the row index.
 *
 * When prev_pixel is non-NULL and frame_number > 0 the kernels read neither
 * prev_frame_camera_matrix (which must still be non-NULL) nor pixel_offset
 * for reprojection.  Margin work-items (mirrored pixels, bmfr.cl:310-317)
 * read the plane at the mirrored pixel, as they read normals and positions.
 * An entry may be any float: taps outside the image are ignored, and an
 * entry all of whose taps are (far off, +-inf, NaN) restarts the pixel's
 * history -- spp 1, accumulated colour = current colour -- exactly as an
 * off-screen projection does.  In a tiled context the reach check applies to
 * the plane's taps as to projected ones (BMFR_ERROR_HALO_EXCEEDED).
 *
 * The plane only says WHERE to look.  Whether a tap is accepted is still the
 * reference's test of prev_positions / prev_normals at the tap against the
 * pixel's current position / normal (bmfr.cl:380-404).  For moving content
 * the caller therefore passes prev_positions and prev_normals moved into the
 * current frame's world: the previous frame's surface points transformed by
 * each object's motion since then, so that the tests compare like with like.
 * (For a static world they are simply the previous frame's planes.)
 *
 * Honoured by bmfr_process_frame, _interior / _border and
 * bmfr_process_sequence (per frame: NULL for some frames, set for others; a
 * sequence frame that carries a plane runs K1 and the previous frame's TAA as
 * two launches instead of one, with the same results).  The library keeps
 * writing bmfr_state_view.prev_frame_pixel: feeding a context the plane
 * another context computed reproduces that context bit for bit.  The stage
 * API is unchanged.
 *
 * bmfr_prepare_frame (below) computes this plane from a renderer's motion
 * vectors, both cases above, and moves prev_positions / prev_normals by one
 * rigid transform per object, on the GPU. */

/* One frame's caller-supplied feature planes, BMFR_FEATURE_AUX0..3.  They
 * travel beside bmfr_frame_inputs, whose layout is unchanged (seven
 * pointers), through the *_aux entry points below. */
typedef struct bmfr_aux_inputs {
    const float *aux[BMFR_MAX_AUX_FEATURES];
} bmfr_aux_inputs;

/* aux: feature planes the caller evaluates, for a regression feature the 13
 * named monomials cannot express -- the reference's FEATURE_BUFFERS takes any
 * C expression (bmfr.cpp:65-77), e.g. world_position.x*world_position.y --
 * or a noise-free quantity only the renderer has (linear depth, roughness, an
 * object id, albedo luminance).  A context whose feature_buffers names
 * BMFR_FEATURE_AUXk reads aux[k]; an aux code may stand anywhere in the list,
 * in the not-scaled or the scaled group, more than once, in any order.
 * Planes the list does not name are ignored, and for a list that names none
 * the whole struct may be NULL.
 *
 * Layout: one f32 per pixel, W x H entries, row stride W; device memory, read
 * only during the call's kernels; must not overlap any state plane.  The
 * plane always describes the CURRENT frame: features are evaluated at the
 * current pixel only, so there is no previous aux plane.
 *
 * Semantics: the reference's treatment of any feature expression; only the
 * source of the value is new.
 *   - The value of AUXk for a work-item is aux[k][lin], lin the same
 *     mirrored pixel index at which the work-item reads normals and positions
 *     (bmfr.cl:310-320).
 *   - In tmp_data it gets what every feature gets: NaN -> 0 and, with half
 *     tmp_data, the +-65504 clamp and rounding to half (bmfr.cl:448-473).
 *   - In the scaled group it is scaled by the block's min / max like a
 *     position feature (bmfr.cl:510-542); its mins_maxs slot is its position
 *     in the scaled list.
 *   - In the weighted sum the raw plane value is used again -- no NaN -> 0,
 *     no clamp, exactly as a named feature is recomputed at bmfr.cl:727-729
 *     --, scaled with the block's min / max if the feature is in the scaled
 *     group, then dotted with the weights in list order.
 * A plane that holds a named monomial's f32 values (one rounding per
 * operation: nx, px * px, (px * px) * px) therefore reproduces the named code
 * bit for bit.
 *
 * Passed through bmfr_process_frame_aux, _interior_aux / _border_aux on an
 * untiled context and bmfr_process_sequence_aux (one bmfr_aux_inputs per
 * frame): the entry points of the same names with one more argument, equal to
 * them when it is NULL.  With and without prev_pixel, half and f32 tmp_data,
 * library_powr 0 and 1.  Every frame entry point, with or without _aux,
 * returns BMFR_ERROR_INVALID_ARGUMENT, before anything is enqueued, when the
 * list names AUXk and the frame has no aux[k] (aux NULL, or aux[k] NULL).  A
 * list that names an aux code is
 * never canonical: fast_fit is ignored, tiled and input_half contexts are
 * BMFR_ERROR_UNSUPPORTED, as for any non-canonical list.  The stage API keeps
 * the reference's signatures: bmfr_accumulate_noisy_data and
 * bmfr_weighted_sum return BMFR_ERROR_UNSUPPORTED for such a context;
 * bmfr_fitter, which reads only tmp_data, works. */

/* prev_frame_camera_matrix: column-major view-projection of frame-1
 * (camera_matrices[max(frame-1,0)], bmfr.cpp:440-442); pixel_offset: the
 * frame's jitter (pixel_offsets[frame], bmfr.cpp:443-444).  frame_number 0
 * starts a new sequence. */
bmfr_status bmfr_process_frame(bmfr_ctx *ctx, void *stream, const bmfr_frame_inputs *in,
    const float prev_frame_camera_matrix[16], const float pixel_offset[2], int frame_number);

/* bmfr_process_frame in two calls, to overlap a tiled context's halo
 * exchange with compute.  _interior (noise table + the K1
 * blocks whose reads of the previous frame's state stay inside the tile, so
 * they need no halo) may be issued BEFORE the caller refreshes the halo ring
 * of bmfr_state(previous = 0) -- which still names the previous frame's
 * state until _border returns -- and runs while the exchange is in flight;
 * _border (same arguments, after the refresh is ordered before it on
 * `stream`) launches the remaining blocks and K2 and completes the frame.
 * The pair equals bmfr_process_frame bit for bit.  Untiled contexts: every
 * block is interior. */
bmfr_status bmfr_process_frame_interior(bmfr_ctx *ctx, void *stream, const bmfr_frame_inputs *in,
    const float prev_frame_camera_matrix[16], const float pixel_offset[2], int frame_number);
bmfr_status bmfr_process_frame_border(bmfr_ctx *ctx, void *stream, const bmfr_frame_inputs *in,
    const float prev_frame_camera_matrix[16], const float pixel_offset[2], int frame_number);

/* `count` consecutive frames first_frame .. first_frame+count-1 in one call
 * (the whole loop of bmfr.cpp:417-485 over frames already in device memory,
 * as tasks() holds the sequence in memory): in[i], the column-major
 * prev_frame_camera_matrices[16*i..] and pixel_offsets[2*i..] are frame
 * first_frame+i's arguments of bmfr_process_frame.  The frames are
 * pipelined: one launch per frame on `stream` runs K1 of frame f and, in its
 * tail, TAA of frame f-1 (half tmp_data, canonical feature lists), else TAA
 * of frame f (K2) runs on a context-owned stream beside K1 of frame f+1
 * (also with the environment variable BMFR_SEQUENCE=streams); all work is
 * joined back onto `stream`, so everything the call enqueues is complete
 * when `stream` reaches the point after it.  All
 * inputs must stay valid until then.  outputs (nullable; entries nullable):
 * outputs[i] receives frame i's output (W*H float3, device or page-locked
 * host memory).  Results equal bmfr_process_frame per frame bit for bit.
 * Untiled contexts only (tiles exchange a halo between frames). */
bmfr_status bmfr_process_sequence(bmfr_ctx *ctx, void *stream, int count, const bmfr_frame_inputs *in,
    const float *prev_frame_camera_matrices, const float *pixel_offsets, int first_frame,
    float *const *outputs);

/* The four entry points above with the frame's caller-supplied feature planes
 * (bmfr_aux_inputs, "aux" above; nullable: then they are the calls above).
 * bmfr_process_sequence_aux: aux[i] holds frame first_frame+i's planes. */
bmfr_status bmfr_process_frame_aux(bmfr_ctx *ctx, void *stream, const bmfr_frame_inputs *in,
    const bmfr_aux_inputs *aux, const float prev_frame_camera_matrix[16], const float pixel_offset[2],
    int frame_number);
bmfr_status bmfr_process_frame_interior_aux(bmfr_ctx *ctx, void *stream, const bmfr_frame_inputs *in,
    const bmfr_aux_inputs *aux, const float prev_frame_camera_matrix[16], const float pixel_offset[2],
    int frame_number);
bmfr_status bmfr_process_frame_border_aux(bmfr_ctx *ctx, void *stream, const bmfr_frame_inputs *in,
    const bmfr_aux_inputs *aux, const float prev_frame_camera_matrix[16], const float pixel_offset[2],
    int frame_number);
bmfr_status bmfr_process_sequence_aux(bmfr_ctx *ctx, void *stream, int count, const bmfr_frame_inputs *in,
    const bmfr_aux_inputs *aux, const float *prev_frame_camera_matrices, const float *pixel_offsets,
    int first_frame, float *const *outputs);

/* ---- G-buffer front end: from a renderer's buffers to bmfr_frame_inputs ----
 * (no reference counterpart: the reference reads a dataset that already holds
 * demodulated colour, world positions and float3 normals, bmfr.cpp:137-176).
 *
 * bmfr_prepare_frame turns what a renderer has -- radiance and albedo, a
 * depth buffer and a camera, packed normals, screen-space motion vectors, an
 * object id per pixel with one rigid transform per object -- into the planes
 * bmfr_process_frame takes, in one streaming kernel launch on `stream`.
 *
 * Planes: every G-buffer plane and every output covers the context's region
 * (bmfr_sizes.region_*; the whole image when untiled), row stride
 * region_width, one element per pixel in the plane's bmfr_format.  Pointers
 * are device memory aligned to the element's natural alignment (planes aligned
 * to 16 bytes take the kernel's wide accesses).  Outputs must not overlap
 * inputs.  Output planes are float3, or half3 in an input_half context (the
 * format bmfr_process_frame of that context reads); prev_pixel is always f32.
 * The same holds for the inputs prev_positions / prev_normals: they are a
 * previous call's PREPARED planes.  Below, (x, y) are IMAGE coordinates
 * (region_x + column, region_y + row), W x H the whole frame, (jx, jy) =
 * pixel_offset, the frame's jitter.
 *
 * Arithmetic: every line is one f32 operation rounded once, associated as
 * written, never contracted; division and square root correctly rounded;
 * half / unorm / snorm widen exactly; a half3 output is the f32 result
 * rounded to nearest even.
 *
 *  noisy, albedo <- radiance, albedo.  Per channel, a = the albedo as f32,
 *      d = (a > albedo_floor) ? a : albedo_floor   (a NaN albedo takes the floor)
 *      noisy = radiance / d;   albedo = a          (not floored: K2 remodulates
 *                                                    with the true albedo)
 *  positions <- positions (copied, narrowed for half3), or, when that is
 *      NULL, depth: the clip-space z / w inv_view_proj expects, with the
 *      pixel's sample at screen position (x + jx, y + 1 - jy), the inverse
 *      of the reprojection's convention (bmfr.cl:343-355):
 *      sx = float(x) + jx;              sy = float(y) + (1.0f - jy)
 *      nx = (sx / float(W)) * 2.0f - 1.0f;   ny likewise with H
 *      h_i = ((m[i]*nx + m[4+i]*ny) + m[8+i]*depth) + m[12+i],  i = 0..3
 *      position_i = h_i / h_3           (m = inv_view_proj, column-major)
 *  normals <- normals.  F32X3 / F16X4 pass through (not renormalised).
 *      OCT_SNORM16X2, per component e = float(s16) / 32767.0f, below -1: -1,
 *      z = (1.0f - |ex|) - |ey|
 *      z < 0:  ox = (1.0f - |ey|) * (ex >= 0 ? 1 : -1),
 *              oy = (1.0f - |ex|) * (ey >= 0 ? 1 : -1);   else (ox, oy) = (ex, ey)
 *      len = sqrt((ox*ox + oy*oy) + z*z);   n = (ox / len, oy / len, z / len)
 *  prev_pixel <- motion, the screen-space vector from the previous to the
 *      current position of the pixel's surface point:
 *      mx = mvx * motion_scale[0];   my = mvy * motion_scale[1]
 *      motion_at_pixel_centre = 0 (vector taken at the jittered sample):
 *          pfx = float(x) - mx;   pfy = float(y) - my
 *      motion_at_pixel_centre = 1 (at (x + 0.5, y + 0.5)):
 *          pfx = ((float(x) + 0.5f) - mx) - jx
 *          pfy = ((float(y) + 0.5f) - my) - (1.0f - jy)
 *      -- the two cases of the prev_pixel comment above.  Any motion value
 *      is legal (K1 makes any plane entry safe).
 *  prev_positions_moved, prev_normals_moved <- prev_positions, prev_normals,
 *      prev_object_id, object_transforms: the previous frame's planes moved
 *      into the current frame's world.  id = prev_object_id[pixel]; if id <
 *      n_objects, with M = object_transforms + 12 * id (row-major 3x4,
 *      previous world -> current world, a rigid motion: no renormalisation,
 *      no inverse transpose):
 *          p'_i = ((M[4i]*p.x + M[4i+1]*p.y) + M[4i+2]*p.z) + M[4i+3]
 *          n'_i =  (M[4i]*n.x + M[4i+1]*n.y) + M[4i+2]*n.z
 *      otherwise (ids at or past the table -- 0xFFFF is never in it --, or
 *      n_objects = 0, for which prev_object_id may be NULL) the pixel is
 *      copied unchanged, byte for byte.
 *
 * Each non-NULL member of bmfr_prepared is computed.  Returns
 * BMFR_ERROR_INVALID_ARGUMENT for a NULL g / out / pixel_offset, a requested
 * output one of whose inputs is NULL, n_objects outside 0..65535 or n_objects
 * > 0 with NULL object_transforms, and for a NULL ctx;
 * BMFR_ERROR_UNSUPPORTED for a non-NULL plane whose format is not listed for
 * it below.  g and out are checked first, in that order, so they can be
 * validated without a context.  A call that requests nothing launches nothing
 * and returns BMFR_OK.  Costs about one device copy of the same bytes
 * (DESIGN.md "G-buffer front end"). */
typedef enum bmfr_format {       /* element formats of G-buffer planes */
    BMFR_FORMAT_NONE = 0,
    BMFR_FORMAT_F32X3,           /* interleaved, 12 B/px (the library's own float3 planes) */
    BMFR_FORMAT_F16X4,           /* 8 B/px, 4th component ignored (RGBA16F) */
    BMFR_FORMAT_UNORM8X4,        /* 4 B/px, v / 255, 4th ignored; albedo only */
    BMFR_FORMAT_OCT_SNORM16X2,   /* 4 B/px octahedral unit vector; normals only */
    BMFR_FORMAT_F32X2,           /* 8 B/px; motion only */
    BMFR_FORMAT_F16X2,           /* 4 B/px; motion only */
    /* output surfaces only (bmfr_resolve_output; bmfr_prepare_frame: unsupported) */
    BMFR_FORMAT_UNORM8X3,        /* 3 B/px packed RGB (the PNG row format) */
    BMFR_FORMAT_UNORM10X3A2      /* 4 B/px, one little-endian u32: R bits 0-9, G 10-19, B 20-29, A 30-31 */
} bmfr_format;

typedef struct bmfr_gbuffer {    /* what the renderer has; every pointer nullable */
    const void *radiance;        /* F32X3 | F16X4 */
    int radiance_format;
    const void *albedo;          /* F32X3 | F16X4 | UNORM8X4 */
    int albedo_format;
    float albedo_floor;          /* demodulation guard */
    const void *normals;         /* F32X3 | F16X4 | OCT_SNORM16X2 */
    int normal_format;
    const float *positions;      /* F32X3 world positions, or NULL and: */
    const float *depth;          /* f32, the clip-space z / w inv_view_proj expects */
    float inv_view_proj[16];     /* column-major inverse of THIS frame's view-projection */
    const void *motion;          /* F32X2 | F16X2, previous -> current screen position */
    int motion_format;
    float motion_scale[2];       /* to pixels: (1, 1); NDC units: (W / 2, H / 2); negate [1] if v runs against rows */
    int motion_at_pixel_centre;  /* 0: taken at the jittered sample; 1: at (x + .5, y + .5) */
    const void *prev_positions;  /* last frame's PREPARED planes (float3, or half3 with input_half) */
    const void *prev_normals;
    const uint16_t *prev_object_id;   /* per pixel of the previous frame */
    const float *object_transforms;   /* n_objects x 12 floats, row-major 3x4, previous world -> current world */
    int n_objects;
} bmfr_gbuffer;

typedef struct bmfr_prepared {   /* outputs, nullable; float3 planes, or half3 with input_half */
    void *noisy;
    void *normals;
    void *positions;
    void *albedo;
    float *prev_pixel;           /* float2, always f32 */
    void *prev_positions_moved;
    void *prev_normals_moved;
} bmfr_prepared;

/* Zeroes *g; albedo_floor = 1 / 255 (the smallest non-zero 8-bit albedo),
 * motion_scale = (1, 1). */
void bmfr_gbuffer_default(bmfr_gbuffer *g);
bmfr_status bmfr_prepare_frame(bmfr_ctx *ctx, void *stream, const bmfr_gbuffer *g,
    const bmfr_prepared *out, const float pixel_offset[2]);

/* Halo exchange support for tiled contexts: copy the rectangles rects[n][5]
 * = {x, y, width, height, planes} (image coordinates inside the context's
 * region; planes = a non-empty mask of BMFR_HALO_*) of the exchanged state
 * planes of bmfr_state(previous = 0) -- noisy_accumulated (12 B/px), spp
 * (1), filtered_accumulated (12), result (12) -- into (unpack = 0) or out of
 * (unpack = 1) `buffer` (device memory), rectangle after rectangle, plane
 * after plane in that order, rows packed, each segment padded to 16 bytes;
 * one kernel launch on `stream`.  *bytes (nullable) receives the packed
 * size; buffer = NULL only computes it.  At most 64 segments (rectangle x
 * plane). */
#define BMFR_HALO_NOISY 1
#define BMFR_HALO_SPP 2
#define BMFR_HALO_FILTERED 4
#define BMFR_HALO_RESULT 8
#define BMFR_HALO_STATE (BMFR_HALO_NOISY | BMFR_HALO_SPP | BMFR_HALO_FILTERED)
#define BMFR_HALO_ALL (BMFR_HALO_STATE | BMFR_HALO_RESULT)
bmfr_status bmfr_halo_copy(bmfr_ctx *ctx, void *stream, const int *rects, int n, void *buffer, int unpack,
    size_t *bytes);

/* What frame `frame_number` of a tiled configuration reads of the previous
 * frame's state ({x, y, width, height}, inside the region; host only, no
 * context): state_rect for noisy_accumulated / spp / filtered_accumulated --
 * the pixels of the frame's K1 blocks (its shifted block grid, bmfr.cl:
 * 267-285; mirrored at the frame border) grown by tile_halo - 33 --, and
 * result_rect for the TAA output -- the tile grown by tile_halo - 33.
 * Before frame_number the caller must refresh the parts of these
 * rectangles outside the tile (refreshing the whole halo ring is also
 * correct); the kernels check the reprojection taps against them.  Both
 * depend on frame_number % 16 only. */
bmfr_status bmfr_halo_need(const bmfr_config *cfg, int frame_number, int state_rect[4], int result_rect[4]);

/* ---- Multi-GPU halo exchange (SURVEY.md 5 "Distributed communication
 * backend", 8e; no reference counterpart: the reference drives one GPU,
 * bmfr.cpp:183-191) ----
 * A tile grid is ntiles rectangles tiles[4 r .. 4 r + 3] = {x, y, width,
 * height} partitioning the frame; rank r runs a tiled context whose
 * bmfr_config has tile_* = tile r (same tile_halo for every rank).
 *
 * bmfr_halo_plan: what rank `rank` exchanges before frame_number (host only):
 * for each of the *n_peers neighbours, peers[k], then send_counts[k]
 * bmfr_halo_copy records of its own tile that the neighbour's frame reads,
 * then recv_counts[k] records of the neighbour's tile its own frame reads,
 * all in `records` (5 ints each, at most max_records).  peers = records =
 * NULL only counts.  Depends on frame_number % 16.  (bmfr_amd/tiling.py
 * TileGrid.frame_plan is the same plan.) */
bmfr_status bmfr_halo_plan(const bmfr_config *cfg, const int *tiles, int ntiles, int rank, int frame_number,
    int *peers, int *send_counts, int *recv_counts, int *records, int max_records, int *n_peers);

/* RCCL communicator of one rank (RCCL is loaded at run time; without it the
 * calls return BMFR_ERROR_UNSUPPORTED).  One process per GPU: rank 0 makes
 * the id (bmfr_comm_unique_id), every rank receives it out of band (e.g.
 * torch.distributed / MPI broadcast) and calls bmfr_comm_create.  One
 * process driving several GPUs: bmfr_comm_create_all (out[i] = rank i, on
 * devices[i]). */
typedef struct bmfr_comm bmfr_comm;
bmfr_status bmfr_comm_unique_id(unsigned char id[128]);
bmfr_status bmfr_comm_create(const unsigned char id[128], int nranks, int rank, int hip_device, bmfr_comm **out);
bmfr_status bmfr_comm_create_all(int ndev, const int *devices, bmfr_comm **out);
bmfr_status bmfr_comm_destroy(bmfr_comm *comm);

/* The per-frame exchange of one rank: the plans of all 16 block-grid shifts
 * and device send / receive buffers are made once here (cfg = the rank's
 * context configuration; comm = its communicator, or NULL for an in-process
 * grid).  bmfr_exchange_run, before frame_number > 0 of the context (after the
 * previous frame, before bmfr_process_frame_border -- or before
 * bmfr_process_frame), enqueues on `stream`: one pack kernel
 * (bmfr_halo_copy), one ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd
 * batch to the neighbours, one unpack kernel.  bmfr_exchange_run_all: every
 * rank of a grid held by this process -- with communicators
 * (bmfr_comm_create_all) all messages in one group, streams[i] rank i's
 * stream; without, every context on one device and everything on
 * streams[0] as device copies (single-GPU runs of a tiled grid). */
typedef struct bmfr_exchange bmfr_exchange;
bmfr_status bmfr_exchange_create(bmfr_ctx *ctx, const bmfr_config *cfg, const int *tiles, int ntiles, int rank,
    bmfr_comm *comm, bmfr_exchange **out);
bmfr_status bmfr_exchange_run(bmfr_exchange *x, void *stream, int frame_number);
bmfr_status bmfr_exchange_run_all(bmfr_exchange *const *xs, int n, void *const *streams, int frame_number);
/* Bytes rank x sends / receives before frame_number. */
bmfr_status bmfr_exchange_bytes(const bmfr_exchange *x, int frame_number, size_t *sent, size_t *received);
bmfr_status bmfr_exchange_destroy(bmfr_exchange *x);

/* Tiled contexts: waits for the last enqueued frame and returns
 * BMFR_ERROR_HALO_EXCEEDED if any frame since frame 0 read reprojection taps
 * past its valid state (see tile_halo), BMFR_OK otherwise; *overshoot
 * (nullable) receives the largest distance in pixels.  Untiled: BMFR_OK.
 * BMFR_ERROR_SYNC_TIMEOUT takes precedence (see bmfr_frame_status). */
bmfr_status bmfr_halo_status(bmfr_ctx *ctx, unsigned *overshoot);

/* Waits for the last enqueued frame and returns the context's sticky report:
 * BMFR_ERROR_SYNC_TIMEOUT if, in any frame since frame 0, a bounded wait of
 * the fused kernels gave up -- a K1 wave waiting for the pivot column another
 * wave of its work-group publishes in LDS, or (one-launch frame) a TAA tile
 * waiting for the completion flags of the K1 blocks under it; the kernels run
 * to their end regardless (no wave waits forever), so that frame's output and
 * state are not valid --, else BMFR_ERROR_HALO_EXCEEDED as bmfr_halo_status,
 * else BMFR_OK.  Every bmfr_process_frame* / bmfr_process_sequence call
 * returns the same report, without waiting, once the host has seen it, until
 * frame_number 0 starts a new sequence (frame 0 first waits for every frame
 * enqueued before it, then clears the reports).  The wait is an event the
 * library records at that point on the stream of the last enqueued frame
 * (none between frames: a marker between two frames' kernels costs GPU time),
 * so it also waits for work the caller queued on that stream after the frame;
 * if that stream no longer exists it waits for the whole device. */
bmfr_status bmfr_frame_status(bmfr_ctx *ctx);

/* Device pointer to the last processed frame's output (TAA result, float3,
 * W*H, the buffer the reference reads back at bmfr.cpp:479-480).  Valid until
 * the next bmfr_process_frame. */
const float *bmfr_output(const bmfr_ctx *ctx);

/* Device pointers to the context's temporal state of the last frame, for
 * inspection / multi-GPU halo exchange: accumulated noisy colour (float3),
 * spp (u8), accumulated filtered colour (float3), prev-frame pixel (float2).
 * tone_mapped is only materialised by the generic-feature fallback (the
 * canonical path tone-maps inside the TAA kernel) and accept bits never are
 * (NULL). */
typedef struct bmfr_state_view {
    float *noisy_accumulated;
    uint8_t *spp;
    float *filtered_accumulated;
    float *tone_mapped;
    float *prev_frame_pixel;
    uint8_t *accept;
    float *result;
} bmfr_state_view;
bmfr_status bmfr_state(const bmfr_ctx *ctx, int previous, bmfr_state_view *out);

/* ---- Output back end: from the context's state to a renderer's surface ----
 * (no reference counterpart: the reference reads the float3 result back and
 * quantises on the CPU, bmfr.cpp:479-480, 519-553).
 *
 * bmfr_resolve_output is the symmetric call to bmfr_prepare_frame: it writes
 * the last processed frame into a surface in the format a swapchain or a post
 * chain takes -- 8-bit, 10-bit or half / float, with a row pitch, an origin,
 * rows bottom-up if wanted -- in one streaming kernel launch on `stream`.
 *
 * Which pixels.  The context's TILE (tile_*; the whole frame when untiled)
 * is written, never the halo.  Frame pixel (x, y) goes to surface pixel
 *     (origin_x + x,  origin_y + (flip_y ? H - 1 - y : y)),   H = image_height.
 * Nothing else of the surface is written: not pixels outside the tile's image,
 * not the bytes of a row past width * bytes_per_pixel (pitch padding), not a
 * fourth byte after a UNORM8X3 pixel.  A negative origin lets a rank resolve
 * into a tile-sized surface (origin = -tile_x, -tile_y); origin 0 lets all
 * tiles of a grid resolve into one whole-frame surface.
 *
 * Source value v per channel.  Every line is one f32 operation rounded once,
 * associated as written, never contracted.
 *   BMFR_RESOLVE_OUTPUT: the last processed frame's TAA result, the plane
 *      bmfr_output() names (display-referred, in [0, 1]).  albedo is ignored.
 *   BMFR_RESOLVE_HDR:  v = a * f,  the linear colour the tone map starts from
 *      (bmfr.cl:851-856): f = that frame's filtered_accumulated
 *      (bmfr_state_view), a = `albedo`, the frame's albedo plane as given to
 *      bmfr_process_frame -- the region with row stride region_width, f32x3,
 *      or half3 widened exactly in an input_half context.
 *
 * Encoding.
 *   F32X3        the bits of v.
 *   F16X4        (half)v, round to nearest even; overflow goes to +-inf, NaN
 *                stays NaN.  4th component: (half)alpha.
 *   UNORM8X4 / UNORM8X3
 *                c = v > 0 ? (v < 1 ? v : 1) : 0          (NaN -> 0)
 *                q = (uint)floorf(c * 255.0f + 0.5f)
 *                4th byte of X4: the same rule applied to alpha.
 *   UNORM10X3A2  the same with 1023.0f; A = floorf(clamp(alpha) * 3.0f + 0.5f).
 *   bgr swaps which source channel lands in component 0 and component 2, in
 *   every format.
 *
 * Ordering.  The call reads the state of the last processed frame; it is
 * enqueued on `stream` and must be ordered after that frame by the caller
 * (the same stream, or an event).  Valid until the next bmfr_process_frame*,
 * like bmfr_output().  It launches one kernel and changes neither the
 * context's state, nor the frame status, nor what bmfr_frame_status waits for.
 *
 * Errors.  dst is checked first and without a context.
 * BMFR_ERROR_INVALID_ARGUMENT: NULL dst or data; width or height <= 0; pitch <
 * width * bytes_per_pixel; data or pitch not a multiple of the element's
 * natural alignment (4 for F32X3, UNORM8X4 and UNORM10X3A2, 8 for F16X4, 1 for
 * UNORM8X3); source not one of the two values; BMFR_RESOLVE_HDR with NULL
 * albedo; then, with a context: NULL ctx, no processed frame yet, a pending
 * _interior without its _border, or the mapped tile rectangle not inside
 * [0, width) x [0, height).  BMFR_ERROR_UNSUPPORTED: a format outside the
 * five listed.  Nothing is written when an error is returned. */
typedef struct bmfr_surface {
    void  *data;        /* device memory (or page-locked host memory the device can write) */
    int    format;      /* F32X3 | F16X4 | UNORM8X4 | UNORM8X3 | UNORM10X3A2 */
    size_t pitch;       /* bytes between surface rows */
    int    width, height;      /* surface size in pixels */
    int    origin_x, origin_y; /* surface pixel of frame pixel (0, 0); may be negative */
    int    flip_y;      /* 1: frame row y lands on surface row origin_y + (H - 1 - y) */
    int    bgr;         /* 1: channels 0 and 2 swapped (BGRA8, B10G10R10A2, ...) */
    float  alpha;       /* 4th component of X4 / A2 formats */
} bmfr_surface;
typedef enum bmfr_resolve_source { BMFR_RESOLVE_OUTPUT = 0, BMFR_RESOLVE_HDR = 1 } bmfr_resolve_source;

void bmfr_surface_default(bmfr_surface *s);   /* zeroes *s; alpha = 1 */
bmfr_status bmfr_resolve_output(bmfr_ctx *ctx, void *stream, int source,
                                const void *albedo, const bmfr_surface *dst);

/* ---- Guided upsampling: a frame traced below display resolution ----
 * (no reference counterpart: the reference denoises and shows one resolution.)
 *
 * A renderer that traces at W x H and shows Wd x Hd still rasterises its
 * G-buffer -- albedo, normals, depth -- at display resolution.  What the
 * library filters and accumulates, filtered_accumulated, is irradiance with the
 * texture detail divided out, so it stretches well; the detail is in the
 * albedo, which the renderer has at full resolution.  bmfr_upsample_output
 * interpolates the last processed frame's filtered_accumulated to Wd x Hd,
 * leaving out the taps that lie on another surface than the display pixel,
 * multiplies by the display-resolution albedo and writes a bmfr_surface, in one
 * kernel launch on `stream`.  It delivers the denoised, temporally accumulated,
 * remodulated image; it does not itself run TAA at display resolution:
 * bmfr_display_taa, below, takes the surface it wrote and does.
 *
 * Planes.  The guides cover Wd x Hd with row stride Wd, one element per pixel
 * in the plane's bmfr_format, device memory aligned to the element (4 bytes;
 * 8 for F16X4).  frame_normals / frame_positions are the frame's planes as
 * given to bmfr_process_frame: W x H, f32x3, or half3 widened exactly in an
 * input_half context.  dst is a bmfr_surface as bmfr_resolve_output takes it;
 * the frame that is placed has size Wd x Hd: display pixel (X, Y) goes to
 * surface pixel (origin_x + X, origin_y + (flip_y ? Hd - 1 - Y : Y)), and
 * nothing else of the surface is written.
 *
 * Arithmetic: every line is one f32 operation rounded once, associated as
 * written, never contracted, with division correctly rounded.  For display
 * pixel (X, Y), W x H the context's frame:
 *
 *  1. Footprint.  rx = float(W) / float(Wd), ry = float(H) / float(Hd), once.
 *       u = (float(X) + 0.5f) * rx - 0.5f;    v = (float(Y) + 0.5f) * ry - 0.5f
 *       x0 = floorf(u);  fx = u - x0;         y0 = floorf(v);  fy = v - y0
 *     Taps k = (i, j) in the order 00, 10, 01, 11 at frame pixel
 *       (clamp(x0 + i, 0, W - 1),  clamp(y0 + j, 0, H - 1))    with weight
 *       w_k = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy)
 *  2. Display guides.  A (albedo), N (normal), P (world position) of the
 *     display pixel come from the guides, decoded exactly as bmfr_prepare_frame
 *     decodes the same formats -- the octahedral rule included, and for `depth`
 *     the position-from-depth lines with (x, y) = (X, Y), (W, H) = (Wd, Hd) and
 *     (jx, jy) = the guides' pixel_offset.
 *  3. Tap test.  n_k, p_k = frame_normals / frame_positions at the tap.
 *       dp = p_k - P;    d = (dp.x*N.x + dp.y*N.y) + dp.z*N.z
 *       dn = n_k - N;    q = (dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z
 *     The tap is accepted when
 *       w_k > 0 && d*d < plane_limit_squared && q < normal_limit_squared
 *     (a NaN compares false).  d is the distance to the display pixel's tangent
 *     plane, not the Euclidean distance: the test does not depend on the
 *     pixel footprint.
 *  4. Accumulate.  e_k = filtered_accumulated at the tap.  sw = the sum, in
 *     tap order, of w_k over the accepted taps, and sc that of w_k * e_k per
 *     channel; a sum begins with its first term (a single tap of weight 1
 *     passes e_k through, the sign of a zero included).
 *       accepted taps exist and sw > 0:   e = sc / sw
 *       otherwise the pixel falls back: the same sums over every tap with
 *       w_k > 0, and stats[0] counts the pixel.
 *     A tap of weight 0 is never read into a sum: 0 * NaN does not reach e.
 *  5. Unguided mode: normals NULL, and positions and depth both NULL.  Every
 *     tap with w_k > 0 is accepted and stats counts nothing.
 *  6. Source value.  c = A * e per channel.
 *       BMFR_UPSAMPLE_HDR:         v = c
 *       BMFR_UPSAMPLE_TONEMAPPED:  v = min(max(powr(max(0, c), 0.454545f), 0), 1)
 *     with the correctly rounded powr (the function tone_map uses by default,
 *     equal to the oracle's (float)pow) whatever the context's library_powr.
 *     v is encoded exactly as bmfr_resolve_output encodes it (bgr, alpha).
 *
 * Ordering and state as bmfr_resolve_output: enqueued on `stream`, ordered
 * after the frame by the caller, valid until the next bmfr_process_frame*.
 * It reads filtered_accumulated and changes neither the context's state, nor
 * the frame status, nor what bmfr_frame_status waits for.
 *
 * stats (nullable): one uint32_t in device memory, the fallback pixels.  The
 * call adds to it; the caller zeroes it.
 *
 * Known limit: tiled contexts are refused (BMFR_ERROR_UNSUPPORTED).  A tile's
 * taps reach one pixel past it, and the halo of filtered_accumulated there
 * holds the previous exchange, not this frame; exchanging a one-pixel ring
 * after the frame is a follow-up.
 *
 * Errors.  dst is checked first and without a context, as
 * bmfr_resolve_output checks it, then source and the guides, then the context.
 * BMFR_ERROR_INVALID_ARGUMENT: source not one of the two values; NULL g or
 * albedo; exactly one of normals and a position source (positions or depth)
 * given; NULL frame_normals or frame_positions in guided mode; a limit that
 * is not finite or not > 0; a guide plane, a frame plane or stats not aligned
 * to its element; then, with a context: NULL ctx, no processed frame yet, a
 * pending _interior without its _border, a size outside W <= Wd <= 4 W,
 * H <= Hd <= 4 H, or the mapped Wd x Hd rectangle not inside the surface.
 * BMFR_ERROR_UNSUPPORTED: a surface format outside the five listed, a guide
 * format not listed for its plane, a tiled context.  Nothing is written and
 * nothing is enqueued when an error is returned. */
typedef struct bmfr_upsample_guides {  /* the renderer's display-resolution G-buffer: Wd x Hd, row stride Wd */
    int width, height;                 /* Wd, Hd:  W <= Wd <= 4 W,  H <= Hd <= 4 H */
    const void *albedo;   int albedo_format;   /* F32X3 | F16X4 | UNORM8X4; required */
    const void *normals;  int normal_format;   /* F32X3 | F16X4 | OCT_SNORM16X2; nullable */
    const float *positions;            /* F32X3 world positions, or NULL and: */
    const float *depth;                /* f32 clip-space z / w, with */
    float inv_view_proj[16];           /* column-major, and */
    float pixel_offset[2];             /* the display G-buffer's own jitter */
    float plane_limit_squared;         /* rule 3 */
    float normal_limit_squared;
} bmfr_upsample_guides;
typedef enum bmfr_upsample_source { BMFR_UPSAMPLE_HDR = 0, BMFR_UPSAMPLE_TONEMAPPED = 1 } bmfr_upsample_source;

/* Zeroes *g; both limits = the values the kernels see for cfg's
 * position_limit_squared and normal_limit_squared (float of their "%g" text;
 * cfg = NULL: of bmfr_config_default's). */
void bmfr_upsample_guides_default(bmfr_upsample_guides *g, const bmfr_config *cfg);
bmfr_status bmfr_upsample_output(bmfr_ctx *ctx, void *stream, int source,
    const void *frame_normals, const void *frame_positions,   /* the frame's planes as given to bmfr_process_frame */
    const bmfr_upsample_guides *g, const bmfr_surface *dst, uint32_t *stats /* device, nullable */);

/* ---- Display-resolution TAA: anti-aliasing what the renderer shows ----
 * (the reference's taa kernel, bmfr.cl:860-974, on planes the caller owns.)
 *
 * The library's own TAA (K2) runs at the resolution the frame was traced at.
 * A renderer that traces at W x H and shows Wd x Hd shows what
 * bmfr_upsample_output wrote, and its display-resolution albedo is rasterised
 * with a moving jitter: every texture and geometry edge crawls.
 * bmfr_display_taa applies the reference's TAA to that image: `current` (this
 * frame's display-resolution colour), `history` (the previous call's result)
 * and a display-resolution reprojection plane give `result`, and, in the same
 * pass, the presentable surface `dst` -- one kernel launch on `stream`.  The
 * caller ping-pongs two planes: this call's `result` is the next call's
 * `history`.  With dst the low-resolution frame order needs no further resolve
 * call: prepare -> (firefly) -> frame -> upsample (tone-mapped, into an F16X4
 * or F32X3 surface) -> display TAA (dst = the swapchain image).
 *
 * The colour space is the caller's.  The reference clamps tone-mapped values,
 * so BMFR_UPSAMPLE_TONEMAPPED is the intended `current`.
 *
 * Planes.  current, history and result are bmfr_plane: Wd x Hd pixels, F32X3
 * or F16X4 (4th component ignored when read; half values widen exactly), rows
 * `pitch` bytes apart, device memory aligned to the element (4 bytes; 8 for
 * F16X4), each in its own format, a pitch at most 2^31 bytes.  result must
 * not overlap current or history, and dst must not overlap any of the three:
 * the kernel reads neighbours and taps that another thread's store would
 * overwrite.  Only result.data equal to current.data or history.data is
 * detected and refused; any other overlap is undefined.  prev_pixel is an F32X2 plane of Wd x Hd entries with row stride Wd:
 * bmfr_frame_inputs.prev_pixel's convention with (W, H) = (Wd, Hd), i.e.
 *     pfx = u * Wd - jx,      pfy = v * Hd - (1 - jy),
 * (u, v) the previous frame's screen position of the display pixel's surface
 * point and (jx, jy) the display G-buffer's current jitter.  Or prev_pixel is
 * NULL and `motion` holds display-resolution motion vectors, with
 * motion_format, motion_scale, motion_at_pixel_centre and pixel_offset exactly
 * bmfr_gbuffer's fields and rule.
 *
 * Arithmetic: the reference's, as K2 computes it.  Every line is one f32
 * operation rounded once, associated as written, never contracted, with
 * division correctly rounded; min / max ignore a NaN operand (and order -0
 * below +0).  The two colour transforms are the reference's dot():
 *     ycocg(c) = (dot(c, (1, 2, 1)), dot(c, (2, 0, -2)), dot(c, (-1, 2, -1)))
 *     rgb(c)   = (dot(c, (.25, .25, -.25)), dot(c, (.25, 0, .25)), dot(c, (.25, -.25, -.25)))
 *     dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))
 * -- every coefficient is a power of two, so each product is exact and a dot
 * is two rounded additions wherever no product overflows or underflows.  For
 * display pixel (X, Y), W = Wd, H = Hd, a = blend_alpha:
 *
 *  1. Own colour.  me = current[Y][X].
 *  2. Previous position.  (pfx, pfy) = prev_pixel[Y][X], or from motion[Y][X]
 *     the "prev_pixel <- motion" lines of bmfr_prepare_frame with (x, y) =
 *     (X, Y) and (jx, jy) = pixel_offset.
 *  3. Off-screen test.  flx = floorf(pfx), fly = floorf(pfy).  If reset, or
 *     history.data is NULL, or  flx < -1 || fly < -1 || flx >= float(W) ||
 *     fly >= float(H)  (compared as floats; a NaN compares false and goes on,
 *     as in K2):  v = me, and rules 4-6 do not apply.
 *  4. Neighbourhood bounds (bmfr.cl:893-920).  Over the pixels (X + dx,
 *     Y + dy), dx, dy in -1..1, that lie inside the image, s = ycocg(current):
 *     mnb / mxb = the minimum / maximum over all of them (the box), mnc / mxc
 *     over those with dx = 0 or dy = 0 (the cross), per component, each
 *     starting from +inf / -inf.
 *  5. History (bmfr.cl:925-966).
 *       ix = (int)min(max(flx, -2.0f), float(W) + 1.0f);   iy likewise with H
 *       fx = pfx - flx;  fy = pfy - fly;  omx = 1.0f - fx;  omy = 1.0f - fy
 *     Taps k = (i, j) in the order 00, 10, 01, 11 at history pixel
 *     (ix + i, iy + j) with weight  w_k = (i ? fx : omx) * (j ? fy : omy).
 *     A tap enters when  (i ? ix < W - 1 : ix >= 0) && (j ? iy < H - 1 : iy >= 0):
 *       prev = prev + w_k * history_k   per channel;   total = total + w_k
 *     both starting from 0.  A tap of weight 0 is multiplied in, as in the
 *     reference: a NaN or inf history value reaches prev.  (Past rule 3 a
 *     tap that enters lies inside the plane, except for a NaN pfx or pfy:
 *     then the nearest pixel inside is read, and every weight is NaN.)  Then
 *       prev = prev / total;   py = ycocg(prev)
 *  6. Clamp and blend (bmfr.cl:922-973).  Per component
 *       lo = (mnb + mnc) / 2.0f;   hi = (mxb + mxc) / 2.0f
 *       cl = min(max(py, lo), hi)                  (a NaN py becomes lo)
 *       pr = rgb(cl);   b = 1.0f - a;   v = a * me + b * pr
 *     so a NaN in history does not survive a frame whose current
 *     neighbourhood is finite.
 *  7. Outputs.  result[Y][X] = the bits of v (F32X3), or (half)v rounded to
 *     nearest even with 4th component (half)1 (F16X4).  A non-NULL dst
 *     receives the f32 v -- not the half-rounded one -- encoded exactly as
 *     bmfr_resolve_output encodes it (five formats, bgr, alpha) at surface
 *     pixel (origin_x + X, origin_y + (flip_y ? Hd - 1 - Y : Y)).  Nothing
 *     else of dst, and nothing of result's pitch padding, is written.
 *
 * With blend_alpha = 1 the result is current wherever pr is finite; with
 * reset = 1 (the reference's frame 0 -- a camera cut, the first frame, a
 * resized window) or history.data NULL it is current bit for bit, and
 * history, prev_pixel and motion are not read.
 *
 * Launch and state.  One kernel on `stream`; the caller orders it after the
 * writer of `current` (the same stream, or an event).  The context only names
 * the device: the call reads and changes no context state, no frame status and
 * nothing bmfr_frame_status waits for; it is legal before any frame and on any
 * context, tiled ones included, and width x height is independent of the
 * context's size.
 *
 * Out of scope: fusing with bmfr_upsample_output (the clamp needs the nine
 * neighbours' finished values); display planes tiled over several GPUs; the
 * bmfr_host program and the stage API, which keep the reference's one
 * resolution.
 *
 * Errors, in this order; nothing is enqueued or written when one is returned.
 * A non-NULL dst is checked first, as bmfr_resolve_output checks it, without a
 * context.  BMFR_ERROR_INVALID_ARGUMENT: NULL a; width or height <= 0; NULL
 * current.data or result.data.  Then per plane (current, history if its data
 * is non-NULL, result): BMFR_ERROR_UNSUPPORTED for a format other than F32X3 /
 * F16X4; BMFR_ERROR_INVALID_ARGUMENT for a pitch below width * bytes per
 * pixel or above 2^31, or a data pointer or pitch not a multiple of the element's alignment
 * (4 for F32X3, 8 for F16X4).  Then, unless the call runs without history
 * (reset, or NULL history.data, which needs and looks at neither):
 * BMFR_ERROR_INVALID_ARGUMENT for both or neither of prev_pixel and motion,
 * BMFR_ERROR_UNSUPPORTED for a motion_format other than F32X2 / F16X2,
 * BMFR_ERROR_INVALID_ARGUMENT for a prev_pixel or motion pointer not a
 * multiple of 4.  Then BMFR_ERROR_INVALID_ARGUMENT: result.data equal to
 * current.data or history.data; blend_alpha not finite; the Wd x Hd rectangle
 * not inside dst; NULL ctx. */
typedef struct bmfr_plane { void *data; int format; size_t pitch; } bmfr_plane;  /* F32X3 | F16X4, Wd x Hd, rows `pitch` bytes apart */

typedef struct bmfr_display_taa_args {
    int width, height;            /* Wd, Hd > 0; independent of the context's size */
    bmfr_plane current;           /* this frame's display-resolution colour, e.g. the surface bmfr_upsample_output wrote */
    bmfr_plane history;           /* the previous call's `result`; data NULL: no history (as reset) */
    bmfr_plane result;            /* written; the next call's history; must not be current's or history's memory */
    const float *prev_pixel;      /* F32X2, Wd x Hd, stride Wd: bmfr_frame_inputs.prev_pixel's convention with (W, H) = (Wd, Hd); or NULL and: */
    const void *motion; int motion_format;   /* F32X2 | F16X2 display-resolution motion vectors, with */
    float motion_scale[2]; int motion_at_pixel_centre; float pixel_offset[2];   /* exactly bmfr_gbuffer's fields and rule */
    float blend_alpha;            /* the reference's TAA_BLEND_ALPHA */
    int reset;                    /* 1: the reference's frame 0: result = current */
} bmfr_display_taa_args;

/* Zeroes *a; blend_alpha = cfg's taa_blend_alpha (cfg = NULL: bmfr_config_default's);
 * motion_scale = (1, 1). */
void bmfr_display_taa_default(bmfr_display_taa_args *a, const bmfr_config *cfg);
bmfr_status bmfr_display_taa(bmfr_ctx *ctx, void *stream, const bmfr_display_taa_args *a,
    const bmfr_surface *dst /* nullable */);

/* ---- Firefly pre-filter: an outlier clamp ahead of the block fit ----
 * (no reference counterpart: the reference's dataset is clean.  A renderer's
 * 1-spp buffers are not: one firefly is a huge residual in a 32x32 block's
 * least-squares fit and bends the whole block's fitted colour, the temporal
 * accumulation keeps it for about 1 / blend_alpha frames, and a NaN or inf
 * sample poisons the block and then its history -- only the feature columns
 * of the design matrix are NaN-guarded, bmfr.cl:448-473, not the colour.)
 *
 * bmfr_suppress_fireflies filters the `noisy` plane into `out`: a pixel may be
 * at most `threshold` times as bright as its brightest neighbour.  One kernel
 * launch on `stream`, between bmfr_prepare_frame (or the renderer) and
 * bmfr_process_frame, which then takes `out` as bmfr_frame_inputs.noisy.
 *
 * Planes.  noisy and out cover the context's region (bmfr_sizes.region_*),
 * row stride region_width, in the context's input format: float3, or half3
 * with input_half -- the plane bmfr_process_frame reads as
 * bmfr_frame_inputs.noisy and bmfr_prepare_frame writes as
 * bmfr_prepared.noisy.  Device memory aligned to the element (planes aligned
 * to 16 bytes take the kernel's wide accesses).
 *
 * Arithmetic: every line is one f32 operation rounded once, associated as
 * written, never contracted; division correctly rounded; half values widen
 * exactly; a half result is the f32 result rounded to nearest even.
 *
 *  Y(q) = (0.2126f * r + 0.7152f * g) + 0.0722f * b      the luminance of pixel q
 *  For a pixel p:
 *  1. If any channel of p is NaN or +-inf, p is invalid: with
 *     replace_nonfinite, out = (+0, +0, +0) and stats[1] counts it; otherwise
 *     p's bytes are copied.  Either way p is done.
 *  2. m = the maximum of Y(q) over the pixels q != p with |dx|, |dy| <= radius
 *     that lie inside the region and have a finite Y(q).  No such q: p's bytes
 *     are copied.
 *  3. limit = threshold * m;   if (!(limit > floor)) limit = floor
 *  4. If Y(p) > limit:  s = limit / Y(p);  out_c = c * s per channel c, and
 *     stats[0] counts it.  Otherwise p's bytes are copied unchanged, the sign
 *     of a zero and denormals included.
 *
 * Limits of the rule, on purpose.  Two adjacent fireflies protect each other
 * (each is the other's brightest neighbour).  With floor = 0 a lone lit pixel
 * among exactly black neighbours is scaled to 0 (m = 0): content with truly
 * black regions -- an unlit background, a mask -- wants a floor near the
 * smallest luminance it considers signal.  threshold 2 at radius 1 is the
 * default: on the test scenes it touches 0.4 % of the pixels and cuts the
 * damage x50 fireflies do to the output about fourfold; threshold 1 clamps
 * every ninth pixel and is worse than no filter (tests/test_firefly_cpu.py).
 *
 * stats (nullable): two uint32_t in device memory, {clamped, replaced}.  The
 * call adds to them; the caller zeroes them.
 *
 * Launch and state.  The call reads no state and changes none: not the state
 * planes, not the frame status, not what bmfr_frame_status waits for.  It is
 * legal before any frame has been processed.
 *
 * Tiled contexts.  The window is clipped to the region.  A pixel whose window
 * lies inside the region, or is cut only by the image border, equals the
 * untiled filter's pixel; only the outermost `radius` rings along a region
 * edge inside the image differ.  K1 reads the current frame's colour over the
 * blocks that cover the tile grown by one pixel (frame_params_cfg,
 * bmfr_capi.hip: 32-pixel blocks, bmfr_kernels.h), so at most 32 pixels past
 * the tile, mirrored into the image at its border; tile_halo >= 34 leaves the
 * rings that differ, 33 and 34 pixels out at radius 2, just beyond that.  A
 * tiled pipeline fed filtered region planes therefore still equals the
 * untiled one bit for bit.
 *
 * Errors.  BMFR_ERROR_INVALID_ARGUMENT, before anything is enqueued and with
 * nothing written: NULL ctx, noisy, out or p; out == noisy (a stencil cannot
 * run in place; any other overlap is undefined); a plane not aligned to its
 * element (4 bytes, 2 with input_half) or stats not aligned to 4; threshold
 * not finite or not > 0; radius outside {1, 2}; floor negative or not finite. */
typedef struct bmfr_firefly_params {
    float threshold;          /* k > 0, finite: a pixel may be at most k x its brightest neighbour. Default 2 */
    int   radius;             /* 1 or 2: the (2r+1)^2 window without its centre. Default 1 */
    float floor;              /* >= 0, finite: the limit is never below this luminance. Default 0 */
    int   replace_nonfinite;  /* 1 (default): a pixel with a NaN / +-inf channel becomes (0,0,0); 0: it passes through */
} bmfr_firefly_params;
void bmfr_firefly_default(bmfr_firefly_params *p);
bmfr_status bmfr_suppress_fireflies(bmfr_ctx *ctx, void *stream, const void *noisy, void *out,
                                    const bmfr_firefly_params *p, uint32_t *stats /* device, nullable */);

/* ---- Profiling: the CL_QUEUE_PROFILING_ENABLE + GPUTimer analogue ----
 * (bmfr.cpp:191, 386-412, 488-517).  When enabled, bmfr_process_frame records
 * HIP events around its two kernels; bmfr_get_profile synchronises on them and
 * returns per-frame device durations in ms, oldest first (at most `capacity`
 * frames are kept; enabling again clears the record). */
typedef struct bmfr_frame_profile {
    int frame_number;
    float fused_block_ms; /* K1: accumulate_noisy .. accumulate_filtered, fused */
    float taa_ms;         /* K2: taa */
    float total_ms;       /* start of K1 -> end of K2 (bmfr.cpp:497-502) */
} bmfr_frame_profile;
bmfr_status bmfr_set_profiling(bmfr_ctx *ctx, int enable, int capacity);
/* Record only frames whose frame_number is a multiple of `stride` (default
 * 1): per-kernel timings sampled inside a long timed run at a small cost. */
bmfr_status bmfr_set_profiling_stride(bmfr_ctx *ctx, int stride);
bmfr_status bmfr_get_profile(bmfr_ctx *ctx, bmfr_frame_profile *out, int max_frames, int *count);

/* ---- Synthetic scene (stands in for the external EXR dataset) ---- */

/* Camera of frame `frame`: column-major view-projection matrix and the
 * pixel offset (jitter) in [0,1)^2, i.e. camera_matrices[frame] and
 * pixel_offsets[frame] of the dataset's camera_matrices.h (bmfr.cpp:44-53). */
void bmfr_synth_camera(int image_width, int image_height, int frame, float vp[16],
    float pixel_offset[2]);

/* Render frame `frame` of the synthetic sequence into float3 planes.  `clean`
 * (nullable) receives the noise-free tone-mapped reference image used for
 * PSNR.  _host runs on the CPU (host pointers), _device on the GPU. */
bmfr_status bmfr_synth_frame_host(int image_width, int image_height, int frame, uint32_t seed,
    float *noisy, float *normals, float *positions, float *albedo, float *clean);
bmfr_status bmfr_synth_frame_device(int image_width, int image_height, int frame, uint32_t seed,
    float *noisy, float *normals, float *positions, float *albedo, float *clean, void *stream);
/* The region [x0, x0+w) x [y0, y0+h) of the same frame into planes of row
 * stride w (a tiled context's inputs). */
bmfr_status bmfr_synth_region_device(int image_width, int image_height, int x0, int y0, int w, int h,
    int frame, uint32_t seed, float *noisy, float *normals, float *positions, float *albedo, float *clean,
    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BMFR_H */
