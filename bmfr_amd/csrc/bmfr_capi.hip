// bmfr_capi.hip -- implementation of include/bmfr.h.
//
// Replaces the reference's host plumbing around the hot path: CLEnv context /
// queue / program creation (bmfr.cpp:183-243), buffer creation
// (bmfr.cpp:315-347), kernel argument binding (bmfr.cpp:349-383, 429-476) and
// the Double_buffer swap (bmfr.cpp:122-135, 482-484).  No allocation happens
// on the per-frame path; every call returns a status code.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../include/bmfr.h"
#include "../../include/bmfr_debug.h"
#include "bmfr_firefly.h"
#include "bmfr_launch.h"
#include "bmfr_prepare.h"
#include "bmfr_resolve.h"
#include "bmfr_upsample.h"
#include "bmfr_display_taa.h"

using bmfr::Params;

struct bmfr_ctx {
    bmfr_config cfg;
    bmfr_sizes sizes;
    Params P;
    int device;
    // Temporal state, double-buffered (index `cur` is this frame's).
    float* noisy_acc[2] = {nullptr, nullptr};
    uint8_t* spp[2] = {nullptr, nullptr};
    float* acc[2] = {nullptr, nullptr};
    float* result[2] = {nullptr, nullptr};
    float* tone[2] = {nullptr, nullptr};  // generic feature lists only (the canonical path tone-maps in K2)
    float2* prev_pixel[2] = {nullptr, nullptr};  // double-buffered: K2 of frame f reads it while K1 of f+1 writes
    // bmfr_process_sequence: side stream for K2 and a ring of ordering events
    hipStream_t side = nullptr;
    static constexpr int kSeqEvents = 4;
    hipEvent_t seq_k1[kSeqEvents] = {}, seq_k2[kSeqEvents] = {}, seq_start = nullptr;
    float* noise_table = nullptr;  // kNoiseFrames consecutive frames' tables from noise_first
    int noise_first = -1;
    unsigned long long* stamps = nullptr;  // diagnostic: BMFR_STAMPS=1 with libbmfr_diag.so
    int cur = 0;
    bool has_frame = false;
    // bmfr_process_frame_interior issued for this frame, border part pending
    int pending_frame = -1;
    int pending_prof_slot = -1;  // profiling slot part 0 took for that frame (-1: none)
    // Tiled contexts: reprojection reach past the valid state.  K1 raises
    // reach_dev (device word); K2 moves it into reach_host[0] (page-locked,
    // max over frames since frame 0) and stamps reach_host[1] = frame + 1.
    unsigned* reach_dev = nullptr;
    volatile unsigned* reach_host = nullptr;
    // Every context: page-locked words the kernels set when a bounded wait
    // gave up ([kSyncPivot], [kSyncTile]: frame + 1), and an event after the
    // last enqueued frame (bmfr_frame_status / bmfr_halo_status wait on it).
    // The event is recorded only when a wait needs it (wait_frames), on the
    // stream of the last enqueued frame: a marker between two frames' kernels
    // costs ~6 us of GPU time per frame (profiles/r06_gap_1080p.txt).
    volatile unsigned* sync_host = nullptr;
    hipEvent_t frame_event = nullptr;
    hipStream_t last_stream = nullptr;
    bool frame_enqueued = false;
    bool event_pending = false;  // frames enqueued since frame_event was last recorded
    // One-launch frames (untiled canonical half-tmp_data path): per K1 block
    // the epoch of the last launch that completed it; epoch counts launches.
    unsigned* done = nullptr;
    unsigned epoch = 0;
    // Profiling ring: 3 events per frame (before K1, after K1, after K2).
    int prof_capacity = 0;
    int prof_stride = 1;  // record frames whose number is a multiple of this
    long prof_count = 0;
    hipEvent_t* prof_events = nullptr;
    int* prof_frames = nullptr;
};

namespace {

thread_local int g_last_hip_error = 0;

// Makes the context's device current for the duration of an entry point
// (a process may hold contexts on several GPUs), restoring the caller's.
struct DeviceGuard {
    int prev = -1, dev;
    explicit DeviceGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess || prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};

bmfr_status hip_status(hipError_t e) {
    if (e == hipSuccess) return BMFR_OK;
    g_last_hip_error = (int)e;
    if (e == hipErrorOutOfMemory) return BMFR_ERROR_OUT_OF_MEMORY;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return BMFR_ERROR_NO_DEVICE;
    return BMFR_ERROR_HIP;
}

// `operator<<` of a double with default stream flags == printf("%g"); the
// kernel then sees convert_float(<that text>) (bmfr.cpp:226-227, bmfr.cl:393).
float as_kernel_literal(double v) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%g", v);
    return (float)std::strtod(buf, nullptr);
}

// Blocks reach 32 px past the tile (K2 needs the tile + 1 px), their
// reprojection taps one more, TAA's bilinear taps one more.
constexpr int kMinTileHalo = 34;

bmfr_status validate(const bmfr_config* c) {
    if (!c) return BMFR_ERROR_INVALID_ARGUMENT;
    // mirror() is only valid less than one image size out of range
    // (bmfr.cl:207-216).  Margin work-items reach pixel -32 and WORKSET+29
    // (gid - 16 + BLOCK_OFFSETS, bmfr.cl:314-315), so both need
    // -size <= p <= 2*size-1; smaller images read out of bounds upstream.
    for (int d = 0; d < 2; ++d) {
        const int n = d ? c->image_height : c->image_width;
        const int E = BMFR_BLOCK_EDGE_LENGTH;
        const int workset = E * ((n + E - 1) / E);
        if (n < E || workset + 30 > 2 * n) return BMFR_ERROR_INVALID_ARGUMENT;
    }
    // Kernels address plane elements at 32-bit byte offsets (ld3/st3 in
    // bmfr_device.h): the widest per-pixel element is 12 bytes.
    if ((unsigned long long)c->image_width * c->image_height * 12ull > 0xffffffffull)
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (c->features_not_scaled < 0 || c->features_scaled < 0 ||
        c->features_not_scaled + c->features_scaled > BMFR_MAX_FEATURES ||
        c->features_not_scaled + c->features_scaled < 1)
        return BMFR_ERROR_INVALID_ARGUMENT;
    for (int i = 0; i < c->features_not_scaled + c->features_scaled; ++i)
        if (c->feature_buffers[i] < 0 || c->feature_buffers[i] >= BMFR_FEATURE_COUNT_)
            return BMFR_ERROR_INVALID_ARGUMENT;
    if (c->tile_x || c->tile_y || c->tile_width || c->tile_height || c->tile_halo) {
        if (c->tile_x < 0 || c->tile_y < 0 || c->tile_width <= 0 || c->tile_height <= 0 ||
            c->tile_x + c->tile_width > c->image_width || c->tile_y + c->tile_height > c->image_height ||
            c->tile_halo < kMinTileHalo)
            return BMFR_ERROR_INVALID_ARGUMENT;
    }
    return BMFR_OK;
}

bool is_tiled(const bmfr_config* c) { return c->tile_width > 0; }
// One completion flag per block of the (untiled) frame's block grid.
size_t done_bytes(const bmfr_ctx* c) { return (size_t)c->P.blocks_x * c->P.blocks_y * sizeof(unsigned); }
// The stage kernels take the reference's whole-frame f32 layouts only.
bool stage_api_ok(const bmfr_config* c) { return !is_tiled(c) && !c->input_half; }
// The stages that evaluate features keep the reference's signatures, which
// have no place for a caller-supplied plane.
bool names_aux(const bmfr_ctx* c) { return bmfr::aux_mask(c->P) != 0; }
// A plane the context's list names must be there (bmfr_aux_inputs, nullable).
bool aux_planes_ok(const bmfr_ctx* c, const bmfr_aux_inputs* aux) {
    const int mask = bmfr::aux_mask(c->P);
    for (int k = 0; k < BMFR_MAX_AUX_FEATURES; ++k)
        if ((mask & (1 << k)) && (!aux || !aux->aux[k])) return false;
    return true;
}

Params make_params(const bmfr_config* c, const bmfr_sizes* s) {
    Params P{};
    P.width = c->image_width;
    P.height = c->image_height;
    P.workset_w = s->workset_width;
    P.workset_h = s->workset_height;
    P.margins_w = s->workset_with_margins_width;
    P.margins_h = s->workset_with_margins_height;
    P.blocks_x = P.margins_w / BMFR_BLOCK_EDGE_LENGTH;
    P.blocks_y = P.margins_h / BMFR_BLOCK_EDGE_LENGTH;
    P.buffers = s->buffer_count;
    P.not_scaled = c->features_not_scaled;
    P.scaled = c->features_scaled;
    for (int i = 0; i < bmfr::kMaxFeatures; ++i) P.codes[i] = c->feature_buffers[i];
    P.noise2 = c->noise_amount * (double)2.f;
    P.blend_alpha = c->blend_alpha;
    P.second_blend_alpha = c->second_blend_alpha;
    P.taa_blend_alpha = c->taa_blend_alpha;
    P.position_limit_sq = as_kernel_literal(c->position_limit_squared);
    P.normal_limit_sq = as_kernel_literal(c->normal_limit_squared);
    P.half_tmp = c->use_half_precision_in_tmp_data ? 1 : 0;
    P.input_half = c->input_half ? 1 : 0;
    P.library_powr = c->library_powr ? 1 : 0;
    P.fast_fit = c->fast_fit ? 1 : 0;
    P.ox = s->region_x;
    P.oy = s->region_y;
    P.stride = s->region_width;
    P.rows = s->region_height;
    // whole-grid launch (stage kernels, untiled frames)
    P.bx0 = P.by0 = 0;
    P.nbx = P.blocks_x;
    P.nby = P.blocks_y;
    P.tx0 = P.ty0 = 0;
    P.tx1 = P.width;
    P.ty1 = P.height;
    // valid previous state: the whole region (checked only for tiles)
    P.check_reach = c->tile_width > 0 ? 1 : 0;
    P.vx0 = P.ox;
    P.vy0 = P.oy;
    P.vx1 = P.ox + P.stride;
    P.vy1 = P.oy + P.rows;
    P.wx0 = P.vx0, P.wy0 = P.vy0, P.wx1 = P.vx1, P.wy1 = P.vy1;
    P.max_polls = bmfr::kDefaultMaxPolls;
    P.debug_delay = 0;
    P.frame_launches = 0;
    return P;
}

// The launch parameters of frame `frame` for a tiled context: the blocks of
// that frame's shifted grid (bmfr.cl:267-285, 310-317) that cover the tile
// plus one pixel (TAA's 3x3), and the tile as K2's output.  Blocks without a
// pixel inside the frame own nothing and are skipped.  The previous state the
// frame reads (bmfr_halo_need): the state planes over the pixels of those
// blocks (mirrored at the frame border) grown by the reprojection reach --
// tile_halo - 34 pixels of motion and one for the bilinear taps -- and the
// TAA output over the tile grown by the same reach; both clipped to the
// region.  [v*] / [w*] are these rectangles (K1 checks the taps against them).
Params frame_params_cfg(const bmfr_config& g, Params P, int frame) {
    const int E = BMFR_BLOCK_EDGE_LENGTH;
    const int ox = bmfr::kBlockOffsetTable[frame & 15][0], oy = bmfr::kBlockOffsetTable[frame & 15][1];
    auto range = [&](int lo, int hi, int off, int nblocks, int& b0, int& nb) {
        // block b covers pixels [E b - E/2 + off, E b + E/2 + off)
        b0 = -1;
        nb = 0;
        for (int b = 0; b < nblocks; ++b) {
            const int p0 = E * b - E / 2 + off, p1 = p0 + E;
            if (p0 < hi && p1 > lo) {
                if (b0 < 0) b0 = b;
                nb = b - b0 + 1;
            }
        }
    };
    range(std::max(0, g.tile_x - 1), std::min(g.image_width, g.tile_x + g.tile_width + 1), ox, P.blocks_x, P.bx0,
          P.nbx);
    range(std::max(0, g.tile_y - 1), std::min(g.image_height, g.tile_y + g.tile_height + 1), oy, P.blocks_y,
          P.by0, P.nby);
    P.tx0 = g.tile_x;
    P.ty0 = g.tile_y;
    P.tx1 = g.tile_x + g.tile_width;
    P.ty1 = g.tile_y + g.tile_height;
    const int reach = g.tile_halo - 33;
    // [lo, hi] of the mirrored pixels of blocks [b0, b0 + nb), grown by reach, clipped to [r0, r1)
    auto need = [&](int b0, int nb, int off, int size, int r0, int r1, int& v0, int& v1) {
        int lo = size, hi = -1;
        for (int p = E * b0 - E / 2 + off; p < E * (b0 + nb) - E / 2 + off; ++p) {
            const int m = p < 0 ? -p - 1 : (p >= size ? 2 * size - p - 1 : p);
            lo = std::min(lo, m);
            hi = std::max(hi, m);
        }
        v0 = std::max(lo - reach, r0);
        v1 = std::min(hi + 1 + reach, r1);
    };
    need(P.bx0, P.nbx, ox, g.image_width, P.ox, P.ox + P.stride, P.vx0, P.vx1);
    need(P.by0, P.nby, oy, g.image_height, P.oy, P.oy + P.rows, P.vy0, P.vy1);
    P.wx0 = std::max(P.tx0 - reach, P.ox), P.wx1 = std::min(P.tx1 + reach, P.ox + P.stride);
    P.wy0 = std::max(P.ty0 - reach, P.oy), P.wy1 = std::min(P.ty1 + reach, P.oy + P.rows);
    return P;
}

Params frame_params(const bmfr_ctx* c, int frame) {
    return is_tiled(&c->cfg) ? frame_params_cfg(c->cfg, c->P, frame) : c->P;
}

hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

bmfr::Camera make_camera(const float m[16], const float off[2]) {
    bmfr::Camera cam;
    for (int i = 0; i < 16; ++i) cam.m[i] = m[i];
    cam.jx = off[0];
    cam.jy = off[1];
    return cam;
}

}  // namespace

extern "C" {

void bmfr_config_default(bmfr_config* c, int w, int h) {
    std::memset(c, 0, sizeof *c);
    c->image_width = w;
    c->image_height = h;
    // NOT_SCALED_FEATURE_BUFFERS / SCALED_FEATURE_BUFFERS, bmfr.cpp:65-77
    const int f[] = {BMFR_FEATURE_ONE,        BMFR_FEATURE_NORMAL_X,   BMFR_FEATURE_NORMAL_Y,
                     BMFR_FEATURE_NORMAL_Z,   BMFR_FEATURE_POSITION_X, BMFR_FEATURE_POSITION_Y,
                     BMFR_FEATURE_POSITION_Z, BMFR_FEATURE_POSITION_X2, BMFR_FEATURE_POSITION_Y2,
                     BMFR_FEATURE_POSITION_Z2};
    c->features_not_scaled = 4;
    c->features_scaled = 6;
    for (int i = 0; i < 10; ++i) c->feature_buffers[i] = f[i];
    c->noise_amount = 1e-2;          // bmfr.cpp:58
    c->blend_alpha = 0.2f;           // bmfr.cpp:60
    c->second_blend_alpha = 0.1f;    // bmfr.cpp:61
    c->taa_blend_alpha = 0.2f;       // bmfr.cpp:62
    c->position_limit_squared = 0.01;
    c->normal_limit_squared = 0.1;
    c->use_half_precision_in_tmp_data = 1;  // bmfr.cpp:88
}

bmfr_status bmfr_config_sizes(const bmfr_config* c, bmfr_sizes* s) {
    const bmfr_status v = validate(c);
    if (v != BMFR_OK) return v;
    if (!s) return BMFR_ERROR_INVALID_ARGUMENT;
    const int E = BMFR_BLOCK_EDGE_LENGTH;
    s->buffer_count = c->features_not_scaled + c->features_scaled + 3;
    s->r_edge = s->buffer_count - 2;
    s->workset_width = E * ((c->image_width + E - 1) / E);
    s->workset_height = E * ((c->image_height + E - 1) / E);
    s->workset_with_margins_width = s->workset_width + E;
    s->workset_with_margins_height = s->workset_height + E;
    s->blocks = (s->workset_with_margins_width / E) * (s->workset_with_margins_height / E);
    const size_t elem = c->use_half_precision_in_tmp_data ? 2 : 4;
    s->tmp_data_bytes = (size_t)s->workset_with_margins_width * s->workset_with_margins_height *
                        s->buffer_count * elem;
    s->weights_bytes = (size_t)s->blocks * (s->buffer_count - 3) * 3 * sizeof(float);
    s->mins_maxs_bytes = (size_t)s->blocks * c->features_scaled * 2 * sizeof(float);
    s->image_bytes = (size_t)c->image_width * c->image_height * 3 * sizeof(float);
    if (is_tiled(c)) {
        s->region_x = std::max(0, c->tile_x - c->tile_halo);
        s->region_y = std::max(0, c->tile_y - c->tile_halo);
        s->region_width = std::min(c->image_width, c->tile_x + c->tile_width + c->tile_halo) - s->region_x;
        s->region_height = std::min(c->image_height, c->tile_y + c->tile_height + c->tile_halo) - s->region_y;
    } else {
        s->region_x = s->region_y = 0;
        s->region_width = c->image_width;
        s->region_height = c->image_height;
    }
    s->region_bytes = (size_t)s->region_width * s->region_height * 3 * sizeof(float);
    s->frame_launches = s->blocks >= bmfr::kTwoLaunchBlocks ? 2 : 1;  // launch_fused_frame's rule
    return BMFR_OK;
}

const char* bmfr_status_string(bmfr_status s) {
    switch (s) {
        case BMFR_OK: return "ok";
        case BMFR_ERROR_INVALID_ARGUMENT: return "invalid argument";
        case BMFR_ERROR_UNSUPPORTED: return "unsupported configuration";
        case BMFR_ERROR_OUT_OF_MEMORY: return "out of device memory";
        case BMFR_ERROR_HIP: return "HIP runtime error";
        case BMFR_ERROR_NO_DEVICE: return "no HIP device";
        case BMFR_ERROR_HALO_EXCEEDED: return "reprojection reached past the tile halo";
        case BMFR_ERROR_SYNC_TIMEOUT: return "a kernel's bounded wait for another work-group gave up";
    }
    return "unknown status";
}

int bmfr_last_hip_error(void) { return g_last_hip_error; }

// The build id (bmfr_amd/_build.py: SHA-256 of the sources, then "+flags" for
// a variant build), behind a marker so the build script can read it from the
// file without loading it.
#if __has_include("bmfr_build_id.h")
#include "bmfr_build_id.h"
#else
#define BMFR_BUILD_ID "unknown"
#endif
static const char kBuildId[] = "bmfr-build-id:" BMFR_BUILD_ID;
const char* bmfr_build_id(void) { return kBuildId + sizeof("bmfr-build-id:") - 1; }

bmfr_status bmfr_create(const bmfr_config* cfg, int device, bmfr_ctx** out) {
    if (!out) return BMFR_ERROR_INVALID_ARGUMENT;
    *out = nullptr;
    bmfr_sizes sz;
    bmfr_status st = bmfr_config_sizes(cfg, &sz);
    if (st != BMFR_OK) return st;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return BMFR_ERROR_NO_DEVICE;
    if (device < 0 || device >= n) return BMFR_ERROR_NO_DEVICE;
    st = hip_status(hipSetDevice(device));
    if (st != BMFR_OK) return st;

    bmfr_ctx* c = new bmfr_ctx;
    c->cfg = *cfg;
    c->sizes = sz;
    c->P = make_params(cfg, &sz);
    c->device = device;
    const size_t px = (size_t)sz.region_width * sz.region_height;  // every plane covers the region
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = hipMalloc(&c->noisy_acc[i], px * 3 * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(&c->spp[i], px);
        if (e == hipSuccess) e = hipMalloc(&c->acc[i], px * 3 * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(&c->result[i], px * 3 * sizeof(float));
    }
    if (!bmfr::fused_supported(c->P))  // the generic path's K1 writes a tone-mapped frame for its TAA
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc(&c->tone[i], px * 3 * sizeof(float));
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc(&c->prev_pixel[i], px * sizeof(float2));
    if (e == hipSuccess && std::getenv("BMFR_STAMPS"))
        e = hipMalloc(&c->stamps, (size_t)sz.blocks * 8 * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMalloc(&c->noise_table,
                      (size_t)bmfr::kNoiseFrames * bmfr::kMaxFeatures * bmfr::kBlockPixels * sizeof(float));
    if (e == hipSuccess) {
        void* h = nullptr;
        e = hipHostMalloc(&h, 2 * sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) {
            c->sync_host = static_cast<volatile unsigned*>(h);
            c->sync_host[0] = c->sync_host[1] = 0;
            e = hipEventCreateWithFlags(&c->frame_event, hipEventDisableTiming);
        }
    }
    if (e == hipSuccess && is_tiled(cfg)) {
        void* h = nullptr;
        e = hipMalloc(&c->reach_dev, sizeof(unsigned));
        if (e == hipSuccess) e = hipMemset(c->reach_dev, 0, sizeof(unsigned));
        if (e == hipSuccess) e = hipHostMalloc(&h, 2 * sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) {
            c->reach_host = static_cast<volatile unsigned*>(h);
            c->reach_host[0] = c->reach_host[1] = 0;
        }
    }
    if (e == hipSuccess && bmfr::frame_fused_supported(c->P)) {
        e = hipMalloc(&c->done, done_bytes(c));
        if (e == hipSuccess) e = hipMemset(c->done, 0, done_bytes(c));
    }
    if (e != hipSuccess) {
        bmfr_destroy(c);
        return hip_status(e);
    }
    *out = c;
    return BMFR_OK;
}

bmfr_status bmfr_destroy(bmfr_ctx* c) {
    if (!c) return BMFR_ERROR_INVALID_ARGUMENT;
    DeviceGuard guard(c->device);
    if (c->frame_enqueued) (void)hipDeviceSynchronize();  // no kernel still uses the buffers or host words
    (void)hipFree(c->reach_dev);
    (void)hipFree(c->done);
    if (c->reach_host) (void)hipHostFree(const_cast<unsigned*>(c->reach_host));
    if (c->sync_host) (void)hipHostFree(const_cast<unsigned*>(c->sync_host));
    if (c->frame_event) (void)hipEventDestroy(c->frame_event);
    for (int i = 0; i < 2; ++i) {
        (void)hipFree(c->noisy_acc[i]);
        (void)hipFree(c->spp[i]);
        (void)hipFree(c->acc[i]);
        (void)hipFree(c->result[i]);
    }
    if (c->prof_events)
        for (int i = 0; i < 3 * c->prof_capacity; ++i) (void)hipEventDestroy(c->prof_events[i]);
    delete[] c->prof_events;
    delete[] c->prof_frames;
    for (int i = 0; i < 2; ++i) (void)hipFree(c->tone[i]);
    for (int i = 0; i < 2; ++i) (void)hipFree(c->prev_pixel[i]);
    if (c->side) {
        (void)hipStreamDestroy(c->side);
        for (int i = 0; i < bmfr_ctx::kSeqEvents; ++i) {
            (void)hipEventDestroy(c->seq_k1[i]);
            (void)hipEventDestroy(c->seq_k2[i]);
        }
        (void)hipEventDestroy(c->seq_start);
    }
    (void)hipFree(c->noise_table);
    (void)hipFree(c->stamps);
    delete c;
    return BMFR_OK;
}

bmfr_status bmfr_get_sizes(const bmfr_ctx* c, bmfr_sizes* out) {
    if (!c || !out) return BMFR_ERROR_INVALID_ARGUMENT;
    *out = c->sizes;
    return BMFR_OK;
}

// ----------------------------------------------------------- stage API ----
bmfr_status bmfr_accumulate_noisy_data(bmfr_ctx* c, void* stream, float* out_prev_frame_pixel,
                                       uint8_t* accept_bools, const float* current_normals,
                                       const float* previous_normals, const float* current_positions,
                                       const float* previous_positions, float* current_noisy,
                                       const float* previous_noisy, const uint8_t* previous_spp,
                                       uint8_t* current_spp, void* tmp_data,
                                       const float prev_frame_camera_matrix[16],
                                       const float pixel_offset[2], int frame_number) {
    if (!c || !out_prev_frame_pixel || !accept_bools || !current_normals || !current_positions ||
        !current_noisy || !current_spp || !tmp_data || !prev_frame_camera_matrix || !pixel_offset ||
        frame_number < 0)
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (!stage_api_ok(&c->cfg) || names_aux(c)) return BMFR_ERROR_UNSUPPORTED;
    if (frame_number > 0 && (!previous_normals || !previous_positions || !previous_noisy || !previous_spp))
        return BMFR_ERROR_INVALID_ARGUMENT;
    bmfr::NoisyInputs in{current_normals, previous_normals, current_positions, previous_positions,
                         current_noisy, previous_noisy, previous_spp};
    DeviceGuard guard(c->device);
    return hip_status(bmfr::launch_accumulate_noisy(
        c->P, as_stream(stream), reinterpret_cast<float2*>(out_prev_frame_pixel), accept_bools, in,
        current_noisy, current_spp, tmp_data, make_camera(prev_frame_camera_matrix, pixel_offset),
        frame_number));
}

bmfr_status bmfr_fitter(bmfr_ctx* c, void* stream, float* weights, float* mins_maxs, void* tmp_data,
                        int frame_number) {
    if (!c || !weights || (!mins_maxs && c->P.scaled > 0) || !tmp_data || frame_number < 0)
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (!stage_api_ok(&c->cfg)) return BMFR_ERROR_UNSUPPORTED;
    if (!bmfr::fitter_supported(c->P.not_scaled, c->P.scaled)) return BMFR_ERROR_UNSUPPORTED;
    DeviceGuard guard(c->device);
    return hip_status(bmfr::launch_fitter(c->P, as_stream(stream), weights, mins_maxs, tmp_data, frame_number));
}

bmfr_status bmfr_weighted_sum(bmfr_ctx* c, void* stream, const float* weights, const float* mins_maxs,
                              float* output, const float* current_normals,
                              const float* current_positions, const float* current_noisy,
                              int frame_number) {
    (void)current_noisy;  // debugging-only argument upstream (bmfr.cl:709)
    if (!c || !weights || (!mins_maxs && c->P.scaled > 0) || !output || !current_normals || !current_positions ||
        frame_number < 0)
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (!stage_api_ok(&c->cfg) || names_aux(c)) return BMFR_ERROR_UNSUPPORTED;
    DeviceGuard guard(c->device);
    return hip_status(bmfr::launch_weighted_sum(c->P, as_stream(stream), weights, mins_maxs, output,
                                                current_normals, current_positions, frame_number));
}

bmfr_status bmfr_accumulate_filtered_data(bmfr_ctx* c, void* stream, const float* filtered_frame,
                                          const float* in_prev_frame_pixel, const uint8_t* accept_bools,
                                          const float* albedo, float* tone_mapped_frame,
                                          const uint8_t* current_spp, const float* accumulated_prev_frame,
                                          float* accumulated_frame, int frame_number) {
    if (!c || !filtered_frame || !in_prev_frame_pixel || !accept_bools || !albedo || !tone_mapped_frame ||
        !current_spp || !accumulated_frame || frame_number < 0)
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (!stage_api_ok(&c->cfg)) return BMFR_ERROR_UNSUPPORTED;
    if (frame_number > 0 && !accumulated_prev_frame) return BMFR_ERROR_INVALID_ARGUMENT;
    DeviceGuard guard(c->device);
    return hip_status(bmfr::launch_accumulate_filtered(
        c->P, as_stream(stream), filtered_frame, reinterpret_cast<const float2*>(in_prev_frame_pixel),
        accept_bools, albedo, tone_mapped_frame, current_spp, accumulated_prev_frame, accumulated_frame,
        frame_number));
}

bmfr_status bmfr_taa(bmfr_ctx* c, void* stream, const float* in_prev_frame_pixel, const float* new_frame,
                     float* result_frame, const float* prev_frame, int frame_number) {
    if (!c || !in_prev_frame_pixel || !new_frame || !result_frame || frame_number < 0)
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (!stage_api_ok(&c->cfg)) return BMFR_ERROR_UNSUPPORTED;
    if (frame_number > 0 && !prev_frame) return BMFR_ERROR_INVALID_ARGUMENT;
    DeviceGuard guard(c->device);
    return hip_status(bmfr::launch_taa(c->P, as_stream(stream),
                                       reinterpret_cast<const float2*>(in_prev_frame_pixel), new_frame,
                                       result_frame, prev_frame, frame_number));
}

// ----------------------------------------------------------- frame API ----
namespace {

bmfr_status check_frame_args(const bmfr_ctx* c, const bmfr_frame_inputs* in, const bmfr_aux_inputs* aux,
                             const float* m, const float* off, int frame_number) {
    if (!c || !in || !in->noisy || !in->normals || !in->positions || !in->albedo || !m || !off || frame_number < 0)
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (frame_number > 0 && (!in->prev_normals || !in->prev_positions || !c->has_frame))
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (!aux_planes_ok(c, aux)) return BMFR_ERROR_INVALID_ARGUMENT;
    if (!bmfr::fitter_supported(c->P.not_scaled, c->P.scaled)) return BMFR_ERROR_UNSUPPORTED;
    if ((is_tiled(&c->cfg) || c->cfg.input_half) && !bmfr::fused_supported(c->P)) return BMFR_ERROR_UNSUPPORTED;
    return BMFR_OK;
}

// The kernels' arguments for frame `frame_number`, writing state slot `cur`.
bmfr::FusedArgs frame_args(const bmfr_ctx* c, const bmfr_frame_inputs* in, const float* m, const float* off,
                           int frame_number, int cur, const bmfr_aux_inputs* aux = nullptr) {
    const int prv = 1 - cur;
    bmfr::FusedArgs A;
    // Input planes are float3 or (input_half) half3; the kernels read them
    // through ld3in<IN> by element type.
    auto plane = [](const void* p) { return static_cast<const float*>(p); };
    A.in = bmfr::NoisyInputs{plane(in->normals), plane(in->prev_normals), plane(in->positions),
                             plane(in->prev_positions), plane(in->noisy), c->noisy_acc[prv], c->spp[prv]};
    A.cam = make_camera(m, off);
    A.frame = frame_number;
    A.albedo = plane(in->albedo);
    A.acc_prev = c->acc[prv];
    A.result_prev = c->result[prv];
    A.noisy_out = c->noisy_acc[cur];
    A.spp_out = c->spp[cur];
    A.prev_pixel_out = c->prev_pixel[cur];
    A.acc_out = c->acc[cur];
    A.tone_out = c->tone[cur];
    A.result_out = c->result[cur];
    A.noise_table = c->noise_table;
    A.reach = c->reach_dev;
    A.reach_host = const_cast<unsigned*>(c->reach_host);
    A.stamps = c->stamps;
    A.done = nullptr;  // set per launch (one_launch_args)
    A.epoch = 0;
    A.sync_err = const_cast<unsigned*>(c->sync_host);
    // The caller's previous-frame pixel plane replaces the projection from
    // frame 1 on (frame 0 has no previous frame: ignored, like prev_normals).
    A.prev_pixel_in = frame_number > 0 ? reinterpret_cast<const float2*>(in->prev_pixel) : nullptr;
    // The planes the list names; the others are ignored.
    const int mask = bmfr::aux_mask(c->P);
    for (int k = 0; k < BMFR_MAX_AUX_FEATURES; ++k) A.aux.p[k] = (aux && (mask & (1 << k))) ? aux->aux[k] : nullptr;
    return A;
}

// The sticky reports of completed frames, as the host sees them now (no wait).
bmfr_status reported(const bmfr_ctx* c) {
    if (c->sync_host[bmfr::kSyncPivot] || c->sync_host[bmfr::kSyncTile]) return BMFR_ERROR_SYNC_TIMEOUT;
    if (c->reach_host && c->reach_host[0] > 0) return BMFR_ERROR_HALO_EXCEEDED;
    return BMFR_OK;
}

// Waits until every frame enqueued so far has completed: frame_event, recorded
// now on the last frame's stream if frames were enqueued since its last record
// (falls back to a device-wide wait if that stream no longer takes a record).
bmfr_status wait_frames(bmfr_ctx* c) {
    if (!c->frame_enqueued) return BMFR_OK;
    if (c->event_pending) {
        if (hipEventRecord(c->frame_event, c->last_stream) != hipSuccess) {
            (void)hipGetLastError();
            const bmfr_status st = hip_status(hipDeviceSynchronize());
            if (st == BMFR_OK) c->event_pending = false, c->frame_enqueued = false;
            return st;
        }
        c->event_pending = false;
    }
    return hip_status(hipEventSynchronize(c->frame_event));
}

// Before a frame is enqueued: BMFR_ERROR_SYNC_TIMEOUT once a completed frame
// reported an exhausted wait, and (tiled contexts) BMFR_ERROR_HALO_EXCEEDED
// once one reported reprojection taps past the exchanged state -- both sticky
// until frame 0 starts a new sequence.  Frame 0 first waits for every frame
// already enqueued (a frame still in flight could raise a report after it was
// cleared), then clears them.
bmfr_status status_check(bmfr_ctx* c, int frame_number) {
    if (frame_number == 0) {
        const bmfr_status st = wait_frames(c);
        if (st != BMFR_OK) return st;
        c->sync_host[0] = c->sync_host[1] = 0;
        if (c->reach_host) c->reach_host[0] = 0;
        return BMFR_OK;
    }
    return reported(c);
}

// After a frame's last kernel: remember its stream for wait_frames (no marker
// on the stream: the next frame's kernel follows this one directly).
void frame_enqueued(bmfr_ctx* c, hipStream_t s) {
    c->last_stream = s;
    c->event_pending = true;
    c->frame_enqueued = true;
}

// Blocks of frame `frame`'s K1 launch (frame_params) whose reads of the
// previous frame's state stay inside the tile: every pixel of the block
// (mirrored at the frame border, bmfr.cl:310-317) plus the reprojection
// reach -- tile_halo - 34 pixels of motion (include/bmfr.h) and one more for
// the bilinear taps -- clipped to the frame lies in the tile.  Those blocks
// need no halo; they form a rectangle [*i0, *i1) of block indices per axis
// (empty when i0 == i1).  Untiled contexts: every block.
void interior_blocks(const bmfr_ctx* c, const Params& P, int frame, int* ix0, int* ix1, int* iy0, int* iy1) {
    const bmfr_config& g = c->cfg;
    if (!is_tiled(&g)) {
        *ix0 = P.bx0, *ix1 = P.bx0 + P.nbx, *iy0 = P.by0, *iy1 = P.by0 + P.nby;
        return;
    }
    const int E = BMFR_BLOCK_EDGE_LENGTH, reach = g.tile_halo - 33;
    auto axis = [&](int b0, int nb, int off, int size, int t0, int t1, int* i0, int* i1) {
        *i0 = *i1 = b0;
        int first = -1, last = -1;
        for (int b = b0; b < b0 + nb; ++b) {
            int lo = size, hi = -1;
            for (int p = E * b - E / 2 + off; p < E * b + E / 2 + off; ++p) {
                const int m = p < 0 ? -p - 1 : (p >= size ? 2 * size - p - 1 : p);
                lo = std::min(lo, m);
                hi = std::max(hi, m);
            }
            const bool in = std::max(lo - reach, 0) >= t0 && std::min(hi + reach, size - 1) < t1;
            if (in) {
                if (first < 0) first = b;
                if (last >= 0 && last != b - 1) return;  // not one run: treat all as border
                last = b;
            }
        }
        if (first >= 0) *i0 = first, *i1 = last + 1;
    };
    const int ox = bmfr::kBlockOffsetTable[frame & 15][0], oy = bmfr::kBlockOffsetTable[frame & 15][1];
    axis(P.bx0, P.nbx, ox, g.image_width, g.tile_x, g.tile_x + g.tile_width, ix0, ix1);
    axis(P.by0, P.nby, oy, g.image_height, g.tile_y, g.tile_y + g.tile_height, iy0, iy1);
    if (*ix0 == *ix1 || *iy0 == *iy1) *ix0 = *ix1 = P.bx0, *iy0 = *iy1 = P.by0;
}

Params block_rect(Params P, int x0, int x1, int y0, int y1) {
    P.bx0 = x0;
    P.nbx = x1 - x0;
    P.by0 = y0;
    P.nby = y1 - y0;
    return P;
}

// Frame f's noise table (k_noise_table), made kNoiseFrames frames at a time on
// stream s when f is outside the cached range.  Frames are ordered on their
// streams by their state dependencies, so a batch is never rewritten under a
// K1 that still reads it.
hipError_t noise_for_frame(bmfr_ctx* c, const Params& P, hipStream_t s, int f, float** out) {
    const size_t per = (size_t)(P.buffers - 4) * bmfr::kBlockPixels;
    if (c->noise_first < 0 || f < c->noise_first || f >= c->noise_first + bmfr::kNoiseFrames) {
        const hipError_t e = bmfr::launch_noise_tables(P, s, f, bmfr::kNoiseFrames, c->noise_table);
        if (e != hipSuccess) return e;
        c->noise_first = f;
    }
    *out = c->noise_table + (size_t)(f - c->noise_first) * per;
    return hipSuccess;
}

// One-launch frames: the next epoch of the completion flags (never 0 and
// below 2^31, the flag's top bit carries a timeout; flags reset on wrap).
bmfr_status next_epoch(bmfr_ctx* c, hipStream_t s, bmfr::FusedArgs* A) {
    if (++c->epoch == bmfr::kDoneTimeout) {
        const bmfr_status st = hip_status(hipMemsetAsync(c->done, 0, done_bytes(c), s));
        if (st != BMFR_OK) return st;
        c->epoch = 1;
    }
    A->done = c->done;
    A->epoch = c->epoch;
    return BMFR_OK;
}

// PART 0: noise table + interior blocks.  PART 1: border blocks + K2 (+ swap).
// PART 2: everything (bmfr_process_frame).
bmfr_status process_part(bmfr_ctx* c, void* stream, const bmfr_frame_inputs* in, const bmfr_aux_inputs* aux,
                         const float* m, const float* off, int frame_number, int part) {
    bmfr_status st = check_frame_args(c, in, aux, m, off, frame_number);
    if (st != BMFR_OK) return st;
    if (part == 1 && c->pending_frame != frame_number) return BMFR_ERROR_INVALID_ARGUMENT;
    if (part != 1 && c->pending_frame >= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    DeviceGuard guard(c->device);
    if (part != 1 && (st = status_check(c, frame_number)) != BMFR_OK) return st;
    const hipStream_t s = as_stream(stream);
    const int cur = c->has_frame ? 1 - c->cur : 0;  // swap, bmfr.cpp:482-484
    bmfr::FusedArgs A = frame_args(c, in, m, off, frame_number, cur, aux);
    const Params P = frame_params(c, frame_number);
    const bool generic = !bmfr::fused_supported(P);  // untiled (check_frame_args): every block is interior
    // Profiling: 3 events of one slot per recorded frame; part 0 takes the
    // slot, part 1 finishes it.
    hipEvent_t* ev = nullptr;
    if (part == 1) {
        if (c->pending_prof_slot >= 0 && c->prof_capacity > 0)
            ev = c->prof_events + 3 * (c->pending_prof_slot % c->prof_capacity);
    } else if (c->prof_capacity > 0 && frame_number % c->prof_stride == 0) {
        const int slot = (int)(c->prof_count % c->prof_capacity);
        ev = c->prof_events + 3 * slot;
        c->prof_frames[slot] = frame_number;
        ++c->prof_count;
        (void)hipEventRecord(ev[0], s);
    }
    if (part == 2) {
        if (bmfr::fused_supported(P) && (st = hip_status(noise_for_frame(c, P, s, frame_number, &A.noise_table))))
            return st;
        if (c->done && !ev && (st = next_epoch(c, s, &A)) != BMFR_OK) return st;  // one launch
        st = hip_status(bmfr::launch_fused_frame(P, s, A, ev ? ev[1] : nullptr));
        if (st != BMFR_OK) return st;
    } else if (generic) {
        // The generic-feature path's two launches: K1 is the interior part, its TAA the border part.
        if (part == 0) {
            if ((st = hip_status(bmfr::launch_fused_generic(P, s, A))) != BMFR_OK) return st;
            c->pending_frame = frame_number;
            c->pending_prof_slot = ev ? (int)((c->prof_count - 1) % c->prof_capacity) : -1;
            return BMFR_OK;
        }
        if (ev) (void)hipEventRecord(ev[1], s);
        st = hip_status(bmfr::launch_taa(P, s, A.prev_pixel_out, A.tone_out, A.result_out, A.result_prev, A.frame));
        if (st != BMFR_OK) return st;
        c->pending_frame = -1;
        c->pending_prof_slot = -1;
    } else {
        int ix0, ix1, iy0, iy1;
        interior_blocks(c, P, frame_number, &ix0, &ix1, &iy0, &iy1);
        // part 0 makes the table if needed, part 1 finds it in the cached range
        if ((st = hip_status(noise_for_frame(c, P, s, frame_number, &A.noise_table))) != BMFR_OK) return st;
        if (part == 0) {
            // Before the exchange only the tile's own state is valid.
            Params I = block_rect(P, ix0, ix1, iy0, iy1);
            const bmfr_config& g = c->cfg;
            I.vx0 = g.tile_x, I.vy0 = g.tile_y, I.vx1 = g.tile_x + g.tile_width, I.vy1 = g.tile_y + g.tile_height;
            I.wx0 = I.vx0, I.wy0 = I.vy0, I.wx1 = I.vx1, I.wy1 = I.vy1;
            st = hip_status(bmfr::launch_fused_k1_blocks(I, s, A));
            if (st != BMFR_OK) return st;
            c->pending_frame = frame_number;
            c->pending_prof_slot = ev ? (int)((c->prof_count - 1) % c->prof_capacity) : -1;
            return BMFR_OK;
        }
        // The border ring in one launch (an empty interior leaves the whole rectangle).
        Params R = P;
        if (ix1 > ix0 && iy1 > iy0) {
            R.ring = P.nbx * P.nby - (ix1 - ix0) * (iy1 - iy0);
            if (R.ring == 0) R.ring = -1;  // nothing outside the interior
            R.rx0 = ix0, R.rx1 = ix1, R.ry0 = iy0, R.ry1 = iy1;
        }
        if (c->done && !ev && bmfr::frame_fused_supported(R)) {
            // the ring's K1 blocks and the tile's TAA in one launch (completion flags)
            if ((st = next_epoch(c, s, &A)) != BMFR_OK) return st;
            if ((st = hip_status(bmfr::launch_fused_frame_one(R, s, A))) != BMFR_OK) return st;
        } else {
            if ((st = hip_status(bmfr::launch_fused_k1_blocks(R, s, A))) != BMFR_OK) return st;
            if (ev) (void)hipEventRecord(ev[1], s);
            if ((st = hip_status(bmfr::launch_fused_k2(P, s, A))) != BMFR_OK) return st;
        }
        c->pending_frame = -1;
        c->pending_prof_slot = -1;
    }
    if (ev) (void)hipEventRecord(ev[2], s);
    frame_enqueued(c, s);
    c->cur = cur;
    c->has_frame = true;
    return BMFR_OK;
}

}  // namespace

bmfr_status bmfr_process_frame(bmfr_ctx* c, void* stream, const bmfr_frame_inputs* in,
                               const float prev_frame_camera_matrix[16], const float pixel_offset[2],
                               int frame_number) {
    return process_part(c, stream, in, nullptr, prev_frame_camera_matrix, pixel_offset, frame_number, 2);
}

bmfr_status bmfr_process_frame_aux(bmfr_ctx* c, void* stream, const bmfr_frame_inputs* in, const bmfr_aux_inputs* aux,
                       const float prev_frame_camera_matrix[16], const float pixel_offset[2], int frame_number) {
    return process_part(c, stream, in, aux, prev_frame_camera_matrix, pixel_offset, frame_number, 2);
}

bmfr_status bmfr_process_sequence(bmfr_ctx* c, void* stream, int count, const bmfr_frame_inputs* in,
                                  const float* prev_frame_camera_matrices, const float* pixel_offsets,
                                  int first_frame, float* const* outputs) {
    return bmfr_process_sequence_aux(c, stream, count, in, nullptr, prev_frame_camera_matrices, pixel_offsets,
                                     first_frame, outputs);
}

bmfr_status bmfr_process_sequence_aux(bmfr_ctx* c, void* stream, int count, const bmfr_frame_inputs* in,
                                      const bmfr_aux_inputs* aux, const float* prev_frame_camera_matrices,
                                      const float* pixel_offsets, int first_frame, float* const* outputs) {
    if (!c || count <= 0 || !in || !prev_frame_camera_matrices || !pixel_offsets || first_frame < 0)
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (c->pending_frame >= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    if (is_tiled(&c->cfg)) return BMFR_ERROR_UNSUPPORTED;  // tiles exchange a halo between frames
    DeviceGuard guard(c->device);
    bmfr_status st = status_check(c, first_frame);
    if (st != BMFR_OK) return st;
    const hipStream_t s = as_stream(stream);
    const size_t out_bytes = c->sizes.region_bytes;
    const bool pipelined = bmfr::fused_supported(c->P);
    if (!pipelined) {  // frame after frame on `stream`
        for (int i = 0; i < count; ++i)  // a missing plane fails the call before any frame is enqueued
            if (!aux_planes_ok(c, aux ? &aux[i] : nullptr)) return BMFR_ERROR_INVALID_ARGUMENT;
        for (int i = 0; i < count; ++i) {
            st = bmfr_process_frame_aux(c, stream, &in[i], aux ? &aux[i] : nullptr,
                                        prev_frame_camera_matrices + 16 * i, pixel_offsets + 2 * i, first_frame + i);
            if (st != BMFR_OK) return st;
            if (outputs && outputs[i])
                if ((st = hip_status(hipMemcpyAsync(outputs[i], c->result[c->cur], out_bytes, hipMemcpyDefault, s))))
                    return st;
        }
        return BMFR_OK;
    }
    if (first_frame > 0 && !c->has_frame) return BMFR_ERROR_INVALID_ARGUMENT;
    for (int i = 0; i < count; ++i) {
        const bmfr_frame_inputs& x = in[i];
        if (!x.noisy || !x.normals || !x.positions || !x.albedo) return BMFR_ERROR_INVALID_ARGUMENT;
        if (first_frame + i > 0 && (!x.prev_normals || !x.prev_positions)) return BMFR_ERROR_INVALID_ARGUMENT;
    }
    hipError_t e = hipSuccess;
    const char* mode = std::getenv("BMFR_SEQUENCE");  // "streams": the two-stream schedule below
    if (bmfr::seq_fused_supported(c->P) && !(mode && std::strcmp(mode, "streams") == 0)) {
        // One launch per frame on `stream`: K1 of frame f with K2 of frame
        // f - 1 in its tail (k_fused_cols_taa), then K2 of the last frame.
        // K1 of f overwrites the state slot of f - 2, whose last reader (K2
        // of f - 2) ran in the previous launch.
        bmfr::FusedArgs prevA{};
        Params prevP{};
        bool pending = false;
        for (int i = 0; i <= count; ++i) {
            const int f = first_frame + i;
            bmfr::FusedArgs A{};
            Params P{};
            int cur = c->cur;
            if (i < count) {
                cur = c->has_frame ? 1 - c->cur : 0;
                A = frame_args(c, &in[i], prev_frame_camera_matrices + 16 * i, pixel_offsets + 2 * i, f, cur);
                P = frame_params(c, f);
                if ((e = noise_for_frame(c, P, s, f, &A.noise_table)) != hipSuccess) return hip_status(e);
            }
            hipEvent_t* ev = nullptr;
            if (i < count && c->prof_capacity > 0 && f % c->prof_stride == 0) {
                const int slot = (int)(c->prof_count % c->prof_capacity);
                ev = c->prof_events + 3 * slot;
                c->prof_frames[slot] = f;
                ++c->prof_count;
            }
            if (ev) (void)hipEventRecord(ev[0], s);
            if (i < count && A.prev_pixel_in) {
                // A frame that carries a prev_pixel plane: K2 of frame f - 1
                // alone, then the plane-reading K1 alone (the same kernels'
                // arithmetic, so the results are the one-launch form's).
                e = pending ? bmfr::launch_fused_k1_taa(P, s, nullptr, prevP, &prevA) : hipSuccess;
                if (e == hipSuccess) e = bmfr::launch_fused_k1_blocks(P, s, A);
            } else {
                e = bmfr::launch_fused_k1_taa(P, s, i < count ? &A : nullptr, prevP, pending ? &prevA : nullptr);
            }
            if (ev) {  // K1 of f and K2 of f - 1 share the launch: all of it is reported as K1
                (void)hipEventRecord(ev[1], s);
                (void)hipEventRecord(ev[2], s);
            }
            if (e == hipSuccess && pending && outputs && outputs[i - 1])
                e = hipMemcpyAsync(outputs[i - 1], prevA.result_out, out_bytes, hipMemcpyDefault, s);
            if (e != hipSuccess) return hip_status(e);
            if (i < count) {
                prevA = A;
                prevP = P;
                pending = true;
                c->cur = cur;
                c->has_frame = true;
            }
        }
        frame_enqueued(c, s);
        return BMFR_OK;
    }
    if (!c->side) {
        e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
        for (int i = 0; i < bmfr_ctx::kSeqEvents && e == hipSuccess; ++i) {
            e = hipEventCreateWithFlags(&c->seq_k1[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->seq_k2[i], hipEventDisableTiming);
        }
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->seq_start, hipEventDisableTiming);
        if (e != hipSuccess) return hip_status(e);
    }
    // K1 of frame f on `stream`, K2 of frame f on the side stream, so that K2
    // of frame f runs beside K1 of frame f+1.  K1 of f waits for K2 of f-2,
    // the last reader of the state slot (accumulated filtered colour,
    // prev-frame pixel) it overwrites; the call joins `stream` at the end.
    const hipStream_t t = c->side;
    (void)hipEventRecord(c->seq_start, s);
    (void)hipStreamWaitEvent(t, c->seq_start, 0);
    for (int i = 0; i < count; ++i) {
        const int f = first_frame + i;
        const int cur = c->has_frame ? 1 - c->cur : 0;
        bmfr::FusedArgs A = frame_args(c, &in[i], prev_frame_camera_matrices + 16 * i, pixel_offsets + 2 * i,
                                       f, cur);
        const Params P = frame_params(c, f);
        hipEvent_t* ev = nullptr;
        if (c->prof_capacity > 0 && f % c->prof_stride == 0) {
            const int slot = (int)(c->prof_count % c->prof_capacity);
            ev = c->prof_events + 3 * slot;
            c->prof_frames[slot] = f;
            ++c->prof_count;
        }
        const int k = i % bmfr_ctx::kSeqEvents;
        if (i >= 2) e = hipStreamWaitEvent(s, c->seq_k2[(i - 2) % bmfr_ctx::kSeqEvents], 0);
        if (ev && e == hipSuccess) e = hipEventRecord(ev[0], s);
        if (e == hipSuccess) e = noise_for_frame(c, P, s, f, &A.noise_table);
        if (e == hipSuccess) e = bmfr::launch_fused_k1_blocks(P, s, A);
        if (ev && e == hipSuccess) e = hipEventRecord(ev[1], s);
        if (e == hipSuccess) e = hipEventRecord(c->seq_k1[k], s);
        if (e == hipSuccess) e = hipStreamWaitEvent(t, c->seq_k1[k], 0);
        if (e == hipSuccess) e = bmfr::launch_fused_k2(P, t, A);
        if (e == hipSuccess && outputs && outputs[i])
            e = hipMemcpyAsync(outputs[i], A.result_out, out_bytes, hipMemcpyDefault, t);
        if (ev && e == hipSuccess) e = hipEventRecord(ev[2], t);
        if (e == hipSuccess) e = hipEventRecord(c->seq_k2[k], t);
        if (e != hipSuccess) return hip_status(e);
        c->cur = cur;
        c->has_frame = true;
    }
    if ((st = hip_status(hipStreamWaitEvent(s, c->seq_k2[(count - 1) % bmfr_ctx::kSeqEvents], 0))) != BMFR_OK)
        return st;
    frame_enqueued(c, s);
    return BMFR_OK;
}

bmfr_status bmfr_process_frame_interior(bmfr_ctx* c, void* stream, const bmfr_frame_inputs* in,
                                        const float prev_frame_camera_matrix[16], const float pixel_offset[2],
                                        int frame_number) {
    return process_part(c, stream, in, nullptr, prev_frame_camera_matrix, pixel_offset, frame_number, 0);
}

bmfr_status bmfr_process_frame_interior_aux(bmfr_ctx* c, void* stream, const bmfr_frame_inputs* in, const bmfr_aux_inputs* aux,
                       const float prev_frame_camera_matrix[16], const float pixel_offset[2], int frame_number) {
    return process_part(c, stream, in, aux, prev_frame_camera_matrix, pixel_offset, frame_number, 0);
}

bmfr_status bmfr_process_frame_border(bmfr_ctx* c, void* stream, const bmfr_frame_inputs* in,
                                      const float prev_frame_camera_matrix[16], const float pixel_offset[2],
                                      int frame_number) {
    return process_part(c, stream, in, nullptr, prev_frame_camera_matrix, pixel_offset, frame_number, 1);
}

bmfr_status bmfr_process_frame_border_aux(bmfr_ctx* c, void* stream, const bmfr_frame_inputs* in, const bmfr_aux_inputs* aux,
                       const float prev_frame_camera_matrix[16], const float pixel_offset[2], int frame_number) {
    return process_part(c, stream, in, aux, prev_frame_camera_matrix, pixel_offset, frame_number, 1);
}

// ------------------------------------------------- G-buffer front end ----
void bmfr_gbuffer_default(bmfr_gbuffer* g) {
    if (!g) return;
    std::memset(g, 0, sizeof *g);
    g->albedo_floor = 1.0f / 255.0f;
    g->motion_scale[0] = g->motion_scale[1] = 1.0f;
}

namespace {

// A non-null plane's format must be one of `listed`.
bool format_listed(const void* plane, int format, std::initializer_list<int> listed) {
    return !plane || std::find(listed.begin(), listed.end(), format) != listed.end();
}

// g and out alone (no context, no device): a requested output whose inputs
// are missing is an invalid argument, an unlisted format unsupported.
bmfr_status check_prepare_args(const bmfr_gbuffer* g, const bmfr_prepared* out, const float* off) {
    if (!g || !out || !off) return BMFR_ERROR_INVALID_ARGUMENT;
    if (g->n_objects < 0 || g->n_objects > 65535 || (g->n_objects > 0 && !g->object_transforms))
        return BMFR_ERROR_INVALID_ARGUMENT;
    const bool moved = out->prev_positions_moved || out->prev_normals_moved;
    if ((out->noisy && (!g->radiance || !g->albedo)) || (out->albedo && !g->albedo) ||
        (out->normals && !g->normals) || (out->positions && !g->positions && !g->depth) ||
        (out->prev_pixel && !g->motion) || (out->prev_positions_moved && !g->prev_positions) ||
        (out->prev_normals_moved && !g->prev_normals) || (moved && g->n_objects > 0 && !g->prev_object_id))
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (!format_listed(g->radiance, g->radiance_format, {BMFR_FORMAT_F32X3, BMFR_FORMAT_F16X4}) ||
        !format_listed(g->albedo, g->albedo_format, {BMFR_FORMAT_F32X3, BMFR_FORMAT_F16X4, BMFR_FORMAT_UNORM8X4}) ||
        !format_listed(g->normals, g->normal_format,
                       {BMFR_FORMAT_F32X3, BMFR_FORMAT_F16X4, BMFR_FORMAT_OCT_SNORM16X2}) ||
        !format_listed(g->motion, g->motion_format, {BMFR_FORMAT_F32X2, BMFR_FORMAT_F16X2}))
        return BMFR_ERROR_UNSUPPORTED;
    return BMFR_OK;
}

}  // namespace

bmfr_status bmfr_prepare_frame(bmfr_ctx* c, void* stream, const bmfr_gbuffer* g, const bmfr_prepared* out,
                               const float pixel_offset[2]) {
    const bmfr_status st = check_prepare_args(g, out, pixel_offset);
    if (st != BMFR_OK) return st;
    if (!c) return BMFR_ERROR_INVALID_ARGUMENT;
    bmfr::PrepareArgs a{};
    a.radiance = g->radiance;
    a.albedo = g->albedo;
    a.normals = g->normals;
    a.positions = g->positions;
    a.depth = g->depth;
    a.motion = g->motion;
    a.prev_positions = g->prev_positions;
    a.prev_normals = g->prev_normals;
    a.prev_id = g->prev_object_id;
    a.transforms = g->object_transforms;
    a.o_noisy = out->noisy;
    a.o_normals = out->normals;
    a.o_positions = out->positions;
    a.o_albedo = out->albedo;
    a.o_prev_pixel = out->prev_pixel;
    a.o_prev_positions = out->prev_positions_moved;
    a.o_prev_normals = out->prev_normals_moved;
    std::memcpy(a.m, g->inv_view_proj, sizeof a.m);
    a.albedo_floor = g->albedo_floor;
    a.mscale_x = g->motion_scale[0];
    a.mscale_y = g->motion_scale[1];
    a.jx = pixel_offset[0];
    a.jy1 = 1.0f - pixel_offset[1];
    a.radiance_fmt = g->radiance_format;
    a.albedo_fmt = g->albedo_format;
    a.normal_fmt = g->normal_format;
    a.motion_fmt = g->motion_format;
    a.motion_centre = g->motion_at_pixel_centre != 0;
    a.n_objects = g->n_objects;
    a.rx = c->sizes.region_x;
    a.ry = c->sizes.region_y;
    a.rw = c->sizes.region_width;
    a.W = c->cfg.image_width;
    a.H = c->cfg.image_height;
    a.n = (uint32_t)c->sizes.region_width * (uint32_t)c->sizes.region_height;
    DeviceGuard guard(c->device);
    return hip_status(bmfr::launch_prepare(a, c->cfg.input_half != 0, static_cast<hipStream_t>(stream)));
}

void bmfr_surface_default(bmfr_surface* s) {
    if (!s) return;
    std::memset(s, 0, sizeof *s);
    s->alpha = 1.0f;
}

namespace {

// Bytes per pixel and alignment of a surface or display-plane format; false: not one.
bool format_layout(int format, size_t* bpp, size_t* align) {
    switch (format) {
    case BMFR_FORMAT_F32X3: *bpp = 12, *align = 4; return true;
    case BMFR_FORMAT_F16X4: *bpp = 8, *align = 8; return true;
    case BMFR_FORMAT_UNORM8X4:
    case BMFR_FORMAT_UNORM10X3A2: *bpp = 4, *align = 4; return true;
    case BMFR_FORMAT_UNORM8X3: *bpp = 3, *align = 1; return true;
    default: return false;
    }
}

// Rows of `width` pixels of `format`, `pitch` bytes apart from `data`: pitch and alignment.
bmfr_status check_rows(const void* data, size_t pitch, int format, int width) {
    size_t bpp, align;
    if (!format_layout(format, &bpp, &align)) return BMFR_ERROR_UNSUPPORTED;
    if (pitch < (size_t)width * bpp || pitch % align != 0 || reinterpret_cast<uintptr_t>(data) % align != 0 ||
        pitch > (size_t)1 << 31)  // row * pitch stays inside 64 bits
        return BMFR_ERROR_INVALID_ARGUMENT;
    return BMFR_OK;
}

// dst alone (no context, no device).
bmfr_status check_surface(const bmfr_surface* d) {
    if (!d || !d->data || d->width <= 0 || d->height <= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    return check_rows(d->data, d->pitch, d->format, d->width);
}

// A w x h rectangle of a stage at (ox, oy) of d's frame of reference, whose
// rows count from the top, or with flip_y from the bottom of a frame of
// frame_height rows: false if it leaves the surface (64-bit: origins are the
// caller's), else its placement -- row 0 is its last surface row when flipped.
bool place_in_surface(const bmfr_surface* d, int ox, int oy, int w, int h, int frame_height, bmfr::SurfaceDst* s) {
    const long long x0 = (long long)d->origin_x + ox;
    const long long y0 = (long long)d->origin_y + (d->flip_y ? frame_height - oy - h : oy);
    if (x0 < 0 || y0 < 0 || x0 + w > d->width || y0 + h > d->height) return false;
    s->dst = d->data;
    s->pitch = (long long)d->pitch;
    s->alpha = d->alpha;
    s->format = d->format;
    s->bgr = d->bgr != 0;
    s->dx0 = (int)x0;
    s->dy0 = (int)(d->flip_y ? y0 + h - 1 : y0);
    s->dy_step = d->flip_y ? -1 : 1;
    return true;
}

// dst, source and albedo alone (no context, no device).
bmfr_status check_resolve_args(int source, const void* albedo, const bmfr_surface* d) {
    const bmfr_status st = check_surface(d);
    if (st != BMFR_OK) return st;
    if (source != BMFR_RESOLVE_OUTPUT && source != BMFR_RESOLVE_HDR) return BMFR_ERROR_INVALID_ARGUMENT;
    if (source == BMFR_RESOLVE_HDR && !albedo) return BMFR_ERROR_INVALID_ARGUMENT;
    return BMFR_OK;
}

}  // namespace

bmfr_status bmfr_resolve_output(bmfr_ctx* c, void* stream, int source, const void* albedo, const bmfr_surface* d) {
    const bmfr_status st = check_resolve_args(source, albedo, d);
    if (st != BMFR_OK) return st;
    if (!c || !c->has_frame || c->pending_frame >= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    const bmfr_config& g = c->cfg;
    const bmfr_sizes& z = c->sizes;
    const bool tiled = is_tiled(&g);
    const int tx = tiled ? g.tile_x : 0, ty = tiled ? g.tile_y : 0;
    const int tw = tiled ? g.tile_width : g.image_width, th = tiled ? g.tile_height : g.image_height;
    bmfr::ResolveArgs a{};
    if (!place_in_surface(d, tx, ty, tw, th, g.image_height, &a.surf)) return BMFR_ERROR_INVALID_ARGUMENT;
    a.src = source == BMFR_RESOLVE_HDR ? c->acc[c->cur] : c->result[c->cur];
    a.albedo = source == BMFR_RESOLVE_HDR ? albedo : nullptr;
    a.albedo_half = g.input_half != 0;
    a.rw = z.region_width;
    a.sx0 = tx - z.region_x;
    a.sy0 = ty - z.region_y;
    a.tw = tw;
    a.th = th;
    DeviceGuard guard(c->device);
    return hip_status(bmfr::launch_resolve(a, as_stream(stream)));
}

// ------------------------------------------------- guided upsampling ----
void bmfr_upsample_guides_default(bmfr_upsample_guides* g, const bmfr_config* cfg) {
    if (!g) return;
    std::memset(g, 0, sizeof *g);
    bmfr_config d;
    if (!cfg) bmfr_config_default(&d, BMFR_BLOCK_EDGE_LENGTH, BMFR_BLOCK_EDGE_LENGTH);
    g->plane_limit_squared = as_kernel_literal((cfg ? cfg : &d)->position_limit_squared);
    g->normal_limit_squared = as_kernel_literal((cfg ? cfg : &d)->normal_limit_squared);
}

namespace {

bool aligned_to(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// source, the guides, the frame planes and stats alone (no context, no device).
bmfr_status check_upsample_args(int source, const void* frame_normals, const void* frame_positions,
                                const bmfr_upsample_guides* g, const uint32_t* stats) {
    if (source != BMFR_UPSAMPLE_HDR && source != BMFR_UPSAMPLE_TONEMAPPED) return BMFR_ERROR_INVALID_ARGUMENT;
    if (!g || !g->albedo || g->width <= 0 || g->height <= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    const bool has_position = g->positions || g->depth;
    if ((g->normals != nullptr) != has_position) return BMFR_ERROR_INVALID_ARGUMENT;
    if (g->normals && (!frame_normals || !frame_positions)) return BMFR_ERROR_INVALID_ARGUMENT;
    for (float limit : {g->plane_limit_squared, g->normal_limit_squared})
        if (!std::isfinite(limit) || !(limit > 0.0f)) return BMFR_ERROR_INVALID_ARGUMENT;
    if (!format_listed(g->albedo, g->albedo_format, {BMFR_FORMAT_F32X3, BMFR_FORMAT_F16X4, BMFR_FORMAT_UNORM8X4}) ||
        !format_listed(g->normals, g->normal_format,
                       {BMFR_FORMAT_F32X3, BMFR_FORMAT_F16X4, BMFR_FORMAT_OCT_SNORM16X2}))
        return BMFR_ERROR_UNSUPPORTED;
    if (!aligned_to(g->albedo, g->albedo_format == BMFR_FORMAT_F16X4 ? 8 : 4) ||
        !aligned_to(g->normals, g->normal_format == BMFR_FORMAT_F16X4 ? 8 : 4) || !aligned_to(g->positions, 4) ||
        !aligned_to(g->depth, 4) || !aligned_to(stats, sizeof(uint32_t)))
        return BMFR_ERROR_INVALID_ARGUMENT;
    return BMFR_OK;
}

}  // namespace

bmfr_status bmfr_upsample_output(bmfr_ctx* c, void* stream, int source, const void* frame_normals,
                                 const void* frame_positions, const bmfr_upsample_guides* g, const bmfr_surface* d,
                                 uint32_t* stats) {
    bmfr_status st = check_surface(d);
    if (st == BMFR_OK) st = check_upsample_args(source, frame_normals, frame_positions, g, stats);
    if (st != BMFR_OK) return st;
    if (!c || !c->has_frame || c->pending_frame >= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    const bmfr_config& cfg = c->cfg;
    // a tile's taps reach one pixel past it, where filtered_accumulated holds the previous exchange
    if (is_tiled(&cfg)) return BMFR_ERROR_UNSUPPORTED;
    const int W = cfg.image_width, H = cfg.image_height, Wd = g->width, Hd = g->height;
    if (Wd < W || Hd < H || Wd > 4ll * W || Hd > 4ll * H) return BMFR_ERROR_INVALID_ARGUMENT;
    const bool guided = g->normals != nullptr;
    const uintptr_t elem = cfg.input_half ? 2 : 4;
    if (guided && (!aligned_to(frame_normals, elem) || !aligned_to(frame_positions, elem)))
        return BMFR_ERROR_INVALID_ARGUMENT;
    bmfr::UpsampleArgs a{};
    if (!place_in_surface(d, 0, 0, Wd, Hd, Hd, &a.surf)) return BMFR_ERROR_INVALID_ARGUMENT;
    a.acc = c->acc[c->cur];
    a.f_normals = guided ? frame_normals : nullptr;
    a.f_positions = guided ? frame_positions : nullptr;
    a.albedo = g->albedo;
    a.normals = g->normals;
    a.positions = g->positions;
    a.depth = g->depth;
    a.stats = guided ? stats : nullptr;
    std::memcpy(a.m, g->inv_view_proj, sizeof a.m);
    a.jx = g->pixel_offset[0];
    a.jy1 = 1.0f - g->pixel_offset[1];
    a.rx = (float)W / (float)Wd;
    a.ry = (float)H / (float)Hd;
    a.plane_limit_sq = g->plane_limit_squared;
    a.normal_limit_sq = g->normal_limit_squared;
    a.albedo_fmt = g->albedo_format;
    a.normal_fmt = g->normal_format;
    a.frame_half = cfg.input_half != 0;
    a.tonemapped = source == BMFR_UPSAMPLE_TONEMAPPED;
    a.W = W;
    a.H = H;
    a.Wd = Wd;
    a.Hd = Hd;
    DeviceGuard guard(c->device);
    return hip_status(bmfr::launch_upsample(a, as_stream(stream)));
}

// ------------------------------------- display-resolution TAA ----
void bmfr_display_taa_default(bmfr_display_taa_args* a, const bmfr_config* cfg) {
    if (!a) return;
    std::memset(a, 0, sizeof *a);
    bmfr_config d;
    if (!cfg) bmfr_config_default(&d, BMFR_BLOCK_EDGE_LENGTH, BMFR_BLOCK_EDGE_LENGTH);
    a->blend_alpha = (cfg ? cfg : &d)->taa_blend_alpha;
    a->motion_scale[0] = a->motion_scale[1] = 1.0f;
}

namespace {

// A display-resolution plane's format, pitch and alignment (data non-NULL).
bmfr_status check_plane(const bmfr_plane& p, int width) {
    if (p.format != BMFR_FORMAT_F32X3 && p.format != BMFR_FORMAT_F16X4) return BMFR_ERROR_UNSUPPORTED;
    return check_rows(p.data, p.pitch, p.format, width);
}

// The arguments and dst alone (no context, no device).
bmfr_status check_display_taa_args(const bmfr_display_taa_args* a, const bmfr_surface* d) {
    if (d) {
        const bmfr_status st = check_surface(d);
        if (st != BMFR_OK) return st;
    }
    if (!a || a->width <= 0 || a->height <= 0 || !a->current.data || !a->result.data)
        return BMFR_ERROR_INVALID_ARGUMENT;
    const bool with_history = !a->reset && a->history.data;
    for (const bmfr_plane* p : {&a->current, &a->history, &a->result}) {
        if (!p->data) continue;  // history: a NULL plane's format and pitch are not looked at
        const bmfr_status st = check_plane(*p, a->width);
        if (st != BMFR_OK) return st;
    }
    if (with_history) {
        if ((a->prev_pixel != nullptr) == (a->motion != nullptr)) return BMFR_ERROR_INVALID_ARGUMENT;
        if (!format_listed(a->motion, a->motion_format, {BMFR_FORMAT_F32X2, BMFR_FORMAT_F16X2}))
            return BMFR_ERROR_UNSUPPORTED;
        if (!aligned_to(a->prev_pixel, 4) || !aligned_to(a->motion, 4)) return BMFR_ERROR_INVALID_ARGUMENT;
    }
    if (a->result.data == a->current.data || a->result.data == a->history.data) return BMFR_ERROR_INVALID_ARGUMENT;
    if (!std::isfinite(a->blend_alpha)) return BMFR_ERROR_INVALID_ARGUMENT;
    return BMFR_OK;
}

}  // namespace

bmfr_status bmfr_display_taa(bmfr_ctx* c, void* stream, const bmfr_display_taa_args* args, const bmfr_surface* d) {
    const bmfr_status st = check_display_taa_args(args, d);
    if (st != BMFR_OK) return st;
    if (!c) return BMFR_ERROR_INVALID_ARGUMENT;
    const bool with_history = !args->reset && args->history.data;
    bmfr::DisplayTaaArgs a{};
    a.current = args->current.data;
    a.history = with_history ? args->history.data : nullptr;
    a.result = args->result.data;
    a.prev_pixel = with_history ? args->prev_pixel : nullptr;
    a.motion = with_history ? args->motion : nullptr;
    a.current_pitch = (long long)args->current.pitch;
    a.history_pitch = with_history ? (long long)args->history.pitch : 0;
    a.result_pitch = (long long)args->result.pitch;
    a.mscale[0] = args->motion_scale[0];
    a.mscale[1] = args->motion_scale[1];
    a.jx = args->pixel_offset[0];
    a.jy1 = 1.0f - args->pixel_offset[1];
    a.blend_a = args->blend_alpha;
    a.blend_b = 1.0f - args->blend_alpha;
    a.current_fmt = args->current.format;
    a.history_fmt = args->history.format;
    a.result_fmt = args->result.format;
    a.motion_fmt = args->motion_format;
    a.motion_centre = args->motion_at_pixel_centre != 0;
    a.Wd = args->width;
    a.Hd = args->height;
    // d null: a.surf.dst stays null, no surface
    if (d && !place_in_surface(d, 0, 0, a.Wd, a.Hd, a.Hd, &a.surf)) return BMFR_ERROR_INVALID_ARGUMENT;
    DeviceGuard guard(c->device);
    return hip_status(bmfr::launch_display_taa(a, as_stream(stream)));
}

// ------------------------------------------------- firefly pre-filter ----
void bmfr_firefly_default(bmfr_firefly_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->threshold = 2.0f;
    p->radius = 1;
    p->replace_nonfinite = 1;
}

namespace {

// The filter over a width x height plane on the current device.
bmfr_status suppress_fireflies(void* stream, const void* noisy, void* out, int width, int height, bool half,
                               const bmfr_firefly_params* p, uint32_t* stats) {
    if (!noisy || !out || !p || out == noisy) return BMFR_ERROR_INVALID_ARGUMENT;
    const uintptr_t elem = half ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(noisy) % elem != 0 || reinterpret_cast<uintptr_t>(out) % elem != 0 ||
        reinterpret_cast<uintptr_t>(stats) % sizeof(uint32_t) != 0)
        return BMFR_ERROR_INVALID_ARGUMENT;
    if (!std::isfinite(p->threshold) || !(p->threshold > 0.0f) || (p->radius != 1 && p->radius != 2) ||
        !std::isfinite(p->floor) || p->floor < 0.0f)
        return BMFR_ERROR_INVALID_ARGUMENT;
    bmfr::FireflyArgs a{};
    a.noisy = noisy;
    a.out = out;
    a.stats = stats;
    a.threshold = p->threshold;
    a.floor = p->floor;
    a.replace_nonfinite = p->replace_nonfinite != 0;
    a.rw = width;
    a.rh = height;
    return hip_status(bmfr::launch_firefly(a, half, p->radius, as_stream(stream)));
}

}  // namespace

bmfr_status bmfr_suppress_fireflies(bmfr_ctx* c, void* stream, const void* noisy, void* out,
                                    const bmfr_firefly_params* p, uint32_t* stats) {
    if (!c) return BMFR_ERROR_INVALID_ARGUMENT;
    DeviceGuard guard(c->device);
    return suppress_fireflies(stream, noisy, out, c->sizes.region_width, c->sizes.region_height,
                              c->cfg.input_half != 0, p, stats);
}

bmfr_status bmfr_debug_suppress_fireflies(void* stream, const void* noisy, void* out, int width, int height,
                                          int half, const bmfr_firefly_params* p, uint32_t* stats) {
    // planes are addressed at 32-bit byte offsets, as a context's (validate)
    if (width <= 0 || height <= 0 || (unsigned long long)width * height * 12ull > 0xffffffffull)
        return BMFR_ERROR_INVALID_ARGUMENT;
    return suppress_fireflies(stream, noisy, out, width, height, half != 0, p, stats);
}

bmfr_status bmfr_halo_copy(bmfr_ctx* c, void* stream, const int* rects, int n, void* buffer, int unpack,
                           size_t* bytes) {
    if (!c || n < 0 || (n > 0 && !rects)) return BMFR_ERROR_INVALID_ARGUMENT;
    if (!is_tiled(&c->cfg)) return BMFR_ERROR_UNSUPPORTED;
    DeviceGuard guard(c->device);
    const int i = c->cur;  // bmfr_state(previous = 0): the last frame's state
    struct {
        uint8_t* base;
        int bpp;
    } planes[4] = {{reinterpret_cast<uint8_t*>(c->noisy_acc[i]), 12}, {c->spp[i], 1},
                   {reinterpret_cast<uint8_t*>(c->acc[i]), 12}, {reinterpret_cast<uint8_t*>(c->result[i]), 12}};
    const bmfr_sizes& s = c->sizes;
    bmfr::HaloArgs a{};
    long long off = 0;
    for (int r = 0; r < n; ++r) {
        const int* q = rects + 5 * r;
        const int x = q[0], y = q[1], w = q[2], h = q[3], mask = q[4];
        if (w <= 0 || h <= 0 || x < s.region_x || y < s.region_y || x + w > s.region_x + s.region_width ||
            y + h > s.region_y + s.region_height || mask <= 0 || mask > BMFR_HALO_ALL)
            return BMFR_ERROR_INVALID_ARGUMENT;
        for (int k = 0; k < 4; ++k) {
            if (!(mask & (1 << k))) continue;
            if (a.nseg == bmfr::kMaxHaloSegs) return BMFR_ERROR_INVALID_ARGUMENT;
            const auto& p = planes[k];
            bmfr::HaloSeg& g = a.seg[a.nseg++];
            const size_t first = ((size_t)(y - s.region_y) * s.region_width + (x - s.region_x)) * p.bpp;
            g.plane = reinterpret_cast<unsigned long long>(p.base + first);
            g.buf_off = off;
            g.row_bytes = w * p.bpp;
            g.rows = h;
            g.pitch = s.region_width * p.bpp;
            off += ((long long)g.row_bytes * h + 15) & ~15LL;
        }
    }
    if (bytes) *bytes = (size_t)off;
    if (!buffer) return BMFR_OK;
    return hip_status(bmfr::launch_halo_copy(a, as_stream(stream), buffer, unpack));
}

bmfr_status bmfr_halo_need(const bmfr_config* cfg, int frame_number, int state_rect[4], int result_rect[4]) {
    if (!cfg || frame_number < 0 || !state_rect || !result_rect) return BMFR_ERROR_INVALID_ARGUMENT;
    bmfr_sizes sz;
    const bmfr_status st = bmfr_config_sizes(cfg, &sz);
    if (st != BMFR_OK) return st;
    if (!is_tiled(cfg)) return BMFR_ERROR_UNSUPPORTED;
    const Params P = frame_params_cfg(*cfg, make_params(cfg, &sz), frame_number);
    const int v[4] = {P.vx0, P.vy0, P.vx1 - P.vx0, P.vy1 - P.vy0}, w[4] = {P.wx0, P.wy0, P.wx1 - P.wx0, P.wy1 - P.wy0};
    for (int k = 0; k < 4; ++k) state_rect[k] = v[k], result_rect[k] = w[k];
    return BMFR_OK;
}

bmfr_status bmfr_set_profiling_stride(bmfr_ctx* c, int stride) {
    if (!c || stride <= 0 || c->pending_frame >= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    c->prof_stride = stride;
    return BMFR_OK;
}

bmfr_status bmfr_set_profiling(bmfr_ctx* c, int enable, int capacity) {
    if (!c || (enable && capacity <= 0) || c->pending_frame >= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    DeviceGuard guard(c->device);
    if (c->prof_events) {
        (void)hipDeviceSynchronize();
        for (int i = 0; i < 3 * c->prof_capacity; ++i) (void)hipEventDestroy(c->prof_events[i]);
        delete[] c->prof_events;
        delete[] c->prof_frames;
        c->prof_events = nullptr;
        c->prof_frames = nullptr;
    }
    c->prof_capacity = 0;
    c->prof_count = 0;
    if (!enable) return BMFR_OK;
    c->prof_events = new hipEvent_t[3 * capacity]();
    c->prof_frames = new int[capacity]();
    for (int i = 0; i < 3 * capacity; ++i) {
        const bmfr_status st = hip_status(hipEventCreate(&c->prof_events[i]));
        if (st != BMFR_OK) return st;
    }
    c->prof_capacity = capacity;
    return BMFR_OK;
}

bmfr_status bmfr_get_profile(bmfr_ctx* c, bmfr_frame_profile* out, int max_frames, int* count) {
    if (!c || !count || (max_frames > 0 && !out)) return BMFR_ERROR_INVALID_ARGUMENT;
    DeviceGuard guard(c->device);
    const long have = c->prof_count < c->prof_capacity ? c->prof_count : c->prof_capacity;
    const long first = c->prof_count - have;
    int n = 0;
    for (long k = first; k < c->prof_count && n < max_frames; ++k, ++n) {
        const int slot = (int)(k % c->prof_capacity);
        hipEvent_t* ev = c->prof_events + 3 * slot;
        bmfr_status st = hip_status(hipEventSynchronize(ev[2]));
        if (st != BMFR_OK) return st;
        float a = 0, b = 0, t = 0;
        if ((st = hip_status(hipEventElapsedTime(&a, ev[0], ev[1]))) != BMFR_OK) return st;
        if ((st = hip_status(hipEventElapsedTime(&b, ev[1], ev[2]))) != BMFR_OK) return st;
        if ((st = hip_status(hipEventElapsedTime(&t, ev[0], ev[2]))) != BMFR_OK) return st;
        out[n].frame_number = c->prof_frames[slot];
        out[n].fused_block_ms = a;
        out[n].taa_ms = b;
        out[n].total_ms = t;
    }
    *count = n;
    return BMFR_OK;
}

bmfr_status bmfr_halo_status(bmfr_ctx* c, unsigned* overshoot) {
    if (!c) return BMFR_ERROR_INVALID_ARGUMENT;
    if (overshoot) *overshoot = 0;
    DeviceGuard guard(c->device);
    const bmfr_status st = wait_frames(c);
    if (st != BMFR_OK) return st;
    if (c->reach_host && overshoot) *overshoot = c->reach_host[0];  // untiled: the whole image is valid state
    return reported(c);
}

bmfr_status bmfr_frame_status(bmfr_ctx* c) {
    if (!c) return BMFR_ERROR_INVALID_ARGUMENT;
    return bmfr_halo_status(c, nullptr);
}

bmfr_status bmfr_debug_sync(bmfr_ctx* c, int max_polls, int k1_delay) {
    if (!c || k1_delay < 0 || c->pending_frame >= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    c->P.max_polls = max_polls < 0 ? bmfr::kDefaultMaxPolls : max_polls;
    c->P.debug_delay = k1_delay;
    return BMFR_OK;
}

bmfr_status bmfr_debug_frame_launches(bmfr_ctx* c, int launches) {
    if (!c || launches < 0 || launches > 2 || c->pending_frame >= 0) return BMFR_ERROR_INVALID_ARGUMENT;
    c->P.frame_launches = launches;
    return BMFR_OK;
}

bmfr_status bmfr_debug_stamps(const bmfr_ctx* c, unsigned long long* host, size_t count) {
    if (!c || !host) return BMFR_ERROR_INVALID_ARGUMENT;
    if (!c->stamps) return BMFR_ERROR_UNSUPPORTED;
    DeviceGuard guard(c->device);
    const size_t n = (size_t)c->sizes.blocks * 8;
    return hip_status(hipMemcpy(host, c->stamps, (count < n ? count : n) * sizeof(unsigned long long),
                                hipMemcpyDeviceToHost));
}

const float* bmfr_output(const bmfr_ctx* c) {
    if (!c || !c->has_frame) return nullptr;
    return c->result[c->cur];
}

bmfr_status bmfr_state(const bmfr_ctx* c, int previous, bmfr_state_view* out) {
    if (!c || !out) return BMFR_ERROR_INVALID_ARGUMENT;
    const int i = previous ? 1 - c->cur : c->cur;
    out->noisy_accumulated = c->noisy_acc[i];
    out->spp = c->spp[i];
    out->filtered_accumulated = c->acc[i];
    out->tone_mapped = c->tone[i];
    out->prev_frame_pixel = reinterpret_cast<float*>(c->prev_pixel[i]);
    out->accept = nullptr;  // the fused kernel keeps accept bits in registers
    out->result = c->result[i];
    return BMFR_OK;
}

}  // extern "C"
