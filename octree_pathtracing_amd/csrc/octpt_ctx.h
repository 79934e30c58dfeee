// octpt_ctx.h -- the context behind the octpt C ABI (include/octpt.h) and what its two host files share:
// octpt_api.cpp (contexts, scenes, renders, builds, statistics) and octpt_post.cpp (guide buffers, denoisers, temporal
// passes, variance, adaptive and final frames).  Host code only (no .hip file includes it).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/octpt.h"
#include "octpt_internal.h"
#include "octpt_emitter.h"

namespace octpt {

constexpr uint32_t kCounterRing = 256;
constexpr uint64_t kMaxChunkPaths = 1ull << 31;    // colour buffer: up to 32 GiB of float4 per chunk (OCTPT_CHUNK)
constexpr uint64_t kDefaultChunkPaths = 1ull << 29;  // 4K: 64-spp chunks (C5 4634 vs 3882 Mrays/s at 2^30; C3 stays one chunk)
                                                    // (C3 = 530 M paths = one chunk: one drain tail)
#ifndef OCTPT_LOOKAHEAD
#define OCTPT_LOOKAHEAD 3
#endif
constexpr uint32_t kLookahead = OCTPT_LOOKAHEAD;    // host steering: iterations queued ahead of the check
constexpr uint32_t kDefaultPool = 512u << 20;        // path slots in flight (124 B each: queues + path state)
constexpr uint32_t kMaxPool = 1u << 30;              // the sun-sampling planes index 4 * pool slots in uint32
constexpr uint32_t kMinPool = 1u << 20;              // floor of the out-of-memory fallback (halving)
constexpr uint32_t kDefaultRefill = 0;               // extend: idle lanes before a wave refills (0: adaptive)
constexpr uint32_t kDefaultDrainRays = 4096;         // drain the chunk in one launch below this many queued rays
#ifndef OCTPT_SAMPLE_GROUP_DEFAULT
#define OCTPT_SAMPLE_GROUP_DEFAULT 64  // best on C3 once resolve reads a grouped chunk's records once
#endif
// a pixel's samples per wave of the chunk's item order, at most (1, 4, 16 or 64; OCTPT_SAMPLE_GROUP)
constexpr uint32_t kDefaultSampleGroup = OCTPT_SAMPLE_GROUP_DEFAULT;
constexpr uint64_t kGroupMinItems = 1ull << 27;       // chunks below this many items keep G = 1 unless OCTPT_SAMPLE_GROUP is set
// extend's refill threshold in the first launch of a grouped chunk whose queue holds the seed's camera records
// (OCTPT_REFILL_FIRST), per extend instance; 0: the adaptive rule, as in every other launch
#ifndef OCTPT_REFILL_FIRST_SPHERES
#define OCTPT_REFILL_FIRST_SPHERES 64  // C3 -6.6 % of its step; 32 / 60 give -1.3 %, 48 / 56 under 1 %
#endif
#ifndef OCTPT_REFILL_FIRST_BOXES
#define OCTPT_REFILL_FIRST_BOXES 64  // C4 -5.6 %; 60 gives -1.3 %, 48 -0.9 %
#endif
constexpr uint32_t kRefillFirstSpheres = OCTPT_REFILL_FIRST_SPHERES;
constexpr uint32_t kRefillFirstBoxes = OCTPT_REFILL_FIRST_BOXES;  // scenes with cuboids, without blocks or models

struct EventPair {
    hipEvent_t start, stop;
};

// a grow-only device buffer of the context: n elements of capacity at p (grow_buf, needs_grow, free_bufs)
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
};

}  // namespace octpt

struct octpt_ctx {
    int device = 0;
    int num_cu = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // scene
    bool has_scene = false;
    octpt::DevScene S{};
    std::vector<void *> scene_allocs;
    // camera
    bool has_camera = false;
    octpt_camera cam{};
    octpt::DevCamera C{};
    // the projection (C40, octpt_set_projection): PINHOLE in a new context; ctx->C carries its mode and half-param
    octpt_projection proj{};
    // the ray source (C41, octpt_set_ray_source): d_rays NULL = none.  The caller's buffer; ctx->C never carries it
    // (ray_source_camera below forms the camera a render passes to its kernels)
    octpt_ray_source rays{};
    // the sky (C42, octpt_set_sky): mode kSkyDefault in a new context.  A MAP's texels are the context's own copy
    // (sky_map, replaced whole by every MAP setting and freed by any other), which sky.texels points into
    octpt::Sky sky{};
    float *sky_map = nullptr;
    octpt_sky sky_pub{};  // the setting as octpt_get_sky returns it
    // sky sampling (C43, octpt_set_sky_sampling): the mode, and the map's distribution on the device while the mode is
    // MAP and the sky a MAP no wider than 32768 (row_cdf NULL else; refresh_sky_distribution keeps the rule)
    uint32_t sky_sampling = OCTPT_SKY_SAMPLING_NONE;
    octpt::DeviceSkyDist sky_dist{};
    // per-context device state
    uint32_t *d_counters = nullptr;  // ring of work counters, one per launch
    // branch schedule of the current render (C20): host copy + grow-only device table
    std::vector<uint2> h_subs;
    octpt::DevBuf<uint2> d_subs;
    // beam starts of the camera rays, one per kBeamTile^2 pixels (beam_kernel), grow-only
    octpt::DevBuf<float> d_beam;
    uint32_t launch_seq = 0;
    unsigned long long *d_stats = nullptr;
    uint8_t *d_lut_byte = nullptr;
    float *d_lut_float = nullptr;
    std::vector<octpt::EventPair> pending;
    double kernel_ms = 0.0;
    uint64_t launches = 0;
    // per-kernel timing (OCTPT_RENDER_KERNEL_TIMING): kind 0 extend, 1 shade
    bool ktiming = false;
    std::vector<std::pair<int, octpt::EventPair>> kpending;
    std::vector<octpt::EventPair> ev_pool;
    double kern_ms[2] = {0.0, 0.0};
    uint64_t kern_n[2] = {0, 0};
    float build_ms = 0.0f;  // device time of the last octpt_build_octree_device
    octpt::BuildScratch build_scratch;
    int blocks_per_cu_cache[octpt::kMaxDepth + 1] = {0};
    int extend_bpc_cache[octpt::kMaxDepth + 1][4] = {};  // [depth][kPrims]
    int shade_bpc_cache[2][2][3] = {};            // [sun sampling][LDS tables][shade_mode]
    bool lean_scene = false;  // no emitters, no sun sampling: the lean path state applies when the pool holds the chunk
    bool no_lean = false;     // OCTPT_LEAN=0: always the 40-B path state (A/B, tests)
    bool sample_group_set = false;                // OCTPT_SAMPLE_GROUP given: no rule about where the order is grouped
    uint32_t sample_group = octpt::kDefaultSampleGroup;  // OCTPT_SAMPLE_GROUP: the item order's G at most; 1 = one sample per wave
    // wavefront pool (grown on demand)
    octpt::WaveBuffers wb{};
    size_t pool = 0, color_cap = 0, nee_pool = 0;  // nee_pool: slots of the sun-sampling planes (wb.pd)
    void *nee_alloc = nullptr;
    std::vector<void *> wave_allocs;
    void *color_alloc = nullptr;
    // device bytes of the wavefront state (queues, path state, colour records, sun-sampling planes),
    // tracked against mem_limit (OCTPT_DEVICE_MEM_LIMIT, MiB, 0 = none: a test hook that makes the
    // out-of-memory fallback reproducible on an idle GPU)
    size_t wave_bytes = 0, mem_limit = 0;
    std::vector<std::pair<void *, size_t>> wave_sizes;
    uint64_t wave_allocs_n = 0;  // successful (re)allocations of the queues + path state
    bool oom_warned = false;
    uint32_t *h_count = nullptr;  // pinned ring: the segment counters after each iteration's shade
    uint32_t *d_count = nullptr;  // its device address (wf_snapshot_kernel)
    hipEvent_t count_ev[octpt::kLookahead + 1] = {};
    uint32_t pool_cap = octpt::kDefaultPool, refill = octpt::kDefaultRefill;
    int32_t refill_first = -1;  // OCTPT_REFILL_FIRST (0..64); -1: unset, the extend instance's compiled default
    bool beam = true;  // camera rays start at their tile's beam (OCTPT_BEAM=0: off)
    uint32_t drain_rays = octpt::kDefaultDrainRays;  // queue length at which the drain takes over (OCTPT_DRAIN_RAYS, 0 = off)
    bool drain_models = false;                // the drain in block-model scenes too (OCTPT_DRAIN_MODELS=1, A/B)
    uint64_t chunk_cap = octpt::kDefaultChunkPaths;  // (pixel, sample) items per chunk (OCTPT_CHUNK)
    // one asynchronous frame may be in flight; device-touching calls join it first
    octpt_frame *inflight = nullptr;
    // multi-device context (octpt_create_multi): one child context per device entry; this context's own
    // device is the first entry's, where the caller's buffers live.  Empty for octpt_create.
    std::vector<octpt_ctx *> sub;
    // multi-device renders: the staged compact tile buffers (this context: every entry's, side by side on
    // the first device; a child: its own), grow-only
    octpt::DevBuf<float4> m_acc;
    octpt::DevBuf<uint32_t> m_seg;
    // the denoiser's two ping-pong frames (octpt_denoise_device, C25), allocated on first use, grow-only
    octpt::DevBuf<float4> dn_frame[2];
    // the tile deal (octpt_set_tile_order): for order_w x order_h frames, dealing position -> frame tile and
    // its inverse, on this context's device; empty = the round-robin deal
    std::vector<uint32_t> h_order;
    uint32_t order_w = 0, order_h = 0;
    uint32_t *d_order = nullptr, *d_order_pos = nullptr;
    // what the beam table in d_beam was computed for (round 5): the scene, camera and tile order (their
    // generations) and the frame size and shard.  A render with the same key reuses it -- a progressive
    // renderer calls render_frame again and again with one camera -- and anything else recomputes it.
    uint64_t scene_gen = 0, camera_gen = 0, order_gen = 0;
    struct BeamKey {
        uint64_t scene = 0, camera = 0, order = 0;
        // a tile-list render (octpt_render_tiles_device) computes only its tiles' starts: its list's number, a
        // fresh one per call (0 = an ordinary render), so that no render takes such a table for its own
        uint64_t list = 0;
        uint32_t w = 0, h = 0, shard_index = 0, shard_count = 0;
        bool valid = false;
        bool operator==(const BeamKey &o) const {
            return valid && o.valid && scene == o.scene && camera == o.camera && order == o.order && list == o.list &&
                   w == o.w && h == o.h && shard_index == o.shard_index && shard_count == o.shard_count;
        }
    } beam_key;
    // tile-list renders (C30): the list as the deal (octpt::DevRender::tile_order), grow-only like d_subs, and the
    // number of the last list (BeamKey::list)
    octpt::DevBuf<uint32_t> d_tiles;
    uint64_t list_gen = 0;
    // the adaptive driver (C32): its device copies of tile_spp and the per-tile error, grow-only
    octpt::DevBuf<uint32_t> d_tile_spp;
    octpt::DevBuf<float> d_tile_err;
    // the sample clamp of resolve (C33, octpt_set_sample_clamp): 0 = off
    float sample_clamp = 0.0f;
    // emitter sampling (C38, octpt_set_emitter_sampling): the setting, the scene's emissive flag per block (empty
    // for a scene of primitive leaves), and the device grid built when strategy ONE and a block-value scene are
    // both known (grid_valid; its three arrays are allocations of their own)
    uint32_t emit_strategy = OCTPT_EMITTERS_NONE, emit_grid_size = 8u;
    float emit_intensity = 1.0f;
    uint32_t emit_flags = 0u;  // OCTPT_EMITTERS_MODELS (C39)
    std::vector<uint32_t> block_emissive;
    // model emitters (C39): the scene's emissive-model table, built on the host at the scene entry, its emissive
    // byte per model, and the table on the device (scene allocations, uploaded once per scene when a grid with
    // OCTPT_EMITTERS_MODELS is first built)
    octpt::EmissiveModelTable emit_models;
    std::vector<uint8_t> model_emissive;
    uint32_t *d_model_first = nullptr, *d_model_quad = nullptr;
    float *d_model_cum = nullptr, *d_model_ouv = nullptr;
    octpt::DeviceEmitterGrid emit_grid;
    bool grid_valid = false;
    octpt::EmitGrid *d_emit_hdr = nullptr;  // the render's octpt::EmitGrid on the device (the emitter instances' S.leaf_sph)
    octpt::EmitGrid emit_hdr_host{};        // ... and what it holds (uploaded again only when the grid or the intensity changed)
    bool emit_hdr_valid = false;
    size_t nee_planes = 0;           // planes of wb.pd per slot: 4 (sun sampling) or 6 (emitter sampling)
    // the seam rule's spread error plane (C34, the _ex driver) and the finished frame's guide and variance planes
    // (C36, octpt_render_final_device), grow-only
    octpt::DevBuf<float> d_tile_spread;
    octpt::DevBuf<float4> fin_normal, fin_albedo;
    octpt::DevBuf<float> fin_depth, fin_var;
    // recorded on the stream that computed the table: a render on another stream that reuses it waits for it
    hipEvent_t beam_ev = nullptr;
    hipStream_t beam_stream = nullptr;  // the stream the valid table was computed on
    bool beam_shared = false;           // ... and whether a render on another stream has read it since
};

struct octpt_frame {
    octpt_ctx *ctx = nullptr;
    octpt_render_params params{};  // the call's parameters (a multi-device context re-derives each entry's)
    std::thread worker;
    std::atomic<bool> finished{false};
    std::atomic<bool> cancel_requested{false};
    octpt_status status = OCTPT_OK;
    float *user_accum = nullptr;
    uint8_t *user_rgba = nullptr;
    size_t n_pixels = 0;
    float4 *d_accum = nullptr;
    uchar4 *d_rgba = nullptr;
    float *h_accum = nullptr;   // pinned
    uint8_t *h_rgba = nullptr;  // pinned
    bool delivered = false;
};

namespace octpt {

inline octpt_status fail(octpt_ctx *ctx, octpt_status st, const std::string &msg) {
    if (ctx) ctx->err = msg;
    return st;
}

inline octpt_status hip_fail(octpt_ctx *ctx, hipError_t e, const char *what) {
    return fail(ctx, e == hipErrorOutOfMemory ? OCTPT_ERR_OOM : OCTPT_ERR_DEVICE,
                std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(ctx, expr)                                 \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return hip_fail(ctx, _e, #expr); \
    } while (0)

// An entry's body under the C boundary's exception rule: nothing crosses it.  `name` names the entry in the message.
template <class Body>
octpt_status guarded(octpt_ctx *ctx, const char *name, Body body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(ctx, OCTPT_ERR_OOM, "host allocation");
    } catch (...) {
        return fail(ctx, OCTPT_ERR_INTERNAL, std::string("unexpected exception in ") + name);
    }
}

// whether one of the buffers has to grow to hold n elements: a buffer that grows is freed, and an earlier call on
// another stream may still read it, so such a call site drains the device first
template <class... T>
bool needs_grow(size_t n, const DevBuf<T> &...bufs) {
    return ((n > bufs.n) || ...);
}

// b holds at least n elements on the current device after this; the old buffer goes first, and a failed allocation
// leaves b empty
template <class T>
octpt_status grow_buf(octpt_ctx *ctx, DevBuf<T> &b, size_t n) {
    if (n <= b.n) return OCTPT_OK;
    if (b.p) (void)hipFree(b.p);
    b = DevBuf<T>{};
    HIP_TRY(ctx, hipMalloc(&b.p, n * sizeof(T)));
    b.n = n;
    return OCTPT_OK;
}

template <class... T>
void free_bufs(DevBuf<T> &...bufs) {
    ((bufs.p ? (void)hipFree(bufs.p) : (void)0, bufs = DevBuf<T>{}), ...);
}

// the status of a call a multi-device context made on its first entry's replica (the caller's buffers live on its
// device), with that entry's message
inline octpt_status forwarded(octpt_ctx *ctx, octpt_status st) { return st == OCTPT_OK ? st : fail(ctx, st, ctx->sub[0]->err); }

inline bool is_multi(const octpt_ctx *ctx) { return !ctx->sub.empty(); }

// the 8x8 tiles of a W x H frame
inline uint32_t frame_tiles(uint32_t W, uint32_t H) { return ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile); }

// the camera a render passes to its kernels: the context's, and under a ray source (C41) that camera carrying the
// list in the fields the ray-list instances do not read (set_cam_ray_list, octpt_internal.h)
inline DevCamera ray_source_camera(const octpt_ctx *ctx) {
    DevCamera C = ctx->C;
    if (ctx->rays.d_rays) set_cam_ray_list(C, ctx->rays.d_rays, ctx->rays.rays_per_pixel);
    return C;
}

// the pixels of a render's accumulation buffer
inline size_t accum_pixels(const DevRender &R) { return R.compact ? (size_t)R.total_items : (size_t)R.W * R.H; }

// octpt_api.cpp: a frame in flight is joined before a call touches the device; the layout of a render call and its
// checks; a render of that layout on stream s (d_moments, nullable: resolve's moments instance, C31; list: the number
// of a tile-list render's list, C30, 0 for every other render)
void join_inflight(octpt_ctx *ctx);
octpt_status make_render(octpt_ctx *ctx, const octpt_render_params *p, DevRender &R);
octpt_status enqueue_render(octpt_ctx *ctx, const DevRender &R, float4 *d_accum, uint32_t *d_seg, hipStream_t s,
                            bool megakernel, const std::atomic<bool> *cancel = nullptr, float2 *d_moments = nullptr,
                            uint64_t list = 0);

}  // namespace octpt
