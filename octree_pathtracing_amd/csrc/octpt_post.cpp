// octpt_post.cpp -- the post-processing entries of the octpt C ABI (include/octpt.h): first-hit guide buffers, the two
// denoisers, temporal reprojection and luminance moments, variance, tile-list renders and the per-tile error, the
// adaptive drivers, the sample clamp, the seam rule's spread, the sample variance and the finished frame.  Each entry
// is a device form and a host-pointer form that stages the caller's buffers (octpt_stage.h) around it.  The context
// and what this file shares with octpt_api.cpp are in octpt_ctx.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "octpt_ctx.h"
#include "octpt_reproject.h"
#include "octpt_stage.h"

using namespace octpt;

extern "C" {

// ---------------- first-hit guide buffers (C24) and the preview denoiser (C25) ----------------
namespace {

// the render layout of a guide-buffer pass: only the frame size, the shard and the compact flag apply
octpt_status make_aov_render(octpt_ctx *ctx, const octpt_render_params *p, DevRender &R) {
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render params NULL");
    octpt_render_params q{};
    q.width = p->width;
    q.height = p->height;
    q.spp_count = 1u;
    q.max_depth = 1u;
    q.branch_count = 1u;
    q.shard_index = p->shard_index;
    q.shard_count = p->shard_count;
    q.flags = p->flags & OCTPT_RENDER_SHARD_COMPACT;
    const bool ktiming = ctx->ktiming;
    const octpt_status st = make_render(ctx, &q, R);
    ctx->ktiming = ktiming;
    return st;
}

bool aov_any(const octpt_aov_buffers &b) { return b.albedo || b.normal || b.depth || b.prim || b.material; }

octpt_status enqueue_aov(octpt_ctx *ctx, const DevRender &R, const octpt_aov_buffers &dev, hipStream_t s) {
    if (R.total_items == 0 || !aov_any(dev)) return OCTPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    EventPair ev{};
    HIP_TRY(ctx, hipEventCreate(&ev.start));
    HIP_TRY(ctx, hipEventCreate(&ev.stop));
    ctx->pending.push_back(ev);  // destroyed by get_stats / destroy
    HIP_TRY(ctx, hipEventRecord(ev.start, s));
    const DevAov out{reinterpret_cast<float4 *>(dev.albedo), reinterpret_cast<float4 *>(dev.normal), dev.depth, dev.prim,
                     dev.material};
    const hipError_t e = launch_gbuffer(ctx->S, ray_source_camera(ctx), R, out, ctx->d_stats, s);
    HIP_TRY(ctx, hipEventRecord(ev.stop, s));
    if (e != hipSuccess) return hip_fail(ctx, e, "guide buffer launch");
    ctx->launches++;
    return OCTPT_OK;
}

octpt_status check_denoise(octpt_ctx *ctx, const octpt_denoise_params *p, const void *color,
                           const octpt_aov_buffers *g, const void *out) {
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise params NULL");
    if (p->width == 0 || p->height == 0) return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise: zero frame size");
    if ((uint64_t)p->width * p->height >= (1ull << 31) || p->height > 8u * 65535u)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise: bad resolution");
    if (p->iterations < 1u || p->iterations > 5u) return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise: iterations must be 1..5");
    for (float s : {p->sigma_color, p->sigma_normal, p->sigma_depth})
        if (!(s > 0.0f) || !std::isfinite(s))
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise: sigma_color, sigma_normal and sigma_depth must be positive and finite");
    if (p->flags & ~OCTPT_DENOISE_DEMODULATE)
        return fail(ctx, OCTPT_ERR_INVALID_ARG,
                    "denoise: unknown flag (full frames only: no shard or compact tile layout; OCTPT_DENOISE_DEMODULATE is the one flag)");
    if (!color || !out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise: NULL colour or output buffer");
    if (!g || !g->normal || !g->depth)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise: the normal and depth guides are required");
    if ((p->flags & OCTPT_DENOISE_DEMODULATE) && !g->albedo)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise: OCTPT_DENOISE_DEMODULATE needs the albedo guide");
    return OCTPT_OK;
}

}  // namespace

octpt_status octpt_render_aov_device(octpt_ctx *ctx, const octpt_render_params *p, const octpt_aov_buffers *dev,
                                     void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render params NULL");
    if (!dev) return fail(ctx, OCTPT_ERR_INVALID_ARG, "guide buffers NULL");
    return guarded(ctx, "guide buffer render", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_render_aov_device(ctx->sub[0], p, dev, stream));
        DevRender R{};
        const octpt_status st = make_aov_render(ctx, p, R);
        if (st != OCTPT_OK) return st;
        return enqueue_aov(ctx, R, *dev, static_cast<hipStream_t>(stream));
    });
}

octpt_status octpt_render_aov(octpt_ctx *ctx, const octpt_render_params *p, const octpt_aov_buffers *host) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render params NULL");
    if (!host) return fail(ctx, OCTPT_ERR_INVALID_ARG, "guide buffers NULL");
    return guarded(ctx, "guide buffer render", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_render_aov(ctx->sub[0], p, host));
        DevRender R{};
        octpt_status st = make_aov_render(ctx, p, R);
        if (st != OCTPT_OK) return st;
        if (R.total_items == 0 || !aov_any(*host)) return OCTPT_OK;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = accum_pixels(R);
        // pixels the pass does not write (a partial shard of a full frame, tile padding) keep the caller's values
        HostStage hs(ctx->stream);
        const octpt_aov_buffers dev{hs.inout(host->albedo, host->albedo, 4 * n), hs.inout(host->normal, host->normal, 4 * n),
                                    hs.inout(host->depth, host->depth, n), hs.inout(host->prim, host->prim, n),
                                    hs.inout(host->material, host->material, n)};
        if (hs.ok() && (st = enqueue_aov(ctx, R, dev, ctx->stream)) != OCTPT_OK) return st;
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "guide buffer render");
        return OCTPT_OK;
    });
}

octpt_status octpt_denoise_device(octpt_ctx *ctx, const octpt_denoise_params *p, const float *d_color,
                                  const octpt_aov_buffers *g, float *d_out, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_denoise(ctx, p, d_color, g, d_out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "denoise", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_denoise_device(ctx->sub[0], p, d_color, g, d_out, stream));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height;
        // the working signal lives in frame 0 after the prep pass, then ping-pongs; the last iteration writes d_out.
        // A frame that has to grow may still be read by an earlier call on another stream: drain first
        const bool two = p->iterations > 1u;
        if (needs_grow(n, ctx->dn_frame[0]) || (two && needs_grow(n, ctx->dn_frame[1]))) HIP_TRY(ctx, hipDeviceSynchronize());
        if ((st = grow_buf(ctx, ctx->dn_frame[0], n)) != OCTPT_OK) return st;
        if (two && (st = grow_buf(ctx, ctx->dn_frame[1], n)) != OCTPT_OK) return st;
        hipStream_t s = static_cast<hipStream_t>(stream);
        DevDenoise D{};
        D.W = p->width;
        D.H = p->height;
        D.sigma_color = p->sigma_color;
        D.sn2 = p->sigma_normal * p->sigma_normal;
        D.sz2 = p->sigma_depth * p->sigma_depth;
        D.normal = reinterpret_cast<const float4 *>(g->normal);
        D.albedo = (p->flags & OCTPT_DENOISE_DEMODULATE) ? reinterpret_cast<const float4 *>(g->albedo) : nullptr;
        D.depth = g->depth;
        HIP_TRY(ctx, launch_denoise_prep(D.W, D.H, reinterpret_cast<const float4 *>(d_color), D.albedo, D.depth,
                                         ctx->dn_frame[0].p, s));
        for (uint32_t i = 0; i < p->iterations; ++i) {
            const bool last = i + 1u == p->iterations;
            float4 *dst = last ? reinterpret_cast<float4 *>(d_out) : ctx->dn_frame[(i + 1u) & 1u].p;
            HIP_TRY(ctx, launch_atrous(D, i, last, ctx->dn_frame[i & 1u].p, dst, s));
        }
        return OCTPT_OK;
    });
}

octpt_status octpt_denoise(octpt_ctx *ctx, const octpt_denoise_params *p, const float *color,
                           const octpt_aov_buffers *g, float *out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_denoise(ctx, p, color, g, out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "denoise", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_denoise(ctx->sub[0], p, color, g, out));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height;
        const bool demod = (p->flags & OCTPT_DENOISE_DEMODULATE) != 0u;
        HostStage hs(ctx->stream);
        float *d_color = hs.inout(color, out, 4 * n);  // filtered in place on the device
        float *d_normal = hs.in(g->normal, 4 * n), *d_depth = hs.in(g->depth, n);
        const octpt_aov_buffers dg{hs.in(demod ? g->albedo : nullptr, 4 * n), d_normal, d_depth, nullptr, nullptr};
        if (hs.ok() && (st = octpt_denoise_device(ctx, p, d_color, &dg, d_color, ctx->stream)) != OCTPT_OK) return st;
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "denoise");
        return OCTPT_OK;
    });
}

// ---------------- temporal reprojection of the preview history (C26) ----------------
namespace {

// `who` names the pass in the messages; moments: the C27 entries, which also accept OCTPT_TEMPORAL_DEMODULATE
octpt_status check_temporal(octpt_ctx *ctx, const char *who, bool moments, const octpt_temporal_params *p, const void *color,
                            const octpt_aov_buffers *g, const octpt_temporal_history *prev, const void *out,
                            const void *out_length) {
    const std::string w = std::string(who) + ": ";
    // the mapping is the pinhole camera's: a context whose renders are projected otherwise has no history to carry (C40)
    if (ctx->proj.mode != OCTPT_PROJECTION_PINHOLE)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, w + "the context's projection is not pinhole (octpt_set_projection)");
    // ... nor has one whose first rays are the caller's (C41)
    if (ctx->rays.d_rays)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, w + "the context has a ray source (octpt_set_ray_source)");
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, std::string(who) + " params NULL");
    if (p->width == 0 || p->height == 0) return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "zero frame size");
    if ((uint64_t)p->width * p->height >= (1ull << 31) || p->height > 8u * 65535u)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "bad resolution");
    if (p->max_history < 1u || p->max_history > 65535u)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "max_history must be 1..65535");
    if (!(p->depth_tolerance > 0.0f) || !std::isfinite(p->depth_tolerance))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "depth_tolerance must be positive and finite");
    if (!(p->normal_threshold >= -1.0f && p->normal_threshold <= 1.0f))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "normal_threshold must be in [-1, 1]");
    if (p->flags & ~(OCTPT_TEMPORAL_MATCH_PRIM | (moments ? OCTPT_TEMPORAL_DEMODULATE : 0u)))
        return fail(ctx, OCTPT_ERR_INVALID_ARG,
                    w + (moments ? "unknown flag (full frames only: no shard or compact tile layout; OCTPT_TEMPORAL_MATCH_PRIM and OCTPT_TEMPORAL_DEMODULATE are the flags)"
                                 : "unknown flag (full frames only: no shard or compact tile layout; OCTPT_TEMPORAL_MATCH_PRIM is the one flag)"));
    const char *why = nullptr;
    const octpt_status st = check_reproject_cameras(&p->camera, &p->prev_camera, &why);
    if (st != OCTPT_OK) return fail(ctx, st, w + why);
    const bool match = (p->flags & OCTPT_TEMPORAL_MATCH_PRIM) != 0u;
    if (!color || !out || !out_length) return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "NULL colour, output or output length buffer");
    if (!g || !g->normal || !g->depth) return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "the normal and depth guides are required");
    if (match && !g->prim) return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "OCTPT_TEMPORAL_MATCH_PRIM needs the prim guide");
    if ((p->flags & OCTPT_TEMPORAL_DEMODULATE) && !g->albedo)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "OCTPT_TEMPORAL_DEMODULATE needs the albedo guide");
    if (prev) {
        if (!prev->color || !prev->normal || !prev->depth || !prev->length)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "the history needs its colour, normal, depth and length");
        if (match && !prev->prim) return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "OCTPT_TEMPORAL_MATCH_PRIM needs the history's prim");
        // the pass gathers from the history while it writes: only the current colour may be the output
        if (out == prev->color) return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "the output must not be the history colour");
        if (out_length == prev->length)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, w + "the output length must not be the history length");
    }
    return OCTPT_OK;
}

// C27's own arguments, after check_temporal
octpt_status check_moments(octpt_ctx *ctx, const octpt_temporal_history *prev, const void *prev_moments,
                           const void *out_moments) {
    if (!out_moments) return fail(ctx, OCTPT_ERR_INVALID_ARG, "temporal_moments: NULL output moments buffer");
    if (prev && !prev_moments)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "temporal_moments: a history needs its moments");
    if (!prev && prev_moments)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "temporal_moments: previous moments without a history (the first frame takes neither)");
    if (out_moments == prev_moments)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "temporal_moments: the output moments must not be the history moments");
    return OCTPT_OK;
}

DevCamera dev_camera(const octpt_camera &c) {
    const CameraBasis b = camera_basis(c.eye, c.direction, c.up, c.fov);
    DevCamera C{};
    std::memcpy(C.eye, b.eye, 12);
    std::memcpy(C.dir, b.dir, 12);
    std::memcpy(C.right, b.right, 12);
    std::memcpy(C.up, b.up, 12);
    C.d_factor = b.d_factor;
    return C;
}

}  // namespace

namespace {

// both temporal entries' device form after their checks; d_out_moments NULL = octpt_temporal_device (C26)
octpt_status enqueue_temporal(octpt_ctx *ctx, const octpt_temporal_params *p, const float *d_color, const octpt_aov_buffers *g,
                              const octpt_temporal_history *prev, const float *d_prev_moments, float *d_out,
                              uint32_t *d_out_length, float *d_out_moments, void *stream) {
    join_inflight(ctx);
    if (is_multi(ctx))
        return forwarded(ctx, d_out_moments
                                  ? octpt_temporal_moments_device(ctx->sub[0], p, d_color, g, prev, d_prev_moments, d_out,
                                                                  d_out_length, d_out_moments, stream)
                                  : octpt_temporal_device(ctx->sub[0], p, d_color, g, prev, d_out, d_out_length, stream));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool match = (p->flags & OCTPT_TEMPORAL_MATCH_PRIM) != 0u;
    DevTemporal T{};
    T.W = p->width;
    T.H = p->height;
    T.dim = (float)(p->width > p->height ? p->width : p->height);
    T.cur = dev_camera(p->camera);
    T.prev = dev_camera(p->prev_camera);
    T.max_history = p->max_history;
    T.depth_tolerance = p->depth_tolerance;
    T.normal_threshold = p->normal_threshold;
    T.match_prim = match ? 1u : 0u;
    T.color = reinterpret_cast<const float4 *>(d_color);
    T.normal = reinterpret_cast<const float4 *>(g->normal);
    T.depth = g->depth;
    T.prim = match ? g->prim : nullptr;
    if (prev) {
        T.h_color = reinterpret_cast<const float4 *>(prev->color);
        T.h_normal = reinterpret_cast<const float4 *>(prev->normal);
        T.h_depth = prev->depth;
        T.h_prim = match ? prev->prim : nullptr;
        T.h_length = prev->length;
        T.h_moments = reinterpret_cast<const float2 *>(d_prev_moments);
    }
    T.out = reinterpret_cast<float4 *>(d_out);
    T.out_length = d_out_length;
    T.albedo = (p->flags & OCTPT_TEMPORAL_DEMODULATE) ? reinterpret_cast<const float4 *>(g->albedo) : nullptr;
    T.out_moments = reinterpret_cast<float2 *>(d_out_moments);
    HIP_TRY(ctx, launch_temporal(T, d_out_moments != nullptr, static_cast<hipStream_t>(stream)));
    return OCTPT_OK;
}

// both temporal entries' host form after their checks; out_moments NULL = octpt_temporal (C26)
octpt_status temporal_host(octpt_ctx *ctx, const octpt_temporal_params *p, const float *color, const octpt_aov_buffers *g,
                           const octpt_temporal_history *prev, const float *prev_moments, float *out, uint32_t *out_length,
                           float *out_moments) {
    join_inflight(ctx);
    if (is_multi(ctx))
        return forwarded(ctx, out_moments ? octpt_temporal_moments(ctx->sub[0], p, color, g, prev, prev_moments, out,
                                                                   out_length, out_moments)
                                          : octpt_temporal(ctx->sub[0], p, color, g, prev, out, out_length));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)p->width * p->height;
    const bool match = (p->flags & OCTPT_TEMPORAL_MATCH_PRIM) != 0u;
    const bool demod = (p->flags & OCTPT_TEMPORAL_DEMODULATE) != 0u;
    HostStage hs(ctx->stream);
    float *d_color = hs.inout(color, out, 4 * n);  // blended in place on the device
    octpt_aov_buffers dg{nullptr, hs.in(g->normal, 4 * n), hs.in(g->depth, n), hs.in(match ? g->prim : nullptr, n), nullptr};
    octpt_temporal_history dp{};
    if (prev)
        dp = {hs.in(prev->color, 4 * n), hs.in(prev->normal, 4 * n), hs.in(prev->depth, n),
              hs.in(match ? prev->prim : nullptr, n), hs.in(prev->length, n)};
    dg.albedo = hs.in(demod ? g->albedo : nullptr, 4 * n);
    const float *d_prev_moments = hs.in(prev ? prev_moments : nullptr, 2 * n);  // (C27)
    uint32_t *d_out_length = hs.out(out_length, n);
    float *d_out_moments = hs.out(out_moments, 2 * n);
    octpt_status st = OCTPT_OK;
    if (hs.ok() && (st = enqueue_temporal(ctx, p, d_color, &dg, prev ? &dp : nullptr, d_prev_moments, d_color, d_out_length,
                                          d_out_moments, ctx->stream)) != OCTPT_OK)
        return st;
    if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "temporal");
    return OCTPT_OK;
}

}  // namespace

octpt_status octpt_temporal_device(octpt_ctx *ctx, const octpt_temporal_params *p, const float *d_color,
                                   const octpt_aov_buffers *g, const octpt_temporal_history *prev, float *d_out,
                                   uint32_t *d_out_length, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    const octpt_status st = check_temporal(ctx, "temporal", false, p, d_color, g, prev, d_out, d_out_length);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "temporal", [&]() -> octpt_status {
        return enqueue_temporal(ctx, p, d_color, g, prev, nullptr, d_out, d_out_length, nullptr, stream);
    });
}

octpt_status octpt_temporal(octpt_ctx *ctx, const octpt_temporal_params *p, const float *color,
                            const octpt_aov_buffers *g, const octpt_temporal_history *prev, float *out,
                            uint32_t *out_length) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    const octpt_status st = check_temporal(ctx, "temporal", false, p, color, g, prev, out, out_length);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "temporal", [&]() -> octpt_status {
        return temporal_host(ctx, p, color, g, prev, nullptr, out, out_length, nullptr);
    });
}

// octpt_reproject_coords for a context's frames: refused while the context's projection is not pinhole (C40)
octpt_status octpt_reproject_coords_ctx(octpt_ctx *ctx, const octpt_camera *camera, const octpt_camera *prev_camera,
                                        uint32_t width, uint32_t height, const float *depth, float *prev_xy,
                                        float *prev_depth) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (ctx->proj.mode != OCTPT_PROJECTION_PINHOLE)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "reproject_coords: the context's projection is not pinhole (octpt_set_projection)");
    if (ctx->rays.d_rays)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "reproject_coords: the context has a ray source (octpt_set_ray_source)");
    const octpt_status st = octpt_reproject_coords(camera, prev_camera, width, height, depth, prev_xy, prev_depth);
    return st == OCTPT_OK ? st : fail(ctx, st, "reproject_coords: refused (octpt_reproject_coords' rules)");
}

// ---------------- luminance moments, variance and the variance-guided filter (C27-C29) ----------------
octpt_status octpt_temporal_moments_device(octpt_ctx *ctx, const octpt_temporal_params *p, const float *d_color,
                                           const octpt_aov_buffers *g, const octpt_temporal_history *prev,
                                           const float *d_prev_moments, float *d_out, uint32_t *d_out_length,
                                           float *d_out_moments, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_temporal(ctx, "temporal_moments", true, p, d_color, g, prev, d_out, d_out_length);
    if (st == OCTPT_OK) st = check_moments(ctx, prev, d_prev_moments, d_out_moments);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "temporal_moments", [&]() -> octpt_status {
        return enqueue_temporal(ctx, p, d_color, g, prev, d_prev_moments, d_out, d_out_length, d_out_moments, stream);
    });
}

octpt_status octpt_temporal_moments(octpt_ctx *ctx, const octpt_temporal_params *p, const float *color,
                                    const octpt_aov_buffers *g, const octpt_temporal_history *prev,
                                    const float *prev_moments, float *out, uint32_t *out_length, float *out_moments) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_temporal(ctx, "temporal_moments", true, p, color, g, prev, out, out_length);
    if (st == OCTPT_OK) st = check_moments(ctx, prev, prev_moments, out_moments);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "temporal_moments", [&]() -> octpt_status {
        return temporal_host(ctx, p, color, g, prev, prev_moments, out, out_length, out_moments);
    });
}

namespace {

octpt_status check_variance(octpt_ctx *ctx, const octpt_variance_params *p, const void *moments, const void *length,
                            const octpt_aov_buffers *g, const void *out) {
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "variance params NULL");
    if (p->width == 0 || p->height == 0) return fail(ctx, OCTPT_ERR_INVALID_ARG, "variance: zero frame size");
    if ((uint64_t)p->width * p->height >= (1ull << 31) || p->height > 8u * 65535u)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "variance: bad resolution");
    if (p->min_history < 1u || p->min_history > 65535u)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "variance: min_history must be 1..65535");
    for (float s : {p->sigma_normal, p->sigma_depth})
        if (!(s > 0.0f) || !std::isfinite(s))
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "variance: sigma_normal and sigma_depth must be positive and finite");
    if (!moments || !length || !out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "variance: NULL moments, length or output buffer");
    if (!g || !g->normal || !g->depth)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "variance: the normal and depth guides are required");
    return OCTPT_OK;
}

octpt_status check_denoise_variance(octpt_ctx *ctx, const octpt_denoise_variance_params *p, const void *color,
                                    const void *variance, const octpt_aov_buffers *g, const void *out) {
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise_variance params NULL");
    if (p->width == 0 || p->height == 0) return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise_variance: zero frame size");
    if ((uint64_t)p->width * p->height >= (1ull << 31) || p->height > 8u * 65535u)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise_variance: bad resolution");
    if (p->iterations < 1u || p->iterations > 5u)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise_variance: iterations must be 1..5");
    for (float s : {p->sigma_luminance, p->luminance_floor, p->sigma_normal, p->sigma_depth})
        if (!(s > 0.0f) || !std::isfinite(s))
            return fail(ctx, OCTPT_ERR_INVALID_ARG,
                        "denoise_variance: sigma_luminance, luminance_floor, sigma_normal and sigma_depth must be positive and finite");
    if (p->flags & ~OCTPT_DENOISE_DEMODULATE)
        return fail(ctx, OCTPT_ERR_INVALID_ARG,
                    "denoise_variance: unknown flag (full frames only: no shard or compact tile layout; OCTPT_DENOISE_DEMODULATE is the one flag)");
    if (!color || !variance || !out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise_variance: NULL colour, variance or output buffer");
    if (!g || !g->normal || !g->depth)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise_variance: the normal and depth guides are required");
    if ((p->flags & OCTPT_DENOISE_DEMODULATE) && !g->albedo)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "denoise_variance: OCTPT_DENOISE_DEMODULATE needs the albedo guide");
    return OCTPT_OK;
}

}  // namespace

octpt_status octpt_variance_device(octpt_ctx *ctx, const octpt_variance_params *p, const float *d_moments,
                                   const uint32_t *d_length, const octpt_aov_buffers *g, float *d_out, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_variance(ctx, p, d_moments, d_length, g, d_out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "variance", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_variance_device(ctx->sub[0], p, d_moments, d_length, g, d_out, stream));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        DevVariance V{};
        V.W = p->width;
        V.H = p->height;
        V.min_history = p->min_history;
        V.sn2 = p->sigma_normal * p->sigma_normal;
        V.sz2 = p->sigma_depth * p->sigma_depth;
        V.moments = reinterpret_cast<const float2 *>(d_moments);
        V.length = d_length;
        V.normal = reinterpret_cast<const float4 *>(g->normal);
        V.depth = g->depth;
        V.out = d_out;
        HIP_TRY(ctx, launch_variance(V, static_cast<hipStream_t>(stream)));
        return OCTPT_OK;
    });
}

octpt_status octpt_variance(octpt_ctx *ctx, const octpt_variance_params *p, const float *moments, const uint32_t *length,
                            const octpt_aov_buffers *g, float *out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_variance(ctx, p, moments, length, g, out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "variance", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_variance(ctx->sub[0], p, moments, length, g, out));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height;
        HostStage hs(ctx->stream);
        const float *d_moments = hs.in(moments, 2 * n);
        const uint32_t *d_length = hs.in(length, n);
        const octpt_aov_buffers dg{nullptr, hs.in(g->normal, 4 * n), hs.in(g->depth, n), nullptr, nullptr};
        float *d_out = hs.out(out, n);
        if (hs.ok() && (st = octpt_variance_device(ctx, p, d_moments, d_length, &dg, d_out, ctx->stream)) != OCTPT_OK)
            return st;
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "variance");
        return OCTPT_OK;
    });
}

octpt_status octpt_denoise_variance_device(octpt_ctx *ctx, const octpt_denoise_variance_params *p, const float *d_color,
                                           const float *d_variance, const octpt_aov_buffers *g, float *d_out,
                                           float *d_out_variance, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_denoise_variance(ctx, p, d_color, d_variance, g, d_out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "denoise_variance", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx))
            return forwarded(ctx, octpt_denoise_variance_device(ctx->sub[0], p, d_color, d_variance, g, d_out, d_out_variance,
                                                                stream));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height;
        // octpt_denoise_device's two frames and its rule: (s.rgb, v) lives in frame 0 after the prep pass, then
        // ping-pongs; the last iteration writes the caller's buffers.  A frame that has to grow may still be read by
        // an earlier call on another stream: drain first
        const bool two = p->iterations > 1u;
        if (needs_grow(n, ctx->dn_frame[0]) || (two && needs_grow(n, ctx->dn_frame[1]))) HIP_TRY(ctx, hipDeviceSynchronize());
        if ((st = grow_buf(ctx, ctx->dn_frame[0], n)) != OCTPT_OK) return st;
        if (two && (st = grow_buf(ctx, ctx->dn_frame[1], n)) != OCTPT_OK) return st;
        hipStream_t s = static_cast<hipStream_t>(stream);
        DevDenoiseVar D{};
        D.W = p->width;
        D.H = p->height;
        D.sigma_luminance = p->sigma_luminance;
        D.luminance_floor = p->luminance_floor;
        D.sn2 = p->sigma_normal * p->sigma_normal;
        D.sz2 = p->sigma_depth * p->sigma_depth;
        D.normal = reinterpret_cast<const float4 *>(g->normal);
        D.albedo = (p->flags & OCTPT_DENOISE_DEMODULATE) ? reinterpret_cast<const float4 *>(g->albedo) : nullptr;
        D.depth = g->depth;
        D.color = reinterpret_cast<const float4 *>(d_color);
        D.out = reinterpret_cast<float4 *>(d_out);
        D.out_variance = d_out_variance;
        HIP_TRY(ctx, launch_denoise_var_prep(D.W, D.H, D.color, d_variance, D.albedo, D.depth, ctx->dn_frame[0].p, s));
        for (uint32_t i = 0; i < p->iterations; ++i) {
            const bool last = i + 1u == p->iterations;
            HIP_TRY(ctx, launch_atrous_var(D, i, last, ctx->dn_frame[i & 1u].p,
                                           last ? nullptr : ctx->dn_frame[(i + 1u) & 1u].p, s));
        }
        return OCTPT_OK;
    });
}

octpt_status octpt_denoise_variance(octpt_ctx *ctx, const octpt_denoise_variance_params *p, const float *color,
                                    const float *variance, const octpt_aov_buffers *g, float *out, float *out_variance) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_denoise_variance(ctx, p, color, variance, g, out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "denoise_variance", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_denoise_variance(ctx->sub[0], p, color, variance, g, out, out_variance));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height;
        const bool demod = (p->flags & OCTPT_DENOISE_DEMODULATE) != 0u;
        HostStage hs(ctx->stream);
        float *d_color = hs.inout(color, out, 4 * n);  // both filtered in place on the device
        float *d_variance = hs.inout(variance, out_variance, n);
        float *d_normal = hs.in(g->normal, 4 * n), *d_depth = hs.in(g->depth, n);
        const octpt_aov_buffers dg{hs.in(demod ? g->albedo : nullptr, 4 * n), d_normal, d_depth, nullptr, nullptr};
        if (hs.ok() && (st = octpt_denoise_variance_device(ctx, p, d_color, d_variance, &dg, d_color,
                                                           out_variance ? d_variance : nullptr, ctx->stream)) != OCTPT_OK)
            return st;
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "denoise_variance");
        return OCTPT_OK;
    });
}

// ---------------- adaptive sampling: tile-list renders, sample moments, per-tile error ----------------
namespace {

// what a tile-list render refuses of the render parameters and the context (C30), before anything else is read
octpt_status check_tile_render(octpt_ctx *ctx, const char *who, const octpt_render_params *p) {
    const std::string w(who);
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, w + ": render params NULL");
    if (p->flags & (OCTPT_RENDER_MEGAKERNEL | OCTPT_RENDER_PREVIEW))
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, w + ": the wavefront path only (no megakernel, no preview)");
    if (is_multi(ctx)) return fail(ctx, OCTPT_ERR_UNSUPPORTED, w + ": not on a multi-device context");
    if (p->shard_count != 1u || p->shard_index != 0u || (p->flags & OCTPT_RENDER_SHARD_COMPACT))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, w + ": full frames of one shard only (shard_count 1, no compact layout)");
    if (!ctx->h_order.empty())
        return fail(ctx, OCTPT_ERR_INVALID_ARG, w + ": a tile order is set on the context (octpt_set_tile_order; NULL resets it)");
    return OCTPT_OK;
}

// octpt_render_tiles_device after its NULL checks
octpt_status render_tiles(octpt_ctx *ctx, const octpt_render_params *p, const uint32_t *tiles, uint32_t n_tiles,
                          float4 *d_accum, float2 *d_moments, uint32_t *d_seg, hipStream_t s) {
    octpt_status st = check_tile_render(ctx, "render_tiles", p);
    if (st != OCTPT_OK) return st;
    join_inflight(ctx);
    DevRender R{};
    if ((st = make_render(ctx, p, R)) != OCTPT_OK) return st;
    uint64_t list = 0;
    if (tiles) {
        const uint32_t T = R.tiles_x * ((R.H + kTile - 1) / kTile);
        if (n_tiles > T) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_tiles: more tiles than the frame has (a duplicate)");
        std::vector<uint8_t> seen(T, 0);
        for (uint32_t i = 0; i < n_tiles; ++i) {
            if (tiles[i] >= T) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_tiles: tile index outside the frame");
            if (seen[tiles[i]]) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_tiles: duplicate tile index");
            seen[tiles[i]] = 1;
        }
        if (n_tiles == 0 || p->spp_count == 0) return OCTPT_OK;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        // the list is the deal.  An earlier render on any stream may still read the table: drain before overwriting
        // it, as the branch schedule's and the tile order's tables do
        HIP_TRY(ctx, hipDeviceSynchronize());
        if ((st = grow_buf(ctx, ctx->d_tiles, (size_t)n_tiles)) != OCTPT_OK) return st;
        HIP_TRY(ctx, hipMemcpy(ctx->d_tiles.p, tiles, (size_t)n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice));
        R.tile_order = ctx->d_tiles.p;
        R.shard_tiles = n_tiles;
        R.total_items = n_tiles * 64u;
        R.div_items = udiv_magic(R.total_items);
        list = ++ctx->list_gen;
    }
    return enqueue_render(ctx, R, d_accum, d_seg, s, false, nullptr, d_moments, list);
}

octpt_status check_tile_error(octpt_ctx *ctx, const octpt_tile_error_params *p, const void *moments, const void *tile_spp,
                              const void *error) {
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "tile_error params NULL");
    if (p->width == 0 || p->height == 0 || (uint64_t)p->width * p->height >= (1ull << 31))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "tile_error: bad resolution");
    if (!(p->luminance_floor > 0.0f) || !std::isfinite(p->luminance_floor))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "tile_error: luminance_floor must be positive and finite");
    if (!moments || !tile_spp || !error)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "tile_error: NULL moments, tile_spp or error buffer");
    return OCTPT_OK;
}

}  // namespace

octpt_status octpt_render_tiles_device(octpt_ctx *ctx, const octpt_render_params *p, const uint32_t *tiles,
                                       uint32_t n_tiles, float *d_accum, float *d_moments, uint32_t *d_seg,
                                       void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!d_accum) return fail(ctx, OCTPT_ERR_INVALID_ARG, "d_accum NULL");
    return guarded(ctx, "render_tiles", [&]() -> octpt_status {
        return render_tiles(ctx, p, tiles, n_tiles, reinterpret_cast<float4 *>(d_accum),
                            reinterpret_cast<float2 *>(d_moments), d_seg, static_cast<hipStream_t>(stream));
    });
}

octpt_status octpt_tile_error_device(octpt_ctx *ctx, const octpt_tile_error_params *p, const float *d_moments,
                                     const uint32_t *d_tile_spp, float *d_error, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_tile_error(ctx, p, d_moments, d_tile_spp, d_error);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "tile_error", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx))
            return forwarded(ctx, octpt_tile_error_device(ctx->sub[0], p, d_moments, d_tile_spp, d_error, stream));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, launch_tile_error(p->width, p->height, p->luminance_floor, reinterpret_cast<const float2 *>(d_moments),
                                       d_tile_spp, d_error, static_cast<hipStream_t>(stream)));
        return OCTPT_OK;
    });
}

octpt_status octpt_tile_error(octpt_ctx *ctx, const octpt_tile_error_params *p, const float *moments,
                              const uint32_t *tile_spp, float *error) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_tile_error(ctx, p, moments, tile_spp, error);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "tile_error", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_tile_error(ctx->sub[0], p, moments, tile_spp, error));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height, T = frame_tiles(p->width, p->height);
        HostStage hs(ctx->stream);
        const float *d_moments = hs.in(moments, 2 * n);
        const uint32_t *d_tile_spp = hs.in(tile_spp, T);
        float *d_error = hs.out(error, T);
        if (hs.ok() && (st = octpt_tile_error_device(ctx, p, d_moments, d_tile_spp, d_error, ctx->stream)) != OCTPT_OK)
            return st;
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "tile_error");
        return OCTPT_OK;
    });
}

namespace {

// the plain driver's parameters as the _ex form's: neighbour weight 0, C32's loop
octpt_adaptive_params_ex adaptive_ex_of(const octpt_adaptive_params &a) {
    octpt_adaptive_params_ex x{};
    x.min_spp = a.min_spp;
    x.step_spp = a.step_spp;
    x.threshold = a.threshold;
    x.luminance_floor = a.luminance_floor;
    return x;
}

// what the adaptive drivers refuse of their parameters (C32, C34b) besides make_render's own refusals; buffers: whether
// the accum, moments and tile_spp pointers are all set
octpt_status check_adaptive(octpt_ctx *ctx, const octpt_render_params *p, const octpt_adaptive_params_ex *a, bool buffers) {
    octpt_status st = check_tile_render(ctx, "render_adaptive", p);
    if (st != OCTPT_OK) return st;
    if (!a) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_adaptive: adaptive params NULL");
    if (!buffers) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_adaptive: NULL accum, moments or tile_spp buffer");
    if (a->min_spp < 2u || a->step_spp < 1u)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_adaptive: min_spp must be >= 2 and step_spp >= 1");
    for (float x : {a->threshold, a->luminance_floor})
        if (!(x > 0.0f) || !std::isfinite(x))
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_adaptive: threshold and luminance_floor must be positive and finite");
    if (!(a->neighbour_weight >= 0.0f && a->neighbour_weight <= 1.0f))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_adaptive: neighbour_weight must be in [0, 1]");
    if (a->reserved[0] | a->reserved[1] | a->reserved[2])
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_adaptive: the reserved words must be 0");
    if (p->spp_start != 0u) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_adaptive: a fresh render (spp_start must be 0)");
    if (p->spp_count < a->min_spp)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_adaptive: spp_count (the per-pixel cap) must be >= min_spp");
    if (p->branch_count > 1u)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "render_adaptive: branch_count > 1 (its pass boundaries fix the round sizes)");
    return OCTPT_OK;
}

// the drivers' device form after the NULL-context check
octpt_status adaptive_device(octpt_ctx *ctx, const octpt_render_params *p, const octpt_adaptive_params_ex *a,
                             float *d_accum, float *d_moments, uint32_t *d_seg, uint32_t *tile_spp,
                             octpt_adaptive_result *result, void *stream) {
    octpt_status st = check_adaptive(ctx, p, a, d_accum && d_moments && tile_spp);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "render_adaptive", [&]() -> octpt_status {
        join_inflight(ctx);
        DevRender R{};
        if ((st = make_render(ctx, p, R)) != OCTPT_OK) return st;  // the remaining refusals, before the buffers are touched
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = static_cast<hipStream_t>(stream);
        const uint32_t T = frame_tiles(p->width, p->height), max_spp = p->spp_count;
        const bool spread = a->neighbour_weight != 0.0f;  // C34: the plane the host reads is the spread one
        // the tables below are rewritten every round, each time after the stream has drained; a call on another
        // stream ended with its own drain
        if ((st = grow_buf(ctx, ctx->d_tile_spp, (size_t)T)) != OCTPT_OK) return st;
        if ((st = grow_buf(ctx, ctx->d_tile_err, (size_t)T)) != OCTPT_OK) return st;
        if (spread && (st = grow_buf(ctx, ctx->d_tile_spread, (size_t)T)) != OCTPT_OK) return st;
        float4 *acc = reinterpret_cast<float4 *>(d_accum);
        float2 *mom = reinterpret_cast<float2 *>(d_moments);
        HIP_TRY(ctx, launch_adaptive_init(p->width * p->height, acc, mom, s));
        std::vector<uint32_t> active(T), next;
        std::vector<float> err(T, INFINITY);
        for (uint32_t t = 0; t < T; ++t) active[t] = t;
        std::fill(tile_spp, tile_spp + T, 0u);
        uint32_t n = 0, rounds = 0;
        while (!active.empty() && n < max_spp) {
            const uint32_t k = std::min(n == 0u ? a->min_spp : a->step_spp, max_spp - n);
            octpt_render_params q = *p;
            q.spp_start = n;
            q.spp_count = k;
            // round 1 is every tile in frame order: the plain deal (its beam starts serve the later lists)
            st = render_tiles(ctx, &q, n == 0u ? nullptr : active.data(), (uint32_t)active.size(), acc, mom, d_seg, s);
            if (st != OCTPT_OK) {
                (void)hipStreamSynchronize(s);
                return st;
            }
            n += k;
            for (uint32_t t : active) tile_spp[t] = n;
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_tile_spp.p, tile_spp, (size_t)T * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(ctx, launch_tile_error(p->width, p->height, a->luminance_floor, mom, ctx->d_tile_spp.p, ctx->d_tile_err.p, s));
            if (spread)
                HIP_TRY(ctx, launch_tile_error_spread(p->width, p->height, a->neighbour_weight, ctx->d_tile_err.p,
                                                      ctx->d_tile_spread.p, s));
            HIP_TRY(ctx, hipMemcpyAsync(err.data(), spread ? ctx->d_tile_spread.p : ctx->d_tile_err.p, (size_t)T * 4,
                                        hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            next.clear();
            for (uint32_t t : active)
                if (err[t] > a->threshold) next.push_back(t);
            active.swap(next);
            ++rounds;
        }
        if (result) {
            octpt_adaptive_result r{};
            r.rounds = rounds;
            r.total_tiles = T;
            for (uint32_t t = 0; t < T; ++t) {
                r.tile_samples += tile_spp[t];
                if (err[t] <= a->threshold) ++r.converged_tiles;
            }
            *result = r;
        }
        return OCTPT_OK;
    });
}

// the drivers' host form after the NULL-context check
octpt_status adaptive_host(octpt_ctx *ctx, const octpt_render_params *p, const octpt_adaptive_params_ex *a, float *accum,
                           float *moments, uint32_t *tile_spp, uint8_t *out_rgba8, octpt_adaptive_result *result) {
    octpt_status st = check_tile_render(ctx, "render_adaptive", p);
    if (st != OCTPT_OK) return st;
    if (!accum) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_adaptive: accum NULL");
    if (p->width == 0 || p->height == 0 || (uint64_t)p->width * p->height >= (1ull << 31))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "bad resolution");
    return guarded(ctx, "render_adaptive", [&]() -> octpt_status {
        join_inflight(ctx);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height;
        std::vector<uint32_t> spp(frame_tiles(p->width, p->height));
        HostStage hs(ctx->stream);
        float *d_accum = hs.out(accum, 4 * n), *d_moments = hs.scratch_out(moments, 2 * n);
        uint8_t *d_rgba8 = hs.out(out_rgba8, 4 * n);
        if (hs.ok() &&
            (st = adaptive_device(ctx, p, a, d_accum, d_moments, nullptr, spp.data(), result, ctx->stream)) != OCTPT_OK)
            return st;
        if (hs.ok() && out_rgba8)
            hs.note(launch_tonemap(reinterpret_cast<float4 *>(d_accum), reinterpret_cast<uchar4 *>(d_rgba8), (uint32_t)n,
                                   ctx->d_lut_byte, ctx->stream));
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "render_adaptive");
        if (tile_spp) std::copy(spp.begin(), spp.end(), tile_spp);
        return OCTPT_OK;
    });
}

}  // namespace

octpt_status octpt_render_adaptive_device(octpt_ctx *ctx, const octpt_render_params *p, const octpt_adaptive_params *a,
                                          float *d_accum, float *d_moments, uint32_t *d_seg, uint32_t *tile_spp,
                                          octpt_adaptive_result *result, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    const octpt_adaptive_params_ex x = a ? adaptive_ex_of(*a) : octpt_adaptive_params_ex{};
    return adaptive_device(ctx, p, a ? &x : nullptr, d_accum, d_moments, d_seg, tile_spp, result, stream);
}

octpt_status octpt_render_adaptive(octpt_ctx *ctx, const octpt_render_params *p, const octpt_adaptive_params *a,
                                   float *accum, float *moments, uint32_t *tile_spp, uint8_t *out_rgba8,
                                   octpt_adaptive_result *result) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    const octpt_adaptive_params_ex x = a ? adaptive_ex_of(*a) : octpt_adaptive_params_ex{};
    return adaptive_host(ctx, p, a ? &x : nullptr, accum, moments, tile_spp, out_rgba8, result);
}

octpt_status octpt_render_adaptive_ex_device(octpt_ctx *ctx, const octpt_render_params *p,
                                             const octpt_adaptive_params_ex *a, float *d_accum, float *d_moments,
                                             uint32_t *d_seg, uint32_t *tile_spp, octpt_adaptive_result *result,
                                             void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    return adaptive_device(ctx, p, a, d_accum, d_moments, d_seg, tile_spp, result, stream);
}

octpt_status octpt_render_adaptive_ex(octpt_ctx *ctx, const octpt_render_params *p, const octpt_adaptive_params_ex *a,
                                      float *accum, float *moments, uint32_t *tile_spp, uint8_t *out_rgba8,
                                      octpt_adaptive_result *result) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    return adaptive_host(ctx, p, a, accum, moments, tile_spp, out_rgba8, result);
}

// ---------------- final-quality adaptive frames: clamp, seam rule, sample variance, finished frame ----------------
octpt_status octpt_set_sample_clamp(octpt_ctx *ctx, float max_luminance) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!(max_luminance >= 0.0f)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sample clamp must be >= 0 (0 or +inf: off), not NaN");
    join_inflight(ctx);  // a frame in flight keeps the value its call was made with
    ctx->sample_clamp = std::isfinite(max_luminance) ? max_luminance : 0.0f;
    for (octpt_ctx *sc : ctx->sub) {
        const octpt_status st = octpt_set_sample_clamp(sc, max_luminance);
        if (st != OCTPT_OK) return fail(ctx, st, sc->err);
    }
    return OCTPT_OK;
}

namespace {

octpt_status check_spread(octpt_ctx *ctx, uint32_t W, uint32_t H, float w, const void *error, const void *out) {
    if (W == 0 || H == 0 || (uint64_t)W * H >= (1ull << 31)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "tile_error_spread: bad resolution");
    if (!(w >= 0.0f && w <= 1.0f)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "tile_error_spread: neighbour_weight must be in [0, 1]");
    if (!error || !out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "tile_error_spread: NULL error or output buffer");
    if (error == out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "tile_error_spread: the output must not be the input plane");
    return OCTPT_OK;
}

octpt_status check_sample_variance(octpt_ctx *ctx, const octpt_sample_variance_params *p, const void *moments,
                                   const void *tile_spp, const octpt_aov_buffers *g, const void *out) {
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sample_variance params NULL");
    if (p->width == 0 || p->height == 0 || (uint64_t)p->width * p->height >= (1ull << 31))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "sample_variance: bad resolution");
    if (p->flags & ~OCTPT_DENOISE_DEMODULATE)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "sample_variance: unknown flag (OCTPT_DENOISE_DEMODULATE is the one flag)");
    if (!moments || !tile_spp || !out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sample_variance: NULL moments, tile_spp or output buffer");
    if (!g || !g->depth) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sample_variance: the depth guide is required");
    const bool demod = (p->flags & OCTPT_DENOISE_DEMODULATE) != 0u;
    if (demod && !g->albedo) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sample_variance: OCTPT_DENOISE_DEMODULATE needs the albedo guide");
    if (out == moments || out == tile_spp || out == g->depth || (demod && out == g->albedo))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "sample_variance: the output must be distinct from the inputs");
    return OCTPT_OK;
}

}  // namespace

octpt_status octpt_tile_error_spread_device(octpt_ctx *ctx, uint32_t W, uint32_t H, float w, const float *d_error,
                                            float *d_out, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_spread(ctx, W, H, w, d_error, d_out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "tile_error_spread", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_tile_error_spread_device(ctx->sub[0], W, H, w, d_error, d_out, stream));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, launch_tile_error_spread(W, H, w, d_error, d_out, static_cast<hipStream_t>(stream)));
        return OCTPT_OK;
    });
}

octpt_status octpt_tile_error_spread(octpt_ctx *ctx, uint32_t W, uint32_t H, float w, const float *error, float *out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_spread(ctx, W, H, w, error, out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "tile_error_spread", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_tile_error_spread(ctx->sub[0], W, H, w, error, out));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t T = frame_tiles(W, H);
        HostStage hs(ctx->stream);
        const float *d_error = hs.in(error, T);
        float *d_out = hs.out(out, T);
        if (hs.ok() && (st = octpt_tile_error_spread_device(ctx, W, H, w, d_error, d_out, ctx->stream)) != OCTPT_OK) return st;
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "tile_error_spread");
        return OCTPT_OK;
    });
}

octpt_status octpt_sample_variance_device(octpt_ctx *ctx, const octpt_sample_variance_params *p, const float *d_moments,
                                          const uint32_t *d_tile_spp, const octpt_aov_buffers *g, float *d_out,
                                          void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_sample_variance(ctx, p, d_moments, d_tile_spp, g, d_out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "sample_variance", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx))
            return forwarded(ctx, octpt_sample_variance_device(ctx->sub[0], p, d_moments, d_tile_spp, g, d_out, stream));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const bool demod = (p->flags & OCTPT_DENOISE_DEMODULATE) != 0u;
        HIP_TRY(ctx, launch_sample_variance(p->width, p->height, reinterpret_cast<const float2 *>(d_moments), d_tile_spp,
                                            g->depth, demod ? reinterpret_cast<const float4 *>(g->albedo) : nullptr, d_out,
                                            static_cast<hipStream_t>(stream)));
        return OCTPT_OK;
    });
}

octpt_status octpt_sample_variance(octpt_ctx *ctx, const octpt_sample_variance_params *p, const float *moments,
                                   const uint32_t *tile_spp, const octpt_aov_buffers *g, float *out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_sample_variance(ctx, p, moments, tile_spp, g, out);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "sample_variance", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_sample_variance(ctx->sub[0], p, moments, tile_spp, g, out));
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height, T = frame_tiles(p->width, p->height);
        const bool demod = (p->flags & OCTPT_DENOISE_DEMODULATE) != 0u;
        HostStage hs(ctx->stream);
        const float *d_moments = hs.in(moments, 2 * n);
        const uint32_t *d_tile_spp = hs.in(tile_spp, T);
        float *d_depth = hs.in(g->depth, n);
        const octpt_aov_buffers dg{hs.in(demod ? g->albedo : nullptr, 4 * n), nullptr, d_depth, nullptr, nullptr};
        float *d_out = hs.out(out, n);
        if (hs.ok() && (st = octpt_sample_variance_device(ctx, p, d_moments, d_tile_spp, &dg, d_out, ctx->stream)) != OCTPT_OK)
            return st;
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "sample_variance");
        return OCTPT_OK;
    });
}

octpt_status octpt_render_final_device(octpt_ctx *ctx, const octpt_render_params *p, const octpt_final_params *f,
                                       float *d_accum, float *d_moments, float *d_out, float *d_out_variance,
                                       uint32_t *tile_spp, octpt_adaptive_result *result, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!f) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_final: final params NULL");
    // every refusal of the four steps, before any buffer is touched
    octpt_status st = check_adaptive(ctx, p, &f->adaptive, d_accum && d_moments && tile_spp);
    if (st != OCTPT_OK) return st;
    const bool demod = (f->filter.flags & OCTPT_DENOISE_DEMODULATE) != 0u;
    {
        // the filter's own checks of its parameters; its buffers are this call's and the context's planes
        const octpt_aov_buffers some{d_accum, d_accum, d_accum, nullptr, nullptr};
        if ((st = check_denoise_variance(ctx, &f->filter, d_accum, d_accum, &some, d_out)) != OCTPT_OK) return st;
    }
    if (f->filter.width != p->width || f->filter.height != p->height)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_final: the filter's width / height differ from the render's");
    if (d_out == d_accum) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_final: d_out must not alias d_accum");
    return guarded(ctx, "render_final", [&]() -> octpt_status {
        join_inflight(ctx);
        {
            DevRender R{};
            if ((st = make_render(ctx, p, R)) != OCTPT_OK) return st;
        }
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height, T = frame_tiles(p->width, p->height);
        // the context's planes, grow-only; one that has to grow may still be read by an earlier call on another
        // stream: drain first
        if (needs_grow(n, ctx->fin_normal, ctx->fin_depth, ctx->fin_var) || (demod && needs_grow(n, ctx->fin_albedo)) ||
            needs_grow(T, ctx->d_tile_spp))
            HIP_TRY(ctx, hipDeviceSynchronize());
        if ((st = grow_buf(ctx, ctx->fin_normal, n)) != OCTPT_OK) return st;
        if ((st = grow_buf(ctx, ctx->fin_depth, n)) != OCTPT_OK) return st;
        if ((st = grow_buf(ctx, ctx->fin_var, n)) != OCTPT_OK) return st;
        if (demod && (st = grow_buf(ctx, ctx->fin_albedo, n)) != OCTPT_OK) return st;
        // 1. the adaptive render; it leaves its final tile_spp in the context's device table
        if ((st = octpt_render_adaptive_ex_device(ctx, p, &f->adaptive, d_accum, d_moments, nullptr, tile_spp, result,
                                                  stream)) != OCTPT_OK)
            return st;
        // 2. the guides
        const octpt_aov_buffers g{demod ? reinterpret_cast<float *>(ctx->fin_albedo.p) : nullptr,
                                  reinterpret_cast<float *>(ctx->fin_normal.p), ctx->fin_depth.p, nullptr, nullptr};
        if ((st = octpt_render_aov_device(ctx, p, &g, stream)) != OCTPT_OK) return st;
        // 3. the variance of the pixel means
        const octpt_sample_variance_params vp{p->width, p->height, f->filter.flags & OCTPT_DENOISE_DEMODULATE};
        if ((st = octpt_sample_variance_device(ctx, &vp, d_moments, ctx->d_tile_spp.p, &g, ctx->fin_var.p, stream)) != OCTPT_OK)
            return st;
        // 4. the filter
        return octpt_denoise_variance_device(ctx, &f->filter, d_accum, ctx->fin_var.p, &g, d_out, d_out_variance, stream);
    });
}

octpt_status octpt_render_final(octpt_ctx *ctx, const octpt_render_params *p, const octpt_final_params *f, float *accum,
                                float *moments, float *out, float *out_variance, uint32_t *tile_spp, uint8_t *out_rgba8,
                                octpt_adaptive_result *result) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_tile_render(ctx, "render_final", p);
    if (st != OCTPT_OK) return st;
    if (!out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render_final: out NULL");
    if (p->width == 0 || p->height == 0 || (uint64_t)p->width * p->height >= (1ull << 31))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "bad resolution");
    return guarded(ctx, "render_final", [&]() -> octpt_status {
        join_inflight(ctx);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)p->width * p->height;
        std::vector<uint32_t> spp(frame_tiles(p->width, p->height));
        HostStage hs(ctx->stream);
        float *d_out = hs.out(out, 4 * n);
        float *d_accum = hs.scratch_out(accum, 4 * n), *d_moments = hs.scratch_out(moments, 2 * n);
        float *d_out_variance = hs.out(out_variance, n);
        uint8_t *d_rgba8 = hs.out(out_rgba8, 4 * n);
        if (hs.ok() && (st = octpt_render_final_device(ctx, p, f, d_accum, d_moments, d_out, d_out_variance, spp.data(), result,
                                                       ctx->stream)) != OCTPT_OK)
            return st;
        if (hs.ok() && out_rgba8)
            hs.note(launch_tonemap(reinterpret_cast<float4 *>(d_out), reinterpret_cast<uchar4 *>(d_rgba8), (uint32_t)n,
                                   ctx->d_lut_byte, ctx->stream));
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "render_final");
        if (tile_spp) std::copy(spp.begin(), spp.end(), tile_spp);
        return OCTPT_OK;
    });
}

}  // extern "C"
