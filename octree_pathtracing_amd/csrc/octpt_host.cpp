// Host-side queries of the C ABI that need no device: Octree::get_traversal_data and, at the end,
// the camera's pixel-centre rays (octpt_camera_rays) and the reprojection mapping (octpt_reproject_coords).
//
// get_traversal_data (octree_traversal.rs:537-714) is the reference's beam-start query: the
// host walks one ray (GPURenderer::render_frame uses the camera's centre ray,
// gpu_renderer.rs:579-581) down the octree to the first leaf and hands the octant it stopped
// in, its scale and the descent stack to the GPU as CameraUniform.traversal_start_idx / scale
// and the index/time stack buffers (gpu_renderer.rs:35-80).  It is one ray per frame, so it
// stays on the host, where the caller's octree already lives; the arithmetic is the ESVO
// setup and step of DESIGN.md §3 (the same float spec as the kernels: no contraction).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/octpt.h"
#include "octpt_lens.h"
#include "octpt_emitter.h"
#include "octpt_mask.h"
#include "octpt_reproject.h"
#include "octpt_sky.h"
#include "octpt_sky_sample.h"

namespace {
constexpr uint32_t kMaxScale = 23u;   // OCTREE_MAX_SCALE, octree_traversal.rs:14
constexpr uint32_t kMaxSteps = 1000u; // OCTREE_MAX_STEPS, :13
constexpr float kEpsilon = 1.1920929e-7f;  // OCTREE_EPSILON = 2^-23, :15

inline uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
// glam min_element / max_element on NaN-free t-values
inline float mn(float a, float b) { return a < b ? a : b; }
inline float mx(float a, float b) { return a > b ? a : b; }
}  // namespace

extern "C" octpt_status octpt_traversal_data(const octpt_octant *octants, uint32_t octant_count, uint32_t root,
                                             uint32_t depth, const float ray[6], float max_dst,
                                             uint32_t *start_octant, uint32_t *scale_out,
                                             uint32_t index_stack[24], float time_stack[24]) {
    if (!octants || !ray || !start_octant || !scale_out || !index_stack || !time_stack) return OCTPT_ERR_INVALID_ARG;
    if (root >= octant_count || depth < 1u || depth > 21u) return OCTPT_ERR_INVALID_ARG;
    for (int i = 0; i < 24; ++i) {  // Default::default() (:552)
        index_stack[i] = 0u;
        time_stack[i] = 0.0f;
    }
    const float octree_scale = std::ldexp(1.0f, -(int)depth);
    float ro[3], rd[3], t_coef[3], t_bias[3], pos[3] = {1.0f, 1.0f, 1.0f};
    for (int i = 0; i < 3; ++i) {
        ro[i] = ray[i] * octree_scale + 1.0f;  // :553, :559
        rd[i] = ray[3 + i];
        // :566-574 epsilon clamp; |rd| is taken after it ([C13], as the kernels)
        if (std::fabs(rd[i]) < kEpsilon) rd[i] = u2f((f2u(kEpsilon) & 0x7FFFFFFFu) | (f2u(rd[i]) & 0x80000000u));
        t_coef[i] = 1.0f / -std::fabs(rd[i]);
        t_bias[i] = t_coef[i] * ro[i];
    }
    const float max_d = max_dst * octree_scale;
    uint32_t mirror = 0u;
    for (int i = 0; i < 3; ++i)
        if (rd[i] > 0.0f) {  // :579-587
            mirror |= 1u << i;
            t_bias[i] = 3.0f * t_coef[i] - t_bias[i];
        }
    float t_min = mx(mx(mx(2.0f * t_coef[0] - t_bias[0], 2.0f * t_coef[1] - t_bias[1]), 2.0f * t_coef[2] - t_bias[2]),
                     0.0f);
    float t_max = mn(mn(t_coef[0] - t_bias[0], t_coef[1] - t_bias[1]), t_coef[2] - t_bias[2]);
    float h = t_max;
    uint32_t idx = 0u, parent = root, scale = kMaxScale - 1u;
    float scale_exp2 = 0.5f;
    for (int i = 0; i < 3; ++i)
        if (1.5f * t_coef[i] - t_bias[i] > t_min) {  // :597-606
            idx ^= 1u << i;
            pos[i] = 1.5f;
        }
    auto done = [&](uint32_t sc) {
        *start_octant = parent;
        *scale_out = sc;
        return OCTPT_OK;
    };
    for (uint32_t it = 0; it < kMaxSteps; ++it) {
        if (max_d >= 0.0f && t_min > max_d) return done(scale);  // :609-611
        float t_corner[3];
        for (int i = 0; i < 3; ++i) t_corner[i] = pos[i] * t_coef[i] - t_bias[i];
        const float tc_max = mn(mn(t_corner[0], t_corner[1]), t_corner[2]);
        const uint32_t cidx = idx ^ mirror;
        const uint32_t mask = octpt::normalized_mask(octants[parent].child_mask);  // C21
        const bool present = (mask >> cidx) & 1u, leaf = (mask >> (cidx + 8u)) & 1u;
        if (present && t_min <= t_max) {  // :622
            if (leaf && t_min > 0.0f) return done(scale);  // :623-625: the first leaf ends the walk
            const float half = scale_exp2 * 0.5f;
            const float tv_max = mn(t_max, tc_max);
            if (t_min <= tv_max && !leaf) {  // :633-651 descend
                const uint32_t child = octants[parent].children[cidx];
                if (child >= octant_count) return OCTPT_ERR_INVALID_ARG;
                if (tc_max < h) {
                    index_stack[scale] = parent;
                    time_stack[scale] = t_max;
                }
                h = tc_max;
                parent = child;
                scale -= 1u;
                scale_exp2 = half;
                idx = 0u;
                for (int i = 0; i < 3; ++i)
                    if (half * t_coef[i] + t_corner[i] > t_min) {
                        idx ^= 1u << i;
                        pos[i] += scale_exp2;
                    }
                t_max = tv_max;
                continue;
            }
        }
        uint32_t step_mask = 0u;  // :655-668 advance
        for (int i = 0; i < 3; ++i)
            if (t_corner[i] <= tc_max) {
                step_mask ^= 1u << i;
                pos[i] -= scale_exp2;
            }
        t_min = tc_max;
        idx ^= step_mask;
        if ((idx & step_mask) != 0u) {  // :670-711 pop
            uint32_t diff = 0u;
            for (int i = 0; i < 3; ++i)
                if (step_mask & (1u << i)) diff |= f2u(pos[i]) ^ f2u(pos[i] + scale_exp2);
            const uint32_t old_scale = scale;
            scale = diff ? 31u - (uint32_t)__builtin_clz(diff) : 0xFFFFFFFFu;  // util::find_msb_u32
            if (scale >= kMaxScale) return done(old_scale);
            scale_exp2 = u2f((scale - kMaxScale + 127u) << 23);
            parent = index_stack[scale];
            t_max = time_stack[scale];
            uint32_t sh[3];
            for (int i = 0; i < 3; ++i) {
                sh[i] = f2u(pos[i]) >> scale;
                pos[i] = u2f(sh[i] << scale);
            }
            idx = (sh[0] & 1u) | ((sh[1] & 1u) << 1) | ((sh[2] & 1u) << 2);
            h = 0.0f;
        }
    }
    return done(scale);
}

// Camera::get_ray (camera.rs:77-86) at the pixel centres: the camera basis as octpt_set_camera derives it
// (right = direction x up, d_factor = 1 / tan(fov / 2)) and the un-jittered ray as the preview and
// guide-buffer kernels form it -- the same f32 operations in the same order, no contraction -- so each ray
// is the device's ray for its pixel bit for bit.
extern "C" octpt_status octpt_camera_rays(const octpt_camera *camera, uint32_t width, uint32_t height, float *rays) {
    if (!camera || !rays || width == 0u || height == 0u) return OCTPT_ERR_INVALID_ARG;
    if ((uint64_t)width * height >= (1ull << 31)) return OCTPT_ERR_INVALID_ARG;
    if (!(camera->fov > 0.0f && camera->fov < 3.14159265f)) return OCTPT_ERR_INVALID_ARG;
    const float *dir = camera->direction, *up = camera->up;
    const float right[3] = {dir[1] * up[2] - up[1] * dir[2], dir[2] * up[0] - up[2] * dir[0],
                            dir[0] * up[1] - up[0] * dir[1]};  // camera.rs:80
    const float d_factor = 1.0f / tanf(camera->fov / 2.0f);    // camera.rs:79
    const float dim = (float)(width > height ? width : height);
    for (uint32_t y = 0; y < height; ++y) {
        const float yn = ((float)(2u * (height - y) - 1u) - (float)height) / dim;
        for (uint32_t x = 0; x < width; ++x) {
            const float xn = ((float)(2u * x + 1u) - (float)width) / dim;
            float nd[3];
            for (int i = 0; i < 3; ++i) nd[i] = (dir[i] * d_factor + right[i] * xn) + up[i] * yn;
            const float r = 1.0f / sqrtf((nd[0] * nd[0] + nd[1] * nd[1]) + nd[2] * nd[2]);
            float *o = rays + 6u * ((size_t)y * width + x);
            o[0] = camera->eye[0];
            o[1] = camera->eye[1];
            o[2] = camera->eye[2];
            o[3] = nd[0] * r;
            o[4] = nd[1] * r;
            o[5] = nd[2] * r;
        }
    }
    return OCTPT_OK;
}

// The first ray of sample `sample` of every pixel as a render of this size and seed forms it:
// csrc/octpt_lens.h's lens_ray, the text new_path compiles, over the whole frame; the direction guard of
// begin_segment after it, as every traced ray passes it.  Every check comes before the first write.
extern "C" octpt_status octpt_lens_rays(const octpt_camera *camera, uint32_t width, uint32_t height, uint32_t seed,
                                        uint32_t sample, float *rays) {
    if (!camera || !rays || width == 0u || height == 0u) return OCTPT_ERR_INVALID_ARG;
    if ((uint64_t)width * height >= (1ull << 31)) return OCTPT_ERR_INVALID_ARG;
    if (!(camera->fov > 0.0f && camera->fov < 3.14159265f)) return OCTPT_ERR_INVALID_ARG;
    if (!octpt::lens_fields_valid(camera->aperture, camera->focal_distance)) return OCTPT_ERR_INVALID_ARG;
    const octpt::LensCamera L = octpt::lens_camera(camera->eye, camera->direction, camera->up, camera->fov,
                                                   camera->aperture, camera->focal_distance);
    octpt::LensFrame F;
    F.W = width;
    F.H = height;
    F.seed = seed;
    F.dim = (float)(width > height ? width : height);  // make_render's dim, jlo and jhi
    F.jlo = -1.0f / F.dim;
    F.jhi = 1.0f / F.dim;
    const bool lens = L.aperture > 0.0f;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            float *o = rays + 6u * ((size_t)y * width + x), *d = o + 3;
            if (lens) (void)octpt::lens_ray<true>(L, F, x, y, sample, o, d);
            else (void)octpt::lens_ray<false>(L, F, x, y, sample, o, d);
            if ((d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) || std::isnan(d[0]) || std::isnan(d[1]) || std::isnan(d[2])) {
                d[0] = 0.0f;  // Scene::hit's direction guard (scene/mod.rs:175-179)
                d[1] = 1.0f;
                d[2] = 0.0f;
            }
        }
    return OCTPT_OK;
}

// The first ray under a projection for chosen samples: csrc/octpt_lens.h's projection_ray, the text
// the projected kernel instances compile; PINHOLE is lens_ray (octpt_lens_rays' text), with the centre flag
// octpt_camera_rays' text.  Every check comes before the first write.
extern "C" octpt_status octpt_projection_rays(const octpt_camera *camera, const octpt_projection *projection,
                                              uint32_t width, uint32_t height, uint32_t seed, const uint32_t *xys,
                                              uint32_t n, uint32_t flags, float *rays, uint32_t *rng_state) {
    if (!camera || !projection || !rays || (n != 0u && !xys) || width == 0u || height == 0u) return OCTPT_ERR_INVALID_ARG;
    if ((uint64_t)width * height >= (1ull << 31)) return OCTPT_ERR_INVALID_ARG;
    if (flags & ~OCTPT_PROJECTION_RAYS_CENTRE) return OCTPT_ERR_INVALID_ARG;
    if (!(camera->fov > 0.0f && camera->fov < 3.14159265f)) return OCTPT_ERR_INVALID_ARG;
    if (!octpt::lens_fields_valid(camera->aperture, camera->focal_distance)) return OCTPT_ERR_INVALID_ARG;
    if (!octpt::proj_mode_known(projection->mode)) return OCTPT_ERR_UNSUPPORTED;
    for (uint32_t r : projection->reserved)
        if (r != 0u) return OCTPT_ERR_INVALID_ARG;
    if (!octpt::proj_param_valid(projection->mode, projection->param)) return OCTPT_ERR_INVALID_ARG;
    const bool pinhole = projection->mode == OCTPT_PROJECTION_PINHOLE;
    if (!pinhole && camera->aperture > 0.0f) return OCTPT_ERR_UNSUPPORTED;
    for (uint32_t i = 0; i < n; ++i)
        if (xys[3u * i] >= width || xys[3u * i + 1u] >= height) return OCTPT_ERR_INVALID_ARG;
    const bool centre = (flags & OCTPT_PROJECTION_RAYS_CENTRE) != 0u;
    const octpt::LensCamera L = octpt::lens_camera(camera->eye, camera->direction, camera->up, camera->fov,
                                                   camera->aperture, camera->focal_distance);
    octpt::ProjCamera P;
    std::memcpy(P.eye, L.eye, 12);
    std::memcpy(P.dir, L.dir, 12);
    std::memcpy(P.right, L.right, 12);
    std::memcpy(P.up, L.up, 12);
    P.proj_mode = projection->mode;
    P.proj_half = projection->param * 0.5f;  // octpt_set_projection's product
    octpt::LensFrame F;
    F.W = width;
    F.H = height;
    F.seed = seed;
    F.dim = (float)(width > height ? width : height);  // make_render's dim, jlo and jhi
    F.jlo = -1.0f / F.dim;
    F.jhi = 1.0f / F.dim;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t x = xys[3u * i], y = xys[3u * i + 1u], sample = xys[3u * i + 2u];
        float *o = rays + 6u * (size_t)i, *d = o + 3;
        uint32_t st;
        if (pinhole && centre) {  // octpt_camera_rays' expressions (the preview's and the guide buffers' ray)
            const float xn = ((float)(2u * x + 1u) - (float)width) / F.dim;
            const float yn = ((float)(2u * (height - y) - 1u) - (float)height) / F.dim;
            float nd[3];
            for (int k = 0; k < 3; ++k) nd[k] = (L.dir[k] * L.d_factor + L.right[k] * xn) + L.up[k] * yn;
            const float r = 1.0f / sqrtf((nd[0] * nd[0] + nd[1] * nd[1]) + nd[2] * nd[2]);
            for (int k = 0; k < 3; ++k) {
                o[k] = L.eye[k];
                d[k] = nd[k] * r;
            }
            st = octpt::path_state(seed, y * width + x, sample);
        } else {
            if (pinhole) st = L.aperture > 0.0f ? octpt::lens_ray<true>(L, F, x, y, sample, o, d)
                                               : octpt::lens_ray<false>(L, F, x, y, sample, o, d);
            else st = centre ? octpt::projection_ray<false>(P, F, x, y, sample, o, d)
                             : octpt::projection_ray<true>(P, F, x, y, sample, o, d);
            if ((d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) || std::isnan(d[0]) || std::isnan(d[1]) || std::isnan(d[2])) {
                d[0] = 0.0f;  // Scene::hit's direction guard (scene/mod.rs:175-179), as octpt_lens_rays applies it
                d[1] = 1.0f;
                d[2] = 0.0f;
            }
        }
        if (rng_state) rng_state[i] = st;
    }
    return OCTPT_OK;
}

// The first ray under a ray source for chosen samples: csrc/octpt_lens.h's ray_list_ray, the text the
// ray-list kernel instances compile, over a host copy of the list.  Every check comes before the first write.
extern "C" octpt_status octpt_ray_source_rays(const octpt_camera *fallback, const float *rays, uint32_t width,
                                              uint32_t height, uint32_t rays_per_pixel, uint32_t seed, const uint32_t *xys,
                                              uint32_t n, float *out_rays, uint32_t *rng_state) {
    if (!fallback || !rays || !out_rays || (n != 0u && !xys)) return OCTPT_ERR_INVALID_ARG;
    if (width == 0u || height == 0u || rays_per_pixel == 0u) return OCTPT_ERR_INVALID_ARG;
    const uint64_t px = (uint64_t)width * height;
    if (px > octpt::kRayListMaxRays || rays_per_pixel > octpt::kRayListMaxRays / px) return OCTPT_ERR_INVALID_ARG;
    if (!(fallback->fov > 0.0f && fallback->fov < 3.14159265f)) return OCTPT_ERR_INVALID_ARG;
    if (!octpt::lens_fields_valid(fallback->aperture, fallback->focal_distance)) return OCTPT_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (xys[3u * i] >= width || xys[3u * i + 1u] >= height) return OCTPT_ERR_INVALID_ARG;
    const octpt::LensCamera L = octpt::lens_camera(fallback->eye, fallback->direction, fallback->up, fallback->fov,
                                                   fallback->aperture, fallback->focal_distance);
    octpt::LensFrame F;
    F.W = width;
    F.H = height;
    F.seed = seed;
    F.dim = (float)(width > height ? width : height);  // make_render's dim, jlo and jhi (not read by this form)
    F.jlo = -1.0f / F.dim;
    F.jhi = 1.0f / F.dim;
    for (uint32_t i = 0; i < n; ++i) {
        float *o = out_rays + 6u * (size_t)i;
        const uint32_t st = octpt::ray_list_ray<true>(L, F, rays, rays_per_pixel, xys[3u * i], xys[3u * i + 1u],
                                                      xys[3u * i + 2u], o, o + 3);
        if (rng_state) rng_state[i] = st;
    }
    return OCTPT_OK;
}

// The sky's colour for n directions: csrc/octpt_sky.h's sky_radiance, the text the sky instances of
// shade, the drain and the preview compile, over a sanitised host copy of the map.  Every check comes before the
// first write.
namespace {
octpt_status host_sky(const octpt_sky *sky, const float *texels, octpt::Sky &K, std::vector<float> &map) {
    if (!sky) return OCTPT_ERR_INVALID_ARG;
    for (uint32_t w : sky->reserved)
        if (w != 0u) return OCTPT_ERR_INVALID_ARG;
    if (!octpt::sky_mode_known(sky->mode)) return OCTPT_ERR_INVALID_ARG;
    if (!octpt::sky_fields_valid(sky->mode, sky->scale, sky->yaw, sky->width, sky->height, texels != nullptr))
        return OCTPT_ERR_INVALID_ARG;
    K = octpt::Sky{};
    K.mode = sky->mode;
    if (sky->mode == OCTPT_SKY_DEFAULT) return OCTPT_OK;
    std::memcpy(K.color, sky->color, 12);
    std::memcpy(K.horizon, sky->horizon, 12);
    std::memcpy(K.zenith, sky->zenith, 12);
    K.scale = sky->scale;
    K.yaw = sky->yaw;
    if (sky->mode == OCTPT_SKY_MAP) {
        const size_t n = (size_t)sky->width * sky->height * 4u;
        try {
            map.resize(n);
        } catch (const std::bad_alloc &) {
            return OCTPT_ERR_OOM;
        }
        for (size_t i = 0; i < n; ++i) map[i] = octpt::sky_sanitise(texels[i]);
        K.width = sky->width;
        K.height = sky->height;
        K.texels = map.data();
    }
    return OCTPT_OK;
}
}  // namespace

extern "C" octpt_status octpt_sky_radiance(const octpt_sky *sky, const float *texels, const float *dirs, uint32_t n,
                                           float *out) {
    if (n != 0u && (!dirs || !out)) return OCTPT_ERR_INVALID_ARG;
    octpt::Sky K;
    std::vector<float> map;
    const octpt_status st = host_sky(sky, texels, K, map);
    if (st != OCTPT_OK) return st;
    for (uint32_t i = 0; i < n; ++i) octpt::sky_radiance(K, dirs + 3u * (size_t)i, out + 3u * (size_t)i);
    return OCTPT_OK;
}

// ... and a MAP's lookup position alone, in texels (sky_map_position): what the bound of the lookup's error is
// measured from
extern "C" octpt_status octpt_sky_map_position(const octpt_sky *sky, const float *dirs, uint32_t n, float *out_xy) {
    if (n != 0u && (!dirs || !out_xy)) return OCTPT_ERR_INVALID_ARG;
    if (!sky || sky->mode != OCTPT_SKY_MAP) return OCTPT_ERR_INVALID_ARG;
    if (!octpt::sky_fields_valid(sky->mode, sky->scale, sky->yaw, sky->width, sky->height, true))
        return OCTPT_ERR_INVALID_ARG;
    octpt::Sky K{};
    K.mode = sky->mode;
    K.yaw = sky->yaw;
    K.width = sky->width;
    K.height = sky->height;
    for (uint32_t i = 0; i < n; ++i)
        octpt::sky_map_position(K, dirs + 3u * (size_t)i, out_xy[2u * (size_t)i], out_xy[2u * (size_t)i + 1u]);
    return OCTPT_OK;
}

// The sky map's distribution: csrc/octpt_sky_sample.h's weight and quantum over a sanitised host copy of
// the map, summed in integers.  The definition the device builder (octpt_build.hip) is compared with.
extern "C" octpt_status octpt_build_sky_distribution(const float *texels, uint32_t width, uint32_t height,
                                                     uint64_t *row_cdf, uint32_t *col_cdf) {
    if (!texels || !row_cdf || !col_cdf) return OCTPT_ERR_INVALID_ARG;
    if (width == 0u || height == 0u || (uint64_t)width * height > octpt::kSkyMaxTexels) return OCTPT_ERR_INVALID_ARG;
    if (width > octpt::kSkySampleMaxWidth) return OCTPT_ERR_UNSUPPORTED;
    const size_t n = (size_t)width * height;
    std::vector<float> map, w;
    try {
        map.resize(n * 4u);
        w.resize(n);
    } catch (const std::bad_alloc &) {
        return OCTPT_ERR_OOM;
    }
    for (size_t i = 0; i < n * 4u; ++i) map[i] = octpt::sky_sanitise(texels[i]);
    octpt::Sky K{};
    K.mode = octpt::kSkyMap;
    K.width = width;
    K.height = height;
    K.texels = map.data();
    float wmax = 0.0f;
    for (uint32_t y = 0; y < height; ++y) {
        const float row = octpt::sky_row_factor(y, height);
        for (uint32_t x = 0; x < width; ++x) {
            const float v = octpt::sky_weight(K, x, y, row);
            w[(size_t)y * width + x] = v;
            wmax = v > wmax ? v : wmax;
        }
    }
    uint64_t total = 0;
    for (uint32_t y = 0; y < height; ++y) {
        uint32_t sum = 0;
        for (uint32_t x = 0; x < width; ++x) {
            sum += octpt::sky_quantise(w[(size_t)y * width + x], wmax);
            col_cdf[(size_t)y * width + x] = sum;
        }
        total += sum;
        row_cdf[y] = total;
    }
    return OCTPT_OK;
}

// ... and its sample for n tuples of draws: sky_sample_draws, the text the sky-sampling instances of shade compile
extern "C" octpt_status octpt_sky_sample(const octpt_sky_distribution_arrays *dist, const octpt_sky *sky, uint32_t n,
                                         const float *u, float *out) {
    if (!dist || !sky || (n != 0u && (!u || !out))) return OCTPT_ERR_INVALID_ARG;
    if (sky->mode != OCTPT_SKY_MAP || !dist->row_cdf || !dist->col_cdf) return OCTPT_ERR_INVALID_ARG;
    if (!octpt::sky_fields_valid(sky->mode, sky->scale, sky->yaw, sky->width, sky->height, true))
        return OCTPT_ERR_INVALID_ARG;
    if (sky->width > octpt::kSkySampleMaxWidth) return OCTPT_ERR_UNSUPPORTED;
    if (dist->width != sky->width || dist->height != sky->height || dist->row_cdf_capacity < sky->height ||
        dist->col_cdf_capacity < (uint64_t)sky->width * sky->height)
        return OCTPT_ERR_INVALID_ARG;
    octpt::Sky K{};
    K.mode = sky->mode;
    K.yaw = sky->yaw;
    K.width = sky->width;
    K.height = sky->height;
    const octpt::SkyDist D{dist->row_cdf, dist->col_cdf, dist->row_cdf[sky->height - 1u]};
    for (uint32_t i = 0; i < n; ++i) {
        octpt::SkyShot s;
        const bool ok = octpt::sky_sample_draws(D, K, u + 4u * (size_t)i, s);
        octpt::sky_sample_pack(s, ok, out + 8u * (size_t)i);
    }
    return OCTPT_OK;
}

// The mapping of DESIGN.md C26 alone: csrc/octpt_reproject.h's reproject_pixel, the text temporal_kernel compiles,
// over the whole frame.
extern "C" octpt_status octpt_reproject_coords(const octpt_camera *camera, const octpt_camera *prev_camera, uint32_t width,
                                               uint32_t height, const float *depth, float *prev_xy, float *prev_depth) {
    if (!camera || !prev_camera || !depth || !prev_xy || !prev_depth) return OCTPT_ERR_INVALID_ARG;
    if (width == 0u || height == 0u || (uint64_t)width * height >= (1ull << 31)) return OCTPT_ERR_INVALID_ARG;
    const char *why = nullptr;
    const octpt_status st = octpt::check_reproject_cameras(camera, prev_camera, &why);
    if (st != OCTPT_OK) return st;
    const octpt::CameraBasis cur = octpt::camera_basis(camera->eye, camera->direction, camera->up, camera->fov);
    const octpt::CameraBasis prev =
        octpt::camera_basis(prev_camera->eye, prev_camera->direction, prev_camera->up, prev_camera->fov);
    const float dim = (float)(width > height ? width : height);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            float fx = NAN, fy = NAN, zp = INFINITY;
            const float z = depth[p];
            if (std::fabs(z) < INFINITY) (void)octpt::reproject_pixel(cur, prev, x, y, width, height, dim, z, fx, fy, zp);
            prev_xy[2u * p] = fx;
            prev_xy[2u * p + 1u] = fy;
            prev_depth[p] = zp;
        }
    return OCTPT_OK;
}

// csrc/octpt_emitter.h's emitter_sample, the text shade_segment's emitter instances compile, for one hit
extern "C" octpt_status octpt_emitter_sample(const octpt_emitter_grid_arrays *grid, uint32_t depth, uint32_t grid_size,
                                             const float hit[3], const float normal[3], uint32_t rng_state,
                                             float out[8], uint32_t *emitter, uint32_t *list_length) {
    uint32_t quad = 0u;
    return octpt_emitter_sample_models(grid, nullptr, nullptr, 0u, depth, grid_size, hit, normal, rng_state, out, emitter,
                                       list_length, &quad);
}

// ... with the emissive-model table (C39); table NULL: a grid of cube emitters, sampled without the flag
extern "C" octpt_status octpt_emitter_sample_models(const octpt_emitter_grid_arrays *grid,
                                                    const octpt_emitter_model_arrays *table, const octpt_quad *quads,
                                                    uint32_t quad_count, uint32_t depth, uint32_t grid_size,
                                                    const float hit[3], const float normal[3], uint32_t rng_state,
                                                    float out[8], uint32_t *emitter, uint32_t *list_length,
                                                    uint32_t *quad) {
    if (!grid || !hit || !normal || !out || !emitter || !list_length || !quad) return OCTPT_ERR_INVALID_ARG;
    if (!grid->cell_first || !grid->cell_emitters || !grid->emitters) return OCTPT_ERR_INVALID_ARG;
    if (depth < 1 || depth > 21 || grid_size == 0u || (grid_size & (grid_size - 1u)) || grid_size > (1u << depth))
        return OCTPT_ERR_INVALID_ARG;
    uint32_t shift = 0;
    while ((1u << shift) < grid_size) ++shift;
    if (grid->cells_per_axis != (1u << (depth - shift))) return OCTPT_ERR_INVALID_ARG;
    octpt::EmitGrid G{grid->cell_first, grid->cell_emitters, grid->emitters, shift, depth - shift, 1u << depth, 1.0f,
                      0u, 0u, nullptr, nullptr, nullptr, nullptr};
    std::vector<float> ouv;
    if (table) {
        if (!table->model_first || !table->quad_index || !table->cum_area || (quad_count && !quads))
            return OCTPT_ERR_INVALID_ARG;
        if (table->model_first[table->model_count] != table->entry_count) return OCTPT_ERR_INVALID_ARG;
        // every model record of the grid names a model of the table that has entries
        for (uint32_t k = 0; k < grid->emitter_count; ++k) {
            const uint32_t w = grid->emitters[k].s;
            if (!(w & octpt::kEmitModelBit)) continue;
            const uint32_t m = w & ~octpt::kEmitModelBit;
            if (m >= table->model_count || table->model_first[m + 1u] <= table->model_first[m] ||
                table->model_first[m + 1u] > table->entry_count)
                return OCTPT_ERR_INVALID_ARG;
        }
        try {
            ouv.resize((size_t)table->entry_count * 9u);
        } catch (const std::bad_alloc &) {
            return OCTPT_ERR_OOM;
        }
        for (uint32_t i = 0; i < table->entry_count; ++i) {
            const uint32_t q = table->quad_index[i];
            if (q >= quad_count) return OCTPT_ERR_INVALID_ARG;
            for (int c = 0; c < 3; ++c) {
                ouv[9u * i + c] = quads[q].origin[c];
                ouv[9u * i + 3 + c] = quads[q].u[c];
                ouv[9u * i + 6 + c] = quads[q].v[c];
            }
        }
        G.flags = OCTPT_EMITTERS_MODELS;
        G.model_first = table->model_first;
        G.quad_index = table->quad_index;
        G.cum_area = table->cum_area;
        G.quad_ouv = ouv.data();
    }
    octpt::EmitShot s{};
    const bool traced = octpt::emitter_sample(G, hit, normal, rng_state, s);
    *list_length = s.K;
    *emitter = traced ? s.emitter : 0xFFFFFFFFu;
    *quad = traced ? s.quad : 0xFFFFFFFFu;
    for (int i = 0; i < 3; ++i) {
        out[i] = s.p[i];
        out[3 + i] = traced ? s.dir[i] : 0.0f;
    }
    out[6] = traced ? s.dist : 0.0f;
    out[7] = traced ? s.geom : 0.0f;
    return OCTPT_OK;
}
