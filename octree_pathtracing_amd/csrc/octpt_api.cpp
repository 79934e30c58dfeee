// octpt_api.cpp -- host side of the octpt C ABI (include/octpt.h).
//
// Replaces the reference's wgpu backend (src/renderer/gpu_renderer.rs:151-702): scene
// validation + upload (set_scene / create_pipeline), camera uniform construction
// (render_frame :590-599), progressive render submission, FrameInFlight polling, and the
// device octree and scene build entries.  The host builders are in octpt_build_host.cpp, the
// post-processing entries (guide buffers, denoisers, temporal passes, variance, adaptive and final
// frames) in octpt_post.cpp; octpt_ctx.h holds the context and what the two files share.
// No CPU rendering path exists here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <thread>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <memory>
#include <vector>

#include "octpt_ctx.h"
#include "octpt_lens.h"
#include "octpt_mask.h"
#include "octpt_stage.h"

using namespace octpt;

namespace {

// log2 of the largest G in {1, 4, 16, 64} that is at most `most` and divides the chunk's sample count
uint32_t group_shift_of(uint32_t most, uint32_t chunk_spp) {
    uint32_t g = 6u;
    while (g && ((1u << g) > most || chunk_spp % (1u << g) != 0u)) g -= 2u;
    return g;
}

uint32_t env_u32(const char *name, uint32_t dflt) {
    const char *v = std::getenv(name);
    if (!v || !*v) return dflt;
    const long x = std::strtol(v, nullptr, 10);
    return x > 0 ? (uint32_t)x : dflt;
}

// colour LUTs (texture.rs:42-62), computed with the host libm like the reference
void make_luts(float lut_float[256], uint8_t lut_byte[256]) {
    for (int i = 0; i < 256; ++i) {
        lut_float[i] = powf((float)i / 255.0f, 2.2f);
        const float b = powf((float)i / 255.0f, 1.0f / 2.2f) * 255.0f;
        lut_byte[i] = (uint8_t)(b > 0.0f ? (b >= 255.0f ? 255u : (uint32_t)b) : 0u);
    }
}

// glam-order f32 helpers for the host-side uniforms
inline float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
inline void cross3(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - b[1] * a[2];
    o[1] = a[2] * b[0] - b[2] * a[0];
    o[2] = a[0] * b[1] - b[0] * a[1];
}

// Sun::new (scene/mod.rs:321-383) + diffuse_reflection sun constants (ray/mod.rs:228-259)
void make_sun(const octpt_sun &p, const float lut_float[256], DevSun &k) {
    const float theta = p.azimuth, phi = p.altitude;
    const float r = fabsf(cosf(phi));
    float sw[3] = {cosf(theta) * r, sinf(phi), sinf(theta) * r};
    float su[3] = {0.0f, 0.0f, 0.0f};
    if (fabsf(sw[0]) > 0.1f) su[1] = 1.0f; else su[0] = 1.0f;
    float sv[3];
    cross3(sw, su, sv);
    const float inv = 1.0f / sqrtf(dot3(sv, sv));
    for (float &c : sv) c = c * inv;
    cross3(sv, sw, su);
    std::memcpy(k.sw, sw, sizeof sw);
    std::memcpy(k.su, su, sizeof su);
    std::memcpy(k.sv, sv, sizeof sv);
    k.width = p.radius * 4.0f;
    k.width2 = k.width * 2.0f;
    const float gamma_b = powf(1.25f, 2.2f);
    k.tex[0] = lut_float[p.texture_rgba[0]];
    k.tex[1] = lut_float[p.texture_rgba[1]];
    k.tex[2] = lut_float[p.texture_rgba[2]];
    k.tex[3] = (float)p.texture_rgba[3] / 255.0f;
    for (int i = 0; i < 3; ++i) {
        const float atb = (p.texture_modification ? p.apparent_color[i] : 1.0f) * gamma_b;
        k.isect_mul[i] = atb * 10.0f;
        k.diffuse_mul[i] = p.color[i] * 10.0f;
        k.emit[i] = p.color[i] * gamma_b;
    }
    k.luminosity = p.luminosity;
    const float pi = 3.14159265358979323846f;
    const float az = p.azimuth, alt_fake = p.altitude;
    const float sgn = std::signbit(alt_fake) ? -1.0f : 1.0f;
    const float alt = fabsf(alt_fake) > pi / 2.0f ? sgn * pi - alt_fake : alt_fake;
    k.sun_dx = cosf(az) * cosf(alt);
    k.sun_dz = sinf(az) * cosf(alt);
    k.sun_dy = sinf(alt);
    k.circle_radius = p.radius * p.importance_sample_radius;
    k.sample_chance = p.importance_sample_chance;
    k.draw_texture = p.draw_texture ? 1 : 0;
    k.importance_sampling = p.importance_sampling ? 1 : 0;
    k.diffuse_sun = p.diffuse_sun ? 1 : 0;
    k.sun_sampling = p.sun_sampling ? 1 : 0;
    k.strict_direct_light = p.strict_direct_light ? 1 : 0;
    k.lum_a = p.sun_luminosity ? p.luminosity_pdf : 1.0f;  // path_tracer.rs:250-254
    k.radius_cos = cosf(p.radius);                          // Sun::new (scene/mod.rs:331)
}

// the emitter grid of the scene (C38)
void drop_emitter_grid(octpt_ctx *ctx) {
    if (ctx->emit_grid.cell_first) (void)hipFree(ctx->emit_grid.cell_first);
    if (ctx->emit_grid.cell_emitters) (void)hipFree(ctx->emit_grid.cell_emitters);
    if (ctx->emit_grid.emitters) (void)hipFree(ctx->emit_grid.emitters);
    ctx->emit_grid = DeviceEmitterGrid{};
    ctx->grid_valid = false;
}

void free_scene(octpt_ctx *ctx) {
    drop_emitter_grid(ctx);
    for (void *p : ctx->scene_allocs) (void)hipFree(p);
    ctx->scene_allocs.clear();
    ctx->d_model_first = ctx->d_model_quad = nullptr;
    ctx->d_model_cum = ctx->d_model_ouv = nullptr;
    ctx->has_scene = false;
}

template <class T>
hipError_t upload(octpt_ctx *ctx, const T *src, size_t n, T **dst) {
    *dst = nullptr;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    ctx->scene_allocs.push_back(p);
    if (n && src) {
        e = hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
    } else {
        e = hipMemset(p, 0, bytes);
        if (e != hipSuccess) return e;
        // hipMemset runs on the null stream, which does not order itself with the context's non-blocking stream:
        // the kernels that fill these tables on ctx->stream (fill_scene_gpu) must not race it
        e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return e;
    }
    *dst = static_cast<T *>(p);
    return hipSuccess;
}

// memoised subtree height with cycle detection; returns -1 on a cycle or bad index.
// masks: the octants' child masks in the reader form (normalized_mask, C21)
int subtree_height(const octpt_scene_desc &d, const std::vector<uint16_t> &masks, uint32_t node, std::vector<int8_t> &h,
                   int level) {
    if (level > (int)kMaxDepth + 1) return -1;
    if (h[node] == -2) return -1;  // on the current DFS path: cycle
    if (h[node] >= 0) return h[node];
    h[node] = -2;
    int best = 1;
    const uint32_t m = masks[node];
    for (int i = 0; i < 8; ++i) {
        const bool present = (m >> i) & 1, leaf = (m >> (i + 8)) & 1;
        if (!present || leaf) continue;
        const int ch = subtree_height(d, masks, d.octants[node].children[i], h, level + 1);
        if (ch < 0) return -1;
        best = std::max(best, ch + 1);
    }
    h[node] = (int8_t)best;
    return best;
}

// Quad::new (quad.rs:90-114): n = u x v, normal = n * (1 / |n|), w = n / (n . n), d = normal . origin
DevQuad make_dev_quad(const octpt_quad &x) {
    const float *u = x.u, *v = x.v, *o = x.origin;
    const float n[3] = {u[1] * v[2] - v[1] * u[2], u[2] * v[0] - v[2] * u[0], u[0] * v[1] - v[0] * u[1]};
    const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const float r = 1.0f / sqrtf(nn);
    const float nrm[3] = {n[0] * r, n[1] * r, n[2] * r};
    const float dd = (nrm[0] * o[0] + nrm[1] * o[1]) + nrm[2] * o[2];
    DevQuad q{};
    uint32_t mb;
    std::memcpy(&mb, &x.material, 4);
    float mat;
    std::memcpy(&mat, &mb, 4);
    q.o_d = make_float4(o[0], o[1], o[2], dd);
    q.u_mat = make_float4(u[0], u[1], u[2], mat);
    q.v_tu0 = make_float4(v[0], v[1], v[2], x.texture_u_range[0]);
    q.w_tu1 = make_float4(n[0] / nn, n[1] / nn, n[2] / nn, x.texture_u_range[1]);
    q.n_tv0 = make_float4(nrm[0], nrm[1], nrm[2], x.texture_v_range[0]);
    q.tv1 = make_float4(x.texture_v_range[1], 0.0f, 0.0f, 0.0f);
    return q;
}

octpt_status validate_tables(octpt_ctx *ctx, const octpt_scene_desc *d);

// the checks that precede the octree's: version, depth, non-empty tables, primitive pointers.
// with_octree = false (octpt_scene_build_device, octpt_scene_build_blocks_device): the octree fields must be
// NULL / 0; which of the two a block table belongs to is the entries' own check
octpt_status validate_head(octpt_ctx *ctx, const octpt_scene_desc *d, bool with_octree) {
    if (!d) return fail(ctx, OCTPT_ERR_INVALID_ARG, "scene is NULL");
    if (d->abi_version != OCTPT_ABI_VERSION) return fail(ctx, OCTPT_ERR_INVALID_ARG, "scene abi_version mismatch");
    if (d->depth < 1 || d->depth > kMaxDepth) return fail(ctx, OCTPT_ERR_INVALID_ARG, "octree depth must be in [1, 21]");
    if (with_octree) {
        if (!d->octants || d->octant_count == 0 || d->root >= d->octant_count)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "octree has no root octant");
    } else if (d->octants || d->octant_count || d->root || d->leaf_first || d->leaf_count || d->leaf_table_size ||
               d->leaf_prims || d->leaf_prim_count) {
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "the device build makes the octree: its scene fields must be NULL / 0");
    }
    if (d->material_count == 0 || !d->materials) return fail(ctx, OCTPT_ERR_INVALID_ARG, "material table is empty");
    if (d->texture_count == 0 || !d->textures) return fail(ctx, OCTPT_ERR_INVALID_ARG, "texture table is empty");
    if (d->leaf_table_size && (!d->leaf_first || !d->leaf_count))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "leaf table pointers are NULL");
    if (d->leaf_prim_count && !d->leaf_prims) return fail(ctx, OCTPT_ERR_INVALID_ARG, "leaf_prims is NULL");
    if (d->sphere_count > kPrimIndexMask || d->cuboid_count > kPrimIndexMask)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "more than 2^27 - 1 spheres or cuboids");
    if (d->sphere_count && !d->spheres) return fail(ctx, OCTPT_ERR_INVALID_ARG, "spheres is NULL");
    if (d->cuboid_count && !d->cuboids) return fail(ctx, OCTPT_ERR_INVALID_ARG, "cuboids is NULL");
    if (d->blocks) {  // block-value leaves (C23): the payloads are block ids, there are no primitives
        if (d->block_count == 0) return fail(ctx, OCTPT_ERR_INVALID_ARG, "block table is empty");
        if (d->block_count > kPrimIndexMask + 1u) return fail(ctx, OCTPT_ERR_UNSUPPORTED, "more than 2^27 blocks");
        if (d->leaf_first || d->leaf_count || d->leaf_table_size || d->leaf_prims || d->leaf_prim_count ||
            d->sphere_count || d->cuboid_count || d->cuboid_model)
            return fail(ctx, OCTPT_ERR_INVALID_ARG,
                        "a block-value scene has no leaf primitive lists, spheres, cuboids or cuboid models");
    } else if (d->block_count) {
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "block_count without blocks");
    }
    return OCTPT_OK;
}

// masks (out): every octant's child mask in the reader form (C21)
octpt_status validate_scene(octpt_ctx *ctx, const octpt_scene_desc *d, std::vector<uint16_t> &masks) {
    octpt_status st = validate_head(ctx, d, true);
    if (st != OCTPT_OK) return st;
    // both octant encodings are accepted (C21): (present, leaf bit) = (1,0) or set_mask_for's (0,1)
    masks.resize(d->octant_count);
    for (uint32_t n = 0; n < d->octant_count; ++n) {
        const octpt_octant &o = d->octants[n];
        const uint32_t m = masks[n] = normalized_mask(o.child_mask);
        for (int i = 0; i < 8; ++i) {
            const bool present = (m >> i) & 1, leaf = (m >> (i + 8)) & 1;
            if (!present) continue;
            if (leaf && o.children[i] >= (d->blocks ? d->block_count : d->leaf_table_size))
                return fail(ctx, OCTPT_ERR_INVALID_ARG, "octant " + std::to_string(n) + " child " + std::to_string(i) +
                                                            (d->blocks ? ": block " : ": leaf payload ") +
                                                            std::to_string(o.children[i]) + " out of range");
            if (!leaf && o.children[i] >= d->octant_count)
                return fail(ctx, OCTPT_ERR_INVALID_ARG, "octant " + std::to_string(n) + " child " + std::to_string(i) +
                                                            ": child octant index " + std::to_string(o.children[i]) +
                                                            " out of range");
        }
    }
    std::vector<int8_t> h(d->octant_count, -1);
    const int height = subtree_height(*d, masks, d->root, h, 0);
    if (height < 0) return fail(ctx, OCTPT_ERR_INVALID_ARG, "octree contains a cycle");
    if ((uint32_t)height > d->depth) return fail(ctx, OCTPT_ERR_INVALID_ARG, "octree is deeper than its declared depth");
    for (uint32_t l = 0; l < d->leaf_table_size; ++l)
        if ((uint64_t)d->leaf_first[l] + d->leaf_count[l] > d->leaf_prim_count)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "leaf range exceeds leaf_prims");
    for (uint32_t k = 0; k < d->leaf_prim_count; ++k) {
        const uint32_t p = d->leaf_prims[k];
        if (p & kPrimCuboidBit) {
            if ((p & ~kPrimCuboidBit) >= d->cuboid_count) return fail(ctx, OCTPT_ERR_INVALID_ARG, "cuboid index out of range");
        } else if (p >= d->sphere_count) {
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "sphere index out of range");
        }
    }
    return validate_tables(ctx, d);
}

// primitive materials, block models, materials and textures
octpt_status validate_tables(octpt_ctx *ctx, const octpt_scene_desc *d) {
    for (uint32_t s = 0; s < d->sphere_count; ++s)
        if (d->spheres[s].material >= d->material_count) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sphere material out of range");
    for (uint32_t c = 0; c < d->cuboid_count; ++c)
        for (int f = 0; f < 6; ++f)
            if (d->cuboids[c].face_material[f] >= d->material_count)
                return fail(ctx, OCTPT_ERR_INVALID_ARG, "cuboid material out of range");
    // block-value leaves (C23)
    for (uint32_t b = 0; d->blocks && b < d->block_count; ++b) {
        const octpt_block &x = d->blocks[b];
        if (x.model != OCTPT_MODEL_NONE) {
            if (x.model >= d->model_count) return fail(ctx, OCTPT_ERR_INVALID_ARG, "block model index out of range");
        } else {
            for (int f = 0; f < 6; ++f)
                if (x.face_material[f] >= d->material_count)
                    return fail(ctx, OCTPT_ERR_INVALID_ARG, "block face material out of range");
        }
    }
    if (d->blocks && d->quad_count > kPrimIndexMask)  // a quad hit record is kPrimCuboidBit | quad (C23)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "more than 2^27 quads in a block-value scene");
    // block models (C19; and of block-value scenes, C23)
    if (d->cuboid_model || d->blocks) {
        if (d->model_count && !d->models) return fail(ctx, OCTPT_ERR_INVALID_ARG, "models is NULL");
        if (d->quad_count && !d->quads) return fail(ctx, OCTPT_ERR_INVALID_ARG, "quads is NULL");
        if (d->quad_count >= kQuadKey) return fail(ctx, OCTPT_ERR_UNSUPPORTED, "more than 2^30 - 1 quads");
        for (uint32_t c = 0; d->cuboid_model && c < d->cuboid_count; ++c) {
            const uint32_t m = d->cuboid_model[c];
            if (m == OCTPT_MODEL_NONE) continue;
            if (m >= d->model_count) return fail(ctx, OCTPT_ERR_INVALID_ARG, "cuboid model index out of range");
            const octpt_cuboid &b = d->cuboids[c];
            for (int a = 0; a < 3; ++a)
                if (b.max[a] != b.min[a] + 1.0f)
                    return fail(ctx, OCTPT_ERR_INVALID_ARG, "a block-model cuboid must be a unit voxel [min, min+1)");
        }
        for (uint32_t m = 0; m < d->model_count; ++m)
            if ((uint64_t)d->models[m].first_quad + d->models[m].quad_count > d->quad_count)
                return fail(ctx, OCTPT_ERR_INVALID_ARG, "model quad range exceeds quads");
        for (uint32_t q = 0; q < d->quad_count; ++q)
            if (d->quads[q].material >= d->material_count)
                return fail(ctx, OCTPT_ERR_INVALID_ARG, "quad material out of range");
    }
    for (uint32_t m = 0; m < d->material_count; ++m)
        if (d->materials[m].texture_index >= d->texture_count)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "material texture_index out of range");
    for (uint32_t t = 0; t < d->texture_count; ++t) {
        const octpt_texture &x = d->textures[t];
        if (x.kind == OCTPT_TEXTURE_IMAGE) {
            if (x.width == 0 || x.height == 0 || !x.pixels)
                return fail(ctx, OCTPT_ERR_INVALID_ARG, "image texture without pixels");
        } else if (x.kind != OCTPT_TEXTURE_COLOR) {
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "unknown texture kind");
        }
    }
    return OCTPT_OK;
}

// The octree-independent part of a scene upload: primitive tables (host_prims; the device build
// writes them itself), block models (C19), materials, textures, LUTs and the sun.  S's octree
// fields are set by the caller.
octpt_status upload_tables(octpt_ctx *ctx, const octpt_scene_desc *d, bool host_prims, DevScene &S) {
    if (host_prims) {
        std::vector<float4> sph(d->sphere_count);
        std::vector<uint32_t> sph_mat(d->sphere_count);
        for (uint32_t s = 0; s < d->sphere_count; ++s) {
            const octpt_sphere &x = d->spheres[s];
            sph[s] = make_float4(x.center[0], x.center[1], x.center[2], x.radius);
            sph_mat[s] = x.material;
        }
        std::vector<float4> cmin(d->cuboid_count);
        std::vector<float2> cmax(d->cuboid_count);
        std::vector<uint32_t> cmat((size_t)d->cuboid_count * 6);
        for (uint32_t c = 0; c < d->cuboid_count; ++c) {
            const octpt_cuboid &x = d->cuboids[c];
            cmin[c] = make_float4(x.min[0], x.min[1], x.min[2], x.max[0]);
            cmax[c] = make_float2(x.max[1], x.max[2]);
            std::memcpy(&cmat[(size_t)c * 6], x.face_material, 24);
        }
        float4 *d_sph, *d_cmin;
        float2 *d_cmax;
        uint32_t *d_sph_mat, *d_cmat;
        HIP_TRY(ctx, upload(ctx, sph.data(), sph.size(), &d_sph));
        HIP_TRY(ctx, upload(ctx, sph_mat.data(), sph_mat.size(), &d_sph_mat));
        HIP_TRY(ctx, upload(ctx, cmin.data(), cmin.size(), &d_cmin));
        HIP_TRY(ctx, upload(ctx, cmax.data(), cmax.size(), &d_cmax));
        HIP_TRY(ctx, upload(ctx, cmat.data(), cmat.size(), &d_cmat));
        S.spheres = d_sph;
        S.sphere_mat = d_sph_mat;
        S.cub_a = d_cmin;
        S.cub_b = d_cmax;
        S.cub_mat = d_cmat;
    }
    // block models (C19): Quad::new (quad.rs:90-114) in glam's f32 operation order
    bool has_models = false;  // the scene draws block models (from cuboids, C19, or from blocks, C23)
    if (d->cuboid_model)
        for (uint32_t c = 0; c < d->cuboid_count && !has_models; ++c) has_models = d->cuboid_model[c] != OCTPT_MODEL_NONE;
    for (uint32_t b = 0; d->blocks && b < d->block_count && !has_models; ++b)
        has_models = d->blocks[b].model != OCTPT_MODEL_NONE;
    std::vector<DevQuad> quads;
    std::vector<uint2> models;
    if (has_models) {
        quads.resize(d->quad_count);
        for (uint32_t q = 0; q < d->quad_count; ++q) quads[q] = make_dev_quad(d->quads[q]);
        models.resize(d->model_count);
        for (uint32_t m = 0; m < d->model_count; ++m) models[m] = make_uint2(d->models[m].first_quad, d->models[m].quad_count);
    }
    float lf[256];
    uint8_t lb[256];
    make_luts(lf, lb);
    std::vector<DevMaterial> mats(d->material_count);
    for (uint32_t m = 0; m < d->material_count; ++m) {
        const octpt_material &x = d->materials[m];
        const octpt_texture &t = d->textures[x.texture_index];
        DevMaterial dm{};
        dm.ior = x.ior;
        dm.specular = x.specular;
        dm.emittance = x.emittance;
        dm.roughness = x.roughness;
        dm.metalness = x.metalness;
        dm.texture_index = x.texture_index;
        dm.flags = x.flags;
        dm.texture_kind = t.kind;
        if (t.kind == OCTPT_TEXTURE_COLOR) {  // F32Color::from(&U8Color) (colors/mod.rs:280-288)
            dm.color[0] = lf[t.rgba[0]];
            dm.color[1] = lf[t.rgba[1]];
            dm.color[2] = lf[t.rgba[2]];
            dm.color[3] = (float)t.rgba[3] / 255.0f;
        }
        mats[m] = dm;
    }
    std::vector<DevTexture> texs(d->texture_count);
    std::vector<uint8_t> texels;
    for (uint32_t t = 0; t < d->texture_count; ++t) {
        const octpt_texture &x = d->textures[t];
        DevTexture dt{};
        dt.kind = x.kind;
        dt.rgba = (uint32_t)x.rgba[0] | ((uint32_t)x.rgba[1] << 8) | ((uint32_t)x.rgba[2] << 16) | ((uint32_t)x.rgba[3] << 24);
        if (x.kind == OCTPT_TEXTURE_IMAGE) {
            dt.width = x.width;
            dt.height = x.height;
            dt.offset = texels.size();
            texels.insert(texels.end(), x.pixels, x.pixels + (size_t)x.width * x.height * 4);
        }
        texs[t] = dt;
    }
    DevMaterial *d_mats;
    DevTexture *d_texs;
    uint8_t *d_texels;
    HIP_TRY(ctx, upload(ctx, mats.data(), mats.size(), &d_mats));
    HIP_TRY(ctx, upload(ctx, texs.data(), texs.size(), &d_texs));
    HIP_TRY(ctx, upload(ctx, texels.data(), texels.size(), &d_texels));
    uint32_t *d_cmodel = nullptr;
    uint2 *d_models = nullptr;
    DevQuad *d_quads = nullptr;
    if (has_models) {
        if (d->cuboid_model) HIP_TRY(ctx, upload(ctx, d->cuboid_model, d->cuboid_count, &d_cmodel));
        HIP_TRY(ctx, upload(ctx, models.data(), models.size(), &d_models));
        HIP_TRY(ctx, upload(ctx, quads.data(), quads.size(), &d_quads));
    }
    uint32_t *d_blk_mat = nullptr, *d_blk_model = nullptr;
    if (d->blocks) {  // C23: six face materials and the model of every block
        std::vector<uint32_t> bm((size_t)d->block_count * 6), bmod(d->block_count);
        for (uint32_t b = 0; b < d->block_count; ++b) {
            std::memcpy(&bm[(size_t)b * 6], d->blocks[b].face_material, 24);
            bmod[b] = d->blocks[b].model;
        }
        HIP_TRY(ctx, upload(ctx, bm.data(), bm.size(), &d_blk_mat));
        HIP_TRY(ctx, upload(ctx, bmod.data(), bmod.size(), &d_blk_model));
    }
    S.depth = d->depth;
    S.has_cuboids = d->cuboid_count ? 1u : 0u;
    S.octree_scale = ldexpf(1.0f, -(int)d->depth);  // Octree::scale (new_octree.rs:40-42)
    S.inv_octree_scale = ldexpf(1.0f, (int)d->depth);
    S.cub_model = d_cmodel;
    S.models = d_models;
    S.quads = d_quads;
    // the cuboid-model path (C19) of the primitive kernels; block-value scenes draw their models in
    // the block instance (has_blocks)
    S.has_models = (has_models && !d->blocks) ? 1u : 0u;
    S.has_blocks = d->blocks ? 1u : 0u;
    S.n_blocks = d->blocks ? d->block_count : 0u;
    S.blk_mat = d_blk_mat;
    S.blk_model = d_blk_model;
    S.mats = d_mats;
    S.n_mats = d->material_count;
    S.texs = d_texs;
    S.n_texs = d->texture_count;
    S.has_images = 0u;
    for (uint32_t t = 0; t < d->texture_count; ++t)
        if (d->textures[t].kind == OCTPT_TEXTURE_IMAGE) S.has_images = 1u;
    S.texels = d_texels;
    S.lut_float = ctx->d_lut_float;
    make_sun(d->sun, lf, S.sun);
    S.sun.f_sub_surface = d->f_sub_surface;
    S.emitters = d->emitters_enabled ? 1 : 0;
    // the lean path state (WaveBuffers::lean): a continuing path's radiance is 0 when nothing adds light
    // before its end -- no emitting material (shade_segment adds emittance > EPSILON when emitters are on)
    // and no sun sampling (C18 adds the sun's direct light mid-path)
    bool emissive = false;
    for (uint32_t i = 0; i < d->material_count && d->emitters_enabled; ++i)
        emissive = emissive || d->materials[i].emittance > 5e-8f;  // RAY_EPSILON
    ctx->lean_scene = !emissive && !d->sun.sun_sampling;
    ctx->block_emissive.clear();  // (validate_tables checked every face material)
    if (d->blocks) block_emissive_flags(d->blocks, d->block_count, d->materials, d->material_count, ctx->block_emissive);
    // ... and the emissive-model table (C39; validate_tables checked the quad ranges, the quad materials and every
    // block's model)
    ctx->emit_models = EmissiveModelTable{};
    ctx->model_emissive.clear();
    if (d->blocks && d->model_count) {
        emissive_model_table(d->models, d->model_count, d->quads, d->quad_count, d->materials, d->material_count,
                             ctx->emit_models);
        ctx->model_emissive = model_emissive_bytes(ctx->emit_models);
    }
    return OCTPT_OK;
}

// The slot flags of every block (C23, kBlock* in octpt_internal.h): kBlockIsModel for a block model, else
// bit f for a face whose material's texture holds a texel of alpha byte 0 -- the only texels that
// SingleBlockModel::intersect's alpha test (texel alpha <= EPSILON, C23) rejects -- so that the leaf test
// reads a texel only where it can decide something
std::vector<uint32_t> block_slot_flags(const octpt_scene_desc *d) {
    std::vector<int8_t> tex_zero(d->texture_count, -1);
    auto zero_alpha = [&](uint32_t t) {
        if (tex_zero[t] < 0) {
            const octpt_texture &x = d->textures[t];
            bool z = false;
            if (x.kind == OCTPT_TEXTURE_COLOR) {
                z = x.rgba[3] == 0;
            } else {
                const size_t n = (size_t)x.width * x.height;
                for (size_t k = 0; k < n && !z; ++k) z = x.pixels[4 * k + 3] == 0;
            }
            tex_zero[t] = z ? 1 : 0;
        }
        return tex_zero[t] != 0;
    };
    std::vector<uint32_t> flags(d->block_count, 0u);
    for (uint32_t b = 0; b < d->block_count; ++b) {
        const octpt_block &x = d->blocks[b];
        if (x.model != OCTPT_MODEL_NONE) {
            flags[b] = kBlockIsModel;
            continue;
        }
        for (uint32_t f = 0; f < 6; ++f)
            if (zero_alpha(d->materials[x.face_material[f]].texture_index)) flags[b] |= 1u << f;
    }
    return flags;
}

uint32_t tiles_of_shard(uint32_t n_tiles, uint32_t shard, uint32_t count) {
    return shard < n_tiles ? (n_tiles - shard + count - 1) / count : 0;
}

}  // namespace

octpt_status octpt::make_render(octpt_ctx *ctx, const octpt_render_params *p, DevRender &R) {
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "render params NULL");
    if (!ctx->has_scene) return fail(ctx, OCTPT_ERR_INVALID_ARG, "no scene uploaded (set_scene)");
    if (!ctx->has_camera) return fail(ctx, OCTPT_ERR_INVALID_ARG, "no camera set");
    if (p->width == 0 || p->height == 0 || (uint64_t)p->width * p->height >= (1ull << 31))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "bad resolution");
    if (p->max_depth == 0) return fail(ctx, OCTPT_ERR_INVALID_ARG, "max_depth must be >= 1");
    if (ctx->rays.d_rays) {  // a ray source (C41) is a list for one frame size, and has no megakernel instance
        if (p->width != ctx->rays.width || p->height != ctx->rays.height)
            return fail(ctx, OCTPT_ERR_INVALID_ARG,
                        "render size differs from the ray source's (octpt_set_ray_source; NULL clears it)");
        if ((p->flags & OCTPT_RENDER_MEGAKERNEL) && !(p->flags & OCTPT_RENDER_PREVIEW))
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "a ray source is set: it runs on the wavefront path only");
    }
    // a sky other than DEFAULT (C42) has wavefront instances only
    if (ctx->sky.mode != kSkyDefault && (p->flags & OCTPT_RENDER_MEGAKERNEL) && !(p->flags & OCTPT_RENDER_PREVIEW))
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "a sky is set (octpt_set_sky): it runs on the wavefront path only");
    // sky sampling (C43) has wavefront instances only, and none together with emitter sampling
    if (ctx->sky_sampling == OCTPT_SKY_SAMPLING_MAP && !(p->flags & OCTPT_RENDER_PREVIEW)) {
        if (p->flags & OCTPT_RENDER_MEGAKERNEL)
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "sky sampling is on (octpt_set_sky_sampling): it runs on the wavefront path only");
        if (ctx->emit_strategy == OCTPT_EMITTERS_ONE)
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "sky sampling together with emitter sampling ONE (DESIGN.md C43)");
    }
    if (ctx->emit_strategy == OCTPT_EMITTERS_ONE && !(p->flags & OCTPT_RENDER_PREVIEW)) {  // C38
        const octpt_ctx *gc = ctx->sub.empty() ? ctx : ctx->sub[0];  // a multi-device context: its entries hold the scene
        if (!gc->S.has_blocks)
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "emitter sampling needs a block-value scene (octpt_scene_desc.blocks)");
        if (p->flags & OCTPT_RENDER_MEGAKERNEL)
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "emitter sampling runs on the wavefront path only");
        if (!gc->grid_valid) return fail(ctx, OCTPT_ERR_INTERNAL, "emitter sampling is on and the context holds no grid");
    }
    if (ctx->sample_clamp != 0.0f && (p->flags & OCTPT_RENDER_MEGAKERNEL) && !(p->flags & OCTPT_RENDER_PREVIEW))
        return fail(ctx, OCTPT_ERR_UNSUPPORTED,
                    "a sample clamp is set (octpt_set_sample_clamp): the megakernel accumulates inside the kernel");
    const uint32_t B = p->branch_count ? p->branch_count : 1u;
    if (B > 64u) return fail(ctx, OCTPT_ERR_INVALID_ARG, "branch_count must be <= 64");
    if (p->shard_count == 0 || p->shard_index >= p->shard_count) return fail(ctx, OCTPT_ERR_INVALID_ARG, "bad shard");
    if ((uint64_t)p->spp_start + p->spp_count >= (1ull << 24))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "spp_start + spp_count must stay below 2^24");
    R.W = p->width;
    R.H = p->height;
    R.spp_start = p->spp_start;
    R.spp_count = p->spp_count;
    R.max_depth = p->max_depth;
    R.seed = p->seed;
    R.shard_index = p->shard_index;
    R.shard_count = p->shard_count;
    R.compact = (p->flags & OCTPT_RENDER_SHARD_COMPACT) ? 1u : 0u;
    ctx->ktiming = (p->flags & OCTPT_RENDER_KERNEL_TIMING) != 0;
    R.tiles_x = (p->width + kTile - 1) / kTile;
    const uint32_t tiles_y = (p->height + kTile - 1) / kTile;
    R.shard_tiles = tiles_of_shard(R.tiles_x * tiles_y, p->shard_index, p->shard_count);
    R.total_items = R.shard_tiles * 64u;
    R.div_tiles_x = udiv_magic(R.tiles_x);
    R.div_items = udiv_magic(R.total_items);
    R.group_shift = 0u;  // the wavefront path sets it per chunk (enqueue_wavefront)
    R.dim = (float)std::max(p->width, p->height);
    R.jlo = -1.0f / R.dim;
    R.jhi = 1.0f / R.dim;
    R.subs = nullptr;
    R.beam = nullptr;
    R.beam_tx = (p->width + kBeamTile - 1) / kBeamTile;
    R.tile_order = nullptr;
    if (!ctx->h_order.empty()) {  // a tile order applies to the frame size it was set for
        if (p->width != ctx->order_w || p->height != ctx->order_h)
            return fail(ctx, OCTPT_ERR_INVALID_ARG,
                        "render size differs from the tile order's (octpt_set_tile_order; NULL resets it)");
        R.tile_order = ctx->d_order;
    }
    if (B > 1u && !(p->flags & OCTPT_RENDER_PREVIEW)) {
        // TileRenderer pass schedule (tile_renderer.rs:416-484, C20): the call covers whole passes
        if (p->flags & OCTPT_RENDER_MEGAKERNEL)
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "branch_count > 1 runs on the wavefront path only");
        uint64_t spp = 0;
        while (spp < p->spp_start) spp += current_branch_count((uint32_t)spp, B);
        if (spp != p->spp_start)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "spp_start is not a pass boundary of the branch schedule");
        const uint64_t end = (uint64_t)p->spp_start + p->spp_count;
        ctx->h_subs.clear();
        while (spp < end) {
            const uint32_t bc = current_branch_count((uint32_t)spp, B);
            for (uint32_t b = 0; b < bc; ++b) ctx->h_subs.push_back(make_uint2((uint32_t)spp, bc | (b << 16)));
            spp += bc;
        }
        if (spp != end)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "spp_start + spp_count is not a pass boundary of the branch schedule");
        if (!ctx->h_subs.empty()) {
            HIP_TRY(ctx, hipDeviceSynchronize());  // an earlier render may still read the table
            const octpt_status st = grow_buf(ctx, ctx->d_subs, ctx->h_subs.size());
            if (st != OCTPT_OK) return st;
            HIP_TRY(ctx, hipMemcpy(ctx->d_subs.p, ctx->h_subs.data(), ctx->h_subs.size() * sizeof(uint2),
                                   hipMemcpyHostToDevice));
            R.subs = ctx->d_subs.p;
        }
    }
    // RendererMode::Preview renders one replacing pass; spp and max_depth do not apply (C16)
    R.preview = (p->flags & OCTPT_RENDER_PREVIEW) ? 1u : 0u;
    if (R.preview) R.spp_count = 1u;
    return OCTPT_OK;
}

namespace {

// wavefront-state allocations, counted against the optional mem_limit
hipError_t wave_malloc(octpt_ctx *ctx, void **p, size_t bytes) {
    *p = nullptr;
    if (ctx->mem_limit && ctx->wave_bytes + bytes > ctx->mem_limit) return hipErrorOutOfMemory;
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return e;
    ctx->wave_bytes += bytes;
    ctx->wave_sizes.emplace_back(*p, bytes);
    return hipSuccess;
}
void wave_free(octpt_ctx *ctx, void *&p) {
    if (!p) return;
    for (size_t i = 0; i < ctx->wave_sizes.size(); ++i)
        if (ctx->wave_sizes[i].first == p) {
            ctx->wave_bytes -= ctx->wave_sizes[i].second;
            ctx->wave_sizes.erase(ctx->wave_sizes.begin() + (ptrdiff_t)i);
            break;
        }
    (void)hipFree(p);
    p = nullptr;
}
// the queues and path state (ctx->wave_allocs)
void free_queues(octpt_ctx *ctx) {
    for (void *p : ctx->wave_allocs) wave_free(ctx, p);
    ctx->wave_allocs.clear();
    ctx->pool = 0;
    ctx->wb.hit4 = nullptr;  // allocated with the queues (block-value scenes)
}

void free_wave(octpt_ctx *ctx) {
    free_queues(ctx);
    wave_free(ctx, ctx->color_alloc);
    wave_free(ctx, ctx->nee_alloc);
    ctx->pool = ctx->color_cap = ctx->nee_pool = 0;
    ctx->wb = WaveBuffers{};
}

template <class T>
hipError_t wave_alloc(octpt_ctx *ctx, size_t n, T **out) {
    void *p = nullptr;
    const hipError_t e = wave_malloc(ctx, &p, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    ctx->wave_allocs.push_back(p);
    *out = static_cast<T *>(p);
    return hipSuccess;
}

// host snapshot of the iteration's counters, read kLookahead iterations later: the kSegs segment counts
// of the queue the iteration's shade filled, then the kSegs chunk item claims (two strided copies of one
// word per 256-B counter line, not the whole 80-KB ctrl block)
constexpr uint32_t kCountSpan = 2u * kSegs;

// queue segment capacity: seed wave w fills segment w % kSegs, so ceil(ceil(pool / 64) / kSegs) waves
size_t seg_cap_for(size_t pool) { return ((pool + 63) / 64 + kSegs - 1) / kSegs * 64; }

// which allocation of ensure_wave ran out of device memory
enum OomPart { kOomNone = 0, kOomQueues, kOomColor, kOomNee };

// The wavefront state of a render: `pool` path slots of queues + path state, `color_items` colour
// records, and (nee) the sun-sampling planes of every slot.  Grow-only.  When the queues + path state
// do not fit (another tenant, the host application's own allocations) the pool halves down to kMinPool
// and the pool obtained becomes the context's cap (pool_cap), so later renders neither retry the larger
// pool nor re-allocate.  A colour or sun-sampling allocation that fails returns OOM with *part set; the
// caller shrinks the chunk or the pool and calls again (enqueue_wavefront).
octpt_status ensure_wave(octpt_ctx *ctx, size_t pool, size_t color_items, bool nee, bool blocks, OomPart *part,
                         bool emit = false) {
    *part = kOomNone;
    if (!ctx->h_count) {
        // coherent (fine-grained) pinned memory: wf_snapshot_kernel's stores reach the host directly
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_count), (kLookahead + 1) * kCountSpan * sizeof(uint32_t),
                                   hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(ctx, hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->d_count), ctx->h_count, 0));
        for (auto &ev : ctx->count_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    if (pool > ctx->pool) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        free_queues(ctx);
        WaveBuffers &B = ctx->wb;
        // queues + path state: 124 B per slot
        size_t want = pool;
        for (;;) {
            B.seg_cap = (uint32_t)seg_cap_for(want);
            const size_t qlen = (size_t)kSegs * B.seg_cap;  // queue positions
            hipError_t e = wave_alloc(ctx, qlen, &B.ray0[0]);
            if (e == hipSuccess) e = wave_alloc(ctx, qlen, &B.ray0[1]);
            if (e == hipSuccess) e = wave_alloc(ctx, qlen, &B.ray1[0]);
            if (e == hipSuccess) e = wave_alloc(ctx, qlen, &B.ray1[1]);
            // pa, pb: per slot, or (the lean state) per position of queue 0 / 1; pc: per slot, or both queues
            if (e == hipSuccess) e = wave_alloc(ctx, qlen, &B.pa);
            if (e == hipSuccess) e = wave_alloc(ctx, qlen, &B.pb);
            if (e == hipSuccess) e = wave_alloc(ctx, 2 * qlen, &B.pc);
            if (e == hipSuccess) e = wave_alloc(ctx, want, &B.item0);
            if (e == hipSuccess) e = wave_alloc(ctx, qlen, &B.hit);
            if (e == hipSuccess) e = wave_alloc(ctx, kCtrlWords, &B.ctrl);
            if (e == hipSuccess) break;
            free_queues(ctx);
            (void)hipGetLastError();
            if (e != hipErrorOutOfMemory || want <= kMinPool) {
                *part = kOomQueues;
                return hip_fail(ctx, e, "wave buffers");
            }
            want = std::max<size_t>(want / 2, kMinPool);
        }
        if (want < pool) {
            if (!ctx->oom_warned)
                std::fprintf(stderr, "octpt: %zu path slots did not fit in device memory; using %zu\n", pool, want);
            ctx->oom_warned = true;
            ctx->pool_cap = (uint32_t)want;  // sticky: later renders ask for at most what fitted
        }
        B.pool = (uint32_t)want;
        ctx->pool = want;
        ctx->wave_allocs_n++;
    }
    // block-value scenes (C23): their 16-B hit records (t, u, v beside the block), one per queue position
    if (blocks && !ctx->wb.hit4) {
        const hipError_t e = wave_alloc(ctx, (size_t)kSegs * ctx->wb.seg_cap, &ctx->wb.hit4);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *part = kOomNee;  // a per-slot plane like the sun-sampling ones: the pool shrinks
            return hip_fail(ctx, e, "block hit coordinates");
        }
    }
    // sun-sampling planes (4 x 16 B per slot) only for scenes that sample the sun (C18)
    // ... six with emitter sampling (C38): the emitter segment rides the same state, a waiting sun sample takes two more
    const size_t planes = emit ? 6u : 4u;
    if ((nee || emit) && (ctx->nee_pool < ctx->pool || ctx->nee_planes < planes)) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        wave_free(ctx, ctx->nee_alloc);
        ctx->nee_pool = 0;
        ctx->nee_planes = 0;
        const hipError_t e = wave_malloc(ctx, &ctx->nee_alloc, planes * ctx->pool * sizeof(float4));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *part = kOomNee;
            return hip_fail(ctx, e, "sun-sampling planes");
        }
        ctx->nee_pool = ctx->pool;
        ctx->nee_planes = planes;
    }
    ctx->wb.pd = static_cast<float4 *>(ctx->nee_alloc);
    if (color_items > ctx->color_cap) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        wave_free(ctx, ctx->color_alloc);
        ctx->color_cap = 0;
        const hipError_t e = wave_malloc(ctx, &ctx->color_alloc, color_items * sizeof(float4));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *part = kOomColor;
            return hip_fail(ctx, e, "colour records");
        }
        ctx->color_cap = color_items;
    }
    ctx->wb.color = static_cast<float4 *>(ctx->color_alloc);
    ctx->wb.pool = (uint32_t)ctx->pool;
    return OCTPT_OK;
}

// begin / end a timed kernel launch of `kind` on stream s (no-op unless ctx->ktiming)
octpt_status ktimer_begin(octpt_ctx *ctx, hipStream_t s, EventPair &ev) {
    if (!ctx->ktiming) return OCTPT_OK;
    if (ctx->ev_pool.empty()) {
        EventPair e{};
        HIP_TRY(ctx, hipEventCreate(&e.start));
        HIP_TRY(ctx, hipEventCreate(&e.stop));
        ctx->ev_pool.push_back(e);
    }
    ev = ctx->ev_pool.back();
    ctx->ev_pool.pop_back();
    HIP_TRY(ctx, hipEventRecord(ev.start, s));
    return OCTPT_OK;
}
octpt_status ktimer_end(octpt_ctx *ctx, hipStream_t s, int kind, const EventPair &ev) {
    if (!ctx->ktiming) return OCTPT_OK;
    ctx->kpending.emplace_back(kind, ev);
    HIP_TRY(ctx, hipEventRecord(ev.stop, s));
    return OCTPT_OK;
}

// megakernel variant (OCTPT_RENDER_MEGAKERNEL): one persistent launch per call
octpt_status enqueue_megakernel(octpt_ctx *ctx, const DevRender &R, float4 *d_accum, uint32_t *d_seg, hipStream_t s) {
    uint32_t *counter = ctx->d_counters + (ctx->launch_seq++ % kCounterRing);
    HIP_TRY(ctx, hipMemsetAsync(counter, 0, sizeof(uint32_t), s));
    int &bpc = ctx->blocks_per_cu_cache[ctx->S.depth];
    if (bpc == 0) bpc = render_blocks_per_cu(ctx->S.depth);
    const uint64_t needed = ((uint64_t)R.total_items + kBlock - 1) / kBlock;
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(needed, (uint64_t)ctx->num_cu * bpc));
    HIP_TRY(ctx, launch_render(ctx->S, ctx->C, R, d_accum, d_seg, counter, ctx->d_stats, grid, s));
    return OCTPT_OK;
}

// wavefront path tracer: per chunk of passes, seed the path pool, then
// alternate extend/shade until the ray queue drains, then resolve the running means.  The
// host steers the loop with a one-iteration lookahead on the queue length.
// d_moments (nullable): resolve's moments instance (C31).  list: the number of a tile-list render's list (C30), 0 for
// every other render.
octpt_status enqueue_wavefront(octpt_ctx *ctx, const DevRender &R, float4 *d_accum, uint32_t *d_seg, hipStream_t s,
                               const std::atomic<bool> *cancel, float2 *d_moments = nullptr, uint64_t list = 0) {
    const uint64_t n_px = R.total_items;
    // the camera as the kernels take it: under a ray source (C41) it carries the caller's list
    const DevCamera C = ray_source_camera(ctx);
    // the sample clamp (C33) as set when the render call was made: octpt_set_sample_clamp joins a frame in flight
    const float clamp = ctx->sample_clamp;
    // emitter sampling (C38): strategy ONE over a grid that holds emitters, in a scene whose emitters are enabled,
    // takes the emitter instances of shade and the drain; an empty grid has nothing to sample and renders through
    // the ordinary ones
    const bool emit = ctx->emit_strategy == OCTPT_EMITTERS_ONE && ctx->grid_valid && ctx->emit_grid.n_emitters != 0u &&
                      ctx->S.emitters != 0 && ctx->S.has_blocks != 0u;
    // the sky (C42) as set when the render call was made (octpt_set_sky joins a frame in flight): other than DEFAULT,
    // shade and the drain are the sky instances and the chunks keep the general path state
    const Sky sky_rec = ctx->sky;
    const Sky *sky = sky_rec.mode != kSkyDefault ? &sky_rec : nullptr;
    // sky sampling (C43): on, the sky a MAP and its distribution's total not 0 -- shade and the drain are the
    // sky-sampling instances then, which read the distribution behind the sky record; every other case renders through
    // the instances it takes without the setting
    const SkyDist dist_rec{ctx->sky_dist.row_cdf, ctx->sky_dist.col_cdf, ctx->sky_dist.total};
    const SkyDist *dist = (sky && sky_rec.mode == kSkyMap && ctx->sky_sampling == OCTPT_SKY_SAMPLING_MAP && !emit &&
                           ctx->sky_dist.row_cdf && ctx->sky_dist.total != 0ull)
                              ? &dist_rec
                              : nullptr;
    DevScene Se = ctx->S;  // what shade and the drain take
    if (emit) {
        const DeviceEmitterGrid &g = ctx->emit_grid;
        uint32_t axis_bits = 0;
        while ((1u << axis_bits) < g.cells_axis) ++axis_bits;
        const bool models = (g.flags & OCTPT_EMITTERS_MODELS) != 0u;  // C39: the table beside the grid
        const EmitGrid hdr{g.cell_first, g.cell_emitters, g.emitters, g.grid_shift, axis_bits, 1u << ctx->S.depth,
                           ctx->emit_intensity, g.flags, 0u,
                           models ? ctx->d_model_first : nullptr, models ? ctx->d_model_quad : nullptr,
                           models ? ctx->d_model_cum : nullptr, models ? ctx->d_model_ouv : nullptr};
        if (!ctx->d_emit_hdr) HIP_TRY(ctx, hipMalloc(&ctx->d_emit_hdr, sizeof(EmitGrid)));
        if (!ctx->emit_hdr_valid || std::memcmp(&ctx->emit_hdr_host, &hdr, sizeof hdr) != 0) {
            // a new grid or intensity: an earlier render (on any stream) may still read the old header
            ctx->emit_hdr_valid = false;
            HIP_TRY(ctx, hipDeviceSynchronize());
            HIP_TRY(ctx, hipMemcpy(ctx->d_emit_hdr, &hdr, sizeof hdr, hipMemcpyHostToDevice));
            ctx->emit_hdr_host = hdr;
            ctx->emit_hdr_valid = true;
        }
        Se.leaf_sph = reinterpret_cast<const float4 *>(ctx->d_emit_hdr);
    }
    uint32_t chunk_spp = 1;
    uint64_t chunk_max = 0;
    octpt_status st = OCTPT_OK;
    for (;;) {
        chunk_spp = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(R.spp_count, ctx->chunk_cap / n_px));
        // a branch-schedule chunk holds whole passes (<= 64 sub-samples each, C20)
        if (R.subs) chunk_spp = std::max(chunk_spp, std::min(64u, R.spp_count));
        chunk_max = (uint64_t)chunk_spp * n_px;
        if (chunk_max > kMaxChunkPaths)  // a branch pass of 64 sub-samples over > 2^25 pixels
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "a branch-schedule pass exceeds the 2^31-item chunk limit");
        OomPart part = kOomNone;
        st = ensure_wave(ctx, (size_t)std::min<uint64_t>(ctx->pool_cap, chunk_max), chunk_max,
                         ctx->S.sun.sun_sampling != 0, ctx->S.has_blocks != 0, &part,
                         emit || dist);  // (the sky segment rides the emitter segment's six planes)
        if (st == OCTPT_OK) break;
        if (st != OCTPT_ERR_OOM) return st;
        // out of device memory past the queues: a smaller chunk (colour records) or pool (planes), kept
        // for later renders; chunks and pools of any size render the same frame
        if (part == kOomColor && chunk_spp > 1 && !R.subs) {
            ctx->chunk_cap = (uint64_t)(chunk_spp / 2) * n_px;
            if (ctx->pool > ctx->chunk_cap) {  // release the queues too: they were sized for the larger chunk
                HIP_TRY(ctx, hipDeviceSynchronize());
                free_queues(ctx);
                ctx->pool_cap = (uint32_t)std::max<uint64_t>(kMinPool, std::min<uint64_t>(ctx->pool_cap, ctx->chunk_cap));
            }
        } else if (part == kOomNee && ctx->pool > kMinPool) {
            HIP_TRY(ctx, hipDeviceSynchronize());
            ctx->pool_cap = (uint32_t)std::max<size_t>(kMinPool, ctx->pool / 2);
            free_queues(ctx);
        } else {
            return st;
        }
        if (!ctx->oom_warned)
            std::fprintf(stderr, "octpt: wavefront state did not fit in device memory; chunk %llu items, pool cap %u\n",
                         (unsigned long long)ctx->chunk_cap, ctx->pool_cap);
        ctx->oom_warned = true;
    }
    // the pool actually held (smaller than asked after an out-of-memory fallback)
    const size_t pool = (size_t)std::min<uint64_t>(std::min<uint64_t>(ctx->pool_cap, chunk_max), ctx->pool);
    int &bpc = ctx->extend_bpc_cache[ctx->S.depth][ctx->S.has_blocks ? 3 : ctx->S.has_models ? 2 : (ctx->S.has_cuboids ? 1 : 0)];
    if (bpc == 0) bpc = extend_blocks_per_cu(ctx->S);
    const int grid_extend = ctx->num_cu * bpc;
    if (std::getenv("OCTPT_DEBUG"))
        std::fprintf(stderr, "octpt: extend %d blocks/CU x %d CUs (depth %u, cuboids %u, models %u), pool %zu\n", bpc,
                     ctx->num_cu, ctx->S.depth, ctx->S.has_cuboids, ctx->S.has_models, pool);
    // shade maps waves to queue segments: a multiple of kSegs waves (kSegs / 4 blocks)
    const int seg_blocks = (int)(kSegs * 64u / kBlock);
    // blocks per CU: what the instance's registers allow (4 with regeneration, 5 without), or OCTPT_SHADE_BPC
    const uint32_t shade_bpc_env = std::min<uint32_t>(env_u32("OCTPT_SHADE_BPC", 0u), 8u);
    // (sized by the ordinary instance's occupancy also when the emitter instances run, C38: they hold more registers,
    // so their grid is oversubscribed; shade's grid-stride loop makes the grid size a matter of speed alone: accepted)
    auto grid_shade_of = [&](int mode) {
        int &cached = ctx->shade_bpc_cache[ctx->S.sun.sun_sampling ? 1 : 0]
                                          [shade_lds_tables(ctx->S) ? 1 : 0]
                                          [mode];
        if (cached == 0) cached = shade_blocks_per_cu(ctx->S, mode);
        const int bpc = shade_bpc_env ? (int)shade_bpc_env : cached;
        return (ctx->num_cu * bpc + seg_blocks - 1) / seg_blocks * seg_blocks;
    };
    {
        float none;
        std::memcpy(&none, &kPrimNone, sizeof none);
        ctx->wb.eye = make_float4(ctx->C.eye[0], ctx->C.eye[1], ctx->C.eye[2], none);
    }
    const WaveBuffers &B = ctx->wb;
    // the camera rays' beam starts, once per render call: every chunk's camera rays
    // share them (OCTPT_BEAM=0 switches them off; results are identical, ESVO iterations fewer)
    // A camera with an aperture (C37) renders without them: behind the focal plane a lens ray leaves the tile's
    // pyramid from the eye without bound, so the table is not conservative for it
    // A projection other than pinhole (C40) likewise: the table is computed for the pinhole's pyramids, and such rays
    // take the lens's path through the chunk (origins of their own, full records, the general shade's twins)
    // A ray source (C41) likewise: its camera's proj_mode is kProjModeRays
    const bool lens = C.aperture > 0.0f || C.proj_mode != OCTPT_PROJECTION_PINHOLE;
    const float *beam = nullptr;
    if (ctx->beam && !lens) {
        const size_t n_tiles = (size_t)R.beam_tx * ((R.H + kBeamTile - 1) / kBeamTile);
        octpt_ctx::BeamKey key;
        key.scene = ctx->scene_gen;
        key.camera = ctx->camera_gen;
        key.order = ctx->order_gen;
        key.w = R.W;
        key.h = R.H;
        key.shard_index = R.shard_index;
        key.shard_count = R.shard_count;
        key.list = list;
        key.valid = true;
        if (list != 0u) {
            // a tile list reads a subset of the whole frame's table: one computed by an ordinary one-shard render
            // of this scene, camera and size serves it (the adaptive driver's later rounds) and stays as it is
            octpt_ctx::BeamKey whole = key;
            whole.list = 0u;
            if (whole == ctx->beam_key) key = whole;
        }
        if (needs_grow(n_tiles, ctx->d_beam)) {
            HIP_TRY(ctx, hipDeviceSynchronize());  // an earlier render may still read the table
            ctx->beam_key.valid = false;
            const octpt_status st = grow_buf(ctx, ctx->d_beam, n_tiles);
            if (st != OCTPT_OK) return st;
        }
        if (!ctx->beam_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->beam_ev, hipEventDisableTiming));
        if (!(key == ctx->beam_key)) {  // same scene, camera, size, shard and deal: the table is already there
            // overwriting a valid table: renders on other streams may still read it (write-after-read),
            // so the device drains first; a render on the computing stream is ordered by the stream itself
            if (ctx->beam_key.valid && (s != ctx->beam_stream || ctx->beam_shared)) HIP_TRY(ctx, hipDeviceSynchronize());
            ctx->beam_key.valid = false;
            HIP_TRY(ctx, launch_beam(ctx->S, C, R, ctx->d_beam.p, s));
            HIP_TRY(ctx, hipEventRecord(ctx->beam_ev, s));
            ctx->beam_key = key;
            ctx->beam_stream = s;
            ctx->beam_shared = false;
        } else {
            HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->beam_ev, 0));  // (a no-op on the stream that computed it)
            ctx->beam_shared |= s != ctx->beam_stream;  // read on another stream: a recompute drains the device
        }
        beam = ctx->d_beam.p;
    }
    for (uint32_t c0 = 0, c1 = 0; c0 < R.spp_count; c0 = c1) {
        c1 = c0 + std::min(chunk_spp, R.spp_count - c0);
        if (R.subs) {  // a chunk ends on a pass boundary (C20): branches of one pass resolve together
            uint32_t e = c1;
            while (e < R.spp_count && (ctx->h_subs[e].y >> 16) != 0u) --e;
            if (e <= c0) {  // one pass larger than the chunk: take the whole pass
                e = c1;
                while (e < R.spp_count && (ctx->h_subs[e].y >> 16) != 0u) ++e;
            }
            c1 = e;
        }
        DevRender Rc = R;
        Rc.spp_start = R.spp_start + c0;
        Rc.spp_count = c1 - c0;
        if (R.subs) Rc.subs = R.subs + c0;
        // the item order's sample group (item_split): a power of four that divides the chunk's samples, so that every
        // wave's G samples exist; a branch schedule keeps one sample per wave
        // Without OCTPT_SAMPLE_GROUP the order is grouped only where it was measured to pay: scenes of
        // spheres and cuboids alone, in chunks of at least kGroupMinItems items.  Elsewhere the grouped order loses at
        // every G although resolve now reads its records once (resolve_pixel_wide): at G = 4 / 16 / 64 C2's 59 M-item
        // frame -2.6 / -27 / -77 %, block-value C5b -0.5 / -4 / -38 %, block-model C5 -1.8 / -7 / -33 %
        const bool grouped = ctx->sample_group_set ||
                             (!ctx->S.has_blocks && !ctx->S.has_models && (uint64_t)Rc.spp_count * n_px >= kGroupMinItems);
        Rc.group_shift = (R.subs || !grouped) ? 0u : group_shift_of(ctx->sample_group, Rc.spp_count);
        Rc.beam = beam;
        const uint32_t chunk_items = (uint32_t)((uint64_t)Rc.spp_count * n_px);
        HIP_TRY(ctx, hipMemsetAsync(B.ctrl, 0, kCtrlWords * sizeof(uint32_t), s));
        const uint32_t n_seed = (uint32_t)std::min<uint64_t>(pool, chunk_items);
        const bool regen = n_seed < chunk_items;  // else the seed claimed every item of the chunk
        // the lean 24-B path state: L stays 0 until the path ends, item = slot
        // (and no branch schedule: the lean shade instances carry no first-reflection split)
        // (nor a lens: its shade instances are the general ones' twins, C37)
        // (nor a sky other than DEFAULT: its shade instances are the general ones' too, C42)
        ctx->wb.lean = (!regen && ctx->lean_scene && !ctx->no_lean && !R.subs && !lens && !emit && !sky) ? 1u : 0u;
        const int grid_shade = grid_shade_of(shade_mode(regen, ctx->wb.lean != 0u));
        // the seed writes its camera rays as 16-B records (store_cam_ray) when every item has its pixel: the first
        // extend (cam) and shade (first = 2) decode them
        // (lens rays have origins of their own: the lens seed writes full records, first = 1)
        const bool cam_rec = !regen && !lens && ((Rc.W | Rc.H) & (kTile - 1u)) == 0u;
        // the first extend of a grouped chunk over camera records refills by a threshold of its own (OCTPT_REFILL_FIRST,
        // else the instance's default; 0 and every other launch: ctx->refill, the adaptive rule unless OCTPT_REFILL
        // is set).  The seed left each wave's 64 positions one pixel's samples (G = 64), which walk in step: a wave
        // that waits for (nearly) all of them keeps its lanes in one iteration kind, where the adaptive rule's 16
        // mixes the next pixel's rays in within one ray length
        uint32_t refill_first = 0u;
        if (Rc.group_shift != 0u && cam_rec)
            refill_first = ctx->refill_first >= 0 ? (uint32_t)ctx->refill_first
                           : (ctx->S.has_blocks || ctx->S.has_models) ? 0u
                           : ctx->S.has_cuboids ? kRefillFirstBoxes : kRefillFirstSpheres;
        if (std::getenv("OCTPT_DEBUG"))  // (tests/test_gpu_sample_group.py and test_gpu_group_refill.py read this line)
            std::fprintf(stderr, "octpt: chunk of %u samples, sample group %u, first-launch refill %u\n", Rc.spp_count,
                         1u << Rc.group_shift, refill_first);
        HIP_TRY(ctx, launch_wf_seed(C, Rc, B, n_seed, chunk_items, ctx->d_stats, s));
        for (uint32_t it = 0;; ++it) {
            if (cancel && cancel->load()) return fail(ctx, OCTPT_CANCELLED, "render cancelled");
            const uint32_t q = it & 1u;
            EventPair ev{};
            if ((st = ktimer_begin(ctx, s, ev)) != OCTPT_OK) return st;
            HIP_TRY(ctx, launch_wf_extend(ctx->S, B, q, it == 0u && cam_rec,
                                          it == 0u && refill_first ? refill_first : ctx->refill, grid_extend,
                                          ctx->d_stats, s));
            if ((st = ktimer_end(ctx, s, 0, ev)) != OCTPT_OK) return st;
            if ((st = ktimer_begin(ctx, s, ev)) != OCTPT_OK) return st;
            HIP_TRY(ctx, launch_wf_shade(Se, C, Rc, B, q, chunk_items, it == 0u ? (cam_rec ? 2u : 1u) : 0u,
                                         regen, grid_shade, ctx->d_stats, s, emit, sky, dist));
            if ((st = ktimer_end(ctx, s, 1, ev)) != OCTPT_OK) return st;
            // snapshot of the queue iteration `it` produced; the host checks the snapshot of
            // iteration it - kLookahead, so the GPU always has kLookahead iterations queued (an
            // iteration over an empty queue exits at once).  The queue only empties once every
            // chunk item is claimed: finished paths regenerate in the same shade pass.
            const uint32_t slot = it % (kLookahead + 1);
            HIP_TRY(ctx, launch_wf_snapshot(B, q ^ 1u, ctx->d_count + slot * kCountSpan, s));
            HIP_TRY(ctx, hipEventRecord(ctx->count_ev[slot], s));
            if (it >= kLookahead) {
                const uint32_t old = (it - kLookahead) % (kLookahead + 1);
                HIP_TRY(ctx, hipEventSynchronize(ctx->count_ev[old]));
                const uint32_t *h = ctx->h_count + old * kCountSpan;  // that iteration's shade's queue, items
                uint64_t queued = 0;
                for (uint32_t k = 0; k < kSegs; ++k) queued += h[k];
                if (queued == 0u) break;  // iteration it - kLookahead + 1 onwards had nothing to do
                // Drain: every chunk item claimed and few rays left, so the queue only shrinks from
                // here (a ray yields at most one ray, and nothing regenerates).  One launch finishes the
                // paths in the queue this iteration's shade filled instead of the launch-latency-bound
                // tail of near-empty iterations.  Not in the extend timer (rocprof reports it as
                // wf_drain_kernel); its statistics (<= 4096 paths) stay in the totals.
                // (not for block-model scenes: their tails are transparent-texel chains, C5 -1 %)
                if (queued <= ctx->drain_rays && (!ctx->S.has_models || ctx->drain_models)) {
                    bool exhausted = true;
                    for (uint32_t k = 0; k < kSegs && exhausted; ++k) {
                        const uint32_t lo = (uint32_t)(((uint64_t)k * chunk_items) / kSegs);
                        const uint32_t hi = (uint32_t)(((uint64_t)(k + 1u) * chunk_items) / kSegs);
                        exhausted = h[kSegs + k] >= hi - lo;
                    }
                    if (exhausted) {
                        // one path per wave (wf_drain_kernel), four waves per block
                        const int grid = (int)std::min<uint64_t>((queued + 3) / 4 + 1, (uint64_t)ctx->num_cu * 16u);
                        HIP_TRY(ctx, launch_wf_drain(Se, Rc, B, q ^ 1u, grid, ctx->d_stats, s, emit, sky, dist));
                        break;
                    }
                }
            }
        }
        HIP_TRY(ctx, launch_wf_resolve(Rc, B, Rc.spp_count, d_accum, d_seg, d_moments, clamp, s));
    }
    return OCTPT_OK;
}

}  // namespace

octpt_status octpt::enqueue_render(octpt_ctx *ctx, const DevRender &R, float4 *d_accum, uint32_t *d_seg, hipStream_t s,
                                   bool megakernel, const std::atomic<bool> *cancel, float2 *d_moments, uint64_t list) {
    if (R.spp_count == 0 || R.total_items == 0) return OCTPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    EventPair ev{};
    HIP_TRY(ctx, hipEventCreate(&ev.start));
    HIP_TRY(ctx, hipEventCreate(&ev.stop));
    ctx->pending.push_back(ev);  // destroyed by get_stats / destroy
    HIP_TRY(ctx, hipEventRecord(ev.start, s));
    octpt_status st = OCTPT_OK;
    if (R.preview) {
        const hipError_t e = launch_preview(ctx->S, ray_source_camera(ctx), R, d_accum, d_seg, ctx->d_stats, s,
                                            ctx->sky.mode != kSkyDefault ? &ctx->sky : nullptr);
        if (e != hipSuccess) st = hip_fail(ctx, e, "preview launch");
    } else {
        st = megakernel ? enqueue_megakernel(ctx, R, d_accum, d_seg, s)
                        : enqueue_wavefront(ctx, R, d_accum, d_seg, s, cancel, d_moments, list);
    }
    HIP_TRY(ctx, hipEventRecord(ev.stop, s));
    if (st == OCTPT_OK) ctx->launches++;
    return st;
}

// ---------------- multi-device contexts (octpt_create_multi) ----------------
// A multi-device context forwards every call to one child context per device entry, each a complete
// single-device context (its own scene replica, stream and wavefront state).  A render deals the caller's
// 8x8 tiles round-robin over the entries (multi_slot: the children's own shards of the kernels' tile
// split), runs each child on a host thread of its own (the wavefront loop is host-steered), and moves the
// tiles between the caller's buffers on the first device and the children's compact buffers with peer
// copies (hipMemcpyPeerAsync: xGMI DMA between MI355X devices; a plain device copy when an entry repeats
// a device).  Per-pixel RNG streams make the result bit-identical to one device's.
namespace {

// fn(i) for every child i, one host thread each; the first failing entry's status and message are returned
template <class F>
octpt_status for_each_sub(octpt_ctx *ctx, F fn) {
    const size_t n = ctx->sub.size();
    std::vector<octpt_status> st(n, OCTPT_OK);
    std::vector<std::thread> th;
    th.reserve(n);
    for (size_t i = 0; i < n; ++i)
        th.emplace_back([&st, &fn, ctx, i]() {
            try {
                st[i] = fn(i);
            } catch (...) {
                st[i] = fail(ctx->sub[i], OCTPT_ERR_INTERNAL, "unexpected exception");
            }
        });
    for (auto &t : th) t.join();
    for (size_t i = 0; i < n; ++i)
        if (st[i] != OCTPT_OK)
            return fail(ctx, st[i], "device entry " + std::to_string(i) + " (HIP device " +
                                        std::to_string(ctx->sub[i]->device) + "): " + ctx->sub[i]->err);
    return OCTPT_OK;
}

// One render call over every device entry: scatter the caller's running mean (and segment counts) into the
// entries' compact tile buffers, render each entry's shard, gather back.  R is the call's layout (on the
// first device, stream s); the caller's buffers are read and written on s, the entries work on their own
// streams.  kernel_ms accumulates the call's wall time (the entries run concurrently).
octpt_status multi_render(octpt_ctx *ctx, const octpt_render_params &p, const DevRender &R, float4 *d_accum,
                          uint32_t *d_seg, hipStream_t s, const std::atomic<bool> *cancel) {
    if (R.spp_count == 0 || R.total_items == 0) return OCTPT_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)ctx->sub.size();
    const size_t stride = (size_t)((R.shard_tiles + n - 1) / n) * 64u;  // the largest entry's pixels
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    octpt_status st = grow_buf(ctx, ctx->m_acc, stride * n);
    if (st == OCTPT_OK && d_seg) st = grow_buf(ctx, ctx->m_seg, stride * n);
    if (st != OCTPT_OK) return st;
    HIP_TRY(ctx, launch_multi_stage(R, n, (uint32_t)stride, d_accum, d_seg, ctx->m_acc.p, ctx->m_seg.p, true, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const bool megakernel = (p.flags & OCTPT_RENDER_MEGAKERNEL) != 0;
    st = for_each_sub(ctx, [&](size_t i) -> octpt_status {
        octpt_ctx *c = ctx->sub[i];
        HIP_TRY(c, hipSetDevice(c->device));
        octpt_render_params pi = p;  // entry i's shard of the caller's shard (multi_slot)
        pi.shard_index = p.shard_index + (uint32_t)i * p.shard_count;
        pi.shard_count = p.shard_count * n;
        pi.flags |= OCTPT_RENDER_SHARD_COMPACT;
        DevRender Ri{};
        octpt_status r = make_render(c, &pi, Ri);
        if (r != OCTPT_OK || Ri.total_items == 0) return r;
        const size_t np = Ri.total_items;
        if ((r = grow_buf(c, c->m_acc, np)) != OCTPT_OK) return r;
        if (d_seg && (r = grow_buf(c, c->m_seg, np)) != OCTPT_OK) return r;
        float4 *stage_acc = ctx->m_acc.p + i * stride;
        uint32_t *stage_seg = d_seg ? ctx->m_seg.p + i * stride : nullptr;
        HIP_TRY(c, hipMemcpyPeerAsync(c->m_acc.p, c->device, stage_acc, ctx->device, np * sizeof(float4), c->stream));
        if (d_seg) HIP_TRY(c, hipMemcpyPeerAsync(c->m_seg.p, c->device, stage_seg, ctx->device, np * 4, c->stream));
        r = enqueue_render(c, Ri, c->m_acc.p, d_seg ? c->m_seg.p : nullptr, c->stream, megakernel, cancel);
        if (r != OCTPT_OK) {
            (void)hipStreamSynchronize(c->stream);
            return r;
        }
        HIP_TRY(c, hipMemcpyPeerAsync(stage_acc, ctx->device, c->m_acc.p, c->device, np * sizeof(float4), c->stream));
        if (d_seg) HIP_TRY(c, hipMemcpyPeerAsync(stage_seg, ctx->device, c->m_seg.p, c->device, np * 4, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return OCTPT_OK;
    });
    if (st != OCTPT_OK) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_multi_stage(R, n, (uint32_t)stride, d_accum, d_seg, ctx->m_acc.p, ctx->m_seg.p, false, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->kernel_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->launches++;
    return OCTPT_OK;
}

}  // namespace

void octpt::join_inflight(octpt_ctx *ctx) {
    octpt_frame *f = ctx->inflight;
    if (f && f->worker.joinable()) f->worker.join();
    ctx->inflight = nullptr;
}

namespace {

void free_frame_buffers(octpt_frame *f) {
    if (f->d_accum) (void)hipFree(f->d_accum);
    if (f->d_rgba) (void)hipFree(f->d_rgba);
    if (f->h_accum) (void)hipHostFree(f->h_accum);
    if (f->h_rgba) (void)hipHostFree(f->h_rgba);
    f->d_accum = nullptr;
    f->d_rgba = nullptr;
    f->h_accum = nullptr;
    f->h_rgba = nullptr;
}

void deliver(octpt_frame *f) {
    if (f->delivered) return;
    std::memcpy(f->user_accum, f->h_accum, f->n_pixels * 16);
    if (f->user_rgba) std::memcpy(f->user_rgba, f->h_rgba, f->n_pixels * 4);
    f->delivered = true;
}

// what build_block_octree_gpu's error word says (kCellErr*): the cells octpt_build_block_octree refuses,
// and for a scene a block id beyond its block table
octpt_status cell_error(octpt_ctx *ctx, uint32_t errors) {
    if (errors & kCellErrRange) return fail(ctx, OCTPT_ERR_INVALID_ARG, "a cell coordinate is >= 2^depth");
    if (errors & kCellErrBlockId) return fail(ctx, OCTPT_ERR_INVALID_ARG, "a cell's block id is >= 2^27");
    if (errors & kCellErrBlockTable)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "a cell's block id is out of range of the block table");
    if (errors & kCellErrPalette)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "a section's palette slice is empty, > 4096 entries or leaves the palette");
    if (errors & kCellErrIndexBlock)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "a section's index_first is not a multiple of 4096 or is past index_count");
    if (errors & kCellErrUniform)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "a uniform section needs palette_count == 1");
    if (errors & kCellErrPaletteIndex)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "a section index is >= its palette_count");
    return fail(ctx, OCTPT_ERR_INVALID_ARG, "two cells at one position");
}

// the argument checks the two device section builds share (after the NULL-context check and join_inflight)
octpt_status check_section_build_args(octpt_ctx *ctx, const octpt_section_world *w, uint32_t depth, uint32_t flags) {
    if (flags & ~(OCTPT_BUILD_COMPACT | OCTPT_BUILD_SECTIONS_ON_DEVICE))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "unknown build flags");
    const octpt_status st = section_world_status(w, depth);
    if (st == OCTPT_ERR_OOM) return fail(ctx, st, "more than 2^31 sections");
    if (st != OCTPT_OK)
        return fail(ctx, st, "section world: NULL, depth outside [4, 21], a NULL array or index_count not a multiple of 4096");
    if ((flags & OCTPT_BUILD_SECTIONS_ON_DEVICE) && is_multi(ctx))
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "device sections live on one device: not on a multi-device context");
    return OCTPT_OK;
}

// the argument checks the two device block builds share (after the NULL-context check and join_inflight)
octpt_status check_block_build_args(octpt_ctx *ctx, const uint32_t *cells, uint32_t cell_count, uint32_t flags) {
    if (flags & ~(OCTPT_BUILD_COMPACT | OCTPT_BUILD_CELLS_ON_DEVICE))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "unknown build flags");
    if (cell_count && !cells) return fail(ctx, OCTPT_ERR_INVALID_ARG, "cells is NULL");
    if (cell_count > kMaxBuildPairs) return fail(ctx, OCTPT_ERR_OOM, "more than 2^31 cells");
    if ((flags & OCTPT_BUILD_CELLS_ON_DEVICE) && is_multi(ctx))
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "device cells live on one device: not on a multi-device context");
    return OCTPT_OK;
}

// what a device builder returned, as the entry's status: `what` names the build in a HIP failure's message, too_many_msg
// is the entry's own text for a world past the pair / cell cap
octpt_status build_status(octpt_ctx *ctx, hipError_t e, uint32_t errors, bool too_many, const char *what,
                          const char *too_many_msg) {
    if (e != hipSuccess) return hip_fail(ctx, e, what);
    if (errors) return cell_error(ctx, errors);
    if (too_many) return fail(ctx, OCTPT_ERR_OOM, too_many_msg);
    return OCTPT_OK;
}

// The three device builders behind their two kinds of entry: dev == nullptr downloads the octree into `out` (the
// octpt_build_*_device entries), else it stays in the build scratch as *dev (the octpt_scene_build_*_device entries).
// block_count: the scene's block table size, 0 = not checked.
octpt_status run_prim_build(octpt_ctx *ctx, const octpt_sphere *spheres, uint32_t ns, const octpt_cuboid *cuboids,
                            uint32_t nc, uint32_t depth, uint32_t flags, BuiltOctree &out, DeviceOctree *dev,
                            float &ms) {
    bool too_many = false;
    const hipError_t e = build_octree_gpu(ctx->stream, ctx->build_scratch, spheres, ns, cuboids, nc, depth,
                                          (flags & OCTPT_BUILD_COMPACT) != 0, kMaxBuildPairs, out, too_many, &ms, dev);
    // too many pairs reads as the device running out of memory does (hip_fail: the same status and text)
    return build_status(ctx, e, 0u, too_many, "octree build", "octree build: out of memory");
}

octpt_status run_block_build(octpt_ctx *ctx, const uint32_t *cells, uint32_t n, uint32_t depth, uint32_t flags,
                             uint32_t block_count, BuiltOctree &out, DeviceOctree *dev, float &ms) {
    uint32_t errors = 0u;
    const hipError_t e = build_block_octree_gpu(ctx->stream, ctx->build_scratch, cells, n,
                                                (flags & OCTPT_BUILD_CELLS_ON_DEVICE) != 0, depth,
                                                (flags & OCTPT_BUILD_COMPACT) != 0, block_count, out, errors, &ms, dev);
    return build_status(ctx, e, errors, false, "block octree build", "");
}

octpt_status run_section_build(octpt_ctx *ctx, const octpt_section_world *world, uint32_t depth, uint32_t flags,
                               uint32_t block_count, BuiltOctree &out, DeviceOctree *dev, float &ms) {
    uint32_t errors = 0u;
    bool too_many = false;
    const hipError_t e = build_section_octree_gpu(ctx->stream, ctx->build_scratch, *world,
                                                  (flags & OCTPT_BUILD_SECTIONS_ON_DEVICE) != 0, depth,
                                                  (flags & OCTPT_BUILD_COMPACT) != 0, block_count, kMaxBuildPairs, out,
                                                  errors, too_many, &ms, dev);
    return build_status(ctx, e, errors, too_many, "section octree build", "more than 2^31 cells");
}

// The frame of the octpt_build_*_device entries after their argument checks: build(octree, ms) selects the device and
// runs its builder into the new handle; `what` names the build in the messages.
template <class Build>
octpt_status build_octree_handle(octpt_ctx *ctx, octpt_octree **out, const char *what, Build build) {
    try {
        std::unique_ptr<octpt_octree> t(new octpt_octree());
        float ms = 0.0f;
        const octpt_status st = build(*t, ms);
        if (st != OCTPT_OK) return st;
        ctx->build_ms = ms;
        *out = t.release();
        return OCTPT_OK;
    } catch (const std::bad_alloc &) {
        return fail(ctx, OCTPT_ERR_OOM, std::string(what) + ": host out of memory");
    } catch (...) {
        return fail(ctx, OCTPT_ERR_INTERNAL, std::string("unexpected exception in ") + what);
    }
}

// The emitter grid of the context's scene and setting (C38): built on the device when strategy ONE and a block-value
// scene are both known, dropped else.  A single-device context's, with its device current and its stream idle.
octpt_status refresh_emitter_grid(octpt_ctx *ctx) {
    drop_emitter_grid(ctx);
    if (ctx->emit_strategy != OCTPT_EMITTERS_ONE || !ctx->has_scene || !ctx->S.has_blocks) return OCTPT_OK;
    if (ctx->emit_grid_size > (1u << ctx->S.depth))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "the emitter grid's grid_size exceeds the world's 2^depth");
    uint32_t shift = 0;
    while ((1u << shift) < ctx->emit_grid_size) ++shift;
    // model emitters (C39): the table goes to the device with the first such grid of the scene
    const bool models = (ctx->emit_flags & OCTPT_EMITTERS_MODELS) != 0u;
    if (models && ctx->model_emissive.size() > 0x7FFFFFFFull)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "OCTPT_EMITTERS_MODELS: more than 2^31 - 1 models");
    if (models && !ctx->d_model_first) {
        const EmissiveModelTable &t = ctx->emit_models;
        const uint32_t none = 0u;  // a scene without models: first[] = {0}
        hipError_t eu = t.first.empty() ? upload(ctx, &none, 1, &ctx->d_model_first)
                                        : upload(ctx, t.first.data(), t.first.size(), &ctx->d_model_first);
        if (eu == hipSuccess) eu = upload(ctx, t.quad.data(), t.quad.size(), &ctx->d_model_quad);
        if (eu == hipSuccess) eu = upload(ctx, t.cum.data(), t.cum.size(), &ctx->d_model_cum);
        if (eu == hipSuccess) eu = upload(ctx, t.ouv.data(), t.ouv.size(), &ctx->d_model_ouv);
        if (eu != hipSuccess) {
            (void)hipGetLastError();
            ctx->d_model_first = nullptr;  // (the allocations made stay the scene's and go with it)
            return hip_fail(ctx, eu, "emissive-model table upload");
        }
    }
    octpt_status refusal = OCTPT_OK;
    const hipError_t e = build_emitter_grid_gpu(ctx->stream, ctx->build_scratch, ctx->S, ctx->block_emissive.data(), shift,
                                                ctx->emit_grid, refusal, models ? ctx->model_emissive.data() : nullptr,
                                                models ? (uint32_t)ctx->model_emissive.size() : 0u);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hip_fail(ctx, e, "emitter grid build");
    }
    if (refusal == OCTPT_ERR_OOM)
        return fail(ctx, OCTPT_ERR_OOM, "the emitter grid exceeds its budget (2^24 emitters, 2^28 list entries, 2^28 cells)");
    if (refusal != OCTPT_OK) return fail(ctx, refusal, "emitter grid build: the scene holds more octants than it counts");
    ctx->emit_grid.flags = ctx->emit_flags;
    ctx->grid_valid = true;
    return OCTPT_OK;
}

// a scene is set: its grid with it; a scene whose grid cannot be built is not kept
octpt_status commit_scene(octpt_ctx *ctx, const DevScene &S) {
    ctx->S = S;
    ctx->has_scene = true;
    ++ctx->scene_gen;
    const octpt_status st = refresh_emitter_grid(ctx);
    if (st != OCTPT_OK) {
        const std::string msg = ctx->err;
        free_scene(ctx);
        ctx->err = msg;
    }
    return st;
}

// a scene entry on a multi-device context: entry(child) makes a replica on every device entry
template <class F>
octpt_status scene_on_every_sub(octpt_ctx *ctx, F entry) {
    ctx->has_scene = false;
    const octpt_status st = for_each_sub(ctx, [&](size_t i) { return entry(ctx->sub[i]); });
    ctx->has_scene = st == OCTPT_OK;
    return st;
}

// The device scene of an octree the builder left in the scratch, either leaf kind: its octants packed into the node
// slots in place, exactly as octpt_scene_upload packs them on the host (§5), and the tables uploaded.  A block-value
// scene's primitive tables are the empty ones it has after octpt_scene_upload (one zeroed element each: its
// primitive counts are 0).  Its slots need no table, so they are filled, and the root's mask read, before the
// tables are allocated; a primitive scene's fill writes the tables and comes after them.
octpt_status pack_device_scene(octpt_ctx *ctx, const octpt_scene_desc *d, const DeviceOctree &t) {
    if ((uint64_t)t.n_octants * 8u >= 0xFFFFFFF0ull)  // the u32 slot scan cannot wrap
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "octree too large for the device build (>= 2^29 octants)");
    uint32_t *d_base = nullptr, n_slots = 0;
    HIP_TRY(ctx, slot_bases_gpu(ctx->stream, ctx->build_scratch, t, &d_base, n_slots));
    uint16_t root_mask = 0;  // the root is octant 0 (pre-order), base 0
    auto read_root_mask = [&] {
        return hipMemcpy(&root_mask, &t.octants[0].child_mask, sizeof root_mask, hipMemcpyDeviceToHost);
    };
    ScenePrimTables out{};
    HIP_TRY(ctx, upload<uint2>(ctx, nullptr, (size_t)n_slots + 8, &out.node_child));  // zeroed: + 8 tail slots
    if (d->blocks) {
        const std::vector<uint32_t> bflags = block_slot_flags(d);
        HIP_TRY(ctx, fill_block_scene_gpu(ctx->stream, ctx->build_scratch, t, d_base, bflags.data(), d->block_count,
                                          out.node_child));
        HIP_TRY(ctx, read_root_mask());
    } else if (!d->cuboid_count) {
        HIP_TRY(ctx, upload<float4>(ctx, nullptr, (size_t)n_slots + 8, &out.leaf_sph));
    }
    HIP_TRY(ctx, upload<uint32_t>(ctx, nullptr, t.n_leaf_prims, &out.leaf_prims));
    HIP_TRY(ctx, upload<float4>(ctx, nullptr, d->sphere_count, &out.spheres));
    HIP_TRY(ctx, upload<uint32_t>(ctx, nullptr, d->sphere_count, &out.sphere_mat));
    HIP_TRY(ctx, upload<float4>(ctx, nullptr, d->cuboid_count, &out.cub_a));
    HIP_TRY(ctx, upload<float2>(ctx, nullptr, d->cuboid_count, &out.cub_b));
    HIP_TRY(ctx, upload<uint32_t>(ctx, nullptr, (size_t)d->cuboid_count * 6, &out.cub_mat));
    if (!d->blocks) {
        HIP_TRY(ctx, fill_scene_gpu(ctx->stream, t, d_base, out));
        HIP_TRY(ctx, read_root_mask());
    }
    DevScene S{};
    S.node_child = out.node_child;
    S.leaf_sph = out.leaf_sph;
    S.leaf_prims = out.leaf_prims;
    S.spheres = out.spheres;
    S.sphere_mat = out.sphere_mat;
    S.cub_a = out.cub_a;
    S.cub_b = out.cub_b;
    S.cub_mat = out.cub_mat;
    S.root = 0u;
    S.root_mask = root_mask;
    S.n_octants = t.n_octants;
    const octpt_status st = upload_tables(ctx, d, false, S);
    if (st != OCTPT_OK) return st;
    return commit_scene(ctx, S);
}

// The three octpt_scene_build_*_device entries after their argument checks.  blocks: the entry builds a block-value
// scene, else a primitive one (whose pair bound can only be taken once the scene's tables are checked, so it is
// refused here).  build(ctx, octree, ms) runs the entry's builder with its result left in the build scratch; on a
// multi-device context every device entry runs it for its own replica.  `what` names the entry in the message of
// an unexpected exception.
template <class Build>
octpt_status build_scene_device(octpt_ctx *ctx, const octpt_scene_desc *d, bool blocks, const char *what, Build build) {
    try {
        if (is_multi(ctx))
            return scene_on_every_sub(ctx, [&](octpt_ctx *c) { return build_scene_device(c, d, blocks, what, build); });
        octpt_status st = validate_head(ctx, d, false);
        if (st != OCTPT_OK) return st;
        if (blocks && !d->blocks)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "the block build needs the scene's block table (blocks is NULL)");
        if (!blocks && d->blocks)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "a block-value scene is uploaded with its octree");
        st = validate_tables(ctx, d);
        if (st != OCTPT_OK) return st;
        if (!blocks && pair_bound(d->spheres, d->sphere_count, d->cuboids, d->cuboid_count, d->depth) > kMaxBuildPairs)
            return fail(ctx, OCTPT_ERR_OOM, "more than 2^31 (cell, primitive) pairs");
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        free_scene(ctx);
        DeviceOctree t;
        float ms = 0.0f;
        st = build(ctx, t, ms);
        if (st != OCTPT_OK) return st;
        ctx->build_ms = ms;
        return pack_device_scene(ctx, d, t);
    } catch (const std::bad_alloc &) {
        free_scene(ctx);
        return fail(ctx, OCTPT_ERR_OOM, "host allocation failed");
    } catch (...) {
        free_scene(ctx);
        return fail(ctx, OCTPT_ERR_INTERNAL, std::string("unexpected exception in ") + what);
    }
}

}  // namespace

extern "C" {

uint32_t octpt_abi_version(void) { return OCTPT_ABI_VERSION; }

int32_t octpt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

octpt_status octpt_create(int32_t device, octpt_ctx **out) {
    if (!out) return OCTPT_ERR_INVALID_ARG;
    *out = nullptr;
    octpt_ctx *ctx = new (std::nothrow) octpt_ctx();
    if (!ctx) return OCTPT_ERR_OOM;
    auto bail = [&](octpt_status st) {
        octpt_destroy(ctx);
        return st;
    };
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return bail(OCTPT_ERR_DEVICE);
    if (device < 0 || device >= n) return bail(OCTPT_ERR_INVALID_ARG);
    hipDeviceProp_t prop{};
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return bail(OCTPT_ERR_DEVICE);
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return bail(OCTPT_ERR_DEVICE);
    ctx->device = device;
    ctx->num_cu = prop.multiProcessorCount;
    ctx->pool_cap = std::max<uint32_t>(std::min<uint32_t>(env_u32("OCTPT_POOL", kDefaultPool), kMaxPool), 64u);
    ctx->chunk_cap = std::min<uint64_t>(env_u32("OCTPT_CHUNK", (uint32_t)kDefaultChunkPaths), kMaxChunkPaths);
    // OCTPT_REFILL=n fixes the threshold (clamped to [1, 64]); unset: adaptive per wave (0)
    const char *refill_env = std::getenv("OCTPT_REFILL");
    ctx->refill = (refill_env && *refill_env)
                      ? std::max<uint32_t>(std::min<uint32_t>(env_u32("OCTPT_REFILL", 16u), 64u), 1u)
                      : kDefaultRefill;
    // OCTPT_DRAIN_RAYS=n: the drain's queue threshold; 0 turns the drain off (A/B)
    const char *drain_env = std::getenv("OCTPT_DRAIN_RAYS");
    if (drain_env && *drain_env) ctx->drain_rays = (uint32_t)std::strtoul(drain_env, nullptr, 10);
    const char *beam_env = std::getenv("OCTPT_BEAM");
    ctx->beam = !(beam_env && beam_env[0] == '0');
    const char *lean_env = std::getenv("OCTPT_LEAN");
    ctx->no_lean = lean_env && lean_env[0] == '0';
    ctx->sample_group = std::min(env_u32("OCTPT_SAMPLE_GROUP", kDefaultSampleGroup), 64u);
    const char *group_env = std::getenv("OCTPT_SAMPLE_GROUP");
    ctx->sample_group_set = group_env && *group_env;  // set: that G at most in every chunk (A/B, tests)
    // OCTPT_REFILL_FIRST=n: the first-launch threshold of a grouped chunk (clamped to 64); 0: the adaptive rule
    const char *first_env = std::getenv("OCTPT_REFILL_FIRST");
    if (first_env && *first_env) ctx->refill_first = (int32_t)std::min<unsigned long>(std::strtoul(first_env, nullptr, 10), 64ul);
    ctx->drain_models = env_u32("OCTPT_DRAIN_MODELS", 0u) != 0u;
    ctx->mem_limit = (size_t)env_u32("OCTPT_DEVICE_MEM_LIMIT", 0u) << 20;  // MiB, test hook (ensure_wave)
    if (hipSetDevice(device) != hipSuccess) return bail(OCTPT_ERR_DEVICE);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return bail(OCTPT_ERR_DEVICE);
    if (hipMalloc(&ctx->d_counters, kCounterRing * sizeof(uint32_t)) != hipSuccess) return bail(OCTPT_ERR_OOM);
    if (hipMalloc(&ctx->d_stats, kStatWords * sizeof(unsigned long long)) != hipSuccess) return bail(OCTPT_ERR_OOM);
    if (hipMemset(ctx->d_stats, 0, kStatWords * sizeof(unsigned long long)) != hipSuccess) return bail(OCTPT_ERR_DEVICE);
    float lf[256];
    uint8_t lb[256];
    make_luts(lf, lb);
    if (hipMalloc(&ctx->d_lut_float, sizeof lf) != hipSuccess) return bail(OCTPT_ERR_OOM);
    if (hipMalloc(&ctx->d_lut_byte, sizeof lb) != hipSuccess) return bail(OCTPT_ERR_OOM);
    if (hipMemcpy(ctx->d_lut_float, lf, sizeof lf, hipMemcpyHostToDevice) != hipSuccess) return bail(OCTPT_ERR_DEVICE);
    if (hipMemcpy(ctx->d_lut_byte, lb, sizeof lb, hipMemcpyHostToDevice) != hipSuccess) return bail(OCTPT_ERR_DEVICE);
    *out = ctx;
    return OCTPT_OK;
}

octpt_status octpt_create_multi(const int32_t *devices, uint32_t n, octpt_ctx **out) {
    if (!out) return OCTPT_ERR_INVALID_ARG;
    *out = nullptr;
    if (!devices || n == 0 || n > 64) return OCTPT_ERR_INVALID_ARG;
    if (n == 1) return octpt_create(devices[0], out);
    int caller_device = 0;
    const bool restore = hipGetDevice(&caller_device) == hipSuccess;
    struct Restore {  // the calling thread's current device is left as it was
        bool on;
        int dev;
        ~Restore() {
            if (on) (void)hipSetDevice(dev);
        }
    } restore_device{restore, caller_device};
    try {
        octpt_ctx *ctx = nullptr;
        octpt_status st = octpt_create(devices[0], &ctx);  // the first entry's device holds the caller's buffers
        if (st != OCTPT_OK) return st;
        for (uint32_t i = 0; i < n && st == OCTPT_OK; ++i) {
            octpt_ctx *c = nullptr;
            st = octpt_create(devices[i], &c);
            if (st == OCTPT_OK) ctx->sub.push_back(c);
        }
        if (st != OCTPT_OK) {
            octpt_destroy(ctx);
            return st;
        }
        // direct peer access between the first device and every other one (xGMI); without it the peer
        // copies still work, staged by the runtime.  A pair that cannot be enabled is not an error, but it is
        // recorded: octpt_last_error then reads "note: peer access ..." 
        std::string note;
        auto enable = [&](int from, int to) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, from, to) != hipSuccess || !can) {
                note += " " + std::to_string(from) + "->" + std::to_string(to) + ": no peer path";
                return;
            }
            if (hipSetDevice(from) != hipSuccess) return;
            const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                note += " " + std::to_string(from) + "->" + std::to_string(to) + ": " + hipGetErrorString(e);
            (void)hipGetLastError();
        };
        for (uint32_t i = 1; i < n; ++i) {
            if (devices[i] == devices[0]) continue;
            enable(devices[0], devices[i]);
            enable(devices[i], devices[0]);
        }
        if (!note.empty()) ctx->err = "note: peer access not enabled (copies staged by the runtime):" + note;
        *out = ctx;
        return OCTPT_OK;
    } catch (...) {
        return OCTPT_ERR_INTERNAL;
    }
}

uint32_t octpt_device_entries(const octpt_ctx *ctx) { return !ctx ? 0u : is_multi(ctx) ? (uint32_t)ctx->sub.size() : 1u; }

void octpt_destroy(octpt_ctx *ctx) {
    if (!ctx) return;
    join_inflight(ctx);
    for (octpt_ctx *c : ctx->sub) octpt_destroy(c);
    ctx->sub.clear();
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto &e : ctx->pending) {
        (void)hipEventSynchronize(e.stop);
        (void)hipEventDestroy(e.start);
        (void)hipEventDestroy(e.stop);
    }
    for (auto &ke : ctx->kpending) ctx->ev_pool.push_back(ke.second);
    for (auto &e : ctx->ev_pool) {
        (void)hipEventSynchronize(e.stop);
        (void)hipEventDestroy(e.start);
        (void)hipEventDestroy(e.stop);
    }
    free_scene(ctx);
    free_wave(ctx);
    if (ctx->d_emit_hdr) (void)hipFree(ctx->d_emit_hdr);
    if (ctx->sky_map) (void)hipFree(ctx->sky_map);
    if (ctx->sky_dist.row_cdf) (void)hipFree(ctx->sky_dist.row_cdf);
    if (ctx->sky_dist.col_cdf) (void)hipFree(ctx->sky_dist.col_cdf);
    ctx->build_scratch.release();
    if (ctx->h_count) (void)hipHostFree(ctx->h_count);
    for (auto &ev : ctx->count_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->d_counters) (void)hipFree(ctx->d_counters);
    if (ctx->beam_ev) (void)hipEventDestroy(ctx->beam_ev);
    if (ctx->d_order) (void)hipFree(ctx->d_order);
    if (ctx->d_order_pos) (void)hipFree(ctx->d_order_pos);
    free_bufs(ctx->d_subs, ctx->d_beam, ctx->d_tiles, ctx->d_tile_spp, ctx->d_tile_err, ctx->d_tile_spread, ctx->fin_normal,
              ctx->fin_albedo, ctx->fin_depth, ctx->fin_var, ctx->m_acc, ctx->m_seg, ctx->dn_frame[0], ctx->dn_frame[1]);
    if (ctx->d_stats) (void)hipFree(ctx->d_stats);
    if (ctx->d_lut_float) (void)hipFree(ctx->d_lut_float);
    if (ctx->d_lut_byte) (void)hipFree(ctx->d_lut_byte);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *octpt_last_error(const octpt_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

octpt_status octpt_scene_upload(octpt_ctx *ctx, const octpt_scene_desc *d) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    join_inflight(ctx);
    try {  // (not guarded(): the handlers drop the half-made scene, here and in build_scene_device)
        if (is_multi(ctx)) return scene_on_every_sub(ctx, [&](octpt_ctx *c) { return octpt_scene_upload(c, d); });
        std::vector<uint16_t> masks;  // reader-form child masks (C21)
        octpt_status st = validate_scene(ctx, d, masks);
        if (st != OCTPT_OK) return st;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        free_scene(ctx);
        DevScene S{};
        // sparse packed child slots: octant n's present children are stored
        // contiguously from base[n] in child order; child i is at base[n] + popcount(mask & (2^i - 1)).
        // One 8-byte load per descend / leaf visit yields the child's own base and mask.
        std::vector<uint32_t> base(d->octant_count);
        size_t n_slots = 0;
        for (uint32_t n = 0; n < d->octant_count; ++n) {
            base[n] = (uint32_t)n_slots;
            n_slots += (size_t)__builtin_popcount(masks[n] & 0xFFu);
        }
        if (n_slots >= 0xFFFFFFFFull) return fail(ctx, OCTPT_ERR_INVALID_ARG, "octree too large");
        // + 8 zero slots: a child index computed for an absent child of the last octant stays in bounds
        std::vector<uint2> child(n_slots + 8, make_uint2(0u, 0u));
        const std::vector<uint32_t> bflags = d->blocks ? block_slot_flags(d) : std::vector<uint32_t>();
        for (uint32_t n = 0; n < d->octant_count; ++n) {
            const octpt_octant &o = d->octants[n];
            uint32_t k = base[n];
            for (int i = 0; i < 8; ++i) {
                const bool present = (masks[n] >> i) & 1, leaf = (masks[n] >> (i + 8)) & 1;
                if (!present) continue;
                const uint32_t v = o.children[i];
                if (!leaf) {
                    child[k++] = make_uint2(base[v], masks[v]);
                } else if (d->blocks) {  // block-value leaf (C23): (block id, its slot flags)
                    child[k++] = make_uint2(v, bflags[v]);
                } else if (d->leaf_count[v] == 1) {  // single-primitive leaf: the prim id itself
                    child[k++] = make_uint2(d->leaf_prims[d->leaf_first[v]], 1u);
                } else {
                    child[k++] = make_uint2(d->leaf_first[v], d->leaf_count[v]);
                }
            }
        }
        // single-sphere leaf slots carry their sphere in a parallel array, so that extend loads it
        // beside the slot instead of after it (sphere-only scenes)
        std::vector<float4> leaf_sph;
        if (!d->cuboid_count && !d->blocks) {
            leaf_sph.assign(child.size(), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            for (uint32_t n = 0; n < d->octant_count; ++n) {
                const octpt_octant &o = d->octants[n];
                uint32_t k = base[n];
                for (int i = 0; i < 8; ++i) {
                    const bool present = (masks[n] >> i) & 1, leaf = (masks[n] >> (i + 8)) & 1;
                    if (!present) continue;
                    if (leaf && d->leaf_count[o.children[i]] == 1) {
                        const octpt_sphere &x = d->spheres[d->leaf_prims[d->leaf_first[o.children[i]]]];
                        leaf_sph[k] = make_float4(x.center[0], x.center[1], x.center[2], x.radius);
                    }
                    ++k;
                }
            }
        }
        uint2 *d_child;
        HIP_TRY(ctx, upload(ctx, child.data(), child.size(), &d_child));
        float4 *d_leaf_sph = nullptr;
        if (!leaf_sph.empty()) HIP_TRY(ctx, upload(ctx, leaf_sph.data(), leaf_sph.size(), &d_leaf_sph));
        uint32_t *d_prims;
        HIP_TRY(ctx, upload(ctx, d->leaf_prims, d->leaf_prim_count, &d_prims));
        S.node_child = d_child;
        S.leaf_sph = d_leaf_sph;
        S.leaf_prims = d_prims;
        S.root = base[d->root];  // traversal "parent" values are child-array bases
        S.root_mask = masks[d->root];
        S.n_octants = d->octant_count;
        st = upload_tables(ctx, d, true, S);
        if (st != OCTPT_OK) return st;
        return commit_scene(ctx, S);
    } catch (const std::bad_alloc &) {
        free_scene(ctx);
        return fail(ctx, OCTPT_ERR_OOM, "host allocation failed");
    } catch (...) {
        free_scene(ctx);
        return fail(ctx, OCTPT_ERR_INTERNAL, "unexpected exception in scene upload");
    }
}

octpt_status octpt_scene_build_device(octpt_ctx *ctx, const octpt_scene_desc *d, uint32_t flags) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    join_inflight(ctx);
    if (flags & ~OCTPT_BUILD_COMPACT) return fail(ctx, OCTPT_ERR_INVALID_ARG, "unknown build flags");
    return build_scene_device(ctx, d, false, "device scene build", [=](octpt_ctx *c, DeviceOctree &t, float &ms) {
        BuiltOctree unused;
        return run_prim_build(c, d->spheres, d->sphere_count, d->cuboids, d->cuboid_count, d->depth, flags, unused, &t,
                              ms);
    });
}

octpt_status octpt_scene_build_blocks_device(octpt_ctx *ctx, const octpt_scene_desc *d, const uint32_t *cells,
                                             uint32_t cell_count, uint32_t flags) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    join_inflight(ctx);
    const octpt_status st = check_block_build_args(ctx, cells, cell_count, flags);
    if (st != OCTPT_OK) return st;
    return build_scene_device(ctx, d, true, "device block scene build", [=](octpt_ctx *c, DeviceOctree &t, float &ms) {
        BuiltOctree unused;
        return run_block_build(c, cells, cell_count, d->depth, flags, d->block_count, unused, &t, ms);
    });
}

octpt_status octpt_scene_build_sections_device(octpt_ctx *ctx, const octpt_scene_desc *d,
                                               const octpt_section_world *world, uint32_t flags) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    join_inflight(ctx);
    if (!d) return fail(ctx, OCTPT_ERR_INVALID_ARG, "scene NULL");
    const octpt_status st = check_section_build_args(ctx, world, d->depth, flags);
    if (st != OCTPT_OK) return st;
    return build_scene_device(ctx, d, true, "device section scene build", [=](octpt_ctx *c, DeviceOctree &t, float &ms) {
        BuiltOctree unused;
        return run_section_build(c, world, d->depth, flags, d->block_count, unused, &t, ms);
    });
}

octpt_status octpt_set_camera(octpt_ctx *ctx, const octpt_camera *c) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!c) return fail(ctx, OCTPT_ERR_INVALID_ARG, "camera NULL");
    if (!(c->fov > 0.0f && c->fov < 3.14159265f)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "fov must be in (0, pi)");
    if (!lens_fields_valid(c->aperture, c->focal_distance))
        return fail(ctx, OCTPT_ERR_INVALID_ARG,
                    "aperture must be finite and >= 0, and focal_distance finite and > 0 when aperture > 0");
    if (c->aperture > 0.0f && ctx->proj.mode != OCTPT_PROJECTION_PINHOLE)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "an aperture needs the pinhole projection (octpt_set_projection)");
    if (c->aperture > 0.0f && ctx->rays.d_rays)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "an aperture while a ray source is set (octpt_set_ray_source)");
    ctx->cam = *c;
    DevCamera C{};
    std::memcpy(C.eye, c->eye, 12);
    std::memcpy(C.dir, c->direction, 12);
    std::memcpy(C.up, c->up, 12);
    cross3(c->direction, c->up, C.right);            // camera.rs:80
    C.d_factor = 1.0f / tanf(c->fov / 2.0f);         // camera.rs:79
    // the thin lens (C37): focal_distance is read with an aperture alone, and divided here once
    C.aperture = c->aperture;
    C.focal_scale = c->aperture > 0.0f ? c->focal_distance / C.d_factor : 0.0f;
    // the projection (C40) rides in the device camera: a projected camera has no aperture, so proj_half takes the
    // slot of focal_scale
    C.proj_mode = ctx->proj.mode;
    if (C.proj_mode != OCTPT_PROJECTION_PINHOLE) C.proj_half = ctx->proj.param * 0.5f;
    ctx->C = C;
    ctx->has_camera = true;
    ++ctx->camera_gen;
    for (octpt_ctx *sc : ctx->sub) {
        const octpt_status st = octpt_set_camera(sc, c);
        if (st != OCTPT_OK) return fail(ctx, st, sc->err);
    }
    return OCTPT_OK;
}

octpt_status octpt_set_projection(octpt_ctx *ctx, const octpt_projection *p) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "projection NULL");
    if (!proj_mode_known(p->mode)) return fail(ctx, OCTPT_ERR_UNSUPPORTED, "unknown projection mode");
    for (uint32_t r : p->reserved)
        if (r != 0u) return fail(ctx, OCTPT_ERR_INVALID_ARG, "projection: a reserved word is not zero");
    if (!proj_param_valid(p->mode, p->param))
        return fail(ctx, OCTPT_ERR_INVALID_ARG,
                    "projection param must be finite and > 0, and an angle at most 2 pi");
    if (p->mode != OCTPT_PROJECTION_PINHOLE && ctx->has_camera && ctx->cam.aperture > 0.0f)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "a projection other than pinhole needs a camera without an aperture");
    if (p->mode != OCTPT_PROJECTION_PINHOLE && ctx->rays.d_rays)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "a projection other than pinhole while a ray source is set (octpt_set_ray_source)");
    // (the pinhole's param is not read: every pinhole setting is one state)
    const float param = p->mode == OCTPT_PROJECTION_PINHOLE ? 0.0f : p->param;
    // the setting the context (and with it every entry) already holds: nothing changes, the beam table stays valid
    if (p->mode == ctx->proj.mode && param == ctx->proj.param) return OCTPT_OK;
    join_inflight(ctx);  // a frame in flight reads ctx->C
    ctx->proj = *p;
    ctx->proj.param = param;
    ctx->C.proj_mode = ctx->proj.mode;
    if (ctx->proj.mode != OCTPT_PROJECTION_PINHOLE) ctx->C.proj_half = ctx->proj.param * 0.5f;
    else if (!(ctx->C.aperture > 0.0f)) ctx->C.focal_scale = 0.0f;  // back to what octpt_set_camera derives
    ++ctx->camera_gen;  // the beam table is the pinhole camera's (enqueue_wavefront)
    for (octpt_ctx *sc : ctx->sub) {
        const octpt_status st = octpt_set_projection(sc, p);
        if (st != OCTPT_OK) return fail(ctx, st, sc->err);
    }
    return OCTPT_OK;
}

octpt_status octpt_get_projection(const octpt_ctx *ctx, octpt_projection *p) {
    if (!ctx || !p) return OCTPT_ERR_INVALID_ARG;
    *p = ctx->proj;
    return OCTPT_OK;
}

// The ray source (C41): the context keeps the caller's pointer and the list's shape; ray_source_camera hands them to the
// kernels of every later render.  Every check comes before the first write.
octpt_status octpt_set_ray_source(octpt_ctx *ctx, const octpt_ray_source *r) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!r || !r->d_rays) {  // clear: every later render is the context's own camera's
        if (!ctx->rays.d_rays) return OCTPT_OK;
        join_inflight(ctx);  // a frame in flight reads the list
        ctx->rays = octpt_ray_source{};
        return OCTPT_OK;
    }
    for (uint32_t w : r->reserved)
        if (w != 0u) return fail(ctx, OCTPT_ERR_INVALID_ARG, "ray source: a reserved word is not zero");
    if (r->rays_per_pixel == 0u || r->width == 0u || r->height == 0u)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "ray source: width, height and rays_per_pixel must be >= 1");
    // (three factors below 2^32: the product of two fits 64 bits, and the third is compared by division)
    const uint64_t px = (uint64_t)r->width * r->height;
    if (px > kRayListMaxRays || r->rays_per_pixel > kRayListMaxRays / px)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "ray source: more than 2^28 rays");
    if (is_multi(ctx))
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "a ray source lives on one device: not on a multi-device context");
    if (ctx->has_camera && ctx->cam.aperture > 0.0f)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "a ray source needs a camera without an aperture");
    if (ctx->proj.mode != OCTPT_PROJECTION_PINHOLE)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "a ray source needs the pinhole projection (octpt_set_projection)");
    join_inflight(ctx);  // a frame in flight reads the earlier setting
    ctx->rays = *r;
    return OCTPT_OK;
}

octpt_status octpt_get_ray_source(const octpt_ctx *ctx, octpt_ray_source *r) {
    if (!ctx || !r) return OCTPT_ERR_INVALID_ARG;
    *r = ctx->rays;
    return OCTPT_OK;
}

// The sky (C42).  Every check comes before the first write, so a refused call leaves the previous sky in force; a MAP is
// copied into a buffer of the context's own and sanitised there (sky_sanitise), and the call returns with the copy made,
// so the caller may free its texels.
namespace {
// The distribution's lifetime (C43): the context holds one exactly while sampling is MAP and the sky a MAP no wider than
// kSkySampleMaxWidth.  Whatever it held is dropped first (an earlier render on any stream may still read it).
octpt_status refresh_sky_distribution(octpt_ctx *ctx) {
    if (ctx->sky_dist.row_cdf || ctx->sky_dist.col_cdf) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        if (ctx->sky_dist.row_cdf) (void)hipFree(ctx->sky_dist.row_cdf);
        if (ctx->sky_dist.col_cdf) (void)hipFree(ctx->sky_dist.col_cdf);
    }
    ctx->sky_dist = DeviceSkyDist{};
    if (ctx->sky_sampling != OCTPT_SKY_SAMPLING_MAP || ctx->sky.mode != kSkyMap || ctx->sky.width > kSkySampleMaxWidth)
        return OCTPT_OK;
    std::vector<float> row(ctx->sky.height);
    for (uint32_t y = 0; y < ctx->sky.height; ++y) row[y] = sky_row_factor(y, ctx->sky.height);
    HIP_TRY(ctx, build_sky_distribution_gpu(ctx->stream, ctx->sky, row.data(), ctx->sky_dist));
    return OCTPT_OK;
}

octpt_status check_sky(octpt_ctx *ctx, const octpt_sky *k, bool texels) {
    if (!k) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky NULL");
    for (uint32_t w : k->reserved)
        if (w != 0u) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky: a reserved word is not zero");
    if (!sky_mode_known(k->mode)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky: unknown mode");
    if (!sky_fields_valid(k->mode, k->scale, k->yaw, k->width, k->height, texels))
        return fail(ctx, OCTPT_ERR_INVALID_ARG,
                    "sky: scale must be finite and >= 0, yaw finite, and a MAP needs texels, width and height >= 1 and "
                    "width * height <= 2^26");
    if (k->mode != OCTPT_SKY_DEFAULT && is_multi(ctx))
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "a sky other than DEFAULT: not on a multi-device context");
    return OCTPT_OK;
}
}  // namespace

octpt_status octpt_set_sky_device(octpt_ctx *ctx, const octpt_sky *k, const float *d_texels, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_sky(ctx, k, d_texels != nullptr);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "set_sky", [&]() -> octpt_status {
        join_inflight(ctx);  // a frame in flight reads the earlier sky
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        Sky s{};
        s.mode = k->mode;
        float *map = nullptr;
        if (k->mode != OCTPT_SKY_DEFAULT) {
            std::memcpy(s.color, k->color, 12);
            std::memcpy(s.horizon, k->horizon, 12);
            std::memcpy(s.zenith, k->zenith, 12);
            s.scale = k->scale;
            s.yaw = k->yaw;
        }
        if (k->mode == OCTPT_SKY_MAP) {
            hipStream_t hs = static_cast<hipStream_t>(stream);
            const size_t n = (size_t)k->width * k->height * 4u;
            HIP_TRY(ctx, hipMalloc(&map, n * sizeof(float)));
            hipError_t e = hipMemcpyAsync(map, d_texels, n * sizeof(float), hipMemcpyDeviceToDevice, hs);
            if (e == hipSuccess) e = launch_sky_sanitise(map, n, hs);
            if (e == hipSuccess) e = hipStreamSynchronize(hs);
            if (e != hipSuccess) {
                (void)hipFree(map);
                return hip_fail(ctx, e, "set_sky: map copy");
            }
            s.width = k->width;
            s.height = k->height;
            s.texels = map;
        }
        // an earlier render on any stream may still read the map this call replaces
        if (ctx->sky_map) {
            const hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) {
                if (map) (void)hipFree(map);
                return hip_fail(ctx, e, "set_sky");
            }
            (void)hipFree(ctx->sky_map);
        }
        ctx->sky_map = map;
        ctx->sky = s;
        ctx->sky_pub = *k;
        if (k->mode == OCTPT_SKY_DEFAULT) ctx->sky_pub = octpt_sky{};
        // sky sampling (C43): a new map rebuilds the distribution, any other sky drops it; a sky that keeps the map's
        // texels out of it (scale and yaw do not enter the distribution) never comes this way -- every MAP call copies.
        // A build that fails (out of device memory, a device error) is this call's status, with the new sky in force
        // and no distribution held: renders follow the sky unsampled until a later call builds one
        return refresh_sky_distribution(ctx);
    });
}

octpt_status octpt_set_sky(octpt_ctx *ctx, const octpt_sky *k, const float *texels) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    octpt_status st = check_sky(ctx, k, texels != nullptr);
    if (st != OCTPT_OK) return st;
    return guarded(ctx, "set_sky", [&]() -> octpt_status {
        join_inflight(ctx);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HostStage hs(ctx->stream);
        const bool map = k->mode == OCTPT_SKY_MAP;
        const float *d_texels = map ? hs.in(texels, (size_t)k->width * k->height * 4u) : nullptr;
        if (hs.ok() && (st = octpt_set_sky_device(ctx, k, d_texels, ctx->stream)) != OCTPT_OK) return st;
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "set_sky");
        return OCTPT_OK;
    });
}

octpt_status octpt_clear_sky(octpt_ctx *ctx) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    const octpt_sky none{};
    return octpt_set_sky_device(ctx, &none, nullptr, nullptr);
}

octpt_status octpt_get_sky(const octpt_ctx *ctx, octpt_sky *k) {
    if (!ctx || !k) return OCTPT_ERR_INVALID_ARG;
    *k = ctx->sky_pub;
    return OCTPT_OK;
}

octpt_status octpt_sky_radiance_device(octpt_ctx *ctx, const float *d_dirs, uint32_t n, float *d_out, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (n != 0u && (!d_dirs || !d_out)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky_radiance: NULL buffer");
    return guarded(ctx, "sky_radiance", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_sky_radiance_device(ctx->sub[0], d_dirs, n, d_out, stream));
        if (n == 0u) return OCTPT_OK;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, launch_sky_radiance(ctx->sky, d_dirs, n, d_out, static_cast<hipStream_t>(stream)));
        return OCTPT_OK;
    });
}

octpt_status octpt_sky_radiance_ctx(octpt_ctx *ctx, const float *dirs, uint32_t n, float *out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (n != 0u && (!dirs || !out)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky_radiance: NULL buffer");
    return guarded(ctx, "sky_radiance", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx)) return forwarded(ctx, octpt_sky_radiance_ctx(ctx->sub[0], dirs, n, out));
        if (n == 0u) return OCTPT_OK;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HostStage hs(ctx->stream);
        const float *d_dirs = hs.in(dirs, 3u * (size_t)n);
        float *d_out = hs.out(out, 3u * (size_t)n);
        octpt_status st = OCTPT_OK;
        if (hs.ok() && (st = octpt_sky_radiance_device(ctx, d_dirs, n, d_out, ctx->stream)) != OCTPT_OK) return st;
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "sky_radiance");
        return OCTPT_OK;
    });
}

// Sky sampling (C43): the setting, the distribution's read-back and the sample's device form.  Every check comes before
// the first write, so a refused call leaves the previous setting in force.
octpt_status octpt_set_sky_sampling(octpt_ctx *ctx, const octpt_sky_sampling *p) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky sampling NULL");
    for (uint32_t w : p->reserved)
        if (w != 0u) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky sampling: a reserved word is not zero");
    if (p->mode > OCTPT_SKY_SAMPLING_MAP) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky sampling: unknown mode");
    if (p->mode == OCTPT_SKY_SAMPLING_MAP) {
        if (is_multi(ctx)) return fail(ctx, OCTPT_ERR_UNSUPPORTED, "sky sampling: not on a multi-device context");
        if (ctx->emit_strategy == OCTPT_EMITTERS_ONE)
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "sky sampling together with emitter sampling ONE (DESIGN.md C43)");
    }
    return guarded(ctx, "set_sky_sampling", [&]() -> octpt_status {
        join_inflight(ctx);  // a frame in flight keeps the setting its call was made with
        if (p->mode == OCTPT_SKY_SAMPLING_MAP && ctx->sky.mode == kSkyMap && ctx->sky.width > kSkySampleMaxWidth)
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "sky sampling: the map is wider than 32768 texels");
        if (p->mode == ctx->sky_sampling) return OCTPT_OK;
        if (is_multi(ctx)) {  // (NONE: nothing to drop)
            ctx->sky_sampling = p->mode;
            return OCTPT_OK;
        }
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const uint32_t old = ctx->sky_sampling;
        ctx->sky_sampling = p->mode;
        const octpt_status st = refresh_sky_distribution(ctx);
        if (st != OCTPT_OK) ctx->sky_sampling = old;  // (the distribution is dropped either way: NONE holds none)
        return st;
    });
}

octpt_status octpt_get_sky_sampling(const octpt_ctx *ctx, octpt_sky_sampling *p) {
    if (!ctx || !p) return OCTPT_ERR_INVALID_ARG;
    *p = octpt_sky_sampling{};
    p->mode = ctx->sky_sampling;
    return OCTPT_OK;
}

octpt_status octpt_sky_distribution(octpt_ctx *ctx, octpt_sky_distribution_arrays *out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky distribution arrays NULL");
    out->width = out->height = 0u;
    out->build_ms = 0.0f;
    return guarded(ctx, "sky_distribution", [&]() -> octpt_status {
        join_inflight(ctx);
        const DeviceSkyDist &g = ctx->sky_dist;
        if (is_multi(ctx) || !g.row_cdf) return OCTPT_OK;  // the context holds none: the counts are 0
        if (!out->row_cdf != !out->col_cdf)
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky distribution: set both arrays, or neither to count");
        if (out->row_cdf && (out->row_cdf_capacity < g.height || out->col_cdf_capacity < (uint64_t)g.width * g.height))
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky distribution: an array's capacity is below its count");
        if (out->row_cdf) {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipMemcpy(out->row_cdf, g.row_cdf, (size_t)g.height * 8u, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(out->col_cdf, g.col_cdf, (size_t)g.width * g.height * 4u, hipMemcpyDeviceToHost));
        }
        out->width = g.width;
        out->height = g.height;
        out->build_ms = g.build_ms;
        return OCTPT_OK;
    });
}

octpt_status octpt_sky_sample_device(octpt_ctx *ctx, const float *d_u, uint32_t n, float *d_out, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (n != 0u && (!d_u || !d_out)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "sky_sample: NULL buffer");
    return guarded(ctx, "sky_sample", [&]() -> octpt_status {
        join_inflight(ctx);
        if (is_multi(ctx) || !ctx->sky_dist.row_cdf)
            return fail(ctx, OCTPT_ERR_INVALID_ARG,
                        "the context holds no sky distribution (sky sampling MAP and a MAP sky build it)");
        if (n == 0u) return OCTPT_OK;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const SkyDist D{ctx->sky_dist.row_cdf, ctx->sky_dist.col_cdf, ctx->sky_dist.total};
        HIP_TRY(ctx, launch_sky_sample(ctx->sky, D, d_u, n, d_out, static_cast<hipStream_t>(stream)));
        return OCTPT_OK;
    });
}

octpt_status octpt_get_camera(const octpt_ctx *ctx, octpt_camera *c) {
    if (!ctx || !c) return OCTPT_ERR_INVALID_ARG;
    if (!ctx->has_camera) return OCTPT_ERR_INVALID_ARG;
    *c = ctx->cam;
    return OCTPT_OK;
}

octpt_status octpt_render_device(octpt_ctx *ctx, const octpt_render_params *p, float *d_accum, uint32_t *d_seg,
                                 void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!d_accum) return fail(ctx, OCTPT_ERR_INVALID_ARG, "d_accum NULL");
    return guarded(ctx, "render", [&]() -> octpt_status {
        join_inflight(ctx);
        DevRender R{};
        octpt_status st = make_render(ctx, p, R);
        if (st != OCTPT_OK) return st;
        if (is_multi(ctx))
            return multi_render(ctx, *p, R, reinterpret_cast<float4 *>(d_accum), d_seg, static_cast<hipStream_t>(stream),
                                nullptr);
        return enqueue_render(ctx, R, reinterpret_cast<float4 *>(d_accum), d_seg, static_cast<hipStream_t>(stream),
                              (p->flags & OCTPT_RENDER_MEGAKERNEL) != 0);
    });
}

namespace {
// FrameInFlight worker: H2D, render, tone map, D2H on the context stream
void frame_worker(octpt_frame *f, DevRender R, bool megakernel) {
    octpt_ctx *ctx = f->ctx;
    octpt_status st = OCTPT_OK;
    auto run = [&]() -> octpt_status {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipMemcpyAsync(f->d_accum, f->h_accum, f->n_pixels * 16, hipMemcpyHostToDevice, ctx->stream));
        octpt_status r = is_multi(ctx) ? multi_render(ctx, f->params, R, f->d_accum, nullptr, ctx->stream, &f->cancel_requested)
                                       : enqueue_render(ctx, R, f->d_accum, nullptr, ctx->stream, megakernel, &f->cancel_requested);
        if (r != OCTPT_OK) return r;
        if (f->d_rgba) {
            HIP_TRY(ctx, launch_tonemap(f->d_accum, f->d_rgba, (uint32_t)f->n_pixels, ctx->d_lut_byte, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(f->h_rgba, f->d_rgba, f->n_pixels * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(ctx, hipMemcpyAsync(f->h_accum, f->d_accum, f->n_pixels * 16, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return OCTPT_OK;
    };
    try {
        st = run();
    } catch (...) {
        st = fail(ctx, OCTPT_ERR_INTERNAL, "unexpected exception in frame worker");
    }
    if (st != OCTPT_OK) (void)hipStreamSynchronize(ctx->stream);
    f->status = st;
    f->finished.store(true);
}

octpt_status frame_result(octpt_frame *f) {
    if (f->worker.joinable()) f->worker.join();
    if (f->ctx && f->ctx->inflight == f) f->ctx->inflight = nullptr;
    if (f->cancel_requested.load()) return OCTPT_CANCELLED;
    if (f->status != OCTPT_OK) return f->status;
    deliver(f);
    return OCTPT_OK;
}
}  // namespace

octpt_status octpt_render_async(octpt_ctx *ctx, const octpt_render_params *p, float *accum, uint8_t *rgba,
                                octpt_frame **out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!out || !accum) return fail(ctx, OCTPT_ERR_INVALID_ARG, "NULL output");
    *out = nullptr;
    octpt_frame *f = nullptr;
    try {
        join_inflight(ctx);
        DevRender R{};
        octpt_status st = make_render(ctx, p, R);
        if (st != OCTPT_OK) return st;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        f = new octpt_frame();
        f->ctx = ctx;
        f->params = *p;
        f->user_accum = accum;
        f->user_rgba = rgba;
        f->n_pixels = accum_pixels(R);
        auto fail_frame = [&](hipError_t e, const char *what) {
            free_frame_buffers(f);
            delete f;
            return hip_fail(ctx, e, what);
        };
        hipError_t e;
        if ((e = hipMalloc(&f->d_accum, f->n_pixels * 16)) != hipSuccess) return fail_frame(e, "hipMalloc accum");
        if ((e = hipHostMalloc(&f->h_accum, f->n_pixels * 16, hipHostMallocDefault)) != hipSuccess)
            return fail_frame(e, "hipHostMalloc accum");
        if (rgba) {
            if ((e = hipMalloc(&f->d_rgba, f->n_pixels * 4)) != hipSuccess) return fail_frame(e, "hipMalloc rgba");
            if ((e = hipHostMalloc(&f->h_rgba, f->n_pixels * 4, hipHostMallocDefault)) != hipSuccess)
                return fail_frame(e, "hipHostMalloc rgba");
        }
        std::memcpy(f->h_accum, accum, f->n_pixels * 16);
        f->worker = std::thread(frame_worker, f, R, (p->flags & OCTPT_RENDER_MEGAKERNEL) != 0);
        ctx->inflight = f;
        *out = f;
        return OCTPT_OK;
    } catch (...) {
        if (f) {
            if (f->worker.joinable()) f->worker.join();
            free_frame_buffers(f);
            delete f;
        }
        return fail(ctx, OCTPT_ERR_INTERNAL, "unexpected exception in render_async");
    }
}

octpt_status octpt_frame_poll(octpt_frame *f) {
    if (!f) return OCTPT_ERR_INVALID_ARG;
    if (!f->finished.load()) return OCTPT_NOT_READY;
    return frame_result(f);
}

octpt_status octpt_frame_wait(octpt_frame *f) {
    if (!f) return OCTPT_ERR_INVALID_ARG;
    return frame_result(f);
}

octpt_status octpt_frame_cancel(octpt_frame *f) {
    if (!f) return OCTPT_ERR_INVALID_ARG;
    if (!f->delivered) f->cancel_requested.store(true);
    return OCTPT_OK;
}

void octpt_frame_release(octpt_frame *f) {
    if (!f) return;
    if (f->worker.joinable()) f->worker.join();
    if (f->ctx && f->ctx->inflight == f) f->ctx->inflight = nullptr;
    free_frame_buffers(f);
    delete f;
}

octpt_status octpt_render(octpt_ctx *ctx, const octpt_render_params *p, float *accum, uint8_t *rgba) {
    octpt_frame *f = nullptr;
    octpt_status st = octpt_render_async(ctx, p, accum, rgba, &f);
    if (st != OCTPT_OK) return st;
    st = octpt_frame_wait(f);
    octpt_frame_release(f);
    return st;
}

octpt_status octpt_tonemap_device(octpt_ctx *ctx, const float *d_accum, uint8_t *d_rgba, uint32_t n, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!d_accum || !d_rgba) return fail(ctx, OCTPT_ERR_INVALID_ARG, "NULL buffer");
    if (n == 0) return OCTPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_tonemap(reinterpret_cast<const float4 *>(d_accum), reinterpret_cast<uchar4 *>(d_rgba), n,
                                ctx->d_lut_byte, static_cast<hipStream_t>(stream)));
    return OCTPT_OK;
}

uint32_t octpt_shard_pixels(uint32_t width, uint32_t height, uint32_t shard_index, uint32_t shard_count) {
    if (shard_count == 0 || shard_index >= shard_count) return 0;
    const uint32_t tiles = ((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile);
    return tiles_of_shard(tiles, shard_index, shard_count) * 64u;
}

octpt_status octpt_unshard_device(octpt_ctx *ctx, uint32_t W, uint32_t H, uint32_t N, const float *d_shards,
                                  uint32_t stride, float *d_frame, void *stream) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!d_shards || !d_frame || N == 0 || W == 0 || H == 0) return fail(ctx, OCTPT_ERR_INVALID_ARG, "bad unshard args");
    if (stride < octpt_shard_pixels(W, H, 0, N)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "shard stride too small");
    if (!ctx->h_order.empty() && (W != ctx->order_w || H != ctx->order_h))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "frame size differs from the tile order's (octpt_set_tile_order)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_unshard(W, H, N, ctx->h_order.empty() ? nullptr : ctx->d_order_pos,
                                reinterpret_cast<const float4 *>(d_shards), stride, reinterpret_cast<float4 *>(d_frame),
                                static_cast<hipStream_t>(stream)));
    return OCTPT_OK;
}

octpt_status octpt_set_tile_order(octpt_ctx *ctx, uint32_t width, uint32_t height, const uint32_t *order) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    join_inflight(ctx);
    try {  // (not guarded(): this entry's message names no entry)
        // validated once, before any entry changes (a failure part-way through a multi-device
        // context's entries must not leave them dealing differently)
        uint32_t T = 0;
        std::vector<uint32_t> pos;
        if (order) {
            if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 31))
                return fail(ctx, OCTPT_ERR_INVALID_ARG, "bad resolution");
            T = ((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile);
            pos.assign(T, 0xFFFFFFFFu);
            for (uint32_t s = 0; s < T; ++s) {
                if (order[s] >= T || pos[order[s]] != 0xFFFFFFFFu)
                    return fail(ctx, OCTPT_ERR_INVALID_ARG, "tile order is not a permutation of the frame's tiles");
                pos[order[s]] = s;
            }
        }
        for (size_t i = 0; i < ctx->sub.size(); ++i) {  // every device entry deals the same way (its sub-shards nest in it)
            const octpt_status st = octpt_set_tile_order(ctx->sub[i], width, height, order);
            if (st != OCTPT_OK) {
                // an entry failed (out of memory): every entry and the parent go back to round robin, so that the
                // parent's staging and the entries' item mappings agree
                const std::string why = ctx->sub[i]->err;
                for (octpt_ctx *c : ctx->sub) (void)octpt_set_tile_order(c, width, height, nullptr);
                ++ctx->order_gen;
                ctx->h_order.clear();
                ctx->order_w = ctx->order_h = 0;
                return fail(ctx, st, why + " (every entry reset to the round-robin deal)");
            }
        }
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        ++ctx->order_gen;
        if (!order) {
            ctx->h_order.clear();
            ctx->order_w = ctx->order_h = 0;
            return OCTPT_OK;
        }
        // the tables are overwritten in place: a render issued on any stream (render_device / unshard_device take
        // the caller's) may still read them, so the whole device drains first
        HIP_TRY(ctx, hipDeviceSynchronize());
        if (ctx->h_order.size() != T) {
            if (ctx->d_order) (void)hipFree(ctx->d_order);
            if (ctx->d_order_pos) (void)hipFree(ctx->d_order_pos);
            ctx->d_order = ctx->d_order_pos = nullptr;
            ctx->h_order.clear();
            HIP_TRY(ctx, hipMalloc(&ctx->d_order, (size_t)T * 4));
            HIP_TRY(ctx, hipMalloc(&ctx->d_order_pos, (size_t)T * 4));
        }
        HIP_TRY(ctx, hipMemcpy(ctx->d_order, order, (size_t)T * 4, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->d_order_pos, pos.data(), (size_t)T * 4, hipMemcpyHostToDevice));
        ctx->h_order.assign(order, order + T);
        ctx->order_w = width;
        ctx->order_h = height;
        return OCTPT_OK;
    } catch (const std::bad_alloc &) {
        return fail(ctx, OCTPT_ERR_OOM, "host allocation");
    } catch (...) {
        return fail(ctx, OCTPT_ERR_INTERNAL, "unexpected exception");
    }
}

octpt_status octpt_balance_tiles(uint32_t width, uint32_t height, uint32_t shard_count, const uint32_t *seg_count,
                                 uint32_t *order) {
    if (!seg_count || !order || shard_count == 0 || width == 0 || height == 0 ||
        (uint64_t)width * height >= (1ull << 31))
        return OCTPT_ERR_INVALID_ARG;
    try {
        const uint32_t tx = (width + kTile - 1) / kTile, T = tx * ((height + kTile - 1) / kTile);
        std::vector<uint64_t> cost(T, 0);
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) cost[(y / kTile) * tx + x / kTile] += seg_count[(size_t)y * width + x];
        // longest processing time first: tiles by cost (ties by index), each to the shard with the least work
        // so far among those with positions left -- shard k keeps exactly its round-robin count of positions
        std::vector<uint32_t> by(T);
        for (uint32_t t = 0; t < T; ++t) by[t] = t;
        std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
        const uint32_t N = shard_count;
        std::vector<uint64_t> load(N, 0);
        std::vector<std::vector<uint32_t>> mine(N);
        for (uint32_t k = 0; k < N; ++k) mine[k].reserve(tiles_of_shard(T, k, N));
        for (uint32_t t : by) {
            uint32_t best = N;
            for (uint32_t k = 0; k < N; ++k)
                if (mine[k].size() < tiles_of_shard(T, k, N) && (best == N || load[k] < load[best])) best = k;
            mine[best].push_back(t);
            load[best] += cost[t];
        }
        // each shard's tiles in image order (the seed's coherence: neighbouring tiles trace side by side)
        for (uint32_t k = 0; k < N; ++k) {
            std::sort(mine[k].begin(), mine[k].end());
            for (uint32_t u = 0; u < mine[k].size(); ++u) order[k + (size_t)u * N] = mine[k][u];
        }
        return OCTPT_OK;
    } catch (...) {
        return OCTPT_ERR_OOM;
    }
}

octpt_status octpt_intersect(octpt_ctx *ctx, const float *rays, const uint32_t *last_prim, const float *last_normal,
                             uint32_t n, float *t, uint32_t *prim, float *normal, uint32_t *steps) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    join_inflight(ctx);
    if (!ctx->has_scene) return fail(ctx, OCTPT_ERR_INVALID_ARG, "no scene uploaded");
    if (n == 0) return OCTPT_OK;
    if (!rays || !t || !prim) return fail(ctx, OCTPT_ERR_INVALID_ARG, "NULL buffer");
    return guarded(ctx, "intersect", [&]() -> octpt_status {
        if (is_multi(ctx))  // one batch on the first entry's replica
            return forwarded(ctx, octpt_intersect(ctx->sub[0], rays, last_prim, last_normal, n, t, prim, normal, steps));
        // esvo_begin's t_coef = 1 / -|d| comes from rcp_rn, exact for |d| in [2^-23, 2^126] (smaller
        // components are clamped to 2^-23 first, octree_traversal.rs:86-93): a ray with a non-finite
        // component or a direction component |d| > 2^126 is outside that range.  Such a ray is reported as a
        // miss -- t = +inf, prim = none, normal 0, 0 steps -- and the rest of the batch is traced as usual (the
        // kernel sees a placeholder ray in its place).  For a non-finite ray this is what the reference's
        // comparisons with NaN t-values give.  For a finite direction above 2^126 it is a DELIBERATE DEVIATION:
        // the reference does not normalise directions (Ray::new, ray/mod.rs:32), its t_coef would be subnormal
        // (octree_traversal.rs:95) and its walk could still hit something; no reference fixture covers that
        // case (parity unpinned), and the render kernels never produce such a direction.
        std::vector<uint32_t> unsupported;
        std::vector<float> clean;
        for (size_t i = 0; i < (size_t)n * 6; ++i) {
            const float v = rays[i];
            if (!std::isfinite(v) || (i % 6 >= 3 && std::fabs(v) > 0x1p126f)) {
                if (clean.empty()) clean.assign(rays, rays + (size_t)n * 6);
                const size_t r = i / 6;
                if (unsupported.empty() || unsupported.back() != r) unsupported.push_back((uint32_t)r);
                for (int k = 0; k < 6; ++k) clean[r * 6 + k] = k == 3 ? 1.0f : 0.0f;
            }
        }
        if (!clean.empty()) rays = clean.data();
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HostStage hs(ctx->stream);
        const float *d_rays = hs.in(rays, (size_t)n * 6);
        const uint32_t *d_lp = hs.in(last_prim, n);
        const float *d_ln = hs.in(last_normal, (size_t)n * 3);
        float *d_t = hs.out(t, n);
        uint32_t *d_p = hs.out(prim, n);
        float *d_n = hs.out(normal, (size_t)n * 3);
        uint32_t *d_s = hs.out(steps, n);
        if (hs.ok()) hs.note(launch_intersect(ctx->S, d_rays, d_lp, d_ln, n, d_t, d_p, d_n, d_s, ctx->stream));
        if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "intersect");
        for (uint32_t r : unsupported) {
            t[r] = INFINITY;
            prim[r] = 0xFFFFFFFFu;
            if (normal) normal[3 * (size_t)r] = normal[3 * (size_t)r + 1] = normal[3 * (size_t)r + 2] = 0.0f;
            if (steps) steps[r] = 0u;
        }
        return OCTPT_OK;
    });
}

// ---------------- emitter sampling: the setting and the grid ----------------
octpt_status octpt_set_emitter_sampling(octpt_ctx *ctx, const octpt_emitter_params *p) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!p) return fail(ctx, OCTPT_ERR_INVALID_ARG, "emitter params NULL");
    if (p->strategy == OCTPT_EMITTERS_ONE_BLOCK || p->strategy == OCTPT_EMITTERS_ALL)
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "emitter sampling strategies ONE_BLOCK and ALL are reserved (DESIGN.md C38)");
    if (p->strategy > OCTPT_EMITTERS_ALL) return fail(ctx, OCTPT_ERR_UNSUPPORTED, "unknown emitter sampling strategy");
    if (p->flags & ~OCTPT_EMITTERS_MODELS)
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "emitter params: unknown flag (OCTPT_EMITTERS_MODELS is the only one)");
    for (uint32_t r : p->reserved)
        if (r) return fail(ctx, OCTPT_ERR_INVALID_ARG, "emitter params: reserved words must be 0");
    if (!(p->intensity >= 0.0f) || !std::isfinite(p->intensity))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "emitter intensity must be finite and >= 0");
    if (p->grid_size == 0u || (p->grid_size & (p->grid_size - 1u)) || p->grid_size > (1u << kMaxDepth))
        return fail(ctx, OCTPT_ERR_INVALID_ARG, "emitter grid_size must be a power of two, 1 .. 2^21");
    join_inflight(ctx);  // a frame in flight keeps the setting its call was made with
    if (p->strategy == OCTPT_EMITTERS_ONE && ctx->sky_sampling == OCTPT_SKY_SAMPLING_MAP)  // C43
        return fail(ctx, OCTPT_ERR_UNSUPPORTED, "emitter sampling ONE together with sky sampling (DESIGN.md C43)");
    if (p->strategy == OCTPT_EMITTERS_ONE && ctx->has_scene) {
        const octpt_ctx *sc = is_multi(ctx) ? ctx->sub[0] : ctx;
        if (!sc->S.has_blocks)
            return fail(ctx, OCTPT_ERR_UNSUPPORTED, "emitter sampling needs a block-value scene (octpt_scene_desc.blocks)");
        if (p->grid_size > (1u << sc->S.depth))
            return fail(ctx, OCTPT_ERR_INVALID_ARG, "emitter grid_size exceeds the world's 2^depth");
    }
    const uint32_t old_strategy = ctx->emit_strategy, old_size = ctx->emit_grid_size, old_flags = ctx->emit_flags;
    const float old_intensity = ctx->emit_intensity;
    ctx->emit_strategy = p->strategy;
    ctx->emit_grid_size = p->grid_size;
    ctx->emit_intensity = p->intensity;
    ctx->emit_flags = p->flags;
    octpt_status st = OCTPT_OK;
    if (is_multi(ctx)) {
        for (octpt_ctx *sc : ctx->sub) {
            st = octpt_set_emitter_sampling(sc, p);
            if (st != OCTPT_OK) {
                fail(ctx, st, sc->err);
                break;
            }
        }
    } else if (old_strategy != p->strategy || old_size != p->grid_size ||
               (p->strategy == OCTPT_EMITTERS_ONE && old_flags != p->flags)) {  // (under NONE the flag means nothing)
        const hipError_t e = hipSetDevice(ctx->device);
        st = e != hipSuccess ? hip_fail(ctx, e, "hipSetDevice") : OCTPT_OK;
        if (st == OCTPT_OK && ctx->has_scene) {
            const hipError_t es = hipStreamSynchronize(ctx->stream);
            st = es != hipSuccess ? hip_fail(ctx, es, "hipStreamSynchronize") : refresh_emitter_grid(ctx);
        }
    }
    if (st != OCTPT_OK) {  // the setting stays what it was (a grid budget refusal: the old grid is built again)
        const std::string msg = ctx->err;
        ctx->emit_strategy = old_strategy;
        ctx->emit_grid_size = old_size;
        ctx->emit_intensity = old_intensity;
        ctx->emit_flags = old_flags;
        if (is_multi(ctx)) {  // every entry back to the old setting, those that had taken the new one included
            octpt_emitter_params old{};
            old.strategy = old_strategy;
            old.grid_size = old_size;
            old.intensity = old_intensity;
            old.flags = old_flags;
            for (octpt_ctx *sc : ctx->sub) (void)octpt_set_emitter_sampling(sc, &old);
        } else if (ctx->has_scene) {
            (void)refresh_emitter_grid(ctx);
        }
        ctx->err = msg;
    }
    return st;
}

octpt_status octpt_emitter_grid(octpt_ctx *ctx, octpt_emitter_grid_arrays *out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "emitter grid arrays NULL");
    out->cell_count = out->entry_count = out->emitter_count = out->cells_per_axis = 0u;
    join_inflight(ctx);
    if (is_multi(ctx)) return forwarded(ctx, octpt_emitter_grid(ctx->sub[0], out));
    if (!ctx->grid_valid)
        return fail(ctx, OCTPT_ERR_INVALID_ARG,
                    "the context holds no emitter grid (strategy OCTPT_EMITTERS_ONE and a block-value scene build it)");
    const DeviceEmitterGrid &g = ctx->emit_grid;
    bool fill = false;
    const octpt_status st = emitter_grid_receive(out, g.n_cells, g.n_entries, g.n_emitters, g.cells_axis, fill);
    if (st != OCTPT_OK) return fail(ctx, st, "emitter grid: set all three arrays, each with the capacity of its count");
    if (!fill) return OCTPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(out->cell_first, g.cell_first, ((size_t)g.n_cells + 1u) * 4, hipMemcpyDeviceToHost));
    if (g.n_entries)
        HIP_TRY(ctx, hipMemcpy(out->cell_emitters, g.cell_emitters, (size_t)g.n_entries * 4, hipMemcpyDeviceToHost));
    if (g.n_emitters)
        HIP_TRY(ctx, hipMemcpy(out->emitters, g.emitters, (size_t)g.n_emitters * sizeof(octpt_emitter), hipMemcpyDeviceToHost));
    return OCTPT_OK;
}

octpt_status octpt_emitter_models(octpt_ctx *ctx, octpt_emitter_model_arrays *out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "emitter model arrays NULL");
    out->model_count = out->entry_count = 0u;
    join_inflight(ctx);
    if (is_multi(ctx)) return forwarded(ctx, octpt_emitter_models(ctx->sub[0], out));
    if (!ctx->grid_valid || !(ctx->emit_grid.flags & OCTPT_EMITTERS_MODELS) || !ctx->d_model_first)
        return fail(ctx, OCTPT_ERR_INVALID_ARG,
                    "the context holds no emissive-model table (a grid built with OCTPT_EMITTERS_MODELS holds one)");
    const uint32_t n_models = (uint32_t)ctx->model_emissive.size(), n_entries = (uint32_t)ctx->emit_models.quad.size();
    bool fill = false;
    const octpt_status st = emitter_models_receive(out, n_models, n_entries, fill);
    if (st != OCTPT_OK) return fail(ctx, st, "emitter models: set all three arrays, each with the capacity of its count");
    if (!fill) return OCTPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(out->model_first, ctx->d_model_first, ((size_t)n_models + 1u) * 4, hipMemcpyDeviceToHost));
    if (n_entries) {
        HIP_TRY(ctx, hipMemcpy(out->quad_index, ctx->d_model_quad, (size_t)n_entries * 4, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out->cum_area, ctx->d_model_cum, (size_t)n_entries * 4, hipMemcpyDeviceToHost));
    }
    return OCTPT_OK;
}

octpt_status octpt_get_stats(const octpt_ctx *cctx, octpt_stats *out) {
    if (!cctx || !out) return OCTPT_ERR_INVALID_ARG;
    octpt_ctx *ctx = const_cast<octpt_ctx *>(cctx);
    join_inflight(ctx);
    if (is_multi(ctx)) {  // the entries' counters summed; kernel_ms = the render calls' wall time
        octpt_stats tot{};
        for (octpt_ctx *c : ctx->sub) {
            octpt_stats cs{};
            const octpt_status st = octpt_get_stats(c, &cs);
            if (st != OCTPT_OK) return fail(ctx, st, c->err);
            tot.paths += cs.paths;
            tot.segments += cs.segments;
            tot.esvo_steps += cs.esvo_steps;
            tot.sphere_tests += cs.sphere_tests;
            tot.cuboid_tests += cs.cuboid_tests;
            tot.shade_events += cs.shade_events;
            tot.texel_reads += cs.texel_reads;
            tot.extend_launches += cs.extend_launches;
            tot.shade_launches += cs.shade_launches;
            tot.extend_ms += cs.extend_ms;
            tot.shade_ms += cs.shade_ms;
            tot.build_ms = std::max(tot.build_ms, cs.build_ms);
            tot.block_tests += cs.block_tests;
            tot.issued_bytes += cs.issued_bytes;
            for (int k = 0; k < OCTPT_STAT_COUNT; ++k) tot.drain[k] += cs.drain[k];
            tot.pool_slots = std::max(tot.pool_slots, cs.pool_slots);
            tot.chunk_items = std::max(tot.chunk_items, cs.chunk_items);
            tot.wave_allocs += cs.wave_allocs;
            tot.beam_restarts += cs.beam_restarts;
            tot.hit_check_failures += cs.hit_check_failures;
        }
        tot.build_ms = std::max(tot.build_ms, (double)ctx->build_ms);  // the builder runs on the first device
        tot.launches = ctx->launches;
        tot.kernel_ms = ctx->kernel_ms;
        *out = tot;
        return OCTPT_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (auto &e : ctx->pending) {
        HIP_TRY(ctx, hipEventSynchronize(e.stop));
        float ms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, e.start, e.stop));
        ctx->kernel_ms += ms;
        (void)hipEventDestroy(e.start);
        (void)hipEventDestroy(e.stop);
    }
    ctx->pending.clear();
    for (auto &ke : ctx->kpending) {
        HIP_TRY(ctx, hipEventSynchronize(ke.second.stop));
        float ms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ke.second.start, ke.second.stop));
        ctx->kern_ms[ke.first] += ms;
        ctx->kern_n[ke.first]++;
        ctx->ev_pool.push_back(ke.second);
    }
    ctx->kpending.clear();
    std::vector<unsigned long long> rows(kStatWords);
    HIP_TRY(ctx, hipMemcpy(rows.data(), ctx->d_stats, kStatWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    // rows [0, kSegs): every kernel but the drain; [kStatDrainRow, +kSegs): the drain (octpt_stats::drain)
    unsigned long long v[kStatCount] = {0}, dr[kStatCount] = {0};
    for (uint32_t r = 0; r < kSegs; ++r)
        for (uint32_t i = 0; i < kStatCount; ++i) {
            v[i] += rows[r * kStatRow + i];
            dr[i] += rows[(kStatDrainRow + r) * kStatRow + i];
        }
    for (uint32_t i = 0; i < kStatCount; ++i) {
        out->drain[i] = dr[i];
        v[i] += dr[i];
    }
    if (std::getenv("OCTPT_PROFILE_LANES")) {  // diagnostic builds (-DOCTPT_PROFILE_LANES) fill words 12..24
        static const char *names[13] = {"iters", "active", "leaf_it", "leaf_ln", "pop_it", "pop_ln", "push_it",
                                        "desc_ln", "exact", "fold_it", "fold_ln", "dfold_it", "dfold_ln"};
        std::fprintf(stderr, "octpt lanes:");
        for (uint32_t i = 0; i < 13; ++i) {
            unsigned long long x = 0;
            for (uint32_t r = 0; r < kSegs; ++r) x += rows[r * kStatRow + 12 + i];
            std::fprintf(stderr, " %s=%llu", names[i], x);
        }
        std::fprintf(stderr, "\n");
    }
    // beam-started rays traced again from the cube entry: extend's retraced ones took a
    // second queue position, which its segment count includes; the drain's restart in place does not
    unsigned long long redo_main = 0, redo_drain = 0;
    for (uint32_t r = 0; r < kSegs; ++r) {
        redo_main += rows[r * kStatRow + kStatBeamRestartWord];
        redo_drain += rows[(kStatDrainRow + r) * kStatRow + kStatBeamRestartWord];
    }
    out->paths = v[kStatPaths];
    out->segments = v[kStatSegments] - redo_main;
    out->esvo_steps = v[kStatSteps];
    out->sphere_tests = v[kStatSphereTests];
    out->cuboid_tests = v[kStatCuboidTests];
    out->shade_events = v[kStatShade];
    out->texel_reads = v[kStatTexels];
    out->block_tests = v[kStatBlockTests];
    out->issued_bytes = v[kStatIssued];
    out->beam_restarts = redo_main + redo_drain;
    out->hit_check_failures = 0;
    for (uint32_t r = 0; r < 2u * kSegs; ++r) out->hit_check_failures += rows[r * kStatRow + kStatHitCheckWord];
    out->pool_slots = ctx->pool;
    out->chunk_items = ctx->color_cap;
    out->wave_allocs = ctx->wave_allocs_n;
    out->launches = ctx->launches;
    out->kernel_ms = ctx->kernel_ms;
    out->extend_launches = ctx->kern_n[0];
    out->shade_launches = ctx->kern_n[1];
    out->extend_ms = ctx->kern_ms[0];
    out->shade_ms = ctx->kern_ms[1];
    out->build_ms = ctx->build_ms;
    return OCTPT_OK;
}

octpt_status octpt_reset_stats(octpt_ctx *ctx) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    join_inflight(ctx);
    if (is_multi(ctx)) {
        for (octpt_ctx *c : ctx->sub) {
            const octpt_status st = octpt_reset_stats(c);
            if (st != OCTPT_OK) return fail(ctx, st, c->err);
        }
        ctx->kernel_ms = 0.0;
        ctx->launches = 0;
        return OCTPT_OK;
    }
    octpt_stats tmp;
    octpt_status st = octpt_get_stats(ctx, &tmp);  // drains pending events
    if (st != OCTPT_OK) return st;
    HIP_TRY(ctx, hipMemset(ctx->d_stats, 0, kStatWords * sizeof(unsigned long long)));
    ctx->kernel_ms = 0.0;
    ctx->launches = 0;
    ctx->kern_ms[0] = ctx->kern_ms[1] = 0.0;
    ctx->kern_n[0] = ctx->kern_n[1] = 0;
    return OCTPT_OK;
}

octpt_status octpt_build_octree_device(octpt_ctx *ctx, const octpt_sphere *spheres, uint32_t ns,
                                       const octpt_cuboid *cuboids, uint32_t nc, uint32_t depth, octpt_octree **out) {
    return octpt_build_octree_device_ex(ctx, spheres, ns, cuboids, nc, depth, 0u, out);
}

octpt_status octpt_build_octree_device_ex(octpt_ctx *ctx, const octpt_sphere *spheres, uint32_t ns,
                                          const octpt_cuboid *cuboids, uint32_t nc, uint32_t depth, uint32_t flags,
                                          octpt_octree **out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    if (!out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "out NULL");
    if (flags & ~OCTPT_BUILD_COMPACT) return fail(ctx, OCTPT_ERR_INVALID_ARG, "unknown build flags");
    *out = nullptr;
    if (depth < 1 || depth > kMaxDepth) return fail(ctx, OCTPT_ERR_INVALID_ARG, "depth must be in [1, 21]");
    if ((ns && !spheres) || (nc && !cuboids)) return fail(ctx, OCTPT_ERR_INVALID_ARG, "NULL primitive array");
    return build_octree_handle(ctx, out, "octree build", [=](BuiltOctree &t, float &ms) {
        join_inflight(ctx);
        if (pair_bound(spheres, ns, cuboids, nc, depth) > kMaxBuildPairs)
            return fail(ctx, OCTPT_ERR_OOM, "more than 2^31 (cell, primitive) pairs");
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        return run_prim_build(ctx, spheres, ns, cuboids, nc, depth, flags, t, nullptr, ms);
    });
}

octpt_status octpt_build_block_octree_device(octpt_ctx *ctx, const uint32_t *cells, uint32_t n, uint32_t depth,
                                             uint32_t flags, octpt_octree **out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    join_inflight(ctx);
    if (!out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "out NULL");
    *out = nullptr;
    if (depth < 1 || depth > kMaxDepth) return fail(ctx, OCTPT_ERR_INVALID_ARG, "depth must be in [1, 21]");
    const octpt_status st = check_block_build_args(ctx, cells, n, flags);
    if (st != OCTPT_OK) return st;
    return build_octree_handle(ctx, out, "block octree build", [=](BuiltOctree &t, float &ms) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        return run_block_build(ctx, cells, n, depth, flags, 0u, t, nullptr, ms);
    });
}

octpt_status octpt_build_block_octree_sections_device(octpt_ctx *ctx, const octpt_section_world *world, uint32_t depth,
                                                      uint32_t flags, octpt_octree **out) {
    if (!ctx) return OCTPT_ERR_INVALID_ARG;
    join_inflight(ctx);
    if (!out) return fail(ctx, OCTPT_ERR_INVALID_ARG, "out NULL");
    *out = nullptr;
    const octpt_status st = check_section_build_args(ctx, world, depth, flags);
    if (st != OCTPT_OK) return st;
    return build_octree_handle(ctx, out, "section octree build", [=](BuiltOctree &t, float &ms) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        return run_section_build(ctx, world, depth, flags, 0u, t, nullptr, ms);
    });
}

}  // extern "C"
