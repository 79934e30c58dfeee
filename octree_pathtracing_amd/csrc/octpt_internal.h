// octpt_internal.h -- device-side scene layout shared by the host API (octpt_api.cpp) and
// the gfx950 kernels (octpt_kernels.hip).  Layout notes live in DESIGN.md §5.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "../../include/octpt.h"
#include "octpt_sky.h"
#include "octpt_sky_sample.h"

namespace octpt {

constexpr uint32_t kPrimNone = 0xFFFFFFFFu;
constexpr uint32_t kPrimCuboidBit = 0x80000000u;
constexpr uint32_t kPrimIndexMask = 0x07FFFFFFu;  // primitive indices < 2^27 (hit records pack flags above)
// camera-ray beam starts (beam_kernel): one per kBeamTile x kBeamTile pixels (A/B knob)
#ifndef OCTPT_BEAM_TILE
#define OCTPT_BEAM_TILE 2
#endif
constexpr uint32_t kBeamTile = OCTPT_BEAM_TILE;
constexpr uint32_t kTile = 8;          // 8x8 pixel tiles = one wave64 of primary rays
constexpr uint32_t kBlock = 256;       // threads per block (4 waves)
constexpr uint32_t kMaxDepth = 21;     // new_octree.rs:14
constexpr uint64_t kMaxBuildPairs = 1ull << 31;  // octree builders: (cell, primitive) pair / cell cap

// GPUMaterial (gpu_material.rs:67-76) + the material's texture kind and, for colour
// textures, the pre-converted F32Color (colors/mod.rs:280-288): 48 B, three float4 loads
struct alignas(16) DevMaterial {
    float ior, specular, emittance, roughness;
    float metalness;
    uint32_t texture_index, flags, texture_kind;
    float color[4];
};

// texture table entry, 16 B
struct alignas(16) DevTexture {
    uint32_t kind;      // 0 colour, 1 image
    uint32_t rgba;      // packed U8Color (r | g<<8 | b<<16 | a<<24) for kind 0
    uint32_t width;     // image only
    uint32_t height;
    uint64_t offset;    // byte offset in the texel pool
    uint64_t pad;
};

// Sun::new derived constants (scene/mod.rs:321-383) + diffuse_reflection importance
// sampling constants (ray/mod.rs:228-259); computed once on the host with libm.
struct DevSun {
    float sw[3], su[3], sv[3];
    float width, width2;
    float tex[4];
    float isect_mul[3];
    float diffuse_mul[3];
    float emit[3];  // Sun::emmittance = color * INTENSITY^GAMMA (scene/mod.rs:352-353), preview shading
    float luminosity;
    float sun_dx, sun_dy, sun_dz;
    float circle_radius, sample_chance;
    int32_t draw_texture, importance_sampling, diffuse_sun;
    // next-event estimation (path_tracer.rs:225-291, 458-483)
    int32_t sun_sampling, strict_direct_light;
    float lum_a;          // sun_luminosity ? luminosity_pdf : 1
    float radius_cos;     // Sun::radius_cos
    float f_sub_surface;  // Scene::f_sub_surface
};

// block-model quad: Quad::new's derived plane, normal and w (quad.rs:90-114), 96 B
struct alignas(16) DevQuad {
    float4 o_d;    // (origin.xyz, d = normal . origin)
    float4 u_mat;  // (u.xyz, material bits)
    float4 v_tu0;  // (v.xyz, texture_u_range.x)
    float4 w_tu1;  // (w.xyz = n / (n . n), texture_u_range.y)
    float4 n_tv0;  // (normal.xyz, texture_v_range.x)
    float4 tv1;    // (texture_v_range.y, 0, 0, 0)
};

// primitive kinds a kernel instance handles (wf_extend_kernel's kPrims); kPrimsBlocks: block-value leaves (C23)
constexpr int kPrimsSpheres = 0, kPrimsBoxes = 1, kPrimsModels = 2, kPrimsBlocks = 3;
// flags of a block leaf's slot (slot.y, set at upload): bit f (f < 6) = face f's texture has a texel with
// alpha 0 (the leaf test reads the texel there), kBlockIsModel = the block is a block model
constexpr uint32_t kBlockFaceAlphaMask = 0x3Fu;
constexpr uint32_t kBlockIsModel = 0x40u;
// self-intersection key of a ray leaving quad q: kQuadKey | q; prim ids are
// sphere indices < 2^27 or kPrimCuboidBit | index, so the keys never collide
constexpr uint32_t kQuadKey = 0x40000000u;

struct DevScene {
    // sparse packed child slots: an octant's present children are contiguous from
    // its base; octant child = (its base, its child_mask), leaf child = (prim id, 1) or
    // (first leaf prim, prim count)
    const uint2 *node_child;
    // parallel to node_child: the sphere of a single-sphere leaf slot (sphere-only scenes; read by their extend alone).
    // OVERLOADED: the emitter instances of shade and the drain (C38) are launched with a copy of a block-value
    // scene whose leaf_sph holds the device address of the render's EmitGrid (csrc/octpt_emitter.h) instead, so
    // that no kernel argument changes its layout; code that reads leaf_sph in a block scene must not be added
    const float4 *leaf_sph;
    uint32_t root, root_mask, depth, n_octants;  // root = the root octant's base
    uint32_t has_cuboids;
    float octree_scale;             // 2^-depth
    float inv_octree_scale;         // 2^depth (x / 2^-depth == x * 2^depth exactly)
    const uint32_t *leaf_prims;
    const float4 *spheres;          // (cx, cy, cz, r)
    const uint32_t *sphere_mat;
    const float4 *cub_a;            // (min.x, min.y, min.z, max.x)
    const float2 *cub_b;            // (max.y, max.z): 24 B per box in two loads, no padding lanes
    const uint32_t *cub_mat;        // 6 per cuboid
    const uint32_t *cub_model;      // per cuboid: OCTPT_MODEL_NONE or a block model (C19); has_models only
    const uint2 *models;            // (first quad, quad count)
    const DevQuad *quads;
    uint32_t has_models;
    // block-value leaves (C23): a leaf slot is (block id, kBlock* flags); blk_mat = 6 face materials per
    // block, blk_model = its model (OCTPT_MODEL_NONE: the block fills its cell)
    uint32_t has_blocks, n_blocks;
    const uint32_t *blk_mat;
    const uint32_t *blk_model;
    const DevMaterial *mats;
    uint32_t n_mats;
    const DevTexture *texs;
    uint32_t n_texs;
    const uint8_t *texels;
    const float *lut_float;         // LUT_TABLE_FLOAT (texture.rs:51-54)
    DevSun sun;
    int32_t emitters;
    uint32_t has_images;  // some texture is an image (shade's colour-only instance when not)
};

// What a sky instance (octpt_kernels_sky.hip, octpt_kernels_sky_emit.hip) takes in the scene's place:
// the scene record as it is, the context's sky behind it.  The instances launched under the DEFAULT sky take DevScene
// as they always did; no struct of theirs changes.
struct SkyScene : DevScene {
    Sky sky;
};
// ... and what a sky-sampling instance (C43; octpt_kernels_skysample.hip) takes: the same, the map's distribution
// (device arrays, csrc/octpt_sky_sample.h) behind it.  SkyScene is what it was.
struct SkySampleScene : SkyScene {
    SkyDist dist;
};

struct DevCamera {
    float eye[3], dir[3], right[3], up[3];
    float d_factor;  // 1 / tan(fov / 2)  (camera.rs:79)
    // the thin lens, read by the lens instances of seed, shade and the megakernel alone
    float aperture;     // lens radius, 0 = pinhole
    // The projection, read by the projected instances alone (octpt_kernels_proj.hip).  A camera has an
    // aperture or a projection, never both (octpt_set_camera, octpt_set_projection), so the projection's float shares
    // the lens's slot, and its mode takes the four bytes that padded the struct to the 8-byte alignment of the kernel
    // argument after it: no kernel's argument block changed in size or layout.
    union {
        float focal_scale;  // focal_distance / d_factor, divided once on the host (0 with aperture 0)
        float proj_half;    // octpt_projection::param * 0.5f, multiplied once on the host
    };
    uint32_t proj_mode;  // OCTPT_PROJECTION_*; 0 = pinhole
};
static_assert(sizeof(DevCamera) == 64, "DevCamera fills the 64 bytes it always took as a kernel argument");

// The ray-list camera (octpt_set_ray_source), read by the ray-list instances alone
// (octpt_kernels_rays.hip).  That form reads eye and dir (its fallback ray) and none of right, up, d_factor, aperture
// and the union, so the camera a render under a ray source passes to its kernels (ray_source_camera, octpt_ctx.h)
// carries the list in `right` -- the buffer's address as the bit patterns of right[0..1], rays per pixel as that of
// right[2] -- and marks itself with a proj_mode no public mode has, which is what the launchers pick the instances by.
// The struct and every kernel's argument block stay as they are.
constexpr uint32_t kProjModeRays = 0x80000000u;
inline void set_cam_ray_list(DevCamera &C, const float *d_rays, uint32_t rpp) {
    const uint64_t a = reinterpret_cast<uint64_t>(d_rays);
    __builtin_memcpy(C.right, &a, 8);
    __builtin_memcpy(C.right + 2, &rpp, 4);
    C.proj_mode = kProjModeRays;
}
__host__ __device__ inline const float *cam_ray_list(const DevCamera &C) {
    uint64_t a;
    __builtin_memcpy(&a, C.right, 8);
    return reinterpret_cast<const float *>(a);
}
__host__ __device__ inline uint32_t cam_ray_list_rpp(const DevCamera &C) {
    uint32_t r;
    __builtin_memcpy(&r, C.right + 2, 4);
    return r;
}

// n / d for a divisor d fixed per launch (Lemire, Kaser & Kurz 2019, "Faster remainder by direct computation"):
// with c = ceil(2^64 / d), floor(c * n / 2^64) = floor(n / d) for every 32-bit n and 2 <= d < 2^32; c = 0 marks d = 1.
// Two integer multiplies instead of the ~25-instruction runtime division (item -> pixel maps of seed, shade, resolve).
inline uint64_t udiv_magic(uint32_t d) { return d <= 1u ? 0ull : ~0ull / d + 1ull; }
__host__ __device__ inline uint32_t udiv_c(uint32_t n, uint64_t c) {
    if (c == 0ull) return n;
#ifdef __HIP_DEVICE_COMPILE__
    const uint64_t hi = (uint64_t)(uint32_t)(c >> 32) * n + __umulhi((uint32_t)c, n);
#else
    const uint64_t hi = (uint64_t)(uint32_t)(c >> 32) * n + (((uint64_t)(uint32_t)c * n) >> 32);
#endif
    return (uint32_t)(hi >> 32);
}

struct DevRender {
    uint32_t W, H;
    uint32_t spp_start, spp_count;
    uint32_t max_depth;
    uint32_t seed;
    uint32_t shard_index, shard_count;
    uint32_t compact;        // accum holds the shard's tiles only (tile-major)
    uint32_t tiles_x;        // ceil(W / 8)
    uint64_t div_tiles_x, div_items;  // udiv_magic(tiles_x), udiv_magic(total_items)
    uint32_t shard_tiles;    // tiles owned by this shard
    uint32_t total_items;    // shard_tiles * 64 work items
    uint32_t group_shift;    // log2 G, G = a pixel's samples in one wave of the chunk's item order (0, 2, 4 or 6;
                             // item_split in octpt_kernels.hip); set per chunk, 0 everywhere else
    float dim;               // max(W, H)
    float jlo, jhi;          // -1 / dim, 1 / dim: the jitter range of render_tile_average (tile_renderer.rs:701-702),
                             // divided once on the host (IEEE division, the same bits as the device's)
    uint32_t preview;        // RendererMode::Preview
    // branch schedule, NULL when branch_count == 1: sub-sample k of this call is
    // subs[k] = (pass spp, pass branch count | branch << 16); spp_count then counts sub-samples
    const uint2 *subs;
    // beam starts of the camera rays, one per kBeamTile^2 pixels of the frame (row-major, beam_tx per
    // row), NULL = off (beam_kernel)
    const float *beam;
    uint32_t beam_tx;
    // the tile deal (octpt_set_tile_order): dealing position s -> frame tile, NULL = identity.  Shard k owns
    // positions s = k + u * shard_count (its local tile u), whatever the order
    const uint32_t *tile_order;
};

// octpt_aov_buffers as the guide-buffer kernel takes it (device pointers, NULL = not wanted)
struct DevAov {
    float4 *albedo, *normal;
    float *depth;
    uint32_t *prim, *material;
};

// one denoise call (octpt_denoise_params + the guides), DESIGN.md C25
struct DevDenoise {
    uint32_t W, H;
    float sigma_color;                  // scaled by 2^-i in iteration i
    float sn2, sz2;                     // sigma_normal^2, sigma_depth^2
    const float4 *normal, *albedo;      // albedo: NULL without OCTPT_DENOISE_DEMODULATE
    const float *depth;
};

// one temporal reprojection call (octpt_temporal_params + the buffers); passed by value
struct DevTemporal {
    uint32_t W, H;
    float dim;                          // max(W, H)
    DevCamera cur, prev;
    uint32_t max_history;
    float depth_tolerance, normal_threshold;
    uint32_t match_prim;
    const float4 *color, *normal;       // the current frame and its guides
    const float *depth;
    const uint32_t *prim;               // NULL without OCTPT_TEMPORAL_MATCH_PRIM
    const float4 *h_color, *h_normal;   // the history; h_color NULL = first frame
    const float *h_depth;
    const uint32_t *h_prim, *h_length;
    float4 *out;
    uint32_t *out_length;
    // C27, read by the moments instance alone: the history's and the output's (m1, m2) planes, and the albedo
    // guide with OCTPT_TEMPORAL_DEMODULATE (NULL without)
    const float4 *albedo;
    const float2 *h_moments;
    float2 *out_moments;
};

// one variance estimate (octpt_variance_params + the buffers), DESIGN.md C28
struct DevVariance {
    uint32_t W, H;
    uint32_t min_history;
    float sn2, sz2;                     // sigma_normal^2, sigma_depth^2
    const float2 *moments;
    const uint32_t *length;
    const float4 *normal;
    const float *depth;
    float *out;
};

// one variance-guided denoise call (octpt_denoise_variance_params + the guides), DESIGN.md C29
struct DevDenoiseVar {
    uint32_t W, H;
    float sigma_luminance, luminance_floor;
    float sn2, sz2;                     // sigma_normal^2, sigma_depth^2
    const float4 *normal, *albedo;      // albedo: NULL without OCTPT_DENOISE_DEMODULATE
    const float *depth;
    const float4 *color;                // the input frame: its alpha, read by the last pass alone
    float4 *out;                        // the caller's frame, written by the last pass (may be `color`)
    float *out_variance;                // nullable; written by the last pass
};

// frame tile at dealing position s (octpt_set_tile_order's permutation, or s itself)
__host__ __device__ inline uint32_t dealt_tile(const uint32_t *order, uint32_t s) { return order ? order[s] : s; }

// TileRenderer::get_current_branch_count (tile_renderer.rs:196-206)
inline uint32_t current_branch_count(uint32_t current_spp, uint32_t scene_branch_count) {
    if (current_spp < scene_branch_count) {
        if (current_spp <= (uint32_t)sqrtf((float)scene_branch_count)) return 1u;
        return scene_branch_count - current_spp;
    }
    return scene_branch_count;
}

// wavefront path tracer state.
// A single device-scope counter sustains only ~88 M atomicAdd/s on MI355X (tools/atomic_bench.hip),
// so every queue and work counter is split into kSegs shards, each on its own 256-B line:
//   ray queue q = kSegs segments of seg_cap positions; segment k holds count(q,k) rays;
//   extend claims from head(q,k); shade appends a ray to the segment it came from (one input ray
//   yields at most one output ray, so a segment never overflows); chunk items are split into
//   kSegs contiguous shards claimed through item(k), stolen from other shards once a wave's own
//   shard is exhausted.
constexpr uint32_t kSegs = 64;
constexpr uint32_t kCtrStride = 64;  // uint32 words between counters (256 B)
constexpr uint32_t kCtrlWords = 5u * kSegs * kCtrStride;
__host__ __device__ constexpr uint32_t ctr_count(uint32_t q, uint32_t k) { return (q * kSegs + k) * kCtrStride; }
__host__ __device__ constexpr uint32_t ctr_head(uint32_t q, uint32_t k) { return ((2u + q) * kSegs + k) * kCtrStride; }
__host__ __device__ constexpr uint32_t ctr_item(uint32_t k) { return (4u * kSegs + k) * kCtrStride; }

struct WaveBuffers {
    float4 *ray0[2];  // per queue position: (o.xyz, last_prim)
    float4 *ray1[2];  // per queue position: (d.xyz, slot | self_inward << 31)
    float4 *pa;     // (T.xyz, L.x)
    float4 *pb;     // (L.y, L.z, rng, item)
    uint2 *pc;      // (cur_mat, depth | specular << 8 | path_segs << 16)
    uint32_t *item0;  // per slot: the chunk item the seed started there (the first shade rebuilds pa / pb / pc)
    uint2 *hit;     // per queue position: (cuboid bit | flags << 27 | prim index, t) -- hit_record()
    // per queue position, block-value scenes only (C23): the whole hit record, (face << 27 | block or the quad, t, u, v)
    // -- the hit's texture coordinates or a quad's barycentrics beside it -- one 16-B store in extend and one
    // 16-B load in shade (round 6; until then an 8-B `hit` record and an 8-B (u, v) record in two arrays)
    uint4 *hit4;
    float4 *color;  // per chunk item: (L.xyz, path segments)
    // sun-sampling state, 4 planes of `pool` float4:
    // (co.xyz, clast), (cd.xyz, ccur), (cn.xyz, mult), att
    float4 *pd;
    uint32_t pool;
    uint32_t *ctrl;    // kCtrlWords sharded counters (see above)
    uint32_t seg_cap;  // positions per queue segment (multiple of 64)
    // (camera eye.xyz, kPrimNone): the first half of every ray record the seed writes, which the
    // chunk's first shade takes from here instead of re-reading it
    float4 eye;
    // the lean 24-B path state (pa = (T, rng), pc; pb and item0 unused): no emitters, no sun sampling and the
    // pool holding the chunk (item = slot), set per chunk by the host
    uint32_t lean;
};
// shade instance: 0 = 40-B path state, 1 = with regeneration (pool smaller than the chunk), 2 = lean
inline int shade_mode(bool regen, bool lean) { return regen ? 1 : (lean ? 2 : 0); }

// per-launch statistics, accumulated with one atomic per wave
enum StatIndex {
    kStatPaths = 0,
    kStatSegments,
    kStatSteps,
    kStatSphereTests,
    kStatCuboidTests,
    kStatShade,
    kStatTexels,
    kStatBlockTests,  // block-value leaf tests (C23)
    kStatIssued,      // extend's issued load bytes (OCTPT_COUNT_ISSUED builds only)
    kStatCount
};
static_assert(kStatCount == OCTPT_STAT_COUNT, "octpt_stats::drain order");
// statistics rows: kSegs rows of kStatRow counters (256 B each), row = blockIdx % kSegs; the host sums.
// The drain kernel counts into a second set of kSegs rows (octpt_stats::drain).
constexpr uint32_t kStatRow = 32;
constexpr uint32_t kStatWords = 2u * kSegs * kStatRow;
constexpr uint32_t kStatDrainRow = kSegs;
// beam-started rays traced again from the cube entry (octpt_stats::beam_restarts): a word of the row
// past the kStatCount counters, counted by one atomic per event
constexpr uint32_t kStatBeamRestartWord = 10;
// hit records with an unwritten field (OCTPT_CHECK_HITS diagnostic builds; octpt_stats::hit_check_failures)
constexpr uint32_t kStatHitCheckWord = 11;
static_assert(kStatBeamRestartWord >= kStatCount && kStatBeamRestartWord < 12, "below the lane-profile words");

// Multi-device renders (octpt_create_multi): item i of a shard's compact tile order (tile
// u = i / 64, pixel k = i % 64 of it) is rendered by device entry u % n_dev as its local tile u / n_dev --
// the entry's own shard of the kernels' tile split, shard_index + (u % n_dev) * shard_count of
// shard_count * n_dev -- whose compact buffer is staged on the first device at (u % n_dev) * stride.
// `caller` is the item's index in the caller's buffer (the shard's compact buffer, or the W x H frame);
// false for a pixel outside the image in a frame layout (never read or written).
__host__ __device__ inline bool multi_slot(uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t shard_index,
                                           uint32_t shard_count, bool compact, uint32_t n_dev, uint32_t stride,
                                           uint32_t i, uint32_t &caller, uint32_t &staged,
                                           const uint32_t *order = nullptr) {
    const uint32_t u = i / 64u, k = i % 64u;
    staged = (u % n_dev) * stride + (u / n_dev) * 64u + k;
    if (compact) {
        caller = i;
        return true;
    }
    const uint32_t t = dealt_tile(order, shard_index + u * shard_count);
    const uint32_t x = (t % tiles_x) * kTile + k % kTile, y = (t / tiles_x) * kTile + k / kTile;
    if (x >= W || y >= H) return false;
    caller = y * W + x;
    return true;
}

// kernel launchers (octpt_kernels.hip)
// sky (here, launch_wf_shade and launch_wf_drain; C42): NULL = the DEFAULT sky, the instances as they always were;
// else the sky instances, which take the scene with *sky behind it (SkyScene)
hipError_t launch_preview(const DevScene &S, const DevCamera &C, const DevRender &R, float4 *accum,
                          uint32_t *segcount, unsigned long long *stats, hipStream_t stream, const Sky *sky = nullptr);
hipError_t launch_render(const DevScene &S, const DevCamera &C, const DevRender &R, float4 *accum,
                         uint32_t *segcount, uint32_t *counter, unsigned long long *stats, int grid,
                         hipStream_t stream);
// the lens instances (C37; octpt_kernels_lens.hip, a module of its own), which the launchers here take for a camera
// with an aperture: the megakernel's, the seed's and the general shade's (mode: shade_mode, 0 or 1)
const void *lens_render_kernel(bool nee, bool blocks);
const void *lens_seed_kernel();
const void *lens_shade_kernel(bool nee, bool lds, int mode);
// the projected instances (C40; octpt_kernels_proj.hip, a module of its own), taken for a camera whose projection is not
// pinhole: the same three, the preview's and the guide-buffer kernel's (prims: the scene's kPrims*), and the emitter
// instances of the general shade (octpt_kernels_proj_emit.hip)
const void *proj_render_kernel(bool nee, bool blocks);
const void *proj_seed_kernel();
const void *proj_shade_kernel(bool nee, bool lds, int mode);
const void *proj_preview_kernel(int prims);
const void *proj_gbuffer_kernel(int prims);
const void *proj_emit_shade_kernel(bool nee, bool lds, int mode);
// the ray-list instances (C41; octpt_kernels_rays.hip and octpt_kernels_rays_emit.hip, modules of their own), taken
// for a camera that carries a ray list (kProjModeRays): the same without the megakernel's
const void *rays_seed_kernel();
const void *rays_shade_kernel(bool nee, bool lds, int mode);
const void *rays_preview_kernel(int prims);
const void *rays_gbuffer_kernel(int prims);
const void *rays_emit_shade_kernel(bool nee, bool lds, int mode);
// the sky instances (C42; octpt_kernels_sky.hip and octpt_kernels_sky_emit.hip, modules of their own), taken under a
// sky other than DEFAULT: the general shade (mode 0 or 1; such chunks never take the lean state), the drain and the
// preview, whose camera form -- pinhole, lens, projection, ray list -- is a launch-uniform run-time switch on the camera
// record, and the emitter twins of shade and the block scene's drain.  The seed is the camera's own, as without a sky.
const void *sky_shade_kernel(bool nee, bool lds, int mode);
const void *sky_drain_kernel(int prims, bool nee);
const void *sky_preview_kernel(int prims);
const void *sky_emit_shade_kernel(bool nee, bool lds, int mode);
const void *sky_emit_drain_kernel(bool nee);
// octpt_set_sky's pass over a map (sky_sanitise on each of n floats, in place) and octpt_sky_radiance_device's kernel
// (sky_radiance for n directions of three floats)
// the sky-sampling instances (C43; octpt_kernels_skysample.hip, a module of its own), which launch_wf_shade and
// launch_wf_drain take with `dist`: sky sampling on, the sky a MAP and the distribution's total not 0
const void *skysample_shade_kernel(bool nee, bool lds, int mode);
const void *skysample_drain_kernel(int prims, bool nee);
hipError_t launch_sky_sanitise(float *texels, size_t n, hipStream_t stream);
hipError_t launch_sky_radiance(const Sky &sky, const float *dirs, uint32_t n, float *out, hipStream_t stream);
hipError_t launch_wf_seed(const DevCamera &C, const DevRender &R, const WaveBuffers &B, uint32_t n_seed,
                          uint32_t chunk_items, unsigned long long *stats, hipStream_t stream);
hipError_t launch_wf_extend(const DevScene &S, const WaveBuffers &B, uint32_t q, bool cam, uint32_t refill, int grid,
                            unsigned long long *stats, hipStream_t stream);
// first: the chunk's first shade (the seed's rays: path state rebuilt from item0); regen: the pool is
// smaller than the chunk, finished paths regenerate their slots (the instance with regeneration)
hipError_t launch_wf_shade(const DevScene &S, const DevCamera &C, const DevRender &R, const WaveBuffers &B, uint32_t q,
                           uint32_t chunk_items, uint32_t first, bool regen, int grid, unsigned long long *stats,
                           hipStream_t stream, bool emit = false, const Sky *sky = nullptr,
                           const SkyDist *dist = nullptr);
// the emitter instances (C38; octpt_kernels_emit.hip, a module of its own), which launch_wf_shade and launch_wf_drain
// take with `emit`: S is then a block-value scene whose leaf_sph holds the device address of the render's EmitGrid
// (csrc/octpt_emitter.h), and the pd planes number six
const void *emit_shade_kernel(bool nee, bool lds, int mode, bool lens);
const void *emit_drain_kernel(bool nee);
// blocks per CU of the shade instance (shade_mode; registers bound it, shade uses no dynamic LDS)
int shade_blocks_per_cu(const DevScene &S, int mode);
// whether the scene's shade instance copies the material / texture tables into LDS
bool shade_lds_tables(const DevScene &S);
// the drain of a chunk's last queued rays (every chunk item claimed): one launch, paths finished in-lane
hipError_t launch_wf_drain(const DevScene &S, const DevRender &R, const WaveBuffers &B, uint32_t q, int grid,
                           unsigned long long *stats, hipStream_t stream, bool emit = false, const Sky *sky = nullptr,
                           const SkyDist *dist = nullptr);
// the host's snapshot of an iteration's counters: queue q's kSegs segment counts, then the kSegs item
// counters, written by one 128-thread block into pinned host memory (enqueue_wavefront's steering)
hipError_t launch_wf_snapshot(const WaveBuffers &B, uint32_t q, uint32_t *host_out, hipStream_t stream);
// moments (nullable, C31): the instance that also keeps the samples' luminance moments, full frame, image order;
// clamp (C33): 0 = off, else the instances that clamp each sample's luminance to it
hipError_t launch_wf_resolve(const DevRender &R, const WaveBuffers &B, uint32_t chunk_spp, float4 *accum,
                             uint32_t *segcount, float2 *moments, float clamp, hipStream_t stream);
// an adaptive render's start (C32): n pixels of accum to (0, 0, 0, 1) and of moments to (0, 0)
hipError_t launch_adaptive_init(uint32_t n, float4 *accum, float2 *moments, hipStream_t stream);
// the per-tile error of C32: one launch, one wave64 per 8 x 8 tile of the W x H frame
hipError_t launch_tile_error(uint32_t W, uint32_t H, float luminance_floor, const float2 *moments,
                             const uint32_t *tile_spp, float *error, hipStream_t stream);
// the seam rule of C34: out[t] = max(error[t], w * the largest error of t's neighbours), one launch
hipError_t launch_tile_error_spread(uint32_t W, uint32_t H, float w, const float *error, float *out, hipStream_t stream);
// the variance of the pixel means of C35: one launch, one thread per pixel; albedo nullable (demodulate)
hipError_t launch_sample_variance(uint32_t W, uint32_t H, const float2 *moments, const uint32_t *tile_spp,
                                  const float *depth, const float4 *albedo, float *out, hipStream_t stream);
int extend_blocks_per_cu(const DevScene &S);
hipError_t launch_intersect(const DevScene &S, const float *rays, const uint32_t *last_prim,
                            const float *last_normal, uint32_t n, float *t, uint32_t *prim, float *normal,
                            uint32_t *steps, hipStream_t stream);
hipError_t launch_beam(const DevScene &S, const DevCamera &C, const DevRender &R, float *beam, hipStream_t stream);
// first-hit guide buffers: the preview's walk, writing the hit it shades; out holds device
// pointers, NULL = not written
hipError_t launch_gbuffer(const DevScene &S, const DevCamera &C, const DevRender &R, const DevAov &out,
                          unsigned long long *stats, hipStream_t stream);
// the a-trous denoiser.  prep: color -> sig (the working signal: demodulated by albedo when
// not NULL, raw on miss pixels; alpha kept).  atrous: one iteration src -> dst with tap spacing 1 << iter;
// last: dst is the caller's frame and albedo (nullable) is multiplied back
hipError_t launch_denoise_prep(uint32_t W, uint32_t H, const float4 *color, const float4 *albedo, const float *depth,
                               float4 *sig, hipStream_t stream);
hipError_t launch_atrous(const DevDenoise &D, uint32_t iter, bool last, const float4 *src, float4 *dst,
                         hipStream_t stream);
// temporal reprojection: one launch, one thread per pixel of the current frame; moments: the
// instance that also carries the luminance moments (C27)
hipError_t launch_temporal(const DevTemporal &T, bool moments, hipStream_t stream);
// the variance estimate of C28: one launch, one thread per pixel
hipError_t launch_variance(const DevVariance &V, hipStream_t stream);
// the variance-guided a-trous filter.  prep: (color, variance) -> sig = (s.rgb, v), the working
// signal as launch_denoise_prep makes it with the variance in w.  atrous_var: one iteration src -> the next
// working frame dst, or with last (dst ignored) into D.out / D.out_variance
hipError_t launch_denoise_var_prep(uint32_t W, uint32_t H, const float4 *color, const float *variance,
                                   const float4 *albedo, const float *depth, float4 *sig, hipStream_t stream);
hipError_t launch_atrous_var(const DevDenoiseVar &D, uint32_t iter, bool last, const float4 *src, float4 *dst,
                             hipStream_t stream);
hipError_t launch_tonemap(const float4 *accum, uchar4 *out, uint32_t n, const uint8_t *lut_byte,
                          hipStream_t stream);
hipError_t launch_unshard(uint32_t W, uint32_t H, uint32_t shard_count, const uint32_t *tile_pos, const float4 *shards,
                          uint32_t stride, float4 *frame, hipStream_t stream);
// the caller's buffers (accum, and seg when not NULL) <-> the staged compact buffers of n_dev device
// entries (multi_slot), to_stage = caller -> staging
hipError_t launch_multi_stage(const DevRender &R, uint32_t n_dev, uint32_t stride, float4 *accum, uint32_t *seg,
                              float4 *stage_accum, uint32_t *stage_seg, bool to_stage, hipStream_t stream);
int render_blocks_per_cu(uint32_t depth);
size_t render_lds_bytes(uint32_t depth);

// std::vector allocator that leaves resized elements uninitialised: the builders overwrite every
// element, and zero-filling a C4 octree's 0.2 GB first costs more than the GPU build itself
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U> &) noexcept {}
    template <class U>
    void construct(U *p) noexcept {
        ::new (static_cast<void *>(p)) U;
    }
    template <class U, class... A>
    void construct(U *p, A &&...a) {
        ::new (static_cast<void *>(p)) U(std::forward<A>(a)...);
    }
};
template <class T>
using RawVec = std::vector<T, NoInitAlloc<T>>;

// host arrays of a built octree (octpt_octree, include/octpt.h)
struct BuiltOctree {
    RawVec<octpt_octant> octants;
    RawVec<uint32_t> leaf_first, leaf_count, leaf_prims;
    uint32_t root = 0, depth = 0;
};

// what the host builders (octpt_build_host.cpp) and the device entries (octpt_api.cpp) share: the upper bound of a
// primitive world's (cell, primitive) pairs, and a section world's own refusals before any array is read
// (OCTPT_OK, or the status)
uint64_t pair_bound(const octpt_sphere *spheres, uint32_t ns, const octpt_cuboid *cuboids, uint32_t nc,
                    uint32_t depth);
octpt_status section_world_status(const octpt_section_world *w, uint32_t depth);

// The emitter grid (octpt_build_emitter_grid in include/octpt.h): its budgets, the emissive flag of
// every block (false: a face material outside the table) and the count-then-fill rule of its arrays, which the host
// builder (octpt_build_host.cpp) and the context's query (octpt_api.cpp) share
constexpr float kEmitterEpsilon = 5e-8f;  // Ray::EPSILON
constexpr uint64_t kMaxEmitters = 1ull << 24, kMaxEmitterEntries = 1ull << 28, kMaxEmitterCells = 1ull << 28;
bool block_emissive_flags(const octpt_block *blocks, uint32_t nb, const octpt_material *mats, uint32_t nm,
                          std::vector<uint32_t> &out);
octpt_status emitter_grid_receive(octpt_emitter_grid_arrays *out, uint32_t n_cells, uint32_t n_entries,
                                  uint32_t n_emitters, uint32_t cells_axis, bool &fill);
// The emissive-model table (C39, octpt_emitter_model_table in include/octpt.h) as the host holds it: first[n_models
// + 1], and per entry the quad, the running area within its model and the quad's (origin, u, v) -- nine floats, what
// the sample reads (EmitGrid::quad_ouv).  emissive_model_table: false on a model whose quad range leaves the table
// or a quad of a model whose material is outside the material table.  emitter_models_receive: the count-then-fill rule.
struct EmissiveModelTable {
    std::vector<uint32_t> first, quad;
    std::vector<float> cum, ouv;
};
bool emissive_model_table(const octpt_block_model *models, uint32_t n_models, const octpt_quad *quads, uint32_t n_quads,
                          const octpt_material *mats, uint32_t nm, EmissiveModelTable &out);
octpt_status emitter_models_receive(octpt_emitter_model_arrays *out, uint32_t n_models, uint32_t n_entries, bool &fill);
// the emissive byte of every model (it has an entry), and the flag of every block when model emitters are listed too:
// 1 a full-cell emitter as block_emissive_flags, kEmitModelBit | model a block whose model is emissive, 0 else --
// a leaf's record's fourth word but for the cube's side; false: a block's model outside the table
std::vector<uint8_t> model_emissive_bytes(const EmissiveModelTable &t);
bool block_emissive_flags_models(const octpt_block *blocks, uint32_t nb, const std::vector<uint8_t> &model_emissive,
                                 std::vector<uint32_t> &flags);

// grow-only device scratch of the GPU octree builder, owned by the context: repeated builds
// (scene edits) reuse it instead of paying hipMalloc / hipFree per buffer
struct BuildScratch {
    static constexpr int kSlots = 32;
    void *dev[kSlots] = {};
    size_t cap[kSlots] = {};
    void release();
};

// a built octree left on the device (pointers into the BuildScratch, valid until the next build):
// the same arrays as BuiltOctree, plus the primitives the builder uploaded
struct DeviceOctree {
    const octpt_octant *octants = nullptr;
    const uint32_t *leaf_first = nullptr, *leaf_count = nullptr, *leaf_prims = nullptr;
    const octpt_sphere *spheres = nullptr;
    const octpt_cuboid *cuboids = nullptr;
    uint32_t n_octants = 0, n_leaves = 0, n_leaf_prims = 0, ns = 0, nc = 0, depth = 0;
};

// the octree builder on the device (octpt_build.hip); too_many: more than max_pairs pairs.
// dev == nullptr: the result is downloaded into `out`; else it stays on the device in *dev.
hipError_t build_octree_gpu(hipStream_t stream, BuildScratch &scratch, const octpt_sphere *spheres, uint32_t ns,
                            const octpt_cuboid *cuboids, uint32_t nc, uint32_t depth, bool compact,
                            uint64_t max_pairs, BuiltOctree &out, bool &too_many, float *ms,
                            DeviceOctree *dev = nullptr);

// The block-value builder on the device (octpt_build_block_octree, C23): cells[4k .. 4k+3] = (x, y, z, block),
// a host array uploaded once into the scratch, or with cells_on_device read where it is (on `stream`).
// The result equals the host builder's array for array and is returned as build_octree_gpu returns its own
// (no leaf tables: the leaf payloads are the block values).  `errors` receives the kCellErr* bits the cells
// raised; when it is not 0 nothing is built.  block_count (the scene entry; 0 = not checked): a block id
// >= block_count raises kCellErrBlockTable.
constexpr uint32_t kCellErrRange = 1u;       // x, y or z >= 2^depth
constexpr uint32_t kCellErrBlockId = 2u;     // block > kPrimIndexMask
constexpr uint32_t kCellErrBlockTable = 4u;  // block >= block_count
constexpr uint32_t kCellErrDuplicate = 8u;   // two cells at one position
hipError_t build_block_octree_gpu(hipStream_t stream, BuildScratch &scratch, const uint32_t *cells, uint32_t n,
                                  bool cells_on_device, uint32_t depth, bool compact, uint32_t block_count,
                                  BuiltOctree &out, uint32_t &errors, float *ms, DeviceOctree *dev = nullptr);

// The block-value builder from 16^3 palette sections (octpt_build_block_octree_sections_device): a front end
// that writes the (Morton code, block) streams of octpt_sections_to_cells' cells already sorted -- count per
// section, sort of the section keys, emit per sorted section in local Morton order -- and the cell builder's
// tail.  The world's three arrays are host arrays uploaded once into the scratch, or with on_device read where
// they are.  `errors`: the kCellErr* bits above (range = a section outside the world, duplicate = two sections
// at one position; block id / block table = a value of a section's palette slice) and the section bits below;
// when it is not 0 nothing is built.  too_many: more than max_cells cells (nothing is built).
constexpr uint32_t kCellErrPalette = 16u;       // palette_count 0 or > 4096, or the slice leaves the palette
constexpr uint32_t kCellErrIndexBlock = 32u;    // index_first not a multiple of 4096 or past index_count
constexpr uint32_t kCellErrUniform = 64u;       // OCTPT_SECTION_UNIFORM with palette_count != 1
constexpr uint32_t kCellErrPaletteIndex = 128u; // an index >= palette_count
hipError_t build_section_octree_gpu(hipStream_t stream, BuildScratch &scratch, const octpt_section_world &world,
                                    bool on_device, uint32_t depth, bool compact, uint32_t block_count,
                                    uint64_t max_cells, BuiltOctree &out, uint32_t &errors, bool &too_many, float *ms,
                                    DeviceOctree *dev = nullptr);

// Device-resident scene packing (octpt_scene_build_device): the sparse child-slot bases of a
// DeviceOctree (exclusive scan of the present-child counts; *d_base in the scratch, n_octants + 1
// entries, the last = slot count), then the slots, the single-sphere leaf table and the primitive
// tables, written exactly as octpt_scene_upload packs them on the host.
hipError_t slot_bases_gpu(hipStream_t stream, BuildScratch &scratch, const DeviceOctree &t, uint32_t **d_base,
                          uint32_t &n_slots);
struct ScenePrimTables {
    uint2 *node_child;   // n_slots + 8 (the tail zeroed by the caller)
    float4 *leaf_sph;    // sphere-only scenes, else nullptr
    uint32_t *leaf_prims;
    float4 *spheres;
    uint32_t *sphere_mat;
    float4 *cub_a;
    float2 *cub_b;
    uint32_t *cub_mat;
};
hipError_t fill_scene_gpu(hipStream_t stream, const DeviceOctree &t, const uint32_t *d_base,
                          const ScenePrimTables &out);
// The slots of a block-value octree (octpt_scene_build_blocks_device): octant child = (its base, its mask),
// leaf child = (block, bflags[block]); bflags = the host's block_slot_flags, one word per block, uploaded
// into the scratch.  node_child: n_slots + 8 (the tail zeroed by the caller).
hipError_t fill_block_scene_gpu(hipStream_t stream, BuildScratch &scratch, const DeviceOctree &t,
                                const uint32_t *d_base, const uint32_t *bflags, uint32_t n_blocks, uint2 *node_child);

// The emitter grid on the device (octpt_build.hip, C38), from the node slots of a resident block-value scene:
// a level-by-level walk of the octants (count, scan, fill), the emissive leaves marked and scanned, (Morton code,
// level) emitted and sorted, the 27-neighbourhood counted per cell, scanned and filled.  The three arrays are
// device allocations of their own (hipMalloc; the caller frees them), the temporaries the scratch's build slots.
// d_emissive: block_emissive_flags on the device.  refusal: OCTPT_OK, or OOM (a budget above) / INTERNAL (more
// octants reached than the scene counts) with nothing allocated.
struct DeviceEmitterGrid {
    uint32_t *cell_first = nullptr, *cell_emitters = nullptr;
    octpt_emitter *emitters = nullptr;
    uint32_t n_cells = 0, n_entries = 0, n_emitters = 0, cells_axis = 0, grid_shift = 0;
    uint32_t flags = 0;  // OCTPT_EMITTERS_MODELS: model emitters are listed (C39; set by the context)
};
// model_emissive (C39, OCTPT_EMITTERS_MODELS; NULL without it): the host's emissive byte of each of the scene's n_models
// models, which the leaf-count and record kernels test beside the per-block flag through S.blk_model; such a leaf's
// record is (x, y, z, 0x80000000 | model).
hipError_t build_emitter_grid_gpu(hipStream_t stream, BuildScratch &scratch, const DevScene &S,
                                  const uint32_t *emissive, uint32_t grid_shift, DeviceEmitterGrid &out,
                                  octpt_status &refusal, const uint8_t *model_emissive = nullptr,
                                  uint32_t n_models = 0u);


// The sky map's distribution on the device (C43, octpt_build.hip): the arrays of csrc/octpt_sky_sample.h built from the
// map the context holds (sky.texels: sanitised device texels) -- a weight kernel, a max reduction, a quantise kernel,
// one scan per row and the scan of the rows' totals -- equal to octpt_build_sky_distribution's integer for integer.
// row: the host's table of sin(pi (y + 0.5) / H), height floats.  The arrays are the caller's to free.
struct DeviceSkyDist {
    uint64_t *row_cdf = nullptr;
    uint32_t *col_cdf = nullptr;
    uint64_t total = 0;
    uint32_t width = 0, height = 0;
    float build_ms = 0.0f;  // the device's time from the weight kernel to the marginal scan
};
hipError_t build_sky_distribution_gpu(hipStream_t stream, const Sky &sky, const float *row, DeviceSkyDist &out);
// octpt_sky_sample_device's kernel: sky_sample_draws for n tuples of four draws, eight floats out each
hipError_t launch_sky_sample(const Sky &sky, const SkyDist &dist, const float *u, uint32_t n, float *out,
                             hipStream_t stream);

}  // namespace octpt

struct octpt_octree : octpt::BuiltOctree {};  // the C ABI's octree handle
