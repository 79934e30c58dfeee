/*
 * octpt.h -- C ABI of the MI355X-native octree path-tracing hot path.
 *
 * This is the drop-in boundary that replaces the reference's GPU backend
 * (kekley/octree_pathtracing, src/renderer/gpu_renderer.rs:151-702, implementing
 * trait RenderingBackend, src/renderer/renderer_trait.rs:19-46).  A Rust host binds
 * these symbols with an `extern "C"` block and keeps its own
 * Scene / Octree / Camera types; every struct below is #[repr(C)]-compatible.
 *
 * Conventions
 *  - Every entry returns octpt_status (int32).  No C++ exception crosses the ABI.
 *  - Input arrays are borrowed for the duration of the call and deep-copied.
 *  - A context is externally synchronised (one host thread at a time); distinct
 *    contexts are independent.  Frames returned by octpt_render_async are owned by
 *    the caller until octpt_frame_release.
 *  - There is no CPU fallback: without a usable gfx950 device octpt_create fails
 *    with OCTPT_ERR_DEVICE.
 *  - "Drop-in": src/octree is used unchanged (the raw octant masks come from Octant's public is_child /
 *    is_leaf / get_child).  A Rust host binding this header adds one accessor to the
 *    reference, Sun::octpt_args in src/scene/mod.rs (Sun's texture, colour and draw flag are private), and
 *    supplies the block table (block value -> face materials / model) that its resource manager resolves and
 *    Scene does not hold.  src/app and the rest of src/scene are untouched.
 */
#ifndef OCTPT_H
#define OCTPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCTPT_ABI_VERSION 4u

typedef int32_t octpt_status;
#define OCTPT_OK 0
#define OCTPT_ERR_INVALID_ARG 1
#define OCTPT_ERR_OOM 2
#define OCTPT_ERR_DEVICE 3
#define OCTPT_NOT_READY 4     /* FrameInFlightPoll::NotReady (renderer_trait.rs:37-41) */
#define OCTPT_ERR_UNSUPPORTED 5
#define OCTPT_CANCELLED 6     /* FrameInFlightPoll::Cancelled */
#define OCTPT_ERR_INTERNAL 7

typedef struct octpt_ctx octpt_ctx;
typedef struct octpt_frame octpt_frame;
typedef struct octpt_octree octpt_octree;

/* new_octree::Octant (src/octree/new_octree.rs:70-74) in C layout, 36 bytes.
 * Two mask bits per child i, (bit i, bit i+8):
 *   (0,0) empty; (1,1) leaf, children[i] = the leaf payload (leaf table index);
 *   (1,0) octant, children[i] = octant index -- the OctantChildIterator reading
 *         (new_octree.rs:84-100), what octpt_build_octree writes;
 *   (0,1) octant, children[i] = octant index -- the form Octant::set_mask_for writes for
 *         ChildType::Octant (new_octree.rs:160-178), i.e. every tree the reference's
 *         expand_by / RegionOctreeBuilder / SectionOctantBuilder build.
 * Leaves may sit at any level (LOD leaves above the bottom, new_octree.rs:534-536).
 * Child index i = x | y << 1 | z << 2 (the ESVO/Morton child order, octree_traversal.rs:22-24). */
typedef struct octpt_octant {
    uint16_t child_mask;
    uint16_t reserved;
    uint32_t children[8];
} octpt_octant;

/* geometry::sphere::Sphere (src/geometry/sphere.rs:10-14), 32 bytes */
typedef struct octpt_sphere {
    float center[3];
    float radius;
    uint32_t material;
    uint32_t reserved[3];
} octpt_sphere;

/* geometry::cuboid::Cuboid (src/geometry/cuboid.rs:48-52): AABB + one material per face,
 * Face order West(-X), East(+X), Bottom(-Y), Top(+Y), South(+Z), North(-Z).  48 bytes. */
typedef struct octpt_cuboid {
    float min[3];
    float max[3];
    uint32_t face_material[6];
} octpt_cuboid;

/* Block models.  A leaf cuboid whose cuboid_model entry is not
 * OCTPT_MODEL_NONE is a Minecraft block-model instance (the reference's ResourceModel::Quad leaf,
 * octree_traversal.rs:207-213; Scene::quads, scene/mod.rs:153): its box is the voxel [min, min+1)
 * and its surface is the model's quads, tested with Quad::hit (src/geometry/quad.rs:172-200) in
 * voxel-local coordinates, instead of the six faces of the box.
 * geometry::quad::Quad::new arguments (quad.rs:90-114): origin, edge vectors u and v (voxel-local,
 * the block is [0,1]^3), texture u/v ranges (the face's uv rectangle / 16) and the material.
 * The plane, normal and w = n / (n.n) are derived at upload exactly as Quad::new does.  64 bytes. */
typedef struct octpt_quad {
    float origin[3];
    uint32_t material;
    float u[3];
    float v[3];
    float texture_u_range[2];
    float texture_v_range[2];
    uint32_t reserved[2];
} octpt_quad;
/* gpu_structs::model::Model (src/gpu_structs/model.rs:14-21): the model's quads are
 * quads[first_quad .. first_quad + quad_count).  16 bytes. */
typedef struct octpt_block_model {
    uint32_t flags; /* reserved, 0 */
    uint32_t first_quad, quad_count;
    uint32_t reserved;
} octpt_block_model;
#define OCTPT_MODEL_NONE 0xFFFFFFFFu

/* GPUMaterial (src/gpu_structs/gpu_material.rs:67-76), 32 bytes */
typedef struct octpt_material {
    float ior, specular, emittance, roughness, metalness;
    uint32_t texture_index, tint_index, flags; /* flags: MaterialFlags bits (material.rs:99-108) */
} octpt_material;

#define OCTPT_TEXTURE_COLOR 0u /* Texture::Color(U8Color)  (texture.rs:15-18) */
#define OCTPT_TEXTURE_IMAGE 1u /* Texture::Image(RTWImage), RGBA8, row-major, top row first */
typedef struct octpt_texture {
    uint32_t kind;
    uint8_t rgba[4];
    uint32_t width, height;
    const uint8_t *pixels; /* width*height*4 bytes for OCTPT_TEXTURE_IMAGE, else NULL */
} octpt_texture;

/* scene::Sun::new arguments (src/scene/mod.rs:321-330) + SunSamplingStrategy flags (:60-69) */
typedef struct octpt_sun {
    float azimuth, altitude, radius;
    float color[4];
    float apparent_color[3];
    int32_t draw_texture, texture_modification;
    float importance_sample_chance, importance_sample_radius;
    float luminosity;
    uint8_t texture_rgba[4];
    int32_t importance_sampling, diffuse_sun;
    /* next-event estimation toward the sun (do_diffuse_reflection, path_tracer.rs:225-291;
     * get_direct_light_attenuation :458-483): presets FAST / HIGH_QUALITY (scene/mod.rs:98-126) */
    int32_t sun_sampling, strict_direct_light, sun_luminosity;
    float luminosity_pdf; /* Sun::luminosity_pdf, 1/100 in Sun::new (scene/mod.rs:376) */
} octpt_sun;

/* Block-value leaves: the reference's own leaf form.  Every octree the reference
 * builds stores a u32 block value in its leaves -- (ChildType::Leaf, value) (new_octree.rs:669),
 * Lod(section_fill_block) (:727), Lod(data) one or more levels up (:534-537, 586) -- and traverses
 * such a leaf as the cell itself (octree_traversal.rs:143-214).  With octpt_scene_desc.blocks set, a
 * leaf payload is an index into this table, at any level:
 *  - model == OCTPT_MODEL_NONE: the block fills its leaf cell (ResourceModel::SingleBlock, :193-206).
 *    The face is the cell face the ray enters, the texture coordinates its entry point over the cell
 *    (:156-190), the material face_material[face]; a texel with alpha <= EPSILON lets the ray through
 *    (the traversal advances), and a ray that starts inside the cell passes it (t_min == 0, :194);
 *  - else the block model (C19) drawn at the leaf cell's corner in unit-voxel coordinates
 *    (ResourceModel::Quad, :207-213).
 * Face order West(-X), East(+X), Bottom(-Y), Top(+Y), South(+Z), North(-Z) (cuboid.rs:9-29).  32 bytes. */
typedef struct octpt_block {
    uint32_t face_material[6];
    uint32_t model;
    uint32_t reserved;
} octpt_block;

/* Scene (src/scene/mod.rs:146-156) flattened: octree + leaf primitive lists + primitive,
 * material and texture tables.  Leaf payload p indexes leaf_first/leaf_count; the prims
 * leaf_prims[first .. first+count) are sphere indices, or cuboid indices | 0x80000000.
 * With `blocks` set the leaf payloads are block ids instead (C23): leaf_*, spheres and cuboids
 * must then be empty, and block models draw from models / quads. */
typedef struct octpt_scene_desc {
    uint32_t abi_version; /* = OCTPT_ABI_VERSION */
    const octpt_octant *octants;
    uint32_t octant_count, root, depth; /* depth <= 21 (new_octree.rs:14); world = [0, 2^depth)^3 */
    const uint32_t *leaf_first;
    const uint32_t *leaf_count;
    uint32_t leaf_table_size;
    const uint32_t *leaf_prims;
    uint32_t leaf_prim_count;
    const octpt_sphere *spheres;
    uint32_t sphere_count;
    const octpt_cuboid *cuboids;
    uint32_t cuboid_count;
    const octpt_material *materials; /* materials[0] is the outer medium (air) */
    uint32_t material_count;
    const octpt_texture *textures;
    uint32_t texture_count;
    octpt_sun sun;
    int32_t emitters_enabled;
    float f_sub_surface; /* Scene::f_sub_surface (scene/mod.rs:152): subsurface sun-sample chance */
    /* block models (C19): cuboid_model (nullable = no models) holds one entry per cuboid,
     * OCTPT_MODEL_NONE for a plain box or a model index; such a cuboid must be a unit voxel */
    const uint32_t *cuboid_model;
    const octpt_block_model *models;
    uint32_t model_count;
    const octpt_quad *quads;
    uint32_t quad_count;
    /* block-value leaves (C23): NULL = primitive leaves */
    const octpt_block *blocks;
    uint32_t block_count;
} octpt_scene_desc;

/* renderer::camera::Camera (src/renderer/camera.rs:8-25) */
typedef struct octpt_camera {
    float eye[3];
    float direction[3];
    float up[3];
    float fov; /* radians */
    /* The thin lens (Camera::focus, camera.rs:68-73): aperture is the lens radius in world units,
     * >= 0 and finite, 0 = pinhole; focal_distance is the distance along `direction` of the plane in focus, > 0
     * and finite whenever aperture > 0 and not read at all when aperture is 0.  Path-traced renders start each
     * path on a point of the lens drawn from a stream of its own, so the path's other draws are what they are
     * without a lens.  OCTPT_RENDER_PREVIEW and the guide buffers (octpt_render_aov*) keep tracing the ray through
     * the lens centre, bit for bit unchanged by the aperture (sharp guides for the filters).  octpt_temporal* and
     * octpt_reproject_coords refuse a camera with an aperture (UNSUPPORTED): pass them the camera with aperture 0. */
    float aperture, focal_distance;
} octpt_camera;

/* One progressive render call = spp_count passes of TileRenderer::render_tile_average
 * (tile_renderer.rs:684-734) continuing a running mean that already holds spp_start samples. */
#define OCTPT_RENDER_SHARD_COMPACT 0x1u /* accum holds only this shard's 8x8 tiles, tile-major */
#define OCTPT_RENDER_MEGAKERNEL 0x2u    /* single persistent megakernel instead of the wavefront loop (A/B) */
#define OCTPT_RENDER_KERNEL_TIMING 0x4u /* bracket every extend / shade launch with HIP events (octpt_stats) */
/* RendererMode::Preview (tile_renderer.rs:293, render_tile_replace :648-682; preview_render,
 * path_tracer.rs:137-158): one un-jittered camera ray per pixel, flat-shaded by the sun
 * (Sun::flat_shading, scene/mod.rs:447-452); rgb is replaced, alpha kept; spp/max_depth ignored */
#define OCTPT_RENDER_PREVIEW 0x8u
typedef struct octpt_render_params {
    uint32_t width, height;
    uint32_t spp_start, spp_count;
    uint32_t max_depth;    /* reference: 5 (path_tracer.rs:56) */
    uint32_t branch_count; /* TileRenderer branch count B <= 64: passes of weight
                            * get_current_branch_count(spp, B), the first reflection split into that many
                            * branches; spp_start and spp_start + spp_count must be pass boundaries */
    uint32_t seed;
    uint32_t shard_index, shard_count; /* 8x8 tile t belongs to shard t % shard_count */
    uint32_t flags;
} octpt_render_params;

/* statistics counter order of octpt_stats::drain */
#define OCTPT_STAT_PATHS 0
#define OCTPT_STAT_SEGMENTS 1
#define OCTPT_STAT_ESVO_STEPS 2
#define OCTPT_STAT_SPHERE_TESTS 3
#define OCTPT_STAT_CUBOID_TESTS 4
#define OCTPT_STAT_SHADE_EVENTS 5
#define OCTPT_STAT_TEXEL_READS 6
#define OCTPT_STAT_BLOCK_TESTS 7
#define OCTPT_STAT_ISSUED_BYTES 8
#define OCTPT_STAT_COUNT 9
typedef struct octpt_stats {
    /* esvo_steps: ESVO iterations executed; camera rays start at their tile's beam start, so
       this is the reference walk's count only with OCTPT_BEAM=0 -- every other field is the same either way */
    uint64_t paths, segments, esvo_steps, sphere_tests, cuboid_tests, shade_events, texel_reads;
    uint64_t launches;
    double kernel_ms; /* HIP-event time of the render calls since the last reset */
    /* per-kernel HIP-event time of the wavefront loop, renders flagged OCTPT_RENDER_KERNEL_TIMING only */
    uint64_t extend_launches, shade_launches;
    double extend_ms, shade_ms;
    double build_ms; /* device time (upload excluded) of the last octpt_build_octree_device */
    uint64_t block_tests;  /* block-value leaf tests */
    /* bytes of the loads wf_extend_kernel issues (node slots actually loaded, primitives, quads, alpha
     * texels): counted only by the OCTPT_COUNT_ISSUED diagnostic build of the library, else 0 */
    uint64_t issued_bytes;
    /* the chunk-tail drain kernel's share of the counters above, in OCTPT_STAT_* order (included in
     * the totals; the extend roofline subtracts it) */
    uint64_t drain[OCTPT_STAT_COUNT];
    uint64_t pool_slots;  /* path slots held by the wavefront state (after any out-of-memory fallback) */
    uint64_t chunk_items; /* (pixel, sample) items per chunk held (likewise) */
    uint64_t wave_allocs; /* wavefront-state (re)allocations since the context was created */
    /* camera rays whose beam start reached the reference's step cap and were traced again from the
     * cube entry (their iterations before the restart are in esvo_steps too) */
    uint64_t beam_restarts;
    /* hit records a field of which the path that produced the hit left unwritten: counted only by the
     * OCTPT_CHECK_HITS diagnostic build of the library, else 0 */
    uint64_t hit_check_failures;
} octpt_stats;

/* --- library / context ------------------------------------------------------ */
uint32_t octpt_abi_version(void);
/* number of visible HIP devices (0 when none) */
int32_t octpt_device_count(void);
/* RenderingBackend construction (gpu_renderer.rs:151-200) on HIP device `device` */
octpt_status octpt_create(int32_t device, octpt_ctx **out);
/* A context over several GPUs of one node (SURVEY.md §8(b) device list, §8(e) tile split):
 * devices[0 .. n) are HIP device ids, n <= 64; an id may repeat (two entries on one GPU).  Every entry
 * point takes such a context: the scene is replicated on every entry, a render deals the 8x8 tiles of the
 * call's shard round-robin over the entries (each renders its tiles concurrently, on a host thread of its
 * own) and gathers them with peer copies into the caller's buffers, which live on devices[0]
 * (octpt_render_device's d_accum / d_seg_count and stream).  Results are bit-identical to one device's.
 * octpt_intersect runs on devices[0]; octpt_stats sums the entries' counters, kernel_ms is the render
 * calls' wall time.  n == 1 is octpt_create(devices[0]). */
octpt_status octpt_create_multi(const int32_t *devices, uint32_t n, octpt_ctx **out);
/* device entries of a context (1 for octpt_create; 0 for NULL) */
uint32_t octpt_device_entries(const octpt_ctx *ctx);
void octpt_destroy(octpt_ctx *ctx);
/* last error message of this context (never NULL) */
const char *octpt_last_error(const octpt_ctx *ctx);

/* --- RenderingBackend surface ----------------------------------------------- */
/* set_scene (gpu_renderer.rs:662-669 -> create_pipeline :201-557): validates and uploads */
octpt_status octpt_scene_upload(octpt_ctx *ctx, const octpt_scene_desc *scene);
/* set_scene with the octree built on the device and kept there (the reference's
 * flattener octree_to_gpu_data, gpu_octree.rs:28-76, is todo!()).  The scene's octree fields
 * (octants, octant_count, root, leaf_*) must be NULL / 0; `depth` is the build depth and flags are
 * the builder's (OCTPT_BUILD_COMPACT).  The primitives are uploaded once, voxelised by the GPU
 * builder and its arrays packed into the device node slots in place: the resulting device scene is
 * the one octpt_scene_upload makes from octpt_build_octree_ex's octree, with no round trip through
 * host memory. */
octpt_status octpt_scene_build_device(octpt_ctx *ctx, const octpt_scene_desc *scene, uint32_t flags);
/* set_camera / get_camera (renderer_trait.rs:20-21).  INVALID_ARG, the camera staying as it was: fov outside
 * (0, pi), an aperture that is negative or not finite, aperture > 0 with a focal_distance that is not finite
 * and > 0.  With an aperture the camera rays' beam starts are not used (they assume rays from the eye). */
octpt_status octpt_set_camera(octpt_ctx *ctx, const octpt_camera *camera);
octpt_status octpt_get_camera(const octpt_ctx *ctx, octpt_camera *camera);

/* The camera's projection: how a pixel's position (sx, sy) -- C37's, jitter included, in units of half
 * the longer image side -- becomes a path's first ray.  It changes that ray and nothing else; a path's random draws are
 * the same in every mode.
 *   PINHOLE    the perspective view of octpt_camera::fov (the state of a new context); param is not read
 *   PARALLEL   every ray along `direction`, from eye + right * (sx * param / 2) + up * (sy * param / 2): param is the
 *              world-space length the longer image side spans, finite and > 0 (isometric map renders)
 *   FISHEYE    equidistant: the angle from `direction` is |(sx, sy)| * param / 2
 *   PANORAMIC  equirectangular: longitude sx * param / 2 about `up`, latitude sy * param / 2 (a 360-degree panorama is
 *              param = 2 pi at width = 2 * height)
 * For FISHEYE and PANORAMIC param is the full angle in radians across the longer image side, finite and in (0, 2 pi]
 * (the float nearest 2 pi included).  octpt_camera::fov is not read in the three new modes -- no ray depends on it --
 * but octpt_set_camera and octpt_projection_rays still validate it: a camera is valid or not whatever the projection.
 * Unknown mode: UNSUPPORTED.  A bad param or a non-zero reserved word: INVALID_ARG.  A mode other than PINHOLE while
 * the context's camera has an aperture: UNSUPPORTED, and likewise octpt_set_camera with an aperture while the
 * projection is not PINHOLE (the camera then stays as it was).  A refused call leaves the setting as it was.
 * The call joins a frame in flight and the setting holds for every later render of the context: sync, device, async,
 * tile list, adaptive, final, megakernel, and with the un-jittered ray the preview and the guide buffers; every entry
 * of a multi-device context follows it.  Camera-ray beam starts are off while it is not PINHOLE.  octpt_temporal*
 * and octpt_reproject_coords_ctx refuse (UNSUPPORTED) while it is not PINHOLE: reprojection is the pinhole camera's. */
#define OCTPT_PROJECTION_PINHOLE 0u /* the state of a new context */
#define OCTPT_PROJECTION_PARALLEL 1u
#define OCTPT_PROJECTION_FISHEYE 2u
#define OCTPT_PROJECTION_PANORAMIC 3u
typedef struct octpt_projection {
    uint32_t mode;
    float param;
    uint32_t reserved[6]; /* 0 */
} octpt_projection;
octpt_status octpt_set_projection(octpt_ctx *ctx, const octpt_projection *projection);
octpt_status octpt_get_projection(const octpt_ctx *ctx, octpt_projection *projection);

/* The ray source: a path's first ray read from a buffer the caller fills, so that any camera -- a
 * stereo panorama, a cube-map face, a distorted lens, a light probe -- is a few lines of host code.  The ray of sample
 * s of pixel (x, y) is the six floats at d_rays[6 * ((y * width + x) * rays_per_pixel + s % rays_per_pixel)]: origin
 * xyz, then direction xyz; s is the absolute sample index (spp_start plus the index in the call), so split calls go on
 * through the list, and samples beyond rays_per_pixel wrap round.  The floats are used as given (the direction is not
 * renormalised).  A record is valid when all six floats are finite and the direction's squared length, (dx^2 + dy^2) +
 * dz^2 in f32, lies within 1e-4 of 1; an invalid record is replaced whole by the central ray of the context's camera
 * (eye, direction), so no bit pattern in the buffer makes anything but an ordinary path.  Only the first ray changes:
 * a path's random draws are what they are under every other camera (the two jitter draws are made and dropped).
 * d_rays is memory of the context's device and stays the caller's: it must remain valid and unchanged until every
 * render that reads it has completed.  The call joins a frame in flight; the setting is read when a render call is
 * made and holds until it is cleared (a NULL source or NULL d_rays; the other fields are then not read).
 * Followed by: sync, device, async, tile-list, adaptive and final wavefront renders, strategy ONE emitter sampling
 * included; OCTPT_RENDER_PREVIEW and the guide buffers (octpt_render_aov*) trace ray 0 of each pixel, the depth guide
 * being the distance from that ray's origin.  Camera-ray beam starts are off under a source.
 * INVALID_ARG: a non-zero reserved word, rays_per_pixel, width or height 0, width * height * rays_per_pixel above
 * 2^28, and a render whose width or height is not the source's.  UNSUPPORTED: a multi-device context; a camera with an
 * aperture or a projection other than PINHOLE -- and, while a source is set, octpt_set_camera with an aperture and
 * octpt_set_projection with another mode (whichever comes second is refused, the earlier setting stays); a render with
 * OCTPT_RENDER_MEGAKERNEL; octpt_temporal* and octpt_reproject_coords_ctx.  Every check comes before any write: a
 * refused call changes nothing.  With the source cleared every render is bit for bit that of a context that never
 * had one. */
typedef struct octpt_ray_source {
    const float *d_rays;     /* device memory of the context's device; NULL = no ray source (the state of a new context) */
    uint32_t width, height;  /* the frame the list is for */
    uint32_t rays_per_pixel; /* R >= 1 */
    uint32_t reserved[5];    /* 0 */
} octpt_ray_source;
octpt_status octpt_set_ray_source(octpt_ctx *ctx, const octpt_ray_source *source);
octpt_status octpt_get_ray_source(const octpt_ctx *ctx, octpt_ray_source *source);

/* The sky: the base colour a ray that leaves the world adds, at every depth, in the drain and in the
 * preview, where every render used to add the constant (0.5, 0.7, 1.0).  The sun's texture, its diffuse term and
 * next-event estimation are untouched and add on top.  A sky changes no random draw: a path's geometry is the same
 * under every sky.  For a unit direction d in world axes, +y up (one text, csrc/octpt_sky.h, compiled by the kernels
 * and by octpt_sky_radiance):
 *   DEFAULT   (0.5, 0.7, 1.0), the state of a new context; no other field is read
 *   COLOR     color * scale
 *   GRADIENT  (horizon + (zenith - horizon) * max(d.y, 0)) * scale: horizon * scale below the horizon
 *   MAP       an equirectangular map of width x height texels of four floats each (RGBA; alpha is not read), row 0 the
 *             zenith: lon = atan2(d.z, d.x) + yaw, u = lon / 2pi + 0.5 wrapped into [0, 1), v = acos(d.y) / pi; bilinear
 *             between the texels at floor and floor + 1 of (u * width - 0.5, v * height - 0.5), wrapped in x and clamped
 *             in y, each lerp a + w * (b - a), then times scale.  +x is the map's centre column at yaw 0.  At the poles
 *             the value is the top or bottom row's at the column of longitude `yaw`.
 * The context copies a MAP's texels into a buffer of its own before the call returns (the caller may free its own), and
 * sanitises them once: NaN and negative become 0, +inf becomes FLT_MAX; a lookup is held at FLT_MAX after the scale.
 * color, horizon and zenith are used as given.  octpt_set_sky takes host texels, octpt_set_sky_device texels in memory
 * of the context's device (copied on `hip_stream`, which the call drains); texels is read for MAP alone.
 * octpt_clear_sky is DEFAULT again, and every render is then bit for bit that of a context that never had a sky.
 * The call joins a frame in flight and the setting holds for every later render of the context: sync, device, async,
 * tile-list, adaptive and final renders under every camera (pinhole, aperture, projection, ray source), with and without
 * sun sampling and strategy ONE emitter sampling, and OCTPT_RENDER_PREVIEW.  The guide buffers (octpt_render_aov*)
 * describe hits and write zeros and an infinite depth for a miss under every sky.  Under a sky other than DEFAULT a
 * render takes the general path state (never the lean one) through the sky's own kernel instances.
 * INVALID_ARG, the previous sky staying in force: an unknown mode, a non-zero reserved word, a scale that is NaN,
 * negative or infinite, a yaw that is not finite, MAP with NULL texels, with width or height 0, or with width * height
 * above 2^26.  UNSUPPORTED: a mode other than DEFAULT on a multi-device context (the setting stays DEFAULT), and a
 * render with OCTPT_RENDER_MEGAKERNEL while the sky is not DEFAULT (the caller's buffers are not touched). */
#define OCTPT_SKY_DEFAULT 0u /* the state of a new context */
#define OCTPT_SKY_COLOR 1u
#define OCTPT_SKY_GRADIENT 2u
#define OCTPT_SKY_MAP 3u
typedef struct octpt_sky {
    uint32_t mode;
    float color[3];   /* COLOR */
    float horizon[3]; /* GRADIENT */
    float zenith[3];  /* GRADIENT */
    float scale;      /* every mode but DEFAULT */
    float yaw;        /* MAP: radians added to the longitude */
    uint32_t width, height; /* MAP */
    uint32_t reserved[2];   /* 0 */
} octpt_sky;
octpt_status octpt_set_sky(octpt_ctx *ctx, const octpt_sky *sky, const float *texels);
octpt_status octpt_set_sky_device(octpt_ctx *ctx, const octpt_sky *sky, const float *d_texels, void *hip_stream);
octpt_status octpt_clear_sky(octpt_ctx *ctx);
octpt_status octpt_get_sky(const octpt_ctx *ctx, octpt_sky *sky);
/* The colour a render adds for n unit directions (dirs[3 * i], out[3 * i]; the sun's terms excluded).
 * octpt_sky_radiance is host-only and knows no context: it runs csrc/octpt_sky.h on the CPU for `sky` and host texels
 * (sanitised as octpt_set_sky sanitises them; octpt_set_sky's argument rules, every check before the first write).
 * octpt_sky_radiance_device runs a kernel of the same text for the context's sky (device buffers, on `hip_stream`),
 * octpt_sky_radiance_ctx is its host-pointer form.  The three agree bit for bit. */
octpt_status octpt_sky_radiance(const octpt_sky *sky, const float *texels, const float *dirs, uint32_t n, float *out);
octpt_status octpt_sky_radiance_device(octpt_ctx *ctx, const float *d_dirs, uint32_t n, float *d_out, void *hip_stream);
octpt_status octpt_sky_radiance_ctx(octpt_ctx *ctx, const float *dirs, uint32_t n, float *out);
/* DIAGNOSTIC, not part of the stable surface (it may change or go with the lookup's arithmetic; hosts have no use for
 * it).  A MAP's lookup position alone: out_xy[2 * i] = (u * width - 0.5, v * height - 0.5) of direction i in f32, as the
 * lookup forms it (mode MAP, width, height and yaw are read; no texels).  Host-only; what the error bound of the
 * lookup against a float64 restatement is measured from. */
octpt_status octpt_sky_map_position(const octpt_sky *sky, const float *dirs, uint32_t n, float *out_xy);

/* Importance sampling of the sky map: next-event estimation toward the map's bright texels.  Off by
 * default; with it off every render is bit for bit what it is without this call.
 * The distribution (one text, csrc/octpt_sky_sample.h, compiled by the host builder, the device builder and the
 * kernels) is piecewise constant over the texels of the sanitised map and made of integers:
 *   lum(x, y) = min((0.2126 r + 0.7152 g) + 0.0722 b, FLT_MAX);  m = the maximum of lum over the 3 x 3 neighbourhood,
 *   wrapped in x and clamped in y (the bilinear lookup's footprint: the weight is non-zero wherever the lookup can be);
 *   w = min(m * row[y], FLT_MAX), row[y] = (float)sin(pi (y + 0.5) / height) computed in double;  wmax = max w;
 *   q = 0 where w == 0, else clamp((uint32)ceilf((w / wmax) * 65536), 1, 65536);
 *   col_cdf[y * width + x] (uint32) the inclusive sum of q along row y, row_cdf[y] (uint64) the inclusive sum of the
 *   rows' totals, total = row_cdf[height - 1] (0: an all-black map).
 * octpt_build_sky_distribution is the definition: host-only, no context; texels as octpt_set_sky takes them
 * (sanitised the same way), row_cdf[height] and col_cdf[width * height] the caller's.  INVALID_ARG: a NULL pointer,
 * width or height 0, width * height above 2^26.  UNSUPPORTED: width above 32768 (a row's total must fit 32 bits).
 * The setting: mode NONE (the default) or MAP, reserved words 0; an unknown mode or a non-zero reserved word is
 * INVALID_ARG and the setting stays.  The call joins a frame in flight, holds for later renders and may come before
 * or after the sky.  While the mode is MAP and the context's sky is a MAP, the context holds the map's distribution,
 * built on its device from the texels resident there (equal to octpt_build_sky_distribution's integer for integer):
 * built by whichever of the two calls comes second, rebuilt by a new map, dropped by octpt_clear_sky, a sky of another
 * mode or the mode NONE.  scale and yaw do not enter it.  When the build itself fails (OOM, DEVICE) the call that
 * asked for it returns that status: octpt_set_sky has then installed the new sky, octpt_set_sky_sampling keeps its
 * previous mode, and the context holds no distribution -- renders follow the sky unsampled until a later call builds one.
 * The estimator (sync, device, async, tile-list, adaptive and final renders, every camera form): at every diffuse
 * reflection a texel is picked from an RNG stream of its own (no draw of the path changes), a direction d inside it,
 * and, when d lies above the surface, one shadow segment is traced from hit + n * OFFSET along d (counted like the
 * sun's; any reported hit blocks it); when it leaves the world, L += T_before * albedo * sky_radiance(d) *
 * (d.n / pi) / pdf.  The bounce drawn at that reflection adds no base sky colour when its own segment leaves the world
 * (the sun's terms add as ever); a camera ray, a specular chain and a bounce that passed a transparent surface see the
 * map as before.  With sun sampling the sky segment runs first, then the sun's, then the bounce.
 * Inert, bit for bit the unsampled render through the instances it takes today: MAP sampling under a DEFAULT, COLOR
 * or GRADIENT sky and under an all-black map.  The preview and the guide buffers ignore the setting.
 * UNSUPPORTED (the setting stays; a refused render leaves the caller's buffers untouched): MAP on a multi-device
 * context; MAP while emitter sampling is ONE, and octpt_set_emitter_sampling(ONE) while the mode is MAP (whichever call
 * comes second; and the render call); a render with OCTPT_RENDER_MEGAKERNEL while the mode is MAP; MAP while the
 * resident map is wider than 32768.  A map wider than that set while the mode is MAP is accepted and renders
 * unsampled. */
#define OCTPT_SKY_SAMPLING_NONE 0u /* the state of a new context */
#define OCTPT_SKY_SAMPLING_MAP 1u
typedef struct octpt_sky_sampling {
    uint32_t mode;
    uint32_t reserved[7]; /* 0 */
} octpt_sky_sampling;
octpt_status octpt_set_sky_sampling(octpt_ctx *ctx, const octpt_sky_sampling *sampling);
octpt_status octpt_get_sky_sampling(const octpt_ctx *ctx, octpt_sky_sampling *sampling);
octpt_status octpt_build_sky_distribution(const float *texels, uint32_t width, uint32_t height, uint64_t *row_cdf,
                                          uint32_t *col_cdf);
/* The context's distribution, copied back from its device in count-then-fill form (as octpt_emitter_grid_arrays):
 * width and height are always received (0 when the context holds none -- sampling off, no MAP, or a dropped one -- and
 * on an error; nothing is written then and the call is OK).  With both pointers NULL the call only counts.  Otherwise
 * both must be set with capacities (in elements) of at least height and width * height, else nothing is written and
 * the call is INVALID_ARG.  build_ms: the device's time for the last build. */
typedef struct octpt_sky_distribution_arrays {
    uint64_t *row_cdf;
    uint64_t row_cdf_capacity;
    uint32_t *col_cdf;
    uint64_t col_cdf_capacity;
    uint32_t width, height;
    float build_ms;
    uint32_t reserved;
} octpt_sky_distribution_arrays;
octpt_status octpt_sky_distribution(octpt_ctx *ctx, octpt_sky_distribution_arrays *out);
/* The sample of n tuples of four draws u[4 * i .. 4 * i + 4) in [0, 1), as the estimator takes it from its stream
 * (csrc/octpt_sky_sample.h): row t = min((uint64)(u0 * (float)total), total - 1), the first y with t < row_cdf[y];
 * column s = min((uint32)(u1 * (float)rowsum), rowsum - 1), the first x with s < col_cdf[y * width + x]; u = (x + u2) /
 * width, v = (y + u3) / height, theta = pi v, lon = 2 pi (u - 0.5) - yaw brought into [-pi, pi]; d = (sin theta cos
 * lon, cos theta, sin theta sin lon); pdf = ((float)q / (float)total) * ((float)width * (float)height) / (2 pi^2 sin
 * theta) by solid angle.  out[8 * i ..]: d.xyz, pdf, then four 32-bit integers stored by bit pattern in the float
 * slots: x, y, q and 1 (a sample) or 0 (none -- total 0, sin theta <= 0 or a pdf not finite and positive -- with d and
 * pdf 0).  octpt_sky_sample is host-only: dist holds filled arrays of a width x height distribution, and of sky the
 * fields width, height and yaw are read (mode must be MAP).  octpt_sky_sample_device runs a kernel of the same text
 * over the context's distribution and sky (device buffers, on `hip_stream`; INVALID_ARG when the context holds no
 * distribution).  The two agree bit for bit. */
octpt_status octpt_sky_sample(const octpt_sky_distribution_arrays *dist, const octpt_sky *sky, uint32_t n,
                              const float *u, float *out);
octpt_status octpt_sky_sample_device(octpt_ctx *ctx, const float *d_u, uint32_t n, float *d_out, void *hip_stream);

/* Synchronous render into host memory.  accum_rgba: width*height*4 floats (or the shard's
 * compact tiles), in/out running mean, initialise to F32Color::BLACK (0,0,0,1).
 * out_rgba8 (nullable): tone-mapped U8Color image (colors/mod.rs:408-420) of accum. */
octpt_status octpt_render(octpt_ctx *ctx, const octpt_render_params *p, float *accum_rgba, uint8_t *out_rgba8);

/* Device-resident render: d_accum is a device pointer (same layout as accum_rgba), the
 * work is enqueued on `hip_stream` (hipStream_t, NULL = default stream).  The wavefront
 * loop is steered from the host (it reads back queue lengths), so the call returns once the
 * last kernel of the render is enqueued, i.e. after the render has essentially finished.
 * d_seg_count (nullable, device, one u32 per accum pixel) receives += ray segments. */
octpt_status octpt_render_device(octpt_ctx *ctx, const octpt_render_params *p, float *d_accum,
                                 uint32_t *d_seg_count, void *hip_stream);

/* render_frame (renderer_trait.rs:30-34) -> FrameInFlight (:42-46) */
octpt_status octpt_render_async(octpt_ctx *ctx, const octpt_render_params *p, float *accum_rgba,
                                uint8_t *out_rgba8, octpt_frame **out_frame);
octpt_status octpt_frame_poll(octpt_frame *frame);   /* OK = Ready, NOT_READY, CANCELLED */
octpt_status octpt_frame_wait(octpt_frame *frame);   /* FrameInFlight::wait_for */
octpt_status octpt_frame_cancel(octpt_frame *frame); /* result buffers are left untouched */
void octpt_frame_release(octpt_frame *frame);

/* Tone map a device accumulation buffer into device RGBA8 (colors/mod.rs:408-420). */
octpt_status octpt_tonemap_device(octpt_ctx *ctx, const float *d_accum, uint8_t *d_rgba8, uint32_t n_pixels,
                                  void *hip_stream);
/* Rank 0 of a sharded render: scatter shard_count compact tile buffers (device, concatenated
 * in shard order, each padded to `shard_stride_pixels`) into a full width*height frame. */
octpt_status octpt_unshard_device(octpt_ctx *ctx, uint32_t width, uint32_t height, uint32_t shard_count,
                                  const float *d_shards, uint32_t shard_stride_pixels, float *d_frame,
                                  void *hip_stream);
/* pixels a shard owns (its compact buffer length in pixels, tile-padded) */
uint32_t octpt_shard_pixels(uint32_t width, uint32_t height, uint32_t shard_index, uint32_t shard_count);

/* The tile deal (round 5).  The reference splits a frame into threads^2 tiles handed to a
 * thread pool (tile_renderer.rs:398-413); here a shard of N owns the 8x8 tiles at dealing positions
 * s = shard_index + u * N (its local tile u).  By default position s is frame tile s (round robin).
 * octpt_set_tile_order sets the frame tile at each position for width x height renders of this context
 * (order: ceil(W/8) * ceil(H/8) entries, a permutation; NULL = round robin again): renders, the async
 * frame, octpt_unshard_device and every entry of a multi-device context follow it, and a render of another
 * size is refused (INVALID_ARG) while it is set.  Per-pixel RNG streams keep the image bit-identical under
 * any order; the order only moves work between shards. */
octpt_status octpt_set_tile_order(octpt_ctx *ctx, uint32_t width, uint32_t height, const uint32_t *order);
/* A balanced order for shard_count shards from a previous render's per-pixel segment counts (seg_count:
 * width * height, image order, e.g. octpt_render's seg_count output): a tile's cost is the sum of its
 * pixels' counts; tiles go, most costly first, to the shard with the least cost so far among those with
 * positions left (each keeps its round-robin number of tiles), then each shard's tiles in image order.
 * Host-only, no context; writes `order` (as octpt_set_tile_order takes it). */
octpt_status octpt_balance_tiles(uint32_t width, uint32_t height, uint32_t shard_count, const uint32_t *seg_count,
                                 uint32_t *order);

/* Batch closest-hit query = Scene::hit (scene/mod.rs:172-187) with the octree traversal
 * (octree_traversal.rs:54-302) restored.  rays: n*6 floats (origin, unit direction), host.  ESVO's
 * 1 / -|d| is exact for direction components up to 2^126 (components below 2^-23 are clamped to it as
 * the reference does); a ray with a non-finite component or a direction component above 2^126 is
 * reported as a miss and the rest of the batch is traced.  For a non-finite ray that is the reference's
 * result; for a finite component above 2^126 it is a deliberate deviation (the reference's walk runs on a
 * subnormal t_coef, octree_traversal.rs:95, and may hit; parity unpinned).
 * last_prim / last_normal (nullable): self-intersection key per ray.
 * Outputs (host): t (world, +inf on miss), prim (0xFFFFFFFF on miss; in a block-value scene, C23, the
 * block id, or 0x40000000 | quad for a block model's quad), normal n*3 (nullable), esvo steps (nullable). */
octpt_status octpt_intersect(octpt_ctx *ctx, const float *rays, const uint32_t *last_prim, const float *last_normal,
                             uint32_t n, float *t, uint32_t *prim, float *normal, uint32_t *steps);

/* Octree::get_traversal_data (octree_traversal.rs:537-714), the beam-start query of
 * GPURenderer::render_frame (gpu_renderer.rs:579-581 -> CameraUniform.traversal_start_idx/scale,
 * index/time stack buffers :35-80).  Walks `ray` (origin xyz, direction xyz, world units) from
 * the root until the first leaf with t_min > 0 and returns the octant it stopped in, its scale
 * and the descent stacks, indexed by scale and zero where unwritten.  Host-only and stateless:
 * no context or device; `octants` is borrowed (the same layout as octpt_scene_desc).
 * max_dst in world units (Scene::hit uses 1024, scene/mod.rs:181). */
octpt_status octpt_traversal_data(const octpt_octant *octants, uint32_t octant_count, uint32_t root, uint32_t depth,
                                  const float ray[6], float max_dst, uint32_t *start_octant, uint32_t *scale,
                                  uint32_t index_stack[24], float time_stack[24]);
octpt_status octpt_get_stats(const octpt_ctx *ctx, octpt_stats *stats);
octpt_status octpt_reset_stats(octpt_ctx *ctx);

/* --- first-hit guide buffers and the preview denoiser ---------------------- */
/* Camera::get_ray (camera.rs:77-86) at the pixel centres of a width x height frame: rays[6 * (y * width + x)]
 * = (origin xyz, unit direction xyz), image order, top row first.  The same f32 expressions in the same
 * order as octpt_set_camera's basis and the kernels' un-jittered camera ray (preview, guide buffers), so a
 * ray from here is bit-identical to the ray the device traces for that pixel: what a host needs to turn a
 * mouse click into an octpt_intersect ray.  Host-only, no context. */
octpt_status octpt_camera_rays(const octpt_camera *camera, uint32_t width, uint32_t height, float *rays);
/* The first ray of a path-traced sample: rays[6 * (y * width + x)] = (origin xyz, unit direction
 * xyz) of the ray that a render of this size and seed traces for sample `sample` (spp_start + the sample's index in
 * the call) of pixel (x, y) -- jittered, and with an aperture leaving its point of the lens -- bit for bit: the
 * kernels and this entry compile one text (csrc/octpt_lens.h).  octpt_camera_rays' argument rules and
 * octpt_set_camera's for aperture and focal_distance; a failed call writes nothing.  Host-only, no context. */
octpt_status octpt_lens_rays(const octpt_camera *camera, uint32_t width, uint32_t height, uint32_t seed,
                             uint32_t sample, float *rays);
/* The first ray under a projection, for n chosen samples: xys[3 * i] = (x, y, sample) and
 * rays[6 * i] = (origin xyz, unit direction xyz) of the ray that a width x height render with this seed traces for
 * that sample of pixel (x, y) under `projection`, bit for bit (one text, csrc/octpt_lens.h).  rng_state (nullable):
 * rng_state[i] = the path's RNG state after the ray, the same in every mode.  With OCTPT_PROJECTION_RAYS_CENTRE the
 * rays are the un-jittered ones of OCTPT_RENDER_PREVIEW and the guide buffers (the sample is not read, rng_state gets
 * the path's initial state).  PINHOLE gives octpt_lens_rays' ray (octpt_camera_rays' with the flag); the camera
 * follows octpt_lens_rays' rules and the projection octpt_set_projection's, an aperture with another mode than
 * PINHOLE UNSUPPORTED as there; x >= width, y >= height or an unknown flag: INVALID_ARG.  Every check comes before
 * the first write: a failed call writes nothing.  Host-only, no context. */
#define OCTPT_PROJECTION_RAYS_CENTRE 0x1u
octpt_status octpt_projection_rays(const octpt_camera *camera, const octpt_projection *projection, uint32_t width,
                                   uint32_t height, uint32_t seed, const uint32_t *xys, uint32_t n, uint32_t flags,
                                   float *rays, uint32_t *rng_state);
/* The first ray under a ray source, for n chosen samples: `rays` is a host copy of the list
 * (octpt_ray_source's layout for this width, height and rays_per_pixel), xys[3 * i] = (x, y, sample), and
 * out_rays[6 * i] = the ray a render with this seed traces for that sample -- the record as given, or, where it is
 * invalid, the central ray (eye, direction) of `fallback` -- bit for bit (one text, csrc/octpt_lens.h's ray_list_ray).
 * rng_state (nullable): rng_state[i] = the path's RNG state after the ray, octpt_projection_rays' for the same
 * (x, y, sample, seed).  `fallback` follows octpt_lens_rays' rules; a zero width, height or rays_per_pixel, more than
 * 2^28 rays, x >= width or y >= height: INVALID_ARG.  Every check comes before the first write.  Host-only, no
 * context. */
octpt_status octpt_ray_source_rays(const octpt_camera *fallback, const float *rays, uint32_t width, uint32_t height,
                                   uint32_t rays_per_pixel, uint32_t seed, const uint32_t *xys, uint32_t n,
                                   float *out_rays, uint32_t *rng_state);

/* First-hit guide buffers (AOVs) of the preview's camera ray (C24): one un-jittered ray per pixel, continued
 * through material-0 and alpha-0 hits exactly as RendererMode::Preview continues it (preview_render,
 * path_tracer.rs:137-158; next_intersection_preview :447-455); the buffers describe the hit the preview
 * shades.  Any pointer may be NULL = not wanted.  Layout as octpt_render's accum: width * height pixels in
 * image order, or the shard's compact tiles with OCTPT_RENDER_SHARD_COMPACT. */
typedef struct octpt_aov_buffers {
    float *albedo;      /* 4 floats / pixel: the hit's texture colour (linear rgb, alpha); miss 0,0,0,0 */
    float *normal;      /* 4 floats / pixel: world normal of the hit, w = 0; miss 0 */
    float *depth;       /* 1 float / pixel: world distance eye -> first visible hit along the ray; miss +inf */
    uint32_t *prim;     /* octpt_intersect's encoding (block id / 0x40000000 | quad in block scenes); miss 0xFFFFFFFF */
    uint32_t *material; /* material index of the hit (never 0, the outer medium); miss 0 */
} octpt_aov_buffers;
/* Host arrays.  Of the render parameters only width, height, shard_index, shard_count and
 * OCTPT_RENDER_SHARD_COMPACT are honoured (a set tile order is followed); spp, depth, seed and the other
 * flags are ignored.  octpt_stats counts the pass as a preview does (paths, segments, esvo_steps).  On a
 * multi-device context it runs on devices[0].  All five pointers NULL: OK, nothing is launched. */
octpt_status octpt_render_aov(octpt_ctx *ctx, const octpt_render_params *p, const octpt_aov_buffers *host);
/* The same into device buffers, enqueued on `hip_stream` (NULL = default stream); returns once enqueued. */
octpt_status octpt_render_aov_device(octpt_ctx *ctx, const octpt_render_params *p, const octpt_aov_buffers *dev,
                                     void *hip_stream);

/* Edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika & Lensch 2010) for low-spp previews (C25):
 * `iterations` passes of a 5x5 B3-spline kernel, pass i with tap spacing 2^i and colour sigma
 * sigma_color * 2^-i, each tap weighted by its colour, normal and relative depth distance to the centre.
 * Guides: normal and depth of octpt_render_aov (full frame), and albedo with OCTPT_DENOISE_DEMODULATE -- the
 * filter then runs on color.rgb / max(albedo.rgb, 1e-3) and multiplies the albedo back, which keeps texture
 * detail.  Pixels with depth +inf (misses) are copied through and never contribute; alpha is copied. */
#define OCTPT_DENOISE_DEMODULATE 0x1u
typedef struct octpt_denoise_params {
    uint32_t width, height;
    uint32_t iterations; /* 1..5 */
    float sigma_color, sigma_normal, sigma_depth; /* > 0, finite */
    uint32_t flags;      /* OCTPT_DENOISE_DEMODULATE */
} octpt_denoise_params;
/* d_color, d_out: width * height * 4 floats on the device (d_out may alias d_color); d_guides: device
 * pointers.  One launch per iteration on `hip_stream` between two frames the context owns, no host
 * synchronisation; returns once enqueued.  The two frames are shared by the context's denoise calls: calls
 * on different streams must be ordered by the caller.  On a multi-device context it runs on devices[0]. */
octpt_status octpt_denoise_device(octpt_ctx *ctx, const octpt_denoise_params *p, const float *d_color,
                                  const octpt_aov_buffers *d_guides, float *d_out, void *hip_stream);
/* The same over host arrays (out may alias color). */
octpt_status octpt_denoise(octpt_ctx *ctx, const octpt_denoise_params *p, const float *color,
                           const octpt_aov_buffers *guides, float *out);

/* --- temporal reprojection of the preview history across camera moves ---------- */
/* The step between "render" and "filter" of an interactive frame: the previous call's accumulated colour is
 * carried to where its surfaces are in the current frame and blended with the new low-spp colour under a
 * per-pixel history length.  For a pixel with finite depth, the point it sees (C24's camera ray at its depth) is
 * projected through the previous camera to (fx, fy) and the depth zp the previous frame would have stored; the
 * four bilinear taps around (fx, fy) count when they lie in the image, had a hit and a history (length > 0),
 * |depth - zp| <= depth_tolerance * zp, normal . normal >= normal_threshold and, with OCTPT_TEMPORAL_MATCH_PRIM,
 * the same prim.  With counted weight >= 2^-10: h = their weighted mean, N = min(min length + 1, max_history),
 * out.rgb = h + (color - h) / N, out_length = N.  Without: out = color, out_length = 1 (a disocclusion).  A miss
 * (depth not finite): out = color, out_length = 0.  Alpha is copied. */
#define OCTPT_TEMPORAL_MATCH_PRIM 0x1u
typedef struct octpt_temporal_params {
    uint32_t width, height;
    octpt_camera camera;      /* the camera the current colour and guides were rendered with */
    octpt_camera prev_camera; /* the history's; orthonormal: |dir.dir - 1|, |up.up - 1|, |dir.up| <= 1e-4 */
    uint32_t max_history;     /* 1..65535: the blend is the running mean up to it, exponential from there on */
    float depth_tolerance;    /* > 0, finite: relative */
    float normal_threshold;   /* in [-1, 1] */
    uint32_t flags;           /* OCTPT_TEMPORAL_MATCH_PRIM */
} octpt_temporal_params;
/* The previous call's output (color, length) with the guides it was made with.  width * height pixels each. */
typedef struct octpt_temporal_history {
    const float *color;     /* 4 floats / pixel */
    const float *normal;    /* 4 floats / pixel */
    const float *depth;
    const uint32_t *prim;   /* required with OCTPT_TEMPORAL_MATCH_PRIM */
    const uint32_t *length;
} octpt_temporal_history;
/* Device buffers, full frames only.  d_guides: normal and depth required, prim with OCTPT_TEMPORAL_MATCH_PRIM.
 * d_prev == NULL is the first frame: out = color, length 1 on hits and 0 on misses.  d_out may alias d_color;
 * d_out must not be d_prev->color nor d_out_length d_prev->length (INVALID_ARG).  One launch on `hip_stream`, no
 * host synchronisation, no memory of the context's; returns once enqueued.  On a multi-device context it runs
 * on devices[0]. */
octpt_status octpt_temporal_device(octpt_ctx *ctx, const octpt_temporal_params *p, const float *d_color,
                                   const octpt_aov_buffers *d_guides, const octpt_temporal_history *d_prev,
                                   float *d_out, uint32_t *d_out_length, void *hip_stream);
/* The same over host arrays (out may alias color). */
octpt_status octpt_temporal(octpt_ctx *ctx, const octpt_temporal_params *p, const float *color,
                            const octpt_aov_buffers *guides, const octpt_temporal_history *prev, float *out,
                            uint32_t *out_length);
/* The mapping alone: prev_xy[2 * (y * width + x)] = (fx, fy), where pixel (x, y) of `camera`'s frame at depth[..]
 * lay in prev_camera's frame (pixel centre x <-> fx = x, not clipped to the image), and prev_depth[..] = zp.  A
 * pixel whose depth is not finite, or whose point is not in front of prev_camera, gets (NaN, NaN) and +inf.  The
 * same f32 expressions in the same order as the kernel, bit for bit, as octpt_camera_rays is to the preview's
 * ray: "where was this pixel last frame".  Both cameras follow octpt_set_camera's rules; prev_camera must be
 * orthonormal as above.  Host-only, no context. */
octpt_status octpt_reproject_coords(const octpt_camera *camera, const octpt_camera *prev_camera, uint32_t width,
                                    uint32_t height, const float *depth, float *prev_xy, float *prev_depth);
/* The same for the frames of a context: UNSUPPORTED, nothing written, while the context's projection is not PINHOLE
 * (C40: the mapping is the pinhole camera's; the entry above knows no context and maps pinhole frames whatever a
 * context renders).  The cameras are the arguments', not the context's. */
octpt_status octpt_reproject_coords_ctx(octpt_ctx *ctx, const octpt_camera *camera, const octpt_camera *prev_camera,
                                        uint32_t width, uint32_t height, const float *depth, float *prev_xy,
                                        float *prev_depth);

/* --- luminance moments, variance and the variance-guided filter (SVGF, Schied et al. 2017) ---
 * The a-trous filter above stops at colour edges under one global sigma_color.  With temporal accumulation in
 * front of it the right control is per pixel: a pixel with a long history needs almost no filtering, a pixel
 * disoccluded this frame needs all of it.  These three passes carry the first and second moments of the working
 * signal's luminance l = (0.2126 r + 0.7152 g) + 0.0722 b through the reprojection, turn them into a variance,
 * and filter with a luminance weight scaled by the local standard deviation.
 * A frame: octpt_render_device (low spp) -> octpt_render_aov_device -> octpt_temporal_moments_device (history in,
 * new history out) -> octpt_variance_device -> octpt_denoise_variance_device -> tone map.  The history that the
 * next frame reads is the temporal pass's output -- the *unfiltered* colour and moments with this frame's guides --
 * never the filter's: filtered history would be filtered again every frame.  Pass the same demodulate choice to
 * the temporal and the filter pass, so that the variance is that of the signal the filter works on. */

/* C27.  octpt_temporal with the moments alongside: d_out and d_out_length are octpt_temporal_device's, bit for
 * bit.  Moments planes hold 2 floats / pixel (m1, m2).  The pixel's own moments are mu = (l(s), l(s)^2) of
 * s = color.rgb, or color.rgb / max(albedo.rgb, 1e-3) with OCTPT_TEMPORAL_DEMODULATE (d_guides->albedo then
 * required).  With history: hm = the weighted mean of the counted taps' moments, out_m = hm + (mu - hm) / N.
 * Without: out_m = mu.  A miss: (0, 0).  d_prev and d_prev_moments are both NULL (the first frame) or both set;
 * d_out_moments must not be d_prev_moments, besides octpt_temporal_device's alias rules (INVALID_ARG).  One launch
 * on `hip_stream`, no host synchronisation, no memory of the context's.  octpt_temporal itself refuses the flag. */
#define OCTPT_TEMPORAL_DEMODULATE 0x2u
octpt_status octpt_temporal_moments_device(octpt_ctx *ctx, const octpt_temporal_params *p, const float *d_color,
                                           const octpt_aov_buffers *d_guides, const octpt_temporal_history *d_prev,
                                           const float *d_prev_moments, float *d_out, uint32_t *d_out_length,
                                           float *d_out_moments, void *hip_stream);
/* The same over host arrays (out may alias color). */
octpt_status octpt_temporal_moments(octpt_ctx *ctx, const octpt_temporal_params *p, const float *color,
                                    const octpt_aov_buffers *guides, const octpt_temporal_history *prev,
                                    const float *prev_moments, float *out, uint32_t *out_length, float *out_moments);

/* C28.  The variance of the luminance from C27's moments and lengths and the frame's normal and depth guides, one
 * float / pixel, never negative.  A miss (depth not finite, or length 0): 0.  A pixel with length N >= min_history:
 * max(m2 - m1^2, 0), the temporal estimate.  A shorter one: the same of the 7 x 7 mean of the moments around it,
 * each tap weighted by the filter's normal and depth weights with their exponential correctly rounded (taps outside
 * the image, misses and length-0 taps skipped), times min_history / N: a spatial estimate, inflated while the history is short. */
typedef struct octpt_variance_params {
    uint32_t width, height;
    uint32_t min_history;            /* 1..65535; SVGF uses 4 */
    float sigma_normal, sigma_depth; /* > 0, finite: octpt_denoise's */
} octpt_variance_params;
/* Device buffers, full frames only; d_guides: normal and depth.  d_out is distinct from the inputs.  One launch on
 * `hip_stream`, no host synchronisation, no memory of the context's; on a multi-device context it runs on
 * devices[0]. */
octpt_status octpt_variance_device(octpt_ctx *ctx, const octpt_variance_params *p, const float *d_moments,
                                   const uint32_t *d_length, const octpt_aov_buffers *d_guides, float *d_out,
                                   void *hip_stream);
/* The same over host arrays. */
octpt_status octpt_variance(octpt_ctx *ctx, const octpt_variance_params *p, const float *moments,
                            const uint32_t *length, const octpt_aov_buffers *guides, float *out);

/* C29.  octpt_denoise with the colour weight replaced by a luminance weight under the local standard deviation.
 * Working signal, miss pixels, alpha and the re-modulation after the last pass are octpt_denoise's.  Pass i, pixel
 * p: vbar = the 3 x 3 (1/4, 1/2, 1/4)^2 mean of the variance around p at spacing 1; k = 1 / (sigma_luminance *
 * sqrtf(vbar) + luminance_floor); taps as octpt_denoise's with wc replaced by wl = expf(-(|l(s_p) - l(s_q)| * k));
 * out = sum(w s_q) / sum(w), variance out = sum(w^2 v_q) / sum(w)^2.  sigma_luminance is not scaled per pass: the
 * variance shrinks instead.  The variance is that of the working signal and is not re-modulated; it must be >= 0;
 * miss pixels keep theirs. */
typedef struct octpt_denoise_variance_params {
    uint32_t width, height;
    uint32_t iterations;   /* 1..5 */
    float sigma_luminance; /* > 0, finite; SVGF uses 4 */
    float luminance_floor; /* > 0, finite: the weight's scale where the variance is 0 */
    float sigma_normal, sigma_depth; /* > 0, finite */
    uint32_t flags;        /* OCTPT_DENOISE_DEMODULATE */
} octpt_denoise_variance_params;
/* d_color, d_out: 4 floats / pixel (d_out may alias d_color); d_variance: 1 float / pixel; d_out_variance: NULL or
 * 1 float / pixel, the filtered variance (may alias d_variance).  One prep launch and one launch per iteration
 * on `hip_stream`, no host synchronisation.  The working frames are octpt_denoise_device's two, owned by the
 * context: its denoise and denoise_variance calls on different streams must be ordered by the caller.  On a
 * multi-device context it runs on devices[0]. */
octpt_status octpt_denoise_variance_device(octpt_ctx *ctx, const octpt_denoise_variance_params *p, const float *d_color,
                                           const float *d_variance, const octpt_aov_buffers *d_guides, float *d_out,
                                           float *d_out_variance, void *hip_stream);
/* The same over host arrays (out may alias color, out_variance may alias variance or be NULL). */
octpt_status octpt_denoise_variance(octpt_ctx *ctx, const octpt_denoise_variance_params *p, const float *color,
                                    const float *variance, const octpt_aov_buffers *guides, float *out,
                                    float *out_variance);

/* --- adaptive sampling: tile-list renders, sample moments and the per-tile error ---
 * The final-quality counterpart of the chain above: instead of one spp_count for every pixel, render until the noise
 * of each 8x8 tile is below a threshold.  Converged tiles (sky, flat directly lit surfaces) stop after a few samples
 * and the budget goes to the tiles that need it (penumbrae, glossy surfaces, emitters).  Three layers: a render entry
 * that takes a list of tiles (C30), the luminance moments of the *samples* kept by resolve (C31; C27's are moments of
 * frames), and a per-tile error with the driver that loops render -> estimate -> drop converged tiles (C32).  Tiles
 * are the wavefront's own: frame tile t = ty * ceil(width / 8) + tx. */

/* C30.  octpt_render_device's spp_count more samples into the listed tiles only.  tiles: a host array of n_tiles
 * distinct frame tile indices in any order, copied by the call (it may be freed on return); NULL = every tile, in
 * frame order (n_tiles is then ignored).  d_accum and d_seg_count (nullable) are full frames as octpt_render_device
 * takes them; d_moments (nullable) holds 2 floats / pixel, full frame, image order (C31).  For every pixel of a
 * listed tile accum, seg_count and moments are afterwards what a full-frame call with the same parameters leaves
 * there -- accum and seg_count bit for bit octpt_render_device's, since the per-pixel RNG streams are keyed by
 * (pixel, sample) -- and every pixel of an unlisted tile keeps all three untouched, bit for bit.  octpt_stats counts
 * the listed tiles' paths only.  The list is the deal of a one-shard render, so seed, extend, shade, drain and resolve
 * run as in any render; branch_count > 1 follows octpt_render_params' pass-boundary rules.  The wavefront state is
 * grow-only: calls with shrinking lists do not reallocate it (octpt_stats.wave_allocs).
 * INVALID_ARG, checked on the host before anything is launched (the buffers stay untouched): a tile index >= the
 * frame's tile count or a duplicate; shard_count != 1, OCTPT_RENDER_SHARD_COMPACT, or a tile order set on the context.
 * UNSUPPORTED: OCTPT_RENDER_MEGAKERNEL, OCTPT_RENDER_PREVIEW, a multi-device context.  tiles != NULL with n_tiles == 0:
 * OK, nothing is launched.  Like octpt_render_device the call returns once the last kernel is enqueued on `hip_stream`. */
octpt_status octpt_render_tiles_device(octpt_ctx *ctx, const octpt_render_params *p, const uint32_t *tiles,
                                       uint32_t n_tiles, float *d_accum, float *d_moments, uint32_t *d_seg_count,
                                       void *hip_stream);

/* C31.  The moments octpt_render_tiles_device keeps with d_moments set: per pixel the running means (m1, m2) of l and
 * l * l over the samples, l = (0.2126 r + 0.7152 g) + 0.0722 b (C27's expression) of each sample's colour, updated in
 * sample order with the colour's own running-mean formula and weights: m = (m * (float)spp + v * (float)bc) *
 * (1.0f / (float)(bc + spp)), spp = the samples held, bc = 1 -- or, with a branch schedule, the pass's branch count,
 * the sample then being the pass's folded colour.  A render with spp_start == 0 starts them from (0, 0) as it starts
 * accum from black; accum is bit for bit the same with and without d_moments. */

/* C32.  The error of every 8x8 tile from C31's moments, one float per tile in frame tile order: the standard error of
 * the tile's mean luminance relative to that luminance.  Tile t covers P pixels inside the image (1..64) and holds
 * n = tile_spp[t] samples per pixel.  n < 2: +inf.  Else, per pixel v = max(m2 - m1 * m1, 0) (a NaN stays one), Sv =
 * the sum of v and Sl = the sum of m1 over the tile's pixels inside the image (f32, summation order unspecified), and
 * error = sqrtf((Sv / P) / (float)(n - 1)) / (Sl / P + luminance_floor); a result that is not finite is +inf. */
typedef struct octpt_tile_error_params {
    uint32_t width, height;
    float luminance_floor; /* > 0, finite */
} octpt_tile_error_params;
/* Device buffers: d_moments width * height * 2 floats, d_tile_spp and d_error one entry per tile.  One launch on
 * `hip_stream`, no host synchronisation, no memory of the context's; on a multi-device context it runs on devices[0]. */
octpt_status octpt_tile_error_device(octpt_ctx *ctx, const octpt_tile_error_params *p, const float *d_moments,
                                     const uint32_t *d_tile_spp, float *d_error, void *hip_stream);
/* The same over host arrays. */
octpt_status octpt_tile_error(octpt_ctx *ctx, const octpt_tile_error_params *p, const float *moments,
                              const uint32_t *tile_spp, float *error);

/* The adaptive driver: a fresh render (p->spp_start must be 0) of at most max_spp = p->spp_count samples per pixel
 * (>= min_spp).  accum and moments are outputs, initialised by the call to (0, 0, 0, 1) and (0, 0).  The loop, which
 * is the definition of the result:
 *   1. active = every tile, n = 0;
 *   2. each round k = min(n == 0 ? min_spp : step_spp, max_spp - n);
 *   3. octpt_render_tiles_device(active, spp_start = n, spp_count = k);
 *   4. n += k, tile_spp[t] = n for the active tiles t;
 *   5. the error (above) of the active tiles;
 *   6. active = the tiles of active with error > threshold, in frame order;
 *   7. stop when active is empty or n == max_spp.
 * All active tiles share one n, so a round is one render call and no per-tile sample key enters the kernels; the host
 * reads one float per tile back per round (the wavefront loop is host-steered already).  result (nullable): rounds
 * run, tile_samples = the sum of tile_spp, converged_tiles = tiles whose last error was <= threshold, total_tiles.
 * UNSUPPORTED: branch_count > 1 (its pass boundaries fix the round sizes).  octpt_render_tiles_device's refusals
 * apply; min_spp < 2, step_spp < 1, a threshold or luminance_floor that is not positive and finite: INVALID_ARG. */
typedef struct octpt_adaptive_params {
    uint32_t min_spp;      /* >= 2: the first round's samples */
    uint32_t step_spp;     /* >= 1: every later round's */
    float threshold;       /* > 0, finite: a tile stops once its error is <= it */
    float luminance_floor; /* > 0, finite */
} octpt_adaptive_params;
typedef struct octpt_adaptive_result {
    uint32_t rounds;
    uint64_t tile_samples;
    uint32_t converged_tiles, total_tiles;
} octpt_adaptive_result;
/* d_accum, d_moments: device, full frames; d_seg_count: nullable, device, += ray segments; tile_spp: host, out, one
 * entry per tile.  The rounds run on `hip_stream`, which the call drains once per round. */
octpt_status octpt_render_adaptive_device(octpt_ctx *ctx, const octpt_render_params *p, const octpt_adaptive_params *a,
                                          float *d_accum, float *d_moments, uint32_t *d_seg_count, uint32_t *tile_spp,
                                          octpt_adaptive_result *result, void *hip_stream);
/* The same into host arrays; moments, tile_spp, out_rgba8 (the tone-mapped final accum) and result are nullable. */
octpt_status octpt_render_adaptive(octpt_ctx *ctx, const octpt_render_params *p, const octpt_adaptive_params *a,
                                   float *accum, float *moments, uint32_t *tile_spp, uint8_t *out_rgba8,
                                   octpt_adaptive_result *result);

/* --- final-quality adaptive frames: sample clamp, seam rule, sample variance, one-pass filter ---
 * What turns the tile loop above into a finished picture: a per-sample luminance clamp, so that one firefly does not
 * hold its tile above the threshold up to the cap (C33); the error of a tile raised to a share of its neighbours', so
 * that adjacent tiles stop at noise levels within a known factor of each other (C34); the variance of each pixel's
 * mean from C31's sample moments (C35), which is what C29's filter needs and a final frame, with no history, cannot
 * get from C27/C28; and one entry that runs render -> guides -> variance -> filter (C36). */

/* C33.  A clamp on every sample's luminance, applied by resolve before the running means: c = the sample's colour
 * (the pass's folded colour under a branch schedule), l = (0.2126 c.r + 0.7152 c.g) + 0.0722 c.b; if l > max_luminance:
 * k = max_luminance / l, c = (c.r * k, c.g * k, c.b * k).  A NaN l compares false: the sample passes unchanged.  C31's
 * moments are those of the clamped colour (l recomputed from it); segment counts are untouched.
 * max_luminance 0 or +inf: off, the state of a new context -- every render is then bit for bit what it was, through
 * the same kernels.  Any other positive finite value: on.  NaN or a negative value: INVALID_ARG, the setting stays.
 * It holds for every later wavefront render of the context (octpt_render, _device, _async, octpt_render_tiles_device,
 * the adaptive drivers and octpt_render_final), read when the render call is made; the call joins a frame in flight
 * first.  OCTPT_RENDER_PREVIEW ignores it (it takes no samples); OCTPT_RENDER_MEGAKERNEL with a clamp on is
 * UNSUPPORTED (it accumulates inside the kernel).  On a multi-device context the value is set on every entry. */
octpt_status octpt_set_sample_clamp(octpt_ctx *ctx, float max_luminance);

/* C34.  The seam rule: out[t] = max(error[t], w * M), w = neighbour_weight in [0, 1] (anything else, NaN included:
 * INVALID_ARG), M = the maximum of error[u] over the up to eight tiles u adjacent to t in the tile grid (tiles outside
 * the grid do not count).  w == 0: out[t] = error[t] exactly, no multiply is made (+inf * 0 never appears).  error and
 * out hold one float per tile in frame tile order, as C32's planes; the inputs are C32's errors, never NaN.  A tile
 * whose spread error is <= threshold has its own error <= threshold and every neighbour's <= threshold / w: adjacent
 * tiles stop at noise levels within a factor 1 / w of each other.  The spread never lowers an error.
 * d_out == d_error: INVALID_ARG.  One launch on `hip_stream`, one thread per tile, no host synchronisation, no memory
 * of the context's; on a multi-device context it runs on devices[0]. */
octpt_status octpt_tile_error_spread_device(octpt_ctx *ctx, uint32_t width, uint32_t height, float neighbour_weight,
                                            const float *d_error, float *d_out, void *hip_stream);
/* The same over host arrays. */
octpt_status octpt_tile_error_spread(octpt_ctx *ctx, uint32_t width, uint32_t height, float neighbour_weight,
                                     const float *error, float *out);

/* The adaptive driver with the seam rule: the loop of octpt_render_adaptive_device with one change -- after step 5
 * the round's error plane (every tile's: inactive tiles keep their moments and tile_spp, hence their last error) goes
 * through C34, and steps 6 and 7 and converged_tiles use the spread plane, which is the one the host reads back.
 * neighbour_weight == 0 is octpt_render_adaptive_device, bit for bit; the plain entries are these with weight 0.
 * A non-zero reserved word or a neighbour_weight outside [0, 1]: INVALID_ARG; the plain entries' refusals apply. */
typedef struct octpt_adaptive_params_ex {
    uint32_t min_spp, step_spp;
    float threshold, luminance_floor; /* octpt_adaptive_params' four */
    float neighbour_weight;           /* [0, 1]; 0 = C32's loop */
    uint32_t reserved[3];             /* 0 */
} octpt_adaptive_params_ex;
octpt_status octpt_render_adaptive_ex_device(octpt_ctx *ctx, const octpt_render_params *p,
                                             const octpt_adaptive_params_ex *a, float *d_accum, float *d_moments,
                                             uint32_t *d_seg_count, uint32_t *tile_spp, octpt_adaptive_result *result,
                                             void *hip_stream);
/* The same into host arrays; moments, tile_spp, out_rgba8 and result are nullable. */
octpt_status octpt_render_adaptive_ex(octpt_ctx *ctx, const octpt_render_params *p, const octpt_adaptive_params_ex *a,
                                      float *accum, float *moments, uint32_t *tile_spp, uint8_t *out_rgba8,
                                      octpt_adaptive_result *result);

/* C35.  The variance of each pixel's mean luminance from C31's sample moments, one float per pixel, never negative:
 * what C29 filters under.  Pixel p in tile t with n = tile_spp[t]: depth not finite (a miss) or n < 2: 0.  Else
 * d = m2 - m1 * m1, v = d > 0 ? d : 0 (a NaN becomes 0), v = v / (float)(n - 1).  With OCTPT_DENOISE_DEMODULATE:
 * a = max(albedo.rgb, 1e-3) componentwise, la = luminance(a), v = v / (la * la) -- the variance moved into the
 * demodulated signal C29 works on; exact for a grey albedo (luminance(c / a) = luminance(c) / la there), an
 * approximation otherwise. */
typedef struct octpt_sample_variance_params {
    uint32_t width, height;
    uint32_t flags; /* OCTPT_DENOISE_DEMODULATE */
} octpt_sample_variance_params;
/* Device buffers: d_moments width * height * 2 floats, d_tile_spp one entry per tile, d_guides->depth required and
 * ->albedo with the flag, d_out one float per pixel, distinct from the inputs (INVALID_ARG).  One launch on
 * `hip_stream`, one thread per pixel, no host synchronisation, no memory of the context's; on a multi-device context
 * it runs on devices[0]. */
octpt_status octpt_sample_variance_device(octpt_ctx *ctx, const octpt_sample_variance_params *p, const float *d_moments,
                                          const uint32_t *d_tile_spp, const octpt_aov_buffers *d_guides, float *d_out,
                                          void *hip_stream);
/* The same over host arrays. */
octpt_status octpt_sample_variance(octpt_ctx *ctx, const octpt_sample_variance_params *p, const float *moments,
                                   const uint32_t *tile_spp, const octpt_aov_buffers *guides, float *out);

/* C36.  The finished frame.  The result is, bit for bit, this composition of public entries on `hip_stream`:
 *   1. octpt_render_adaptive_ex_device(p, &f->adaptive) -> d_accum, d_moments, tile_spp, result;
 *   2. octpt_render_aov_device for normal and depth, and albedo with OCTPT_DENOISE_DEMODULATE in f->filter.flags, into
 *      guide planes the context owns (grow-only, like its one variance plane);
 *   3. octpt_sample_variance_device with that demodulate bit and the driver's final tile_spp;
 *   4. octpt_denoise_variance_device(&f->filter, d_accum, variance, guides) -> d_out, d_out_variance (nullable).
 * d_accum and d_moments keep the unfiltered result.  d_out must not alias d_accum (INVALID_ARG).  The driver's and the
 * filter's refusals apply, and filter.width / height must equal the render's (INVALID_ARG); all are checked before any
 * buffer is touched.  The clamp set on the context (C33) applies.  The context's planes are shared by its
 * octpt_render_final calls: calls on different streams must be ordered by the caller. */
typedef struct octpt_final_params {
    octpt_adaptive_params_ex adaptive;
    octpt_denoise_variance_params filter; /* width / height must equal the render's */
} octpt_final_params;
octpt_status octpt_render_final_device(octpt_ctx *ctx, const octpt_render_params *p, const octpt_final_params *f,
                                       float *d_accum, float *d_moments, float *d_out, float *d_out_variance,
                                       uint32_t *tile_spp, octpt_adaptive_result *result, void *hip_stream);
/* The same into host arrays: out is required; accum, moments, out_variance, tile_spp, out_rgba8 (the tone map of out)
 * and result are nullable. */
octpt_status octpt_render_final(octpt_ctx *ctx, const octpt_render_params *p, const octpt_final_params *f, float *accum,
                                float *moments, float *out, float *out_variance, uint32_t *tile_spp,
                                uint8_t *out_rgba8, octpt_adaptive_result *result);

/* --- host octree builder (replaces the Rust-side build for primitive scenes) ---
 * Voxelises spheres/cuboids into depth-`depth` leaf cells, Morton-sorts
 * them (new_octree.rs:752-835 code order) and emits octants in pre-order. */
typedef struct octpt_octree_view {
    const octpt_octant *octants;
    uint32_t octant_count, root, depth;
    const uint32_t *leaf_first, *leaf_count;
    uint32_t leaf_table_size;
    const uint32_t *leaf_prims;
    uint32_t leaf_prim_count;
} octpt_octree_view;
octpt_status octpt_build_octree(const octpt_sphere *spheres, uint32_t sphere_count, const octpt_cuboid *cuboids,
                                uint32_t cuboid_count, uint32_t depth, octpt_octree **out);
/* The same builder on the context's device (the reference's flattener
 * octree_to_gpu_data, gpu_octree.rs:28-76, is todo!()): count / scan / emit (cell, primitive) pairs,
 * stable radix sort by Morton code, leaf tables, pre-order octant ids by a scan of the octants each
 * leaf opens.  The result equals octpt_build_octree's array for array.  Inputs are host arrays
 * (borrowed), the result is a host octree as above. */
octpt_status octpt_build_octree_device(octpt_ctx *ctx, const octpt_sphere *spheres, uint32_t sphere_count,
                                       const octpt_cuboid *cuboids, uint32_t cuboid_count, uint32_t depth,
                                       octpt_octree **out);
/* Builder options (the _ex forms; the plain forms pass 0).
 * OCTPT_BUILD_COMPACT: Octant::is_compactable (new_octree.rs:227-233) applied bottom-up at every
 * level, as RegionOctreeBuilder::recursive_build does (:679-690): an octant whose eight children are
 * leaves holding the same primitive list becomes one leaf of its parent with child 0's payload (the
 * other seven leaf table entries stay, unreferenced).  The root is never merged away (a Lod root
 * stays one octant of eight equal leaves, :534-545).  Host and device builds stay equal array for
 * array. */
#define OCTPT_BUILD_COMPACT 0x1u
octpt_status octpt_build_octree_ex(const octpt_sphere *spheres, uint32_t sphere_count, const octpt_cuboid *cuboids,
                                   uint32_t cuboid_count, uint32_t depth, uint32_t flags, octpt_octree **out);
octpt_status octpt_build_octree_device_ex(octpt_ctx *ctx, const octpt_sphere *spheres, uint32_t sphere_count,
                                          const octpt_cuboid *cuboids, uint32_t cuboid_count, uint32_t depth,
                                          uint32_t flags, octpt_octree **out);
/* Block-value octree builder (C23): one block per voxel cell, cells[4k .. 4k+3] = (x, y, z, block id),
 * x, y, z < 2^depth.  Morton-sorted (new_octree.rs:752-835 order) and emitted in pre-order like
 * octpt_build_octree; the leaf payloads are the block ids (the view's leaf tables are empty).
 * OCTPT_BUILD_COMPACT merges eight sibling leaves holding the same block value into one leaf of their
 * parent, bottom-up at every level: Octant::is_compactable's value equality (new_octree.rs:227-233) as
 * SectionOctantBuilder / RegionOctreeBuilder apply it (:675-690, 582-587); the root is never merged
 * away.  Two cells at one position, or a block id >= 2^27, are INVALID_ARG. */
octpt_status octpt_build_block_octree(const uint32_t *cells, uint32_t cell_count, uint32_t depth, uint32_t flags,
                                      octpt_octree **out);
/* The block-value builder on the context's device: one thread per cell emits (Morton code,
 * block), a radix sort on the code, then the octants, the merge passes of OCTPT_BUILD_COMPACT and the
 * pre-order numbering as octpt_build_octree_device makes them.  The result equals octpt_build_block_octree's
 * array for array, and the same cells are INVALID_ARG.  At most 2^31 cells (else OOM).
 * OCTPT_BUILD_CELLS_ON_DEVICE (these two entries only; octpt_build_block_octree refuses it): `cells` is a
 * device pointer on the context's device and is read where it is, with no upload.  The cells must be complete
 * before the call: the library reads them on a stream of its own and does not synchronise with the stream
 * that wrote them.  UNSUPPORTED on a multi-device context (the cells live on one device). */
#define OCTPT_BUILD_CELLS_ON_DEVICE 0x2u
octpt_status octpt_build_block_octree_device(octpt_ctx *ctx, const uint32_t *cells, uint32_t cell_count,
                                             uint32_t depth, uint32_t flags, octpt_octree **out);
/* set_scene for a block-value scene (C23) with the octree built on the device and kept there: the block
 * counterpart of octpt_scene_build_device.  `scene` carries the block table (blocks must be set), materials,
 * textures, models and the build depth, and no octree and no primitives; the cells are voxelised by the
 * device block builder and its octants packed into the device node slots in place.  The resulting device
 * scene is the one octpt_scene_upload makes from octpt_build_block_octree's octree.  Besides the builder's
 * errors, a cell whose block id is >= block_count is INVALID_ARG.  flags: OCTPT_BUILD_COMPACT,
 * OCTPT_BUILD_CELLS_ON_DEVICE (as above).  On a multi-device context every entry builds its own replica. */
octpt_status octpt_scene_build_blocks_device(octpt_ctx *ctx, const octpt_scene_desc *scene, const uint32_t *cells,
                                             uint32_t cell_count, uint32_t flags);
/* Block-value worlds as 16^3 palette sections: the form the reference ingests a world in
 * (section_to_compacted_octree / RegionOctreeBuilder, new_octree.rs:446-750).  A section is 4096 palette
 * indices in the order of section_index_to_block_coordinates (new_octree.rs:838-850) plus a slice of a palette
 * of block values.  A palette value of 0 is air (the reference's NonZeroU32) and produces no cell; any other
 * value v is block id v, the leaf payload, exactly as in the cell form -- so block 0 of the block table cannot
 * be placed through sections.  Sections may share palette slices and index blocks. */
#define OCTPT_SECTION_UNIFORM 0xFFFFFFFFu
typedef struct octpt_section {       /* 24 bytes */
    uint32_t x, y, z;                /* section coordinates: cells [16x, 16x+16) etc.; 16*(x+1) <= 2^depth */
    uint32_t palette_first, palette_count;  /* block values palette[palette_first .. +palette_count), 1..4096 entries */
    uint32_t index_first;            /* indices[index_first .. +4096), a multiple of 4096; entry i = y<<8 | z<<4 | x
                                        (section_index_to_block_coordinates, new_octree.rs:838-850) is a palette index.
                                        OCTPT_SECTION_UNIFORM: no indices, every cell is palette[palette_first]
                                        (palette_count must be 1): the reference's one-entry-palette case, :716-732 */
} octpt_section;
typedef struct octpt_section_world {
    const octpt_section *sections; uint32_t section_count;
    const uint32_t *palette;       uint32_t palette_size;
    const uint16_t *indices;       uint32_t index_count;   /* multiple of 4096 */
} octpt_section_world;
/* The cells of a section world, as the rows (x, y, z, block) octpt_build_block_octree takes: sections in
 * ascending Morton code of their section coordinates, each section's non-air cells in ascending local Morton
 * code -- ascending Morton order of the world.  This is the definition of what the section builds below build.
 * Host-only, no context.  *count always receives the number of cells; cells == NULL only counts; cells != NULL
 * with capacity (in rows) < *count writes nothing and is INVALID_ARG.  INVALID_ARG also: depth < 4 or > 21; a
 * section outside the world; two sections at one position; palette_first + palette_count > palette_size;
 * palette_count 0 or > 4096; index_first not a multiple of 4096 or index_first + 4096 > index_count;
 * OCTPT_SECTION_UNIFORM with palette_count != 1; an index >= palette_count; a value >= 2^27 in a section's
 * palette slice (used by an index or not).  More than 2^31 cells is OOM. */
octpt_status octpt_sections_to_cells(const octpt_section_world *world, uint32_t depth, uint32_t *cells,
                                     uint32_t capacity, uint32_t *count);
/* The block-value builder on the context's device, from sections: one block of threads per section
 * counts its non-air cells, the (section Morton code, section) pairs are sorted, and one block per sorted section
 * writes its (Morton code, block) pairs in local Morton order -- already sorted, so the octants follow with no
 * sort of the cells.  The result equals octpt_build_block_octree of octpt_sections_to_cells' cells array for array,
 * with and without OCTPT_BUILD_COMPACT, and the same worlds are INVALID_ARG / OOM.  A world whose cells are all
 * air builds the childless root.
 * OCTPT_BUILD_SECTIONS_ON_DEVICE (the two section entries only): world->sections, palette and indices are device
 * pointers on the context's device and are read where they are (the struct itself is host memory); indices may be
 * only 2-byte aligned.  They must be complete before the call, as for OCTPT_BUILD_CELLS_ON_DEVICE.  UNSUPPORTED on
 * a multi-device context.  OCTPT_BUILD_CELLS_ON_DEVICE is INVALID_ARG here, as OCTPT_BUILD_SECTIONS_ON_DEVICE is on
 * the cell entries. */
#define OCTPT_BUILD_SECTIONS_ON_DEVICE 0x4u
octpt_status octpt_build_block_octree_sections_device(octpt_ctx *ctx, const octpt_section_world *world, uint32_t depth,
                                                      uint32_t flags, octpt_octree **out);
/* The section counterpart of octpt_scene_build_blocks_device, with the same scene rules (blocks set, no octree,
 * no primitives; the build depth in scene->depth): the octree is built on the device from the sections and packed
 * into the node slots in place; the device scene is the one octpt_scene_upload makes from the host builder's octree
 * of octpt_sections_to_cells' cells.  Besides the builder's errors, a value >= block_count in a section's palette
 * slice is INVALID_ARG.  flags: OCTPT_BUILD_COMPACT, OCTPT_BUILD_SECTIONS_ON_DEVICE.  On a multi-device context
 * every entry builds its own replica. */
octpt_status octpt_scene_build_sections_device(octpt_ctx *ctx, const octpt_scene_desc *scene,
                                               const octpt_section_world *world, uint32_t flags);
/* --- the emitter grid: what next-event estimation toward emissive blocks samples from ---
 * Block-value worlds only.  An emitter is a leaf of the block octree, at any level, whose block has
 * model == OCTPT_MODEL_NONE and at least one face material with emittance > EPSILON (5e-8); a leaf of side
 * s = 2^k (a LOD or compacted leaf) is one emitter (x, y, z, s): its minimum corner and its side.  Block-model
 * leaves are listed only with OCTPT_EMITTERS_MODELS (C39, below).  The grid has cells of grid_size voxels per side
 * (a power of two, 1 .. 2^depth),
 * cells_per_axis = 2^depth / grid_size per axis, cell (cx, cy, cz) at index cx + cells_per_axis * (cy +
 * cells_per_axis * cz).  An emitter's home cell is (x, y, z) / grid_size; the list of cell c holds every emitter
 * whose home cell is within Chebyshev distance 1 of c, in ascending Morton code of (x, y, z) (x bit 0, y bit 1,
 * z bit 2 per level) -- Chunky's Grid.  CSR form: cell c's list is cell_emitters[cell_first[c] .. cell_first[c + 1]),
 * indices into emitters[], which is in ascending Morton code itself. */
typedef struct octpt_emitter {
    uint32_t x, y, z, s;
} octpt_emitter;
/* Count-then-fill, as octpt_sections_to_cells: the three counts and cells_per_axis are always received (0 on an
 * error).  With the three pointers NULL the call only counts.  Otherwise all three must be set and each capacity
 * (in elements) must hold its array -- cell_count + 1, entry_count, emitter_count -- else nothing is written and
 * the call is INVALID_ARG. */
typedef struct octpt_emitter_grid_arrays {
    uint32_t *cell_first;
    uint32_t cell_first_capacity;
    uint32_t *cell_emitters;
    uint32_t cell_emitters_capacity;
    octpt_emitter *emitters;
    uint32_t emitters_capacity;
    uint32_t cell_count, entry_count, emitter_count, cells_per_axis;
} octpt_emitter_grid_arrays;
/* The definition of the grid.  Host-only, no context.  cells are the rows (x, y, z, block) of
 * octpt_build_block_octree, whose octree (with OCTPT_BUILD_COMPACT: the compacted one) provides the leaves.
 * INVALID_ARG: what octpt_build_block_octree refuses, a block id >= block_count, a face material >=
 * material_count, grid_size 0, not a power of two or above 2^depth, count-then-fill misuse.  OOM: more than 2^24
 * emitters, more than 2^28 list entries, or more than 2^28 cells. */
octpt_status octpt_build_emitter_grid(const uint32_t *cells, uint32_t cell_count, const octpt_block *blocks,
                                      uint32_t block_count, const octpt_material *materials, uint32_t material_count,
                                      uint32_t depth, uint32_t flags, uint32_t grid_size,
                                      octpt_emitter_grid_arrays *out);
/* --- emissive block models as emitters: torches, lanterns, candles ---
 * The emissive-model table.  The emissive quads of model m are the quads of [first_quad, first_quad + quad_count)
 * whose material has emittance > EPSILON (5e-8) and whose area a = |u x v| is finite and > 0, in table order; the
 * area in plain f32 without contraction, each cross component a * b - c * d, the length sqrtf((x^2 + y^2) + z^2).
 * model m's entries are [model_first[m], model_first[m + 1]): quad_index[] the quad, cum_area[] the running f32 sum
 * of the areas within the model, in order; A_m, the model's emissive area, is its last cum_area, and a model is
 * emissive when it has an entry.  Count-then-fill as octpt_emitter_grid_arrays: the two counts are always received
 * (0 on an error); the three pointers NULL: the call only counts; else all three set with capacities (in elements)
 * of model_count + 1, entry_count, entry_count, or nothing is written and the call is INVALID_ARG. */
typedef struct octpt_emitter_model_arrays {
    uint32_t *model_first;
    uint32_t model_first_capacity;
    uint32_t *quad_index;
    uint32_t quad_index_capacity;
    float *cum_area;
    uint32_t cum_area_capacity;
    uint32_t model_count, entry_count;
} octpt_emitter_model_arrays;
/* The definition of the table.  Host-only, no context.  INVALID_ARG: a model whose quad range leaves the quad table,
 * a quad of a model with material >= material_count, count-then-fill misuse. */
octpt_status octpt_emitter_model_table(const octpt_block_model *models, uint32_t model_count, const octpt_quad *quads,
                                       uint32_t quad_count, const octpt_material *materials, uint32_t material_count,
                                       octpt_emitter_model_arrays *out);
/* Flags of emitter sampling (octpt_emitter_params.flags, octpt_build_emitter_grid_models' emitter_flags).
 * OCTPT_EMITTERS_MODELS: a leaf at any level whose block has model != OCTPT_MODEL_NONE and an emissive model is an
 * emitter too, with the record (x, y, z, 0x80000000 | model): the leaf's minimum corner, where C23 draws the model in
 * unit-voxel coordinates whatever the leaf's level.  A cube emitter keeps s = 2^k, so the top bit of the fourth word
 * tells the two kinds apart. */
#define OCTPT_EMITTERS_MODELS 0x1u
/* octpt_build_emitter_grid with the model and quad tables and the flags above: with emitter_flags 0 it equals
 * octpt_build_emitter_grid array for array (the two tables are not read).  INVALID_ARG besides: an emitter flag
 * other than OCTPT_EMITTERS_MODELS, and with it what octpt_emitter_model_table refuses, a block's model >=
 * model_count, model_count above 2^31 - 1. */
octpt_status octpt_build_emitter_grid_models(const uint32_t *cells, uint32_t cell_count, const octpt_block *blocks,
                                             uint32_t block_count, const octpt_material *materials,
                                             uint32_t material_count, const octpt_block_model *models,
                                             uint32_t model_count, const octpt_quad *quads, uint32_t quad_count,
                                             uint32_t depth, uint32_t flags, uint32_t grid_size, uint32_t emitter_flags,
                                             octpt_emitter_grid_arrays *out);
/* Emitter sampling (Scene::emitter_sampling_strategy and emmitter_intensity, scene/mod.rs:5-58).  The default is
 * NONE, with which every render is what it is without this call.  ONE_BLOCK and ALL have their values reserved and
 * are UNSUPPORTED, as is every other strategy value.  grid_size: a power of two, 1 .. 2^21, and with ONE on a
 * context that holds a scene at most 2^depth; intensity finite and >= 0; flags 0 or OCTPT_EMITTERS_MODELS (C39;
 * accepted and without meaning under NONE; under ONE a change of it rebuilds the grid, and with it a scene of more
 * than 2^31 - 1 models is INVALID_ARG); reserved words 0: else INVALID_ARG and the setting stays.  ONE on a context whose scene has primitive leaves is UNSUPPORTED.  Like
 * octpt_set_sample_clamp the call joins a frame in flight, holds for later renders and is read when a render call
 * is made.  It may come before or after the scene: with ONE and a block-value scene both known, the context's
 * device builds the grid from the octree resident there (after octpt_scene_upload, octpt_scene_build_blocks_device
 * or octpt_scene_build_sections_device alike; no host round trip), equal to octpt_build_emitter_grid's array for
 * array; a new scene or grid_size rebuilds it, NONE drops it.  A scene set while ONE holds a grid_size above its
 * 2^depth is INVALID_ARG; the grid's budgets are OOM as above.  On a multi-device context every entry builds its
 * own replica.
 * Renders: the preview and the guide buffers ignore the setting.  ONE with OCTPT_RENDER_MEGAKERNEL is UNSUPPORTED,
 * as is ONE on a scene of primitive leaves.  With ONE and an empty grid (no emitter to sample) a render runs the
 * ordinary kernel instances and equals NONE bit for bit.
 * The estimator (csrc/octpt_emitter.h), at a diffuse reflection in a scene with emitters_enabled: own
 * emittance is added at depth 1 as ever and dropped at depth > 1 exactly on a full-cell block leaf; unless it was just
 * added at depth 1, one emitter of the hit point's cell list (K entries) is picked from an RNG stream of its own, one
 * target in its cube, and one shadow segment is traced (counted like the sun's); when it hits a full-cell block leaf
 * whose entered face emits and is not transparent there, L += T * albedo * col_e^2 * (|dir.n| / max(dist^2, 1) *
 * emittance_e * intensity * K).  The factor K makes ONE an unbiased pick over the list: a deliberate choice.  With sun
 * sampling the emitter segment runs first, then the sun's, then the bounce.
 * With OCTPT_EMITTERS_MODELS (C39) a picked model emitter's target is a point of one of its model's emissive quads,
 * the quad picked in proportion to its area -- the first i of the model's entries with u1 * A_m < cum_area[i], the
 * last one else -- and t = ((origin + u * u2) + v * u3) + corner per component; the factor is (|dir.n| / max(dist^2,
 * 1)) * A_m, Chunky's face-area form.  The segment then also contributes when it hits a block-model quad whose
 * material emits and whose texel's alpha is above EPSILON, and own emittance at depth > 1 is dropped on every
 * emissive hit, quads included: every emissive surface of the scene is listed. */
#define OCTPT_EMITTERS_NONE 0u
#define OCTPT_EMITTERS_ONE 1u
#define OCTPT_EMITTERS_ONE_BLOCK 2u /* reserved */
#define OCTPT_EMITTERS_ALL 3u       /* reserved */
typedef struct octpt_emitter_params {
    uint32_t strategy;
    uint32_t grid_size;
    float intensity;
    uint32_t flags; /* OCTPT_EMITTERS_MODELS or 0 */
    uint32_t reserved[4];
} octpt_emitter_params;
octpt_status octpt_set_emitter_sampling(octpt_ctx *ctx, const octpt_emitter_params *params);
/* The context's device grid, copied back in count-then-fill form (the rules of octpt_emitter_grid_arrays).  With
 * NONE, or no block-value scene, the context holds no grid: INVALID_ARG.  On a multi-device context the first
 * entry's replica. */
octpt_status octpt_emitter_grid(octpt_ctx *ctx, octpt_emitter_grid_arrays *out);
/* The emissive-model table the context's device holds beside its grid (built on the host at the scene entry with
 * octpt_emitter_model_table's arithmetic and uploaded once per scene), copied back in count-then-fill form.  The
 * context holds it when it holds a grid built with OCTPT_EMITTERS_MODELS: INVALID_ARG else.  On a multi-device
 * context the first entry's replica. */
octpt_status octpt_emitter_models(octpt_ctx *ctx, octpt_emitter_model_arrays *out);

/* The emitter sample of one diffuse hit as the emitter instances take it (csrc/octpt_emitter.h, the text they compile):
 * host-only.  grid: filled arrays of a grid of this depth and grid_size; rng_state: the path's RNG state before any
 * draw of the hit.  out = (p.xyz, dir.xyz, dist, |dir.n| / max(dist^2, 1)), *list_length = K of the hit's cell,
 * *emitter the picked index into emitters[], or 0xFFFFFFFF with dir, dist and the factor 0 when no segment is traced
 * (K == 0, or a target at distance 0). */
octpt_status octpt_emitter_sample(const octpt_emitter_grid_arrays *grid, uint32_t depth, uint32_t grid_size,
                                  const float hit[3], const float normal[3], uint32_t rng_state, float out[8],
                                  uint32_t *emitter, uint32_t *list_length);
/* ... over a grid that lists model emitters (C39): table and quads are the filled emissive-model table and the quad
 * table it indexes (INVALID_ARG: a record's model outside the table or without entries, an entry's quad outside the
 * quad table); *quad is the picked quad's index into quads[], or 0xFFFFFFFF for a cube emitter or no segment.  A
 * cube emitter is sampled as octpt_emitter_sample samples it, draw for draw; out[7] carries A_m for a model. */
octpt_status octpt_emitter_sample_models(const octpt_emitter_grid_arrays *grid, const octpt_emitter_model_arrays *table,
                                         const octpt_quad *quads, uint32_t quad_count, uint32_t depth,
                                         uint32_t grid_size, const float hit[3], const float normal[3],
                                         uint32_t rng_state, float out[8], uint32_t *emitter, uint32_t *list_length,
                                         uint32_t *quad);

octpt_status octpt_octree_get_view(const octpt_octree *tree, octpt_octree_view *view);
void octpt_octree_free(octpt_octree *tree);

/* --- the reference's Scene, element by element (the host flattener of INTEGRATION.md §3) ---------
 * textures::material::Material (src/textures/material.rs:91-101) with its Texture (texture.rs:15-18):
 * Texture::Color(U8Color) or Texture::Image(RTWImage) as RGBA8 rows (rtw_image.rs:30-36). */
typedef struct octpt_reference_material {
    float index_of_refraction, specular, emittance, roughness, metalness;
    uint32_t material_flags, tint_index;
    uint32_t texture_kind; /* OCTPT_TEXTURE_COLOR / OCTPT_TEXTURE_IMAGE */
    uint8_t color[4];
    uint32_t image_width, image_height;
    const uint8_t *image_rgba; /* image_width * image_height * 4 bytes, top row first */
} octpt_reference_material;
/* geometry::quad::Quad (src/geometry/quad.rs:7-17) field by field: origin, u, v and the texture
 * ranges are Quad::new's arguments; normal, w and d are what Quad::new derived from them (:90-114) */
typedef struct octpt_reference_quad {
    float origin[3], u[3], v[3], w[3], normal[3], d;
    uint32_t material_id;
    float texture_u_range[2], texture_v_range[2];
} octpt_reference_quad;
/* scene::Scene (src/scene/mod.rs:146-156): the octree as new_octree::Octree holds it (octants_slice,
 * root, depth; either mask encoding, C21; block-value leaves), Box<[Quad]>, Box<[Material]>, the Sun::new
 * arguments with the SunSamplingStrategy, emitters_enabled, f_sub_surface -- plus the block table the
 * host's resource manager resolves block values with (block value -> six face materials or a model;
 * resource_manager.rs:126-318, out of scope) and its block models over `quads`. */
typedef struct octpt_reference_scene {
    const octpt_octant *octants;
    uint32_t octant_count, root, depth;
    const octpt_block *blocks;
    uint32_t block_count;
    const octpt_block_model *models;
    uint32_t model_count;
    const octpt_reference_quad *quads;
    uint32_t quad_count;
    const octpt_reference_material *materials;
    uint32_t material_count;
    octpt_sun sun;
    int32_t emitters_enabled;
    float f_sub_surface;
} octpt_reference_scene;
/* Fill an octpt_scene_desc (for octpt_scene_upload) from the reference's Scene.  Material i becomes
 * octpt_material i with its own texture i (the one-texture-per-material layout GPURenderer uploads,
 * gpu_renderer.rs:221-307); quads keep Quad::new's arguments (octpt_scene_upload derives normal, w and d
 * again, in glam's order).  No allocation: the caller provides materials_out / textures_out
 * (material_count each) and quads_out (quad_count); desc_out points into them and into `ref`'s arrays,
 * so all of them must outlive the upload.  Host-only, no context.  A material, model or quad index out
 * of range, an image without pixels, or a quad whose stored normal disagrees with u x v is INVALID_ARG. */
octpt_status octpt_scene_from_reference(const octpt_reference_scene *ref, octpt_material *materials_out,
                                        octpt_texture *textures_out, octpt_quad *quads_out,
                                        octpt_scene_desc *desc_out);

#ifdef __cplusplus
}
#endif
#endif /* OCTPT_H */
