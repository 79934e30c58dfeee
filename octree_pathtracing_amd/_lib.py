"""ctypes binding of liboctpt.so (include/octpt.h).

This is the Python-side view of the C ABI the Rust host would bind.  The
library is built in-tree by ``__graft_entry__.build()`` into ``octree_pathtracing_amd/lib``;
there is no fallback: importing a renderer without the library raises ``OctptLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

LIB_DIR = Path(__file__).resolve().parent / "lib"
LIB_PATH = LIB_DIR / "liboctpt.so"

OCTPT_ABI_VERSION = 4

OK = 0
ERR_INVALID_ARG = 1
ERR_OOM = 2
ERR_DEVICE = 3
NOT_READY = 4
ERR_UNSUPPORTED = 5
CANCELLED = 6
ERR_INTERNAL = 7

TEXTURE_COLOR = 0
TEXTURE_IMAGE = 1
RENDER_SHARD_COMPACT = 0x1
RENDER_MEGAKERNEL = 0x2
RENDER_KERNEL_TIMING = 0x4
RENDER_PREVIEW = 0x8
BUILD_COMPACT = 0x1  # OCTPT_BUILD_COMPACT
BUILD_CELLS_ON_DEVICE = 0x2  # OCTPT_BUILD_CELLS_ON_DEVICE (the device block builds)
BUILD_SECTIONS_ON_DEVICE = 0x4  # OCTPT_BUILD_SECTIONS_ON_DEVICE (the device section builds)
SECTION_UNIFORM = 0xFFFFFFFF  # OCTPT_SECTION_UNIFORM
PRIM_NONE = 0xFFFFFFFF
PRIM_CUBOID_BIT = 0x80000000

STATUS_NAMES = {
    OK: "OK",
    ERR_INVALID_ARG: "INVALID_ARG",
    ERR_OOM: "OOM",
    ERR_DEVICE: "DEVICE_ERROR",
    NOT_READY: "NOT_READY",
    ERR_UNSUPPORTED: "UNSUPPORTED",
    CANCELLED: "CANCELLED",
    ERR_INTERNAL: "INTERNAL",
}


class OctptLibraryError(RuntimeError):
    """liboctpt.so is missing or failed to load (no CPU fallback exists)."""


class OctptError(RuntimeError):
    def __init__(self, status: int, message: str):
        self.status = status
        super().__init__(f"octpt error {STATUS_NAMES.get(status, status)}: {message}")


class Octant(C.Structure):
    _fields_ = [("child_mask", C.c_uint16), ("reserved", C.c_uint16), ("children", C.c_uint32 * 8)]


class Sphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("material", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class Cuboid(C.Structure):
    _fields_ = [("min", C.c_float * 3), ("max", C.c_float * 3), ("face_material", C.c_uint32 * 6)]


class Quad(C.Structure):
    """octpt_quad: Quad::new arguments (quad.rs:90-114), voxel-local."""
    _fields_ = [("origin", C.c_float * 3), ("material", C.c_uint32), ("u", C.c_float * 3), ("v", C.c_float * 3),
                ("texture_u_range", C.c_float * 2), ("texture_v_range", C.c_float * 2), ("reserved", C.c_uint32 * 2)]


class BlockModel(C.Structure):
    """octpt_block_model (gpu_structs/model.rs:14-21)."""
    _fields_ = [("flags", C.c_uint32), ("first_quad", C.c_uint32), ("quad_count", C.c_uint32),
                ("reserved", C.c_uint32)]


MODEL_NONE = 0xFFFFFFFF


class Block(C.Structure):
    """octpt_block: a block value's six face materials or its block model."""
    _fields_ = [("face_material", C.c_uint32 * 6), ("model", C.c_uint32), ("reserved", C.c_uint32)]


class Section(C.Structure):
    """octpt_section: a 16^3 section's position, palette slice and index block."""
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("z", C.c_uint32), ("palette_first", C.c_uint32),
                ("palette_count", C.c_uint32), ("index_first", C.c_uint32)]


class SectionWorld(C.Structure):
    """octpt_section_world: the three arrays of a world of sections."""
    _fields_ = [("sections", C.c_void_p), ("section_count", C.c_uint32), ("palette", C.c_void_p),
                ("palette_size", C.c_uint32), ("indices", C.c_void_p), ("index_count", C.c_uint32)]


class EmitterGridArrays(C.Structure):
    """octpt_emitter_grid_arrays: the emitter grid's three arrays, count-then-fill."""
    _fields_ = [("cell_first", C.c_void_p), ("cell_first_capacity", C.c_uint32), ("cell_emitters", C.c_void_p),
                ("cell_emitters_capacity", C.c_uint32), ("emitters", C.c_void_p), ("emitters_capacity", C.c_uint32),
                ("cell_count", C.c_uint32), ("entry_count", C.c_uint32), ("emitter_count", C.c_uint32),
                ("cells_per_axis", C.c_uint32)]


class _EmitterParamsTail(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved_tail", C.c_uint32 * 4)]


class EmitterParams(C.Structure):
    """octpt_emitter_params (octpt_set_emitter_sampling).  `reserved` views the five words after intensity, whose
    first is `flags` (EMITTERS_MODELS) and whose other four are reserved."""
    _anonymous_ = ("_tail",)
    _fields_ = [("strategy", C.c_uint32), ("grid_size", C.c_uint32), ("intensity", C.c_float),
                ("_tail", type("_EmitterParamsWords", (C.Union,), {
                    "_anonymous_": ("_named",),
                    "_fields_": [("reserved", C.c_uint32 * 5), ("_named", _EmitterParamsTail)]}))]


class EmitterModelArrays(C.Structure):
    """octpt_emitter_model_arrays: the emissive-model table's three arrays, count-then-fill."""
    _fields_ = [("model_first", C.c_void_p), ("model_first_capacity", C.c_uint32), ("quad_index", C.c_void_p),
                ("quad_index_capacity", C.c_uint32), ("cum_area", C.c_void_p), ("cum_area_capacity", C.c_uint32),
                ("model_count", C.c_uint32), ("entry_count", C.c_uint32)]


EMITTERS_NONE, EMITTERS_ONE, EMITTERS_ONE_BLOCK, EMITTERS_ALL = 0, 1, 2, 3
EMITTERS_MODELS = 1  # octpt_emitter_params.flags: emissive block models are emitters too (C39)


# numpy view of octpt_section rows (scene.SectionWorld.sections)
SECTION_DTYPE = [("x", "<u4"), ("y", "<u4"), ("z", "<u4"), ("palette_first", "<u4"), ("palette_count", "<u4"),
                 ("index_first", "<u4")]
# numpy view of octpt_quad rows (Scene.quads)
QUAD_DTYPE = [("origin", "<f4", (3,)), ("material", "<u4"), ("u", "<f4", (3,)), ("v", "<f4", (3,)),
              ("texture_u_range", "<f4", (2,)), ("texture_v_range", "<f4", (2,)), ("reserved", "<u4", (2,))]


class Material(C.Structure):
    _fields_ = [
        ("ior", C.c_float), ("specular", C.c_float), ("emittance", C.c_float), ("roughness", C.c_float),
        ("metalness", C.c_float), ("texture_index", C.c_uint32), ("tint_index", C.c_uint32), ("flags", C.c_uint32),
    ]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("rgba", C.c_uint8 * 4), ("width", C.c_uint32), ("height", C.c_uint32),
                ("pixels", C.c_void_p)]


class Sun(C.Structure):
    _fields_ = [
        ("azimuth", C.c_float), ("altitude", C.c_float), ("radius", C.c_float), ("color", C.c_float * 4),
        ("apparent_color", C.c_float * 3), ("draw_texture", C.c_int32), ("texture_modification", C.c_int32),
        ("importance_sample_chance", C.c_float), ("importance_sample_radius", C.c_float), ("luminosity", C.c_float),
        ("texture_rgba", C.c_uint8 * 4), ("importance_sampling", C.c_int32), ("diffuse_sun", C.c_int32),
        ("sun_sampling", C.c_int32), ("strict_direct_light", C.c_int32), ("sun_luminosity", C.c_int32),
        ("luminosity_pdf", C.c_float),
    ]


class SceneDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("octants", C.c_void_p), ("octant_count", C.c_uint32), ("root", C.c_uint32),
        ("depth", C.c_uint32), ("leaf_first", C.c_void_p), ("leaf_count", C.c_void_p),
        ("leaf_table_size", C.c_uint32), ("leaf_prims", C.c_void_p), ("leaf_prim_count", C.c_uint32),
        ("spheres", C.c_void_p), ("sphere_count", C.c_uint32), ("cuboids", C.c_void_p), ("cuboid_count", C.c_uint32),
        ("materials", C.c_void_p), ("material_count", C.c_uint32), ("textures", C.c_void_p),
        ("texture_count", C.c_uint32), ("sun", Sun), ("emitters_enabled", C.c_int32), ("f_sub_surface", C.c_float),
        ("cuboid_model", C.c_void_p), ("models", C.c_void_p), ("model_count", C.c_uint32), ("quads", C.c_void_p),
        ("quad_count", C.c_uint32), ("blocks", C.c_void_p), ("block_count", C.c_uint32),
    ]


class ReferenceMaterial(C.Structure):
    """octpt_reference_material: textures::material::Material + its Texture (material.rs:91-101)."""
    _fields_ = [("index_of_refraction", C.c_float), ("specular", C.c_float), ("emittance", C.c_float),
                ("roughness", C.c_float), ("metalness", C.c_float), ("material_flags", C.c_uint32),
                ("tint_index", C.c_uint32), ("texture_kind", C.c_uint32), ("color", C.c_uint8 * 4),
                ("image_width", C.c_uint32), ("image_height", C.c_uint32), ("image_rgba", C.c_void_p)]


class ReferenceQuad(C.Structure):
    """octpt_reference_quad: geometry::quad::Quad field by field (quad.rs:7-17)."""
    _fields_ = [("origin", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("w", C.c_float * 3),
                ("normal", C.c_float * 3), ("d", C.c_float), ("material_id", C.c_uint32),
                ("texture_u_range", C.c_float * 2), ("texture_v_range", C.c_float * 2)]


class ReferenceScene(C.Structure):
    """octpt_reference_scene: scene::Scene (scene/mod.rs:146-156) + the host's block table."""
    _fields_ = [("octants", C.c_void_p), ("octant_count", C.c_uint32), ("root", C.c_uint32), ("depth", C.c_uint32),
                ("blocks", C.c_void_p), ("block_count", C.c_uint32), ("models", C.c_void_p),
                ("model_count", C.c_uint32), ("quads", C.c_void_p), ("quad_count", C.c_uint32),
                ("materials", C.c_void_p), ("material_count", C.c_uint32), ("sun", Sun),
                ("emitters_enabled", C.c_int32), ("f_sub_surface", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("direction", C.c_float * 3), ("up", C.c_float * 3), ("fov", C.c_float),
                ("aperture", C.c_float), ("focal_distance", C.c_float)]


PROJECTION_PINHOLE = 0  # OCTPT_PROJECTION_* 
PROJECTION_PARALLEL = 1
PROJECTION_FISHEYE = 2
PROJECTION_PANORAMIC = 3
PROJECTION_RAYS_CENTRE = 0x1  # OCTPT_PROJECTION_RAYS_CENTRE


class Projection(C.Structure):
    """octpt_projection (octpt_set_projection): the mode and its extent or angle."""
    _fields_ = [("mode", C.c_uint32), ("param", C.c_float), ("reserved", C.c_uint32 * 6)]


class RaySource(C.Structure):
    """octpt_ray_source (octpt_set_ray_source): the caller's list of first rays and its shape."""
    _fields_ = [("d_rays", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32),
                ("rays_per_pixel", C.c_uint32), ("reserved", C.c_uint32 * 5)]


SKY_DEFAULT, SKY_COLOR, SKY_GRADIENT, SKY_MAP = 0, 1, 2, 3  # OCTPT_SKY_* 


class SkyDesc(C.Structure):
    """octpt_sky (octpt_set_sky): the sky's mode and the fields it reads."""
    _fields_ = [("mode", C.c_uint32), ("color", C.c_float * 3), ("horizon", C.c_float * 3), ("zenith", C.c_float * 3),
                ("scale", C.c_float), ("yaw", C.c_float), ("width", C.c_uint32), ("height", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


SKY_SAMPLING_NONE, SKY_SAMPLING_MAP = 0, 1  # OCTPT_SKY_SAMPLING_* 


class SkySampling(C.Structure):
    """octpt_sky_sampling (octpt_set_sky_sampling)."""
    _fields_ = [("mode", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class SkyDistributionArrays(C.Structure):
    """octpt_sky_distribution_arrays: the sky map's distribution, count-then-fill."""
    _fields_ = [("row_cdf", C.c_void_p), ("row_cdf_capacity", C.c_uint64), ("col_cdf", C.c_void_p),
                ("col_cdf_capacity", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32),
                ("build_ms", C.c_float), ("reserved", C.c_uint32)]


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp_start", C.c_uint32), ("spp_count", C.c_uint32),
                ("max_depth", C.c_uint32), ("branch_count", C.c_uint32), ("seed", C.c_uint32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("flags", C.c_uint32)]


DENOISE_DEMODULATE = 0x1  # OCTPT_DENOISE_DEMODULATE
AOV_NAMES = ("albedo", "normal", "depth", "prim", "material")  # octpt_aov_buffers field order


class AovBuffers(C.Structure):
    """octpt_aov_buffers: first-hit guide buffers, NULL = not wanted."""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("prim", C.c_void_p),
                ("material", C.c_void_p)]


class DenoiseParams(C.Structure):
    """octpt_denoise_params."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("flags", C.c_uint32)]


TEMPORAL_MATCH_PRIM = 0x1  # OCTPT_TEMPORAL_MATCH_PRIM
HISTORY_NAMES = ("color", "normal", "depth", "prim", "length")  # octpt_temporal_history field order


class TemporalParams(C.Structure):
    """octpt_temporal_params."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("camera", Camera), ("prev_camera", Camera),
                ("max_history", C.c_uint32), ("depth_tolerance", C.c_float), ("normal_threshold", C.c_float),
                ("flags", C.c_uint32)]


class TemporalHistory(C.Structure):
    """octpt_temporal_history: the previous call's output and the guides it was made with."""
    _fields_ = [("color", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("prim", C.c_void_p),
                ("length", C.c_void_p)]


TEMPORAL_DEMODULATE = 0x2  # OCTPT_TEMPORAL_DEMODULATE: the moments entries alone (C27)


class VarianceParams(C.Structure):
    """octpt_variance_params."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("min_history", C.c_uint32),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


class DenoiseVarianceParams(C.Structure):
    """octpt_denoise_variance_params."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_luminance", C.c_float), ("luminance_floor", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("flags", C.c_uint32)]


class TileErrorParams(C.Structure):
    """octpt_tile_error_params."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("luminance_floor", C.c_float)]


class AdaptiveParams(C.Structure):
    """octpt_adaptive_params."""
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("threshold", C.c_float),
                ("luminance_floor", C.c_float)]


class AdaptiveResult(C.Structure):
    """octpt_adaptive_result."""
    _fields_ = [("rounds", C.c_uint32), ("tile_samples", C.c_uint64), ("converged_tiles", C.c_uint32),
                ("total_tiles", C.c_uint32)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class AdaptiveParamsEx(C.Structure):
    """octpt_adaptive_params_ex: octpt_adaptive_params and the seam rule's neighbour weight."""
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("threshold", C.c_float),
                ("luminance_floor", C.c_float), ("neighbour_weight", C.c_float), ("reserved", C.c_uint32 * 3)]


class SampleVarianceParams(C.Structure):
    """octpt_sample_variance_params."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32)]


class FinalParams(C.Structure):
    """octpt_final_params: the adaptive driver's and the variance-guided filter's."""
    _fields_ = [("adaptive", AdaptiveParamsEx), ("filter", DenoiseVarianceParams)]


TILE = 8  # the wavefront's 8x8 pixel tiles: frame tile t = ty * ceil(W / TILE) + tx (C30)


# octpt_stats::drain order (OCTPT_STAT_*)
STAT_NAMES = ("paths", "segments", "esvo_steps", "sphere_tests", "cuboid_tests", "shade_events", "texel_reads",
              "block_tests", "issued_bytes")
STAT_COUNT = len(STAT_NAMES)


class Stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("esvo_steps", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("cuboid_tests", C.c_uint64), ("shade_events", C.c_uint64),
                ("texel_reads", C.c_uint64), ("launches", C.c_uint64), ("kernel_ms", C.c_double),
                ("extend_launches", C.c_uint64), ("shade_launches", C.c_uint64), ("extend_ms", C.c_double),
                ("shade_ms", C.c_double), ("build_ms", C.c_double), ("block_tests", C.c_uint64),
                ("issued_bytes", C.c_uint64), ("drain", C.c_uint64 * STAT_COUNT), ("pool_slots", C.c_uint64),
                ("chunk_items", C.c_uint64), ("wave_allocs", C.c_uint64), ("beam_restarts", C.c_uint64),
                ("hit_check_failures", C.c_uint64)]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["drain"] = dict(zip(STAT_NAMES, list(self.drain)))  # the drain kernel's share (in the totals)
        return d


class OctreeView(C.Structure):
    _fields_ = [("octants", C.c_void_p), ("octant_count", C.c_uint32), ("root", C.c_uint32), ("depth", C.c_uint32),
                ("leaf_first", C.c_void_p), ("leaf_count", C.c_void_p), ("leaf_table_size", C.c_uint32),
                ("leaf_prims", C.c_void_p), ("leaf_prim_count", C.c_uint32)]


# every symbol include/octpt.h declares, with its ctypes signature
_vp, _u32, _i32, _f = C.c_void_p, C.c_uint32, C.c_int32, C.c_float
SIGNATURES = {
    "octpt_abi_version": (_u32, []),
    "octpt_device_count": (_i32, []),
    "octpt_create": (_i32, [_i32, C.POINTER(_vp)]),
    "octpt_create_multi": (_i32, [_vp, _u32, C.POINTER(_vp)]),
    "octpt_device_entries": (_u32, [_vp]),
    "octpt_destroy": (None, [_vp]),
    "octpt_last_error": (C.c_char_p, [_vp]),
    "octpt_scene_upload": (_i32, [_vp, C.POINTER(SceneDesc)]),
    "octpt_scene_build_device": (_i32, [_vp, C.POINTER(SceneDesc), _u32]),
    "octpt_set_camera": (_i32, [_vp, C.POINTER(Camera)]),
    "octpt_get_camera": (_i32, [_vp, C.POINTER(Camera)]),
    "octpt_set_projection": (_i32, [_vp, C.POINTER(Projection)]),
    "octpt_get_projection": (_i32, [_vp, C.POINTER(Projection)]),
    "octpt_set_ray_source": (_i32, [_vp, C.POINTER(RaySource)]),
    "octpt_get_ray_source": (_i32, [_vp, C.POINTER(RaySource)]),
    "octpt_set_sky": (_i32, [_vp, C.POINTER(SkyDesc), _vp]),
    "octpt_set_sky_device": (_i32, [_vp, C.POINTER(SkyDesc), _vp, _vp]),
    "octpt_clear_sky": (_i32, [_vp]),
    "octpt_get_sky": (_i32, [_vp, C.POINTER(SkyDesc)]),
    "octpt_sky_radiance": (_i32, [C.POINTER(SkyDesc), _vp, _vp, _u32, _vp]),
    "octpt_sky_radiance_device": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "octpt_sky_radiance_ctx": (_i32, [_vp, _vp, _u32, _vp]),
    "octpt_sky_map_position": (_i32, [C.POINTER(SkyDesc), _vp, _u32, _vp]),
    "octpt_set_sky_sampling": (_i32, [_vp, C.POINTER(SkySampling)]),
    "octpt_get_sky_sampling": (_i32, [_vp, C.POINTER(SkySampling)]),
    "octpt_build_sky_distribution": (_i32, [_vp, _u32, _u32, _vp, _vp]),
    "octpt_sky_distribution": (_i32, [_vp, C.POINTER(SkyDistributionArrays)]),
    "octpt_sky_sample": (_i32, [C.POINTER(SkyDistributionArrays), C.POINTER(SkyDesc), _u32, _vp, _vp]),
    "octpt_sky_sample_device": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "octpt_render": (_i32, [_vp, C.POINTER(RenderParams), _vp, _vp]),
    "octpt_render_device": (_i32, [_vp, C.POINTER(RenderParams), _vp, _vp, _vp]),
    "octpt_render_async": (_i32, [_vp, C.POINTER(RenderParams), _vp, _vp, C.POINTER(_vp)]),
    "octpt_frame_poll": (_i32, [_vp]),
    "octpt_frame_wait": (_i32, [_vp]),
    "octpt_frame_cancel": (_i32, [_vp]),
    "octpt_frame_release": (None, [_vp]),
    "octpt_tonemap_device": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "octpt_unshard_device": (_i32, [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp]),
    "octpt_shard_pixels": (_u32, [_u32, _u32, _u32, _u32]),
    "octpt_set_tile_order": (_i32, [_vp, _u32, _u32, _vp]),
    "octpt_balance_tiles": (_i32, [_u32, _u32, _u32, _vp, _vp]),
    "octpt_intersect": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "octpt_traversal_data": (_i32, [_vp, _u32, _u32, _u32, _vp, _f, _vp, _vp, _vp, _vp]),
    "octpt_camera_rays": (_i32, [C.POINTER(Camera), _u32, _u32, _vp]),
    "octpt_lens_rays": (_i32, [C.POINTER(Camera), _u32, _u32, _u32, _u32, _vp]),
    "octpt_projection_rays": (_i32, [C.POINTER(Camera), C.POINTER(Projection), _u32, _u32, _u32, _vp, _u32, _u32, _vp,
                                     _vp]),
    "octpt_ray_source_rays": (_i32, [C.POINTER(Camera), _vp, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _vp]),
    "octpt_render_aov": (_i32, [_vp, C.POINTER(RenderParams), C.POINTER(AovBuffers)]),
    "octpt_render_aov_device": (_i32, [_vp, C.POINTER(RenderParams), C.POINTER(AovBuffers), _vp]),
    "octpt_denoise_device": (_i32, [_vp, C.POINTER(DenoiseParams), _vp, C.POINTER(AovBuffers), _vp, _vp]),
    "octpt_denoise": (_i32, [_vp, C.POINTER(DenoiseParams), _vp, C.POINTER(AovBuffers), _vp]),
    "octpt_temporal_device": (_i32, [_vp, C.POINTER(TemporalParams), _vp, C.POINTER(AovBuffers),
                                     C.POINTER(TemporalHistory), _vp, _vp, _vp]),
    "octpt_temporal": (_i32, [_vp, C.POINTER(TemporalParams), _vp, C.POINTER(AovBuffers),
                              C.POINTER(TemporalHistory), _vp, _vp]),
    "octpt_temporal_moments_device": (_i32, [_vp, C.POINTER(TemporalParams), _vp, C.POINTER(AovBuffers),
                                             C.POINTER(TemporalHistory), _vp, _vp, _vp, _vp, _vp]),
    "octpt_temporal_moments": (_i32, [_vp, C.POINTER(TemporalParams), _vp, C.POINTER(AovBuffers),
                                      C.POINTER(TemporalHistory), _vp, _vp, _vp, _vp]),
    "octpt_variance_device": (_i32, [_vp, C.POINTER(VarianceParams), _vp, _vp, C.POINTER(AovBuffers), _vp, _vp]),
    "octpt_variance": (_i32, [_vp, C.POINTER(VarianceParams), _vp, _vp, C.POINTER(AovBuffers), _vp]),
    "octpt_denoise_variance_device": (_i32, [_vp, C.POINTER(DenoiseVarianceParams), _vp, _vp, C.POINTER(AovBuffers),
                                             _vp, _vp, _vp]),
    "octpt_denoise_variance": (_i32, [_vp, C.POINTER(DenoiseVarianceParams), _vp, _vp, C.POINTER(AovBuffers), _vp,
                                      _vp]),
    "octpt_render_tiles_device": (_i32, [_vp, C.POINTER(RenderParams), _vp, _u32, _vp, _vp, _vp, _vp]),
    "octpt_tile_error_device": (_i32, [_vp, C.POINTER(TileErrorParams), _vp, _vp, _vp, _vp]),
    "octpt_tile_error": (_i32, [_vp, C.POINTER(TileErrorParams), _vp, _vp, _vp]),
    "octpt_render_adaptive_device": (_i32, [_vp, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), _vp, _vp, _vp, _vp,
                                            C.POINTER(AdaptiveResult), _vp]),
    "octpt_render_adaptive": (_i32, [_vp, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), _vp, _vp, _vp, _vp,
                                     C.POINTER(AdaptiveResult)]),
    "octpt_set_sample_clamp": (_i32, [_vp, _f]),
    "octpt_tile_error_spread_device": (_i32, [_vp, _u32, _u32, _f, _vp, _vp, _vp]),
    "octpt_tile_error_spread": (_i32, [_vp, _u32, _u32, _f, _vp, _vp]),
    "octpt_render_adaptive_ex_device": (_i32, [_vp, C.POINTER(RenderParams), C.POINTER(AdaptiveParamsEx), _vp, _vp, _vp,
                                               _vp, C.POINTER(AdaptiveResult), _vp]),
    "octpt_render_adaptive_ex": (_i32, [_vp, C.POINTER(RenderParams), C.POINTER(AdaptiveParamsEx), _vp, _vp, _vp, _vp,
                                        C.POINTER(AdaptiveResult)]),
    "octpt_sample_variance_device": (_i32, [_vp, C.POINTER(SampleVarianceParams), _vp, _vp, C.POINTER(AovBuffers), _vp,
                                            _vp]),
    "octpt_sample_variance": (_i32, [_vp, C.POINTER(SampleVarianceParams), _vp, _vp, C.POINTER(AovBuffers), _vp]),
    "octpt_render_final_device": (_i32, [_vp, C.POINTER(RenderParams), C.POINTER(FinalParams), _vp, _vp, _vp, _vp, _vp,
                                         C.POINTER(AdaptiveResult), _vp]),
    "octpt_render_final": (_i32, [_vp, C.POINTER(RenderParams), C.POINTER(FinalParams), _vp, _vp, _vp, _vp, _vp, _vp,
                                  C.POINTER(AdaptiveResult)]),
    "octpt_reproject_coords": (_i32, [C.POINTER(Camera), C.POINTER(Camera), _u32, _u32, _vp, _vp, _vp]),
    "octpt_reproject_coords_ctx": (_i32, [_vp, C.POINTER(Camera), C.POINTER(Camera), _u32, _u32, _vp, _vp, _vp]),
    "octpt_get_stats": (_i32, [_vp, C.POINTER(Stats)]),
    "octpt_reset_stats": (_i32, [_vp]),
    "octpt_build_octree": (_i32, [_vp, _u32, _vp, _u32, _u32, C.POINTER(_vp)]),
    "octpt_build_octree_device": (_i32, [_vp, _vp, _u32, _vp, _u32, _u32, C.POINTER(_vp)]),
    "octpt_build_octree_ex": (_i32, [_vp, _u32, _vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "octpt_build_octree_device_ex": (_i32, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "octpt_build_block_octree": (_i32, [_vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "octpt_build_block_octree_device": (_i32, [_vp, _vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "octpt_scene_build_blocks_device": (_i32, [_vp, C.POINTER(SceneDesc), _vp, _u32, _u32]),
    "octpt_build_emitter_grid": (_i32, [_vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _u32,
                                        C.POINTER(EmitterGridArrays)]),
    "octpt_set_emitter_sampling": (_i32, [_vp, C.POINTER(EmitterParams)]),
    "octpt_emitter_sample": (_i32, [C.POINTER(EmitterGridArrays), _u32, _u32, _vp, _vp, _u32, _vp, C.POINTER(_u32),
                                    C.POINTER(_u32)]),
    "octpt_emitter_grid": (_i32, [_vp, C.POINTER(EmitterGridArrays)]),
    "octpt_emitter_model_table": (_i32, [_vp, _u32, _vp, _u32, _vp, _u32, C.POINTER(EmitterModelArrays)]),
    "octpt_build_emitter_grid_models": (_i32, [_vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _u32,
                                               _u32, C.POINTER(EmitterGridArrays)]),
    "octpt_emitter_models": (_i32, [_vp, C.POINTER(EmitterModelArrays)]),
    "octpt_emitter_sample_models": (_i32, [C.POINTER(EmitterGridArrays), C.POINTER(EmitterModelArrays), _vp, _u32, _u32,
                                           _u32, _vp, _vp, _u32, _vp, C.POINTER(_u32), C.POINTER(_u32),
                                           C.POINTER(_u32)]),
    "octpt_sections_to_cells": (_i32, [C.POINTER(SectionWorld), _u32, _vp, _u32, C.POINTER(_u32)]),
    "octpt_build_block_octree_sections_device": (_i32, [_vp, C.POINTER(SectionWorld), _u32, _u32, C.POINTER(_vp)]),
    "octpt_scene_build_sections_device": (_i32, [_vp, C.POINTER(SceneDesc), C.POINTER(SectionWorld), _u32]),
    "octpt_scene_from_reference": (_i32, [C.POINTER(ReferenceScene), _vp, _vp, _vp, C.POINTER(SceneDesc)]),
    "octpt_octree_get_view": (_i32, [_vp, C.POINTER(OctreeView)]),
    "octpt_octree_free": (None, [_vp]),
}

_lib = None


def load(path: str | os.PathLike | None = None) -> C.CDLL:
    """Load liboctpt.so and bind every declared symbol; raises if missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # OCTPT_LIB: developer override to A/B differently built kernels (same ABI)
    p = Path(path) if path else Path(os.environ.get("OCTPT_LIB") or LIB_PATH)
    try:  # share torch's HIP runtime (same soname libamdhip64.so.7) when torch is present
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover
        pass
    if not p.exists():
        raise OctptLibraryError(f"{p} not built; run __graft_entry__.build() (no CPU fallback exists)")
    try:
        lib = C.CDLL(str(p))
    except OSError as e:  # pragma: no cover - depends on the box
        raise OctptLibraryError(f"cannot load {p}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.octpt_abi_version() != OCTPT_ABI_VERSION:
        raise OctptLibraryError("liboctpt ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def check(lib, ctx, status: int) -> None:
    if status != OK:
        msg = lib.octpt_last_error(ctx).decode() if ctx else ""
        raise OctptError(status, msg)
