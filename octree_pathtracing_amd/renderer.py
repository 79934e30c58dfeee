"""HipRenderer -- the RenderingBackend / FrameInFlight surface over liboctpt.

Mirrors trait RenderingBackend (reference src/renderer/renderer_trait.rs:19-35),
FrameInFlight / FrameInFlightPoll (:37-46) and the progressive controls of TileRenderer
(src/renderer/tile_renderer.rs:139-296: set_target_spp, get_current_spp, get_image,
reset_render).  Every render goes to the gfx950 kernels; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum

import numpy as np

from . import _lib
from .scene import Camera, RenderSettings, Scene, Sky


class RendererStatus(enum.IntEnum):  # tile_renderer.rs:30-60
    Running = 0
    Paused = 1
    Stopped = 2


class RendererMode(enum.Enum):  # tile_renderer.rs:62-66
    Preview = "Preview"
    PathTraced = "Path Traced"


class FrameInFlightPoll(enum.Enum):  # renderer_trait.rs:37-41
    Ready = "ready"
    NotReady = "not_ready"
    Cancelled = "cancelled"


class FrameInFlight:
    """One progressive pass batch in flight (renderer_trait.rs:42-46)."""

    def __init__(self, renderer: "HipRenderer", handle: C.c_void_p, accum: np.ndarray, rgba: np.ndarray,
                 spp_after: int):
        self._r = renderer
        self._h = handle
        self.accum = accum
        self.rgba = rgba
        self._spp_after = spp_after
        self._done = False

    def _finish(self, cancelled: bool = False):
        if not self._done:
            self._done = True
            self._r._frame_done(self, cancelled)
            self._r._lib.octpt_frame_release(self._h)

    def poll(self):
        """FrameInFlight::poll -> (FrameInFlightPoll, image | self | None)."""
        lib = self._r._lib
        st = lib.octpt_frame_poll(self._h)
        if st == _lib.NOT_READY:
            return FrameInFlightPoll.NotReady, self
        if st == _lib.CANCELLED:
            self._finish(cancelled=True)
            return FrameInFlightPoll.Cancelled, None
        _lib.check(lib, self._r._ctx, st)
        self._finish()
        return FrameInFlightPoll.Ready, self.rgba

    def wait_for(self) -> np.ndarray:
        """FrameInFlight::wait_for -> the tone-mapped image."""
        lib = self._r._lib
        st = lib.octpt_frame_wait(self._h)
        if st == _lib.CANCELLED:
            self._finish(cancelled=True)
            raise _lib.OctptError(st, "frame cancelled")
        _lib.check(lib, self._r._ctx, st)
        self._finish()
        return self.rgba

    def cancel(self) -> None:
        self._r._lib.octpt_frame_cancel(self._h)


# denoise_variance's default luminance_floor: the smallest power of ten at which the filter's f32
# arithmetic stays well conditioned on low-spp frames (tests/test_gpu_svgf.py states the condition)
LUMINANCE_FLOOR = 1e-2


class HipRenderer:
    """RenderingBackend implemented on one MI355X (HIP device `device`), or on several GPUs of the node
    through one context (`devices`: a list of HIP device ids, octpt_create_multi; ids may repeat)."""

    def __init__(self, device: int = 0, resolution=(500, 500), target_spp: int = 1, seed: int = 1,
                 max_depth: int = 5, lib_path=None, devices=None):
        # lib_path: another build of the same ABI (bench.py's issued-bytes diagnostic library)
        self._lib = _lib.load(lib_path) if lib_path else _lib.load()
        ctx = C.c_void_p()
        if devices is None:
            st = self._lib.octpt_create(int(device), C.byref(ctx))
            what = f"octpt_create(device={device})"
        else:
            devs = (C.c_int32 * len(devices))(*map(int, devices))
            st = self._lib.octpt_create_multi(devs, len(devices), C.byref(ctx))
            what = f"octpt_create_multi(devices={list(devices)})"
        if st != _lib.OK:
            raise _lib.OctptError(st, f"{what} failed: no usable gfx950 device")
        self._ctx = ctx
        self._device = int(device) if devices is None else int(devices[0])  # where the caller's buffers live
        self.device_entries = int(self._lib.octpt_device_entries(ctx))
        self._camera = Camera()
        self._resolution = tuple(resolution)
        self._mode = RendererMode.PathTraced
        self._status = RendererStatus.Stopped
        self.target_spp = target_spp
        self.seed = seed
        self.max_depth = max_depth
        self.branch_count = 1  # TileRenderer branch count; 1 = one path per sample
        self._scene_keep = None
        self._scene_emitters = False  # the last set_scene's Scene had emitter sampling on
        self._accum = None
        self._spp = 0
        self._in_flight = None
        self._ray_source = None  # (the tensor set_ray_source keeps alive, (H, W, R)) while a ray source is set
        self._sky = Sky()  # the sky in force (set_sky)
        self.set_camera(self._camera)

    # ------------------------------------------------------------ lifecycle
    def close(self):
        if self._ctx:
            self._lib.octpt_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        _lib.check(self._lib, self._ctx, st)

    # ------------------------------------------------------------ RenderingBackend
    def get_camera(self) -> Camera:
        return self._camera

    def set_camera(self, camera: Camera) -> None:
        """octpt_set_camera, and the camera's projection through set_projection.  The library refuses
        an aperture together with a projection other than pinhole whichever call comes second, so the order is: the
        pinhole projection, the camera, any other projection.  A refused call leaves both as they were."""
        mode, param = int(camera.projection[0]), float(camera.projection[1])
        pinhole = mode == _lib.PROJECTION_PINHOLE
        if not pinhole and camera.aperture > 0.0:
            raise _lib.OctptError(_lib.ERR_UNSUPPORTED, "an aperture needs the pinhole projection")
        old = self._camera
        changed = (mode, param) != tuple(old.projection)  # else the setter is not called
        if pinhole and changed:
            self.set_projection(mode, param)
        try:
            self._check(self._lib.octpt_set_camera(self._ctx, C.byref(_c_camera(camera, lens=True))))
            if not pinhole and changed:
                self.set_projection(mode, param)
        except _lib.OctptError:
            # one of the two is already set; the other call, refused, left its half as it was
            if pinhole and changed:
                self.set_projection(*old.projection)
            else:
                self._lib.octpt_set_camera(self._ctx, C.byref(_c_camera(old, lens=True)))
            raise
        self._camera = camera
        self.reset_render()

    def set_projection(self, mode: int, param: float = 0.0) -> None:
        """octpt_set_projection: _lib.PROJECTION_PINHOLE (a new renderer's), PARALLEL (param: the world-space length
        across the longer image side), FISHEYE or PANORAMIC (param: the full angle across it, radians, at most 2 pi),
        for every later render of this renderer -- path traced, preview and guide buffers."""
        p = _lib.Projection(int(mode), float(param))
        self._check(self._lib.octpt_set_projection(self._ctx, C.byref(p)))
        self._camera = dataclasses.replace(self._camera, projection=(int(mode), float(param)))
        self.reset_render()

    def get_projection(self) -> tuple:
        p = _lib.Projection()
        self._check(self._lib.octpt_get_projection(self._ctx, C.byref(p)))
        return int(p.mode), float(p.param)

    def set_ray_source(self, rays, rays_per_pixel: int | None = None) -> None:
        """octpt_set_ray_source: every later render of this renderer takes the first ray of sample s
        of pixel (x, y) from rays[y, x, s % R] = (origin xyz, direction xyz), a unit direction used as given; an
        invalid record (non-finite, or not of unit length) renders as the camera's central ray.  `rays`: a float32
        torch tensor on this renderer's device or a numpy array (uploaded), of shape (H, W, R, 6); the renderer holds
        it until clear_ray_source or the next set_ray_source, and it must not be written while renders read it.
        Renders must then be H x W; the preview and the guide buffers trace rays[y, x, 0]."""
        import torch

        dev = torch.device("cuda", self._device)
        t = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(dev) if isinstance(rays, np.ndarray) else rays
        if t.dim() != 4 or t.shape[3] != 6:
            raise ValueError(f"rays has shape {tuple(t.shape)}, not (H, W, R, 6)")
        if rays_per_pixel is not None and int(rays_per_pixel) != t.shape[2]:
            raise ValueError(f"rays holds {t.shape[2]} rays per pixel, not {rays_per_pixel}")
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"rays must be a contiguous float32 tensor on {dev}")
        H, W, R = (int(v) for v in t.shape[:3])
        src = _lib.RaySource(t.data_ptr(), W, H, R)
        self._check(self._lib.octpt_set_ray_source(self._ctx, C.byref(src)))
        self._ray_source = (t, (H, W, R))
        self.reset_render()

    def clear_ray_source(self) -> None:
        """Back to the renderer's own camera: renders are bit for bit those of a renderer that never had a source."""
        self._check(self._lib.octpt_set_ray_source(self._ctx, None))
        self._ray_source = None
        self.reset_render()

    def get_ray_source(self):
        """octpt_get_ray_source: (device pointer or None, width, height, rays_per_pixel)."""
        src = _lib.RaySource()
        self._check(self._lib.octpt_get_ray_source(self._ctx, C.byref(src)))
        return src.d_rays, int(src.width), int(src.height), int(src.rays_per_pixel)

    def ray_source_rays(self, rays: np.ndarray, seed: int, xys):
        """octpt_ray_source_rays with this renderer's camera as the fallback: for rows (x, y, sample) the first rays
        [n, 6] a render under the list `rays` (H, W, R, 6) traces, bit for bit, and the paths' RNG states [n]."""
        return ray_source_rays(self._camera, rays, seed, xys)

    def set_sky(self, sky: Sky) -> None:
        """octpt_set_sky: the base colour every later render of this renderer adds where a ray leaves
        the world -- scene.Sky.color / gradient / map, or Sky() for the default constant.  The library copies a map
        (a numpy array is staged, a tensor on this renderer's device is copied there), so the caller's stays its own.
        A refused setting (OctptError) leaves the previous sky in force."""
        d = sky.desc()
        tex = sky.texels
        if tex is None or isinstance(tex, np.ndarray):
            host = np.ascontiguousarray(tex, np.float32) if tex is not None else None
            st = self._lib.octpt_set_sky(self._ctx, C.byref(d), host.ctypes.data if host is not None else None)
        else:
            import torch

            dev = torch.device("cuda", self._device)
            if tex.dtype != torch.float32 or tex.device != dev or not tex.is_contiguous():
                raise ValueError(f"a sky map tensor must be contiguous float32 on {dev}")
            st = self._lib.octpt_set_sky_device(self._ctx, C.byref(d), tex.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream)
        self._check(st)
        self._sky = sky
        self.reset_render()

    def clear_sky(self) -> None:
        """Back to the default sky: renders are bit for bit those of a renderer that never had one."""
        self._check(self._lib.octpt_clear_sky(self._ctx))
        self._sky = Sky()
        self.reset_render()

    def get_sky(self) -> Sky:
        """The setting in force (the last accepted set_sky's, or Sky())."""
        return self._sky

    def set_sky_sampling(self, on: bool) -> None:
        """octpt_set_sky_sampling: next-event estimation toward the sky map's bright texels in every
        later render of this renderer.  It may come before or after set_sky; under a sky that is not a map, or an
        all-black one, renders are what they are without it.  A refused setting (OctptError) leaves the previous one."""
        p = _lib.SkySampling()
        p.mode = _lib.SKY_SAMPLING_MAP if on else _lib.SKY_SAMPLING_NONE
        self._check(self._lib.octpt_set_sky_sampling(self._ctx, C.byref(p)))
        self.reset_render()

    @property
    def sky_sampling(self) -> bool:
        """The setting in force (octpt_get_sky_sampling)."""
        p = _lib.SkySampling()
        self._check(self._lib.octpt_get_sky_sampling(self._ctx, C.byref(p)))
        return p.mode == _lib.SKY_SAMPLING_MAP

    def sky_distribution(self):
        """octpt_sky_distribution: the distribution this renderer's device built from its map, copied back --
        {"row_cdf": uint64 [H], "col_cdf": uint32 [H, W], "total": int, "build_ms": float} -- or None when it holds
        none (sampling off, no map sky).  scene.build_sky_distribution is the CPU definition; the two are equal."""
        a = _lib.SkyDistributionArrays()
        self._check(self._lib.octpt_sky_distribution(self._ctx, C.byref(a)))
        if a.width == 0:
            return None
        row = np.zeros(a.height, np.uint64)
        col = np.zeros((a.height, a.width), np.uint32)
        a.row_cdf, a.row_cdf_capacity, a.col_cdf, a.col_cdf_capacity = row.ctypes.data, row.size, col.ctypes.data, col.size
        self._check(self._lib.octpt_sky_distribution(self._ctx, C.byref(a)))
        return {"row_cdf": row, "col_cdf": col, "total": int(row[-1]), "build_ms": float(a.build_ms)}

    def sky_samples(self, u) -> dict:
        """octpt_sky_sample_device: the sky sample of draw tuples u [n, 4] over this renderer's distribution and sky,
        computed on the device by the kernels' text (scene.sky_samples is the CPU form; the two agree bit for bit)."""
        import torch

        from .scene import unpack_sky_samples

        dev = torch.device("cuda", self._device)
        du = torch.from_numpy(np.ascontiguousarray(u, np.float32).reshape(-1, 4)).to(dev)
        out = torch.zeros((du.shape[0], 8), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev)
        self._check(self._lib.octpt_sky_sample_device(self._ctx, du.data_ptr(), du.shape[0], out.data_ptr(),
                                                      stream.cuda_stream))
        stream.synchronize()
        return unpack_sky_samples(out.cpu().numpy())

    def sky_radiance(self, dirs) -> np.ndarray:
        """octpt_sky_radiance_ctx: the colour [n, 3] this renderer's sky adds for unit directions [n, 3] (the sun's
        terms excluded), computed on the device by the kernels' text.  scene.Sky.radiance is the CPU form; the two
        agree bit for bit."""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros_like(dirs)
        self._check(self._lib.octpt_sky_radiance_ctx(self._ctx, dirs.ctypes.data, len(dirs), out.ctypes.data))
        return out

    def which_backend(self) -> str:
        return "HIP (gfx950)"

    def set_resolution(self, resolution) -> None:
        self._resolution = (int(resolution[0]), int(resolution[1]))
        self.reset_render()

    def get_resolution(self):
        return self._resolution

    def get_status(self) -> RendererStatus:
        return self._status

    def set_mode(self, mode: RendererMode) -> None:
        """TileRenderer::set_mode (tile_renderer.rs:188-191): stops and restarts the accumulation."""
        self._mode = RendererMode(mode)
        self.reset_render()

    def get_mode(self) -> RendererMode:
        return self._mode

    def update_scene(self, *_args) -> None:
        """RenderingBackend::update_scene (egui hook) -- nothing to do for HIP."""

    def set_scene(self, scene: Scene) -> None:
        desc, keep = scene.to_desc()
        self._check(self._lib.octpt_scene_upload(self._ctx, C.byref(desc)))
        # the scene's emitter sampling (C38) is the renderer's from here on: a scene with NONE switches it off
        if scene.emitter_sampling != _lib.EMITTERS_NONE or self._scene_emitters:
            self.set_emitter_sampling(scene.emitter_sampling, scene.emitter_grid_size, scene.emitter_intensity,
                                      models=scene.emitter_models)
        self._scene_emitters = scene.emitter_sampling != _lib.EMITTERS_NONE
        self._scene_keep = keep
        self.reset_render()

    def set_scene_built(self, scene: Scene, depth: int, compact: bool = False) -> None:
        """set_scene with the octree built on this GPU and kept there (octpt_scene_build_device): the
        device scene equals set_scene(scene) after scene.build_octree(depth, compact=compact), without
        the host round trip.  scene.octree is left untouched.  A block-value scene (scene.blocks set) builds
        from scene.cells with octpt_scene_build_blocks_device."""
        if scene.blocks is not None:
            cells = scene.cells_array()
            self._set_scene_built_blocks(scene, depth, cells.ctypes.data if len(cells) else None, len(cells),
                                         _lib.BUILD_COMPACT if compact else 0)
            return
        desc, keep = scene.to_desc(octree=False, depth=depth)
        self._check(self._lib.octpt_scene_build_device(self._ctx, C.byref(desc), _lib.BUILD_COMPACT if compact else 0))
        self._scene_keep = keep
        self.reset_render()

    def set_scene_built_cells(self, scene: Scene, depth: int, cells_ptr: int, cell_count: int,
                              compact: bool = False) -> None:
        """set_scene_built for a block-value scene whose cells are already on this GPU: cells_ptr is a device
        pointer to cell_count rows of (x, y, z, block) uint32, e.g. a torch int32 tensor's data_ptr()
        (OCTPT_BUILD_CELLS_ON_DEVICE).  The cells must be complete before the call (synchronise the stream
        that wrote them): the library reads them on its own stream.  scene.cells is not read."""
        if scene.blocks is None:
            raise ValueError("set_scene_built_cells: a block-value scene (scene.blocks) is needed")
        self._set_scene_built_blocks(scene, depth, int(cells_ptr), int(cell_count),
                                     _lib.BUILD_CELLS_ON_DEVICE | (_lib.BUILD_COMPACT if compact else 0))

    def set_scene_built_sections(self, scene: Scene, depth: int, world, compact: bool = False,
                                 on_device=False) -> None:
        """set_scene_built for a block-value scene from a scene.SectionWorld (octpt_scene_build_sections_device):
        the device scene equals set_scene after a host build of world.to_cells().  on_device: the (sections,
        palette, indices) device addresses of copies of the world's arrays on this GPU, complete before the call
        (OCTPT_BUILD_SECTIONS_ON_DEVICE); False: the host arrays are uploaded.  scene.cells is not read."""
        if scene.blocks is None:
            raise ValueError("set_scene_built_sections: a block-value scene (scene.blocks) is needed")
        flags = (_lib.BUILD_COMPACT if compact else 0) | (_lib.BUILD_SECTIONS_ON_DEVICE if on_device else 0)
        desc, keep = scene.to_desc(octree=False, depth=depth)
        w = world.struct(on_device if on_device else None)
        self._check(self._lib.octpt_scene_build_sections_device(self._ctx, C.byref(desc), C.byref(w), flags))
        self._scene_keep = keep
        self.reset_render()

    def _set_scene_built_blocks(self, scene: Scene, depth: int, cells_ptr, cell_count: int, flags: int) -> None:
        desc, keep = scene.to_desc(octree=False, depth=depth)
        self._check(self._lib.octpt_scene_build_blocks_device(self._ctx, C.byref(desc), cells_ptr, cell_count, flags))
        self._scene_keep = keep
        self.reset_render()

    def render_frame(self, spp_count: int | None = None) -> FrameInFlight:
        """RenderingBackend::render_frame: enqueue the next pass batch, return a FrameInFlight."""
        if self._in_flight is not None:
            raise RuntimeError("a frame is already in flight")
        W, H = self._resolution
        if self._accum is None:
            self._accum = np.zeros((H, W, 4), np.float32)
            self._accum[..., 3] = 1.0
        preview = self._mode is RendererMode.Preview
        n = spp_count if spp_count is not None else max(self.target_spp - self._spp, 1)
        if self.branch_count > 1:  # whole passes of the branch schedule (C20), as TileRenderer runs them
            n = branch_pass_end(self._spp, n, self.branch_count) - self._spp
        if preview:  # render_preview (tile_renderer.rs:339-374): one replacing pass, current_spp stays 0
            n = 0
        p = self.params(W, H, self._spp, n, preview=preview)
        rgba = np.zeros((H, W, 4), np.uint8)
        h = C.c_void_p()
        self._check(self._lib.octpt_render_async(self._ctx, C.byref(p), self._accum.ctypes.data_as(C.c_void_p),
                                                 rgba.ctypes.data_as(C.c_void_p), C.byref(h)))
        self._status = RendererStatus.Running
        f = FrameInFlight(self, h, self._accum, rgba, self._spp + n)
        self._in_flight = f
        return f

    def _frame_done(self, f: FrameInFlight, cancelled: bool = False):
        if not cancelled:  # a cancelled frame leaves the accumulation untouched
            self._spp = f._spp_after
        self._in_flight = None
        self._status = RendererStatus.Stopped

    # ------------------------------------------------------------ TileRenderer-style controls
    def reset_render(self) -> None:
        self._accum = None
        self._spp = 0

    def set_target_spp(self, spp: int) -> None:
        self.target_spp = max(self.target_spp, int(spp))

    def get_current_spp(self) -> int:
        return self._spp

    def get_float_image(self) -> np.ndarray | None:
        return self._accum

    # ------------------------------------------------------------ direct entry points
    def params(self, W, H, spp_start, spp_count, shard_index=0, shard_count=1, compact=False,
               megakernel=False, kernel_timing=False, preview=False) -> "_lib.RenderParams":
        flags = ((_lib.RENDER_SHARD_COMPACT if compact else 0) | (_lib.RENDER_MEGAKERNEL if megakernel else 0)
                 | (_lib.RENDER_KERNEL_TIMING if kernel_timing else 0) | (_lib.RENDER_PREVIEW if preview else 0))
        return _lib.RenderParams(W, H, spp_start, spp_count, self.max_depth, self.branch_count, self.seed,
                                 shard_index, shard_count, flags)

    def render(self, settings: RenderSettings, accum: np.ndarray | None = None, spp_start: int = 0,
               with_rgba: bool = False):
        """Synchronous progressive render into host memory: returns (accum[H,W,4], rgba or None)."""
        W, H = settings.width, settings.height
        if accum is None:
            accum = np.zeros((H, W, 4), np.float32)
            accum[..., 3] = 1.0
        accum = np.ascontiguousarray(accum, np.float32)
        rgba = np.zeros((H, W, 4), np.uint8) if with_rgba else None
        self.max_depth = settings.max_depth
        self.seed = settings.seed
        p = self.params(W, H, spp_start, settings.spp)
        self._check(self._lib.octpt_render(self._ctx, C.byref(p), accum.ctypes.data_as(C.c_void_p),
                                           rgba.ctypes.data_as(C.c_void_p) if rgba is not None else None))
        return accum, rgba

    def render_device(self, params: "_lib.RenderParams", d_accum: int, d_seg_count: int | None = None,
                      stream: int | None = None) -> None:
        """Enqueue a render on device buffers (raw device pointers, e.g. torch tensor.data_ptr())."""
        self._check(self._lib.octpt_render_device(self._ctx, C.byref(params), C.c_void_p(d_accum),
                                                  C.c_void_p(d_seg_count) if d_seg_count else None,
                                                  C.c_void_p(stream) if stream else None))

    def tonemap_device(self, d_accum: int, d_rgba: int, n_pixels: int, stream: int | None = None) -> None:
        self._check(self._lib.octpt_tonemap_device(self._ctx, C.c_void_p(d_accum), C.c_void_p(d_rgba), n_pixels,
                                                   C.c_void_p(stream) if stream else None))

    def unshard_device(self, W, H, shard_count, d_shards: int, stride: int, d_frame: int, stream=None) -> None:
        self._check(self._lib.octpt_unshard_device(self._ctx, W, H, shard_count, C.c_void_p(d_shards), stride,
                                                   C.c_void_p(d_frame), C.c_void_p(stream) if stream else None))

    def set_tile_order(self, W: int, H: int, order: np.ndarray | None) -> None:
        """The tile deal for W x H renders (octpt_set_tile_order): order[s] = the frame tile at dealing position s
        (shard k owns positions k + u * N); None = round robin."""
        if order is None:
            self._check(self._lib.octpt_set_tile_order(self._ctx, W, H, None))
            return
        o = np.ascontiguousarray(order, np.uint32)
        self._check(self._lib.octpt_set_tile_order(self._ctx, W, H, o.ctypes.data_as(C.c_void_p)))

    def intersect(self, rays: np.ndarray, last_prim=None, last_normal=None):
        """Batch Scene::hit: returns (t, prim, normal, steps)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        t = np.zeros(n, np.float32)
        prim = np.zeros(n, np.uint32)
        nrm = np.zeros((n, 3), np.float32)
        steps = np.zeros(n, np.uint32)
        lp = None if last_prim is None else np.ascontiguousarray(last_prim, np.uint32)
        ln = None if last_normal is None else np.ascontiguousarray(last_normal, np.float32)

        def P(a):
            return a.ctypes.data_as(C.c_void_p) if a is not None else None

        self._check(self._lib.octpt_intersect(self._ctx, P(rays), P(lp), P(ln), n, P(t), P(prim), P(nrm), P(steps)))
        return t, prim, nrm, steps

    # ------------------------------------------------------------ guide buffers and denoise (C24, C25)
    def camera_rays(self, W: int, H: int) -> np.ndarray:
        """octpt_camera_rays of the current camera: [H, W, 6] (origin, unit direction), the rays the device
        traces for the pixel centres, bit for bit."""
        return camera_rays(self._camera, W, H)

    def lens_rays(self, W: int, H: int, seed: int, sample: int) -> np.ndarray:
        """octpt_lens_rays of the current camera: [H, W, 6], the first ray a W x H render with this seed traces
        for sample `sample` of each pixel, bit for bit."""
        return lens_rays(self._camera, W, H, seed, sample)

    def projection_rays(self, W: int, H: int, seed: int, xys, centre: bool = False):
        """octpt_projection_rays of the current camera and its projection: for rows (x, y, sample) the first rays
        [n, 6] a W x H render with this seed traces, bit for bit, and the paths' RNG states after them [n]; centre:
        the un-jittered rays of the preview and the guide buffers."""
        return projection_rays(self._camera, W, H, seed, xys, centre=centre)

    def reproject_coords(self, prev_camera: Camera, W: int, H: int, depth: np.ndarray):
        """octpt_reproject_coords_ctx for this renderer's camera and frames: reproject_coords, refused (UNSUPPORTED)
        while the renderer's projection is not pinhole."""
        depth = np.ascontiguousarray(depth, np.float32)
        if depth.size != W * H:
            raise ValueError(f"depth holds {depth.size} pixels, not {W} x {H}")
        xy = np.zeros((H, W, 2), np.float32)
        zp = np.zeros((H, W), np.float32)
        self._check(self._lib.octpt_reproject_coords_ctx(
            self._ctx, C.byref(_c_camera(self._camera)), C.byref(_c_camera(prev_camera)), W, H,
            depth.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p), zp.ctypes.data_as(C.c_void_p)))
        return xy, zp

    def render_aov(self, settings: RenderSettings, which=_lib.AOV_NAMES, shard=(0, 1), compact: bool = False,
                   out: dict | None = None) -> dict:
        """First-hit guide buffers (octpt_render_aov) -> {name: array} for the names in `which`: albedo and
        normal [.., 4] f32, depth f32, prim and material u32; shaped [H, W] for a full frame, or flat over the
        shard's tile-major pixels with compact.  shard = (index, count).  `out` supplies the arrays to fill
        (a partial shard of a full frame leaves the other pixels as they are)."""
        W, H = settings.width, settings.height
        n = shard_pixels(W, H, *shard) if compact else W * H
        shape = (n,) if compact else (H, W)
        res, b = {}, _lib.AovBuffers()
        for name in which:
            if name not in _lib.AOV_NAMES:
                raise ValueError(f"unknown guide buffer {name!r}; known: {_lib.AOV_NAMES}")
            dt, tail = (np.float32, (4,)) if name in ("albedo", "normal") else \
                (np.float32, ()) if name == "depth" else (np.uint32, ())
            a = out[name] if out is not None else np.zeros(shape + tail, dt)
            if a.dtype != dt or a.size != n * (4 if tail else 1) or not a.flags.c_contiguous:
                raise ValueError(f"{name}: expected a contiguous {np.dtype(dt).name} array of {shape + tail}")
            res[name] = a
            setattr(b, name, a.ctypes.data)
        p = self.params(W, H, 0, 0, shard_index=shard[0], shard_count=shard[1], compact=compact)
        self._check(self._lib.octpt_render_aov(self._ctx, C.byref(p), C.byref(b)))
        return res

    def render_aov_device(self, params: "_lib.RenderParams", buffers: dict, stream: int | None = None) -> None:
        """Enqueue the guide-buffer pass into device buffers: {name: raw device pointer} (e.g. torch
        tensor.data_ptr()) for the wanted names of _lib.AOV_NAMES."""
        b = _lib.AovBuffers(**{k: C.c_void_p(int(v)) for k, v in buffers.items() if v})
        self._check(self._lib.octpt_render_aov_device(self._ctx, C.byref(params), C.byref(b),
                                                      C.c_void_p(stream) if stream else None))

    def denoise(self, color: np.ndarray, aov: dict, iterations: int = 5, sigma_color: float = 0.6,
                sigma_normal: float = 0.3, sigma_depth: float = 0.1, demodulate: bool = True) -> np.ndarray:
        """Edge-avoiding a-trous filter (octpt_denoise) of a [H, W, 4] frame guided by render_aov's normal and
        depth (and albedo with demodulate); returns the filtered frame."""
        color = np.ascontiguousarray(color, np.float32)
        H, W = color.shape[:2]
        b = _lib.AovBuffers()
        keep = []
        for name in ("normal", "depth") + (("albedo",) if demodulate else ()):
            if aov.get(name) is None:
                continue  # the library reports the missing guide
            a = np.ascontiguousarray(aov[name], np.float32)
            if a.size != W * H * (1 if name == "depth" else 4):
                raise ValueError(f"{name} guide does not match the {W} x {H} frame")
            keep.append(a)
            setattr(b, name, a.ctypes.data)
        p = _lib.DenoiseParams(W, H, iterations, sigma_color, sigma_normal, sigma_depth,
                               _lib.DENOISE_DEMODULATE if demodulate else 0)
        out = np.empty_like(color)
        self._check(self._lib.octpt_denoise(self._ctx, C.byref(p), color.ctypes.data_as(C.c_void_p), C.byref(b),
                                            out.ctypes.data_as(C.c_void_p)))
        return out

    def denoise_device(self, params: "_lib.DenoiseParams", d_color: int, guides: dict, d_out: int,
                       stream: int | None = None) -> None:
        """Enqueue octpt_denoise_device on raw device pointers (d_out may equal d_color)."""
        b = _lib.AovBuffers(**{k: C.c_void_p(int(v)) for k, v in guides.items() if v})
        self._check(self._lib.octpt_denoise_device(self._ctx, C.byref(params), C.c_void_p(d_color), C.byref(b),
                                                   C.c_void_p(d_out), C.c_void_p(stream) if stream else None))

    # ------------------------------------------------------------ temporal reprojection (C26)
    def temporal(self, color: np.ndarray, aov: dict, history: dict | None = None, prev_camera: Camera | None = None,
                 max_history: int = 32, depth_tolerance: float = 0.1, normal_threshold: float = 0.9,
                 match_prim: bool = True, moments: bool = False, demodulate: bool = False) -> dict:
        """Carry `history` (the dict a previous call returned, None on the first frame) to the current camera's
        frame and blend the new [H, W, 4] `color` into it (octpt_temporal), guided by render_aov's normal, depth
        and (with match_prim) prim of the current frame.  prev_camera: the history's camera, by default the one
        it recorded.  Returns the new history: color (the blended frame, what denoise takes next), normal, depth,
        prim, length (u32 [H, W]: samples of history per pixel, 0 on misses) and camera.
        moments: octpt_temporal_moments (C27) -- the luminance moments [H, W, 2] of the working signal travel with
        the colour: read from history["moments"], returned as "moments"; demodulate (only with moments): the
        working signal is color / max(albedo, 1e-3), as denoise_variance's is."""
        if demodulate and not moments:
            raise ValueError("demodulate applies to the moments (moments=True)")
        color = np.ascontiguousarray(color, np.float32)
        H, W = color.shape[:2]
        keep = []

        def ptr(src, name, dt):
            if src.get(name) is None:
                return None  # the library reports what is missing
            a = np.ascontiguousarray(src[name], dt)
            if a.size != W * H * {"color": 4, "normal": 4, "albedo": 4, "moments": 2}.get(name, 1):
                raise ValueError(f"{name} does not match the {W} x {H} frame")
            keep.append(a)
            return a.ctypes.data

        names = ("normal", "depth") + (("prim",) if match_prim else ())
        dtype = {"color": np.float32, "normal": np.float32, "depth": np.float32, "prim": np.uint32, "length": np.uint32,
                 "albedo": np.float32, "moments": np.float32}
        g = _lib.AovBuffers(**{k: ptr(aov, k, dtype[k]) for k in names + (("albedo",) if demodulate else ())})
        prev = None
        if history is not None:
            prev = _lib.TemporalHistory(**{k: ptr(history, k, dtype[k]) for k in ("color", "length") + names})
            prev_camera = prev_camera or history.get("camera")
        cam = self._camera
        p = _lib.TemporalParams(W, H, _c_camera(cam), _c_camera(prev_camera or cam), max_history, depth_tolerance,
                                normal_threshold, _lib.TEMPORAL_MATCH_PRIM if match_prim else 0)
        out = np.empty_like(color)
        length = np.empty((H, W), np.uint32)
        res = {"color": out, "normal": aov.get("normal"), "depth": aov.get("depth"), "prim": aov.get("prim"),
               "length": length, "camera": cam}
        if moments:
            p.flags |= _lib.TEMPORAL_DEMODULATE if demodulate else 0
            res["moments"] = np.empty((H, W, 2), np.float32)
            self._check(self._lib.octpt_temporal_moments(
                self._ctx, C.byref(p), color.ctypes.data_as(C.c_void_p), C.byref(g),
                C.byref(prev) if prev is not None else None,
                ptr(history, "moments", np.float32) if history is not None else None, out.ctypes.data_as(C.c_void_p),
                length.ctypes.data_as(C.c_void_p), res["moments"].ctypes.data_as(C.c_void_p)))
            return res
        self._check(self._lib.octpt_temporal(self._ctx, C.byref(p), color.ctypes.data_as(C.c_void_p), C.byref(g),
                                             C.byref(prev) if prev is not None else None,
                                             out.ctypes.data_as(C.c_void_p), length.ctypes.data_as(C.c_void_p)))
        return res

    def temporal_device(self, params: "_lib.TemporalParams", d_color: int, guides: dict, prev: dict | None, d_out: int,
                        d_out_length: int, stream: int | None = None) -> None:
        """Enqueue octpt_temporal_device on raw device pointers: guides {normal, depth, prim}, prev {color,
        normal, depth, prim, length} or None for the first frame (d_out may equal d_color)."""
        b = _lib.AovBuffers(**{k: C.c_void_p(int(v)) for k, v in guides.items() if v})
        h = _lib.TemporalHistory(**{k: C.c_void_p(int(v)) for k, v in prev.items() if v}) if prev is not None else None
        self._check(self._lib.octpt_temporal_device(self._ctx, C.byref(params), C.c_void_p(d_color), C.byref(b),
                                                    C.byref(h) if h is not None else None, C.c_void_p(d_out),
                                                    C.c_void_p(d_out_length), C.c_void_p(stream) if stream else None))

    def temporal_moments_device(self, params: "_lib.TemporalParams", d_color: int, guides: dict, prev: dict | None,
                                d_prev_moments: int | None, d_out: int, d_out_length: int, d_out_moments: int,
                                stream: int | None = None) -> None:
        """Enqueue octpt_temporal_moments_device on raw device pointers: temporal_device's arguments (guides with
        albedo under TEMPORAL_DEMODULATE) and the previous and the output moments planes."""
        b = _lib.AovBuffers(**{k: C.c_void_p(int(v)) for k, v in guides.items() if v})
        h = _lib.TemporalHistory(**{k: C.c_void_p(int(v)) for k, v in prev.items() if v}) if prev is not None else None
        self._check(self._lib.octpt_temporal_moments_device(
            self._ctx, C.byref(params), C.c_void_p(d_color), C.byref(b), C.byref(h) if h is not None else None,
            C.c_void_p(d_prev_moments) if d_prev_moments else None, C.c_void_p(d_out), C.c_void_p(d_out_length),
            C.c_void_p(d_out_moments), C.c_void_p(stream) if stream else None))

    # ------------------------------------------------------------ variance and the variance-guided filter (C28, C29)
    def _guides(self, aov: dict, names, W: int, H: int, keep: list) -> "_lib.AovBuffers":
        b = _lib.AovBuffers()
        for name in names:
            if aov.get(name) is None:
                continue  # the library reports the missing guide
            a = np.ascontiguousarray(aov[name], np.float32)
            if a.size != W * H * (1 if name == "depth" else 4):
                raise ValueError(f"{name} guide does not match the {W} x {H} frame")
            keep.append(a)
            setattr(b, name, a.ctypes.data)
        return b

    def variance(self, history: dict, aov: dict, min_history: int = 4, sigma_normal: float = 0.3,
                 sigma_depth: float = 0.1) -> np.ndarray:
        """The per-pixel variance [H, W] of the working signal's luminance (octpt_variance) from the moments and
        length of `history` (what temporal(..., moments=True) returned) and render_aov's normal and depth: the
        temporal estimate where the history is min_history long, a 7 x 7 spatial one where it is shorter."""
        length = np.ascontiguousarray(history["length"], np.uint32)
        H, W = length.shape
        m = np.ascontiguousarray(history["moments"], np.float32)
        if m.size != 2 * W * H:
            raise ValueError(f"moments do not match the {W} x {H} frame")
        keep = []
        b = self._guides(aov, ("normal", "depth"), W, H, keep)
        p = _lib.VarianceParams(W, H, min_history, sigma_normal, sigma_depth)
        out = np.empty((H, W), np.float32)
        self._check(self._lib.octpt_variance(self._ctx, C.byref(p), m.ctypes.data_as(C.c_void_p),
                                             length.ctypes.data_as(C.c_void_p), C.byref(b),
                                             out.ctypes.data_as(C.c_void_p)))
        return out

    def variance_device(self, params: "_lib.VarianceParams", d_moments: int, d_length: int, guides: dict, d_out: int,
                        stream: int | None = None) -> None:
        """Enqueue octpt_variance_device on raw device pointers: guides {normal, depth}."""
        b = _lib.AovBuffers(**{k: C.c_void_p(int(v)) for k, v in guides.items() if v})
        self._check(self._lib.octpt_variance_device(self._ctx, C.byref(params), C.c_void_p(d_moments),
                                                    C.c_void_p(d_length), C.byref(b), C.c_void_p(d_out),
                                                    C.c_void_p(stream) if stream else None))

    def denoise_variance(self, color: np.ndarray, variance: np.ndarray, aov: dict, iterations: int = 5,
                         sigma_luminance: float = 4.0, luminance_floor: float = LUMINANCE_FLOOR,
                         sigma_normal: float = 0.3, sigma_depth: float = 0.1, demodulate: bool = True):
        """The variance-guided a-trous filter (octpt_denoise_variance) of a [H, W, 4] frame and its [H, W]
        variance (variance()'s), guided by render_aov's normal and depth (and albedo with demodulate) ->
        (filtered frame, filtered variance)."""
        color = np.ascontiguousarray(color, np.float32)
        H, W = color.shape[:2]
        variance = np.ascontiguousarray(variance, np.float32)
        if variance.size != W * H:
            raise ValueError(f"variance does not match the {W} x {H} frame")
        keep = []
        b = self._guides(aov, ("normal", "depth") + (("albedo",) if demodulate else ()), W, H, keep)
        p = _lib.DenoiseVarianceParams(W, H, iterations, sigma_luminance, luminance_floor, sigma_normal, sigma_depth,
                                       _lib.DENOISE_DEMODULATE if demodulate else 0)
        out, out_var = np.empty_like(color), np.empty((H, W), np.float32)
        self._check(self._lib.octpt_denoise_variance(self._ctx, C.byref(p), color.ctypes.data_as(C.c_void_p),
                                                     variance.ctypes.data_as(C.c_void_p), C.byref(b),
                                                     out.ctypes.data_as(C.c_void_p), out_var.ctypes.data_as(C.c_void_p)))
        return out, out_var

    def denoise_variance_device(self, params: "_lib.DenoiseVarianceParams", d_color: int, d_variance: int, guides: dict,
                                d_out: int, d_out_variance: int | None = None, stream: int | None = None) -> None:
        """Enqueue octpt_denoise_variance_device on raw device pointers (d_out may equal d_color, d_out_variance
        d_variance or None)."""
        b = _lib.AovBuffers(**{k: C.c_void_p(int(v)) for k, v in guides.items() if v})
        self._check(self._lib.octpt_denoise_variance_device(
            self._ctx, C.byref(params), C.c_void_p(d_color), C.c_void_p(d_variance), C.byref(b), C.c_void_p(d_out),
            C.c_void_p(d_out_variance) if d_out_variance else None, C.c_void_p(stream) if stream else None))

    # ------------------------------------------------------------ adaptive sampling (C30-C32)
    def render_tiles_device(self, params: "_lib.RenderParams", tiles, d_accum: int, d_moments: int | None = None,
                            d_seg_count: int | None = None, stream: int | None = None) -> None:
        """Enqueue octpt_render_tiles_device on raw device pointers: params.spp_count more samples into the listed
        frame tiles only (tiles: distinct indices t = ty * ceil(W / 8) + tx in any order, a host sequence; None =
        every tile).  d_moments: the samples' luminance moments, 2 floats / pixel (C31)."""
        t = None if tiles is None else np.ascontiguousarray(tiles, np.uint32).reshape(-1)
        # an empty list is still a list (nothing is rendered): a pointer that is not NULL, never read
        ptr = None if t is None else (t.ctypes.data_as(C.c_void_p) if len(t) else C.cast(C.pointer(C.c_uint32(0)), C.c_void_p))
        self._check(self._lib.octpt_render_tiles_device(
            self._ctx, C.byref(params), ptr, 0 if t is None else len(t), C.c_void_p(d_accum),
            C.c_void_p(d_moments) if d_moments else None, C.c_void_p(d_seg_count) if d_seg_count else None,
            C.c_void_p(stream) if stream else None))

    def render_tiles(self, settings: RenderSettings, tiles=None, accum: np.ndarray | None = None,
                     moments: np.ndarray | None = None, seg_count: np.ndarray | None = None, spp_start: int = 0):
        """settings.spp more samples into the listed tiles of host frames (render_tiles_device through torch
        buffers on this renderer's GPU): accum [H, W, 4] (black when None), moments [H, W, 2] and seg_count [H, W]
        u32 (zeros when None), each holding spp_start samples.  Returns (accum, moments, seg_count); pixels of
        unlisted tiles come back as they went in."""
        import torch

        W, H = settings.width, settings.height
        if accum is None:
            accum = np.zeros((H, W, 4), np.float32)
            accum[..., 3] = 1.0
        host = [np.ascontiguousarray(accum, np.float32).reshape(H, W, 4),
                np.ascontiguousarray(np.zeros((H, W, 2)) if moments is None else moments, np.float32).reshape(H, W, 2),
                np.ascontiguousarray(np.zeros((H, W)) if seg_count is None else seg_count, np.uint32).reshape(H, W)]
        dev = torch.device("cuda", self._device)
        d_acc, d_mom = (torch.from_numpy(a).to(dev) for a in host[:2])
        d_seg = torch.from_numpy(host[2].view(np.int32)).to(dev)
        self.max_depth = settings.max_depth
        self.seed = settings.seed
        p = self.params(W, H, spp_start, settings.spp)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            self.render_tiles_device(p, tiles, d_acc.data_ptr(), d_mom.data_ptr(), d_seg.data_ptr(), stream)
            torch.cuda.synchronize()
        return d_acc.cpu().numpy(), d_mom.cpu().numpy(), d_seg.cpu().numpy().view(np.uint32)

    def tile_error(self, moments: np.ndarray, tile_spp: np.ndarray, luminance_floor: float = LUMINANCE_FLOOR) -> np.ndarray:
        """The per-tile error (octpt_tile_error) of a [H, W, 2] moments frame whose tile t holds tile_spp[t]
        samples per pixel: the standard error of the tile's mean luminance relative to it, one float per 8x8 tile
        in frame tile order, +inf below 2 samples."""
        m = np.ascontiguousarray(moments, np.float32)
        H, W = m.shape[:2]
        T = tile_count(W, H)
        n = np.ascontiguousarray(tile_spp, np.uint32).reshape(-1)
        if m.shape != (H, W, 2) or n.size != T:
            raise ValueError(f"moments must be [H, W, 2] and tile_spp hold one entry per tile ({T})")
        p = _lib.TileErrorParams(W, H, luminance_floor)
        err = np.empty(T, np.float32)
        self._check(self._lib.octpt_tile_error(self._ctx, C.byref(p), m.ctypes.data_as(C.c_void_p),
                                               n.ctypes.data_as(C.c_void_p), err.ctypes.data_as(C.c_void_p)))
        return err

    def tile_error_device(self, params: "_lib.TileErrorParams", d_moments: int, d_tile_spp: int, d_error: int,
                          stream: int | None = None) -> None:
        """Enqueue octpt_tile_error_device on raw device pointers."""
        self._check(self._lib.octpt_tile_error_device(self._ctx, C.byref(params), C.c_void_p(d_moments),
                                                      C.c_void_p(d_tile_spp), C.c_void_p(d_error),
                                                      C.c_void_p(stream) if stream else None))

    def render_adaptive(self, settings: RenderSettings, min_spp: int, step_spp: int, threshold: float,
                        luminance_floor: float = LUMINANCE_FLOOR, with_rgba: bool = False,
                        neighbour_weight: float = 0.0):
        """Render until every 8x8 tile's error (tile_error) is at most `threshold`, or settings.spp samples per
        pixel are reached (octpt_render_adaptive): min_spp samples everywhere, then rounds of step_spp into the
        tiles still above the threshold.  neighbour_weight > 0 (octpt_render_adaptive_ex): the seam rule -- a tile
        goes on while a neighbour's error times the weight is above the threshold (tile_error_spread).  Returns
        (accum [H, W, 4], moments [H, W, 2], tile_spp u32 per tile, result dict: rounds, tile_samples,
        converged_tiles, total_tiles -- and "rgba" with with_rgba)."""
        W, H = settings.width, settings.height
        accum = np.empty((H, W, 4), np.float32)
        moments = np.empty((H, W, 2), np.float32)
        tile_spp = np.zeros(tile_count(W, H), np.uint32)
        rgba = np.zeros((H, W, 4), np.uint8) if with_rgba else None
        self.max_depth = settings.max_depth
        self.seed = settings.seed
        p = self.params(W, H, 0, settings.spp)
        if neighbour_weight == 0:
            entry, a = self._lib.octpt_render_adaptive, _lib.AdaptiveParams(min_spp, step_spp, threshold, luminance_floor)
        else:
            entry = self._lib.octpt_render_adaptive_ex
            a = _lib.AdaptiveParamsEx(min_spp, step_spp, threshold, luminance_floor, neighbour_weight)
        res = _lib.AdaptiveResult()
        self._check(entry(
            self._ctx, C.byref(p), C.byref(a), accum.ctypes.data_as(C.c_void_p), moments.ctypes.data_as(C.c_void_p),
            tile_spp.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.c_void_p) if rgba is not None else None,
            C.byref(res)))
        result = res.as_dict()
        if rgba is not None:
            result["rgba"] = rgba
        return accum, moments, tile_spp, result

    def render_adaptive_device(self, params: "_lib.RenderParams", adaptive: "_lib.AdaptiveParams", d_accum: int,
                               d_moments: int, d_seg_count: int | None = None, stream: int | None = None):
        """octpt_render_adaptive_device on raw device pointers (params.spp_count is the per-pixel cap); returns
        (tile_spp, result dict).  The call drains `stream` once per round."""
        tile_spp = np.zeros(tile_count(params.width, params.height), np.uint32)
        res = _lib.AdaptiveResult()
        self._check(self._lib.octpt_render_adaptive_device(
            self._ctx, C.byref(params), C.byref(adaptive), C.c_void_p(d_accum), C.c_void_p(d_moments),
            C.c_void_p(d_seg_count) if d_seg_count else None, tile_spp.ctypes.data_as(C.c_void_p), C.byref(res),
            C.c_void_p(stream) if stream else None))
        return tile_spp, res.as_dict()

    # ------------------------------------------------------------ emitter sampling (C38)
    def set_emitter_sampling(self, strategy: int, grid_size: int = 8, intensity: float = 1.0,
                             models: bool = False) -> None:
        """Scene::emitter_sampling_strategy and emmitter_intensity (octpt_set_emitter_sampling): _lib.EMITTERS_NONE or
        _lib.EMITTERS_ONE, the emitter grid's cell side in voxels and the intensity, for every later render.  With
        ONE and a block-value scene this GPU builds the emitter grid (emitter_grid).  models: emissive block models
        (torches, lanterns) are emitters too (_lib.EMITTERS_MODELS; emitter_models)."""
        p = _lib.EmitterParams(int(strategy), int(grid_size), float(intensity))
        p.flags = _lib.EMITTERS_MODELS if models else 0
        self._check(self._lib.octpt_set_emitter_sampling(self._ctx, C.byref(p)))

    def emitter_models(self) -> dict:
        """The emissive-model table this GPU holds beside a grid built with models=True (octpt_emitter_models), as
        scene.emitter_model_table returns the host's."""
        from .scene import take_emitter_models

        return take_emitter_models(lambda t: self._check(self._lib.octpt_emitter_models(self._ctx, C.byref(t))))

    def emitter_grid(self) -> dict:
        """The emitter grid this GPU built (octpt_emitter_grid), as scene.build_emitter_grid returns the host's."""
        from .scene import take_emitter_grid

        return take_emitter_grid(lambda g: self._check(self._lib.octpt_emitter_grid(self._ctx, C.byref(g))))

    # ------------------------------------------------------------ final-quality adaptive frames (C33-C36)
    def set_sample_clamp(self, max_luminance: float) -> None:
        """Clamp every sample's luminance to max_luminance in resolve (octpt_set_sample_clamp), for every later
        wavefront render of this renderer; 0 or +inf switch the clamp off."""
        self._check(self._lib.octpt_set_sample_clamp(self._ctx, max_luminance))

    def tile_error_spread(self, error: np.ndarray, W: int, H: int, neighbour_weight: float) -> np.ndarray:
        """The seam rule (octpt_tile_error_spread): each tile's error raised to neighbour_weight times the largest
        error among its up to eight neighbours in the W x H frame's tile grid."""
        e = np.ascontiguousarray(error, np.float32).reshape(-1)
        if e.size != tile_count(W, H):
            raise ValueError(f"error must hold one entry per tile ({tile_count(W, H)})")
        out = np.empty_like(e)
        self._check(self._lib.octpt_tile_error_spread(self._ctx, W, H, neighbour_weight, e.ctypes.data_as(C.c_void_p),
                                                      out.ctypes.data_as(C.c_void_p)))
        return out

    def tile_error_spread_device(self, W: int, H: int, neighbour_weight: float, d_error: int, d_out: int,
                                 stream: int | None = None) -> None:
        """Enqueue octpt_tile_error_spread_device on raw device pointers (d_out must not be d_error)."""
        self._check(self._lib.octpt_tile_error_spread_device(self._ctx, W, H, neighbour_weight, C.c_void_p(d_error),
                                                             C.c_void_p(d_out), C.c_void_p(stream) if stream else None))

    def sample_variance(self, moments: np.ndarray, tile_spp: np.ndarray, aov: dict, demodulate: bool = True) -> np.ndarray:
        """The variance [H, W] of each pixel's mean luminance (octpt_sample_variance) from the sample moments
        [H, W, 2] of a render whose tile t holds tile_spp[t] samples per pixel, with render_aov's depth (and albedo
        with demodulate, which moves it into the signal denoise_variance filters): what denoise_variance takes."""
        m = np.ascontiguousarray(moments, np.float32)
        H, W = m.shape[:2]
        n = np.ascontiguousarray(tile_spp, np.uint32).reshape(-1)
        if m.shape != (H, W, 2) or n.size != tile_count(W, H):
            raise ValueError(f"moments must be [H, W, 2] and tile_spp hold one entry per tile ({tile_count(W, H)})")
        keep = []
        b = self._guides(aov, ("depth",) + (("albedo",) if demodulate else ()), W, H, keep)
        p = _lib.SampleVarianceParams(W, H, _lib.DENOISE_DEMODULATE if demodulate else 0)
        out = np.empty((H, W), np.float32)
        self._check(self._lib.octpt_sample_variance(self._ctx, C.byref(p), m.ctypes.data_as(C.c_void_p),
                                                    n.ctypes.data_as(C.c_void_p), C.byref(b),
                                                    out.ctypes.data_as(C.c_void_p)))
        return out

    def sample_variance_device(self, params: "_lib.SampleVarianceParams", d_moments: int, d_tile_spp: int, guides: dict,
                               d_out: int, stream: int | None = None) -> None:
        """Enqueue octpt_sample_variance_device on raw device pointers: guides {depth, albedo}."""
        b = _lib.AovBuffers(**{k: C.c_void_p(int(v)) for k, v in guides.items() if v})
        self._check(self._lib.octpt_sample_variance_device(self._ctx, C.byref(params), C.c_void_p(d_moments),
                                                           C.c_void_p(d_tile_spp), C.byref(b), C.c_void_p(d_out),
                                                           C.c_void_p(stream) if stream else None))

    def render_adaptive_ex_device(self, params: "_lib.RenderParams", adaptive: "_lib.AdaptiveParamsEx", d_accum: int,
                                  d_moments: int, d_seg_count: int | None = None, stream: int | None = None):
        """octpt_render_adaptive_ex_device on raw device pointers: render_adaptive_device with the seam rule's
        neighbour weight; returns (tile_spp, result dict)."""
        tile_spp = np.zeros(tile_count(params.width, params.height), np.uint32)
        res = _lib.AdaptiveResult()
        self._check(self._lib.octpt_render_adaptive_ex_device(
            self._ctx, C.byref(params), C.byref(adaptive), C.c_void_p(d_accum), C.c_void_p(d_moments),
            C.c_void_p(d_seg_count) if d_seg_count else None, tile_spp.ctypes.data_as(C.c_void_p), C.byref(res),
            C.c_void_p(stream) if stream else None))
        return tile_spp, res.as_dict()

    def render_final(self, settings: RenderSettings, min_spp: int, step_spp: int, threshold: float,
                     neighbour_weight: float = 0.5, luminance_floor: float = LUMINANCE_FLOOR, iterations: int = 5,
                     sigma_luminance: float = 4.0, sigma_normal: float = 0.3, sigma_depth: float = 0.1,
                     demodulate: bool = True, with_rgba: bool = False):
        """A finished frame (octpt_render_final): render_adaptive with the seam rule, the guide buffers, the variance
        of the pixel means (sample_variance) and the variance-guided filter (denoise_variance) in one call.  Returns
        a dict: out [H, W, 4] (filtered), out_variance [H, W], accum and moments (unfiltered), tile_spp, result -- and
        rgba (the tone map of out) with with_rgba.  The clamp of set_sample_clamp applies."""
        W, H = settings.width, settings.height
        r = {"accum": np.empty((H, W, 4), np.float32), "moments": np.empty((H, W, 2), np.float32),
             "out": np.empty((H, W, 4), np.float32), "out_variance": np.empty((H, W), np.float32),
             "tile_spp": np.zeros(tile_count(W, H), np.uint32)}
        if with_rgba:
            r["rgba"] = np.zeros((H, W, 4), np.uint8)
        self.max_depth = settings.max_depth
        self.seed = settings.seed
        p = self.params(W, H, 0, settings.spp)
        f = _lib.FinalParams(
            _lib.AdaptiveParamsEx(min_spp, step_spp, threshold, luminance_floor, neighbour_weight),
            _lib.DenoiseVarianceParams(W, H, iterations, sigma_luminance, luminance_floor, sigma_normal, sigma_depth,
                                       _lib.DENOISE_DEMODULATE if demodulate else 0))
        res = _lib.AdaptiveResult()
        P = lambda k: r[k].ctypes.data_as(C.c_void_p) if k in r else None  # noqa: E731
        self._check(self._lib.octpt_render_final(self._ctx, C.byref(p), C.byref(f), P("accum"), P("moments"), P("out"),
                                                 P("out_variance"), P("tile_spp"), P("rgba"), C.byref(res)))
        r["result"] = res.as_dict()
        return r

    def render_final_device(self, params: "_lib.RenderParams", final: "_lib.FinalParams", d_accum: int, d_moments: int,
                            d_out: int, d_out_variance: int | None = None, stream: int | None = None):
        """octpt_render_final_device on raw device pointers (d_out must not be d_accum); returns (tile_spp, result
        dict).  The call drains `stream` once per adaptive round."""
        tile_spp = np.zeros(tile_count(params.width, params.height), np.uint32)
        res = _lib.AdaptiveResult()
        self._check(self._lib.octpt_render_final_device(
            self._ctx, C.byref(params), C.byref(final), C.c_void_p(d_accum), C.c_void_p(d_moments), C.c_void_p(d_out),
            C.c_void_p(d_out_variance) if d_out_variance else None, tile_spp.ctypes.data_as(C.c_void_p), C.byref(res),
            C.c_void_p(stream) if stream else None))
        return tile_spp, res.as_dict()

    def stats(self) -> dict:
        s = _lib.Stats()
        self._check(self._lib.octpt_get_stats(self._ctx, C.byref(s)))
        return s.as_dict()

    def reset_stats(self) -> None:
        self._check(self._lib.octpt_reset_stats(self._ctx))


def current_branch_count(current_spp: int, scene_branch_count: int) -> int:
    """TileRenderer::get_current_branch_count (tile_renderer.rs:196-206), f32 square root."""
    if current_spp < scene_branch_count:
        if current_spp <= int(np.sqrt(np.float32(scene_branch_count))):
            return 1
        return scene_branch_count - current_spp
    return scene_branch_count


def branch_pass_end(spp_start: int, spp_count: int, scene_branch_count: int) -> int:
    """The first pass boundary of the branch schedule at or after spp_start + spp_count (C20)."""
    spp = 0
    while spp < spp_start + spp_count:
        spp += current_branch_count(spp, scene_branch_count)
    return spp


def camera_rays(camera: Camera, W: int, H: int) -> np.ndarray:
    """octpt_camera_rays: Camera::get_ray at the pixel centres, [H, W, 6] f32 (host-only, no context)."""
    c = _lib.Camera((C.c_float * 3)(*camera.eye), (C.c_float * 3)(*camera.direction), (C.c_float * 3)(*camera.up),
                    camera.fov, 0.0, 0.0)
    rays = np.zeros((H, W, 6), np.float32)
    st = _lib.load().octpt_camera_rays(C.byref(c), W, H, rays.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise _lib.OctptError(st, "octpt_camera_rays")
    return rays


def lens_rays(camera: Camera, W: int, H: int, seed: int, sample: int) -> np.ndarray:
    """octpt_lens_rays: the first ray of sample `sample` of every pixel as a W x H render with this seed traces it
    (jittered; from its point of the lens when the camera has an aperture), [H, W, 6] f32 (host-only, no context)."""
    c = _lib.Camera((C.c_float * 3)(*camera.eye), (C.c_float * 3)(*camera.direction), (C.c_float * 3)(*camera.up),
                    camera.fov, camera.aperture, camera.focal_distance)
    rays = np.zeros((H, W, 6), np.float32)
    st = _lib.load().octpt_lens_rays(C.byref(c), W, H, seed, sample, rays.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise _lib.OctptError(st, "octpt_lens_rays")
    return rays


def frame_samples(W: int, H: int, sample: int) -> np.ndarray:
    """Rows (x, y, sample) for every pixel of a W x H frame in image order: projection_rays' xys for one sample."""
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.ravel(), ys.ravel(), np.full(W * H, sample)], 1).astype(np.uint32)


def projection_rays(camera: Camera, W: int, H: int, seed: int, xys, centre: bool = False):
    """octpt_projection_rays: for rows (x, y, sample) of `xys` the first rays [n, 6] f32 (origin, unit direction) that
    a W x H render with this seed traces under camera.projection, and the paths' RNG states after them [n] u32
    (host-only, no context).  centre: the un-jittered pixel-centre rays of the preview and the guide buffers."""
    xys = np.ascontiguousarray(xys, np.uint32).reshape(-1, 3)
    c = _c_camera(camera, lens=True)
    p = _lib.Projection(int(camera.projection[0]), float(camera.projection[1]))
    rays = np.zeros((len(xys), 6), np.float32)
    state = np.zeros(len(xys), np.uint32)
    st = _lib.load().octpt_projection_rays(C.byref(c), C.byref(p), W, H, seed, xys.ctypes.data_as(C.c_void_p), len(xys),
                                           _lib.PROJECTION_RAYS_CENTRE if centre else 0,
                                           rays.ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise _lib.OctptError(st, "octpt_projection_rays")
    return rays, state


def ray_source_rays(fallback: Camera, rays: np.ndarray, seed: int, xys):
    """octpt_ray_source_rays: for rows (x, y, sample) of `xys` the first rays [n, 6] f32 that a render under the ray
    list `rays` (H, W, R, 6) traces -- the record as given, or `fallback`'s central ray where it is invalid -- and the
    paths' RNG states after them [n] u32 (host-only, no context)."""
    rays = np.ascontiguousarray(rays, np.float32)
    if rays.ndim != 4 or rays.shape[3] != 6:
        raise ValueError(f"rays has shape {rays.shape}, not (H, W, R, 6)")
    H, W, R = rays.shape[:3]
    xys = np.ascontiguousarray(xys, np.uint32).reshape(-1, 3)
    out = np.zeros((len(xys), 6), np.float32)
    state = np.zeros(len(xys), np.uint32)
    st = _lib.load().octpt_ray_source_rays(C.byref(_c_camera(fallback, lens=True)), rays.ctypes.data_as(C.c_void_p), W, H,
                                           R, seed, xys.ctypes.data_as(C.c_void_p), len(xys),
                                           out.ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise _lib.OctptError(st, "octpt_ray_source_rays")
    return out, state


def _c_camera(camera: Camera, lens: bool = False) -> "_lib.Camera":
    # (the temporal entries take the camera without its lens: they refuse an aperture)
    return _lib.Camera((C.c_float * 3)(*camera.eye), (C.c_float * 3)(*camera.direction), (C.c_float * 3)(*camera.up),
                       camera.fov, camera.aperture if lens else 0.0, camera.focal_distance if lens else 0.0)


def reproject_coords(camera: Camera, prev_camera: Camera, W: int, H: int, depth: np.ndarray):
    """octpt_reproject_coords: where each pixel of `camera`'s W x H frame, at its `depth`, lay in prev_camera's
    frame -> (xy [H, W, 2] f32 in pixel units, pixel centre x <-> fx = x; depth [H, W] f32 from prev_camera's
    eye).  (NaN, NaN) and +inf where the depth is not finite or the point is not in front of prev_camera.  The
    temporal kernel's own mapping, bit for bit (host-only, no context)."""
    depth = np.ascontiguousarray(depth, np.float32)
    if depth.size != W * H:
        raise ValueError(f"depth holds {depth.size} pixels, not {W} x {H}")
    xy = np.zeros((H, W, 2), np.float32)
    zp = np.zeros((H, W), np.float32)
    st = _lib.load().octpt_reproject_coords(C.byref(_c_camera(camera)), C.byref(_c_camera(prev_camera)), W, H,
                                            depth.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p),
                                            zp.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise _lib.OctptError(st, "octpt_reproject_coords")
    return xy, zp


def tile_count(W: int, H: int) -> int:
    """8x8 tiles of a W x H frame (the entries of tile_spp and tile_error, C30-C32)."""
    return ((W + _lib.TILE - 1) // _lib.TILE) * ((H + _lib.TILE - 1) // _lib.TILE)


def shard_pixels(W: int, H: int, shard_index: int, shard_count: int) -> int:
    return int(_lib.load().octpt_shard_pixels(W, H, shard_index, shard_count))


def balance_tiles(W: int, H: int, shard_count: int, seg_count: np.ndarray) -> np.ndarray:
    """octpt_balance_tiles: a tile order that balances shard_count shards by a previous render's per-pixel
    segment counts (W * H, image order)."""
    seg = np.ascontiguousarray(seg_count, np.uint32).reshape(-1)
    if seg.size != W * H:
        raise ValueError(f"seg_count holds {seg.size} pixels, not {W} x {H}")
    T = ((W + 7) // 8) * ((H + 7) // 8)
    order = np.zeros(T, np.uint32)
    st = _lib.load().octpt_balance_tiles(W, H, shard_count, seg.ctypes.data_as(C.c_void_p),
                                         order.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise _lib.OctptError(st, "octpt_balance_tiles")
    return order
