"""The ray-list camera on the GPU: renders whose first rays the caller supplies.  octpt_lens_rays and
octpt_projection_rays publish the exact first ray of every sample under every other camera, so a list filled from
them must reproduce that camera's frame bit for bit -- through the seed, shade's first-launch rebuild and shade's
regeneration (a pool smaller than the chunk), under every general shade instance the scene selects and the emitter
shade.  Beside that: what the first ray decides alone (max_depth = 1), the guides and the preview on ray 0, invalid
records, the worked stereo panorama, and the refusals."""
import ctypes as C
import contextlib
import math
from dataclasses import replace

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd.rays import stereo_panorama_rays
from octree_pathtracing_amd.renderer import HipRenderer, frame_samples, lens_rays, projection_rays
from tests import emitter_ref as E
from tests import ray_source_ref as RS
from tests.adaptive_ref import tile_mask
from tests.test_gpu_beam import _renderer_with
from tests.test_gpu_parity import gpu_render, torch_cuda  # noqa: F401
from tests.test_gpu_projection import SHADE_VARIANTS, _camera, _marked_render, _projection, shade_variant
from tests.test_projection_cpu import ROOM_FRAME, inside_camera, outside_camera, room
from tests.test_ray_source_cpu import STEREO_IPD, invalid_records

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = ROOM_FRAME  # 40 x 24: partial tiles on both axes
W2, H2 = 33, 17               # odd on both axes
TWO_PI = float(np.float32(2.0 * math.pi))
MISS = 0xFFFFFFFF
UNSUPPORTED, INVALID_ARG, OK = _lib.ERR_UNSUPPORTED, _lib.ERR_INVALID_ARG, _lib.OK
NONE, ONE = 0, 1


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    """A renderer of this module's own: the ray source is a setting of the context."""
    r = HipRenderer(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def small_pool(torch_cuda):
    """100 path slots under chunks of two samples (tests/test_gpu_projection.py's): nine paths in ten are formed by
    shade's regeneration."""
    r = _renderer_with({"OCTPT_POOL": "100", "OCTPT_CHUNK": "2000"})
    yield r
    r.close()


@pytest.fixture(scope="module")
def tiny():
    """The 'tiny' config's spheres and cuboids (tests/test_gpu_parity.py, smoke()), at this module's frame."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config("tiny")
    return sc, cam, replace(rs, width=W, height=H, spp=SPP, max_depth=5, seed=SEED)


def camera_of(cam, kind):
    return {"pinhole": cam, "lens": cam.focus((16.0, 16.0, 16.0), 0.5), "parallel": cam.parallel(30.0),
            "fisheye": cam.fisheye(math.pi), "panoramic": cam.panoramic(TWO_PI)}[kind]


CAMERAS = ["pinhole", "lens", "parallel", "fisheye", "panoramic"]


def list_of(cam, R, w=W, h=H, seed=SEED, centre=False):
    """The list (h, w, R, 6) of the first rays of samples 0 .. R-1 under `cam`, as the library publishes them:
    octpt_lens_rays for the pinhole and the lens, octpt_projection_rays for the projections."""
    if cam.projection[0] == _lib.PROJECTION_PINHOLE and not centre:
        per = [lens_rays(cam, w, h, seed, s).reshape(h, w, 6) for s in range(R)]
    else:
        per = [projection_rays(cam, w, h, seed, frame_samples(w, h, s), centre=centre)[0].reshape(h, w, 6) for s in range(R)]
    return np.ascontiguousarray(np.stack(per, 2))


@contextlib.contextmanager
def source(r, base, rays):
    """`rays` as r's ray source over the plain camera `base` (its fallback), cleared afterwards."""
    r.set_camera(base)
    r.set_ray_source(rays)
    try:
        yield r
    finally:
        r.clear_ray_source()


def same_frame(got, want, counters=("paths", "segments")):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1], want[1])
    for k in counters:
        assert got[2][k] == want[2][k], k


# ------------------------------------------------------------------ 1: bit identity with every existing camera
@pytest.mark.parametrize("variant", SHADE_VARIANTS)
@pytest.mark.parametrize("kind", CAMERAS)
def test_list_of_a_camera_is_that_cameras_frame(torch_cuda, renderer, small_pool, tiny, kind, variant):
    """R = spp, the list filled from the camera's published rays: accum, seg_count and the paths and segments counters
    are the camera's, on the default pool (seed and first-launch rebuild) and on 100 path slots (regeneration), with
    and without sun sampling, with the material tables in LDS and too long for it."""
    from octree_pathtracing_amd import scene as S

    sc, base, rs = tiny
    sc = shade_variant(sc, variant, S.SunSamplingStrategy(**vars(S.STRATEGY_HIGH_QUALITY)))
    cam = camera_of(base, kind)
    want = gpu_render(torch_cuda, renderer, sc, cam, rs)
    assert np.all(np.isfinite(want[0])) and want[0][..., :3].max() > 0.0 and want[2]["paths"] == W * H * SPP
    rays = list_of(cam, SPP)
    assert RS.valid(rays).all()
    small_pool.set_scene(sc)
    for r in (renderer, small_pool):
        with source(r, base, rays):
            got = gpu_render(torch_cuda, r, sc, base, rs, upload=False)
        same_frame(got, want)
        assert got[2]["beam_restarts"] == 0  # beam starts are off under a source
    if kind != "pinhole":  # and the frame is the list's, not the fallback camera's
        assert not np.array_equal(gpu_render(torch_cuda, renderer, sc, base, rs, upload=False)[0], want[0])


# ------------------------------------------------------------------ 2: split calls, and the render paths
def test_split_calls_and_render_paths_agree(torch_cuda, renderer, tiny):
    sc, base, rs = tiny
    rs = replace(rs, width=W2, height=H2)
    rays = list_of(base.fisheye(math.pi), 3, W2, H2)  # R = 3 under 4 spp: sample 3 wraps to record 0
    renderer.set_scene(sc)
    with source(renderer, base, rays):
        want = gpu_render(torch_cuda, renderer, sc, base, rs, upload=False)
        assert np.all(np.isfinite(want[0])) and want[0][..., :3].max() > 0.0
        # samples 0-1, then 2-3: the absolute sample index goes on through the list
        half = gpu_render(torch_cuda, renderer, sc, base, replace(rs, spp=2), upload=False)
        two = gpu_render(torch_cuda, renderer, sc, base, replace(rs, spp=2), spp_start=2, accum=half[0], upload=False)
        assert np.array_equal(two[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(half[1] + two[1], want[1])
        # the whole frame as a tile list, and a list of some tiles: the same on their tiles, the others untouched
        acc, _, segs = renderer.render_tiles(rs, tiles=None)
        assert np.array_equal(acc.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(segs, want[1])
        tiles = [0, 3, 7, 14]  # a 5 x 3 tile grid: corners of both partial edges among them
        m = tile_mask(W2, H2, tiles)
        acc, _, segs = renderer.render_tiles(rs, tiles=tiles)
        assert np.array_equal(acc[m].view(np.uint32), want[0][m].view(np.uint32)) and np.array_equal(segs[m], want[1][m])
        assert np.all(acc[~m] == (0.0, 0.0, 0.0, 1.0)) and np.all(segs[~m] == 0)
        # sync and async host frames
        host, _ = renderer.render(rs)
        assert np.array_equal(host.view(np.uint32), want[0].view(np.uint32))
        renderer.set_resolution((W2, H2))
        renderer.reset_render()
        renderer.max_depth, renderer.seed = rs.max_depth, rs.seed
        renderer.render_frame(rs.spp).wait_for()
        assert np.array_equal(renderer.get_float_image().reshape(H2, W2, 4).view(np.uint32), want[0].view(np.uint32))
    # the list with the wrap written out (R = 4) is the same frame
    with source(renderer, base, np.ascontiguousarray(rays[:, :, [0, 1, 2, 0]])):
        same_frame(gpu_render(torch_cuda, renderer, sc, base, rs, upload=False), want)


# ------------------------------------------------------------------ 3: the first ray decides at max_depth = 1
@pytest.mark.parametrize("pool", ["default", "small"])
def test_black_exactly_where_the_supplied_ray_hits(torch_cuda, renderer, small_pool, tiny, pool):
    sc, base, rs = tiny
    r = renderer if pool == "default" else small_pool
    r.set_scene(sc)
    rays = list_of(base.fisheye(math.pi), 1, centre=True)  # R = 1: every sample of a pixel traces this ray
    hit = (r.intersect(rays.reshape(-1, 6))[1] != MISS).reshape(H, W)
    assert 0.01 <= hit.mean() <= 0.99  # the frame has both, so the equality below says something
    with source(r, base, rays):
        for spp, start in ((1, 0), (SPP, 0), (2, 5)):
            acc, segs, st = gpu_render(torch_cuda, r, sc, base, replace(rs, spp=spp, max_depth=1), spp_start=start,
                                       upload=False)
            black = np.all(acc[..., :3] == 0.0, axis=-1)
            assert np.array_equal(black, hit), np.argwhere(black != hit)[:5]
            assert np.all(segs == spp) and st["paths"] == W * H * spp


# ------------------------------------------------------------------ 4: the guides and the preview follow ray 0
def test_guides_and_preview_follow_ray_0(torch_cuda, renderer):
    from octree_pathtracing_amd import scene as S

    sc = room()
    fish = outside_camera().fisheye(math.pi)
    base = outside_camera()
    rs = S.RenderSettings(width=W, height=H, spp=1, max_depth=5, seed=SEED)
    ray0 = list_of(fish, 1, centre=True)
    # records 1 and 2 look elsewhere: only record 0 may show in the guides
    rays = np.ascontiguousarray(np.concatenate([ray0, list_of(inside_camera().panoramic(TWO_PI), 2)], 2))
    renderer.set_scene(sc)
    t, prim, nrm, _ = renderer.intersect(ray0.reshape(-1, 6))
    t, prim, nrm = t.reshape(H, W), prim.reshape(H, W), nrm.reshape(H, W, 3)
    hit = prim != MISS
    assert hit.sum() >= 8 and (~hit).sum() >= 8
    # the fisheye camera's own preview traces the same rays
    want_prev = gpu_render(torch_cuda, renderer, sc, fish, rs, preview=True, upload=False)
    with source(renderer, base, rays):
        aov = renderer.render_aov(rs)
        prev = gpu_render(torch_cuda, renderer, sc, base, rs, preview=True, upload=False)
    assert np.array_equal(aov["prim"], prim)
    assert np.array_equal(aov["depth"].view(np.uint32), t.view(np.uint32))  # opaque stone: one segment, its t
    assert np.array_equal(aov["material"], np.where(hit, 1, 0).astype(np.uint32))
    assert np.array_equal(aov["normal"][..., :3][hit], nrm[hit])
    assert np.array_equal(prev[0].view(np.uint32), want_prev[0].view(np.uint32)) and np.array_equal(prev[1], want_prev[1])
    # the depth guide is the distance from the ray's own origin: the same directions from origins moved back along
    # them by 2 see the same surfaces 2 further away
    back = ray0.copy()
    back[..., :3] -= 2.0 * back[..., 3:]
    with source(renderer, base, back):
        far = renderer.render_aov(rs, which=("depth", "prim"))
    both = hit & (far["prim"] == prim)  # (a ray grazing an edge may round to the other side of it from the new origin)
    assert both.sum() >= 0.9 * hit.sum()
    # Coordinates and distances here lie below 64, where an f32 ulp is 3.8e-6.  The moved origin rounds once per
    # component, the two distances once each, their slab arithmetic a few times more at the same scale: 8 ulp bound it.
    assert np.abs(far["depth"][both] - (aov["depth"][both] + 2.0)).max() <= 8 * 3.8147e-6


def test_final_and_adaptive_follow(torch_cuda, renderer, tiny):
    from tests.test_gpu_final import final_composed, final_device
    from tests.test_gpu_adaptive import same

    sc, base, rs = tiny
    cam = base.panoramic(TWO_PI)
    renderer.set_scene(sc)
    with source(renderer, base, list_of(cam, SPP)):
        (ca, cm, co, cv), c_spp, c_res, _, _ = final_composed(torch_cuda, renderer, W, H, 0.05, True)
        (da, dm, do, dv), d_spp, d_res = final_device(torch_cuda, renderer, W, H, 0.05, True)
        assert same(da, ca) and same(dm, cm) and same(do, co) and same(dv, cv)
        assert np.array_equal(d_spp, c_spp) and d_res == c_res
        assert np.all(np.isfinite(do)) and do[..., :3].max() > 0.0
        # the adaptive driver's first round is the tile-list render of its samples: the list's frame
        acc = renderer.render_adaptive(replace(rs, spp=4), min_spp=4, step_spp=4, threshold=0.05)[0]
    want = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)  # R = spp = 4: the panoramic camera's frame
    assert np.array_equal(acc.view(np.uint32), want[0].view(np.uint32))


# ------------------------------------------------------------------ 5: emitter sampling
@pytest.mark.parametrize("variant", ["plain", "sun-long-tables"])
def test_emitter_sampling_follows_the_list(torch_cuda, renderer, small_pool, variant):
    """Strategy ONE (C38) in the room with its emitters under a list filled from the pinhole rays: the pinhole ONE
    frame bit for bit, through the emitter shade's ray-list instances with and without regeneration."""
    from octree_pathtracing_amd import scene as S

    sc = E.room_scene(second=True, hole="sun" in variant)
    sc = shade_variant(sc, variant, S.SunSamplingStrategy(True, False, False, True, False))
    sc.build_octree(E.DEPTH)
    rs = S.RenderSettings(width=W, height=H, spp=SPP, max_depth=3, seed=SEED)
    cam = inside_camera()
    rays = list_of(cam, SPP)
    both = (renderer, small_pool)
    try:
        for r in both:
            r.set_emitter_sampling(NONE)
            r.set_scene(sc)
        none = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        for r in both:
            r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
        want = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        assert np.all(np.isfinite(want[0])) and want[2]["segments"] > none[2]["segments"]  # the emitter segments
        for r in both:
            with source(r, outside_camera(), rays):  # (a fallback that looks elsewhere: it is not read)
                same_frame(gpu_render(torch_cuda, r, sc, outside_camera(), rs, upload=False), want)
    finally:
        for r in both:
            r.set_emitter_sampling(NONE)


# ------------------------------------------------------------------ 6: invalid records
def test_invalid_records_render_as_the_central_ray(torch_cuda, renderer, small_pool, tiny):
    sc, base, rs = tiny
    rays = list_of(base.fisheye(math.pi), SPP)
    rng = np.random.default_rng(5)
    flat = rays.reshape(-1, 6)
    bad = invalid_records()
    where = rng.choice(len(flat), len(flat) // 5, replace=False)
    for k, i in enumerate(where):
        flat[i] = bad[k % len(bad)]
    flat[:6] = bad[:6]  # ray 0 of the first pixels too (the preview and the guides)
    assert (~RS.valid(rays)).sum() >= len(where)
    fixed = RS.effective(base, rays)  # the same list with those records replaced on the host
    assert RS.valid(fixed).all()
    renderer.set_scene(sc)
    small_pool.set_scene(sc)
    one = replace(rs, spp=1)
    with source(renderer, base, fixed):
        want = gpu_render(torch_cuda, renderer, sc, base, rs, upload=False)
        want_prev = gpu_render(torch_cuda, renderer, sc, base, one, preview=True, upload=False)
        want_aov = renderer.render_aov(one)
    for r in (renderer, small_pool):
        with source(r, base, rays):
            got = gpu_render(torch_cuda, r, sc, base, rs, upload=False)
            same_frame(got, want)
            assert np.all(np.isfinite(got[0]))
            if r is renderer:
                prev = gpu_render(torch_cuda, r, sc, base, one, preview=True, upload=False)
                aov = r.render_aov(one)
    assert np.array_equal(prev[0].view(np.uint32), want_prev[0].view(np.uint32)) and np.all(np.isfinite(prev[0]))
    for k in want_aov:
        assert np.array_equal(aov[k].view(np.uint32), want_aov[k].view(np.uint32)), k
        assert not np.isnan(aov[k]).any() if aov[k].dtype == np.float32 else True


# ------------------------------------------------------------------ 7: the stereo panorama in the closed room
def test_stereo_panorama_in_the_closed_room(torch_cuda, renderer):
    from octree_pathtracing_amd import scene as S

    sc = room()
    cam = inside_camera()
    renderer.set_scene(sc)
    frames = {}
    for eye in ("left", "right"):
        rays = stereo_panorama_rays(cam, W, H, STEREO_IPD, eye)
        with source(renderer, cam, rays):
            # no sky at max_depth = 1: every ray of the list meets a wall (tests/test_ray_source_cpu.py checks the
            # list against the oracle first)
            acc, segs, _ = gpu_render(torch_cuda, renderer, sc, cam, S.RenderSettings(W, H, SPP, max_depth=1, seed=SEED),
                                      upload=False)
            assert np.all(acc[..., :3] == 0.0) and np.all(segs == SPP)
            frames[eye] = renderer.render_aov(S.RenderSettings(W, H, 1, max_depth=5, seed=SEED), which=("depth", "prim"))
    assert (frames["left"]["prim"] != MISS).all() and (frames["right"]["prim"] != MISS).all()
    assert not np.array_equal(frames["left"]["depth"], frames["right"]["depth"])  # two eyes, two views
    # an open room would not pass: through the hole in the ceiling the same lists see the sky
    open_room = E.room_scene(emitter=False, hole=True)
    open_room.build_octree(E.DEPTH)
    with source(renderer, cam, stereo_panorama_rays(cam, W, H, STEREO_IPD, "left")):
        acc, _, _ = gpu_render(torch_cuda, renderer, open_room, cam, S.RenderSettings(W, H, SPP, max_depth=1, seed=SEED))
    assert (acc[..., :3].max(-1) > 0.0).any()


# ------------------------------------------------------------------ 8: refusals; set then clear is never set
def _source(r):
    s = _lib.RaySource()
    assert r._lib.octpt_get_ray_source(r._ctx, C.byref(s)) == OK
    return s.d_rays, s.width, s.height, s.rays_per_pixel, tuple(s.reserved)


def _set(r, ptr, w=W, h=H, rpp=SPP, word=None):
    s = _lib.RaySource(ptr, w, h, rpp)
    if word is not None:
        s.reserved[word] = 1
    return r._lib.octpt_set_ray_source(r._ctx, C.byref(s))


def _status(call, *a, **kw):
    try:
        call(*a, **kw)
    except _lib.OctptError as e:
        return e.status
    return OK


def test_refusals(torch_cuda, tiny):
    sc, cam, rs = tiny
    torch = torch_cuda
    rays = list_of(cam.fisheye(math.pi), SPP)
    other = torch.from_numpy(list_of(cam.panoramic(TWO_PI), SPP)).cuda()
    with HipRenderer(device=0) as r:
        r.set_scene(sc)
        r.set_camera(cam)
        r.set_ray_source(rays)
        held, held_cam, held_proj = _source(r), _camera(r), _projection(r)
        assert held[0] and held[1:] == (W, H, SPP, (0,) * 5) and r.get_ray_source()[1:] == (W, H, SPP)
        want = _marked_render(torch, r, rs)
        # the setter: a held setting survives every refused call
        p = other.data_ptr()
        for word in range(5):
            assert _set(r, p, word=word) == INVALID_ARG
        for kw in (dict(rpp=0), dict(w=0), dict(h=0), dict(w=1 << 14, h=1 << 14, rpp=2), dict(w=1 << 31, h=2),
                   dict(rpp=0xFFFFFFFF, w=0xFFFFFFFF, h=0xFFFFFFFF)):
            assert _set(r, p, **kw) == INVALID_ARG, kw
        assert _source(r) == held
        # an aperture or a projection second: refused, the camera, the projection and the source stay
        lens = cam.focus((16.0, 16.0, 16.0), 0.5)
        c = _lib.Camera((C.c_float * 3)(*lens.eye), (C.c_float * 3)(*lens.direction), (C.c_float * 3)(*lens.up), lens.fov,
                        lens.aperture, lens.focal_distance)
        assert r._lib.octpt_set_camera(r._ctx, C.byref(c)) == UNSUPPORTED
        assert _status(r.set_camera, lens) == UNSUPPORTED
        for mode, param in ((1, 10.0), (2, 1.0), (3, TWO_PI)):
            pr = _lib.Projection(mode, param)
            assert r._lib.octpt_set_projection(r._ctx, C.byref(pr)) == UNSUPPORTED
            assert _status(r.set_camera, replace(cam, projection=(mode, param))) == UNSUPPORTED
        assert (_source(r), _camera(r), _projection(r)) == (held, held_cam, held_proj)
        # renders: another size, the megakernel -- into marked buffers, which stay marked
        n = W * H
        acc = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
        segs = torch.full((n,), 9, dtype=torch.int32, device="cuda")
        r.max_depth, r.seed = rs.max_depth, rs.seed
        for p_, st_ in ((r.params(W - 8, H, 0, SPP), INVALID_ARG), (r.params(W, H - 8, 0, SPP), INVALID_ARG),
                        (r.params(H, W, 0, SPP), INVALID_ARG), (r.params(W, H, 0, SPP, megakernel=True), UNSUPPORTED)):
            assert _status(r.render_device, p_, acc.data_ptr(), segs.data_ptr()) == st_
            assert _status(r.render_tiles_device, p_, None, acc.data_ptr()) == st_
        assert _status(r.render_device, r.params(W - 8, H, 0, 1, preview=True), acc.data_ptr(), segs.data_ptr()) == INVALID_ARG
        small = replace(rs, width=W - 8)
        assert _status(r.render, small) == INVALID_ARG and _status(r.render_aov, small) == INVALID_ARG
        assert _status(r.render_adaptive, small, 4, 4, 0.05) == INVALID_ARG
        torch.cuda.synchronize()
        assert (acc.cpu().numpy() == 7.0).all() and (segs.cpu().numpy() == 9).all()
        # the temporal passes and the context's reprojection refuse, their outputs untouched
        color = np.zeros((H, W, 4), np.float32)
        aov = {"normal": np.zeros((H, W, 4), np.float32), "depth": np.ones((H, W), np.float32),
               "prim": np.zeros((H, W), np.uint32), "albedo": np.ones((H, W, 4), np.float32)}
        g = _lib.AovBuffers(**{k: v.ctypes.data for k, v in aov.items()})
        c0 = _lib.Camera((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.direction), (C.c_float * 3)(*cam.up), cam.fov, 0.0, 0.0)
        tp = _lib.TemporalParams(W, H, c0, c0, 32, 0.1, 0.9, _lib.TEMPORAL_MATCH_PRIM)
        out = np.full((H, W, 4), 7.0, np.float32)
        length = np.full((H, W), 9, np.uint32)
        mom = np.full((H, W, 2), 5.0, np.float32)
        P_ = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert r._lib.octpt_temporal(r._ctx, C.byref(tp), P_(color), C.byref(g), None, P_(out), P_(length)) == UNSUPPORTED
        assert r._lib.octpt_temporal_moments(r._ctx, C.byref(tp), P_(color), C.byref(g), None, None, P_(out), P_(length),
                                             P_(mom)) == UNSUPPORTED
        xy, zp = np.full((H, W, 2), 7.0, np.float32), np.full((H, W), 9.0, np.float32)
        assert r._lib.octpt_reproject_coords_ctx(r._ctx, C.byref(c0), C.byref(c0), W, H, P_(aov["depth"]), P_(xy),
                                                 P_(zp)) == UNSUPPORTED
        assert _status(r.reproject_coords, cam, W, H, aov["depth"]) == UNSUPPORTED
        assert (out == 7.0).all() and (length == 9).all() and (mom == 5.0).all() and (xy == 7.0).all() and (zp == 9.0).all()
        # after all of them the held source renders the frame it rendered before
        got = _marked_render(torch, r, rs)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
        # cleared (NULL, or a source with NULL d_rays -- its other fields are not read): they all run again
        assert r._lib.octpt_set_ray_source(r._ctx, None) == OK and _source(r) == (None, 0, 0, 0, (0,) * 5)
        r.set_ray_source(rays)
        assert _set(r, None, w=0, rpp=0, word=2) == OK and _source(r)[0] is None
        assert r._lib.octpt_temporal(r._ctx, C.byref(tp), P_(color), C.byref(g), None, P_(out), P_(length)) == OK
        r.reproject_coords(cam, W, H, aov["depth"])
        r.render(small)
        # a source second: refused under an aperture and under a projection, the earlier setting stays
        r.set_camera(lens)
        assert _set(r, p) == UNSUPPORTED and _status(r.set_ray_source, other) == UNSUPPORTED
        r.set_camera(cam.fisheye(2.0))
        assert _set(r, p) == UNSUPPORTED and _status(r.set_ray_source, other) == UNSUPPORTED
        assert _source(r)[0] is None and _projection(r)[0] == _lib.PROJECTION_FISHEYE
        # the Python surface checks the tensor it is handed
        r.set_camera(cam)
        for bad in (np.zeros((H, W, 6), np.float32), np.zeros((H, W, 2, 5), np.float32), other.double(), other.cpu(),
                    other[:, ::2]):
            with pytest.raises(ValueError):
                r.set_ray_source(bad)
        with pytest.raises(ValueError):
            r.set_ray_source(rays, rays_per_pixel=SPP + 1)
        assert _source(r)[0] is None
    # a multi-device context has no one device for the buffer
    with HipRenderer(devices=[0, 0]) as m:
        assert _set(m, other.data_ptr()) == UNSUPPORTED and _source(m)[0] is None


def test_set_then_clear_is_never_set(torch_cuda, tiny):
    sc, cam, rs = tiny
    with HipRenderer(device=0) as fresh:  # octpt_set_ray_source is never called on this context
        never = gpu_render(torch_cuda, fresh, sc, cam, rs)
        never_prev = gpu_render(torch_cuda, fresh, sc, cam, rs, preview=True)
        never_aov = fresh.render_aov(rs)
    with HipRenderer(device=0) as r:
        r.set_scene(sc)
        with source(r, cam, list_of(cam.fisheye(math.pi), SPP)):
            other = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
        back = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
        back_prev = gpu_render(torch_cuda, r, sc, cam, rs, preview=True, upload=False)
        back_aov = r.render_aov(rs)
        mk = gpu_render(torch_cuda, r, sc, cam, rs, megakernel=True, upload=False)  # and the megakernel runs again
    same_frame(back, never, ("paths", "segments", "esvo_steps", "shade_events"))
    assert np.array_equal(back_prev[0].view(np.uint32), never_prev[0].view(np.uint32))
    for k in never_aov:
        assert np.array_equal(back_aov[k].view(np.uint32), never_aov[k].view(np.uint32)), k
    assert np.array_equal(mk[1], never[1])
    assert not np.array_equal(other[0], never[0])
