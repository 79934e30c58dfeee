"""The sky on the GPU.  The device lookup is the host's bit for bit; a cleared sky leaves no trace;
the sky instances are the existing code plus the lookup (COLOR (0.5, 0.7, 1.0) renders the DEFAULT frame's bits under
every camera form, with sun sampling and with emitter sampling); a map of equal texels is COLOR; a panorama of an empty
world is the map; every sample goes through the lookup; the scale reaches every bounce; bounce directions have the
right sign; every render form agrees; the guide buffers; the refusals; and the smallest maps."""
import ctypes as C
import math

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd.renderer import HipRenderer, frame_samples, projection_rays
from octree_pathtracing_amd.scene import Sky
from tests import emitter_ref as E
from tests import sky_ref as R
from tests.test_gpu_parity import gpu_render, torch_cuda  # noqa: F401
from tests.test_sky_cpu import YAWS, c_sky, lookup_bound, rgba, sample_map

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, SPP, SEED = 32, 16, 4, 11  # the frame of the panorama is the map's size (W = 2H)
TWO_PI = float(F32(2.0 * math.pi))
MISS = 0xFFFFFFFF
DEFAULT_RGB = (0.5, 0.7, 1.0)
NONE, ONE = 0, 1


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    """A renderer of this module's own: the sky is a setting of the context."""
    r = HipRenderer(device=0)
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    assert np.array_equal(bits(got[0]), bits(want[0]))
    assert np.array_equal(got[1], want[1])


def settings(w=W, h=H, spp=SPP, depth=5):
    from octree_pathtracing_amd import scene as S

    return S.RenderSettings(width=w, height=h, spp=spp, max_depth=depth, seed=SEED)


def tiny_scene():
    """The 'tiny' config's spheres and cuboids (smoke()'s scene) and its camera."""
    from octree_pathtracing_amd import scene as S

    sc, cam, _ = S.make_config("tiny")
    return sc, cam


def block_scene(cells, sun=False):
    """A block-value world of tests/emitter_ref.py's block table; sun=False: the sun's texture and diffuse term off."""
    from octree_pathtracing_amd import scene as S

    sc = E.make_scene(cells)
    sc.textures = [S.Texture(), S.Texture(rgba=(200, 200, 200, 255)), S.Texture(rgba=(255, 255, 255, 255))]
    sc.materials[1].texture_index, sc.materials[2].texture_index = 1, 2
    if not sun:
        sc.strategy = S.SunSamplingStrategy(**vars(S.STRATEGY_NON_LUMINOUS))
        sc.sun = S.Sun(draw_texture=False)
    sc.build_octree(E.DEPTH)
    return sc


def open_room(sun=False, emitters=False):
    """tests/emitter_ref.py's stone room with its ceiling open to the sky."""
    from octree_pathtracing_amd import scene as S

    sc = E.room_scene(emitter=emitters, second=emitters, hole=True)
    if not sun:
        sc.strategy = S.SunSamplingStrategy(**vars(S.STRATEGY_NON_LUMINOUS))
        sc.sun = S.Sun(draw_texture=False)
    sc.build_octree(E.DEPTH)
    return sc


def empty_world():
    """As empty as a scene gets: one stone cell in the corner of the 32^3 world, the eye at the centre."""
    from octree_pathtracing_amd import scene as S

    return block_scene([(0, 0, 0, E.STONE)]), S.Camera(eye=(16.0, 16.0, 16.0), direction=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))


# ------------------------------------------------------------------ device against host
def test_device_lookup_is_the_hosts(renderer):
    dirs = R.direction_set(W, H)
    t = sample_map()
    skies = [Sky(), Sky.color((0.3, 1.7, 0.05), 2.5), Sky.gradient((0.9, 0.8, 0.7), (0.1, 0.3, 1.5), 0.5)]
    skies += [Sky.map(t, yaw=y, scale=1.5) for y in YAWS] + [Sky.map(sample_map(8, 4), yaw=0.3)]
    try:
        for sky in skies:
            renderer.set_sky(sky)
            assert np.array_equal(bits(renderer.sky_radiance(dirs)), bits(sky.radiance(dirs))), sky.mode
    finally:
        renderer.clear_sky()
    assert np.array_equal(renderer.sky_radiance(dirs), np.broadcast_to(np.asarray(DEFAULT_RGB, F32), dirs.shape))


def test_device_map_tensor_is_copied(torch_cuda, renderer):
    """octpt_set_sky_device: a tensor on the device is copied and sanitised; the caller may overwrite its own."""
    dirs = R.direction_set(8, 4, n_random=100)
    t = sample_map(8, 4)
    t[1, 2] = (np.nan, -1.0, np.inf)
    d = torch_cuda.as_tensor(rgba(t), device="cuda")
    try:
        renderer.set_sky(Sky.map(d, yaw=0.4))
        d.zero_()
        torch_cuda.cuda.synchronize()
        got = renderer.sky_radiance(dirs)
    finally:
        renderer.clear_sky()
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(Sky.map(t, yaw=0.4).radiance(dirs)))


# ------------------------------------------------------------------ nothing changes by default
@pytest.mark.parametrize("world", ["spheres", "blocks"])
def test_a_cleared_sky_leaves_no_trace(torch_cuda, world):
    sc, cam = tiny_scene() if world == "spheres" else (open_room(sun=True), E.room_camera())
    rs = settings(40, 24)
    with HipRenderer(device=0) as fresh:
        want = gpu_render(torch_cuda, fresh, sc, cam, rs)
        want_prev = gpu_render(torch_cuda, fresh, sc, cam, rs, preview=True, upload=False)
    with HipRenderer(device=0) as r:
        r.set_sky(Sky.map(sample_map(), yaw=0.5, scale=2.0))
        other = gpu_render(torch_cuda, r, sc, cam, rs)
        r.clear_sky()
        got = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
        got_prev = gpu_render(torch_cuda, r, sc, cam, rs, preview=True, upload=False)
    assert want[0][..., :3].max() > 0.0 and not np.array_equal(other[0], want[0])
    same(got, want)
    same(got_prev, want_prev)
    for k in ("paths", "segments", "esvo_steps", "shade_events"):
        assert got[2][k] == want[2][k], k


# ------------------------------------------------------------------ the sky instances are the existing code plus the lookup
def _default_colour():
    return Sky.color(DEFAULT_RGB, 1.0)


@pytest.mark.parametrize("camera", ["pinhole", "lens", "fisheye", "rays"])
@pytest.mark.parametrize("sun", [False, True], ids=["plain", "sun-sampling"])
def test_default_colour_renders_the_default_frame(torch_cuda, renderer, camera, sun):
    from octree_pathtracing_amd import scene as S

    sc, base = tiny_scene()
    if sun:
        sc.strategy = S.SunSamplingStrategy(**vars(S.STRATEGY_HIGH_QUALITY))
    rs = settings(40, 24)
    cam = {"pinhole": base, "lens": base.focus((16.0, 16.0, 16.0), 0.5), "fisheye": base.fisheye(math.pi), "rays": base}[camera]
    renderer.set_scene(sc)
    try:
        if camera == "rays":  # a list of the fisheye's first rays over the plain camera
            fish = base.fisheye(math.pi)
            per = [projection_rays(fish, 40, 24, SEED, frame_samples(40, 24, s))[0].reshape(24, 40, 6) for s in range(SPP)]
            renderer.set_camera(base)
            renderer.set_ray_source(np.ascontiguousarray(np.stack(per, 2)))
        want = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        want_prev = gpu_render(torch_cuda, renderer, sc, cam, rs, preview=True, upload=False)
        renderer.set_sky(_default_colour())
        got = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        got_prev = gpu_render(torch_cuda, renderer, sc, cam, rs, preview=True, upload=False)
        renderer.set_sky(Sky.color((0.1, 0.9, 0.2), 1.0))
        other = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
    finally:
        renderer.clear_sky()
        renderer.clear_ray_source()
    assert np.isfinite(want[0]).all() and want[0][..., :3].max() > 0.0
    same(got, want)
    same(got_prev, want_prev)
    for k in ("paths", "segments", "shade_events"):
        assert got[2][k] == want[2][k], k
    # the geometry is the same under every sky, the colour is not
    assert np.array_equal(other[1], want[1]) and not np.array_equal(other[0], want[0])


@pytest.mark.parametrize("sun", [False, True], ids=["plain", "sun-sampling"])
def test_default_colour_under_emitter_sampling(torch_cuda, renderer, sun):
    from octree_pathtracing_amd import scene as S

    sc = open_room(sun=True, emitters=True)
    if sun:
        sc.strategy = S.SunSamplingStrategy(True, False, False, True, False)
        sc.build_octree(E.DEPTH)
    rs, cam = settings(16, 16, depth=3), E.room_camera()
    try:
        renderer.set_emitter_sampling(NONE)
        renderer.set_scene(sc)
        none = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        renderer.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
        want = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        assert want[2]["segments"] > none[2]["segments"]  # the emitter segments are traced
        renderer.set_sky(_default_colour())
        got = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        renderer.set_sky(Sky.color(DEFAULT_RGB, 3.0))
        brighter = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
    finally:
        renderer.clear_sky()
        renderer.set_emitter_sampling(NONE)
    same(got, want)
    assert got[2]["segments"] == want[2]["segments"]
    assert np.array_equal(brighter[1], want[1]) and brighter[0][..., :3].sum() > want[0][..., :3].sum()  # the sky is seen


# ------------------------------------------------------------------ a uniform map is COLOR
@pytest.mark.parametrize("size", [(32, 16), (1, 1), (2, 1)])
def test_uniform_map_is_color(torch_cuda, renderer, size):
    """... and the 1 x 1 and 2 x 1 maps render: the smallest shapes at which wrap and clamp can go wrong."""
    w, h = size
    texel = (0.37, 1.5, 0.02)
    sc, cam = tiny_scene()
    rs = settings(40, 24)
    renderer.set_scene(sc)
    try:
        renderer.set_sky(Sky.color(texel, 2.0))
        want = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        want_prev = gpu_render(torch_cuda, renderer, sc, cam, rs, preview=True, upload=False)
        renderer.set_sky(Sky.map(np.broadcast_to(np.asarray(texel, F32), (h, w, 3)), yaw=0.3, scale=2.0))
        got = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        got_prev = gpu_render(torch_cuda, renderer, sc, cam, rs, preview=True, upload=False)
        if (w, h) == (2, 1):  # two different texels: finite, and between them
            renderer.set_sky(Sky.map(np.asarray([[(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)]], F32)))
            two = gpu_render(torch_cuda, renderer, sc, cam, settings(40, 24, depth=1), upload=False)
            assert np.isfinite(two[0]).all() and two[0][..., :3].min() >= 0.0 and two[0][..., :3].max() <= 1.0
            assert 0.0 < two[0][..., :3].max()
    finally:
        renderer.clear_sky()
    assert want[0][..., :3].max() > 0.0
    same(got, want)
    same(got_prev, want_prev)


# ------------------------------------------------------------------ the panorama is the map
def _miss_mask(r, rays):
    return r.intersect(rays)[1] == MISS


def test_panorama_of_an_empty_world_is_the_map(torch_cuda, renderer):
    sc, eye = empty_world()
    cam = eye.panoramic(TWO_PI)
    t = sample_map(W, H)
    sky = Sky.map(t)
    rs = settings(W, H)
    renderer.set_scene(sc)
    try:
        renderer.set_sky(sky)
        prev = gpu_render(torch_cuda, renderer, sc, cam, rs, preview=True, upload=False)[0][..., :3]
        rays, _ = projection_rays(cam, W, H, SEED, frame_samples(W, H, 0), centre=True)
        miss = _miss_mask(renderer, rays).reshape(H, W)
    finally:
        renderer.clear_sky()
    assert miss.mean() > 0.95
    want = sky.radiance(rays[:, 3:6]).reshape(H, W, 3)
    assert np.array_equal(bits(prev[miss]), bits(want[miss]))
    # pixel centres lie on texel centres: the preview is the map, within the CPU test's bound
    assert np.abs(prev.astype(np.float64) - t)[miss].max() <= lookup_bound(t, (W, H), 0.0)


def test_every_sample_goes_through_the_lookup(torch_cuda, renderer):
    sc, eye = empty_world()
    w, h = 16, 8
    rng = np.random.default_rng(9)
    d = rng.normal(size=(h, w, SPP, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros((h, w, SPP, 6), F32)
    rays[..., :3] = eye.eye
    rays[..., 3:] = d
    sky = Sky.map(sample_map(W, H), yaw=-1.1, scale=0.75)
    rs = settings(w, h)
    renderer.set_scene(sc)
    renderer.set_camera(eye)
    try:
        renderer.set_ray_source(rays)
        renderer.set_sky(sky)
        acc, segs, _ = gpu_render(torch_cuda, renderer, sc, eye, rs, upload=False)
        miss = _miss_mask(renderer, rays.reshape(-1, 6)).reshape(h, w, SPP).all(-1)
    finally:
        renderer.clear_sky()
        renderer.clear_ray_source()
    assert miss.mean() > 0.9 and (segs[miss] == SPP).all()
    want = sky.radiance(rays[..., 3:].reshape(-1, 3)).astype(np.float64).reshape(h, w, SPP, 3).mean(2)
    err = np.abs(acc[..., :3].astype(np.float64) - want)[miss]
    rel = (err / want[miss]).max()
    print(f"max relative error {rel:.3g} against {SPP * 2.0 ** -23:.3g}")
    assert (err <= SPP * 2.0 ** -23 * want[miss]).all()


# ------------------------------------------------------------------ scale reaches every bounce
def test_scale_two_doubles_the_frame(torch_cuda, renderer):
    sc, cam = open_room(), E.room_camera()
    rs = settings(24, 24)
    t = sample_map()
    renderer.set_scene(sc)
    try:
        renderer.set_sky(Sky.map(t, yaw=0.2, scale=1.0))
        one = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        renderer.set_sky(Sky.map(t, yaw=0.2, scale=2.0))
        two = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
    finally:
        renderer.clear_sky()
    assert one[0][..., :3].max() > 0.0 and (one[1] > SPP).any()  # light arrives, over more than one segment
    assert np.array_equal(bits(two[0][..., :3]), bits(one[0][..., :3] * F32(2.0)))
    assert np.array_equal(two[1], one[1])


# ------------------------------------------------------------------ directions at bounces have the right sign
def test_a_floor_sees_the_upper_half_of_the_map(torch_cuda, renderer):
    from octree_pathtracing_amd import scene as S

    sc = block_scene([(x, 4, z, E.STONE) for x in range(4, 28) for z in range(4, 28)])
    cam = S.Camera.look_at((16.0, 13.0, 16.0), (16.0, 5.0, 16.0), up=(0.0, 0.0, 1.0))
    rs = settings(24, 24)
    below = np.zeros((H, W, 3), F32)
    below[H // 2 + 1:] = sample_map()[H // 2 + 1:] + F32(0.5)  # rows under the horizon, clear of the bilinear band
    renderer.set_scene(sc)
    try:
        renderer.set_sky(Sky.map(below))
        dark = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
        renderer.set_sky(Sky.map(below[::-1]))
        lit = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
    finally:
        renderer.clear_sky()
    assert (dark[1] >= 2 * SPP).all()  # every pixel is a floor pixel: each sample bounces at least once
    assert (dark[0][..., :3] == 0.0).all()
    assert (lit[0][..., :3] > 0.0).all()


# ------------------------------------------------------------------ render forms agree
def test_render_forms_agree_under_a_map(torch_cuda, renderer):
    """tests/test_gpu_emitters.py's standard: the bits of the device render."""
    sc, cam = open_room(sun=True), E.room_camera()
    w = h = 16
    rs = settings(w, h, depth=4)
    r = renderer
    r.set_scene(sc)
    try:
        r.set_sky(Sky.map(sample_map(), yaw=1.0, scale=1.5))
        full = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
        assert full[0][..., :3].max() > 0.0
        acc, _, seg = r.render_tiles(rs, tiles=None)  # a tile list of every tile
        assert np.array_equal(bits(acc), bits(full[0])) and np.array_equal(seg, full[1])
        host, _ = r.render(rs)  # the sync render into host memory
        assert np.array_equal(bits(host), bits(full[0]))
        r.set_resolution((w, h))  # the async frame
        r.reset_render()
        r.max_depth, r.seed = rs.max_depth, rs.seed
        r.render_frame(rs.spp).wait_for()
        assert np.array_equal(bits(r.get_float_image().reshape(h, w, 4)), bits(full[0]))
        # the adaptive and the final driver, whose first round (min_spp = the cap: no threshold stops it) is the frame
        ada = r.render_adaptive(rs, min_spp=SPP, step_spp=SPP, threshold=1e-30)[0]
        assert np.array_equal(bits(ada), bits(full[0]))
        fin = r.render_final(rs, min_spp=SPP, step_spp=SPP, threshold=1e-30)
        assert np.array_equal(bits(fin["accum"]), bits(full[0])) and np.isfinite(fin["out"]).all()
    finally:
        r.clear_sky()


# ------------------------------------------------------------------ guide buffers
def test_guide_buffers_under_a_sky(torch_cuda, renderer):
    """The guide buffers describe hits; a miss is zeros and an infinite depth under every sky, the preview's miss is
    the sky's colour at every miss pixel (the sun's texture is off: nothing is drawn on the sky)."""
    from octree_pathtracing_amd import scene as S

    sc, cam = tiny_scene()
    sc.sun = S.Sun(draw_texture=False)
    rs = settings(40, 24)
    renderer.set_scene(sc)
    renderer.set_camera(cam)
    want = renderer.render_aov(rs)
    sky = Sky.gradient((0.9, 0.8, 0.7), (0.1, 0.3, 1.5), 2.0)
    try:
        renderer.set_sky(sky)
        got = renderer.render_aov(rs)
        prev = gpu_render(torch_cuda, renderer, sc, cam, rs, preview=True, upload=False)[0][..., :3]
    finally:
        renderer.clear_sky()
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    miss = got["prim"] == MISS
    assert miss.any() and not miss.all()
    assert (got["albedo"][miss] == 0.0).all() and np.isinf(got["depth"][miss]).all()
    rays, _ = projection_rays(cam, 40, 24, SEED, frame_samples(40, 24, 0), centre=True)
    sky_rgb = sky.radiance(rays[:, 3:6]).reshape(24, 40, 3)
    assert np.array_equal(bits(prev[miss]), bits(sky_rgb[miss]))


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_previous_sky(torch_cuda, renderer):
    r, lib = renderer, renderer._lib
    dirs = R.direction_set(8, 4, n_random=64)
    t = sample_map(8, 4)
    good = Sky.map(t, yaw=0.3, scale=1.25)
    nan, inf = float("nan"), float("inf")
    tex = rgba(t)
    try:
        r.set_sky(good)
        want = good.radiance(dirs)

        def refused(desc, texels=tex, status=_lib.ERR_INVALID_ARG):
            assert lib.octpt_set_sky(r._ctx, C.byref(desc), texels.ctypes.data if texels is not None else None) == status
            assert np.array_equal(bits(r.sky_radiance(dirs)), bits(want))

        base = dict(mode=R.MAP, texels=t, yaw=0.0, scale=1.0)
        for field, bad in (("mode", 4), ("scale", nan), ("scale", -0.5), ("scale", inf), ("yaw", nan), ("yaw", inf),
                           ("width", 0), ("height", 0)):
            d = c_sky(base)
            setattr(d, field, bad)
            refused(d)
        d = c_sky(base)
        d.width, d.height = 1 << 14, (1 << 12) + 1  # above 2^26 texels
        refused(d)
        refused(c_sky(base), texels=None)
        d = c_sky(base)
        d.reserved[0] = 1
        refused(d)
        for mode in (R.COLOR, R.GRADIENT):
            refused(c_sky(dict(mode=mode, scale=nan)))
        assert lib.octpt_set_sky(r._ctx, None, None) == _lib.ERR_INVALID_ARG
        got = _lib.SkyDesc()
        assert lib.octpt_get_sky(r._ctx, C.byref(got)) == _lib.OK
        assert (got.mode, got.width, got.height) == (R.MAP, 8, 4) and got.scale == 1.25
        with pytest.raises(_lib.OctptError):
            r.set_sky(Sky.color((1, 1, 1), nan))
        assert r.get_sky() is good
    finally:
        r.clear_sky()


def test_megakernel_and_multi_device_are_refused(torch_cuda, renderer):
    sc, cam = tiny_scene()
    rs = settings(40, 24)
    r = renderer
    r.set_scene(sc)
    r.set_camera(cam)
    try:
        r.set_sky(Sky.color((1.0, 0.5, 0.25), 1.0))
        n = rs.width * rs.height
        acc = torch_cuda.full((n, 4), 7.0, dtype=torch_cuda.float32, device="cuda")
        segs = torch_cuda.full((n,), 9, dtype=torch_cuda.int32, device="cuda")
        p = r.params(rs.width, rs.height, 0, rs.spp, megakernel=True)
        st = r._lib.octpt_render_device(r._ctx, C.byref(p), acc.data_ptr(), segs.data_ptr(), None)
        torch_cuda.cuda.synchronize()
        assert st == _lib.ERR_UNSUPPORTED
        assert (acc.cpu().numpy() == 7.0).all() and (segs.cpu().numpy() == 9).all()
        # the preview flag beside the megakernel flag is the preview, which follows the sky
        prev = gpu_render(torch_cuda, r, sc, cam, rs, megakernel=True, preview=True, upload=False)
        assert np.isfinite(prev[0]).all()
    finally:
        r.clear_sky()
    mk = r.params(rs.width, rs.height, 0, rs.spp, megakernel=True)
    # with the sky cleared the megakernel renders again
    assert r._lib.octpt_render_device(r._ctx, C.byref(mk), acc.data_ptr(), segs.data_ptr(), None) == _lib.OK
    torch_cuda.cuda.synchronize()
    # a multi-device context refuses every sky but DEFAULT, and renders what it rendered
    with HipRenderer(devices=[0, 0]) as m:
        m.set_scene(sc)
        m.set_camera(cam)
        m.max_depth, m.seed = rs.max_depth, rs.seed
        want, _ = m.render(rs)
        for sky in (Sky.color((1, 1, 1)), Sky.gradient((1, 1, 1), (0, 0, 1)), Sky.map(sample_map(8, 4))):
            d = sky.desc()
            tex = sky.texels
            st = m._lib.octpt_set_sky(m._ctx, C.byref(d), tex.ctypes.data if tex is not None else None)
            assert st == _lib.ERR_UNSUPPORTED
        m.clear_sky()  # DEFAULT is accepted
        marked = np.full((rs.height, rs.width, 4), 0.0, F32)
        marked[..., 3] = 1.0
        got, _ = m.render(rs, accum=marked)
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(m.sky_radiance(np.asarray([[0, 1, 0]], F32)), np.asarray([DEFAULT_RGB], F32))
