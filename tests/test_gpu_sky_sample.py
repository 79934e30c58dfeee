"""Importance sampling of the sky map on the GPU.  The device's distribution is the host builder's,
integer for integer; the device sample is the host's bit for bit; off is off, and the inert cases render the unsampled
frame's bits; no draw of a path changes; the sampled render has the unsampled render's expectation (the parent's code
path is the reference), with sun sampling and under the fisheye too; it cuts the variance where the map's power sits in
one texel; every render form agrees; and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd import scene as S
from octree_pathtracing_amd.renderer import HipRenderer, frame_samples, projection_rays, tile_count
from octree_pathtracing_amd.scene import Sky
from tests import emitter_ref as E
from tests import sky_ref as R
from tests import sky_sample_ref as SS
from tests.test_gpu_parity import gpu_render, torch_cuda  # noqa: F401
from tests.test_gpu_sky import bits, block_scene, same, settings, tiny_scene
from tests.test_sky_sample_cpu import SIZES, bright_map, draws, hostile_map, random_map

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 11
FLT_MAX = float(np.finfo(F32).max)


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    """A renderer of this module's own: the sky and its sampling are settings of the context."""
    r = HipRenderer(device=0)
    yield r
    r.set_sky_sampling(False)
    r.close()


def smooth_map():
    """32 x 16, texels in 0.5 .. 2."""
    y, x = np.mgrid[0:16, 0:32]
    t = np.stack([1.25 + 0.75 * np.sin(2 * np.pi * x / 32), 1.25 + 0.75 * np.cos(np.pi * (y + 0.5) / 16),
                  1.25 + 0.75 * np.sin(2 * np.pi * x / 32 + 1.0) * np.sin(np.pi * (y + 0.5) / 16)], -1)
    assert t.min() >= 0.5 and t.max() <= 2.0
    return t.astype(F32)


def floor_cells():
    return [(x, 4, z, E.STONE) for x in range(4, 28) for z in range(4, 28)]


def floor_scene(occluder=True, sun_sampling=False):
    """A floor of the diffuse stone block, one block above it casting a shadow; the sun's texture is off, and without
    sun sampling its diffuse term too."""
    sc = block_scene(floor_cells() + ([(16, 6, 16, E.STONE)] if occluder else []))
    if sun_sampling:
        sc.strategy = S.SunSamplingStrategy(True, False, False, True, False)
        sc.build_octree(E.DEPTH)
    return sc


def floor_camera():
    return S.Camera.look_at((16.0, 13.0, 16.0), (16.0, 5.0, 16.0), up=(0.0, 0.0, 1.0))


def regions(r, cam, rs):
    """(shadowed floor, lit floor, the rest) as boolean [H, W], from the guide buffers' depth along the pixel-centre
    rays: the floor's top is y = 5, the shadow the 5 x 5 cells under the block."""
    w, h = rs.width, rs.height
    r.set_camera(cam)
    depth = r.render_aov(rs, which=("depth",))["depth"]
    rays, _ = projection_rays(cam, w, h, SEED, frame_samples(w, h, 0), centre=True)
    hit = np.isfinite(depth)
    pos = rays[:, :3].reshape(h, w, 3) + rays[:, 3:].reshape(h, w, 3) * np.where(hit, depth, 0.0)[..., None]
    floor = hit & (np.abs(pos[..., 1] - 5.0) < 1e-3)
    under = (np.abs(pos[..., 0] - 16.5) < 2.5) & (np.abs(pos[..., 2] - 16.5) < 2.5)
    return floor & under, floor & ~under, ~floor


def moments_frame(r, rs):
    """(mean luminance [H, W], variance of that mean [H, W], accum, seg_count) of a tile-list render of every tile."""
    acc, mom, seg = r.render_tiles(rs, tiles=None)
    spp = np.full(tile_count(rs.width, rs.height), rs.spp, np.uint32)
    aov = r.render_aov(rs, which=("depth", "albedo"))
    var = r.sample_variance(mom, spp, aov, demodulate=False)
    return mom[..., 0].astype(np.float64), var.astype(np.float64), acc, seg


# ------------------------------------------------------------------ the distribution
def test_device_distribution_is_the_host_builders(renderer):
    r = renderer
    maps = [random_map(w, h) for (w, h) in SIZES] + [hostile_map(), bright_map(), np.full((4, 8, 3), FLT_MAX, F32)]
    try:
        r.set_sky_sampling(True)
        assert r.sky_distribution() is None  # no map yet
        for t in maps:
            r.set_sky(Sky.map(t, yaw=0.3, scale=2.0))  # a second octpt_set_sky rebuilds it
            got, want = r.sky_distribution(), S.build_sky_distribution(t)
            assert np.array_equal(got["col_cdf"], want["col_cdf"]) and np.array_equal(got["row_cdf"], want["row_cdf"])
            assert got["total"] == want["total"] > 0
        r.set_sky(Sky.map(np.zeros((4, 8, 3), F32)))
        assert r.sky_distribution()["total"] == 0 and not r.sky_distribution()["col_cdf"].any()
        r.set_sky(Sky.color((1, 1, 1)))  # a sky of another mode drops it
        assert r.sky_distribution() is None
        r.set_sky(Sky.map(maps[0]))
        assert r.sky_distribution() is not None
        r.clear_sky()
        a = _lib.SkyDistributionArrays()
        assert r._lib.octpt_sky_distribution(r._ctx, C.byref(a)) == _lib.OK and (a.width, a.height) == (0, 0)
        r.set_sky(Sky.map(maps[1]))
        r.set_sky_sampling(False)  # ... and so does turning sampling off
        assert r.sky_distribution() is None
        r.set_sky_sampling(True)  # the setting after the sky: built by whichever comes second
        assert r.sky_distribution()["total"] == S.build_sky_distribution(maps[1])["total"]
    finally:
        r.set_sky_sampling(False)
        r.clear_sky()


@pytest.mark.parametrize("yaw", [0.0, 0.7])
def test_device_sample_is_the_hosts(renderer, yaw):
    r = renderer
    u = draws(4096, seed=5)
    u[:8, :] = [[0, 0, 0, 0], [0.99999994] * 4, [0, 0.99999994, 0, 0.99999994], [0.5, 0.5, 0, 0], [0.5, 0.5, 0.99999994, 0.5],
                [0.25, 0.75, 0.5, 0], [0.99999994, 0, 0.5, 0.5], [0.1, 0.2, 0.3, 0.4]]
    try:
        r.set_sky_sampling(True)
        for t in (random_map(33, 17), bright_map(), random_map(5, 1), random_map(1, 1)):
            r.set_sky(Sky.map(t, yaw=yaw))
            got, want = r.sky_samples(u), S.sky_samples(S.build_sky_distribution(t), u, yaw)
            for k in ("d", "pdf", "x", "y", "q"):
                assert np.array_equal(bits(got[k]), bits(want[k])), k
            assert np.array_equal(got["ok"], want["ok"]) and want["ok"].mean() > 0.99
    finally:
        r.set_sky_sampling(False)
        r.clear_sky()


# ------------------------------------------------------------------ off is off; the inert cases
@pytest.mark.parametrize("sun", [False, True], ids=["plain", "sun-sampling"])
def test_off_is_off_and_the_inert_cases(torch_cuda, sun):
    sc, cam = floor_scene(sun_sampling=sun), floor_camera()
    rs = settings(32, 32, spp=4)
    sky = Sky.map(smooth_map(), yaw=0.5, scale=1.5)
    colour, black = Sky.color((0.3, 0.9, 0.4), 2.0), Sky.map(np.zeros((4, 8, 3), F32))
    with HipRenderer(device=0) as fresh:  # a context that never called the setter
        fresh.set_sky(sky)
        want = gpu_render(torch_cuda, fresh, sc, cam, rs)
        fresh.set_sky(colour)
        want_colour = gpu_render(torch_cuda, fresh, sc, cam, rs, upload=False)
        fresh.set_sky(black)
        want_black = gpu_render(torch_cuda, fresh, sc, cam, rs, upload=False)
    with HipRenderer(device=0) as r:
        r.set_sky_sampling(True)
        r.set_sky(sky)
        sampled = gpu_render(torch_cuda, r, sc, cam, rs)
        r.set_sky(colour)
        same(gpu_render(torch_cuda, r, sc, cam, rs, upload=False), want_colour)
        r.set_sky(black)
        same(gpu_render(torch_cuda, r, sc, cam, rs, upload=False), want_black)
        r.set_sky(sky)
        r.set_sky_sampling(False)
        got = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
    same(got, want)
    for k in ("paths", "segments", "shade_events"):
        assert got[2][k] == want[2][k], k
    # the sampled frame is another estimate: its shadow segments are counted
    assert not np.array_equal(sampled[0], want[0]) and sampled[2]["segments"] > want[2]["segments"]


# ------------------------------------------------------------------ no draw of the path changes
def test_mirrors_render_the_same_bits(torch_cuda, renderer):
    sc, cam = tiny_scene()
    for m in sc.materials:
        m.specular = 1.0
    rs = settings(40, 24)
    r = renderer
    try:
        r.set_sky(Sky.map(smooth_map(), yaw=0.2))
        off = gpu_render(torch_cuda, r, sc, cam, rs)
        r.set_sky_sampling(True)
        on = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
    finally:
        r.set_sky_sampling(False)
        r.clear_sky()
    assert off[0][..., :3].max() > 0.0 and (off[1] > rs.spp).any()
    same(on, off)
    assert on[2]["segments"] == off[2]["segments"] and on[2]["shade_events"] == off[2]["shade_events"]


# ------------------------------------------------------------------ the same expectation
def expectation_case(r, sc, cam, rs, sky):
    r.set_scene(sc)
    r.set_camera(cam)
    r.max_depth, r.seed = rs.max_depth, rs.seed
    try:
        r.set_sky_sampling(False)
        r.set_sky(sky)
        a = moments_frame(r, rs)
        r.set_sky_sampling(True)
        b = moments_frame(r, rs)
    finally:
        r.set_sky_sampling(False)
        r.clear_sky()
    return a, b, regions(r, cam, rs)


@pytest.mark.parametrize("case", ["plain", "sun-sampling", "fisheye"])
def test_sampled_render_has_the_unsampled_expectation(torch_cuda, renderer, case):
    sc = floor_scene(sun_sampling=case == "sun-sampling")
    cam = floor_camera().fisheye(0.75 * math.pi) if case == "fisheye" else floor_camera()
    rs = settings(32, 32, spp=256, depth=3)
    a, b, regs = expectation_case(renderer, sc, cam, rs, Sky.map(smooth_map(), yaw=0.4))
    assert b[3].sum() > a[3].sum()  # the sky's shadow segments are counted
    for name, mask in zip(("shadowed", "lit", "rest"), regs):
        n = int(mask.sum())
        if name != "rest" or n:
            assert n > 0, name
        if n == 0:
            continue
        da = abs(a[0][mask].mean() - b[0][mask].mean())
        tol = 5.0 * math.sqrt((a[1][mask] + b[1][mask]).sum()) / n
        print(f"{case} {name}: n {n} A {a[0][mask].mean():.6g} B {b[0][mask].mean():.6g} |d| {da:.3g} tol {tol:.3g}")
        assert da <= tol, (case, name)
    # the shadow is there: the floor under the block is darker than the open floor
    assert a[0][regs[0]].mean() < a[0][regs[1]].mean()


def test_uniform_map_matches_the_exact_floor(torch_cuda, renderer):
    """An open floor at max_depth 2 under a map of equal texels: every unsampled floor sample is the same number (zero
    variance), which the sampled frame must match within 5 of its own standard errors."""
    sc, cam = floor_scene(occluder=False), floor_camera()
    rs = settings(32, 32, spp=64, depth=2)
    t = np.full((16, 32, 3), 0.8, F32)
    a, b, regs = expectation_case(renderer, sc, cam, rs, Sky.map(t))
    floor = regs[0] | regs[1]
    assert floor.all() and np.median(a[1][floor]) <= 1e-6 * a[0][floor].max() ** 2  # (f32 rounding; a rare grazing bounce meets the floor again)
    da = abs(a[0][floor].mean() - b[0][floor].mean())
    tol = 5.0 * math.sqrt(b[1][floor].sum()) / floor.sum()
    print(f"uniform: A {a[0][floor].mean():.6g} B {b[0][floor].mean():.6g} |d| {da:.3g} tol {tol:.3g}")
    assert b[1][floor].max() > 0 and da <= tol


# ------------------------------------------------------------------ it helps where it should
def test_one_bright_texel_converges_ten_times_faster(torch_cuda, renderer):
    """An open floor at max_depth 2, 64 spp, under a 64 x 32 map of 0.05 with one texel of row 4 at 2000: the texel
    covers less than 1 / 2000 of the sphere and carries more than 90 % of the floor's cosine-weighted power, so the
    unsampled estimate's relative variance per sample is above 1000 and the sampled one's O(1): the mean variance of
    the pixel means must fall at least 10 times (measured: DESIGN.md C43)."""
    t = np.full((32, 64, 3), 0.05, F32)
    t[4, 20] = 2000.0
    assert SS.texel_solid_angle(64, 32, 4) / (4 * math.pi) < 1.0 / 2000.0

    def floor_power(tex):  # the integral of lum(bilinear map) * max(d.y, 0) over the sphere, float64 midpoint rule
        sub = 8
        fx = (np.arange(64 * sub) + 0.5) / sub - 0.5
        fy = (np.arange(32 * sub) + 0.5) / sub - 0.5
        FX, FY = np.meshgrid(fx, fy)
        theta = np.pi * (FY + 0.5) / 32
        val = SS.lum64(R.bilinear(tex.astype(np.float64), FX.ravel(), FY.ravel())).reshape(FY.shape)
        return float((val * np.sin(theta) * np.maximum(np.cos(theta), 0.0)).sum())

    without = t.copy()
    without[4, 20] = 0.05
    assert 1.0 - floor_power(without) / floor_power(t) > 0.9
    sc, cam = floor_scene(occluder=False), floor_camera()
    rs = settings(32, 32, spp=64, depth=2)
    a, b, regs = expectation_case(renderer, sc, cam, rs, Sky.map(t, yaw=0.3))
    floor = regs[0] | regs[1]
    assert floor.all()
    va, vb = a[1][floor].mean(), b[1][floor].mean()
    print(f"bright texel: variance of the mean unsampled {va:.6g}, sampled {vb:.6g}, ratio {va / vb:.4g}; "
          f"means {a[0][floor].mean():.6g} {b[0][floor].mean():.6g}")
    assert vb > 0 and va >= 10.0 * vb


# ------------------------------------------------------------------ render forms agree
def test_render_forms_agree_under_sampling(torch_cuda, renderer):
    """tests/test_gpu_sky.py's relations, with sampling on: the bits of the device render."""
    sc, cam = floor_scene(sun_sampling=True), floor_camera()
    w = h = 32
    rs = settings(w, h, spp=4, depth=3)
    r = renderer
    r.set_scene(sc)
    try:
        r.set_sky(Sky.map(smooth_map(), yaw=1.0, scale=1.5))
        r.set_sky_sampling(True)
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
        ada = r.render_adaptive(rs, min_spp=rs.spp, step_spp=rs.spp, threshold=1e-30)[0]
        assert np.array_equal(bits(ada), bits(full[0]))
        fin = r.render_final(rs, min_spp=rs.spp, step_spp=rs.spp, threshold=1e-30)
        assert np.array_equal(bits(fin["accum"]), bits(full[0])) and np.isfinite(fin["out"]).all()
        # the preview ignores the setting
        prev = gpu_render(torch_cuda, r, sc, cam, rs, preview=True, upload=False)
        r.set_sky_sampling(False)
        same(gpu_render(torch_cuda, r, sc, cam, rs, preview=True, upload=False), prev)
    finally:
        r.set_sky_sampling(False)
        r.clear_sky()


# ------------------------------------------------------------------ refusals
def test_refusals(torch_cuda, renderer):
    r, lib = renderer, renderer._lib
    sc, cam = floor_scene(), floor_camera()
    rs = settings(32, 32, spp=2, depth=3)
    r.set_scene(sc)
    r.set_camera(cam)
    r.max_depth, r.seed = rs.max_depth, rs.seed
    n = rs.width * rs.height

    def mode():
        p = _lib.SkySampling()
        assert lib.octpt_get_sky_sampling(r._ctx, C.byref(p)) == _lib.OK
        return p.mode

    try:
        r.set_sky(Sky.map(smooth_map()))
        r.set_sky_sampling(True)
        # a reserved word, an unknown mode: INVALID_ARG, the setting stays
        p = _lib.SkySampling()
        p.mode, p.reserved[6] = _lib.SKY_SAMPLING_NONE, 1
        assert lib.octpt_set_sky_sampling(r._ctx, C.byref(p)) == _lib.ERR_INVALID_ARG
        p = _lib.SkySampling()
        p.mode = 2
        assert lib.octpt_set_sky_sampling(r._ctx, C.byref(p)) == _lib.ERR_INVALID_ARG
        assert lib.octpt_set_sky_sampling(r._ctx, None) == _lib.ERR_INVALID_ARG
        assert mode() == _lib.SKY_SAMPLING_MAP and r.sky_sampling and r.sky_distribution() is not None
        # the megakernel flag: UNSUPPORTED, the buffers untouched
        acc = torch_cuda.full((n, 4), 7.0, dtype=torch_cuda.float32, device="cuda")
        segs = torch_cuda.full((n,), 9, dtype=torch_cuda.int32, device="cuda")
        mk = r.params(rs.width, rs.height, 0, rs.spp, megakernel=True)
        assert lib.octpt_render_device(r._ctx, C.byref(mk), acc.data_ptr(), segs.data_ptr(), None) == _lib.ERR_UNSUPPORTED
        torch_cuda.cuda.synchronize()
        assert (acc.cpu().numpy() == 7.0).all() and (segs.cpu().numpy() == 9).all()
        # emitter sampling ONE after sky sampling ...
        with pytest.raises(_lib.OctptError) as refused:
            r.set_emitter_sampling(_lib.EMITTERS_ONE, E.ROOM_GRID, 1.0)
        assert refused.value.status == _lib.ERR_UNSUPPORTED
        wf = r.params(rs.width, rs.height, 0, rs.spp)
        assert lib.octpt_render_device(r._ctx, C.byref(wf), acc.data_ptr(), segs.data_ptr(), None) == _lib.OK  # (ONE was not taken)
        torch_cuda.cuda.synchronize()
        # ... and sky sampling after emitter sampling ONE
        r.set_sky_sampling(False)
        r.set_emitter_sampling(_lib.EMITTERS_ONE, E.ROOM_GRID, 1.0)
        p = _lib.SkySampling()
        p.mode = _lib.SKY_SAMPLING_MAP
        assert lib.octpt_set_sky_sampling(r._ctx, C.byref(p)) == _lib.ERR_UNSUPPORTED
        assert mode() == _lib.SKY_SAMPLING_NONE and r.sky_distribution() is None
    finally:
        r.set_emitter_sampling(_lib.EMITTERS_NONE)
        r.set_sky_sampling(False)
        r.clear_sky()
    with HipRenderer(devices=[0, 0]) as m:  # a multi-device context
        p = _lib.SkySampling()
        p.mode = _lib.SKY_SAMPLING_MAP
        assert m._lib.octpt_set_sky_sampling(m._ctx, C.byref(p)) == _lib.ERR_UNSUPPORTED
        assert not m.sky_sampling
        m.set_sky_sampling(False)  # NONE is accepted
