"""Camera projections on the GPU: parallel, fisheye and panoramic renders.  The oracle renders pinhole
cameras only, so -- as for the lens (C37) -- a projection is pinned by what a path's first ray decides alone: at
max_depth = 1 a sample is black exactly when the ray octpt_projection_rays publishes for it hits; the preview and the
guide buffers equal octpt_intersect of the un-jittered published ray; the full-depth frame is the same through every
code path that forms the ray -- shade's regeneration (a pool smaller than the chunk) and the emitter-sampling shade
(C38) among them, under every instance the scene selects; and with the pinhole projection everything is bit for bit
what it is without the call."""
import ctypes as C
import math
from dataclasses import replace

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd.renderer import HipRenderer, frame_samples
from tests import emitter_ref as E
from tests.test_gpu_beam import _renderer_with
from tests.test_gpu_parity import REL_TOL_FORWARD, gpu_render, rel_err, torch_cuda  # noqa: F401
from tests.test_projection_cpu import ROOM_FRAME, inside_camera, outside_camera, room

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = ROOM_FRAME  # 40 x 24: partial tiles on both axes
TWO_PI = float(np.float32(2.0 * math.pi))
MISS = 0xFFFFFFFF
UNSUPPORTED, INVALID_ARG = _lib.ERR_UNSUPPORTED, _lib.ERR_INVALID_ARG


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    """A renderer of this module's own: the projection is a setting of the context."""
    r = HipRenderer(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def tiny():
    """The 'tiny' config's spheres and cuboids (tests/test_gpu_parity.py, smoke()), at this module's frame."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config("tiny")
    return sc, cam, replace(rs, width=W, height=H, spp=SPP, max_depth=5, seed=SEED)


def project(cam, mode):
    return {"parallel": cam.parallel(30.0), "fisheye": cam.fisheye(math.pi), "panoramic": cam.panoramic(TWO_PI)}[mode]


MODES = ["parallel", "fisheye", "panoramic"]


# ------------------------------------------------------------------ the first ray decides: max_depth = 1
@pytest.mark.parametrize("megakernel", [False, True], ids=["wavefront", "megakernel"])
@pytest.mark.parametrize("mode", MODES)
def test_first_hit_is_the_published_ray(torch_cuda, renderer, tiny, mode, megakernel):
    sc, cam, rs = tiny
    cam = project(cam, mode)
    one = replace(rs, spp=1, max_depth=1)
    renderer.set_scene(sc)
    n_hit = 0
    for s in range(SPP):
        acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, one, spp_start=s, megakernel=megakernel, upload=False)
        rays, _ = renderer.projection_rays(W, H, SEED, frame_samples(W, H, s))
        hit = (renderer.intersect(rays)[1] != MISS).reshape(H, W)
        black = np.all(acc[..., :3] == 0.0, axis=-1)
        assert np.array_equal(black, hit), f"sample {s}: {np.argwhere(black != hit)[:5]}"
        assert np.all(segs == 1)
        assert st["beam_restarts"] == 0  # beam starts are off for a projection
        n_hit += int(hit.sum())
    frac = n_hit / (SPP * W * H)
    print(f"{mode}: hit {frac:.3f}")
    assert 0.01 <= frac <= 0.99  # the frame has both, so the equality above says something


# ------------------------------------------------------------------ preview and guide buffers
@pytest.mark.parametrize("view", ["outside", "inside"])
@pytest.mark.parametrize("mode", MODES)
def test_guides_and_preview_follow_the_projection(torch_cuda, renderer, mode, view):
    sc = room()
    cam = project(outside_camera() if view == "outside" else inside_camera(), mode)
    from octree_pathtracing_amd import scene as S

    rs = S.RenderSettings(width=W, height=H, spp=1, max_depth=5, seed=SEED)
    renderer.set_scene(sc)
    renderer.set_camera(cam)
    aov = renderer.render_aov(rs)
    rays, _ = renderer.projection_rays(W, H, SEED, frame_samples(W, H, 0), centre=True)
    t, prim, nrm, _ = renderer.intersect(rays)
    t, prim, nrm = t.reshape(H, W), prim.reshape(H, W), nrm.reshape(H, W, 3)
    hit = prim != MISS
    assert np.array_equal(aov["prim"], prim)
    assert np.array_equal(aov["depth"].view(np.uint32), t.view(np.uint32))  # the stone is opaque: one segment, its t
    assert np.array_equal(aov["material"], np.where(hit, 1, 0).astype(np.uint32))  # stone's material, 0 on a miss
    assert np.array_equal(aov["normal"][..., :3][hit], nrm[hit])
    print(f"{mode} {view}: hit {hit.mean():.3f}")
    if view == "inside" and mode != "parallel":  # (a parallel camera's origins spread beyond the walls)
        assert hit.all()
    if view == "outside":
        assert hit.sum() >= 8 and (~hit).sum() >= 8  # both, so the equalities above say something
    # the preview: the same pixels hit.  The room is one opaque material of one colour, so a hit pixel's flat shading
    # is a function of its normal alone -- the pinhole preview's colour for that normal -- and a miss is sky.
    prev, segs, _ = gpu_render(torch_cuda, renderer, sc, cam, rs, preview=True, upload=False)
    assert np.all(segs == 1)
    by_normal = {}
    back = S.Camera.look_at(E.ROOM_EYE, (5.0, 11.0, 7.0))
    for pin_cam in (outside_camera(), inside_camera(), back):  # pinhole views that see every face from both sides
        pin, _, _ = gpu_render(torch_cuda, renderer, sc, pin_cam, rs, preview=True, upload=False)
        pin_aov = renderer.render_aov(rs)
        seen = pin_aov["prim"] != MISS
        for n, c in zip(pin_aov["normal"][..., :3][seen], pin[..., :3][seen]):
            assert tuple(by_normal.setdefault(tuple(n), c)) == tuple(c)  # one colour per normal
    hit_colours = {tuple(c) for c in by_normal.values()}
    compared = 0
    for y in range(H):
        for x in range(W):
            c = tuple(prev[y, x, :3])
            if hit[y, x]:
                want = by_normal.get(tuple(nrm[y, x]))
                if want is not None:  # (a face no pinhole view saw has no colour to compare)
                    assert c == tuple(want), (x, y)
                    compared += 1
            else:
                assert c not in hit_colours and all(np.isfinite(c)), (x, y)
    assert compared >= 0.9 * hit.sum()


def test_parallel_depth_of_a_slab_is_constant(torch_cuda, renderer):
    """A parallel camera straight above an axis-aligned slab: every ray is the same direction from the same height,
    so the depth guide is one value over the slab's pixels -- the height above its top."""
    from octree_pathtracing_amd import scene as S

    sc = E.make_scene([(x, 8, z, E.STONE) for x in range(2, 30) for z in range(2, 30)])
    sc.build_octree(E.DEPTH)
    cam = S.Camera(eye=(16.0, 20.0, 16.0), direction=(0.0, -1.0, 0.0), up=(0.0, 0.0, 1.0)).parallel(16.0)
    rs = S.RenderSettings(width=W, height=H, spp=1, max_depth=5, seed=SEED)
    renderer.set_scene(sc)
    renderer.set_camera(cam)
    aov = renderer.render_aov(rs, which=("depth", "prim", "normal"))
    assert (aov["prim"] != MISS).all()
    assert np.all(aov["normal"][..., 1] == 1.0)
    assert len(np.unique(aov["depth"])) == 1, np.unique(aov["depth"])
    assert abs(float(aov["depth"][0, 0]) - 11.0) <= 1e-5
    # the pinhole view of the same slab is not flat: the check above is the projection's
    renderer.set_camera(replace(cam, projection=(0, 0.0)))
    assert len(np.unique(renderer.render_aov(rs, which=("depth",))["depth"])) > 1


# ------------------------------------------------------------------ one frame through every path that forms the ray
@pytest.fixture(scope="module")
def one_shot(torch_cuda, renderer, tiny):
    sc, cam, rs = tiny
    return {m: gpu_render(torch_cuda, renderer, sc, project(cam, m), rs) for m in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_full_depth_paths_agree(torch_cuda, renderer, tiny, one_shot, mode):
    sc, cam, rs = tiny
    cam = project(cam, mode)
    want = one_shot[mode]
    assert want[2]["beam_restarts"] == 0
    assert np.all(np.isfinite(want[0])) and want[0][..., :3].max() > 0.0
    # the megakernel: the same segments, the radiance as C37 compares it
    mk = gpu_render(torch_cuda, renderer, sc, cam, rs, megakernel=True)
    assert np.array_equal(mk[1], want[1])
    assert rel_err(mk[0], want[0]).max() <= REL_TOL_FORWARD
    # samples 0-1, then 2-3
    half = gpu_render(torch_cuda, renderer, sc, cam, replace(rs, spp=2))
    two = gpu_render(torch_cuda, renderer, sc, cam, replace(rs, spp=2), spp_start=2, accum=half[0])
    assert np.array_equal(two[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(half[1] + two[1], want[1])
    # the tile list
    acc, _, segs = renderer.render_tiles(rs, tiles=None)
    assert np.array_equal(acc.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(segs, want[1])
    # sync and async host frames
    host, _ = renderer.render(rs)
    assert np.array_equal(host.view(np.uint32), want[0].view(np.uint32))
    renderer.set_resolution((W, H))
    renderer.reset_render()
    renderer.max_depth, renderer.seed = rs.max_depth, rs.seed
    renderer.render_frame(rs.spp).wait_for()
    assert np.array_equal(renderer.get_float_image().reshape(H, W, 4).view(np.uint32), want[0].view(np.uint32))
    # two entries on one device
    with HipRenderer(devices=[0, 0]) as m:
        got = gpu_render(torch_cuda, m, sc, cam, rs)
        assert m.get_projection() == renderer.get_projection()
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    # and the frame is the projection's, not the pinhole's
    pin = gpu_render(torch_cuda, renderer, sc, replace(cam, projection=(0, 0.0)), rs)
    assert not np.array_equal(pin[0], want[0])


def test_adaptive_and_final_follow(torch_cuda, renderer, tiny):
    sc, cam, rs = tiny
    renderer.set_scene(sc)
    renderer.set_camera(cam.panoramic(TWO_PI))
    r = renderer.render_final(replace(rs, spp=8), min_spp=4, step_spp=4, threshold=0.05)
    assert np.all(np.isfinite(r["out"])) and r["out"][..., :3].max() > 0.0
    # the first round of the adaptive driver is the tile-list render of its samples: the projection's frame
    acc = renderer.render_adaptive(replace(rs, spp=4), min_spp=4, step_spp=4, threshold=0.05)[0]
    want = gpu_render(torch_cuda, renderer, sc, cam.panoramic(TWO_PI), rs)
    assert np.array_equal(acc.view(np.uint32), want[0].view(np.uint32))


# ------------------------------------------------------------------ pinhole is what it was
def test_pinhole_is_unchanged(torch_cuda, tiny):
    sc, cam, rs = tiny
    with HipRenderer(device=0) as fresh:  # octpt_set_projection is never called on this context
        never = gpu_render(torch_cuda, fresh, sc, cam, rs)
        never_prev = gpu_render(torch_cuda, fresh, sc, cam, rs, preview=True)
    with HipRenderer(device=0) as r:
        r.set_projection(_lib.PROJECTION_PINHOLE)
        assert r.get_projection() == (0, 0.0)
        explicit = gpu_render(torch_cuda, r, sc, cam, rs)
        r.set_projection(_lib.PROJECTION_FISHEYE, 2.0)
        other = gpu_render(torch_cuda, r, sc, replace(cam, projection=(2, 2.0)), rs)
        back = gpu_render(torch_cuda, r, sc, cam, rs)  # set_camera applies the camera's pinhole projection
        assert r.get_projection() == (0, 0.0)
        back_prev = gpu_render(torch_cuda, r, sc, cam, rs, preview=True)
    assert never[2]["segments"] > 0
    for got in (explicit, back):
        assert np.array_equal(got[0].view(np.uint32), never[0].view(np.uint32))
        assert np.array_equal(got[1], never[1])
        for k in ("paths", "segments", "esvo_steps", "shade_events"):
            assert got[2][k] == never[2][k], k
    assert np.array_equal(back_prev[0].view(np.uint32), never_prev[0].view(np.uint32))
    assert not np.array_equal(other[0], never[0])


# ------------------------------------------------------------------ a panorama inside a closed room sees no sky
@pytest.mark.parametrize("megakernel", [False, True], ids=["wavefront", "megakernel"])
def test_closed_room_panorama_sees_no_sky(torch_cuda, renderer, megakernel):
    from octree_pathtracing_amd import scene as S

    sc = room()
    cam = inside_camera().panoramic(TWO_PI)
    rs = S.RenderSettings(width=W, height=H, spp=SPP, max_depth=1, seed=SEED)
    acc, segs, _ = gpu_render(torch_cuda, renderer, sc, cam, rs, megakernel=megakernel)
    assert np.all(acc[..., :3] == 0.0) and np.all(segs == SPP)
    # the pinhole camera at the same place sees the same walls; an open room would not pass: without the ceiling ...
    open_room = E.room_scene(emitter=False, hole=True)
    open_room.build_octree(E.DEPTH)
    acc, _, _ = gpu_render(torch_cuda, renderer, open_room, cam, rs, megakernel=megakernel)
    assert (acc[..., :3].max(-1) > 0.0).any()  # ... the panorama sees the sky through the hole


# ------------------------------------------------------------------ refusals
def _projection(r):
    p = _lib.Projection()
    assert r._lib.octpt_get_projection(r._ctx, C.byref(p)) == _lib.OK
    return p.mode, p.param, tuple(p.reserved)


def _camera(r):
    c = _lib.Camera()
    assert r._lib.octpt_get_camera(r._ctx, C.byref(c)) == _lib.OK
    return tuple(c.eye), tuple(c.direction), tuple(c.up), c.fov, c.aperture, c.focal_distance


def _set(r, mode, param, word=None):
    p = _lib.Projection(mode, param)
    if word is not None:
        p.reserved[word] = 1
    return r._lib.octpt_set_projection(r._ctx, C.byref(p))


def _marked_render(torch, r, rs):
    """(accum, seg_count) of a render into marked buffers."""
    n = rs.width * rs.height
    acc = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    segs = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    r.max_depth, r.seed = rs.max_depth, rs.seed
    r.render_device(r.params(rs.width, rs.height, 0, rs.spp), acc.data_ptr(), segs.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return acc.cpu().numpy(), segs.cpu().numpy()


def test_refusals(torch_cuda, tiny):
    sc, cam, rs = tiny
    nan, inf = float("nan"), float("inf")
    with HipRenderer(device=0) as r:
        r.set_scene(sc)
        r.set_camera(cam)
        # a held setting survives every refused call, and the frame after them is the held setting's
        r.set_projection(_lib.PROJECTION_FISHEYE, 2.5)
        held = _projection(r)
        want = _marked_render(torch_cuda, r, rs)
        assert _set(r, 4, 1.0) == UNSUPPORTED and _set(r, 0x80000000, 1.0) == UNSUPPORTED
        for mode in (1, 2, 3):
            for param in (0.0, -2.0, nan, inf):
                assert _set(r, mode, param) == INVALID_ARG, (mode, param)
            for word in range(6):
                assert _set(r, mode, 1.0, word) == INVALID_ARG
        assert _set(r, 2, 7.0) == INVALID_ARG and _set(r, 3, 7.0) == INVALID_ARG  # above 2 pi
        assert _set(r, 0, 0.0, 2) == INVALID_ARG
        assert r._lib.octpt_set_projection(r._ctx, None) == INVALID_ARG
        assert _projection(r) == held
        got = _marked_render(torch_cuda, r, rs)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
        # an aperture second: the camera stays
        before = _camera(r)
        lens = cam.focus((16.0, 16.0, 16.0), 0.5)
        c = _lib.Camera((C.c_float * 3)(*lens.eye), (C.c_float * 3)(*lens.direction), (C.c_float * 3)(*lens.up), lens.fov,
                        lens.aperture, lens.focal_distance)
        assert r._lib.octpt_set_camera(r._ctx, C.byref(c)) == UNSUPPORTED
        assert _camera(r) == before and _projection(r) == held
        with pytest.raises(_lib.OctptError) as e:  # the Python surface: both stay too
            r.set_camera(replace(lens, projection=(2, 2.5)))
        assert e.value.status == UNSUPPORTED and _camera(r) == before and _projection(r) == held
        got = _marked_render(torch_cuda, r, rs)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        # the temporal passes and the context's reprojection refuse, their outputs untouched
        n = W * H
        color = np.zeros((H, W, 4), np.float32)
        aov = {"normal": np.zeros((H, W, 4), np.float32), "depth": np.ones((H, W), np.float32),
               "prim": np.zeros((H, W), np.uint32), "albedo": np.ones((H, W, 4), np.float32)}
        g = _lib.AovBuffers(**{k: v.ctypes.data for k, v in aov.items()})
        tp = _lib.TemporalParams(W, H, c, c, 32, 0.1, 0.9, _lib.TEMPORAL_MATCH_PRIM)
        tp.camera.aperture = tp.prev_camera.aperture = 0.0
        out = np.full((H, W, 4), 7.0, np.float32)
        length = np.full((H, W), 9, np.uint32)
        mom = np.full((H, W, 2), 5.0, np.float32)
        P_ = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert r._lib.octpt_temporal(r._ctx, C.byref(tp), P_(color), C.byref(g), None, P_(out), P_(length)) == UNSUPPORTED
        assert r._lib.octpt_temporal_moments(r._ctx, C.byref(tp), P_(color), C.byref(g), None, None, P_(out), P_(length),
                                             P_(mom)) == UNSUPPORTED
        d = {k: torch_cuda.as_tensor(v, device="cuda") for k, v in (("color", color), ("out", out), ("mom", mom))}
        d["length"] = torch_cuda.as_tensor(length.view(np.int32), device="cuda")
        dg = {k: torch_cuda.as_tensor(v.view(np.int32) if v.dtype == np.uint32 else v, device="cuda") for k, v in aov.items()}
        gd = _lib.AovBuffers(**{k: v.data_ptr() for k, v in dg.items()})
        vp = C.c_void_p
        assert r._lib.octpt_temporal_device(r._ctx, C.byref(tp), vp(d["color"].data_ptr()), C.byref(gd), None,
                                            vp(d["out"].data_ptr()), vp(d["length"].data_ptr()), None) == UNSUPPORTED
        assert r._lib.octpt_temporal_moments_device(r._ctx, C.byref(tp), vp(d["color"].data_ptr()), C.byref(gd), None, None,
                                                    vp(d["out"].data_ptr()), vp(d["length"].data_ptr()),
                                                    vp(d["mom"].data_ptr()), None) == UNSUPPORTED
        torch_cuda.cuda.synchronize()
        assert (d["out"].cpu().numpy() == 7.0).all() and (d["length"].cpu().numpy() == 9).all()
        assert (d["mom"].cpu().numpy() == 5.0).all()
        with pytest.raises(_lib.OctptError) as e:
            r.reproject_coords(cam, W, H, aov["depth"])
        assert e.value.status == UNSUPPORTED
        xy, zp = np.full((H, W, 2), 7.0, np.float32), np.full((H, W), 9.0, np.float32)
        assert r._lib.octpt_reproject_coords_ctx(r._ctx, C.byref(tp.camera), C.byref(tp.prev_camera), W, H,
                                                 P_(aov["depth"]), P_(xy), P_(zp)) == UNSUPPORTED
        assert (out == 7.0).all() and (length == 9).all() and (mom == 5.0).all() and (xy == 7.0).all() and (zp == 9.0).all()
        # under the pinhole projection they run
        r.set_projection(_lib.PROJECTION_PINHOLE)
        assert r._lib.octpt_temporal(r._ctx, C.byref(tp), P_(color), C.byref(g), None, P_(out), P_(length)) == _lib.OK
        assert not (out == 7.0).all()
        r.reproject_coords(cam, W, H, aov["depth"])
        # an aperture first: the projection stays
        r.set_camera(lens)
        held = _projection(r)
        assert held[0] == 0
        want = _marked_render(torch_cuda, r, rs)
        for mode, param in ((1, 10.0), (2, 1.0), (3, TWO_PI)):
            assert _set(r, mode, param) == UNSUPPORTED
            with pytest.raises(_lib.OctptError):
                r.set_projection(mode, param)
        assert _projection(r) == held and _camera(r)[4] == np.float32(0.5)
        got = _marked_render(torch_cuda, r, rs)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------ shade's regeneration, and the emitter shade
@pytest.fixture(scope="module")
def small_pool(torch_cuda):
    """100 path slots under chunks of two samples (1920 items), the knobs of tests/test_gpu_parity.py's small-pool
    case: the seed claims 100 items of a chunk, and every other path of it is formed where a finished one ends, by
    shade's regeneration (new_path in the regenerating shade instances)."""
    r = _renderer_with({"OCTPT_POOL": "100", "OCTPT_CHUNK": "2000"})
    yield r
    r.close()


# What selects a general shade instance besides regeneration: sun sampling (kNee), and material tables too long for
# their LDS copies (kLds off: more than 128 materials; the added ones are referenced by nothing)
SHADE_VARIANTS = ["plain", "sun", "long-tables", "sun-long-tables"]
NONE, ONE = 0, 1


def shade_variant(sc, variant, strategy):
    from octree_pathtracing_amd import scene as S

    sc = replace(sc)
    if "sun" in variant:
        sc.strategy = strategy
    if "long-tables" in variant:
        sc.materials = list(sc.materials) + [S.Material() for _ in range(129)]
    return sc


def _first_hits(torch, r, sc, cam, one, samples):
    """max_depth = 1 renders of the scene on r: black exactly where the published ray hits; the hit fraction."""
    n_hit = 0
    for s in samples:
        acc, segs, st = gpu_render(torch, r, sc, cam, one, spp_start=s, upload=False)
        rays, _ = r.projection_rays(W, H, SEED, frame_samples(W, H, s))
        hit = (r.intersect(rays)[1] != MISS).reshape(H, W)
        black = np.all(acc[..., :3] == 0.0, axis=-1)
        assert np.array_equal(black, hit), f"sample {s}: {np.argwhere(black != hit)[:5]}"
        assert np.all(segs == 1) and st["paths"] == W * H
        n_hit += int(hit.sum())
    return n_hit / (len(samples) * W * H)


def _same_frame(got, want):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1], want[1])
    for k in ("paths", "segments", "shade_events"):
        assert got[2][k] == want[2][k], k


@pytest.mark.parametrize("variant", SHADE_VARIANTS)
@pytest.mark.parametrize("mode", MODES)
def test_regenerated_paths_follow_the_projection(torch_cuda, renderer, small_pool, tiny, mode, variant):
    """960 items a sample against 100 path slots: nine paths in ten are regenerated.  Their first ray is the published
    one, and the full-depth frame (two chunks) is the default pool's bit for bit, which
    test_full_depth_paths_agree ties to every other path; the megakernel agrees as C37 compares it."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = tiny
    sc = shade_variant(sc, variant, S.SunSamplingStrategy(**vars(S.STRATEGY_HIGH_QUALITY)))
    cam = project(cam, mode)
    small_pool.set_scene(sc)
    frac = _first_hits(torch_cuda, small_pool, sc, cam, replace(rs, spp=1, max_depth=1), range(SPP))
    print(f"{mode} {variant}: hit {frac:.3f}")
    assert 0.01 <= frac <= 0.99
    want = gpu_render(torch_cuda, renderer, sc, cam, rs)
    assert np.all(np.isfinite(want[0])) and want[0][..., :3].max() > 0.0
    _same_frame(gpu_render(torch_cuda, small_pool, sc, cam, rs, upload=False), want)
    mk = gpu_render(torch_cuda, renderer, sc, cam, rs, megakernel=True, upload=False)
    assert np.array_equal(mk[1], want[1])
    assert rel_err(mk[0], want[0]).max() <= REL_TOL_FORWARD


@pytest.mark.parametrize("variant", SHADE_VARIANTS)
@pytest.mark.parametrize("mode", MODES)
def test_emitter_sampling_follows_the_projection(torch_cuda, renderer, small_pool, mode, variant):
    """Strategy ONE (C38) in the room with its two emitters, under a projection: the emitter shade's projected
    instances, with and without regeneration.  The first ray is the published one (from outside: hits and misses),
    and from inside the full-depth frame is the same as a tile list and on the small pool, bit for bit, with the
    emitter segments traced.  sun: the ceiling open, FAST with the sun's weight (test_gpu_emitters.py's setup)."""
    from octree_pathtracing_amd import scene as S

    sc = E.room_scene(second=True, hole="sun" in variant)
    sc = shade_variant(sc, variant, S.SunSamplingStrategy(True, False, False, True, False))
    sc.build_octree(E.DEPTH)
    rs = S.RenderSettings(width=W, height=H, spp=SPP, max_depth=3, seed=SEED)
    outside, inside = project(outside_camera(), mode), project(inside_camera(), mode)
    both = (renderer, small_pool)
    try:
        for r in both:
            r.set_emitter_sampling(NONE)
            r.set_scene(sc)
        none = gpu_render(torch_cuda, renderer, sc, inside, rs, upload=False)
        for r in both:
            r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
            assert len(r.emitter_grid()["emitters"]) == 2
            frac = _first_hits(torch_cuda, r, sc, outside, replace(rs, spp=1, max_depth=1), (0, SPP - 1))
            print(f"{mode} {variant}: hit {frac:.3f}")
            assert 0.01 <= frac <= 0.99
        full = gpu_render(torch_cuda, renderer, sc, inside, rs, upload=False)
        assert np.all(np.isfinite(full[0])) and full[0][..., :3].max() > 0.0
        assert full[2]["segments"] > none[2]["segments"]  # the emitter segments
        acc, _, segs = renderer.render_tiles(rs, tiles=None)
        assert np.array_equal(acc.view(np.uint32), full[0].view(np.uint32)) and np.array_equal(segs, full[1])
        _same_frame(gpu_render(torch_cuda, small_pool, sc, inside, rs, upload=False), full)
        pin = gpu_render(torch_cuda, renderer, sc, replace(inside, projection=(0, 0.0)), rs, upload=False)
        assert not np.array_equal(pin[0], full[0])
    finally:
        for r in both:
            r.set_emitter_sampling(NONE)
