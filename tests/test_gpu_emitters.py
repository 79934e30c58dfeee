"""The emitter grid on the device and the emitter-sampling setting.

The device grid must equal the host builder's (octpt_build_emitter_grid, itself pinned to the numpy definition by
tests/test_emitter_cpu.py) array for array, after each of the three scene paths, on a multi-device context and
across changes of the setting; ONE over a scene with nothing to sample renders bit for bit what NONE renders; and
the refusals leave the caller's buffers untouched.  The estimator: exact occlusion behind a wall with the shadow
segment counted, the lit value against the float64 statement of tests/emitter_ref.py within the reference's own
standard error, less variance than NONE, and bit-identity across tile lists, devices and the async frame."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import emitter_ref as E
from tests.test_gpu_parity import gpu_render, renderer, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, 5
NONE, ONE = 0, 1


def _host(name, grid_size):
    from octree_pathtracing_amd import scene as S

    cells, compact = E.WORLDS[name]
    return S.build_emitter_grid(E.make_scene(cells), E.DEPTH, grid_size, compact=compact)


def _set_scene(r, name, path):
    """The world on the renderer through one of the three scene paths."""
    from octree_pathtracing_amd import scene as S

    cells, compact = E.WORLDS[name]
    sc = E.make_scene(cells)
    if path == "upload":
        sc.build_octree(E.DEPTH, compact=compact)
        r.set_scene(sc)
    elif path == "cells":
        r.set_scene_built(sc, E.DEPTH, compact=compact)
    else:
        r.set_scene_built_sections(sc, E.DEPTH, S.SectionWorld.from_cells(sc.cells_array(), E.DEPTH), compact=compact)
    return sc


# (a section world needs a section: the empty world goes through the other two paths)
@pytest.mark.parametrize("name,path", [(n, p) for n in sorted(E.WORLDS) for p in ("upload", "cells", "sections")
                                       if (n, p) != ("empty", "sections")])
def test_device_grid_equals_host_grid(renderer, name, path):
    r = renderer
    r.set_emitter_sampling(NONE)
    for grid_size in E.GRID_SIZES:  # the setting first, then the scene: the scene call builds the grid
        r.set_emitter_sampling(ONE, grid_size, 1.0)
        _set_scene(r, name, path)
        E.assert_same_grid(r.emitter_grid(), _host(name, grid_size))
    r.set_emitter_sampling(NONE)


def test_grid_follows_the_setting(renderer):
    """NONE -> ONE -> NONE -> ONE with another grid_size over one resident scene; NONE holds no grid."""
    from octree_pathtracing_amd._lib import OctptError

    r = renderer
    r.set_emitter_sampling(NONE)
    _set_scene(r, "big_compact", "cells")
    with pytest.raises(OctptError) as e:
        r.emitter_grid()
    assert e.value.status == INVALID_ARG
    r.set_emitter_sampling(ONE, 4, 1.0)
    E.assert_same_grid(r.emitter_grid(), _host("big_compact", 4))
    r.set_emitter_sampling(NONE, 4, 1.0)
    with pytest.raises(OctptError):
        r.emitter_grid()
    r.set_emitter_sampling(ONE, 16, 2.0)
    E.assert_same_grid(r.emitter_grid(), _host("big_compact", 16))
    r.set_emitter_sampling(NONE)


def test_multi_device_grid(torch_cuda):
    from octree_pathtracing_amd.renderer import HipRenderer

    with HipRenderer(devices=[0, 0]) as r:
        r.set_emitter_sampling(ONE, 4, 1.0)
        for name, path in (("corners", "upload"), ("group_compact", "cells"), ("border", "sections")):
            _set_scene(r, name, path)
            E.assert_same_grid(r.emitter_grid(), _host(name, 4))


def _view():
    from octree_pathtracing_amd import scene as S

    cam = S.Camera.look_at((28.0, 20.0, 30.0), (4.0, 3.0, 4.0))
    return cam, S.RenderSettings(width=48, height=32, spp=8, max_depth=5, seed=3)


@pytest.mark.parametrize("aperture", [0.0, 0.4])
def test_nothing_to_sample_changes_nothing(torch_cuda, renderer, aperture):
    """A block scene with no emissive full-cell leaf: ONE against NONE, accum, seg_count and the segment total bit
    for bit, with a pinhole camera and with an aperture."""
    r = renderer
    cam, rs = _view()
    if aperture:
        cam = cam.focus((4.0, 3.0, 4.0), aperture)
    r.set_emitter_sampling(NONE)
    sc = _set_scene(r, "no_emitters", "upload")
    want = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
    r.set_emitter_sampling(ONE, 4, 1.0)
    assert len(r.emitter_grid()["emitters"]) == 0
    got = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
    r.set_emitter_sampling(NONE)
    assert want[2]["segments"] > 0 and (want[1] > 0).any()
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1], want[1])
    assert got[2]["segments"] == want[2]["segments"]


def _render_status(torch, r, rs, megakernel=False):
    """(status, accum, seg_count) of a render into marked buffers."""
    from octree_pathtracing_amd._lib import OctptError

    n = rs.width * rs.height
    acc = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    segs = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    p = r.params(rs.width, rs.height, 0, rs.spp, 0, 1, False, megakernel)
    status = 0
    try:
        r.render_device(p, acc.data_ptr(), segs.data_ptr(), torch.cuda.current_stream().cuda_stream)
    except OctptError as e:
        status = e.status
    torch.cuda.synchronize()
    return status, acc.cpu().numpy(), segs.cpu().numpy()


def test_refusals_leave_everything_untouched(torch_cuda, renderer):
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S

    r, torch = renderer, torch_cuda
    cam, rs = _view()
    r.set_emitter_sampling(NONE)
    _set_scene(r, "two_in_cell", "upload")
    r.set_camera(cam)
    r.set_emitter_sampling(ONE, 8, 1.5)
    held = r.emitter_grid()

    def status(strategy, grid_size, intensity, reserved=0):
        p = _lib.EmitterParams(strategy, grid_size, intensity)
        p.reserved[3] = reserved
        return r._lib.octpt_set_emitter_sampling(r._ctx, C.byref(p))

    assert status(2, 8, 1.0) == UNSUPPORTED and status(3, 8, 1.0) == UNSUPPORTED and status(9, 8, 1.0) == UNSUPPORTED
    for gs in (0, 3, 24, 64, 1 << 22):  # 0, not a power of two, above 2^depth = 32
        assert status(ONE, gs, 1.0) == INVALID_ARG, gs
    for bad in (float("nan"), -1.0, float("inf")):
        assert status(ONE, 8, bad) == INVALID_ARG
    assert status(ONE, 8, 1.0, reserved=1) == INVALID_ARG
    E.assert_same_grid(r.emitter_grid(), held)  # the setting stayed
    # renders: the megakernel
    st, acc, segs = _render_status(torch, r, rs, megakernel=True)
    assert st == UNSUPPORTED and (acc == 7.0).all() and (segs == 9).all()
    # ONE on a scene of primitive leaves
    sph, scam, srs = S.make_config("tiny")
    with pytest.raises(_lib.OctptError) as e:
        r.set_scene(dataclasses.replace(sph, emitter_sampling=ONE))
    assert e.value.status == UNSUPPORTED
    r.set_camera(scam)
    st, acc, segs = _render_status(torch, r, dataclasses.replace(srs, width=16, height=16, spp=1))
    assert st == UNSUPPORTED and (acc == 7.0).all() and (segs == 9).all()
    r.set_emitter_sampling(NONE)
    st, acc, _ = _render_status(torch, r, dataclasses.replace(srs, width=16, height=16, spp=1))
    assert st == 0 and not (acc == 7.0).all()


# ------------------------------------------------------------------ the estimator (the room of tests/emitter_ref.py)
def _room(r, **kw):
    sc = E.room_scene(**kw)
    sc.build_octree(E.DEPTH)
    r.set_scene(sc)
    r.set_camera(E.room_camera())
    return sc


def _room_settings(spp, max_depth, W=16, H=16):
    from octree_pathtracing_amd import scene as S

    return S.RenderSettings(width=W, height=H, spp=spp, max_depth=max_depth, seed=5)


def _floor_hits(r, rs):
    """Per pixel: whether the pixel centre's first hit is the floor top, and its z."""
    aov = r.render_aov(rs, which=("normal", "depth", "prim", "albedo"))
    rays = r.camera_rays(rs.width, rs.height).reshape(rs.height, rs.width, 6)
    z = rays[..., 2] + rays[..., 5] * aov["depth"]
    floor = (aov["normal"][..., 1] == 1.0) & np.isfinite(aov["depth"])
    return floor, z, aov


def test_occlusion_is_exact(torch_cuda, renderer):
    """The emitter behind a full wall: the floor on the camera's side stays exactly black, and every sample traced
    camera, shadow and bounce segments (3) where NONE traces 2."""
    r, torch = renderer, torch_cuda
    r.set_emitter_sampling(NONE)
    sc = _room(r, wall=True)
    rs = _room_settings(8, 2)
    floor, z, aov = _floor_hits(r, rs)
    sel = floor & (z < 13.0) & (z > 8.5)  # whole pixels on the near side of the wall at z = 14
    assert sel.sum() >= 64 and len(np.unique(aov["prim"][sel])) == 1
    cam = E.room_camera()
    none = gpu_render(torch, r, sc, cam, rs, upload=False)
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
    assert len(r.emitter_grid()["emitters"]) == 1
    one = gpu_render(torch, r, sc, cam, rs, upload=False)
    r.set_emitter_sampling(NONE)
    assert (one[0][sel][:, :3] == 0.0).all()
    assert (none[1][sel] == 2 * rs.spp).all() and (one[1][sel] == 3 * rs.spp).all()
    assert one[2]["segments"] > none[2]["segments"]


_CUBE_MOMENTS = {}


def _lit_reference(r, rs, cubes, albedo, pixels, intensity=1.0):
    """Per chosen pixel: expectation, standard error and quadrature error of the rendered value (one channel scale:
    multiply by the pixel's albedo), from the published first rays and the float64 estimator."""
    n = np.array([0.0, 1.0, 0.0])
    lo, hi = np.array([5.0, 5.0, 5.0]), np.array([19.0, 12.0, 19.0])
    for x, y, z, s in cubes:  # the reference decides visibility: the interior is convex and holds only the emitters
        assert (np.array([x, y, z]) >= lo).all() and (np.array([x, y, z]) + s <= hi).all()

    def crosses(p, q, box):  # segments p[i] -> q[j] against an open box (slab test), any crossing
        d = q[None, :, :] - p[:, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (box[0] - p[:, None, :]) / d, (box[1] - p[:, None, :]) / d
        near, far = np.fmin(t0, t1).max(-1), np.fmax(t0, t1).min(-1)
        return bool(((near < far) & (far > 0.0) & (near < 1.0)).any())
    out = {}
    rays = [r.lens_rays(rs.width, rs.height, rs.seed, k).astype(np.float64) for k in range(rs.spp)]
    for (py, px) in pixels:
        o = np.stack([rays[k][py, px, :3] for k in range(rs.spp)])
        d = np.stack([rays[k][py, px, 3:] for k in range(rs.spp)])
        t = (5.0 - o[:, 1]) / d[:, 1]
        p = o + d * t[:, None]
        # every sample's first ray meets the floor top
        assert (t > 0).all() and ((p[:, [0, 2]] > 5.0) & (p[:, [0, 2]] < 19.0)).all()
        # no segment from a hit point to a corner of one emitter cube crosses another emitter cube (a cube is convex:
        # the corners' segments bound every target's), so nothing in the room occludes
        for cube in cubes:
            corners = np.array([[cube[0] + i * cube[3], cube[1] + j * cube[3], cube[2] + k * cube[3]]
                                for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64)
            for other in cubes:
                if other != cube:
                    box = (np.array(other[:3], np.float64), np.array(other[:3], np.float64) + other[3])
                    assert not crosses(p, corners, box)
        m16 = m32 = s32 = 0.0
        for cube in cubes:  # each cube's quadrature once, shared by the K = 1 and K = 2 cases
            key = (py, px, cube, rs.spp, rs.seed)
            if key not in _CUBE_MOMENTS:
                _CUBE_MOMENTS[key] = (E.estimator_moments(p, n, [cube], 16)[0],) + E.estimator_moments(p, n, [cube], 32)
            c16, c32, cs32 = _CUBE_MOMENTS[key]
            m16, m32, s32 = m16 + intensity * c16, m32 + intensity * c32, s32 + len(cubes) * intensity ** 2 * cs32
        var = np.maximum(s32 - m32 * m32, 0.0).sum()
        out[(py, px)] = (m32.mean(), np.sqrt(var) / rs.spp, np.abs(m32 - m16).mean())
    return out


@pytest.mark.parametrize("second", [False, True])
def test_lit_value(torch_cuda, renderer, second):
    """The floor's value under ONE at max_depth 2 is albedo * the estimator's expectation over the pixel's samples,
    within 5 standard errors of the reference's own variance plus the quadrature error; K = 2: the sum of two."""
    r, torch = renderer, torch_cuda
    r.set_emitter_sampling(NONE)
    sc = _room(r, second=second)
    rs = _room_settings(256, 2)
    floor, z, aov = _floor_hits(r, rs)
    assert floor.all()
    pixels = [(y, x) for y in (2, 6, 10, 13) for x in (1, 5, 9, 14)]
    cubes = [(*E.ROOM_EMITTER, 1)] + ([(*E.ROOM_EMITTER_2, 1)] if second else [])
    ref = _lit_reference(r, rs, cubes, aov["albedo"], pixels)
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
    got = gpu_render(torch, r, sc, E.room_camera(), rs, upload=False)[0]
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 0.0)
    black = gpu_render(torch, r, sc, E.room_camera(), rs, upload=False)[0]
    r.set_emitter_sampling(NONE)
    assert (black[..., :3] == 0.0).all()  # intensity 0
    for (py, px), (mean, se, q) in ref.items():
        for c in range(3):
            a = float(aov["albedo"][py, px, c])
            print(f"pixel ({px},{py}) ch {c}: gpu {got[py, px, c]:.6g} ref {a * mean:.6g} se {a * se:.3g} q {a * q:.3g}")
            assert abs(got[py, px, c] - a * mean) <= 5 * a * se + a * q


def test_sampling_lowers_the_variance(torch_cuda, renderer):
    """max_depth 3, 64 spp: the mean per-pixel luminance variance over the floor under ONE is below NONE's."""
    r = renderer
    r.set_emitter_sampling(NONE)
    _room(r)
    rs = _room_settings(64, 3)
    floor, _, _ = _floor_hits(r, rs)

    def variance():
        _, mom, _ = r.render_tiles(rs)
        v = mom[..., 1] - mom[..., 0] ** 2
        return float(v[floor].mean())

    v_none = variance()
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
    v_one = variance()
    r.set_emitter_sampling(NONE)
    print(f"variance ONE {v_one:.6g} NONE {v_none:.6g} ratio {v_one / v_none:.4g}")
    assert v_one < v_none


def test_estimator_is_consistent(torch_cuda, renderer):
    """With ONE in the lit room: a tile list of half the tiles, a [0, 0] context and the async frame give the full
    render's bits."""
    from octree_pathtracing_amd.renderer import HipRenderer

    r, torch = renderer, torch_cuda
    sc = _room(r, second=True)
    rs = _room_settings(16, 3)
    cam = E.room_camera()
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
    full = gpu_render(torch, r, sc, cam, rs, upload=False)
    assert full[0][..., :3].max() > 0.0
    # tile list: half of the four tiles
    acc, _, seg = r.render_tiles(rs, tiles=[0, 3])
    tiles = np.zeros((16, 16), bool)
    tiles[:8, :8] = tiles[8:, 8:] = True
    assert np.array_equal(acc[tiles].view(np.uint32), full[0][tiles].view(np.uint32))
    assert np.array_equal(seg[tiles], full[1][tiles])
    assert (acc[~tiles][:, :3] == 0.0).all() and (seg[~tiles] == 0).all()
    # the async frame
    host, _ = r.render(rs)
    assert np.array_equal(host.view(np.uint32), full[0].view(np.uint32))
    r.set_resolution((16, 16))
    r.reset_render()
    r.max_depth, r.seed = rs.max_depth, rs.seed
    r.render_frame(rs.spp).wait_for()
    assert np.array_equal(r.get_float_image().reshape(16, 16, 4).view(np.uint32), full[0].view(np.uint32))
    # two entries on one device
    with HipRenderer(devices=[0, 0]) as m:
        m.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
        m.set_scene(sc)
        m.set_camera(cam)
        two, _ = m.render(rs)
    assert np.array_equal(two.view(np.uint32), full[0].view(np.uint32))
    r.set_emitter_sampling(NONE)


def test_sun_and_emitters_add(torch_cuda, renderer):
    """Sun sampling together with ONE, in the room with its ceiling open to the sun: the emitter segment runs first,
    then the waiting sun sample's shadow segments, then the bounce.  The terms alone are rendered with the draws of
    the combined render -- the emitter term with the sun's direct light weighted 0 (luminosity_pdf 0 under
    sun_luminosity: `mult` is 0, nothing else reads it), the sun term with emitter intensity 0 -- so the combined
    render is not below either at any pixel, exactly, and above both on the mean.  And at max_depth 2 (own emittance at
    depth 1 under either strategy) ONE at intensity 0 must leave the sun render's radiance bit for bit: the sun
    sample that waited behind the emitter segment is the one NONE draws."""
    from octree_pathtracing_amd import scene as S

    r, torch = renderer, torch_cuda
    cam = E.room_camera()
    nee = S.SunSamplingStrategy(True, False, False, True, False)  # FAST with the sun's weight in luminosity_pdf

    def scene(pdf):
        sc = E.room_scene(second=True, hole=True)
        sc.strategy = nee
        sc.sun = S.Sun(luminosity_pdf=pdf)
        sc.build_octree(E.DEPTH)
        return sc

    def shot(sc, strategy, intensity, rs):
        r.set_emitter_sampling(NONE)
        r.set_scene(sc)
        r.set_emitter_sampling(strategy, E.ROOM_GRID, intensity)
        out = gpu_render(torch, r, sc, cam, rs, upload=False)
        r.set_emitter_sampling(NONE)
        return out

    rs = _room_settings(32, 3)
    lit, dark = scene(1.0), scene(0.0)
    both = shot(lit, ONE, 1.0, rs)
    emitters_alone = shot(dark, ONE, 1.0, rs)
    sun_alone = shot(lit, ONE, 0.0, rs)
    a, e, s = (x[0][..., :3].astype(np.float64) for x in (both, emitters_alone, sun_alone))
    print(f"mean both {a.mean():.6g} emitters alone {e.mean():.6g} sun alone {s.mean():.6g}")
    assert np.isfinite(both[0]).all()
    assert (a >= e).all() and (a >= s).all()
    assert a.mean() > e.mean() > 0.0 and a.mean() > s.mean() > 0.0
    assert np.array_equal(both[1], emitters_alone[1]) and np.array_equal(both[1], sun_alone[1])  # the same segments
    # the hand-over restores the sun sample exactly
    rs2 = _room_settings(16, 2)
    none = shot(lit, NONE, 1.0, rs2)
    zero = shot(lit, ONE, 0.0, rs2)
    assert np.array_equal(zero[0].view(np.uint32), none[0].view(np.uint32))
    assert (zero[1] >= none[1]).all() and zero[1].sum() > none[1].sum()
