"""Emissive block models as emitters on the device (OCTPT_EMITTERS_MODELS).

The flag is accepted and bad bits are refused; the device grid with torches equals the host builder's (itself pinned
to the numpy definition by tests/test_emitter_models_cpu.py) after each of the three scene paths, on a [0, 0] context
and across flag off -> on -> off, and the device's model table equals the host's; a world without an emissive model
renders bit for bit what it renders without the flag.  The estimator: exact occlusion behind a wall, the lit value
against the float64 statement of tests/emitter_models_ref.py within the reference's own standard error, less variance
than ONE without the flag, bit-identity across tile lists, devices and the async frame, and sun plus emitters."""
import ctypes as C

import numpy as np
import pytest

from tests import emitter_models_ref as M
from tests import emitter_ref as E
from tests.test_gpu_parity import gpu_render, renderer, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID_ARG = 1
NONE, ONE = 0, 1


def _set_scene(r, cells, path, compact=False):
    from octree_pathtracing_amd import scene as S

    sc = M.make_scene(cells)
    if path == "upload":
        sc.build_octree(M.DEPTH, compact=compact)
        r.set_scene(sc)
    elif path == "cells":
        r.set_scene_built(sc, M.DEPTH, compact=compact)
    else:
        r.set_scene_built_sections(sc, M.DEPTH, S.SectionWorld.from_cells(sc.cells_array(), M.DEPTH), compact=compact)
    return sc


def _host(cells, grid_size, compact=False, models=True):
    from octree_pathtracing_amd import scene as S

    return S.build_emitter_grid(M.make_scene(cells), M.DEPTH, grid_size, compact=compact, models=models)


def test_flag_is_accepted_and_bad_bits_are_refused(renderer):
    """flags = OCTPT_EMITTERS_MODELS is a setting (before this feature the word was reserved: INVALID_ARG); flags = 2
    and a non-zero later reserved word are INVALID_ARG and leave the held grid as it is."""
    from octree_pathtracing_amd import _lib

    r = renderer
    r.set_emitter_sampling(NONE)
    cells = M.random_world(0)
    _set_scene(r, cells, "upload")

    def status(strategy, flags, reserved_tail=0):
        p = _lib.EmitterParams(strategy, 4, 1.0)
        p.flags = flags
        p.reserved_tail[3] = reserved_tail
        return r._lib.octpt_set_emitter_sampling(r._ctx, C.byref(p))

    assert status(NONE, 1) == 0  # accepted under NONE, and means nothing: no grid
    with pytest.raises(_lib.OctptError):
        r.emitter_grid()
    assert status(ONE, 1) == 0
    held = r.emitter_grid()
    E.assert_same_grid(held, _host(cells, 4))
    assert (held["emitters"][:, 3] & M.MODEL_BIT).any()
    for flags, tail in ((2, 0), (3, 0), (0x80000000, 0), (1, 1), (0, 1)):
        assert status(ONE, flags, tail) == INVALID_ARG, (flags, tail)
        E.assert_same_grid(r.emitter_grid(), held)
    M.assert_same_table(r.emitter_models(), M.model_table(M.make_scene([])))
    r.set_emitter_sampling(NONE)


@pytest.mark.parametrize("path,compact", [("upload", False), ("upload", True), ("cells", True), ("sections", False)])
def test_device_grid_equals_host_grid(torch_cuda, path, compact):
    """On a [0, 0] context: flag off -> on -> off over one resident world of cubes and torches, at grid sizes 1, 4 and
    32; the device's model table is the host's."""
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import HipRenderer

    cells = M.random_world(1 if compact else 2)
    with HipRenderer(devices=[0, 0]) as r:
        r.set_emitter_sampling(ONE, 4, 1.0, models=True)  # the setting first: the scene call builds the grid
        sc = _set_scene(r, cells, path, compact)
        E.assert_same_grid(r.emitter_grid(), _host(cells, 4, compact))
        M.assert_same_table(r.emitter_models(), S.emitter_model_table(sc))
        for gs in (1, 32):
            r.set_emitter_sampling(ONE, gs, 1.0, models=False)
            E.assert_same_grid(r.emitter_grid(), _host(cells, gs, compact, models=False))
            with pytest.raises(_lib.OctptError) as e:
                r.emitter_models()
            assert e.value.status == INVALID_ARG
            r.set_emitter_sampling(ONE, gs, 1.0, models=True)
            got = r.emitter_grid()
            E.assert_same_grid(got, _host(cells, gs, compact))
            assert (got["emitters"][:, 3] & M.MODEL_BIT).any() and (~got["emitters"][:, 3] & M.MODEL_BIT).any()
            M.assert_same_table(r.emitter_models(), S.emitter_model_table(sc))
        r.set_emitter_sampling(ONE, 4, 1.0)
        E.assert_same_grid(r.emitter_grid(), _host(cells, 4, compact, models=False))


def test_no_emissive_model_changes_nothing(torch_cuda, renderer):
    """Cube emitters and models that do not emit: the flag leaves the grid and a 32 x 32, 4 spp, full-depth render as
    they are, bit for bit."""
    from octree_pathtracing_amd import scene as S

    r = renderer
    cam = S.Camera.look_at((28.0, 20.0, 30.0), (9.0, 9.0, 9.0))
    rs = S.RenderSettings(width=32, height=32, spp=4, max_depth=5, seed=3)
    r.set_emitter_sampling(NONE)
    sc = _set_scene(r, M.NO_EMISSIVE_MODEL, "upload")
    r.set_emitter_sampling(ONE, 4, 1.0)
    off_grid = r.emitter_grid()
    off = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
    r.set_emitter_sampling(ONE, 4, 1.0, models=True)
    on_grid = r.emitter_grid()
    on = gpu_render(torch_cuda, r, sc, cam, rs, upload=False)
    r.set_emitter_sampling(NONE)
    E.assert_same_grid(on_grid, off_grid)
    assert len(off_grid["emitters"]) == 2 and off[2]["segments"] > 0 and (off[0][..., :3] > 0).any()
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
    assert np.array_equal(on[1], off[1]) and on[2]["segments"] == off[2]["segments"]


# ------------------------------------------------------------------ the estimator (the room with a torch)
def _room(r, **kw):
    sc = M.room_scene(**kw)
    sc.build_octree(M.DEPTH)
    r.set_scene(sc)
    r.set_camera(E.room_camera())
    return sc


def _settings(spp, max_depth):
    from octree_pathtracing_amd import scene as S

    return S.RenderSettings(width=16, height=16, spp=spp, max_depth=max_depth, seed=5)


def _floor_hits(r, rs):
    aov = r.render_aov(rs, which=("normal", "depth", "prim", "albedo"))
    rays = r.camera_rays(rs.width, rs.height).reshape(rs.height, rs.width, 6)
    z = rays[..., 2] + rays[..., 5] * aov["depth"]
    floor = (aov["normal"][..., 1] == 1.0) & np.isfinite(aov["depth"])
    return floor, z, aov


def test_occlusion_is_exact(torch_cuda, renderer):
    """The torch behind a full wall: the floor on the camera's side stays exactly black at max_depth 2, and every
    sample traced camera, shadow and bounce segments (3) where the flag off traces 2."""
    r, torch = renderer, torch_cuda
    r.set_emitter_sampling(NONE)
    sc = _room(r, wall=True)
    rs = _settings(8, 2)
    floor, z, aov = _floor_hits(r, rs)
    sel = floor & (z < 13.0) & (z > 8.5)
    assert sel.sum() >= 64 and len(np.unique(aov["prim"][sel])) == 1
    cam = E.room_camera()
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
    assert len(r.emitter_grid()["emitters"]) == 0
    off = gpu_render(torch, r, sc, cam, rs, upload=False)
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0, models=True)
    assert r.emitter_grid()["emitters"].tolist() == [[*M.ROOM_TORCH, M.MODEL_BIT | M.M_TORCH]]
    on = gpu_render(torch, r, sc, cam, rs, upload=False)
    r.set_emitter_sampling(NONE)
    assert (on[0][sel][:, :3] == 0.0).all()
    assert (off[1][sel] == 2 * rs.spp).all() and (on[1][sel] == 3 * rs.spp).all()


_MOMENTS = {}


def _reference(r, rs, pixels, cube):
    """Per chosen pixel: expectation, standard error and quadrature error of the rendered value (per unit albedo) from
    the published first rays and the float64 estimator -- the rule of tests/test_gpu_emitters.py::test_lit_value."""
    n = np.array([0.0, 1.0, 0.0])
    K = 2 if cube else 1
    rays = [r.lens_rays(rs.width, rs.height, rs.seed, k).astype(np.float64) for k in range(rs.spp)]
    corner = np.array(M.ROOM_TORCH, np.float64)
    out = {}
    for (py, px) in pixels:
        o = np.stack([rays[k][py, px, :3] for k in range(rs.spp)])
        d = np.stack([rays[k][py, px, 3:] for k in range(rs.spp)])
        t = (5.0 - o[:, 1]) / d[:, 1]
        p = o + d * t[:, None]
        assert (t > 0).all() and ((p[:, [0, 2]] > 5.0) & (p[:, [0, 2]] < 19.0)).all()
        key = (py, px, rs.spp, rs.seed)
        if key not in _MOMENTS:
            _MOMENTS[key] = (M.torch_moments(p, n, corner, 32)[0],) + M.torch_moments(p, n, corner, 64)
        m_lo, m_hi, t_m2 = _MOMENTS[key]
        s_hi = K * t_m2
        if cube:
            # neither emitter shadows the other: no segment from a hit point to a corner of one's box crosses the
            # other's box (both are convex: the corners' segments bound every target's)
            boxes = [(np.array(M.ROOM_CUBE, np.float64), np.array(M.ROOM_CUBE, np.float64) + 1.0),
                     (corner + M.TORCH_BOX[0], corner + M.TORCH_BOX[1])]
            for (alo, ahi), (blo, bhi) in (boxes, boxes[::-1]):
                corners = np.array([[(alo, ahi)[i][0], (alo, ahi)[j][1], (alo, ahi)[k][2]]
                                    for i in (0, 1) for j in (0, 1) for k in (0, 1)])
                dd = corners[None, :, :] - p[:, None, :]
                with np.errstate(divide="ignore", invalid="ignore"):
                    t0, t1 = (blo - p[:, None, :]) / dd, (bhi - p[:, None, :]) / dd
                near, far = np.fmin(t0, t1).max(-1), np.fmax(t0, t1).min(-1)
                assert not ((near < far) & (far > 0.0) & (near < 1.0)).any()
            if ("cube",) + key not in _MOMENTS:
                _MOMENTS[("cube",) + key] = (E.estimator_moments(p, n, [(*M.ROOM_CUBE, 1)], 16)[0],) + \
                    E.estimator_moments(p, n, [(*M.ROOM_CUBE, 1)], 32)
            c_lo, c_hi, c_m2 = _MOMENTS[("cube",) + key]
            m_lo, m_hi, s_hi = m_lo + c_lo, m_hi + c_hi, s_hi + K * c_m2
        var = np.maximum(s_hi - m_hi * m_hi, 0.0).sum()
        out[(py, px)] = (m_hi.mean(), np.sqrt(var) / rs.spp, np.abs(m_hi - m_lo).mean())
    return out


@pytest.mark.parametrize("cube", [False, True])
def test_lit_value(torch_cuda, renderer, cube):
    """The floor's value at max_depth 2 and 256 spp is albedo * the estimator's expectation over the pixel's samples,
    within 5 standard errors of the reference's own variance plus the quadrature's error; with a cube emitter in the
    cell too (K = 2) the sum of the two; exactly black at intensity 0."""
    r, torch = renderer, torch_cuda
    r.set_emitter_sampling(NONE)
    sc = _room(r, cube=cube)
    rs = _settings(256, 2)
    floor, z, aov = _floor_hits(r, rs)
    assert floor.all()
    pixels = [(y, x) for y in (2, 6, 10, 13) for x in (1, 5, 9, 14)]
    ref = _reference(r, rs, pixels, cube)
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0, models=True)
    assert len(r.emitter_grid()["emitters"]) == (2 if cube else 1)
    got = gpu_render(torch, r, sc, E.room_camera(), rs, upload=False)[0]
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 0.0, models=True)
    black = gpu_render(torch, r, sc, E.room_camera(), rs, upload=False)[0]
    r.set_emitter_sampling(NONE)
    assert (black[..., :3] == 0.0).all()
    for (py, px), (mean, se, q) in ref.items():
        for c in range(3):
            a = float(aov["albedo"][py, px, c])
            print(f"pixel ({px},{py}) ch {c}: gpu {got[py, px, c]:.6g} ref {a * mean:.6g} se {a * se:.3g} q {a * q:.3g}")
            assert abs(got[py, px, c] - a * mean) <= 5 * a * se + a * q


def test_sampling_lowers_the_variance(torch_cuda, renderer):
    """max_depth 3, 64 spp: the mean per-pixel luminance variance over the floor with the flag is below ONE's without
    it (whose grid lists nothing in this room: the torch's light arrives by blind bounces alone)."""
    r = renderer
    r.set_emitter_sampling(NONE)
    _room(r)
    rs = _settings(64, 3)
    floor, _, _ = _floor_hits(r, rs)

    def variance():
        _, mom, _ = r.render_tiles(rs)
        v = mom[..., 1] - mom[..., 0] ** 2
        return float(v[floor].mean())

    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0)
    v_off = variance()
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0, models=True)
    v_on = variance()
    r.set_emitter_sampling(NONE)
    print(f"variance with models {v_on:.6g} without {v_off:.6g} ratio {v_on / v_off:.4g}")
    assert v_on < v_off


def test_estimator_is_consistent(torch_cuda, renderer):
    """With the flag in the lit room (a torch and a cube): a tile list of half the tiles, a [0, 0] context and the
    async frame give the full render's bits."""
    from octree_pathtracing_amd.renderer import HipRenderer

    r, torch = renderer, torch_cuda
    sc = _room(r, cube=True)
    rs = _settings(16, 3)
    cam = E.room_camera()
    r.set_emitter_sampling(ONE, E.ROOM_GRID, 1.0, models=True)
    full = gpu_render(torch, r, sc, cam, rs, upload=False)
    assert full[0][..., :3].max() > 0.0
    acc, _, seg = r.render_tiles(rs, tiles=[0, 3])
    tiles = np.zeros((16, 16), bool)
    tiles[:8, :8] = tiles[8:, 8:] = True
    assert np.array_equal(acc[tiles].view(np.uint32), full[0][tiles].view(np.uint32))
    assert np.array_equal(seg[tiles], full[1][tiles])
    assert (acc[~tiles][:, :3] == 0.0).all() and (seg[~tiles] == 0).all()
    host, _ = r.render(rs)
    assert np.array_equal(host.view(np.uint32), full[0].view(np.uint32))
    r.set_resolution((16, 16))
    r.reset_render()
    r.max_depth, r.seed = rs.max_depth, rs.seed
    r.render_frame(rs.spp).wait_for()
    assert np.array_equal(r.get_float_image().reshape(16, 16, 4).view(np.uint32), full[0].view(np.uint32))
    sc.emitter_sampling, sc.emitter_grid_size, sc.emitter_models = ONE, E.ROOM_GRID, True  # carried by set_scene
    with HipRenderer(devices=[0, 0]) as m:
        m.set_scene(sc)
        m.set_camera(cam)
        assert (m.emitter_grid()["emitters"][:, 3] & M.MODEL_BIT).any()
        two, _ = m.render(rs)
    assert np.array_equal(two.view(np.uint32), full[0].view(np.uint32))
    r.set_emitter_sampling(NONE)


def test_sun_and_model_emitters_add(torch_cuda, renderer):
    """Sun sampling together with the flag, in the room with its ceiling open: with the draws of the combined render,
    the result is pixel for pixel not below the emitter-only render (the sun's direct light weighted 0) nor the
    sun-only render (intensity 0); and at max_depth 2 with intensity 0 it equals the sun render without emitter
    sampling bit for bit."""
    from octree_pathtracing_amd import scene as S

    r, torch = renderer, torch_cuda
    cam = E.room_camera()
    nee = S.SunSamplingStrategy(True, False, False, True, False)

    def scene(pdf):
        sc = M.room_scene(cube=True, hole=True)
        sc.strategy = nee
        sc.sun = S.Sun(luminosity_pdf=pdf)
        sc.build_octree(M.DEPTH)
        return sc

    def shot(sc, strategy, intensity, rs):
        r.set_emitter_sampling(NONE)
        r.set_scene(sc)
        r.set_emitter_sampling(strategy, E.ROOM_GRID, intensity, models=True)
        out = gpu_render(torch, r, sc, cam, rs, upload=False)
        r.set_emitter_sampling(NONE)
        return out

    rs = _settings(32, 3)
    lit, dark = scene(1.0), scene(0.0)
    both = shot(lit, ONE, 1.0, rs)
    emitters_alone = shot(dark, ONE, 1.0, rs)
    sun_alone = shot(lit, ONE, 0.0, rs)
    a, e, s = (x[0][..., :3].astype(np.float64) for x in (both, emitters_alone, sun_alone))
    print(f"mean both {a.mean():.6g} emitters alone {e.mean():.6g} sun alone {s.mean():.6g}")
    assert np.isfinite(both[0]).all()
    assert (a >= e).all() and (a >= s).all()
    assert a.mean() > e.mean() > 0.0 and a.mean() > s.mean() > 0.0
    assert np.array_equal(both[1], emitters_alone[1]) and np.array_equal(both[1], sun_alone[1])
    rs2 = _settings(16, 2)
    none = shot(lit, NONE, 1.0, rs2)
    zero = shot(lit, ONE, 0.0, rs2)
    assert np.array_equal(zero[0].view(np.uint32), none[0].view(np.uint32))
    assert (zero[1] >= none[1]).all() and zero[1].sum() > none[1].sum()
