"""Adaptive sampling on the GPU (octpt_render_tiles_device, the samples' luminance moments in resolve, octpt_tile_error
and octpt_render_adaptive) against octpt_render_device, bit for bit, and against the numpy
restatement (tests/adaptive_ref.py) within the project's forward tolerance.

Scene C3 at 64 x 64 (every tile inside the image: the direct seed and its 16-B camera-ray records) and 37 x 21 (a
5 x 3 tile grid overhanging both edges); both hold hit and miss pixels.  At most 16 samples.

The regeneration path (a pool smaller than the chunk) is reached with OCTPT_POOL, as tests/test_gpu_beam.py and
tests/test_gpu_tile_order.py reach it: OCTPT_DEVICE_MEM_LIMIT cannot put the pool below a chunk of these sizes, since
the out-of-memory fallback stops halving at 2^20 slots and a 64 x 64 x 16 spp chunk holds 2^16 items.  That the path
was taken is asserted through octpt_stats.pool_slots < the chunk's items.

The variance of a pixel is the difference m2 - m1^2 of two quantities that are each checked at REL / ABS; its bound
is the sum of theirs, REL * (m2 + 2 m1^2) + 2 ABS (m1^2 carries twice m1's relative error)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.adaptive_ref import (adaptive_loop, luminance, sample_moments_ref, tile_error_ref, tile_grid, tile_mask)

pytestmark = pytest.mark.gpu

F32 = np.float32
F64 = np.float64
REL, ABS = 1e-5, 1e-6  # the project's forward tolerance, as tests/test_gpu_denoise.py
SIZES = [(64, 64), (37, 21)]
IDS = ["64x64", "37x21"]
FLOOR = 1e-2


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _renderer_with(env, **kw):
    """A HipRenderer created under `env` (read at octpt_create), with C3 uploaded."""
    from octree_pathtracing_amd.renderer import HipRenderer

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        r = HipRenderer(**(kw or {"device": 0}))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    sc, cam, _ = c3()
    r.set_scene(sc)
    r.set_camera(cam)
    return r


_c3 = []


def c3():
    from octree_pathtracing_amd import scene as S

    if not _c3:
        _c3.append(S.make_config("C3"))
    return _c3[0]


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    r = _renderer_with({})
    yield r
    r.close()


def close(got, ref):
    return np.abs(got - ref) <= REL * np.abs(ref) + ABS


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def black(W, H):
    a = np.zeros((H, W, 4), F32)
    a[..., 3] = 1.0
    return a


def sentinel(W, H):
    """accum, moments and seg_count filled with a pattern no render produces by chance."""
    i = np.arange(W * H, dtype=np.uint32)
    acc = (0x3F000000 + 4 * i[:, None] + np.arange(4, dtype=np.uint32)).view(F32).reshape(H, W, 4).copy()
    mom = (0x3E000000 + 2 * i[:, None] + np.arange(2, dtype=np.uint32)).view(F32).reshape(H, W, 2).copy()
    seg = (1000 + i).reshape(H, W).copy()
    return acc, mom, seg


class Frames:
    """accum / moments / seg_count of one W x H frame on the device, as torch tensors."""

    def __init__(self, torch, W, H, accum=None, moments=None, seg=None):
        self.torch, self.W, self.H = torch, W, H
        self.acc = torch.from_numpy(np.ascontiguousarray(black(W, H) if accum is None else accum, F32)).cuda()
        self.mom = torch.from_numpy(np.ascontiguousarray(np.zeros((H, W, 2), F32) if moments is None else moments)).cuda()
        s = np.zeros((H, W), np.uint32) if seg is None else np.ascontiguousarray(seg, np.uint32)
        self.seg = torch.from_numpy(s.view(np.int32)).cuda()

    def host(self):
        self.torch.cuda.synchronize()
        return self.acc.cpu().numpy(), self.mom.cpu().numpy(), self.seg.cpu().numpy().view(np.uint32)


def params(r, W, H, spp_start, spp, branch_count=1, **kw):
    _, _, rs = c3()
    r.max_depth, r.seed, r.branch_count = rs.max_depth, rs.seed, branch_count
    p = r.params(W, H, spp_start, spp, **kw)
    r.branch_count = 1
    return p


def render_full(torch, r, W, H, spp, spp_start=0, accum=None, seg=None, branch_count=1):
    """octpt_render_device -> (accum, seg_count)."""
    f = Frames(torch, W, H, accum, None, seg)
    r.render_device(params(r, W, H, spp_start, spp, branch_count), f.acc.data_ptr(), f.seg.data_ptr())
    a, _, s = f.host()
    return a, s


def render_tiles(torch, r, W, H, spp, tiles, spp_start=0, accum=None, moments=None, seg=None, branch_count=1,
                 with_moments=True):
    """octpt_render_tiles_device -> (accum, moments, seg_count)."""
    f = Frames(torch, W, H, accum, moments, seg)
    r.render_tiles_device(params(r, W, H, spp_start, spp, branch_count), tiles, f.acc.data_ptr(),
                          f.mom.data_ptr() if with_moments else None, f.seg.data_ptr())
    return f.host()


def half_list(W, H):
    """About half the tiles in a scrambled order: the four corner tiles (at 37 x 21 the last column and row overhang)
    and every second tile of the rest."""
    tx, ty = tile_grid(W, H)
    T = tx * ty
    corners = [0, tx - 1, T - tx, T - 1]
    rest = [t for t in range(T) if t not in corners][::2]
    lst = corners + rest
    lst = lst[::-1][: max(T // 2, len(corners))]
    for t in corners:
        if t not in lst:
            lst.append(t)
    return np.asarray(lst, np.uint32)


_ref = {}


def full_ref(torch, r, W, H, spp):
    """The plain render the tile-list renders are compared with, computed once per size and sample count."""
    if (W, H, spp) not in _ref:
        _ref[(W, H, spp)] = render_full(torch, r, W, H, spp)
    return _ref[(W, H, spp)]


# ---------------------------------------------------------------------------------------------- 1: list = full render
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_whole_list_equals_render_device(torch_cuda, renderer, size):
    W, H = size
    T = int(np.prod(tile_grid(W, H)))
    ref_a, ref_s = full_ref(torch_cuda, renderer, W, H, 4)
    for tiles in (None, np.arange(T, dtype=np.uint32)[::-1]):
        a, _, s = render_tiles(torch_cuda, renderer, W, H, 4, tiles)
        assert same(a, ref_a) and np.array_equal(s, ref_s)
    # continuing a 4-spp accumulation
    ref8_a, ref8_s = render_full(torch_cuda, renderer, W, H, 4, 4, ref_a, ref_s)
    for tiles in (None, np.arange(T, dtype=np.uint32)[::-1]):
        a, _, s = render_tiles(torch_cuda, renderer, W, H, 4, tiles, 4, ref_a, None, ref_s)
        assert same(a, ref8_a) and np.array_equal(s, ref8_s)
    assert same(ref8_a, full_ref(torch_cuda, renderer, W, H, 8)[0])


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_whole_list_with_branch_schedule(torch_cuda, renderer, size):
    """branch_count = 10 over whole passes: 0, 1, 2, 3 alone, then a pass of weight 6 -> 10 samples."""
    from octree_pathtracing_amd.renderer import branch_pass_end

    W, H = size
    T = int(np.prod(tile_grid(W, H)))
    n = branch_pass_end(0, 5, 10)
    assert n == 10
    ref_a, ref_s = render_full(torch_cuda, renderer, W, H, n, branch_count=10)
    for tiles in (None, np.arange(T, dtype=np.uint32)[::-1]):
        a, m, s = render_tiles(torch_cuda, renderer, W, H, n, tiles, branch_count=10)
        assert same(a, ref_a) and np.array_equal(s, ref_s)
        assert np.all(np.isfinite(m)) and np.all(m[..., 1] >= 0)


# ---------------------------------------------------------------------------------------------- 2, 3: a subset
def check_subset(torch, r, W, H, spp=4):
    from octree_pathtracing_amd import _lib

    lst = half_list(W, H)
    tx, ty = tile_grid(W, H)
    assert 0 in lst and tx * ty - 1 in lst and tx - 1 in lst and len(set(lst.tolist())) == len(lst) < tx * ty
    inside = tile_mask(W, H, lst)
    assert inside.any() and (~inside).any()
    # the listed tiles from black: the full render's pixels
    ref_a, ref_s = full_ref(torch, r, W, H, spp)
    ref_m = render_tiles(torch, r, W, H, spp, None)[1]
    sa, sm, ss = sentinel(W, H)
    start_a = np.where(inside[..., None], black(W, H), sa)
    start_m = np.where(inside[..., None], F32(0), sm)
    start_s = np.where(inside, np.uint32(0), ss)
    r.reset_stats()
    a, m, s = render_tiles(torch, r, W, H, spp, lst, 0, start_a, start_m, start_s)
    st = r.stats()
    assert same(a[inside], ref_a[inside]) and same(m[inside], ref_m[inside]) and np.array_equal(s[inside], ref_s[inside])
    assert same(a[~inside], sa[~inside]) and same(m[~inside], sm[~inside]) and np.array_equal(s[~inside], ss[~inside])
    assert st["paths"] == int(inside.sum()) * spp, "octpt_stats counts the listed tiles' paths only"
    # refused lists leave everything untouched
    for bad in (np.append(lst, lst[0]), np.append(lst[:3], np.uint32(tx * ty))):
        f = Frames(torch, W, H, sa, sm, ss)
        with pytest.raises(_lib.OctptError) as ei:
            r.render_tiles_device(params(r, W, H, 0, spp), bad, f.acc.data_ptr(), f.mom.data_ptr(), f.seg.data_ptr())
        assert ei.value.status == _lib.ERR_INVALID_ARG
        a2, m2, s2 = f.host()
        assert same(a2, sa) and same(m2, sm) and np.array_equal(s2, ss)
    return st, len(lst)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_subset_leaves_the_rest_untouched(torch_cuda, renderer, size):
    check_subset(torch_cuda, renderer, *size)


def test_subset_with_regeneration(torch_cuda, renderer):
    """A pool of 4096 slots under the subset's chunk: the seed claims items and finished paths regenerate."""
    full_ref(torch_cuda, renderer, 64, 64, 4)  # from the ordinary context
    small = _renderer_with({"OCTPT_POOL": "4096"})
    try:
        st, n = check_subset(torch_cuda, small, 64, 64)
        assert st["pool_slots"] < 64 * n * 4, st
    finally:
        small.close()


# ---------------------------------------------------------------------------------------------- 4: the beam-start cache
def test_ordinary_render_after_tile_lists_with_beam(torch_cuda, renderer):
    """With the camera rays' beam starts on, a tile-list render computes only its tiles' starts.  The table it leaves
    must not serve the next ordinary render, nor a list of other tiles: the unlisted entries were computed for another
    camera."""
    from tests.test_gpu_svgf import moved

    W, H = 64, 64
    _, cam0, _ = c3()
    cam1 = moved(cam0, right=3.0, up=-1.0, forward=2.0, yaw=0.02)
    r = _renderer_with({"OCTPT_BEAM": "1"})
    try:
        r.set_camera(cam1)
        r.reset_stats()
        ref_a, ref_s = render_full(torch_cuda, r, W, H, 4)
        ref_st = r.stats()
        r.set_camera(cam0)
        render_full(torch_cuda, r, W, H, 4)  # the table now holds cam0's starts
        r.set_camera(cam1)
        lst = half_list(W, H)
        others = np.asarray([t for t in range(64) if t not in lst], np.uint32)
        a, _, s = render_tiles(torch_cuda, r, W, H, 4, lst)
        a, _, s = render_tiles(torch_cuda, r, W, H, 4, others, 0, a, None, s)  # a list of the other tiles
        assert same(a, ref_a) and np.array_equal(s, ref_s)
        r.reset_stats()
        a, s = render_full(torch_cuda, r, W, H, 4)  # the ordinary render, as before
        st = r.stats()
        assert same(a, ref_a) and np.array_equal(s, ref_s)
        assert st["esvo_steps"] == ref_st["esvo_steps"] and st["segments"] == ref_st["segments"]
        # and the renders without the beam agree (tests/test_gpu_beam.py's property)
        renderer.set_camera(cam1)
        try:
            b, sb = render_full(torch_cuda, renderer, W, H, 4)
        finally:
            renderer.set_camera(cam0)
        assert same(b, ref_a) and np.array_equal(sb, ref_s)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 5: moments
_samples = {}


def sample_colours(torch, r, W, H, n=8):
    """[n, H, W, 3] f64: sample i's colour, recovered from a 1-spp render at spp_start = i into a black buffer
    (accum = c / (i + 1) there), times i + 1."""
    if (W, H) not in _samples:
        cs = [render_full(torch, r, W, H, 1, i)[0][..., :3].astype(F64) * (i + 1) for i in range(n)]
        _samples[(W, H)] = np.stack(cs)
    return _samples[(W, H)]


_moments = {}


def rendered_moments(torch, r, W, H):
    """(accum, moments) of 8 spp in one call, computed once."""
    if (W, H) not in _moments:
        a, m, _ = render_tiles(torch, r, W, H, 8, None)
        _moments[(W, H)] = (a, m)
    return _moments[(W, H)]


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_moments(torch_cuda, renderer, size):
    from octree_pathtracing_amd.scene import RenderSettings

    W, H = size
    a8, m8 = rendered_moments(torch_cuda, renderer, W, H)
    # accum with the moments equals accum without, and the plain render
    a_plain, _, _ = render_tiles(torch_cuda, renderer, W, H, 8, None, with_moments=False)
    assert same(a8, a_plain) and same(a8, full_ref(torch_cuda, renderer, W, H, 8)[0])
    # 8 spp in one call = 4 + 4 in two
    a4, m4, s4 = render_tiles(torch_cuda, renderer, W, H, 4, None)
    a44, m44, _ = render_tiles(torch_cuda, renderer, W, H, 4, None, 4, a4, m4, s4)
    assert same(a44, a8) and same(m44, m8)
    # against the f64 means of the per-sample colours
    cs = sample_colours(torch_cuda, renderer, W, H)
    ref = sample_moments_ref(cs)
    ok = close(m8.astype(F64), ref)
    assert ok.all(), (np.abs(m8 - ref) / (REL * np.abs(ref) + ABS)).max()
    # miss pixels: the variance is that of the jittered sky samples, and v is never negative
    miss = ~np.isfinite(renderer.render_aov(RenderSettings(W, H, 1), which=("depth",))["depth"])
    assert miss.any() and (~miss).any()
    l = luminance(cs)
    var_ref = (l * l).mean(0) - l.mean(0) ** 2
    d = m8[..., 1].astype(F64) - m8[..., 0].astype(F64) ** 2
    tol = REL * (ref[..., 1] + 2 * ref[..., 0] ** 2) + 2 * ABS
    assert np.all(np.abs(d - var_ref)[miss] <= tol[miss]), (np.abs(d - var_ref) / tol)[miss].max()
    d32 = m8[..., 1] - m8[..., 0] * m8[..., 0]
    v = np.where(d32 < 0, F32(0), d32)
    assert np.all(v[miss] >= 0) and np.all(np.isfinite(v[miss])) and np.all(d32[miss] >= -tol[miss])


# ---------------------------------------------------------------------------------------------- 6: tile error
def tile_error_device(torch, r, moments, tile_spp, floor=FLOOR):
    from octree_pathtracing_amd import _lib

    H, W = moments.shape[:2]
    m = torch.from_numpy(np.ascontiguousarray(moments, F32)).cuda()
    n = torch.from_numpy(np.ascontiguousarray(tile_spp, np.uint32).view(np.int32)).cuda()
    e = torch.full((len(tile_spp),), -1.0, dtype=torch.float32, device="cuda")
    r.tile_error_device(_lib.TileErrorParams(W, H, floor), m.data_ptr(), n.data_ptr(), e.data_ptr())
    torch.cuda.synchronize()
    return e.cpu().numpy()


def assert_errors(got, ref):
    inf = np.isposinf(ref)
    assert np.array_equal(np.isposinf(got), inf) and not np.isnan(got).any()
    assert close(got[~inf].astype(F64), ref[~inf]).all(), (got, ref)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_tile_error(torch_cuda, renderer, size):
    W, H = size
    T = int(np.prod(tile_grid(W, H)))
    _, m8 = rendered_moments(torch_cuda, renderer, W, H)
    spp = np.full(T, 8, np.uint32)
    ref = tile_error_ref(m8, spp, FLOOR)
    assert np.isfinite(ref).all() and (ref > 0).any()
    dev = tile_error_device(torch_cuda, renderer, m8, spp)
    host = renderer.tile_error(m8, spp, FLOOR)
    assert_errors(dev, ref)  # overhanging tiles included at 37 x 21
    assert_errors(host, ref)
    assert same(dev, host)
    # synthetic moments: a zero-variance tile, tiles of 0 and 1 samples, a NaN moment
    rng = np.random.default_rng(5)
    m = np.empty((H, W, 2), F32)
    m[..., 0] = rng.random((H, W), F32) + F32(0.1)
    m[..., 1] = m[..., 0] * m[..., 0] + rng.random((H, W), F32)
    flat = tile_mask(W, H, [1])
    m[flat, 1] = (m[flat, 0] * m[flat, 0])
    nan_at = np.argwhere(tile_mask(W, H, [T - 1]))[-1]  # the last pixel of the last (overhanging) tile
    m[nan_at[0], nan_at[1], 1] = np.nan
    spp = np.full(T, 5, np.uint32)
    spp[2], spp[3] = 0, 1
    ref = tile_error_ref(m, spp, FLOOR)
    dev = tile_error_device(torch_cuda, renderer, m, spp)
    assert ref[1] == 0 and dev[1] == 0
    assert np.isposinf(dev[[2, 3, T - 1]]).all()
    assert_errors(dev, ref)
    assert_errors(renderer.tile_error(m, spp, FLOOR), ref)


# ---------------------------------------------------------------------------------------------- 7: the driver
def composed(torch, r, W, H, min_spp, step_spp, max_spp, threshold):
    """The header's loop composed from render_tiles_device and tile_error_device -> (accum, moments, tile_spp, last
    errors, rounds, wave_allocs after round 1 and at the end)."""
    from octree_pathtracing_amd import _lib

    T = int(np.prod(tile_grid(W, H)))
    f = Frames(torch, W, H)
    d_err = torch.zeros(T, dtype=torch.float32, device="cuda")
    allocs = []

    def render(active, start, count):
        r.render_tiles_device(params(r, W, H, start, count), np.asarray(active, np.uint32), f.acc.data_ptr(),
                              f.mom.data_ptr(), None)
        allocs.append(r.stats()["wave_allocs"])

    def error(tile_spp):
        d_spp = torch.from_numpy(tile_spp.view(np.int32)).cuda()
        r.tile_error_device(_lib.TileErrorParams(W, H, FLOOR), f.mom.data_ptr(), d_spp.data_ptr(), d_err.data_ptr())
        torch.cuda.synchronize()
        return d_err.cpu().numpy()

    tile_spp, err, rounds = adaptive_loop(T, render, error, min_spp, step_spp, max_spp, threshold)
    a, m, _ = f.host()
    return a, m, tile_spp, err, rounds, allocs


def adaptive_device(torch, r, W, H, min_spp, step_spp, max_spp, threshold):
    from octree_pathtracing_amd import _lib

    sa, sm, _ = sentinel(W, H)  # outputs: the call initialises them
    f = Frames(torch, W, H, sa, sm)
    tile_spp, res = r.render_adaptive_device(params(r, W, H, 0, max_spp),
                                             _lib.AdaptiveParams(min_spp, step_spp, threshold, FLOOR),
                                             f.acc.data_ptr(), f.mom.data_ptr())
    a, m, _ = f.host()
    return a, m, tile_spp, res


def first_round_errors(torch, r, W, H):
    _, m4, _ = render_tiles(torch, r, W, H, 4, None)
    T = int(np.prod(tile_grid(W, H)))
    return tile_error_device(torch, r, m4, np.full(T, 4, np.uint32))


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_adaptive_driver(torch_cuda, renderer, size):
    from octree_pathtracing_amd.scene import RenderSettings

    W, H = size
    _, _, rs = c3()
    e1 = first_round_errors(torch_cuda, renderer, W, H)
    threshold = float(np.median(e1[np.isfinite(e1)]))
    assert threshold > 0
    fresh = _renderer_with({})  # a context of its own: its wavefront state is first sized by round 1
    try:
        a, m, tile_spp, err, rounds, allocs = composed(torch_cuda, fresh, W, H, 4, 4, 16, threshold)
    finally:
        fresh.close()
    assert (tile_spp == 4).any() and (tile_spp > 4).any(), "tiles that stopped at 4 and tiles that went on"
    assert allocs[0] >= 1 and allocs[-1] == allocs[0], "shrinking lists do not reallocate the wavefront state"
    assert np.all(err[tile_spp < 16] <= threshold)
    da, dm, d_spp, res = adaptive_device(torch_cuda, renderer, W, H, 4, 4, 16, threshold)
    assert same(da, a) and same(dm, m) and np.array_equal(d_spp, tile_spp)
    assert res == dict(rounds=rounds, tile_samples=int(tile_spp.sum()), converged_tiles=int((err <= threshold).sum()),
                       total_tiles=len(tile_spp))
    assert res["tile_samples"] == int(d_spp.astype(np.uint64).sum())
    # the host form
    settings = RenderSettings(W, H, 16, max_depth=rs.max_depth, seed=rs.seed)
    ha, hm, h_spp, hres = renderer.render_adaptive(settings, 4, 4, threshold, FLOOR, with_rgba=True)
    rgba = hres.pop("rgba")
    assert same(ha, da) and same(hm, dm) and np.array_equal(h_spp, d_spp) and hres == res
    assert rgba.shape == (H, W, 4) and rgba.any()
    # a huge threshold: one round, every tile at 4
    a4, _, spp4, res4 = adaptive_device(torch_cuda, renderer, W, H, 4, 4, 16, 3e38)
    finite = np.isfinite(e1)
    assert res4["rounds"] == 1 and np.all(spp4 == 4) and res4["converged_tiles"] == int(finite.sum())
    assert same(a4, full_ref(torch_cuda, renderer, W, H, 4)[0])
    # a tiny one: every tile with any error at all runs to the cap, and is the plain 16-spp render there
    a16, _, spp16, res16 = adaptive_device(torch_cuda, renderer, W, H, 4, 4, 16, 1e-30)
    assert np.all(spp16[e1 > 0] == 16) and np.all(spp16[e1 == 0] == 4) and (spp16 == 16).any()
    at16 = tile_mask(W, H, np.flatnonzero(spp16 == 16))
    assert same(a16[at16], full_ref(torch_cuda, renderer, W, H, 16)[0][at16])
    assert res16["tile_samples"] == int(spp16.sum())


# ---------------------------------------------------------------------------------------------- 8: refusals
def test_refusals(torch_cuda, renderer):
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd.renderer import HipRenderer

    W, H = 64, 64
    sa, sm, ss = sentinel(W, H)
    f = Frames(torch_cuda, W, H, sa, sm, ss)
    ok_a = _lib.AdaptiveParams(4, 4, 0.1, FLOOR)

    def tiles_status(r, p, tiles=None):
        try:
            r.render_tiles_device(p, tiles, f.acc.data_ptr(), f.mom.data_ptr(), f.seg.data_ptr())
        except _lib.OctptError as e:
            return e.status
        return _lib.OK

    def adaptive_status(r, p, a):
        try:
            r.render_adaptive_device(p, a, f.acc.data_ptr(), f.mom.data_ptr())
        except _lib.OctptError as e:
            return e.status
        return _lib.OK

    both = lambda r, p: (tiles_status(r, p), adaptive_status(r, p, ok_a))  # noqa: E731
    inv, uns = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    assert both(renderer, params(renderer, W, H, 0, 4, shard_index=0, shard_count=2)) == (inv, inv)
    assert both(renderer, params(renderer, W, H, 0, 4, compact=True)) == (inv, inv)
    assert both(renderer, params(renderer, W, H, 0, 4, megakernel=True)) == (uns, uns)
    assert both(renderer, params(renderer, W, H, 0, 4, preview=True)) == (uns, uns)
    renderer.set_tile_order(W, H, np.arange(64, dtype=np.uint32)[::-1].copy())
    try:
        assert both(renderer, params(renderer, W, H, 0, 4)) == (inv, inv)
    finally:
        renderer.set_tile_order(W, H, None)
    multi = HipRenderer(devices=[0, 0])
    try:
        sc, cam, _ = c3()
        multi.set_scene(sc)
        multi.set_camera(cam)
        assert both(multi, params(multi, W, H, 0, 4)) == (uns, uns)
    finally:
        multi.close()
    # an empty list: OK, nothing launched
    renderer.reset_stats()
    assert tiles_status(renderer, params(renderer, W, H, 0, 4), np.zeros(0, np.uint32)) == _lib.OK
    assert renderer.stats()["paths"] == 0
    # the driver's own
    assert adaptive_status(renderer, params(renderer, W, H, 4, 8), ok_a) == inv  # spp_start != 0
    assert adaptive_status(renderer, params(renderer, W, H, 0, 8), _lib.AdaptiveParams(1, 4, 0.1, FLOOR)) == inv
    assert adaptive_status(renderer, params(renderer, W, H, 0, 8), _lib.AdaptiveParams(4, 0, 0.1, FLOOR)) == inv
    assert adaptive_status(renderer, params(renderer, W, H, 0, 2), ok_a) == inv  # the cap below min_spp
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert adaptive_status(renderer, params(renderer, W, H, 0, 8), _lib.AdaptiveParams(4, 4, bad, FLOOR)) == inv
        assert adaptive_status(renderer, params(renderer, W, H, 0, 8), _lib.AdaptiveParams(4, 4, 0.1, bad)) == inv
    assert adaptive_status(renderer, params(renderer, W, H, 0, 10, branch_count=10), ok_a) == uns
    a, m, s = f.host()
    assert same(a, sa) and same(m, sm) and np.array_equal(s, ss), "a refused call leaves the buffers untouched"
