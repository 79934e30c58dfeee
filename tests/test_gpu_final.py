"""Final-quality adaptive frames on the GPU: the sample clamp in resolve, the seam rule's spread
of the tile error, the variance of the pixel means from the sample moments, the _ex driver and octpt_render_final,
against the existing entries bit for bit and against the numpy restatement (tests/final_ref.py).

Scenes and sizes are tests/test_gpu_adaptive.py's: C3 at 64 x 64 (every tile inside the image) and 37 x 21 (a 5 x 3
tile grid overhanging both edges), at most 16 samples.  Where a comparison is not bit-exact the tolerance is the
project's forward one, REL, ABS = 1e-5, 1e-6; the variance m2 - m1^2 of a clamped render carries the bound of
tests/test_gpu_adaptive.py's docstring, REL * (m2 + 2 m1^2) + 2 ABS."""
import contextlib

import numpy as np
import pytest

from tests import svgf_ref
from tests.adaptive_ref import luminance, sample_moments_ref, tile_grid, tile_mask
from tests.final_ref import adaptive_loop_ex, clamp_samples, neighbours, sample_variance_ref, spread_ref
from tests.test_gpu_adaptive import (ABS, FLOOR, IDS, REL, SIZES, Frames, _renderer_with, bits, black, c3, close,
                                     first_round_errors, half_list, params, render_full, render_tiles, rendered_moments,
                                     same, sample_colours, sentinel, tile_error_device)

pytestmark = pytest.mark.gpu

F32 = np.float32
F64 = np.float64
WEIGHTS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    r = _renderer_with({})
    yield r
    r.close()


@contextlib.contextmanager
def clamped(r, value):
    r.set_sample_clamp(value)
    try:
        yield r
    finally:
        r.set_sample_clamp(0.0)


def status_of(call, *a, **kw):
    from octree_pathtracing_amd import _lib

    try:
        call(*a, **kw)
    except _lib.OctptError as e:
        return e.status
    return _lib.OK


def median_clamp(torch, r, W, H):
    """The median positive luminance of the 8 per-sample colours of every pixel, as the f32 the library is given."""
    l = luminance(sample_colours(torch, r, W, H))
    return float(F32(np.median(l[l > 0])))


# ---------------------------------------------------------------------------------------------- 1: clamp off is today
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_clamp_off_is_today(torch_cuda, renderer, size):
    W, H = size
    fresh = _renderer_with({})
    try:
        ref_a, ref_s = render_full(torch_cuda, fresh, W, H, 8)
        ref_ta, ref_tm, ref_ts = render_tiles(torch_cuda, fresh, W, H, 8, None)
    finally:
        fresh.close()
    for value in (3e38, 0.0, float("inf")):
        with clamped(renderer, value):
            a, s = render_full(torch_cuda, renderer, W, H, 8)
            ta, tm, ts = render_tiles(torch_cuda, renderer, W, H, 8, None)
        assert same(a, ref_a) and np.array_equal(s, ref_s), value
        assert same(ta, ref_ta) and same(tm, ref_tm) and np.array_equal(ts, ref_ts), value


# ---------------------------------------------------------------------------------------------- 2: against the samples
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_clamp_against_the_samples(torch_cuda, renderer, size):
    W, H = size
    cs = sample_colours(torch_cuda, renderer, W, H)
    clamp = median_clamp(torch_cuda, renderer, W, H)
    l = luminance(cs)
    assert (l > clamp).any() and (l < clamp).any() and clamp > 0
    _, _, s_plain = render_tiles(torch_cuda, renderer, W, H, 8, None)
    with clamped(renderer, clamp):
        a, m, s = render_tiles(torch_cuda, renderer, W, H, 8, None)
    cc = clamp_samples(cs, clamp, F64)
    ref_a = cc.mean(0)
    ref_m = sample_moments_ref(cc)
    err_a = np.abs(a[..., :3] - ref_a) / (REL * np.abs(ref_a) + ABS)
    err_m = np.abs(m - ref_m) / (REL * np.abs(ref_m) + ABS)
    lc = luminance(cc)
    var_ref = (lc * lc).mean(0) - lc.mean(0) ** 2
    d = m[..., 1].astype(F64) - m[..., 0].astype(F64) ** 2
    tol = REL * (ref_m[..., 1] + 2 * ref_m[..., 0] ** 2) + 2 * ABS
    print(f"{size}: clamp {clamp:.6g}, {(l > clamp).mean():.3f} of the samples above; accum {err_a.max():.3f}, moments "
          f"{err_m.max():.3f}, variance {(np.abs(d - var_ref) / tol).max():.3f} of their bounds")
    assert close(a[..., :3].astype(F64), ref_a).all(), err_a.max()
    assert np.all(a[..., 3] == 1)
    assert close(m.astype(F64), ref_m).all(), err_m.max()
    assert np.all(np.abs(d - var_ref) <= tol), (np.abs(d - var_ref) / tol).max()
    assert np.array_equal(s, s_plain), "segment counts are untouched"
    # the clamp did something: some pixel's mean moved by more than the tolerance
    plain = cs.mean(0)
    assert (np.abs(ref_a - plain) > 10 * (REL * np.abs(plain) + ABS)).any()


# ---------------------------------------------------------------------------------------------- 3: exact properties
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_clamp_exact_properties(torch_cuda, renderer, size):
    from octree_pathtracing_amd import _lib

    W, H = size
    t = torch_cuda
    clamp = median_clamp(t, renderer, W, H)
    preview = lambda: render_full_flags(t, renderer, W, H, preview=True)  # noqa: E731
    preview_plain = preview()
    with clamped(renderer, clamp):
        a8, m8, s8 = render_tiles(t, renderer, W, H, 8, None)
        # 8 spp in one call = 4 + 4
        a4, m4, s4 = render_tiles(t, renderer, W, H, 4, None)
        a44, m44, s44 = render_tiles(t, renderer, W, H, 4, None, 4, a4, m4, s4)
        assert same(a44, a8) and same(m44, m8) and np.array_equal(s44, s8)
        # a half list leaves the unlisted tiles untouched
        lst = half_list(W, H)
        inside = tile_mask(W, H, lst)
        sa, sm, ss = sentinel(W, H)
        start = (np.where(inside[..., None], black(W, H), sa), np.where(inside[..., None], F32(0), sm),
                 np.where(inside, np.uint32(0), ss))
        a, m, s = render_tiles(t, renderer, W, H, 8, lst, 0, *start)
        assert same(a[inside], a8[inside]) and same(m[inside], m8[inside]) and np.array_equal(s[inside], s8[inside])
        assert same(a[~inside], sa[~inside]) and same(m[~inside], sm[~inside]) and np.array_equal(s[~inside], ss[~inside])
        # branch_count = 10: the passes 3 and 4..9 (a pass of weight 6, folded) in one call and in two
        base = render_tiles(t, renderer, W, H, 3, None, branch_count=10)
        one = render_tiles(t, renderer, W, H, 7, None, 3, *base, branch_count=10)
        mid = render_tiles(t, renderer, W, H, 1, None, 3, *base, branch_count=10)
        two = render_tiles(t, renderer, W, H, 6, None, 4, *mid, branch_count=10)
        assert same(one[0], two[0]) and same(one[1], two[1]) and np.array_equal(one[2], two[2])
        # the megakernel is refused, a preview ignores the clamp
        f = Frames(t, W, H, sa, sm, ss)
        st = status_of(renderer.render_device, params(renderer, W, H, 0, 4, megakernel=True), f.acc.data_ptr())
        assert st == _lib.ERR_UNSUPPORTED
        assert same(f.host()[0], sa)
        assert same(preview(), preview_plain)
        # refused values keep the setting
        for bad in (float("nan"), -1.0):
            assert status_of(renderer.set_sample_clamp, bad) == _lib.ERR_INVALID_ARG
        again = render_tiles(t, renderer, W, H, 8, None)
        assert same(again[0], a8) and same(again[1], m8)
    plain = render_tiles(t, renderer, W, H, 8, None)
    assert not same(plain[0], a8), "the clamp is off again and had acted"


def render_full_flags(torch, r, W, H, **kw):
    f = Frames(torch, W, H)
    r.render_device(params(r, W, H, 0, 1, **kw), f.acc.data_ptr())
    return f.host()[0]


# ---------------------------------------------------------------------------------------------- 4: the spread kernel
def spread_device(torch, r, e, W, H, w):
    d_e = torch.from_numpy(np.ascontiguousarray(e, F32)).cuda()
    d_o = torch.full((len(e),), -1.0, dtype=torch.float32, device="cuda")
    r.tile_error_spread_device(W, H, w, d_e.data_ptr(), d_o.data_ptr())
    torch.cuda.synchronize()
    return d_o.cpu().numpy()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_spread(torch_cuda, renderer, size):
    from octree_pathtracing_amd import _lib

    W, H = size
    T = int(np.prod(tile_grid(W, H)))
    _, m8 = rendered_moments(torch_cuda, renderer, W, H)
    rendered = tile_error_device(torch_cuda, renderer, m8, np.full(T, 8, np.uint32))
    synthetic = np.random.default_rng(9).random(T, F32)
    tx = tile_grid(W, H)[0]
    synthetic[[0, tx - 1, T // 2, T - 1]] = np.inf  # corners and an inner tile
    for e in (rendered, synthetic):
        for w in WEIGHTS:
            ref = spread_ref(e, W, H, w)
            assert same(spread_device(torch_cuda, renderer, e, W, H, w), ref), w
            assert same(renderer.tile_error_spread(e, W, H, w), ref), w
    assert same(spread_ref(synthetic, W, H, 0.0), synthetic)
    assert np.isposinf(spread_ref(synthetic, W, H, 0.5)[[1, tx]]).all(), "+inf reaches the neighbours"
    # refusals
    d = torch_cuda.zeros(2 * T, dtype=torch_cuda.float32, device="cuda")
    inv = _lib.ERR_INVALID_ARG
    for w in (-0.1, 1.5, float("nan"), float("inf")):
        assert status_of(renderer.tile_error_spread_device, W, H, w, d.data_ptr(), d.data_ptr() + 4 * T) == inv
    assert status_of(renderer.tile_error_spread_device, W, H, 0.5, d.data_ptr(), d.data_ptr()) == inv
    assert status_of(renderer.tile_error_spread_device, W, H, 0.5, d.data_ptr(), d.data_ptr() + 4 * T) == _lib.OK
    torch_cuda.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5: the sample variance
def guides_of(r, W, H):
    from octree_pathtracing_amd.scene import RenderSettings

    return r.render_aov(RenderSettings(W, H, 1), which=("albedo", "normal", "depth"))


def variance_device(torch, r, moments, tile_spp, aov, demodulate):
    from octree_pathtracing_amd import _lib

    H, W = moments.shape[:2]
    m = torch.from_numpy(np.ascontiguousarray(moments, F32)).cuda()
    n = torch.from_numpy(np.ascontiguousarray(tile_spp, np.uint32).view(np.int32)).cuda()
    g = {k: torch.from_numpy(np.ascontiguousarray(aov[k], F32)).cuda() for k in ("depth", "albedo")}
    out = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
    p = _lib.SampleVarianceParams(W, H, _lib.DENOISE_DEMODULATE if demodulate else 0)
    r.sample_variance_device(p, m.data_ptr(), n.data_ptr(), {k: v.data_ptr() for k, v in g.items()}, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_sample_variance(torch_cuda, renderer, size):
    from octree_pathtracing_amd import _lib

    W, H = size
    T = int(np.prod(tile_grid(W, H)))
    aov = guides_of(renderer, W, H)
    miss = ~np.isfinite(aov["depth"])
    assert miss.any() and (~miss).any()
    _, m8 = rendered_moments(torch_cuda, renderer, W, H)
    spp = np.full(T, 8, np.uint32)
    spp[1], spp[2], spp[T - 1], spp[T // 2] = 0, 1, 5, 2
    # synthetic moments: m2 < m1^2, a NaN, and an albedo component below the floor
    rng = np.random.default_rng(13)
    syn = np.empty((H, W, 2), F32)
    syn[..., 0] = rng.random((H, W), F32) + F32(0.1)
    syn[..., 1] = syn[..., 0] * syn[..., 0] + rng.random((H, W), F32) - F32(0.2)
    hits = np.argwhere(~miss & tile_mask(W, H, np.flatnonzero(spp >= 2)))
    nan_at, low_at = hits[len(hits) // 3], hits[len(hits) // 2]
    syn[nan_at[0], nan_at[1], 1] = np.nan
    alb = aov["albedo"].copy()
    alb[low_at[0], low_at[1], :3] = (F32(1e-5), F32(0.5), F32(0.0))
    d = syn[..., 1] - syn[..., 0] * syn[..., 0]
    assert (d < 0).any() and (d > 0).any()
    for moments, g in ((m8, aov), (syn, dict(aov, albedo=alb))):
        for demodulate in (False, True):
            ref = sample_variance_ref(moments, spp, g["depth"], g["albedo"] if demodulate else None)
            assert np.all(ref >= 0) and np.all(np.isfinite(ref)) and (ref > 0).any()
            dev = variance_device(torch_cuda, renderer, moments, spp, g, demodulate)
            host = renderer.sample_variance(moments, spp, g, demodulate=demodulate)
            assert same(dev, ref), (demodulate, np.abs(dev - ref).max())
            assert same(host, ref), demodulate
            assert np.all(dev[miss] == 0) and np.all(dev[tile_mask(W, H, [1, 2])] == 0)
    assert sample_variance_ref(syn, spp, aov["depth"])[nan_at[0], nan_at[1]] == 0
    # refusals: the depth guide, the albedo guide with the flag, an unknown flag, an output that is an input
    t = torch_cuda
    buf = t.zeros(W * H * 2, dtype=t.float32, device="cuda")
    n = t.zeros(T, dtype=t.int32, device="cuda")
    out = t.zeros(W * H, dtype=t.float32, device="cuda")
    call = renderer.sample_variance_device
    inv = _lib.ERR_INVALID_ARG
    P = _lib.SampleVarianceParams
    assert status_of(call, P(W, H, 0), buf.data_ptr(), n.data_ptr(), {}, out.data_ptr()) == inv
    assert status_of(call, P(W, H, 1), buf.data_ptr(), n.data_ptr(), {"depth": buf.data_ptr()}, out.data_ptr()) == inv
    assert status_of(call, P(W, H, 2), buf.data_ptr(), n.data_ptr(), {"depth": buf.data_ptr()}, out.data_ptr()) == inv
    assert status_of(call, P(W, H, 0), buf.data_ptr(), n.data_ptr(), {"depth": out.data_ptr()}, out.data_ptr()) == inv
    assert status_of(call, P(W, H, 0), buf.data_ptr(), n.data_ptr(), {"depth": buf.data_ptr()}, buf.data_ptr()) == inv


# ---------------------------------------------------------------------------------------------- 6: the _ex driver
def composed_ex(torch, r, W, H, w, threshold, min_spp=4, step_spp=4, max_spp=16):
    """The _ex loop composed from render_tiles_device, tile_error_device and tile_error_spread_device -> (accum,
    moments, tile_spp, last spread plane, rounds); asserts the seam rule in every round."""
    from octree_pathtracing_amd import _lib

    T = int(np.prod(tile_grid(W, H)))
    f = Frames(torch, W, H)
    d_err = torch.zeros(T, dtype=torch.float32, device="cuda")
    d_spr = torch.zeros(T, dtype=torch.float32, device="cuda")

    def render(active, start, count):
        r.render_tiles_device(params(r, W, H, start, count), np.asarray(active, np.uint32), f.acc.data_ptr(),
                              f.mom.data_ptr(), None)

    def error(tile_spp):
        d_spp = torch.from_numpy(tile_spp.view(np.int32)).cuda()
        r.tile_error_device(_lib.TileErrorParams(W, H, FLOOR), f.mom.data_ptr(), d_spp.data_ptr(), d_err.data_ptr())
        torch.cuda.synchronize()
        return d_err.cpu().numpy()

    def spread(raw):
        r.tile_error_spread_device(W, H, w, d_err.data_ptr(), d_spr.data_ptr())
        torch.cuda.synchronize()
        out = d_spr.cpu().numpy()
        assert same(out, spread_ref(raw, W, H, w))
        return out

    def seam_rule(active, raw, plane, n):
        if n >= max_spp:
            return
        for t in active:
            if plane[t] <= threshold:  # t stops before the cap
                assert raw[t] <= threshold
                for u in neighbours(W, H, t):
                    assert F32(w) == 0 or F32(w) * raw[u] <= threshold, (t, u, raw[u])

    tile_spp, err, rounds = adaptive_loop_ex(T, render, error, spread, min_spp, step_spp, max_spp, threshold, seam_rule)
    a, m, _ = f.host()
    return a, m, tile_spp, err, rounds


def adaptive_ex_device(torch, r, W, H, w, threshold, reserved=(0, 0, 0), max_spp=16):
    from octree_pathtracing_amd import _lib

    sa, sm, _ = sentinel(W, H)
    f = Frames(torch, W, H, sa, sm)
    a = _lib.AdaptiveParamsEx(4, 4, threshold, FLOOR, w, (_lib.C.c_uint32 * 3)(*reserved))
    tile_spp, res = r.render_adaptive_ex_device(params(r, W, H, 0, max_spp), a, f.acc.data_ptr(), f.mom.data_ptr())
    acc, mom, _ = f.host()
    return acc, mom, tile_spp, res


def median_threshold(torch, r, W, H):
    e1 = first_round_errors(torch, r, W, H)
    finite = e1[np.isfinite(e1)]
    threshold = float(np.median(finite))
    assert (finite < threshold).any() and (finite > threshold).any() and threshold > 0
    return threshold


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_adaptive_ex_driver(torch_cuda, renderer, size):
    from octree_pathtracing_amd import _lib

    W, H = size
    threshold = median_threshold(torch_cuda, renderer, W, H)
    spp_of = {}
    fresh = _renderer_with({})
    try:
        for w in WEIGHTS:
            a, m, tile_spp, err, rounds = composed_ex(torch_cuda, fresh, W, H, w, threshold)
            da, dm, d_spp, res = adaptive_ex_device(torch_cuda, renderer, W, H, w, threshold)
            assert same(da, a) and same(dm, m) and np.array_equal(d_spp, tile_spp), w
            assert res == dict(rounds=rounds, tile_samples=int(tile_spp.sum()),
                               converged_tiles=int((err <= threshold).sum()), total_tiles=len(tile_spp)), w
            spp_of[w] = tile_spp
    finally:
        fresh.close()
    print(f"{size}: tile samples " + ", ".join(f"w={w}: {int(s.sum())}" for w, s in spp_of.items()))
    assert not np.array_equal(spp_of[1.0], spp_of[0.0]), "an adjacent pair lies across the median threshold"
    assert np.all(spp_of[1.0] >= spp_of[0.5]) and np.all(spp_of[0.5] >= spp_of[0.0])
    assert np.all(spp_of[1.0] >= spp_of[0.0])
    # w = 0 is the plain driver
    sa, sm, _ = sentinel(W, H)
    f = Frames(torch_cuda, W, H, sa, sm)
    p_spp, p_res = renderer.render_adaptive_device(params(renderer, W, H, 0, 16),
                                                   _lib.AdaptiveParams(4, 4, threshold, FLOOR), f.acc.data_ptr(),
                                                   f.mom.data_ptr())
    pa, pm, _ = f.host()
    xa, xm, x_spp, x_res = adaptive_ex_device(torch_cuda, renderer, W, H, 0.0, threshold)
    assert same(pa, xa) and same(pm, xm) and np.array_equal(p_spp, x_spp) and p_res == x_res
    # the host form, which render_adaptive reaches with a weight
    from octree_pathtracing_amd.scene import RenderSettings

    _, _, rs = c3()
    ha, hm, h_spp, hres = renderer.render_adaptive(RenderSettings(W, H, 16, max_depth=rs.max_depth, seed=rs.seed), 4, 4,
                                                   threshold, FLOOR, neighbour_weight=0.5)
    ea, em, e_spp, eres = adaptive_ex_device(torch_cuda, renderer, W, H, 0.5, threshold)
    assert same(ha, ea) and same(hm, em) and np.array_equal(h_spp, e_spp) and hres == eres
    # refusals leave the buffers untouched
    f = Frames(torch_cuda, W, H, sa, sm)
    for reserved, w in (((1, 0, 0), 0.5), ((0, 0, 7), 0.0), ((0, 0, 0), 1.5), ((0, 0, 0), float("nan"))):
        a = _lib.AdaptiveParamsEx(4, 4, threshold, FLOOR, w, (_lib.C.c_uint32 * 3)(*reserved))
        st = status_of(renderer.render_adaptive_ex_device, params(renderer, W, H, 0, 16), a, f.acc.data_ptr(),
                       f.mom.data_ptr())
        assert st == _lib.ERR_INVALID_ARG, (reserved, w)
    a, m, _ = f.host()
    assert same(a, sa) and same(m, sm)


# ---------------------------------------------------------------------------------------------- 7: the finished frame
ITERATIONS = 3
SIGMA_LUMINANCE = 4.0


def final_params(W, H, threshold, demodulate, w=0.5, fw=None, fh=None):
    from octree_pathtracing_amd import _lib

    return _lib.FinalParams(
        _lib.AdaptiveParamsEx(4, 4, threshold, FLOOR, w),
        _lib.DenoiseVarianceParams(W if fw is None else fw, H if fh is None else fh, ITERATIONS, SIGMA_LUMINANCE, FLOOR,
                                   0.3, 0.1, _lib.DENOISE_DEMODULATE if demodulate else 0))


class FinalFrames:
    def __init__(self, torch, W, H):
        sa, sm, _ = sentinel(W, H)
        self.torch = torch
        self.sent = (sa, sm)
        self.acc = torch.from_numpy(sa).cuda()
        self.mom = torch.from_numpy(sm).cuda()
        self.out = torch.full((H, W, 4), -2.0, dtype=torch.float32, device="cuda")
        self.var = torch.full((H, W), -3.0, dtype=torch.float32, device="cuda")

    def host(self):
        self.torch.cuda.synchronize()
        return tuple(x.cpu().numpy() for x in (self.acc, self.mom, self.out, self.var))


def final_composed(torch, r, W, H, threshold, demodulate):
    """octpt_render_final_device's four steps through the public entries."""
    from octree_pathtracing_amd import _lib

    fp = final_params(W, H, threshold, demodulate)
    f = FinalFrames(torch, W, H)
    p = params(r, W, H, 0, 16)
    tile_spp, res = r.render_adaptive_ex_device(p, fp.adaptive, f.acc.data_ptr(), f.mom.data_ptr())
    g = {"normal": torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"),
         "depth": torch.zeros((H, W), dtype=torch.float32, device="cuda")}
    if demodulate:
        g["albedo"] = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    ptrs = {k: v.data_ptr() for k, v in g.items()}
    r.render_aov_device(p, ptrs)
    d_spp = torch.from_numpy(tile_spp.view(np.int32)).cuda()
    d_v = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    r.sample_variance_device(_lib.SampleVarianceParams(W, H, fp.filter.flags), f.mom.data_ptr(), d_spp.data_ptr(), ptrs,
                             d_v.data_ptr())
    r.denoise_variance_device(fp.filter, f.acc.data_ptr(), d_v.data_ptr(), ptrs, f.out.data_ptr(), f.var.data_ptr())
    torch.cuda.synchronize()
    guides = {k: v.cpu().numpy() for k, v in g.items()}
    return f.host(), tile_spp, res, guides, d_v.cpu().numpy()


def final_device(torch, r, W, H, threshold, demodulate):
    f = FinalFrames(torch, W, H)
    tile_spp, res = r.render_final_device(params(r, W, H, 0, 16), final_params(W, H, threshold, demodulate),
                                          f.acc.data_ptr(), f.mom.data_ptr(), f.out.data_ptr(), f.var.data_ptr())
    return f.host(), tile_spp, res


@pytest.mark.parametrize("case", ["plain", "demodulate", "demodulate-clamp"])
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_render_final(torch_cuda, renderer, size, case):
    from octree_pathtracing_amd.scene import RenderSettings

    W, H = size
    demodulate = case != "plain"
    clamp = median_clamp(torch_cuda, renderer, W, H) if case.endswith("clamp") else 0.0
    _, _, rs = c3()
    with clamped(renderer, clamp):
        threshold = median_threshold(torch_cuda, renderer, W, H)  # of the errors under the clamp, when one is set
        (ca, cm, co, cv), c_spp, c_res, guides, var = final_composed(torch_cuda, renderer, W, H, threshold, demodulate)
        (da, dm, do, dv), d_spp, d_res = final_device(torch_cuda, renderer, W, H, threshold, demodulate)
        h = renderer.render_final(RenderSettings(W, H, 16, max_depth=rs.max_depth, seed=rs.seed), 4, 4, threshold,
                                  neighbour_weight=0.5, luminance_floor=FLOOR, iterations=ITERATIONS,
                                  sigma_luminance=SIGMA_LUMINANCE, demodulate=demodulate, with_rgba=True)
    assert same(da, ca) and same(dm, cm) and same(do, co) and same(dv, cv)
    assert np.array_equal(d_spp, c_spp) and d_res == c_res
    assert same(h["accum"], da) and same(h["moments"], dm) and same(h["out"], do) and same(h["out_variance"], dv)
    assert np.array_equal(h["tile_spp"], d_spp) and h["result"] == d_res
    assert h["rgba"].shape == (H, W, 4) and h["rgba"].any()
    assert (d_spp == 4).any() and (d_spp > 4).any()
    # against the restatements: C35's variance bit for bit, C29's filter of it within the tolerance
    ref_var = sample_variance_ref(dm, d_spp, guides["depth"], guides.get("albedo"))
    assert same(var, ref_var)
    ref, ref_v = svgf_ref.denoise_variance_ref(da, ref_var, guides["normal"], guides["depth"], guides.get("albedo"),
                                               iterations=ITERATIONS, sigma_luminance=SIGMA_LUMINANCE,
                                               luminance_floor=FLOOR, demodulate=demodulate)
    err, err_v = np.abs(do - ref), np.abs(dv - ref_v)
    print(f"{size} {case}: colour {(err / (REL * np.abs(ref) + ABS)).max():.3f}, variance "
          f"{(err_v / (REL * np.abs(ref_v) + ABS)).max():.3f} of the tolerance")
    assert close(do, ref).all(), float(err.max())
    assert close(dv, ref_v).all(), float(err_v.max())
    hit = np.isfinite(guides["depth"])
    assert np.abs(do[hit] - da[hit]).max() > 1e-3, "the filter does something"
    if clamp:
        unclamped = final_device(torch_cuda, renderer, W, H, threshold, demodulate)[0][0]
        assert not same(unclamped, da), "the context's clamp applies"


def test_render_final_refusals(torch_cuda, renderer):
    from octree_pathtracing_amd import _lib

    W, H = 64, 64
    f = FinalFrames(torch_cuda, W, H)
    p = params(renderer, W, H, 0, 16)
    call = renderer.render_final_device
    inv = _lib.ERR_INVALID_ARG
    ok = final_params(W, H, 0.1, True)
    # d_out aliasing d_accum, a resolution mismatch, the driver's and the filter's own refusals
    assert status_of(call, p, ok, f.acc.data_ptr(), f.mom.data_ptr(), f.acc.data_ptr(), f.var.data_ptr()) == inv
    for bad in (final_params(W, H, 0.1, True, fw=W + 1), final_params(W, H, 0.1, True, fh=H - 1),
                final_params(W, H, float("nan"), True), final_params(W, H, 0.1, True, w=2.0)):
        assert status_of(call, p, bad, f.acc.data_ptr(), f.mom.data_ptr(), f.out.data_ptr(), f.var.data_ptr()) == inv
    bad = final_params(W, H, 0.1, True)
    bad.filter.iterations = 6
    assert status_of(call, p, bad, f.acc.data_ptr(), f.mom.data_ptr(), f.out.data_ptr(), f.var.data_ptr()) == inv
    bad = final_params(W, H, 0.1, True)
    bad.adaptive.reserved[1] = 1
    assert status_of(call, p, bad, f.acc.data_ptr(), f.mom.data_ptr(), f.out.data_ptr(), f.var.data_ptr()) == inv
    assert status_of(call, params(renderer, W, H, 0, 16, megakernel=True), ok, f.acc.data_ptr(), f.mom.data_ptr(),
                     f.out.data_ptr(), f.var.data_ptr()) == _lib.ERR_UNSUPPORTED
    a, m, o, v = f.host()
    assert same(a, f.sent[0]) and same(m, f.sent[1]) and np.all(o == -2.0) and np.all(v == -3.0)


def test_firefly_budget_mechanism(renderer):
    """What C33 exists for, without a lucky scene: one pixel whose eight samples hold one of luminance 1000 keeps its
    tile's error above a threshold that the same samples, clamped, are below."""
    W, H = 37, 21
    T = int(np.prod(tile_grid(W, H)))
    threshold, clamp = 0.05, 1.0
    samples = np.full((8, 3), 0.5, F64)
    samples[5] = 1000.0
    calm = np.empty((H, W, 2), F32)
    calm[..., 0], calm[..., 1] = F32(0.5), F32(0.25 + 1e-4)
    y, x = 12, 19
    t = (y // 8) * tile_grid(W, H)[0] + x // 8
    hot, cool = calm.copy(), calm.copy()
    hot[y, x] = sample_moments_ref(samples).astype(F32)
    cool[y, x] = sample_moments_ref(clamp_samples(samples, clamp, F64)).astype(F32)
    spp = np.full(T, 8, np.uint32)
    e_hot, e_cool = renderer.tile_error(hot, spp, FLOOR), renderer.tile_error(cool, spp, FLOOR)
    assert e_hot[t] > threshold >= e_cool[t], (e_hot[t], e_cool[t])
    others = np.arange(T) != t
    assert same(e_hot[others], e_cool[others]) and np.all(e_hot[others] <= threshold)
