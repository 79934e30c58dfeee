"""Luminance moments, variance and the variance-guided a-trous filter (octpt_temporal_moments, octpt_variance,
octpt_denoise_variance) against the numpy restatements of the three rows (tests/svgf_ref.py),
the properties the rows promise, the call forms and the refusals that need a context.

luminance_floor in the C29 comparisons is LUMINANCE_FLOOR = 1e-2, the Python default and DESIGN.md C29's value.  The
weight expf(-|dl| k) is ill-conditioned where k is large: |dl| carries the rounding of l, about 2^-24 l, and
k <= 1 / luminance_floor multiplies it; the condition on the inputs, asserted before the device comparison, is that
the f32 restatement agrees with its own f64 evaluation to within half the tolerance.  On these frames (variance up
to 1e7, exactly 0 on a handful of hit pixels) it does so at every power of ten from 1e-30 to 10 (at most 0.37 of the
tolerance; 0.17 at 1e-2), so the condition does not pick a smallest one here; 1e-2 is the smallest power of ten that
keeps 2^-24 l / luminance_floor inside the tolerance for a signal of unit luminance and no variance (6e-6; 6e-5 at
1e-3)."""
import ctypes as C

import numpy as np
import pytest

from tests.svgf_ref import (denoise_variance_ref, luminance, temporal_moments_ref, variance_ref, working_signal)

pytestmark = pytest.mark.gpu

F32 = np.float32
F64 = np.float64
REL, ABS = 1e-5, 1e-6  # the project's forward tolerance, as tests/test_gpu_denoise.py
SIZES = [(64, 64), (37, 21)]
KW = dict(max_history=32, depth_tolerance=0.1, normal_threshold=0.9, match_prim=True)
LUMINANCE_FLOOR = 1e-2
SIGMA_LUMINANCE = 4.0


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    from octree_pathtracing_amd.renderer import HipRenderer

    r = HipRenderer(device=0)
    yield r
    r.close()


def close(got, ref):
    return np.abs(got - ref) <= REL * np.abs(ref) + ABS


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def moved(cam, right=0.0, up=0.0, forward=0.0, yaw=0.0):
    """cam translated along its own axes and turned by `yaw` radians towards its right."""
    from octree_pathtracing_amd.scene import Camera

    d, u = np.asarray(cam.direction, np.float64), np.asarray(cam.up, np.float64)
    r = np.cross(d, u)
    eye = np.asarray(cam.eye, np.float64) + right * r + up * u + forward * d
    c = Camera.look_at(tuple(eye), tuple(eye + np.cos(yaw) * d + np.sin(yaw) * r), up=tuple(u))
    c.fov = cam.fov
    return c


@pytest.fixture(scope="module")
def frames(renderer):
    """(W, H) -> the C3 frames of tests/test_gpu_temporal.py's camera move, computed once: `prev` (4 spp) and `cur`
    (2 spp, the camera translated by 3 to the right, 1 down, 2 forward and yawed by 0.02 rad), each as (colour,
    guides, camera)."""
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.scene import RenderSettings

    sc, cam0, _ = S.make_config("C3")
    cam1 = moved(cam0, right=3.0, up=-1.0, forward=2.0, yaw=0.02)
    renderer.set_scene(sc)
    out = {}
    for W, H in SIZES:
        f = {}
        for name, cam, spp in (("prev", cam0, 4), ("cur", cam1, 2)):
            renderer.set_camera(cam)
            rs = RenderSettings(W, H, spp)
            color, _ = renderer.render(rs)
            aov = renderer.render_aov(rs)
            hit = np.isfinite(aov["depth"])
            assert hit.any() and (~hit).any(), "the frames must hold hit and miss pixels"
            f[name] = (color, aov, cam)
        out[(W, H)] = f
    return out


def variants(color):
    """Four different frames over one set of guides: the render, its point mirror, and both scaled."""
    flipped = color[::-1, ::-1].copy()
    return [color, flipped, (color * F32(0.5)).astype(F32), (flipped * F32(1.5)).astype(F32)]


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def history(renderer, f, size, demodulate, frames_n=4):
    """The history after `frames_n` static frames at the previous camera (lengths frames_n on hits), with moments."""
    def make():
        color, aov, cam = f["prev"]
        renderer.set_camera(cam)
        h = None
        for c in variants(color)[:frames_n]:
            h = renderer.temporal(c, aov, h, moments=True, demodulate=demodulate, **KW)
        return h
    return cached(("history", size, demodulate, frames_n), make)


def current(renderer, f, size, demodulate):
    """The moving-camera frame blended into the 4-frame history: temporal(..., moments=True)'s dict."""
    def make():
        hist = history(renderer, f, size, demodulate)
        color, aov, cam = f["cur"]
        renderer.set_camera(cam)
        return renderer.temporal(color, aov, hist, moments=True, demodulate=demodulate, **KW)
    return cached(("current", size, demodulate), make)


# ---------------------------------------------------------------------------------------------- C27
@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulate", "plain"])
@pytest.mark.parametrize("size", SIZES, ids=["64x64", "37x21"])
def test_moments_moving_camera(renderer, frames, size, demodulate):
    """Colour and length bit-identical to renderer.temporal on the same inputs; moments within 1e-5 relative +
    1e-6 absolute of the restatement, exactly 0 on misses; pixels with history, disoccluded pixels and misses all
    occur."""
    f = frames[size]
    hist = history(renderer, f, size, demodulate)
    color, aov, cam = f["cur"]
    got = current(renderer, f, size, demodulate)
    renderer.set_camera(cam)
    plain = renderer.temporal(color, aov, hist, **KW)
    assert "moments" not in plain and got["moments"].shape == color.shape[:2] + (2,)
    assert np.array_equal(bits(got["color"]), bits(plain["color"]))
    assert np.array_equal(got["length"], plain["length"])
    ref, ref_len = temporal_moments_ref(color, aov, hist, cam, f["prev"][2], demodulate=demodulate, **KW)
    hit = np.isfinite(aov["depth"])
    err = np.abs(got["moments"] - ref)
    print(f"{size} demodulate={demodulate}: max moment error {err.max():.3e} (max |ref| {np.abs(ref).max():.3e}), "
          f"history {int((ref_len > 1).sum())}, disoccluded {int(((ref_len == 1) & hit).sum())}, "
          f"misses {int((~hit).sum())}")
    assert np.array_equal(got["length"], ref_len)
    assert (ref_len[hit] == 5).any(), "no pixel carries its history"
    assert (ref_len[hit] == 1).any(), "no disoccluded pixel"
    assert (~hit).any() and np.all(ref_len[~hit] == 0), "no miss"
    assert np.all(np.isfinite(got["moments"]))
    bad = ~close(got["moments"], ref)
    assert not bad.any(), (int(bad.sum()), float(err.max()))
    assert np.all(bits(got["moments"][~hit]) == 0)
    # the moments of a pixel with history are not the frame's own
    mu, _ = temporal_moments_ref(color, aov, None, cam, cam, demodulate=demodulate)
    assert np.abs(got["moments"][ref_len == 5] - mu[ref_len == 5]).max() > 1e-3
    assert close(got["moments"][ref_len == 1], mu[ref_len == 1]).all()


@pytest.mark.parametrize("max_history", [32, 3])
def test_static_camera_moments_follow_the_running_means(renderer, frames, max_history):
    """K = 6 frames of constant colours over real guides: after frame k the moments are the running means of l and
    l^2 (1e-5 relative), the exponential blend with weight 1/3 from frame 3 on with max_history = 3."""
    _, aov, cam = frames[(64, 64)]["prev"]
    renderer.set_camera(cam)
    hit = np.isfinite(aov["depth"])
    hist, m1, m2 = None, 0.0, 0.0
    for k in range(1, 7):
        c = np.array([0.05 + 0.1 * k, 0.9 / k, 0.3 + 0.07 * (k % 3)])
        color = np.empty((64, 64, 4), F32)
        color[...] = (*c, 1.0)
        hist = renderer.temporal(color, aov, hist, max_history=max_history, moments=True)
        l = float(luminance(color[0, 0, :3].astype(F64), F64))
        n = min(k, max_history)
        m1, m2 = m1 + (l - m1) / n, m2 + (l * l - m2) / n
        assert np.all(hist["length"][hit] == n) and np.all(hist["length"][~hit] == 0), k
        assert np.all(np.abs(hist["moments"][hit] - (m1, m2)) <= 1e-5 * np.abs((m1, m2))), k
        assert np.all(bits(hist["moments"][~hit]) == 0)


# ---------------------------------------------------------------------------------------------- C28
@pytest.mark.parametrize("min_history", [1, 4, 100])
@pytest.mark.parametrize("size", SIZES, ids=["64x64", "37x21"])
def test_variance_matches_restatement(renderer, frames, size, min_history):
    """The moving-camera history (lengths 5 where the history was kept, 1 where disoccluded, 0 on misses) with
    min_history 1, 4 and 100: none, some and all hit pixels on the spatial branch.  |got - ref| <= 1e-5 (M2 + M1^2)
    + 1e-6 -- the difference cancels, so the bound is relative to its terms; misses exactly 0; nothing negative or
    non-finite.

    The result carries the factor min_history / N, 100 on a disoccluded pixel, which the bound does not, so a
    last-bit difference in a weight already exceeds it (measured with the device's expf against numpy's f32 exp:
    2.65 times the bound at 64 x 64, 1.61 times at 37 x 21).  The row therefore asks for the correctly rounded
    exponential, the kernel and the restatement both evaluate it in f64 and round once, and the results are
    bit-equal in all six cases (measured on an MI355X)."""
    f = frames[size]
    cur = current(renderer, f, size, False)
    aov = f["cur"][1]
    got = renderer.variance(cur, aov, min_history=min_history)
    ref, terms = variance_ref(cur["moments"], cur["length"], aov["normal"], aov["depth"], min_history=min_history,
                              return_terms=True)
    hit = np.isfinite(aov["depth"])
    spatial = hit & (cur["length"] < min_history)
    expect = {1: "none", 4: "some", 100: "all"}[min_history]
    seen = "none" if not spatial.any() else "all" if spatial[hit].all() else "some"
    err = np.abs(got - ref)
    print(f"{size} min_history={min_history}: spatial {int(spatial.sum())} of {int(hit.sum())}, max error "
          f"{err.max():.3e}, max error / bound {(err / (REL * terms + ABS)).max():.3e}, max variance {ref.max():.3e}")
    assert seen == expect, (seen, expect)
    assert got.shape == ref.shape and got.dtype == F32
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    assert np.all(bits(got[~hit]) == 0)
    bad = err > REL * terms + ABS
    assert not bad.any(), (int(bad.sum()), float(err.max()))
    assert got[hit].max() > 1e-4  # there is variance to estimate


# ---------------------------------------------------------------------------------------------- C29
def filter_inputs(renderer, f, size, demodulate):
    """The blended colour of the moving-camera frame and its C28 variance (min_history 4), with the guides."""
    def make():
        cur = current(renderer, f, size, demodulate)
        aov = f["cur"][1]
        return cur["color"], renderer.variance(cur, aov, min_history=4), aov
    return cached(("filter_inputs", size, demodulate), make)


def filter_ref(color, var, aov, iterations, demodulate, dtype, key):
    return cached(("filter_ref", key, iterations, demodulate, dtype), lambda: denoise_variance_ref(
        color, var, aov["normal"], aov["depth"], aov["albedo"], iterations=iterations, sigma_luminance=SIGMA_LUMINANCE,
        luminance_floor=LUMINANCE_FLOOR, demodulate=demodulate, dtype=dtype))


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulate", "plain"])
@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("size", SIZES, ids=["64x64", "37x21"])
def test_filter_matches_restatement(renderer, frames, size, iterations, demodulate):
    """Colour and variance within 1e-5 relative + 1e-6 absolute of the restatement; miss pixels and alpha
    bit-identical to the input.  Before that, the condition on the inputs: the f32 restatement agrees with its f64
    evaluation to within half the tolerance (luminance_floor = 1e-2, sigma_luminance = 4)."""
    color, var, aov = filter_inputs(renderer, frames[size], size, demodulate)
    hit = np.isfinite(aov["depth"])
    ref, ref_v = filter_ref(color, var, aov, iterations, demodulate, F32, size)
    r64, r64_v = filter_ref(color, var, aov, iterations, demodulate, F64, size)
    cond = max((np.abs(ref - r64) / (REL * np.abs(r64) + ABS)).max(), (np.abs(ref_v - r64_v) / (REL * np.abs(r64_v) + ABS)).max())
    got, got_v = renderer.denoise_variance(color, var, aov, iterations=iterations, sigma_luminance=SIGMA_LUMINANCE,
                                           luminance_floor=LUMINANCE_FLOOR, demodulate=demodulate)
    err, err_v = np.abs(got - ref), np.abs(got_v - ref_v)
    print(f"{size} it={iterations} demodulate={demodulate}: f32 vs f64 restatement {cond:.3f} of the tolerance; device "
          f"colour {(err / (REL * np.abs(ref) + ABS)).max():.3f}, variance {(err_v / (REL * np.abs(ref_v) + ABS)).max():.3f}")
    assert cond <= 0.5, cond
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(got_v)) and np.all(got_v >= 0)
    bad, bad_v = ~close(got, ref), ~close(got_v, ref_v)
    assert not bad.any(), (int(bad.sum()), float(err.max()))
    assert not bad_v.any(), (int(bad_v.sum()), float(err_v.max()))
    assert np.array_equal(bits(got[~hit]), bits(color[~hit]))
    assert np.array_equal(bits(got_v[~hit]), bits(var[~hit]))
    assert np.array_equal(bits(got[..., 3]), bits(color[..., 3]))
    assert np.abs(got[hit] - color[hit]).max() > 1e-3  # the filter does something
    assert got_v.max() <= var.max()  # the filtered variance never exceeds the input's maximum


def test_huge_variance_is_the_plain_filter_without_its_colour_weight(renderer, frames):
    """A variance plane of 1e30: k = 1 / (4e15 + floor), so wl = expf(-|dl| k) = 1 exactly, and sigma_color = 1e18
    makes C25's wc = 1 exactly: the two filters are the same arithmetic."""
    for size in SIZES:
        color, _, aov = filter_inputs(renderer, frames[size], size, True)
        var = np.full(color.shape[:2], 1e30, F32)
        got, got_v = renderer.denoise_variance(color, var, aov, iterations=3, luminance_floor=LUMINANCE_FLOOR)
        want = renderer.denoise(color, aov, iterations=3, sigma_color=1e18)
        assert close(got, want).all(), float(np.abs(got - want).max())
        assert np.all(np.isfinite(got_v)) and got_v.max() <= var.max()


def test_zero_variance_and_a_tiny_floor_keep_the_signal(renderer, frames):
    """A variance plane of 0 with luminance_floor = 1e-30: k = 1e30, a tap whose luminance differs at all weighs
    0, so a pixel all of whose taps differ from it keeps its working signal -- after re-modulation, its colour --
    to the tolerance.  Such pixels are most of the frame."""
    size = (64, 64)
    color, _, aov = filter_inputs(renderer, frames[size], size, True)
    H, W = color.shape[:2]
    hit = np.isfinite(aov["depth"])
    s, _ = working_signal(color, aov["albedo"], hit, True)
    l = luminance(s)
    alone = hit.copy()
    for i in range(2):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                oy, ox = dy << i, dx << i
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                same = np.abs(l[y0:y1, x0:x1] - l[y0 + oy:y1 + oy, x0 + ox:x1 + ox]) <= 1e-5 * np.abs(l[y0:y1, x0:x1])
                alone[y0:y1, x0:x1] &= ~(same & hit[y0 + oy:y1 + oy, x0 + ox:x1 + ox])
    assert alone.sum() > hit.sum() // 2
    got, got_v = renderer.denoise_variance(color, np.zeros((H, W), F32), aov, iterations=2, luminance_floor=1e-30)
    assert close(got[alone], color[alone]).all(), float(np.abs(got[alone] - color[alone]).max())
    assert np.all(got_v == 0)


def test_filtered_variance_falls_from_pass_to_pass(renderer):
    """Flat guides, a constant colour and a constant variance v on 48 x 48: three passes reach 2 + 4 + 8 = 14
    pixels, so the 16 x 16 interior never sees the border and every weight there is h[dx] h[dy]: the variance
    after pass i is v (sum h^2)^(2 i) = v (35/128)^(2 i), falling from pass to pass."""
    H = W = 48
    normal = np.zeros((H, W, 4), F32)
    normal[..., 2] = 1.0
    g = {"normal": normal, "depth": np.full((H, W), 10.0, F32), "albedo": np.full((H, W, 4), 0.5, F32)}
    color = np.empty((H, W, 4), F32)
    color[...] = (0.25, 0.5, 0.75, 1.0)
    var = np.full((H, W), 0.3, F32)
    inner = (slice(16, 32), slice(16, 32))
    last = var[inner]
    for it in (1, 2, 3):
        out, v = renderer.denoise_variance(color, var, g, iterations=it, luminance_floor=LUMINANCE_FLOOR,
                                           demodulate=False)
        assert np.abs(out - color).max() <= 1e-6
        assert np.all(v[inner] < last)
        assert np.all(np.abs(v[inner] - 0.3 * (35.0 / 128.0) ** (2 * it)) <= 1e-5 * 0.3)
        last = v[inner]


# ---------------------------------------------------------------------------------------------- call forms
def dev(torch, a):  # u32 planes travel as i32 bits
    a = np.ascontiguousarray(a)
    return torch.as_tensor(a.view(np.int32) if a.dtype == np.uint32 else a, device="cuda")


def device_moments(renderer, torch, p, color, aov, hist, in_place):
    """octpt_temporal_moments_device over torch tensors on a side stream -> (out, length, moments) as numpy."""
    g = {k: dev(torch, aov[k]) for k in ("normal", "depth", "prim", "albedo")}
    h = {k: dev(torch, hist[k]) for k in ("color", "normal", "depth", "prim", "length")} if hist is not None else None
    hm = dev(torch, hist["moments"]) if hist is not None else None
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = dev(torch, color)
        out = c if in_place else torch.zeros_like(c)
        length = torch.zeros(color.shape[:2], dtype=torch.int32, device="cuda")
        m = torch.zeros(color.shape[:2] + (2,), device="cuda")
        renderer.temporal_moments_device(p, c.data_ptr(), {k: v.data_ptr() for k, v in g.items()},
                                         {k: v.data_ptr() for k, v in h.items()} if h is not None else None,
                                         hm.data_ptr() if hm is not None else None, out.data_ptr(), length.data_ptr(),
                                         m.data_ptr(), s.cuda_stream)
    s.synchronize()
    if not in_place:
        assert np.array_equal(c.cpu().numpy(), color)  # the out-of-place input is left alone
    return out.cpu().numpy(), length.cpu().numpy().view(np.uint32), m.cpu().numpy()


def device_variance(renderer, torch, p, cur, aov):
    g = {k: dev(torch, aov[k]) for k in ("normal", "depth")}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m, n = dev(torch, cur["moments"]), dev(torch, cur["length"])
        out = torch.zeros(cur["length"].shape, device="cuda")
        renderer.variance_device(p, m.data_ptr(), n.data_ptr(), {k: v.data_ptr() for k, v in g.items()}, out.data_ptr(),
                                 s.cuda_stream)
    s.synchronize()
    return out.cpu().numpy()


def device_filter(renderer, torch, p, color, var, aov, in_place):
    g = {k: dev(torch, aov[k]) for k in ("normal", "depth", "albedo")}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c, v = dev(torch, color), dev(torch, var)
        out, out_v = (c, v) if in_place else (torch.zeros_like(c), torch.zeros_like(v))
        renderer.denoise_variance_device(p, c.data_ptr(), v.data_ptr(), {k: t.data_ptr() for k, t in g.items()},
                                         out.data_ptr(), out_v.data_ptr(), s.cuda_stream)
    s.synchronize()
    if not in_place:
        assert np.array_equal(c.cpu().numpy(), color) and np.array_equal(v.cpu().numpy(), var)
    return out.cpu().numpy(), out_v.cpu().numpy()


def test_call_forms_agree(renderer, frames, torch_cuda):
    """For each pass: host form = device form on a side stream; in place = out of place (d_out = d_color,
    d_out_variance = d_variance); a [0, 0] two-entry context gives the same bits; the first frame (d_prev = NULL)
    gives out_m = mu on hits."""
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd.renderer import HipRenderer, _c_camera

    size = (64, 64)
    f = frames[size]
    hist = history(renderer, f, size, True)
    color, aov, cam = f["cur"]
    hit = np.isfinite(aov["depth"])
    renderer.set_camera(cam)
    flags = _lib.TEMPORAL_MATCH_PRIM | _lib.TEMPORAL_DEMODULATE
    p = _lib.TemporalParams(64, 64, _c_camera(cam), _c_camera(f["prev"][2]), 32, 0.1, 0.9, flags)
    # C27: the first frame
    first = renderer.temporal(color, aov, moments=True, demodulate=True)
    mu, _ = temporal_moments_ref(color, aov, None, cam, cam, demodulate=True)
    assert np.array_equal(bits(first["color"]), bits(color)) and np.array_equal(first["length"], hit.astype(np.uint32))
    assert close(first["moments"], mu).all() and np.all(bits(first["moments"][~hit]) == 0)
    d_first = device_moments(renderer, torch_cuda, p, color, aov, None, False)
    assert np.array_equal(bits(d_first[0]), bits(color)) and np.array_equal(d_first[1], first["length"])
    assert np.array_equal(bits(d_first[2]), bits(first["moments"]))
    # C27: with history
    host = current(renderer, f, size, True)
    assert (host["length"] > 1).any()
    forms = [device_moments(renderer, torch_cuda, p, color, aov, hist, False),
             device_moments(renderer, torch_cuda, p, color, aov, hist, True)]
    # C28, C29 on its output
    var = renderer.variance(host, aov, min_history=4)
    pv = _lib.VarianceParams(64, 64, 4, 0.3, 0.1)
    assert np.array_equal(bits(device_variance(renderer, torch_cuda, pv, host, aov)), bits(var))
    pf = _lib.DenoiseVarianceParams(64, 64, 3, SIGMA_LUMINANCE, LUMINANCE_FLOOR, 0.3, 0.1, _lib.DENOISE_DEMODULATE)
    filt = renderer.denoise_variance(host["color"], var, aov, iterations=3, luminance_floor=LUMINANCE_FLOOR)
    f_forms = [device_filter(renderer, torch_cuda, pf, host["color"], var, aov, False),
               device_filter(renderer, torch_cuda, pf, host["color"], var, aov, True)]
    with HipRenderer(devices=[0, 0]) as r2:
        assert r2.device_entries == 2
        r2.set_camera(cam)
        m2 = r2.temporal(color, aov, hist, moments=True, demodulate=True, **KW)
        forms += [(m2["color"], m2["length"], m2["moments"]), device_moments(r2, torch_cuda, p, color, aov, hist, False)]
        assert np.array_equal(bits(r2.variance(host, aov, min_history=4)), bits(var))
        assert np.array_equal(bits(device_variance(r2, torch_cuda, pv, host, aov)), bits(var))
        f_forms += [r2.denoise_variance(host["color"], var, aov, iterations=3, luminance_floor=LUMINANCE_FLOOR),
                    device_filter(r2, torch_cuda, pf, host["color"], var, aov, False)]
    for out, length, m in forms:
        assert np.array_equal(bits(out), bits(host["color"])) and np.array_equal(length, host["length"])
        assert np.array_equal(bits(m), bits(host["moments"]))
    for out, v in f_forms:
        assert np.array_equal(bits(out), bits(filt[0])) and np.array_equal(bits(v), bits(filt[1]))
    # d_out_variance = NULL: the colour alone, the same bits
    t = {k: dev(torch_cuda, a) for k, a in (("c", host["color"]), ("v", var), ("normal", aov["normal"]),
                                            ("depth", aov["depth"]), ("albedo", aov["albedo"]))}
    out = torch_cuda.zeros_like(t["c"])
    renderer.denoise_variance_device(pf, t["c"].data_ptr(), t["v"].data_ptr(),
                                     {k: t[k].data_ptr() for k in ("normal", "depth", "albedo")}, out.data_ptr(), None,
                                     torch_cuda.cuda.current_stream().cuda_stream)
    torch_cuda.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(filt[0])) and np.array_equal(t["v"].cpu().numpy(), var)


# ---------------------------------------------------------------------------------------------- refusals
def flat_guides(H, W):
    normal = np.zeros((H, W, 4), F32)
    normal[..., 2] = 1.0
    return {"normal": normal, "depth": np.full((H, W), 10.0, F32), "prim": np.zeros((H, W), np.uint32),
            "albedo": np.full((H, W, 4), 0.5, F32)}


def ptr(a):
    return a.ctypes.data


BAD_FLOATS = (0.0, -1.0, float("inf"), float("nan"))


def test_temporal_moments_refusals(renderer):
    """INVALID_ARG, a message that begins with the pass's name, and nothing written."""
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd.renderer import _c_camera
    from octree_pathtracing_amd.scene import Camera

    lib, ctx = renderer._lib, renderer._ctx
    W = H = 4
    g = flat_guides(H, W)
    color = np.full((H, W, 4), 0.25, F32)
    h_color, h_len, h_m = np.full((H, W, 4), 0.5, F32), np.ones((H, W), np.uint32), np.full((H, W, 2), 0.5, F32)
    out, out_len, out_m = np.full((H, W, 4), 7.0, F32), np.full((H, W), 7, np.uint32), np.full((H, W, 2), 7.0, F32)
    cam = Camera.look_at((3.0, 2.0, -1.0), (3.5, 2.5, 9.0))
    both = _lib.TEMPORAL_MATCH_PRIM | _lib.TEMPORAL_DEMODULATE

    def call(params=None, color_p=ptr(color), guides=None, prev="default", prev_m=ptr(h_m), out_p=ptr(out),
             len_p=ptr(out_len), m_p=ptr(out_m), entry="octpt_temporal_moments", **over):
        f = dict(width=W, height=H, camera=_c_camera(cam), prev_camera=_c_camera(cam), max_history=32,
                 depth_tolerance=0.1, normal_threshold=0.9, flags=both)
        f.update(over)
        p = _lib.TemporalParams(*(f[k] for k, _ in _lib.TemporalParams._fields_))
        gd = {k: ptr(g[k]) for k in ("normal", "depth", "prim", "albedo")}
        gd.update(guides or {})
        hd = dict(color=ptr(h_color), normal=ptr(g["normal"]), depth=ptr(g["depth"]), prim=ptr(g["prim"]),
                  length=ptr(h_len))
        if isinstance(prev, dict):
            hd.update(prev)
        b, h = _lib.AovBuffers(**gd), _lib.TemporalHistory(**hd)
        args = [ctx, None if params == "null" else C.byref(p), color_p, C.byref(b), None if prev is None else C.byref(h)]
        if entry == "octpt_temporal":
            st = lib.octpt_temporal(*args, out_p, len_p)
        else:
            st = lib.octpt_temporal_moments(*args, prev_m, out_p, len_p, m_p)
        if st != _lib.OK:
            assert lib.octpt_last_error(ctx).decode().startswith("temporal_moments" if entry != "octpt_temporal" else "temporal"), \
                lib.octpt_last_error(ctx)
        return st

    refused = [
        dict(params="null"), dict(color_p=None), dict(out_p=None), dict(len_p=None), dict(m_p=None),
        dict(guides=dict(normal=None)), dict(guides=dict(depth=None)), dict(guides=dict(prim=None)),
        dict(guides=dict(albedo=None)),  # the demodulate flag without albedo
        dict(prev=dict(color=None)), dict(prev=dict(normal=None)), dict(prev=dict(depth=None)),
        dict(prev=dict(prim=None)), dict(prev=dict(length=None)),
        dict(prev_m=None),  # d_prev without d_prev_moments
        dict(prev=None),  # d_prev_moments without d_prev
        dict(width=0), dict(height=0), dict(width=1 << 16, height=1 << 15),
        dict(max_history=0), dict(max_history=65536),
        *(dict(depth_tolerance=v) for v in BAD_FLOATS),
        dict(normal_threshold=1.5), dict(normal_threshold=-1.5), dict(normal_threshold=float("nan")),
        dict(flags=4), dict(flags=both | 0x10),
        # the forbidden aliases
        dict(out_p=ptr(h_color)), dict(len_p=ptr(h_len)), dict(m_p=ptr(h_m)),
    ]
    for kw in refused:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert np.all(out == 7.0) and np.all(out_len == 7) and np.all(out_m == 7.0)
    # octpt_temporal still refuses the new flag
    assert call(entry="octpt_temporal", flags=2) == _lib.ERR_INVALID_ARG
    assert call(entry="octpt_temporal", flags=both) == _lib.ERR_INVALID_ARG
    assert np.all(out == 7.0) and np.all(out_len == 7)
    # what is allowed: no albedo without its flag, the first frame with neither history nor moments
    assert call(flags=_lib.TEMPORAL_MATCH_PRIM, guides=dict(albedo=None)) == _lib.OK
    assert call(prev=None, prev_m=None) == _lib.OK
    l = luminance(np.full(3, F32(0.25)) / F32(0.5))
    assert np.array_equal(out, color) and np.all(out_len == 1) and np.allclose(out_m, (l, l * l), rtol=1e-6)


def test_variance_refusals(renderer):
    from octree_pathtracing_amd import _lib

    lib, ctx = renderer._lib, renderer._ctx
    W = H = 4
    g = flat_guides(H, W)
    m, n = np.full((H, W, 2), 0.5, F32), np.ones((H, W), np.uint32)
    out = np.full((H, W), 7.0, F32)

    def call(params=None, m_p=ptr(m), n_p=ptr(n), guides=None, out_p=ptr(out), **over):
        f = dict(width=W, height=H, min_history=4, sigma_normal=0.3, sigma_depth=0.1)
        f.update(over)
        p = _lib.VarianceParams(*(f[k] for k, _ in _lib.VarianceParams._fields_))
        gd = dict(normal=ptr(g["normal"]), depth=ptr(g["depth"]))
        gd.update(guides or {})
        st = lib.octpt_variance(ctx, None if params == "null" else C.byref(p), m_p, n_p, C.byref(_lib.AovBuffers(**gd)),
                                out_p)
        if st != _lib.OK:
            assert lib.octpt_last_error(ctx).decode().startswith("variance"), lib.octpt_last_error(ctx)
        return st

    refused = [
        dict(params="null"), dict(m_p=None), dict(n_p=None), dict(out_p=None),
        dict(guides=dict(normal=None)), dict(guides=dict(depth=None)),
        dict(width=0), dict(height=0), dict(width=1 << 16, height=1 << 15),
        dict(min_history=0), dict(min_history=65536),
        *(dict(sigma_normal=v) for v in BAD_FLOATS), *(dict(sigma_depth=v) for v in BAD_FLOATS),
    ]
    for kw in refused:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert np.all(out == 7.0)
    assert call(min_history=1) == _lib.OK
    assert np.allclose(out, 0.25)  # m2 - m1^2 = 0.5 - 0.25


def test_denoise_variance_refusals(renderer):
    from octree_pathtracing_amd import _lib

    lib, ctx = renderer._lib, renderer._ctx
    W = H = 4
    g = flat_guides(H, W)
    color, var = np.full((H, W, 4), 0.25, F32), np.full((H, W), 0.1, F32)
    out, out_v = np.full((H, W, 4), 7.0, F32), np.full((H, W), 7.0, F32)

    def call(params=None, color_p=ptr(color), var_p=ptr(var), guides=None, out_p=ptr(out), out_v_p=ptr(out_v), **over):
        f = dict(width=W, height=H, iterations=3, sigma_luminance=4.0, luminance_floor=1e-2, sigma_normal=0.3,
                 sigma_depth=0.1, flags=_lib.DENOISE_DEMODULATE)
        f.update(over)
        p = _lib.DenoiseVarianceParams(*(f[k] for k, _ in _lib.DenoiseVarianceParams._fields_))
        gd = dict(normal=ptr(g["normal"]), depth=ptr(g["depth"]), albedo=ptr(g["albedo"]))
        gd.update(guides or {})
        st = lib.octpt_denoise_variance(ctx, None if params == "null" else C.byref(p), color_p, var_p,
                                        C.byref(_lib.AovBuffers(**gd)), out_p, out_v_p)
        if st != _lib.OK:
            assert lib.octpt_last_error(ctx).decode().startswith("denoise_variance"), lib.octpt_last_error(ctx)
        return st

    refused = [
        dict(params="null"), dict(color_p=None), dict(var_p=None), dict(out_p=None),
        dict(guides=dict(normal=None)), dict(guides=dict(depth=None)),
        dict(guides=dict(albedo=None)),  # the demodulate flag without albedo
        dict(width=0), dict(height=0), dict(width=1 << 16, height=1 << 15),
        dict(iterations=0), dict(iterations=6),
        *(dict(**{k: v}) for k in ("sigma_luminance", "luminance_floor", "sigma_normal", "sigma_depth")
          for v in BAD_FLOATS),
        dict(flags=2), dict(flags=_lib.DENOISE_DEMODULATE | 0x10),
    ]
    for kw in refused:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert np.all(out == 7.0) and np.all(out_v == 7.0)
    # what is allowed: no albedo without the flag, no output variance, the outputs aliasing the inputs
    assert call(flags=0, guides=dict(albedo=None)) == _lib.OK
    assert np.abs(out - color).max() <= 1e-6 and np.all(out_v < 0.1) and np.all(out_v > 0)
    assert call(out_v_p=None) == _lib.OK
    assert call(out_p=ptr(color), out_v_p=ptr(var)) == _lib.OK
    assert np.array_equal(var, out_v)
