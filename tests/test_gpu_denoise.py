"""The edge-avoiding a-trous denoiser (octpt_denoise, atrous_kernel) against an f32 numpy
restatement of the contract, written from its text: same taps, same weights, same order of operations."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
# the project's forward tolerance (tests/test_gpu_parity.py) plus an absolute floor: the device's expf and
# numpy's differ by ulps, and the normalised 25-term sum keeps that below 1e-6
REL, ABS = 1e-5, 1e-6
H_KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F32)


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


def atrous_ref(color, normal, depth, albedo, iterations, sigma_color, sigma_normal, sigma_depth, demodulate):
    """C25 in f32 numpy.  Iteration i, pixel p with finite depth: taps q = p + 2^i (dx, dy), dx, dy in -2..2,
    row-major; outside the image or infinite depth: skipped; w = h[dx] h[dy] wc wn wz, the centre tap's edge
    weights 1; out = sum w s_q / sum w.  Miss pixels are copied through."""
    Hh, W = depth.shape
    hit = np.isfinite(depth)
    s = color[..., :3].astype(F32).copy()
    a = None
    with np.errstate(all="ignore"):
        if demodulate:
            a = np.maximum(albedo[..., :3], F32(1e-3))
            s = np.where(hit[..., None], s / a, s)
        sn2 = F32(sigma_normal) * F32(sigma_normal)
        sz2 = F32(sigma_depth) * F32(sigma_depth)
        n3 = normal[..., :3]
        for i in range(iterations):
            step = 1 << i
            sc = F32(sigma_color) * F32(2.0 ** -i)
            sc2 = sc * sc
            num = np.zeros((Hh, W, 3), F32)
            den = np.zeros((Hh, W), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * step, dx * step
                    y0, y1, x0, x1 = max(0, -oy), min(Hh, Hh - oy), max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    w = np.full((y1 - y0, x1 - x0), H_KERNEL[dx + 2] * H_KERNEL[dy + 2], F32)
                    if dx or dy:
                        d = s[P] - s[Q]
                        wc = np.exp(-(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / sc2))
                        d = n3[P] - n3[Q]
                        wn = np.exp(-(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / sn2))
                        dz = (depth[P] - depth[Q]) / depth[P]
                        wz = np.exp(-((dz * dz) / sz2))
                        w = ((w * wc) * wn) * wz
                    ok = hit[P] & hit[Q]
                    w = np.where(ok, w, F32(0)).astype(F32)
                    num[P] = num[P] + np.where(ok[..., None], w[..., None] * s[Q], F32(0))
                    den[P] = den[P] + w
            s = np.where(hit[..., None], num / den[..., None], s).astype(F32)
        if demodulate:
            s = np.where(hit[..., None], s * a, s)
    out = color.astype(F32).copy()
    out[..., :3] = np.where(hit[..., None], s, color[..., :3])
    return out


def close(got, ref):
    return np.abs(got - ref) <= REL * np.abs(ref) + ABS


@pytest.fixture(scope="module")
def frames(renderer):
    """(W, H) -> an 8-spp C3 render and its guide buffers, computed once."""
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.scene import RenderSettings

    sc, cam, _ = S.make_config("C3")
    renderer.set_scene(sc)
    renderer.set_camera(cam)
    out = {}
    for W, H in [(64, 64), (37, 21)]:
        rs = RenderSettings(W, H, 8)
        color, _ = renderer.render(rs)
        out[(W, H)] = (color, renderer.render_aov(rs))
    return out


SIGMAS = dict(sigma_color=0.6, sigma_normal=0.3, sigma_depth=0.1)


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulate", "plain"])
@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("size", [(64, 64), (37, 21)], ids=["64x64", "37x21"])
def test_matches_restatement(renderer, frames, size, iterations, demodulate):
    """Within 1e-5 relative + 1e-6 absolute of the restatement; miss pixels and alpha bit-identical to the
    input.  At 37x21 the spacing-16 pass of 5 iterations is mostly out of the image."""
    color, aov = frames[size]
    hit = np.isfinite(aov["depth"])
    assert hit.any() and (~hit).any()
    got = renderer.denoise(color, aov, iterations=iterations, demodulate=demodulate, **SIGMAS)
    ref = atrous_ref(color, aov["normal"], aov["depth"], aov["albedo"], iterations, demodulate=demodulate, **SIGMAS)
    assert np.all(np.isfinite(got))
    bad = ~close(got, ref)
    assert not bad.any(), (int(bad.sum()), float(np.abs(got - ref).max()))
    assert np.array_equal(got[~hit].view(np.uint32), color[~hit].view(np.uint32))
    assert np.array_equal(got[..., 3].view(np.uint32), color[..., 3].view(np.uint32))
    # the filter does something: a hit pixel with hit neighbours changes
    assert np.abs(got[hit] - color[hit]).max() > 1e-3


def test_in_place_equals_out_of_place(renderer, frames, torch_cuda):
    from octree_pathtracing_amd import _lib

    torch = torch_cuda
    color, aov = frames[(64, 64)]
    H, W = color.shape[:2]
    g = {k: torch.as_tensor(aov[k], device="cuda").contiguous() for k in ("albedo", "normal", "depth")}
    ptrs = {k: v.data_ptr() for k, v in g.items()}
    p = _lib.DenoiseParams(W, H, 3, 0.6, 0.3, 0.1, _lib.DENOISE_DEMODULATE)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = torch.as_tensor(color, device="cuda").contiguous()
        b = a.clone()
        out = torch.zeros_like(a)
        renderer.denoise_device(p, a.data_ptr(), ptrs, out.data_ptr(), s.cuda_stream)
        renderer.denoise_device(p, b.data_ptr(), ptrs, b.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(a.cpu().numpy(), color)  # the out-of-place input is left alone
    assert np.array_equal(out.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    host = renderer.denoise(color, aov, iterations=3, demodulate=True, **SIGMAS)
    assert np.array_equal(host.view(np.uint32), out.cpu().numpy().view(np.uint32))


def flat_guides(H, W):
    normal = np.zeros((H, W, 4), F32)
    normal[..., 2] = 1.0
    return {"normal": normal, "depth": np.full((H, W), 10.0, F32), "albedo": np.full((H, W, 4), 0.5, F32)}


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulate", "plain"])
def test_constant_frame_is_unchanged(renderer, demodulate):
    H, W = 40, 52
    color = np.empty((H, W, 4), F32)
    color[...] = (0.25, 0.5, 0.75, 1.0)
    got = renderer.denoise(color, flat_guides(H, W), iterations=5, demodulate=demodulate, **SIGMAS)
    assert np.abs(got - color).max() <= 1e-6


def step_frame():
    """Left of column 20: one colour, depth 10, normal +Z; right of it: another colour, depth 20, normal +X."""
    H, W, X = 33, 45, 20
    g = flat_guides(H, W)
    g["normal"][:, X:] = (1.0, 0.0, 0.0, 0.0)
    g["depth"][:, X:] = 20.0
    color = np.empty((H, W, 4), F32)
    color[:, :X] = (0.9, 0.2, 0.1, 1.0)
    color[:, X:] = (0.1, 0.3, 0.8, 1.0)
    return color, g, X


def test_edges_stop_the_filter(renderer):
    """sigma_normal = sigma_depth = 1e-3 across a depth and normal discontinuity (the colour sigma wide open):
    neither side's colour bleeds into the other, each keeps its mean to 1e-4."""
    color, g, X = step_frame()
    got = renderer.denoise(color, g, iterations=5, sigma_color=1e3, sigma_normal=1e-3, sigma_depth=1e-3,
                           demodulate=False)
    for side in (slice(0, X), slice(X, None)):
        assert np.abs(got[:, side].mean(axis=(0, 1)) - color[:, side].mean(axis=(0, 1))).max() <= 1e-4
        assert np.abs(got[:, side] - color[:, side]).max() <= 1e-4


def b3_blur(color, iterations):
    """The plain a-trous B3-spline blur: every edge weight 1, renormalised at the image border."""
    s = color[..., :3].astype(np.float64)
    H, W = s.shape[:2]
    for i in range(iterations):
        step = 1 << i
        num, den = np.zeros_like(s), np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                w = float(H_KERNEL[dx + 2]) * float(H_KERNEL[dy + 2])
                num[y0:y1, x0:x1] += w * s[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
                den[y0:y1, x0:x1] += w
        s = num / den[..., None]
    return s


def test_wide_sigmas_tend_to_the_b3_blur(renderer):
    """All sigmas 1e3: the normal and depth weights are exp(-d^2 / 1e6) with d^2 <= 2 and <= 1, the colour
    weight of pass i is exp(-d^2 / (1e3 / 2^i)^2) with d^2 <= 1.14 for the two colours here, at worst
    (i = 2) 1 - 1.8e-5; so every weight is within 2.1e-5 of 1 and each of the three passes is the B3-spline
    blur to about 2e-5 of the signal's range (0.8): 1e-4 bounds the three together.  The blur itself moves
    the step's neighbourhood by far more."""
    color, g, X = step_frame()
    got = renderer.denoise(color, g, iterations=3, sigma_color=1e3, sigma_normal=1e3, sigma_depth=1e3,
                           demodulate=False)
    want = b3_blur(color, 3)
    assert np.abs(got[..., :3] - want).max() <= 1e-4
    assert np.abs(want - color[..., :3]).max() > 0.1
    ref = atrous_ref(color, g["normal"], g["depth"], g["albedo"], 3, 1e3, 1e3, 1e3, False)
    assert close(got, ref).all()
