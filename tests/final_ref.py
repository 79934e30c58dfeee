"""numpy restatement of the final-frame rows (include/octpt.h).

C33: the sample clamp, per sample, in the header's order of operations; with dtype = float32 it is resolve's own
arithmetic, bit for bit (the build has no contraction and correctly rounded division).
C34: the seam rule, bit for bit in f32.
C35: the variance of the pixel means, bit for bit in f32.
The _ex driver: C32's seven steps (tests/adaptive_ref.py) with the round's error plane spread before steps 6 and 7.
The filter of C36 is C29's own (tests/svgf_ref.py)."""
import numpy as np

from tests.adaptive_ref import TILE, luminance, tile_grid
from tests.svgf_ref import ALBEDO_FLOOR
from tests.svgf_ref import luminance as luminance_of

F32 = np.float32
F64 = np.float64


def clamp_samples(samples, clamp, dtype=F32):
    """C33 on [..., 3] colours: l = luminance(c); where l > clamp, c * (clamp / l) componentwise.  A NaN l compares
    false and the sample passes unchanged.  Each operation is one operation of `dtype`."""
    c = np.asarray(samples, dtype)
    with np.errstate(all="ignore"):
        l = luminance(c, dtype)
        over = l > dtype(clamp)
        k = np.where(over, dtype(clamp) / np.where(over, l, dtype(1)), dtype(1))
        return np.where(over[..., None], c * k[..., None], c)


def neighbours(W, H, t):
    """The up to eight frame tiles adjacent to tile t in the W x H frame's tile grid."""
    tx, ty = tile_grid(W, H)
    y, x = divmod(int(t), tx)
    return [v * tx + u for v in range(max(y - 1, 0), min(y + 2, ty)) for u in range(max(x - 1, 0), min(x + 2, tx))
            if (u, v) != (x, y)]


def spread_ref(error, W, H, w):
    """C34 -> f32 per tile: max(e[t], w * max of e over t's neighbours); w == 0 copies."""
    e = np.asarray(error, F32).reshape(-1)
    assert e.size == int(np.prod(tile_grid(W, H)))
    if F32(w) == 0:
        return e.copy()
    out = e.copy()
    with np.errstate(all="ignore"):
        for t in range(e.size):
            nb = neighbours(W, H, t)
            if nb:
                out[t] = max(e[t], F32(w) * e[nb].max())
    return out


def sample_variance_ref(moments, tile_spp, depth, albedo=None):
    """C35 -> [H, W] f32, bit for bit.  albedo (not None): the demodulate form."""
    m = np.asarray(moments, F32)
    H, W = m.shape[:2]
    tx, _ = tile_grid(W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    n = np.asarray(tile_spp, np.uint32).reshape(-1)[(ys // TILE) * tx + xs // TILE].astype(np.int64)
    ok = np.isfinite(np.asarray(depth, F32).reshape(H, W)) & (n >= 2)
    with np.errstate(all="ignore"):
        d = m[..., 1] - m[..., 0] * m[..., 0]
        v = np.where(d > 0, d, F32(0))
        v = v / np.maximum(n - 1, 1).astype(F32)
        if albedo is not None:
            a = np.maximum(np.asarray(albedo, F32).reshape(H, W, 4)[..., :3], ALBEDO_FLOOR)
            la = luminance_of(a, F32)
            v = v / (la * la)
    v = np.where(ok, v, F32(0))
    assert v.dtype == F32
    return v


def adaptive_loop_ex(n_tiles, render, error, spread, min_spp, step_spp, max_spp, threshold, on_round=None):
    """The _ex driver: render(active, spp_start, spp_count) adds the samples to the active tiles, error(tile_spp)
    returns the per-tile error plane of the current moments, spread(plane) is C34 of it.  on_round(active, raw, spread
    plane, n): called with each round's tiles before step 6.  Returns (tile_spp, the last round's spread plane,
    rounds)."""
    active = list(range(n_tiles))
    tile_spp = np.zeros(n_tiles, np.uint32)
    err = np.full(n_tiles, np.inf, F32)
    n = rounds = 0
    while active and n < max_spp:
        k = min(min_spp if n == 0 else step_spp, max_spp - n)
        render(active, n, k)
        n += k
        tile_spp[active] = n
        raw = np.asarray(error(tile_spp), F32)
        err = np.asarray(spread(raw), F32)
        if on_round is not None:
            on_round(list(active), raw, err, n)
        active = [t for t in active if err[t] > threshold]
        rounds += 1
    return tile_spp, err, rounds
