"""numpy restatement of the adaptive-sampling rows (include/octpt.h).

C31: the running means of the samples' luminance l and of l * l, from the per-sample colours, in f64 (the device
keeps them in f32 with running_mean's formula; for unit weights both are the plain mean).
C32: the per-tile error with v formed in f32 as the header specifies and the two sums in f64, and the adaptive loop
as the header's seven steps over two callables (render, error)."""
import numpy as np

F32 = np.float32
F64 = np.float64
TILE = 8


def luminance(rgb, dtype=F64):
    """C27's l = (0.2126 r + 0.7152 g) + 0.0722 b, each operation rounded to `dtype`."""
    c = np.asarray(rgb, dtype)
    return (dtype(0.2126) * c[..., 0] + dtype(0.7152) * c[..., 1]) + dtype(0.0722) * c[..., 2]


def sample_moments_ref(samples, weights=None):
    """samples: [n, ..., 3] per-sample colours in sample order; weights: their n weights (branch counts), 1 each by
    default.  Returns [..., 2] f64: the weighted means of l and l * l, what C31's running means converge to."""
    s = np.asarray(samples, F64)
    w = np.ones(len(s), F64) if weights is None else np.asarray(weights, F64)
    l = luminance(s)
    w = w.reshape((-1,) + (1,) * (l.ndim - 1))
    m1 = (l * w).sum(0) / w.sum()
    m2 = (l * l * w).sum(0) / w.sum()
    return np.stack([m1, m2], -1)


def tile_grid(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def tile_pixels(W, H, t):
    """(y slice, x slice) of frame tile t inside the image."""
    tx, _ = tile_grid(W, H)
    y0, x0 = (t // tx) * TILE, (t % tx) * TILE
    return slice(y0, min(y0 + TILE, H)), slice(x0, min(x0 + TILE, W))


def tile_mask(W, H, tiles):
    """[H, W] bool: the pixels of the listed tiles."""
    m = np.zeros((H, W), bool)
    for t in tiles:
        m[tile_pixels(W, H, int(t))] = True
    return m


def tile_error_ref(moments, tile_spp, luminance_floor):
    """C32: one f64 per tile, frame tile order.  v = max(m2 - m1 * m1, 0) in f32 (a NaN stays one), Sv and Sl summed in
    f64 over the tile's P pixels inside the image, error = sqrt((Sv / P) / (n - 1)) / (Sl / P + floor); n < 2 and a
    result that is not finite are +inf."""
    m = np.asarray(moments, F32)
    H, W = m.shape[:2]
    tx, ty = tile_grid(W, H)
    n_all = np.asarray(tile_spp).reshape(-1)
    assert n_all.size == tx * ty
    d = m[..., 1] - m[..., 0] * m[..., 0]  # f32, each operation rounded
    v = np.where(d < 0, F32(0), d).astype(F64)
    out = np.full(tx * ty, np.inf, F64)
    for t in range(tx * ty):
        n = int(n_all[t])
        if n < 2:
            continue
        ys, xs = tile_pixels(W, H, t)
        P = (ys.stop - ys.start) * (xs.stop - xs.start)
        Sv, Sl = v[ys, xs].sum(), m[ys, xs, 0].astype(F64).sum()
        with np.errstate(all="ignore"):
            e = np.sqrt((Sv / P) / (n - 1)) / (Sl / P + F64(F32(luminance_floor)))
        if np.isfinite(e):
            out[t] = e
    return out


def adaptive_loop(n_tiles, render, error, min_spp, step_spp, max_spp, threshold):
    """The header's seven steps.  render(active, spp_start, spp_count) adds the samples to the active tiles;
    error(tile_spp) returns the per-tile error of the current moments.  Returns (tile_spp, last errors, rounds)."""
    active = list(range(n_tiles))
    tile_spp = np.zeros(n_tiles, np.uint32)
    err = np.full(n_tiles, np.inf, F32)
    n = rounds = 0
    while active and n < max_spp:
        k = min(min_spp if n == 0 else step_spp, max_spp - n)
        render(active, n, k)
        n += k
        tile_spp[active] = n
        e = np.asarray(error(tile_spp))
        err[active] = e[active]
        active = [t for t in active if e[t] > threshold]
        rounds += 1
    return tile_spp, err, rounds
