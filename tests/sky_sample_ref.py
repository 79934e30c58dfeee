"""A numpy restatement of the sky map's importance sampling (csrc/octpt_sky_sample.h): the distribution
in float32 operation for operation (its integers must equal the library's), the sample and its pdf in float64, and a
float64 quadrature of the bilinear map over the sphere."""
import math

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
QUANTUM = 65536


def sanitise(texels):
    t = np.asarray(texels, F32)[..., :3].copy()
    with np.errstate(invalid="ignore"):
        t[~(t > 0)] = 0
    return np.minimum(t, FLT_MAX)


def lum32(t):
    with np.errstate(over="ignore"):
        l = (F32(0.2126) * t[..., 0] + F32(0.7152) * t[..., 1]) + F32(0.0722) * t[..., 2]
    return np.minimum(l, FLT_MAX).astype(F32)


def row_table(H):
    return np.sin(np.pi * (np.arange(H, dtype=np.float64) + 0.5) / H).astype(F32)


def neighbourhood_max(l):
    """The maximum over the 3 x 3 neighbourhood, wrapped in x and clamped in y."""
    H, W = l.shape
    ys = [np.clip(np.arange(H) + dy, 0, H - 1) for dy in (-1, 0, 1)]
    xs = [(np.arange(W) + dx) % W for dx in (-1, 0, 1)]
    m = np.zeros_like(l)
    for y in ys:
        for x in xs:
            m = np.maximum(m, l[y][:, x])
    return m


def weights(texels):
    l = lum32(sanitise(texels))
    m = neighbourhood_max(l)
    with np.errstate(over="ignore"):
        w = (m * row_table(l.shape[0])[:, None]).astype(F32)
    return np.minimum(w, FLT_MAX), l


def distribution(texels):
    """{"q", "col_cdf" uint32 [H, W], "row_cdf" uint64 [H], "total"}."""
    w, _ = weights(texels)
    wmax = w.max()
    q = np.zeros(w.shape, np.uint32)
    if wmax > 0:
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.ceil((w / wmax).astype(F32) * F32(QUANTUM)).astype(F32)
        q = np.where(w > 0, np.clip(c, 1, QUANTUM), 0).astype(np.uint32)
    col = np.cumsum(q.astype(np.uint64), axis=1)
    assert col.max(initial=0) < 2 ** 32
    row = np.cumsum(col[:, -1])
    return {"q": q, "col_cdf": col.astype(np.uint32), "row_cdf": row.astype(np.uint64), "total": int(row[-1])}


def q_of(dist):
    col = dist["col_cdf"].astype(np.int64)
    return np.diff(col, axis=1, prepend=0)


def pick(dist, u):
    """(x, y, q) of draws u [n, 4] (float32), by the integers: the row and column rules of the header."""
    row, col = dist["row_cdf"], dist["col_cdf"]
    total = int(row[-1])
    u = np.asarray(u, F32)
    t = np.minimum((u[:, 0] * F32(total)).astype(np.uint64), np.uint64(total - 1))
    y = np.searchsorted(row, t, side="right")
    rowsum = col[y, -1]
    s = np.minimum((u[:, 1] * rowsum.astype(F32)).astype(np.uint32), rowsum - 1)
    x = np.array([np.searchsorted(col[yy], ss, side="right") for yy, ss in zip(y, s)])
    return x, y, q_of(dist)[y, x]


def sample64(dist, u, yaw):
    """The sample in float64 from the f32 draws: (d [n, 3], pdf [n], x, y)."""
    x, y, q = pick(dist, u)
    H, W = dist["col_cdf"].shape
    u = np.asarray(u, np.float64)
    uu, vv = (x + u[:, 2]) / W, (y + u[:, 3]) / H
    theta, lon = np.pi * vv, 2 * np.pi * (uu - 0.5) - float(F32(yaw))
    st = np.sin(theta)
    d = np.stack([st * np.cos(lon), np.cos(theta), st * np.sin(lon)], -1)
    with np.errstate(divide="ignore"):
        pdf = (q / dist["total"]) * (W * H) / (2 * np.pi ** 2 * st)
    return d, pdf, x, y


def lum64(rgb):
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def sphere_integral(texels, sub=16):
    """The integral of lum(bilinear map) over the sphere, float64: the midpoint rule on sub x sub cells per texel."""
    from tests import sky_ref as R

    t = sanitise(texels).astype(np.float64)
    H, W = t.shape[:2]
    fx = (np.arange(W * sub) + 0.5) / sub - 0.5
    fy = (np.arange(H * sub) + 0.5) / sub - 0.5
    FX, FY = np.meshgrid(fx, fy)
    val = lum64(R.bilinear(t, FX.ravel(), FY.ravel())).reshape(FY.shape)
    theta = np.pi * (FY + 0.5) / H
    cell = (2 * np.pi / (W * sub)) * (np.pi / (H * sub))
    return float((val * np.sin(theta)).sum() * cell)


def texel_solid_angle(W, H, y):
    return (2 * math.pi / W) * (math.cos(math.pi * y / H) - math.cos(math.pi * (y + 1) / H))
