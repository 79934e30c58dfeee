"""The sky of DESIGN.md C42 restated in numpy float64: what csrc/octpt_sky.h's sky_radiance states in f32, with libm's
atan2 and acos.  A sky is a dict: mode, color, horizon, zenith, scale, yaw, and for a MAP texels (H, W, 3 or 4)."""
import numpy as np

DEFAULT, COLOR, GRADIENT, MAP = 0, 1, 2, 3


def map_position(d, W, H, yaw):
    """(fx, fy) [n] of unit directions d [n, 3]: the lookup position in texels."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    lon = np.arctan2(d[:, 2], d[:, 0]) + float(yaw)
    u = lon / (2.0 * np.pi) + 0.5
    u = u - np.floor(u)
    v = np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi
    return u * W - 0.5, v * H - 0.5


def bilinear(texels, fx, fy):
    """Taps at floor and floor + 1, wrapped in x, clamped in y; a + w * (b - a), x first, then y."""
    t = np.asarray(texels, np.float64)[..., :3]
    H, W = t.shape[:2]
    x0f, y0f = np.floor(fx), np.floor(fy)
    wx, wy = (fx - x0f)[:, None], (fy - y0f)[:, None]
    x0 = x0f.astype(np.int64) % W
    x1 = (x0 + 1) % W
    y0 = np.clip(y0f.astype(np.int64), 0, H - 1)
    y1 = np.clip(y0f.astype(np.int64) + 1, 0, H - 1)
    top = t[y0, x0] + wx * (t[y0, x1] - t[y0, x0])
    bot = t[y1, x0] + wx * (t[y1, x1] - t[y1, x0])
    return top + wy * (bot - top)


def radiance(sky, d):
    """[n, 3] float64."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    mode = sky.get("mode", DEFAULT)
    scale = float(sky.get("scale", 1.0))
    if mode == DEFAULT:
        return np.tile(np.array([0.5, 0.7, 1.0]), (len(d), 1))
    if mode == COLOR:
        return np.tile(np.asarray(sky["color"], np.float64) * scale, (len(d), 1))
    if mode == GRADIENT:
        h, z = np.asarray(sky["horizon"], np.float64), np.asarray(sky["zenith"], np.float64)
        return (h + (z - h) * np.maximum(d[:, 1], 0.0)[:, None]) * scale
    t = np.asarray(sky["texels"])
    fx, fy = map_position(d, t.shape[1], t.shape[0], sky.get("yaw", 0.0))
    return bilinear(t, fx, fy) * scale


def neighbour_difference(texels):
    """The largest difference between neighbouring texels of a map, per the lookup's neighbourhoods: along x
    (wrapped) and along y, over the colour channels."""
    t = np.asarray(texels, np.float64)[..., :3]
    dx = np.abs(t - np.roll(t, -1, axis=1)).max()
    dy = np.abs(t[1:] - t[:-1]).max() if t.shape[0] > 1 else 0.0
    return float(max(dx, dy))


def texel_centre_dirs(W, H):
    """Unit directions [H, W, 3] through the texel centres of a W x H map at yaw 0 (float64)."""
    u = (np.arange(W) + 0.5) / W
    v = (np.arange(H) + 0.5) / H
    lon = (u - 0.5) * 2.0 * np.pi
    th = v * np.pi
    d = np.empty((H, W, 3))
    d[..., 0] = np.sin(th)[:, None] * np.cos(lon)[None, :]
    d[..., 1] = np.cos(th)[:, None]
    d[..., 2] = np.sin(th)[:, None] * np.sin(lon)[None, :]
    return d


def direction_set(W, H, n_random=4000, seed=5):
    """The directions of the CPU test (float32 [n, 3], unit in f32 up to rounding): the six axes (both poles among
    them), both sides of the lon = +-pi seam at several latitudes, texel centres and texel edges of a W x H map, and
    n_random random unit vectors."""
    rng = np.random.default_rng(seed)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    seam = []
    for y in (-0.9, -0.3, 0.0, 0.4, 0.95):
        r = np.sqrt(1.0 - y * y)
        for eps in (1e-7, 1e-5, 1e-3):
            for s in (1.0, -1.0):
                a = np.pi - eps
                seam.append([r * np.cos(a), y, s * r * np.sin(a)])
        seam.append([-r, y, 0.0])
        seam.append([-r, y, -0.0])
    centres = texel_centre_dirs(W, H).reshape(-1, 3)
    # texel edges: the corners of the texel grid (poles excluded: they are among the axes)
    u = np.arange(W) / W
    v = np.arange(1, H) / H
    lon = (u - 0.5) * 2.0 * np.pi
    th = v * np.pi
    edges = np.stack([np.sin(th)[:, None] * np.cos(lon)[None, :], np.broadcast_to(np.cos(th)[:, None], (H - 1, W)),
                      np.sin(th)[:, None] * np.sin(lon)[None, :]], -1).reshape(-1, 3)
    rnd = rng.normal(size=(n_random, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([axes, np.array(seam), centres, edges, rnd]), np.float32)
