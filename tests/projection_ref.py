"""A restatement of DESIGN.md C40, the first ray of a sample under a camera projection (pinhole, parallel, equidistant
fisheye, equirectangular panorama), in numpy.  The counter-based RNG is restated here in integer
arithmetic, its draws are exact f32 values k / 2^24; everything after them is evaluated in `dtype`: float64 is the
reference, float32 the same formulas in the contract's order with numpy's sin and cos (what the tolerance of
tests/test_projection_cpu.py is measured from)."""
import numpy as np

PINHOLE, PARALLEL, FISHEYE, PANORAMIC = 0, 1, 2, 3
U32 = np.uint32


def lowbias32(x):
    x = np.asarray(x, U32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U32(16)
        x *= U32(0x7FEB352D)
        x ^= x >> U32(15)
        x *= U32(0x846CA68B)
        x ^= x >> U32(16)
    return x


def path_state(seed: int, pixel, sample):
    h = lowbias32(U32(seed ^ 0xA511E9B3))
    h = lowbias32(h ^ np.asarray(pixel, U32))
    with np.errstate(over="ignore"):
        return lowbias32(h ^ (np.asarray(sample, U32) * U32(0x9E3779B9)))


def rng_next(st):
    """(new state, draw as float64: an exact multiple of 2^-24 in [0, 1))."""
    with np.errstate(over="ignore"):
        s = st * U32(747796405) + U32(2891336453)
        w = ((s >> ((s >> U32(28)) + U32(4))) ^ s) * U32(277803737)
    w = (w >> U32(22)) ^ w
    return s, (w >> U32(8)).astype(np.float64) / 16777216.0


def screen(W: int, H: int, seed: int, xys, centre: bool, dtype):
    """(sx, sy, rng state after the ray) of rows (x, y, sample): the common part of every mode."""
    xys = np.asarray(xys, np.int64).reshape(-1, 3)
    x, y, s = xys[:, 0], xys[:, 1], xys[:, 2]
    T = dtype
    dim = T(max(W, H))
    xn = (T(1) * (2 * x + 1).astype(T) - T(W)) / dim
    yn = (T(1) * (2 * (H - y) - 1).astype(T) - T(H)) / dim
    st = path_state(seed, (y * W + x).astype(U32), s.astype(U32))
    if centre:
        return xn, yn, st
    jlo, jhi = T(-1) / dim, T(1) / dim
    st, u1 = rng_next(st)
    st, u2 = rng_next(st)
    dx = jlo + (jhi - jlo) * u1.astype(T)
    dy = jlo + (jhi - jlo) * u2.astype(T)
    return xn + dx, yn + dy, st


def projection_rays(cam, W: int, H: int, seed: int, xys, centre: bool = False, dtype=np.float64):
    """([n, 6] rays (origin, unit direction) in `dtype`, [n] uint32 RNG states) under cam.projection = (mode, param).
    The camera's and the projection's values are their f32 values, as the library receives them."""
    T = dtype
    mode, param = cam.projection
    eye, d, up = (np.asarray(v, np.float32).astype(T) for v in (cam.eye, cam.direction, cam.up))
    right = np.array([d[1] * up[2] - up[1] * d[2], d[2] * up[0] - up[2] * d[0], d[0] * up[1] - up[0] * d[1]], T)
    sx, sy, st = screen(W, H, seed, xys, centre, T)
    sx, sy = sx[:, None], sy[:, None]
    half = T(np.float32(param)) * T(0.5)
    o = np.broadcast_to(eye, (len(sx), 3)).astype(T)
    if mode == PINHOLE:
        d_factor = T(1) / np.tan(T(np.float32(cam.fov)) / T(2))
        t = (d * d_factor + right * sx) + up * sy
    elif mode == PARALLEL:
        o = (eye + right * (sx * half)) + up * (sy * half)
        t = np.broadcast_to(d, (len(sx), 3)).astype(T)
    elif mode == FISHEYE:
        ax, ay = sx * half, sy * half
        ang = np.sqrt(ax * ax + ay * ay)
        safe = np.where(ang == 0, T(1), ang)
        k = np.sin(safe) / safe
        t = np.where(ang == 0, d, (d * np.cos(safe) + right * (ax * k)) + up * (ay * k))
    elif mode == PANORAMIC:
        lon, lat = sx * half, sy * half
        cl, sl = np.cos(lat), np.sin(lat)
        t = (d * (cl * np.cos(lon)) + right * (cl * np.sin(lon))) + up * sl
    else:
        raise ValueError(f"unknown projection mode {mode}")
    t = t.astype(T)
    n = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
    dirs = t * (T(1) / n)[:, None]
    return np.concatenate([o, dirs], 1).astype(T), st
