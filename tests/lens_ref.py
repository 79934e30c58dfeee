"""A float64 statement of DESIGN.md C37, the first ray of a path-traced sample: the jittered Camera::get_ray
(camera.rs:77-86, tile_renderer.rs:695-703) and, with an aperture, the thin-lens ray through the same point of
the focal plane.  The uniform draws are the oracle's (ref_rng_path_state, ref_rng_next: exact f32 values k / 2^24)
and the lens stream's key is hashed here in numpy; everything after the draws is float64."""
import ctypes as C

import numpy as np

K_LENS = 0x4C454E53  # the lens stream's constant


def lowbias32(x: int) -> int:
    x = np.uint32(x)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return int(x)


def draws(W: int, H: int, seed: int, sample: int):
    """(jitter u [H, W, 2], lens u [H, W, 2]) as float64: the path stream's first two draws and the lens stream's."""
    from oracle import cpu_ref

    lib = cpu_ref.load()
    ju, lu = np.empty((H, W, 2)), np.empty((H, W, 2))
    for y in range(H):
        for x in range(W):
            st0 = lib.ref_rng_path_state(seed, y * W + x, sample)
            st = C.c_uint32(st0)
            ju[y, x] = lib.ref_rng_next(C.byref(st)), lib.ref_rng_next(C.byref(st))
            ls = C.c_uint32(lowbias32(st0 ^ K_LENS))
            lu[y, x] = lib.ref_rng_next(C.byref(ls)), lib.ref_rng_next(C.byref(ls))
    return ju, lu


def lens_rays_f64(cam, W: int, H: int, seed: int, sample: int, u=None) -> np.ndarray:
    """[H, W, 6] float64 (origin, unit direction) of sample `sample` of every pixel; u = draws(...) to reuse."""
    ju, lu = u if u is not None else draws(W, H, seed, sample)
    eye, d, up = (np.asarray(v, np.float32).astype(np.float64) for v in (cam.eye, cam.direction, cam.up))
    fov = np.float64(np.float32(cam.fov))
    d_factor = 1.0 / np.tan(fov / 2.0)
    right = np.cross(d, up)
    dim = float(max(W, H))
    xn = ((2.0 * np.arange(W) + 1.0) - W) / dim
    yn = ((2.0 * (H - np.arange(H)) - 1.0) - H) / dim
    jlo, jhi = -1.0 / dim, 1.0 / dim
    sx = xn[None, :] + (jlo + (jhi - jlo) * ju[..., 0])
    sy = yn[:, None] + (jlo + (jhi - jlo) * ju[..., 1])
    nd = d_factor * d + sx[..., None] * right + sy[..., None] * up
    out = np.empty((H, W, 6))
    a = np.float64(np.float32(cam.aperture))
    if a == 0.0:  # focal_distance is not read
        out[..., :3] = eye
        t = nd
    else:
        fd = np.float64(np.float32(cam.focal_distance))
        r = a * np.sqrt(lu[..., 0])
        phi = 2.0 * np.pi * lu[..., 1]
        l = (r * np.cos(phi))[..., None] * right + (r * np.sin(phi))[..., None] * up
        out[..., :3] = eye + l
        t = nd * (fd / d_factor) - l
    out[..., 3:] = t / np.linalg.norm(t, axis=-1, keepdims=True)
    return out
