"""A restatement of DESIGN.md C41, the first ray of a sample under a ray source, in numpy: the record of the caller's
list at (y, x, sample % R) as given, or the fallback camera's central ray where the record is invalid, and the path's
RNG state after the two jitter draws that are made and dropped.  The validity predicate is evaluated in float32, in the
contract's order -- numpy's float32 products and sums are the IEEE ones, so the restatement is exact, not approximate.
The RNG is tests/projection_ref.py's integer restatement."""
import numpy as np

from tests.projection_ref import path_state, rng_next

F32 = np.float32
BAND = F32(1e-4)


def valid(records: np.ndarray) -> np.ndarray:
    """[..., 6] float32 records -> bool: all six floats finite and |((dx^2 + dy^2) + dz^2) - 1| <= 1e-4 in f32."""
    r = np.asarray(records, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        len2 = (r[..., 3] * r[..., 3] + r[..., 4] * r[..., 4]) + r[..., 5] * r[..., 5]
        unit = np.abs(len2 - F32(1.0)) <= BAND  # False for NaN
    return unit & np.isfinite(r).all(-1)


def central_ray(fallback) -> np.ndarray:
    return np.concatenate([np.asarray(fallback.eye, F32), np.asarray(fallback.direction, F32)])


def effective(fallback, rays: np.ndarray) -> np.ndarray:
    """The list with every invalid record replaced by the fallback's central ray: what a render under it traces."""
    rays = np.asarray(rays, F32)
    return np.where(valid(rays)[..., None], rays, central_ray(fallback)).astype(F32)


def ray_source_rays(fallback, rays: np.ndarray, seed: int, xys):
    """([n, 6] float32 effective rays, [n] uint32 RNG states) for rows (x, y, sample) under the list (H, W, R, 6)."""
    rays = np.asarray(rays, F32)
    H, W, R = rays.shape[:3]
    xys = np.asarray(xys, np.int64).reshape(-1, 3)
    x, y, s = xys[:, 0], xys[:, 1], xys[:, 2]
    out = effective(fallback, rays[y, x, s % R])
    st = path_state(seed, (y * W + x).astype(np.uint32), s.astype(np.uint32))
    st, _ = rng_next(st)
    st, _ = rng_next(st)
    return out, st
