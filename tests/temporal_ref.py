"""DESIGN.md C26 in f32 numpy, written from the contract's text: the reprojection mapping and the temporal blend.
Every operation is one correctly rounded f32 operation in the contract's order; tanf comes from the C library, so
d_factor has the library's bits.  Shared by tests/test_temporal_cpu.py and tests/test_gpu_temporal.py."""
import ctypes as C
import ctypes.util

import numpy as np

F32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = C.c_float
_libm.tanf.argtypes = [C.c_float]


def dot(a, b):
    """glam's order: (x.x + y.y) + z.z."""
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def basis(cam):
    """The basis octpt_set_camera derives: eye, dir, right = dir x up, up, d_factor = 1 / tanf(fov / 2)."""
    eye, d, up = ([F32(v) for v in t] for t in (cam.eye, cam.direction, cam.up))
    right = [d[1] * up[2] - up[1] * d[2], d[2] * up[0] - up[2] * d[0], d[0] * up[1] - up[0] * d[1]]
    d_factor = F32(1.0) / F32(_libm.tanf(F32(cam.fov) / F32(2.0)))
    return eye, d, right, up, d_factor


def reproject_ref(cam, prev_cam, W, H, depth):
    """-> fx, fy, zp [H, W] f32 and valid [H, W] bool (finite depth and zc > 0); the first three are only
    meaningful where valid."""
    eye, d, right, up, d_factor = basis(cam)
    peye, pd, pright, pup, pd_factor = basis(prev_cam)
    dim = F32(max(W, H))
    z = np.asarray(depth, F32).reshape(H, W)
    x = np.arange(W, dtype=np.uint32)
    y = np.arange(H, dtype=np.uint32)
    with np.errstate(all="ignore"):
        xc = (((2 * x + 1).astype(F32) - F32(W)) / dim)[None, :]
        yc = (((2 * (H - y) - 1).astype(F32) - F32(H)) / dim)[:, None]
        nd = [(d[i] * d_factor + right[i] * xc) + up[i] * yc for i in range(3)]
        r = F32(1.0) / np.sqrt(dot(nd, nd))
        v = [(eye[i] + (nd[i] * r) * z) - peye[i] for i in range(3)]
        zc = dot(v, pd)
        s = pd_factor / zc
        xn = dot(v, pright) * s
        yn = dot(v, pup) * s
        fx = ((xn * dim + F32(W)) - F32(1.0)) * F32(0.5)
        fy = ((F32(H) - F32(1.0)) - yn * dim) * F32(0.5)
        zp = np.sqrt(dot(v, v))
        valid = np.isfinite(z) & (zc > 0)
    for a in (fx, fy, zp):
        assert a.dtype == F32
    return fx, fy, zp, valid


def coords_ref(cam, prev_cam, W, H, depth):
    """octpt_reproject_coords' outputs: xy [H, W, 2] and zp [H, W]; (NaN, NaN), +inf where not valid."""
    fx, fy, zp, valid = reproject_ref(cam, prev_cam, W, H, depth)
    xy = np.stack([np.where(valid, fx, F32(np.nan)), np.where(valid, fy, F32(np.nan))], axis=-1).astype(F32)
    return xy, np.where(valid, zp, F32(np.inf)).astype(F32)


def temporal_ref(color, aov, history, cam, prev_cam, max_history=32, depth_tolerance=0.1, normal_threshold=0.9,
                 match_prim=True):
    """-> (out [H, W, 4] f32, length [H, W] u32).  history: dict color, normal, depth, prim, length, or None."""
    color = np.asarray(color, F32)
    H, W = color.shape[:2]
    depth = np.asarray(aov["depth"], F32).reshape(H, W)
    hit = np.isfinite(depth)
    out = color.copy()
    length = hit.astype(np.uint32)
    if history is None:
        return out, length
    fx, fy, zp, valid = reproject_ref(cam, prev_cam, W, H, depth)
    with np.errstate(all="ignore"):
        inb = valid & (fx >= F32(-1.0)) & (fx < F32(W)) & (fy >= F32(-1.0)) & (fy < F32(H))  # False on NaN
        fx = np.where(inb, fx, F32(0.0))
        fy = np.where(inb, fy, F32(0.0))
        x0f, y0f = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        n_p = np.asarray(aov["normal"], F32).reshape(H, W, 4)
        h_color = np.asarray(history["color"], F32).reshape(H, W, 4)
        h_normal = np.asarray(history["normal"], F32).reshape(H, W, 4)
        h_depth = np.asarray(history["depth"], F32).reshape(H, W)
        h_length = np.asarray(history["length"], np.uint32).reshape(H, W).astype(np.int64)
        tol, thr = F32(depth_tolerance), F32(normal_threshold)
        B = np.zeros((H, W), F32)
        hs = np.zeros((H, W, 3), F32)
        n_prev = np.full((H, W), 2 ** 32 - 1, np.int64)
        for j in (0, 1):
            for i in (0, 1):
                b = (wx if i else F32(1.0) - wx) * (wy if j else F32(1.0) - wy)
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                Q = (np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1))
                zq, nq, lq = h_depth[Q], h_normal[Q], h_length[Q]
                counts = inb & (b > 0) & inside & np.isfinite(zq) & (lq > 0)
                counts &= np.abs(zq - zp) <= tol * zp
                counts &= (n_p[..., 0] * nq[..., 0] + n_p[..., 1] * nq[..., 1]) + n_p[..., 2] * nq[..., 2] >= thr
                if match_prim:
                    counts &= np.asarray(history["prim"], np.uint32).reshape(H, W)[Q] == \
                        np.asarray(aov["prim"], np.uint32).reshape(H, W)
                B = np.where(counts, B + b, B)
                hs = np.where(counts[..., None], hs + b[..., None] * h_color[Q][..., :3], hs)
                n_prev = np.where(counts, np.minimum(n_prev, lq), n_prev)
        has = inb & (B >= F32(2.0 ** -10))
        N = np.minimum(n_prev + 1, max_history)
        a = F32(1.0) / N.astype(F32)
        h = hs / B[..., None]
        c = color[..., :3]
        out[..., :3] = np.where(has[..., None], h + (c - h) * a[..., None], c)
    assert out.dtype == F32
    length = np.where(hit, np.where(has, N, 1), 0).astype(np.uint32)
    return out, length
