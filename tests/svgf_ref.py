"""DESIGN.md C27-C29 in numpy, written from the contract's text: the luminance moments carried through C26's taps,
the variance made from them, and the variance-guided a-trous filter.  Every operation is one operation of `dtype`
in the contract's order, so with dtype = float32 the text is the kernels' arithmetic and with float64 it is the same
expressions at a precision where their rounding does not matter (the parameters and constants keep their f32
values).  C26's mapping and its counted set are C26's own, always in f32 (tests/temporal_ref.py).  Shared by
tests/test_svgf_cpu.py and tests/test_gpu_svgf.py."""
import numpy as np

from tests.temporal_ref import reproject_ref

F32 = np.float32
ALBEDO_FLOOR = F32(1e-3)
LUMA = (F32(0.2126), F32(0.7152), F32(0.0722))
H_KERNEL = (F32(1 / 16), F32(1 / 4), F32(3 / 8), F32(1 / 4), F32(1 / 16))
G_KERNEL = (F32(1 / 4), F32(1 / 2), F32(1 / 4))


def luminance(s, dtype=F32):
    """l = (0.2126 r + 0.7152 g) + 0.0722 b of [..., 3]."""
    r, g, b = (dtype(c) for c in LUMA)
    return (r * s[..., 0] + g * s[..., 1]) + b * s[..., 2]


def working_signal(color, albedo, hit, demodulate, dtype=F32):
    """C25's: color.rgb, or color.rgb / max(albedo.rgb, 1e-3) on hit pixels when demodulating -> (s, a or None)."""
    s = np.asarray(color, F32)[..., :3].astype(dtype)
    if not demodulate:
        return s, None
    a = np.maximum(np.asarray(albedo, F32)[..., :3], ALBEDO_FLOOR).astype(dtype)
    return np.where(hit[..., None], s / a, s), a


def temporal_moments_ref(color, aov, history, cam, prev_cam, max_history=32, depth_tolerance=0.1, normal_threshold=0.9,
                         match_prim=True, demodulate=False, dtype=F32):
    """C27 -> (moments [H, W, 2] dtype, length [H, W] u32).  history: C26's dict plus "moments", or None."""
    color = np.asarray(color, F32)
    H, W = color.shape[:2]
    depth = np.asarray(aov["depth"], F32).reshape(H, W)
    hit = np.isfinite(depth)
    with np.errstate(all="ignore"):
        s, _ = working_signal(color, aov.get("albedo"), hit, demodulate, dtype)
        l = luminance(s, dtype)
        mu = np.stack([l, l * l], -1)
    zero = np.zeros((H, W, 2), dtype)
    if history is None:
        return np.where(hit[..., None], mu, zero), hit.astype(np.uint32)
    fx, fy, zp, valid = reproject_ref(cam, prev_cam, W, H, depth)
    with np.errstate(all="ignore"):
        inb = valid & (fx >= F32(-1.0)) & (fx < F32(W)) & (fy >= F32(-1.0)) & (fy < F32(H))
        fx, fy = np.where(inb, fx, F32(0.0)), np.where(inb, fy, F32(0.0))
        x0f, y0f = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        n_p = np.asarray(aov["normal"], F32).reshape(H, W, 4)
        h_normal = np.asarray(history["normal"], F32).reshape(H, W, 4)
        h_depth = np.asarray(history["depth"], F32).reshape(H, W)
        h_length = np.asarray(history["length"], np.uint32).reshape(H, W).astype(np.int64)
        h_moments = np.asarray(history["moments"], F32).reshape(H, W, 2).astype(dtype)
        tol, thr = F32(depth_tolerance), F32(normal_threshold)
        B = np.zeros((H, W), F32)  # C26's B: f32, as the colour's
        ms = np.zeros((H, W, 2), dtype)
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
                ms = np.where(counts[..., None], ms + b.astype(dtype)[..., None] * h_moments[Q], ms)
                n_prev = np.where(counts, np.minimum(n_prev, lq), n_prev)
        has = inb & (B >= F32(2.0 ** -10))
        N = np.minimum(n_prev + 1, max_history)
        a = (F32(1.0) / N.astype(F32)).astype(dtype)
        hm = ms / B.astype(dtype)[..., None]
        out = np.where(has[..., None], hm + (mu - hm) * a[..., None], mu)
    out = np.where(hit[..., None], out, zero)
    assert out.dtype == dtype
    return out, np.where(hit, np.where(has, N, 1), 0).astype(np.uint32)


def _window(Hh, W, oy, ox):
    """The pixels p whose tap p + (ox, oy) lies in the image, and those taps: (P, Q) as slice pairs, or None."""
    y0, y1, x0, x1 = max(0, -oy), min(Hh, Hh - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def expf(x):
    """expf of an array of `dtype`, correctly rounded: numpy's own f32 exp is a vector routine that may be a few
    ulp off, so an f32 argument goes through the f64 one and is rounded once."""
    return np.exp(x.astype(np.float64)).astype(x.dtype)


def _edge_weights(n3, depth, P, Q, sn2, sz2):
    """C25's wn and wz of the taps Q as seen from P."""
    d = n3[P] - n3[Q]
    wn = expf(-(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / sn2))
    dz = (depth[P] - depth[Q]) / depth[P]
    return wn, expf(-((dz * dz) / sz2))


def variance_ref(moments, length, normal, depth, min_history=4, sigma_normal=0.3, sigma_depth=0.1, dtype=F32,
                 return_terms=False):
    """C28 -> variance [H, W] dtype; with return_terms also M2 + M1 M1 per pixel, the size of the two terms whose
    difference the variance is (the pixel's own moments on the temporal branch, the window's means on the
    spatial one; 0 on misses)."""
    depth32 = np.asarray(depth, F32)
    Hh, W = depth32.shape
    length = np.asarray(length, np.uint32).reshape(Hh, W)
    ok_px = np.isfinite(depth32) & (length > 0)
    m = np.asarray(moments, F32).reshape(Hh, W, 2).astype(dtype)
    n3 = np.asarray(normal, F32).reshape(Hh, W, 4)[..., :3].astype(dtype)
    z = depth32.astype(dtype)
    # the library squares the sigmas in f32 on the host
    sn2, sz2 = dtype(F32(sigma_normal) * F32(sigma_normal)), dtype(F32(sigma_depth) * F32(sigma_depth))
    with np.errstate(all="ignore"):
        temporal = np.maximum(m[..., 1] - m[..., 0] * m[..., 0], dtype(0))
        num = np.zeros((Hh, W, 2), dtype)
        den = np.zeros((Hh, W), dtype)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                win = _window(Hh, W, dy, dx)
                if win is None:
                    continue
                P, Q = win
                w = np.ones(den[P].shape, dtype)
                if dx or dy:
                    wn, wz = _edge_weights(n3, z, P, Q, sn2, sz2)
                    w = wn * wz
                ok = ok_px[P] & ok_px[Q]
                num[P] = np.where(ok[..., None], num[P] + w[..., None] * m[Q], num[P])
                den[P] = np.where(ok, den[P] + w, den[P])
        M = num / den[..., None]
        n_f = length.astype(F32).astype(dtype)
        spatial = np.maximum(M[..., 1] - M[..., 0] * M[..., 0], dtype(0)) * (dtype(F32(min_history)) / n_f)
        terms = np.where(length >= min_history, m[..., 1] + m[..., 0] * m[..., 0], M[..., 1] + M[..., 0] * M[..., 0])
    v = np.where(ok_px, np.where(length >= min_history, temporal, spatial), dtype(0))
    assert v.dtype == dtype
    return (v, np.where(ok_px, terms, dtype(0))) if return_terms else v


def denoise_variance_ref(color, variance, normal, depth, albedo, iterations=5, sigma_luminance=4.0, luminance_floor=1e-2,
                         sigma_normal=0.3, sigma_depth=0.1, demodulate=True, dtype=F32):
    """C29 -> (out [H, W, 4] dtype, out variance [H, W] dtype)."""
    color = np.asarray(color, F32)
    depth32 = np.asarray(depth, F32)
    Hh, W = depth32.shape
    hit = depth32 != np.inf
    z = depth32.astype(dtype)
    n3 = np.asarray(normal, F32).reshape(Hh, W, 4)[..., :3].astype(dtype)
    v = np.asarray(variance, F32).reshape(Hh, W).astype(dtype)
    sl, fl = dtype(F32(sigma_luminance)), dtype(F32(luminance_floor))
    # the library squares the sigmas in f32 on the host
    sn2, sz2 = dtype(F32(sigma_normal) * F32(sigma_normal)), dtype(F32(sigma_depth) * F32(sigma_depth))
    with np.errstate(all="ignore"):
        s, a = working_signal(color, albedo, hit, demodulate, dtype)
        for i in range(iterations):
            step = 1 << i
            # 1. the variance prefiltered over 3 x 3 at spacing 1
            sv = np.zeros((Hh, W), dtype)
            sg = np.zeros((Hh, W), dtype)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    win = _window(Hh, W, dy, dx)
                    if win is None:
                        continue
                    P, Q = win
                    g = dtype(G_KERNEL[dx + 1]) * dtype(G_KERNEL[dy + 1])
                    ok = hit[P] & hit[Q]
                    sv[P] = np.where(ok, sv[P] + g * v[Q], sv[P])
                    sg[P] = np.where(ok, sg[P] + g, sg[P])
            # 2. the luminance scale
            k = dtype(1) / (sl * np.sqrt(sv / sg) + fl)
            lum = luminance(s, dtype)
            # 3. the taps
            num = np.zeros((Hh, W, 3), dtype)
            vs = np.zeros((Hh, W), dtype)
            den = np.zeros((Hh, W), dtype)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    win = _window(Hh, W, dy * step, dx * step)
                    if win is None:
                        continue
                    P, Q = win
                    w = np.full(den[P].shape, dtype(H_KERNEL[dx + 2]) * dtype(H_KERNEL[dy + 2]), dtype)
                    if dx or dy:
                        wl = expf(-(np.abs(lum[P] - lum[Q]) * k[P]))
                        wn, wz = _edge_weights(n3, z, P, Q, sn2, sz2)
                        w = ((w * wl) * wn) * wz
                    ok = hit[P] & hit[Q]
                    num[P] = np.where(ok[..., None], num[P] + w[..., None] * s[Q], num[P])
                    vs[P] = np.where(ok, vs[P] + (w * w) * v[Q], vs[P])
                    den[P] = np.where(ok, den[P] + w, den[P])
            # 4. the outputs
            s = np.where(hit[..., None], num / den[..., None], s)
            v = np.where(hit, vs / (den * den), v)
        if demodulate:
            s = np.where(hit[..., None], s * a, s)
    out = color.astype(dtype)
    out[..., :3] = np.where(hit[..., None], s, out[..., :3])
    assert out.dtype == dtype and v.dtype == dtype
    return out, v
