"""The thin-lens camera without a GPU: octpt_lens_rays, the host's statement of the first ray of
a path-traced sample -- the text the kernels compile (csrc/octpt_lens.h) -- against the float64 reference of
tests/lens_ref.py, its geometry and distribution, its argument checks, and the Python surface."""
import ctypes as C

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd.renderer import lens_rays
from octree_pathtracing_amd.scene import Camera
from tests import lens_ref

F32 = np.float32
CAMERAS = {
    "axis": Camera(eye=(0.0, 0.0, 0.0)).focus((0.0, 0.0, 12.0), 0.35),
    "oblique": Camera.look_at((16.0, 20.0, -14.0), (16.0, 16.0, 16.0)).focus((16.0, 16.0, 16.0), 0.5),
    "narrow": Camera.look_at((3.5, -7.25, 11.0), (-20.0, 4.0, 2.5), up=(0.3, 1.0, -0.2), fov=0.6)
    .focus((-20.0, 4.0, 2.5), 0.8),
}
SIZES = [(37, 21), (8, 8)]
SEED = 7


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def basis(cam):
    eye, d, up = f64(cam.eye), f64(cam.direction), f64(cam.up)
    return eye, d, np.cross(d, up), up


# The bound of tests/test_aov_cpu.py for octpt_camera_rays against its f64 reference: 1e-6 on a unit direction,
# "a few f32 roundings on unit-scale values" (about 8 ulp of 1).
BASE_TOL = 1e-6


def direction_tol(cam) -> float:
    """The direction is t / |t| with t = f - l, one subtraction more than the pinhole ray.  f = nd * focal_scale and
    l = right * (r cos) + up * (r sin) each carry a few f32 roundings relative to their own size -- the budget BASE_TOL
    already grants a unit-scale value -- so t carries at most BASE_TOL * (|f| + |l|) of absolute error and the unit
    direction that over |t| >= |f| - |l|.  For an orthonormal camera nd . direction = d_factor, so |f| >=
    focal_distance, and |l| <= aperture; (|f| + |l|) / (|f| - |l|) falls in |f|, so the factor is at most
    (focal_distance + aperture) / (focal_distance - aperture): 1 for a pinhole, where the bound is test_aov_cpu's."""
    a, fd = cam.aperture, cam.focal_distance
    return BASE_TOL if a == 0.0 else BASE_TOL * (fd + a) / (fd - a)


def origin_tol(cam) -> float:
    """o = eye + l: the same few roundings on a value of the eye's scale, not of unit scale."""
    return BASE_TOL * max(1.0, float(np.abs(f64(cam.eye)).max()) + cam.aperture)


@pytest.mark.parametrize("sample", [0, 5])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(CAMERAS))
def test_lens_rays_match_reference(name, size, sample):
    cam = CAMERAS[name]
    W, H = size
    rays = lens_rays(cam, W, H, SEED, sample)
    assert rays.shape == (H, W, 6) and rays.dtype == np.float32
    ref = lens_ref.lens_rays_f64(cam, W, H, SEED, sample)
    eo = np.abs(rays[..., :3].astype(np.float64) - ref[..., :3]).max()
    ed = np.abs(rays[..., 3:].astype(np.float64) - ref[..., 3:]).max()
    print(f"{name} {W}x{H} s{sample}: origin err {eo:.3e} (tol {origin_tol(cam):.3e}), "
          f"direction err {ed:.3e} (tol {direction_tol(cam):.3e})")
    assert np.abs(np.linalg.norm(rays[..., 3:].astype(np.float64), axis=-1) - 1.0).max() <= 2e-7
    assert eo <= origin_tol(cam)
    assert ed <= direction_tol(cam)


@pytest.mark.parametrize("name", list(CAMERAS))
def test_aperture_zero_is_the_jittered_pinhole(name):
    from dataclasses import replace

    W, H, sample = 37, 21, 3
    pin = replace(CAMERAS[name], aperture=0.0, focal_distance=0.0)
    rays = lens_rays(pin, W, H, SEED, sample)
    assert np.array_equal(rays[..., :3], np.broadcast_to(np.asarray(pin.eye, F32), (H, W, 3)))
    # focal_distance is not read: any value, the same bits
    for fd in (7.0, -3.0, float("nan"), float("inf")):
        other = lens_rays(replace(pin, focal_distance=fd), W, H, SEED, sample)
        assert np.array_equal(rays.view(np.uint32), other.view(np.uint32)), fd
    ref = lens_ref.lens_rays_f64(pin, W, H, SEED, sample)  # the reference's jittered get_ray
    assert np.abs(rays[..., 3:].astype(np.float64) - ref[..., 3:]).max() <= BASE_TOL
    # and the jitter is there: the rays differ from sample to sample and stay within one pixel of the centre ray
    assert not np.array_equal(rays, lens_rays(pin, W, H, SEED, sample + 1))


@pytest.mark.parametrize("name", list(CAMERAS))
def test_lens_geometry(name):
    """In float64 on the published f32 rays: origins on the lens disc, and every ray through the point of the focal
    plane its aperture-0 twin (same seed and sample) goes through."""
    from dataclasses import replace

    cam = CAMERAS[name]
    W, H, sample = 37, 21, 5
    eye, d, right, up = basis(cam)
    rays = lens_rays(cam, W, H, SEED, sample).astype(np.float64)
    twin = lens_rays(replace(cam, aperture=0.0), W, H, SEED, sample).astype(np.float64)
    o, v = rays[..., :3], rays[..., 3:]
    l = o - eye
    scale = max(1.0, np.abs(eye).max() + cam.aperture)
    eps = 2.0 ** -23
    # (o - eye) . dir: l lies in span(right, up), both perpendicular to dir up to look_at's own f32 rounding (a few
    # eps on unit vectors), and o = eye + l rounds once at the eye's scale
    assert np.abs(l @ d).max() <= 4 * eps * (scale + cam.aperture)
    assert np.linalg.norm(l, axis=-1).max() <= cam.aperture * (1.0 + 8 * eps) + eps * scale
    assert np.linalg.norm(l, axis=-1).max() > 0.5 * cam.aperture  # a lens, not a pinhole
    # the focal plane: (p - eye) . dir = focal_distance
    fd = np.float64(F32(cam.focal_distance))
    t_lens = (fd - l @ d) / (v @ d)
    t_twin = fd / (twin[..., 3:] @ d)
    p_lens = o + t_lens[..., None] * v
    p_twin = eye + t_twin[..., None] * twin[..., 3:]
    err = np.abs(p_lens - p_twin).max()
    # both directions are within direction_tol of exact; over the distance to the plane (at most fd / cos of the
    # frame's corner angle, cos >= 0.5 for these cameras) that moves the point by t * tol each, plus the origin's rounding
    bound = 2.0 * fd * (direction_tol(cam) + BASE_TOL) * 2.0 + origin_tol(cam)
    print(f"{name}: focal-plane distance between twin rays {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_lens_distribution():
    """Uniform over the disc: |l|^2 / aperture^2 = u1 is uniform on [0, 1) (mean 1/2, variance 1/12), and the angle is
    uniform, a quarter of the samples per quadrant of (right, up)."""
    cam = CAMERAS["axis"]
    W = H = 64
    S = 16
    eye, d, right, up = basis(cam)
    q, quad = [], np.zeros(4)
    for s in range(S):
        l = lens_rays(cam, W, H, SEED, s)[..., :3].astype(np.float64) - eye
        q.append((l * l).sum(-1) / cam.aperture ** 2)
        a, b = l @ right, l @ up
        for k, m in enumerate([(a >= 0) & (b >= 0), (a < 0) & (b >= 0), (a < 0) & (b < 0), (a >= 0) & (b < 0)]):
            quad[k] += m.sum()
    q = np.concatenate([x.ravel() for x in q])
    n = q.size
    assert n == W * H * S
    se_mean = np.sqrt(1.0 / 12.0 / n)
    print(f"mean of |l|^2/a^2 {q.mean():.5f} (1/2 +- 5 * {se_mean:.2e}); quadrants {quad / n}")
    assert abs(q.mean() - 0.5) <= 5.0 * se_mean
    se_quad = np.sqrt(0.25 * 0.75 / n)  # a binomial share of 1/4
    assert np.abs(quad / n - 0.25).max() <= 5.0 * se_quad


def c_camera(cam, **over):
    f = dict(fov=cam.fov, aperture=cam.aperture, focal_distance=cam.focal_distance)
    f.update(over)
    return _lib.Camera((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.direction), (C.c_float * 3)(*cam.up),
                       f["fov"], f["aperture"], f["focal_distance"])


def test_lens_rays_arguments():
    lib = _lib.load()
    cam = CAMERAS["oblique"]
    W, H = 8, 8
    base = lens_rays(cam, W, H, SEED, 0)
    assert not np.array_equal(base, lens_rays(cam, W, H, SEED + 1, 0))  # another seed
    assert not np.array_equal(base, lens_rays(cam, W, H, SEED, 1))      # another sample
    assert np.array_equal(base, lens_rays(cam, W, H, SEED, 0))          # and nothing else

    sentinel = np.full((H, W, 6), 123.25, np.float32)

    def call(c, w=W, h=H, out=sentinel):
        p = out.ctypes.data_as(C.c_void_p) if out is not None else None
        return lib.octpt_lens_rays(C.byref(c) if c is not None else None, w, h, SEED, 0, p)

    nan, inf = float("nan"), float("inf")
    bad = [c_camera(cam, aperture=-0.1), c_camera(cam, aperture=nan), c_camera(cam, aperture=inf),
           c_camera(cam, focal_distance=0.0), c_camera(cam, focal_distance=-2.0), c_camera(cam, focal_distance=nan),
           c_camera(cam, focal_distance=inf), c_camera(cam, fov=0.0), c_camera(cam, fov=4.0)]
    for c in bad:
        assert call(c) == _lib.ERR_INVALID_ARG
    assert call(None) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), out=None) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), w=0) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), h=0) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), w=1 << 16, h=1 << 15) == _lib.ERR_INVALID_ARG  # 2^31 pixels
    assert np.all(sentinel == 123.25)  # a failed call writes nothing
    assert call(c_camera(cam)) == _lib.OK
    assert np.array_equal(sentinel, base)
    assert C.sizeof(_lib.Camera) == 48  # three vec3, fov, aperture, focal_distance: the ABI layout is unchanged
    assert lib.octpt_abi_version() == 4


def test_python_camera():
    # the positional construction from before the lens fields
    cam = Camera((1.0, 2.0, 3.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 0.9)
    assert cam.aperture == 0.0 and cam.focal_distance == 0.0 and cam.fov == 0.9
    assert Camera().aperture == 0.0
    # Camera::focus (camera.rs:69-73) in f32: focal_distance = (focal_point - eye) . direction
    cam = Camera.look_at((3.5, -7.25, 11.0), (-20.0, 4.0, 2.5), up=(0.3, 1.0, -0.2))
    p = (-18.0, 3.0, 1.5)
    foc = cam.focus(p, 0.3)
    v = np.asarray(p, F32) - np.asarray(cam.eye, F32)
    d = np.asarray(cam.direction, F32)
    want = F32(F32(F32(v[0] * d[0]) + F32(v[1] * d[1])) + F32(v[2] * d[2]))
    assert F32(foc.focal_distance) == want and F32(foc.aperture) == F32(0.3)
    assert (foc.eye, foc.direction, foc.up, foc.fov) == (cam.eye, cam.direction, cam.up, cam.fov)
    assert cam.aperture == 0.0  # a copy, as the reference's builder returns one
