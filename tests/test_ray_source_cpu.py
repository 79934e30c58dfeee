"""The ray-list camera without a GPU: octpt_ray_source_rays, the host's statement of a path's first ray
under a ray source -- the text the kernels compile (csrc/octpt_lens.h's ray_list_ray) -- against the numpy restatement
of tests/ray_source_ref.py, exactly; the RNG state against octpt_projection_rays'; the s % R indexing; every class of
invalid record; the refusals; the worked stereo panorama of octree_pathtracing_amd/rays.py; and the host entry in a
stand-alone program under AddressSanitizer and UBSan (tools/ray_source_host.cpp; nothing is loaded into Python under a
sanitizer)."""
import ctypes as C
import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd.rays import stereo_panorama_rays
from octree_pathtracing_amd.renderer import frame_samples, projection_rays, ray_source_rays
from octree_pathtracing_amd.scene import Camera
from tests import ray_source_ref as RS
from tests.test_projection_cpu import BASE_TOL, ROOM_FRAME, c_camera, inside_camera, room

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
TWO_PI = float(F32(2.0 * math.pi))
SEED = 7
FALLBACK = Camera.look_at((16.0, 20.0, -14.0), (16.0, 16.0, 16.0))
# odd and wide frames, partial 8x8 tiles on both axes
SIZES = [(33, 17), (40, 24), (8, 8)]
NAN, INF = float("nan"), float("inf")
STEREO_IPD = 1.5  # wide against the room, so that the two eyes' frames differ at 40 x 24


def unit_dirs(rng, shape):
    d = rng.normal(size=shape + (3,))
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)


def random_list(W, H, R, seed=3, invalid=0.0):
    """(H, W, R, 6): origins around the scene, float32 unit directions; `invalid`: that fraction of the records made
    invalid, one class after the other (invalid_records)."""
    rng = np.random.default_rng(seed)
    rays = np.concatenate([rng.uniform(-40.0, 40.0, (H, W, R, 3)).astype(F32), unit_dirs(rng, (H, W, R))], -1)
    if invalid:
        flat = rays.reshape(-1, 6)
        bad = invalid_records()
        for k, i in enumerate(rng.choice(len(flat), int(invalid * len(flat)), replace=False)):
            flat[i] = bad[k % len(bad)]
    return rays


def all_samples(W, H, samples):
    return np.concatenate([frame_samples(W, H, s) for s in samples])


def band_edges():
    """The float32 x nearest the band's edges on both sides of 1: (inside_lo, outside_lo, inside_hi, outside_hi), for the
    direction (x, 0, 0), whose squared length is the single f32 product x * x."""
    def ok(x):
        return abs(F32(x) * F32(x) - F32(1.0)) <= RS.BAND

    out = []
    for away in (F32(0.0), F32(2.0)):
        x = F32(1.0)
        while ok(x):  # walk out of the band, one float at a time (about 800 below 1, 400 above)
            x = np.nextafter(x, away)
        inside = np.nextafter(x, F32(1.0))
        assert ok(inside) and not ok(x)
        out += [float(inside), float(x)]
    return out


def invalid_records():
    """One record of every invalid class: a NaN and an infinity of either sign in each of the six floats, a zero and a
    negative-zero direction, directions just outside the band on both sides, a denormal and a huge one (whose squared
    length overflows), and one unit in each component but sqrt(3) long."""
    good = np.array([1.0, 2.0, 3.0, 0.0, 0.6, 0.8], F32)
    out = []
    for k in range(6):
        for v in (NAN, INF, -INF):
            r = good.copy()
            r[k] = v
            out.append(r)
    _, lo, _, hi = band_edges()
    for d in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (lo, 0.0, 0.0), (hi, 0.0, 0.0), (0.0, -lo, 0.0), (0.0, 0.0, hi),
              (1e-42, 0.0, 0.0), (3e38, 3e38, 0.0), (1.0, 1.0, 1.0), (NAN, NAN, NAN)):
        r = good.copy()
        r[3:] = d
        out.append(r)
    return np.array(out, F32)


# ------------------------------------------------------------------ against the restatement, exactly
@pytest.mark.parametrize("R", [1, 3, 4])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rays_match_restatement(size, R):
    W, H = size
    rays = random_list(W, H, R, invalid=0.2)
    xys = all_samples(W, H, (0, 1, 2, 5, 9))  # beyond R for every R here
    got, st = ray_source_rays(FALLBACK, rays, SEED, xys)
    want, wst = RS.ray_source_rays(FALLBACK, rays, SEED, xys)
    assert got.dtype == np.float32 and st.dtype == np.uint32 and got.shape == (len(xys), 6)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(st, wst)
    assert np.isfinite(got).all()
    n_bad = int((~RS.valid(rays)).sum())
    assert 0 < n_bad < rays.size // 6  # the list has both


def test_rng_state_is_every_other_cameras():
    """The state after the ray is lens_ray's: octpt_projection_rays' rng_state for the same (x, y, sample, seed), under
    the pinhole and under a projection."""
    for W, H in SIZES:
        rays = random_list(W, H, 2)
        xys = all_samples(W, H, (0, 3, 70000))
        _, st = ray_source_rays(FALLBACK, rays, SEED, xys)
        for cam in (FALLBACK, FALLBACK.panoramic(TWO_PI), FALLBACK.focus((1.0, 2.0, 30.0), 0.4)):
            assert np.array_equal(st, projection_rays(cam, W, H, SEED, xys)[1])
        assert not np.array_equal(st, ray_source_rays(FALLBACK, rays, SEED + 1, xys)[1])


@pytest.mark.parametrize("R", [1, 3, 4])
def test_sample_indexing(R):
    """Record k of pixel (x, y) carries (x, y, k) as its origin: sample s reads record s % R, for samples beyond R too
    (4 = the spp of the GPU tests)."""
    W, H = 33, 17
    ys, xs, ks = np.mgrid[0:H, 0:W, 0:R]
    rays = np.zeros((H, W, R, 6), F32)
    rays[..., 0], rays[..., 1], rays[..., 2] = xs, ys, ks
    rays[..., 3:] = unit_dirs(np.random.default_rng(1), (H, W, R))
    for s in (0, 1, 2, 3, 4, 7, 11, (1 << 24) - 1):
        got, _ = ray_source_rays(FALLBACK, rays, SEED, frame_samples(W, H, s))
        got = got.reshape(H, W, 6)
        assert np.array_equal(got[..., 0], xs[..., 0]) and np.array_equal(got[..., 1], ys[..., 0])
        assert np.all(got[..., 2] == s % R)
        assert np.array_equal(got[..., 3:].view(np.uint32), rays[:, :, s % R, 3:].view(np.uint32))


# ------------------------------------------------------------------ invalid records
def test_every_invalid_class_yields_the_fallback_ray():
    bad = invalid_records()
    assert not RS.valid(bad).any()
    rays = bad.reshape(1, len(bad), 1, 6)
    got, _ = ray_source_rays(FALLBACK, rays, SEED, frame_samples(len(bad), 1, 0))
    want = RS.central_ray(FALLBACK)
    assert np.array_equal(got.view(np.uint32), np.broadcast_to(want, got.shape).view(np.uint32))


def test_inside_the_band_passes_untouched():
    in_lo, out_lo, in_hi, out_hi = band_edges()
    print(f"band: {out_lo!r} < {in_lo!r} ... {in_hi!r} < {out_hi!r}")
    assert out_lo < in_lo < 1.0 < in_hi < out_hi
    good = []
    for x in (in_lo, in_hi, -in_lo, -in_hi, 1.0):
        for axis in range(3):
            r = np.array([-5.0, 1e30, -0.0, 0.0, 0.0, 0.0], F32)  # any finite origin, a negative zero kept as it is
            r[3 + axis] = x
            good.append(r)
    good.append(np.array([1e-42, 0.0, 3.0, 0.6, 0.0, -0.8], F32))  # a denormal origin
    good = np.array(good, F32)
    assert RS.valid(good).all()
    got, _ = ray_source_rays(FALLBACK, good.reshape(1, len(good), 1, 6), SEED, frame_samples(len(good), 1, 0))
    assert np.array_equal(got.view(np.uint32), good.view(np.uint32))  # not renormalised: the bits as given


# ------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    lib = _lib.load()
    W, H, R = 8, 8, 2
    rays = random_list(W, H, R)
    xys = frame_samples(W, H, 0)
    out = np.full((len(xys), 6), 123.25, np.float32)
    state = np.full(len(xys), 0xA5A5A5A5, np.uint32)

    def call(c, lst=rays, w=W, h=H, r=R, x=xys, o=out, st=state):
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        return lib.octpt_ray_source_rays(C.byref(c) if c is not None else None, ptr(lst), w, h, r, SEED, ptr(x),
                                         len(x) if x is not None else 4, ptr(o), ptr(st))

    cam = c_camera(FALLBACK)
    assert call(None) == _lib.ERR_INVALID_ARG
    assert call(cam, lst=None) == _lib.ERR_INVALID_ARG
    assert call(cam, o=None) == _lib.ERR_INVALID_ARG
    assert call(cam, x=None) == _lib.ERR_INVALID_ARG
    for kw in (dict(w=0), dict(h=0), dict(r=0)):
        assert call(cam, **kw) == _lib.ERR_INVALID_ARG, kw
    # more than 2^28 rays, in any factor (refused before the list is read)
    for kw in (dict(w=1 << 15, h=1 << 14), dict(w=1 << 14, h=1 << 14, r=2), dict(r=(1 << 22) + 1), dict(w=1 << 31, h=2),
               dict(w=0xFFFFFFFF, h=0xFFFFFFFF, r=0xFFFFFFFF)):
        assert call(cam, **kw) == _lib.ERR_INVALID_ARG, kw
    assert call(c_camera(FALLBACK, fov=0.0)) == _lib.ERR_INVALID_ARG  # octpt_lens_rays' camera rules
    assert call(c_camera(FALLBACK, aperture=-1.0)) == _lib.ERR_INVALID_ARG
    for bad_row in ([W, 0, 0], [0, H, 0]):  # a pixel outside the frame, in the last row: nothing before it is written
        x = xys.copy()
        x[-1] = bad_row
        assert call(cam, x=x) == _lib.ERR_INVALID_ARG
    assert np.all(out == 123.25) and np.all(state == 0xA5A5A5A5)  # refused calls write nothing
    # the accepted edges: a NULL state array, an empty batch, exactly 2^28 rays (one sample asked of a list that large
    # is not made here: the list would be 6 GiB)
    assert call(cam, st=None) == _lib.OK
    assert call(cam, x=xys[:0]) == _lib.OK
    assert C.sizeof(_lib.RaySource) == 40
    assert lib.octpt_abi_version() == 4  # additive: the ABI version stays


# ------------------------------------------------------------------ the worked camera: a stereo panorama
def test_stereo_panorama_without_ipd_is_the_panorama():
    for cam in (FALLBACK, inside_camera(), Camera.look_at((3.5, -7.25, 11.0), (-20.0, 4.0, 2.5))):
        for W, H in ((40, 20), (33, 17)):
            for angle in (TWO_PI, 2.0):
                pano = cam.panoramic(angle)
                want, _ = projection_rays(pano, W, H, SEED, frame_samples(W, H, 0), centre=True)
                for eye in (-1, 1, "left"):
                    got = stereo_panorama_rays(pano, W, H, 0.0, eye)
                    assert got.shape == (H, W, 1, 6) and got.dtype == np.float32
                    err = np.abs(got.reshape(-1, 6).astype(np.float64) - want.astype(np.float64))
                    tol_o = BASE_TOL * max(1.0, float(np.abs(np.asarray(cam.eye)).max()))
                    assert err[:, 3:].max() <= BASE_TOL and err[:, :3].max() <= tol_o
                    assert RS.valid(got).all()
        # a camera that is not panoramic gets the full panorama
        a = stereo_panorama_rays(cam, 40, 20, 0.3, 1)
        assert np.array_equal(a, stereo_panorama_rays(cam.panoramic(2.0 * math.pi), 40, 20, 0.3, 1))


def test_stereo_panorama_geometry():
    cam = inside_camera()
    W, H, ipd = 40, 20, 0.5
    left = stereo_panorama_rays(cam, W, H, ipd, "left").reshape(H, W, 6).astype(np.float64)
    right = stereo_panorama_rays(cam, W, H, ipd, "right").reshape(H, W, 6).astype(np.float64)
    eye, up = np.asarray(cam.eye, np.float64), np.asarray(cam.up, np.float64)
    # the list is float32: each origin component is rounded by half an ulp at the eye's scale, a vector error below one
    # ulp, and a unit direction's by 6e-8; twice the ulp bounds every length and dot product below
    tol = 2.0 * float(np.spacing(F32(np.abs(eye).max() + ipd)))
    assert np.allclose(left[..., 3:], right[..., 3:], atol=0, rtol=0)  # one direction per pixel for both eyes
    for rays in (left, right):
        off = rays[..., :3] - eye
        assert np.abs(np.linalg.norm(off, axis=-1) - ipd / 2).max() <= tol  # on the viewing circle
        assert np.abs(off @ up).max() <= tol                                   # which is horizontal
        horiz = rays[..., 3:] - (rays[..., 3:] @ up)[..., None] * up
        assert np.abs((off * horiz).sum(-1)).max() <= tol                      # and the ray is tangent to it
    assert np.abs((left[..., :3] - eye) + (right[..., :3] - eye)).max() <= tol  # the eyes are opposite
    # the right eye sits on the right of the viewing direction: offset . (direction x up) > 0
    side = ((right[..., :3] - eye) * np.cross(right[..., 3:], up)).sum(-1)
    assert (side[H // 2] > 0).all()
    with pytest.raises(ValueError):
        stereo_panorama_rays(cam, W, H, ipd, 0)


def test_closed_room_stereo_reference_rays_all_hit():
    """What tests/test_gpu_ray_source.py's closed-room stereo render relies on, checked here first: every ray of both
    eyes' lists from inside the room meets a wall, by the oracle's closest hit."""
    from oracle import cpu_ref

    W, H, _, _ = ROOM_FRAME
    sc = room()
    for eye in ("left", "right"):
        rays = stereo_panorama_rays(inside_camera(), W, H, STEREO_IPD, eye)
        assert RS.valid(rays).all()
        assert (cpu_ref.intersect(sc, rays.reshape(-1, 6))[1] != 0xFFFFFFFF).all()


# ------------------------------------------------------------------ the host entry under sanitizers
def test_host_entry_under_sanitizers(tmp_path):
    """octpt_ray_source_rays in a program of its own with -fsanitize=address,undefined over lists that hold every
    invalid class, R in {1, 3, 4} and samples beyond R, into exact-size arrays, the refusals included: clean, and the
    rays it prints are the bits the library returns."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "ray_source_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    f"-I{os.environ.get('ROCM_PATH', '/opt/rocm')}/include",
                    str(ROOT / "tools" / "ray_source_host.cpp"),
                    str(ROOT / "octree_pathtracing_amd" / "csrc" / "octpt_host.cpp"), "-o", str(exe)], check=True)
    lines, want = [], []
    S = 6
    for (W, H), R in zip(((9, 5), (8, 8), (13, 3)), (1, 3, 4)):
        rays = random_list(W, H, R, invalid=0.3)
        cam = [float(F32(v)).hex() for v in (*FALLBACK.eye, *FALLBACK.direction, *FALLBACK.up, FALLBACK.fov)]
        words = " ".join(f"{w:x}" for w in rays.view(np.uint32).ravel())
        lines.append(f"{W} {H} {R} {SEED} {S} " + " ".join(cam) + " " + words)
        want.append(ray_source_rays(FALLBACK, rays, SEED, all_samples(W, H, range(S))))
    inp = tmp_path / "cases.txt"
    inp.write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    out = run.stdout.strip().split("\n")
    assert len(out) == len(want)
    for line, (rays, st) in zip(out, want):
        words = np.array([int(w, 16) for w in line.split()], np.uint32)
        assert np.array_equal(words[:rays.size], rays.view(np.uint32).ravel())
        assert np.array_equal(words[rays.size:], st)
