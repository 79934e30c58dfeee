"""Camera projections without a GPU: octpt_projection_rays, the host's statement of a path's first ray
under the parallel, fisheye and panoramic projections -- the text the kernels compile (csrc/octpt_lens.h) -- against
the float64 restatement of tests/projection_ref.py, the exact statements of the contract, the refusals, the Python
surface, and the host entry in a stand-alone program under AddressSanitizer and UBSan (tools/projection_rays_host.cpp;
nothing is loaded into Python under a sanitizer)."""
import ctypes as C
import math
import os
import shutil
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd.renderer import frame_samples, lens_rays, projection_rays
from octree_pathtracing_amd.scene import Camera
from tests import projection_ref as P

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
TWO_PI = float(F32(2.0 * math.pi))
SEED = 7

CAMERAS = {
    "axis": Camera(eye=(0.0, 0.0, 0.0)),
    "oblique": Camera.look_at((16.0, 20.0, -14.0), (16.0, 16.0, 16.0)),
    "rolled": Camera.look_at((3.5, -7.25, 11.0), (-20.0, 4.0, 2.5), up=(0.3, 1.0, -0.2), fov=0.6),
}
# odd and even W and H, W > H and H > W, one partial 8x8 tile and whole ones
SIZES = [(37, 21), (8, 8), (12, 30), (48, 24)]
# small values and the largest angle; the parallel extent small and large against the eye
PARAMS = {P.PINHOLE: [0.0], P.PARALLEL: [0.25, 40.0], P.FISHEYE: [0.05, math.pi, TWO_PI],
          P.PANORAMIC: [0.05, math.pi, TWO_PI]}
MODE_NAMES = {P.PINHOLE: "pinhole", P.PARALLEL: "parallel", P.FISHEYE: "fisheye", P.PANORAMIC: "panoramic"}


def samples(W, H):
    """Every pixel of the frame -- its corners and its centre pixel among them -- at samples 0 and 5."""
    xys = np.concatenate([frame_samples(W, H, 0), frame_samples(W, H, 5)])
    px = {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)}
    assert px <= {(int(a), int(b)) for a, b, _ in xys}
    return xys


# The bound of tests/test_lens_cpu.py for a unit direction against its f64 reference: 1e-6, "a few f32 roundings on
# unit-scale values"; an origin carries the same roundings at its own scale.
BASE_TOL = 1e-6
# Every mode meets it, dm_sincos on the wider domain included (lon, lat in [-pi, pi], fisheye angles up to 3.9 on
# these frames): measured over the cameras, sizes, params and samples below, octpt_projection_rays is within 4.2e-7
# (fisheye) and 2.8e-7 (panoramic) of float64, and the contract's formulas evaluated in numpy float32 within 4.6e-7
# and 2.8e-7 (test_f32_formula_error prints them), so no wider bound is derived.
DIR_TOL = {m: BASE_TOL for m in (P.PINHOLE, P.PARALLEL, P.FISHEYE, P.PANORAMIC)}


def origin_tol(cam) -> float:
    """test_lens_cpu's: the eye's scale plus the offset's (a parallel origin lies within param of the eye)."""
    mode, param = cam.projection
    return BASE_TOL * max(1.0, float(np.abs(np.asarray(cam.eye, np.float64)).max()) + (param if mode == P.PARALLEL else 0.0))


def cases():
    for name, cam in CAMERAS.items():
        for mode, params in PARAMS.items():
            for param in params:
                yield pytest.param(replace(cam, projection=(mode, param)), id=f"{name}-{MODE_NAMES[mode]}-{param:.3g}")


@pytest.mark.parametrize("centre", [False, True], ids=["jittered", "centre"])
@pytest.mark.parametrize("cam", cases())
def test_rays_match_reference(cam, centre):
    mode = cam.projection[0]
    worst_o = worst_d = 0.0
    for W, H in SIZES:
        xys = samples(W, H)
        rays, st = projection_rays(cam, W, H, SEED, xys, centre=centre)
        assert rays.shape == (len(xys), 6) and rays.dtype == np.float32 and st.dtype == np.uint32
        ref, rst = P.projection_rays(cam, W, H, SEED, xys, centre=centre)
        assert np.array_equal(st, rst)
        worst_o = max(worst_o, np.abs(rays[:, :3].astype(np.float64) - ref[:, :3]).max())
        worst_d = max(worst_d, np.abs(rays[:, 3:].astype(np.float64) - ref[:, 3:]).max())
        assert np.abs(np.linalg.norm(rays[:, 3:].astype(np.float64), axis=-1) - 1.0).max() <= 2e-7
    print(f"origin err {worst_o:.3e} (tol {origin_tol(cam):.3e}), direction err {worst_d:.3e} (tol {DIR_TOL[mode]:.3e})")
    assert worst_o <= origin_tol(cam)
    assert worst_d <= DIR_TOL[mode]


def test_f32_formula_error():
    """The contract's formulas in numpy float32 against float64 on the inputs of test_rays_match_reference: the lens
    tolerance is one that plain f32 arithmetic meets in every mode, so it is the bound and no wider one is derived."""
    worst = {m: 0.0 for m in PARAMS}
    for cam in (c.values[0] for c in cases()):
        for W, H in SIZES:
            xys = samples(W, H)
            a, _ = P.projection_rays(cam, W, H, SEED, xys, dtype=np.float32)
            b, _ = P.projection_rays(cam, W, H, SEED, xys)
            m = cam.projection[0]
            worst[m] = max(worst[m], np.abs(a[:, 3:].astype(np.float64) - b[:, 3:]).max())
    print({MODE_NAMES[m]: f"{v:.3e}" for m, v in worst.items()})
    assert max(worst.values()) <= BASE_TOL


@pytest.mark.parametrize("name", list(CAMERAS))
def test_pinhole_is_lens_rays_bit_for_bit(name):
    for cam in (CAMERAS[name], CAMERAS[name].focus((1.0, 2.0, 30.0), 0.4)):
        for W, H in SIZES[:2]:
            for s in (0, 5):
                got, _ = projection_rays(cam, W, H, SEED, frame_samples(W, H, s))
                want = lens_rays(cam, W, H, SEED, s).reshape(-1, 6)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    from octree_pathtracing_amd.renderer import camera_rays

    got, _ = projection_rays(CAMERAS[name], 37, 21, SEED, frame_samples(37, 21, 3), centre=True)
    assert np.array_equal(got.view(np.uint32), camera_rays(CAMERAS[name], 37, 21).reshape(-1, 6).view(np.uint32))


@pytest.mark.parametrize("name", list(CAMERAS))
def test_exact_statements(name):
    base = CAMERAS[name]
    W, H = 37, 21
    xys = samples(W, H)
    eye = np.broadcast_to(np.asarray(base.eye, F32), (len(xys), 3))
    states = []
    for mode, params in PARAMS.items():
        for param in params:
            rays, st = projection_rays(replace(base, projection=(mode, param)), W, H, SEED, xys)
            states.append(st)
            if mode == P.PARALLEL:  # one direction, the camera's, normalised once; the origins differ
                assert len(np.unique(rays[:, 3:].view(np.uint32), axis=0)) == 1
                assert len(np.unique(rays[:, :3], axis=0)) > len(xys) // 2
            else:
                assert np.array_equal(rays[:, :3].view(np.uint32), eye.view(np.uint32))
    for st in states[1:]:  # the returned RNG state does not depend on the projection
        assert np.array_equal(st, states[0])
    _, st_centre = projection_rays(replace(base, projection=(P.FISHEYE, 1.0)), W, H, SEED, xys, centre=True)
    assert np.array_equal(st_centre, P.path_state(SEED, xys[:, 1] * W + xys[:, 0], xys[:, 2]))


@pytest.mark.parametrize("name", list(CAMERAS))
def test_panorama_mirrors_in_right(name):
    """param = 2 pi, W = 2 H, un-jittered: pixel x and its mirror W - 1 - x have sx and -sx exactly and the same sy, so
    sin(lon) changes sign and nothing else does: the directions mirror in their `right` component.  Checked in float64
    on the published rays: the components along dir and up agree, the ones along right are opposite."""
    cam = CAMERAS[name].panoramic(TWO_PI)
    W, H = 48, 24
    rays, _ = projection_rays(cam, W, H, SEED, frame_samples(W, H, 0), centre=True)
    d = rays[:, 3:].reshape(H, W, 3).astype(np.float64)
    dirv, up = np.asarray(cam.direction, F32).astype(np.float64), np.asarray(cam.up, F32).astype(np.float64)
    right = np.cross(dirv, up)
    m = d[:, ::-1]
    tol = 4 * 2.0 ** -23  # the basis is orthonormal to look_at's f32 rounding; the rays are f32
    assert np.abs(d @ right + m @ right).max() <= tol
    assert np.abs(d @ dirv - m @ dirv).max() <= tol
    assert np.abs(d @ up - m @ up).max() <= tol
    assert np.abs(d @ right).max() > 0.99  # the frame does look sideways
    assert (d @ dirv).min() < -0.99        # ... and behind


def test_fisheye_centre_and_geometry():
    """Odd W and H: the centre pixel's un-jittered ray is the camera's direction (ang == 0 takes dir itself); the angle
    from the axis of every un-jittered ray is |(sx, sy)| * param / 2."""
    cam = CAMERAS["oblique"].fisheye(math.pi)
    W, H = 37, 21
    rays, _ = projection_rays(cam, W, H, SEED, frame_samples(W, H, 0), centre=True)
    d = rays[:, 3:].reshape(H, W, 3)
    dirv = np.asarray(cam.direction, F32)
    n = dirv * (F32(1.0) / np.sqrt((dirv[0] * dirv[0] + dirv[1] * dirv[1]) + dirv[2] * dirv[2]))
    assert np.array_equal(d[H // 2, W // 2].view(np.uint32), n.view(np.uint32))
    xn = ((2.0 * np.arange(W) + 1.0) - W) / W
    yn = ((2.0 * (H - np.arange(H)) - 1.0) - H) / W
    want = np.hypot(xn[None, :], yn[:, None]) * (math.pi / 2.0)
    got = np.arccos(np.clip(d.astype(np.float64) @ dirv.astype(np.float64), -1.0, 1.0))
    assert np.abs(got - want).max() <= 4e-6  # arccos near the axis magnifies the f32 rounding of the direction


# ------------------------------------------------------------------ the room of tests/test_gpu_projection.py
ROOM_FRAME = (40, 24, 4, 11)  # W, H, spp, seed


def room():
    """The closed stone room of tests/emitter_ref.py (tests/test_gpu_emitters.py), without its emitter."""
    from tests import emitter_ref as E

    sc = E.room_scene(emitter=False)
    sc.build_octree(E.DEPTH)
    return sc


def outside_camera():
    """Outside the room, looking at it."""
    return Camera.look_at((30.0, 22.0, 32.0), (12.0, 8.0, 12.0))


def inside_camera():
    """At the room's eye point, under its ceiling."""
    from tests import emitter_ref as E

    return Camera.look_at(E.ROOM_EYE, (18.0, 6.0, 16.0))


def test_closed_room_reference_rays_all_hit():
    """What tests/test_gpu_projection.py's closed-room render relies on, checked here first: every ray of the float64
    reference for a 2 pi panorama from inside the room meets a wall, by the oracle's closest hit."""
    from oracle import cpu_ref

    W, H, spp, seed = ROOM_FRAME
    sc = room()
    cam = inside_camera().panoramic(TWO_PI)
    for s in range(spp):
        rays, _ = P.projection_rays(cam, W, H, seed, frame_samples(W, H, s))
        assert (cpu_ref.intersect(sc, rays.astype(np.float32))[1] != 0xFFFFFFFF).all()


def c_camera(cam, **over):
    f = dict(fov=cam.fov, aperture=cam.aperture, focal_distance=cam.focal_distance)
    f.update(over)
    return _lib.Camera((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.direction), (C.c_float * 3)(*cam.up),
                       f["fov"], f["aperture"], f["focal_distance"])


def test_refusals_write_nothing():
    lib = _lib.load()
    cam = CAMERAS["oblique"]
    W, H = 8, 8
    xys = frame_samples(W, H, 0)
    rays = np.full((len(xys), 6), 123.25, np.float32)
    state = np.full(len(xys), 0xA5A5A5A5, np.uint32)

    def call(c, p, w=W, h=H, x=xys, flags=0, out=rays, st=state):
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        return lib.octpt_projection_rays(C.byref(c) if c is not None else None, C.byref(p) if p is not None else None,
                                         w, h, SEED, ptr(x), len(x) if x is not None else 4, flags, ptr(out), ptr(st))

    def proj(mode, param, word=None):
        p = _lib.Projection(mode, param)
        if word is not None:
            p.reserved[word] = 1
        return p

    nan, inf = float("nan"), float("inf")
    good = proj(P.FISHEYE, 1.0)
    assert call(c_camera(cam), proj(4, 1.0)) == _lib.ERR_UNSUPPORTED          # an unknown mode
    assert call(c_camera(cam), proj(0xFFFFFFFF, 1.0)) == _lib.ERR_UNSUPPORTED
    for mode in (P.PARALLEL, P.FISHEYE, P.PANORAMIC):
        for param in (0.0, -1.0, nan, inf, -inf):
            assert call(c_camera(cam), proj(mode, param)) == _lib.ERR_INVALID_ARG, (mode, param)
        for word in range(6):
            assert call(c_camera(cam), proj(mode, 1.0, word)) == _lib.ERR_INVALID_ARG
        # an aperture with a projection other than pinhole
        assert call(c_camera(cam, aperture=0.5, focal_distance=3.0), proj(mode, 1.0)) == _lib.ERR_UNSUPPORTED
    above = float(np.nextafter(F32(TWO_PI), F32(10.0)))
    for mode in (P.FISHEYE, P.PANORAMIC):
        assert call(c_camera(cam), proj(mode, above)) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), proj(P.PINHOLE, 0.0, 3)) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam, fov=0.0), good) == _lib.ERR_INVALID_ARG             # octpt_lens_rays' camera rules
    assert call(c_camera(cam, aperture=-1.0), good) == _lib.ERR_INVALID_ARG
    assert call(None, good) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), None) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), good, out=None) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), good, x=None) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), good, w=0) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), good, w=1 << 16, h=1 << 15) == _lib.ERR_INVALID_ARG
    assert call(c_camera(cam), good, flags=2) == _lib.ERR_INVALID_ARG
    for bad_row in ([W, 0, 0], [0, H, 0]):  # a pixel outside the frame, in the last row: nothing before it is written
        x = xys.copy()
        x[-1] = bad_row
        assert call(c_camera(cam), good, x=x) == _lib.ERR_INVALID_ARG
    assert np.all(rays == 123.25) and np.all(state == 0xA5A5A5A5)  # refused calls write nothing
    # the accepted edges: the largest angle, any pinhole param, a NULL state array, an empty batch
    assert call(c_camera(cam), proj(P.PANORAMIC, TWO_PI)) == _lib.OK
    assert call(c_camera(cam), proj(P.PINHOLE, nan)) == _lib.OK
    assert call(c_camera(cam), good, st=None) == _lib.OK
    assert call(c_camera(cam), good, x=xys[:0]) == _lib.OK
    assert C.sizeof(_lib.Projection) == 32 and C.sizeof(_lib.Camera) == 48
    assert lib.octpt_abi_version() == 4  # additive: the ABI version stays


def test_python_camera_helpers():
    cam = Camera.look_at((1.0, 2.0, 3.0), (4.0, 5.0, 6.0))
    assert cam.projection == (_lib.PROJECTION_PINHOLE, 0.0) and Camera().projection == (0, 0.0)
    assert cam.parallel(12.5).projection == (_lib.PROJECTION_PARALLEL, 12.5)
    assert cam.fisheye(3.0).projection == (_lib.PROJECTION_FISHEYE, 3.0)
    assert cam.panoramic(TWO_PI).projection == (_lib.PROJECTION_PANORAMIC, TWO_PI)
    assert cam.projection == (0, 0.0)  # copies
    p = cam.parallel(2.0)
    assert (p.eye, p.direction, p.up, p.fov, p.aperture) == (cam.eye, cam.direction, cam.up, cam.fov, cam.aperture)
    # the positional construction from before the field
    assert Camera((1.0, 2.0, 3.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 0.9, 0.0, 0.0).projection == (0, 0.0)


def test_host_entry_under_sanitizers(tmp_path):
    """octpt_projection_rays in a program of its own with -fsanitize=address,undefined over the cameras, sizes, modes
    and params of this file, into exact-size arrays, the refusals included: clean, and the rays it prints are the bits
    the library returns."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "projection_rays_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    f"-I{os.environ.get('ROCM_PATH', '/opt/rocm')}/include",
                    str(ROOT / "tools" / "projection_rays_host.cpp"),
                    str(ROOT / "octree_pathtracing_amd" / "csrc" / "octpt_host.cpp"), "-o", str(exe)], check=True)
    lines, want = [], []
    for cam in (c.values[0] for c in cases()):
        mode, param = cam.projection
        for (W, H) in SIZES[:2]:
            for centre in (0, 1):
                f = [float(F32(v)).hex() for v in (*cam.eye, *cam.direction, *cam.up, cam.fov, param)]
                lines.append(f"{mode} {W} {H} {SEED} 5 {centre} " + " ".join(f))
                rays, st = projection_rays(cam, W, H, SEED, frame_samples(W, H, 5), centre=bool(centre))
                want.append((rays, st))
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
