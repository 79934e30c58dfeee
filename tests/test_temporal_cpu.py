"""Temporal reprojection without a GPU: octpt_reproject_coords against the f32 numpy
restatement of the mapping (tests/temporal_ref.py) bit for bit, the identity under an unmoved camera, the
refusals that need no device, and the layouts of the two new structs."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd.renderer import reproject_coords
from octree_pathtracing_amd.scene import Camera
from tests.temporal_ref import coords_ref, reproject_ref

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "octpt.h"
F32 = np.float32

EYE, CENTER = (16.0, 20.0, -14.0), (16.0, 16.0, 16.0)
BASE = Camera.look_at(EYE, CENTER)


def yawed(angle, eye=EYE):
    """BASE turned by `angle` radians about the world's Y axis, from `eye`."""
    v = np.subtract(CENTER, EYE)
    c, s = np.cos(angle), np.sin(angle)
    w = (c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2])
    return Camera.look_at(eye, tuple(np.add(eye, w)))


# (current, previous)
PAIRS = {
    "identical": (BASE, BASE),
    "translated": (Camera.look_at((16.7, 19.7, -13.5), (16.7, 15.7, 16.5)), BASE),
    "yawed": (yawed(0.05), BASE),
    # the previous camera a quarter turn away: part of the frame lies behind it (zc <= 0)
    "looking_away": (BASE, yawed(np.pi / 2)),
}


def depths(W, H, seed=7):
    """Random in [1, 1000], about one in eight +inf."""
    rng = np.random.default_rng(seed + W * 31 + H)
    d = rng.uniform(1.0, 1000.0, (H, W)).astype(F32)
    d[rng.random((H, W)) < 0.125] = np.inf
    if W * H == 1:
        d[...] = 10.0
    return d


def same_bits(a, b):
    """Equal as uint32 views, NaNs compared as NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


@pytest.mark.parametrize("size", [(64, 64), (37, 21), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", list(PAIRS))
def test_coords_match_restatement_bit_for_bit(pair, size):
    cam, prev = PAIRS[pair]
    W, H = size
    d = depths(W, H)
    xy, zp = reproject_coords(cam, prev, W, H, d)
    ref_xy, ref_zp = coords_ref(cam, prev, W, H, d)
    assert xy.shape == (H, W, 2) and zp.shape == (H, W) and xy.dtype == zp.dtype == F32
    assert same_bits(xy, ref_xy), int((xy.view(np.uint32) != ref_xy.view(np.uint32)).sum())
    assert same_bits(zp, ref_zp)
    miss = ~np.isfinite(d)
    assert np.all(np.isnan(xy[miss])) and np.all(zp[miss] == np.inf)
    if pair == "looking_away" and W > 1:  # zc <= 0 occurs, and so does zc > 0
        behind = np.isnan(xy[..., 0]) & ~miss
        assert behind.any() and (~np.isnan(xy[..., 0])).any()
        assert np.all(zp[behind] == np.inf) and np.all(np.isnan(xy[behind]))
    elif pair != "looking_away":
        assert not np.isnan(xy[~miss]).any()


@pytest.mark.parametrize("size", [(64, 64), (37, 21), (1920, 1080)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_under_an_unmoved_camera(size):
    """Steps 7 and 8 invert C24's xn, yn: with identical cameras every finite pixel maps onto itself, first on
    the restatement, then on the library; zp is the depth again to a few roundings."""
    W, H = size
    d = depths(W, H)
    hit = np.isfinite(d)
    X, Y = np.meshgrid(np.arange(W), np.arange(H))
    fx, fy, zp, valid = reproject_ref(BASE, BASE, W, H, d)
    assert np.array_equal(valid, hit)
    assert np.array_equal(np.rint(fx[hit]), X[hit]) and np.array_equal(np.rint(fy[hit]), Y[hit])
    xy, lzp = reproject_coords(BASE, BASE, W, H, d)
    assert np.array_equal(np.rint(xy[..., 0][hit]), X[hit]) and np.array_equal(np.rint(xy[..., 1][hit]), Y[hit])
    assert np.abs(xy[..., 0][hit] - X[hit]).max() < 0.05 and np.abs(xy[..., 1][hit] - Y[hit]).max() < 0.05
    # P = eye + d z rounds at |P| < 32 + z, half an ulp (2^-24 relative) per component, and v = P - eye and the
    # norm add a few more: 1e-5 of z bounds them from z = 1 up
    assert np.all(np.abs(lzp[hit] - d[hit]) <= 1e-5 * d[hit])


def c_camera(cam, **over):
    f = dict(eye=cam.eye, direction=cam.direction, up=cam.up, fov=cam.fov, aperture=0.0)
    f.update(over)
    return _lib.Camera((C.c_float * 3)(*f["eye"]), (C.c_float * 3)(*f["direction"]), (C.c_float * 3)(*f["up"]),
                       f["fov"], f["aperture"], 0.0)


def test_reproject_coords_refusals():
    lib = _lib.load()
    d = np.full(4, 5.0, F32)
    xy = np.full(8, 7.0, F32)
    zp = np.full(4, 7.0, F32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cam = c_camera(BASE)

    def call(cur=cam, prev=cam, W=2, H=2, depth=d, out_xy=xy, out_zp=zp):
        return lib.octpt_reproject_coords(C.byref(cur) if cur else None, C.byref(prev) if prev else None, W, H,
                                          P(depth) if depth is not None else None,
                                          P(out_xy) if out_xy is not None else None,
                                          P(out_zp) if out_zp is not None else None)

    # NULL required pointers, a zero size, 2^31 pixels
    for kw in (dict(cur=None), dict(prev=None), dict(depth=None), dict(out_xy=None), dict(out_zp=None), dict(W=0),
               dict(H=0), dict(W=1 << 16, H=1 << 15)):
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    # octpt_set_camera's rules, for either camera
    for which in ("cur", "prev"):
        assert call(**{which: c_camera(BASE, fov=0.0)}) == _lib.ERR_INVALID_ARG
        assert call(**{which: c_camera(BASE, fov=3.2)}) == _lib.ERR_INVALID_ARG
        assert call(**{which: c_camera(BASE, fov=float("nan"))}) == _lib.ERR_INVALID_ARG
        assert call(**{which: c_camera(BASE, aperture=0.1)}) == _lib.ERR_UNSUPPORTED
    # the previous camera is the one inverted: it must be orthonormal to 1e-4
    dirn, up = np.asarray(BASE.direction), np.asarray(BASE.up)
    bad = [dict(direction=tuple(dirn * 1.001)), dict(up=tuple(up * 0.999)), dict(up=tuple(up + 0.001 * dirn)),
           dict(direction=(0.0, 0.0, 0.0)), dict(up=(float("nan"), 0.0, 0.0))]
    for over in bad:
        assert call(prev=c_camera(BASE, **over)) == _lib.ERR_INVALID_ARG, over
    assert np.all(xy == 7.0) and np.all(zp == 7.0)  # the refused calls wrote nothing
    # within the bound it is accepted, and the current camera is not held to it
    assert call(prev=c_camera(BASE, direction=tuple(dirn * 1.00001))) == _lib.OK
    assert call(cur=c_camera(BASE, direction=tuple(dirn * 1.001))) == _lib.OK
    assert not np.any(xy == 7.0)


def test_null_context_calls_fail_cleanly():
    lib = _lib.load()
    cam = c_camera(BASE)
    p = _lib.TemporalParams(8, 8, cam, cam, 32, 0.1, 0.9, 0)
    g, h = _lib.AovBuffers(), _lib.TemporalHistory()
    assert lib.octpt_temporal(None, C.byref(p), None, C.byref(g), C.byref(h), None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_temporal(None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_temporal_device(None, C.byref(p), None, C.byref(g), None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_temporal_device(None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG


NEW_STRUCTS = {"octpt_temporal_params": "TemporalParams", "octpt_temporal_history": "TemporalHistory"}


def test_new_struct_layouts_match_gcc(tmp_path):
    probe = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for c_name, mirror in NEW_STRUCTS.items():
        lines.append(f'    printf("{c_name} %zu %zu\\n", sizeof({c_name}), _Alignof({c_name}));')
        for field, _ in getattr(_lib, mirror)._fields_:
            lines.append(f'    printf("{c_name}.{field} %zu 0\\n", offsetof({c_name}, {field}));')
    lines.append("    return 0;\n}")
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        name, size, align = line.split()
        if "." in name:
            c_name, field = name.split(".")
            assert getattr(getattr(_lib, NEW_STRUCTS[c_name]), field).offset == int(size), name
        else:
            mirror = getattr(_lib, NEW_STRUCTS[name])
            assert C.sizeof(mirror) == int(size), (name, C.sizeof(mirror), size)
            assert C.alignment(mirror) == int(align)
        seen += 1
    assert seen == 2 + 8 + 5
    assert tuple(f for f, _ in _lib.TemporalHistory._fields_) == _lib.HISTORY_NAMES
