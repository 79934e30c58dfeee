"""Guide buffers and denoiser without a GPU: octpt_camera_rays against an f64
statement of Camera::get_ray, the layouts of the two new structs, and the argument checks of the new
entry points that need no device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd.renderer import camera_rays
from octree_pathtracing_amd.scene import Camera

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "octpt.h"

CAMERAS = {
    "default": Camera(),
    "look_at": Camera.look_at((16.0, 20.0, -14.0), (16.0, 16.0, 16.0)),
    # off-axis: an up hint far from the view's normal plane and a narrow field of view
    "off_axis": Camera.look_at((3.5, -7.25, 11.0), (-20.0, 4.0, 2.5), up=(0.3, 1.0, -0.2), fov=0.6),
}
SIZES = [(1, 1), (37, 21), (160, 90)]


def get_ray_f64(cam: Camera, W: int, H: int) -> np.ndarray:
    """Camera::get_ray (camera.rs:77-86) at the pixel centres in f64: (x, y) normalised by max(W, H), y up."""
    eye, d, up = (np.asarray(v, np.float64) for v in (cam.eye, cam.direction, cam.up))
    depth = 1.0 / np.tan(np.float64(cam.fov) / 2.0)
    right = np.cross(d, up)
    dim = float(max(W, H))
    x = ((2.0 * np.arange(W) + 1.0) - W) / dim
    y = ((2.0 * (H - np.arange(H)) - 1.0) - H) / dim
    nd = depth * d + x[None, :, None] * right + y[:, None, None] * up
    nd /= np.linalg.norm(nd, axis=-1, keepdims=True)
    out = np.empty((H, W, 6))
    out[..., :3] = eye
    out[..., 3:] = nd
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(CAMERAS))
def test_camera_rays_match_get_ray(name, size):
    cam = CAMERAS[name]
    W, H = size
    rays = camera_rays(cam, W, H)
    assert rays.shape == (H, W, 6) and rays.dtype == np.float32
    ref = get_ray_f64(cam, W, H)
    assert np.array_equal(rays[..., :3], np.broadcast_to(np.asarray(cam.eye, np.float32), (H, W, 3)))
    d = rays[..., 3:].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() <= 2e-7
    assert np.abs(d - ref[..., 3:]).max() <= 1e-6  # a few f32 roundings on unit-scale values


def test_camera_rays_image_order():
    """Top row first: for the +Z camera (up +Y, right = direction x up = -X) pixel (0, 0) looks up and to
    +X, pixel (W-1, H-1) down and to -X."""
    W, H = 37, 21
    rays = camera_rays(Camera(eye=(0.0, 0.0, 0.0)), W, H)
    first, last = rays[0, 0, 3:], rays[H - 1, W - 1, 3:]
    assert first[0] > 0 and first[1] > 0 and first[2] > 0
    assert last[0] < 0 and last[1] < 0 and last[2] > 0
    # rows step in y only, columns in x only, and the frame is symmetric about its centre
    assert np.all(np.diff(rays[:, 0, 4]) < 0) and np.all(np.diff(rays[0, :, 3]) < 0)
    assert np.array_equal(rays[::-1, ::-1, 3:5], -rays[..., 3:5])


def test_camera_rays_argument_errors():
    lib = _lib.load()
    cam = _lib.Camera((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0, 0, 1), (C.c_float * 3)(0, 1, 0), 1.0, 0.0, 0.0)
    buf = np.zeros(6, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.octpt_camera_rays(C.byref(cam), 1, 1, p) == _lib.OK
    assert lib.octpt_camera_rays(None, 1, 1, p) == _lib.ERR_INVALID_ARG
    assert lib.octpt_camera_rays(C.byref(cam), 1, 1, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_camera_rays(C.byref(cam), 0, 1, p) == _lib.ERR_INVALID_ARG
    assert lib.octpt_camera_rays(C.byref(cam), 1, 0, p) == _lib.ERR_INVALID_ARG
    assert lib.octpt_camera_rays(C.byref(cam), 1 << 16, 1 << 15, p) == _lib.ERR_INVALID_ARG  # 2^31 pixels
    bad = _lib.Camera((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0, 0, 1), (C.c_float * 3)(0, 1, 0), 0.0, 0.0, 0.0)
    assert lib.octpt_camera_rays(C.byref(bad), 1, 1, p) == _lib.ERR_INVALID_ARG  # fov outside (0, pi)
    assert np.all(buf[3:] == np.float32([0, 0, 1]))  # the failed calls wrote nothing


NEW_STRUCTS = {"octpt_aov_buffers": "AovBuffers", "octpt_denoise_params": "DenoiseParams"}


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
            assert C.alignment(mirror) <= int(align)
        seen += 1
    assert seen == 2 + 5 + 7
    assert tuple(f for f, _ in _lib.AovBuffers._fields_) == _lib.AOV_NAMES


def test_null_context_calls_fail_cleanly():
    lib = _lib.load()
    p = _lib.RenderParams(8, 8, 0, 1, 5, 1, 1, 0, 1, 0)
    b = _lib.AovBuffers()
    d = _lib.DenoiseParams(8, 8, 1, 1.0, 1.0, 1.0, 0)
    assert lib.octpt_render_aov(None, C.byref(p), C.byref(b)) == _lib.ERR_INVALID_ARG
    assert lib.octpt_render_aov(None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_render_aov_device(None, C.byref(p), C.byref(b), None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_render_aov_device(None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_denoise(None, C.byref(d), None, C.byref(b), None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_denoise(None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_denoise_device(None, C.byref(d), None, C.byref(b), None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_denoise_device(None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
