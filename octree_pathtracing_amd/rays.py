"""Ray lists for HipRenderer.set_ray_source: a camera is a few lines of numpy.

A list is a float32 array of shape (H, W, R, 6): for each pixel R records of (origin xyz, unit direction xyz); sample
s of a pixel takes record s % R.  One worked camera follows; a cube-map face, a distorted lens or a light probe is
written the same way: compute origins and unit directions per pixel, stack them, hand them to the renderer.
"""
from __future__ import annotations

import numpy as np

from .scene import Camera

PROJECTION_PANORAMIC = 3  # _lib.PROJECTION_PANORAMIC


def pixel_positions(width: int, height: int):
    """(sx, sy) of the pixel centres, each [H, W] float64: the image position every camera of the renderer starts
    from, in units of half the longer image side, y up."""
    dim = float(max(width, height))
    xs = (2.0 * np.arange(width) + 1.0 - width) / dim
    ys = (2.0 * (height - np.arange(height)) - 1.0 - height) / dim
    return np.broadcast_to(xs[None, :], (height, width)), np.broadcast_to(ys[:, None], (height, width))


def stereo_panorama_rays(camera: Camera, width: int, height: int, ipd: float, eye) -> np.ndarray:
    """Omnidirectional stereo (ODS), one ray per pixel: (H, W, 1, 6) float32.

    The direction is the panoramic projection's (C40) at the pixel centre: longitude sx * angle / 2 about the camera's
    up, latitude sy * angle / 2, with angle the camera's panoramic angle (camera.panoramic(a)), else 2 pi -- the full
    360 x 180 degree panorama at width = 2 * height.  The origin leaves the camera's eye by ipd / 2 along the horizontal
    tangent of the viewing circle at that longitude: towards growing longitude for the right eye (eye = +1 or
    "right"), the other way for the left (eye = -1 or "left").  Every ray is thus tangent to a circle of diameter ipd
    about the eye point, which is what makes the two panoramas a stereo pair in every viewing direction; ipd = 0 is
    the plain panorama.  The camera's direction and up are taken as orthonormal, as the renderer takes them."""
    sign = {"left": -1.0, "right": 1.0}.get(eye, eye)
    if sign not in (-1, 1, -1.0, 1.0):
        raise ValueError(f"eye must be -1 / 'left' or +1 / 'right', not {eye!r}")
    mode, param = camera.projection
    angle = float(np.float32(param if int(mode) == PROJECTION_PANORAMIC else 2.0 * np.pi))  # as the library takes it
    fwd = np.asarray(camera.direction, np.float64)
    up = np.asarray(camera.up, np.float64)
    right = np.cross(fwd, up)  # camera.rs:80
    sx, sy = pixel_positions(width, height)
    lon, lat = sx * (angle / 2.0), sy * (angle / 2.0)
    cl, sl, co, so = np.cos(lat), np.sin(lat), np.cos(lon), np.sin(lon)
    d = (cl * co)[..., None] * fwd + (cl * so)[..., None] * right + sl[..., None] * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    tangent = co[..., None] * right - so[..., None] * fwd  # d(direction) / d(longitude) on the horizon
    o = np.asarray(camera.eye, np.float64) + (float(sign) * float(ipd) / 2.0) * tangent
    return np.concatenate([o, d], -1).astype(np.float32)[:, :, None, :]
