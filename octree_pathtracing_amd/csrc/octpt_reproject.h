// The reprojection mapping of DESIGN.md C26, stated once for the device (temporal_kernel) and the host
// (octpt_reproject_coords): where the surface point a pixel of the current frame sees lay in the previous
// camera's frame.  Plain f32, glam's dot-product order, correctly rounded division and sqrtf; both sides
// compile this text with contraction off, which is what makes the host mirror bit-identical.
#pragma once
#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "../../include/octpt.h"

#if defined(__HIP__)
#define OCTPT_HD __host__ __device__
#else
#define OCTPT_HD
#endif

namespace octpt {

// a camera with its derived basis, as octpt_set_camera derives it (DevCamera has these fields)
struct CameraBasis {
    float eye[3], dir[3], right[3], up[3];
    float d_factor;  // 1 / tan(fov / 2)  (camera.rs:79)
};

// host: the basis octpt_set_camera derives (right = direction x up, camera.rs:80; d_factor, camera.rs:79)
inline CameraBasis camera_basis(const float eye[3], const float dir[3], const float up[3], float fov) {
    CameraBasis B;
    for (int i = 0; i < 3; ++i) {
        B.eye[i] = eye[i];
        B.dir[i] = dir[i];
        B.up[i] = up[i];
    }
    B.right[0] = dir[1] * up[2] - up[1] * dir[2];
    B.right[1] = dir[2] * up[0] - up[2] * dir[0];
    B.right[2] = dir[0] * up[1] - up[0] * dir[1];
    B.d_factor = 1.0f / tanf(fov / 2.0f);
    return B;
}

// host: what the inversion asks of the previous camera (C26)
inline bool camera_orthonormal(const float dir[3], const float up[3]) {
    const float dd = (dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2];
    const float uu = (up[0] * up[0] + up[1] * up[1]) + up[2] * up[2];
    const float du = (dir[0] * up[0] + dir[1] * up[1]) + dir[2] * up[2];
    return fabsf(dd - 1.0f) <= 1e-4f && fabsf(uu - 1.0f) <= 1e-4f && fabsf(du) <= 1e-4f;  // false on NaN
}

// host: octpt_set_camera's rules for both cameras of a reprojection, orthonormality for the inverted one.
// OCTPT_OK, or the status with *why set
inline octpt_status check_reproject_cameras(const octpt_camera *cur, const octpt_camera *prev, const char **why) {
    for (const octpt_camera *c : {cur, prev}) {
        if (!(c->fov > 0.0f && c->fov < 3.14159265f)) {
            *why = "fov must be in (0, pi)";
            return OCTPT_ERR_INVALID_ARG;
        }
        if (c->aperture != 0.0f) {
            *why = "thin-lens aperture is not used by the reference path";
            return OCTPT_ERR_UNSUPPORTED;
        }
    }
    if (!camera_orthonormal(prev->direction, prev->up)) {
        *why = "the previous camera must be orthonormal (direction and up of unit length and perpendicular, to 1e-4)";
        return OCTPT_ERR_INVALID_ARG;
    }
    return OCTPT_OK;
}

OCTPT_HD inline float rp_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Pixel (x, y) of the current W x H frame at depth z (finite) -> (fx, fy), its position in the previous frame in
// pixel units (pixel centre x <-> fx = x), and zp, the depth the previous frame would have stored for the point.
// false (outputs untouched) when the point is not in front of the previous camera: !(zc > 0).
template <class Cam, class PrevCam>
OCTPT_HD inline bool reproject_pixel(const Cam &cur, const PrevCam &prev, uint32_t x, uint32_t y, uint32_t W, uint32_t H,
                                     float dim, float z, float &fx, float &fy, float &zp) {
    // 1. C24's camera ray of the current camera (Camera::get_ray at the pixel centre, camera.rs:77-86)
    const float xc = ((float)(2u * x + 1u) - (float)W) / dim;
    const float yc = ((float)(2u * (H - y) - 1u) - (float)H) / dim;
    float nd[3];
    for (int i = 0; i < 3; ++i) nd[i] = (cur.dir[i] * cur.d_factor + cur.right[i] * xc) + cur.up[i] * yc;
    const float r = 1.0f / sqrtf(rp_dot(nd, nd));
    float v[3];
    for (int i = 0; i < 3; ++i) {
        const float P = cur.eye[i] + (nd[i] * r) * z;  // 2. the point the pixel sees
        v[i] = P - prev.eye[i];                        // 3.
    }
    const float zc = rp_dot(v, prev.dir);  // 4.
    if (!(zc > 0.0f)) return false;
    const float s = prev.d_factor / zc;  // 5.
    const float xn = rp_dot(v, prev.right) * s, yn = rp_dot(v, prev.up) * s;  // 6.
    fx = ((xn * dim + (float)W) - 1.0f) * 0.5f;                           // 7. C24's xn, yn inverted
    fy = (((float)H - 1.0f) - yn * dim) * 0.5f;                           // 8.
    zp = sqrtf(rp_dot(v, v));                                               // 9.
    return true;
}

}  // namespace octpt
