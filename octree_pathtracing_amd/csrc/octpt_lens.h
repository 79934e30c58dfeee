// The camera ray of a path, DESIGN.md C37, stated once for the device (new_path: the seed kernel, shade's path
// regeneration, the megakernel) and the host (octpt_lens_rays): the jittered pinhole ray of camera.rs:77-86 and
// tile_renderer.rs:695-703, and with an aperture the thin-lens ray through the same point of the focal plane.
// With it what the expression needs: the counter-based RNG and the portable f32 sincos
// (§3.11), which the kernels use everywhere else from here too.  Plain f32, glam's dot-product order, correctly
// rounded division and sqrtf; both sides compile this text with contraction off, which is what makes the host
// mirror bit-identical.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIP__)
#define OCTPT_LENS_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define OCTPT_LENS_FN inline
#endif

namespace octpt {

// ---------------------------------------------------------------------------
// portable f32 math -- identical constants and order to the oracle
// ---------------------------------------------------------------------------
OCTPT_LENS_FN void dm_sincos(float x, float &s, float &c) {
    const float kf = floorf(x * 0.636619772367581343f + 0.5f);
    const int k = (int)kf;
    const float r = ((x - kf * 1.5703125f) - kf * 4.837512969970703125e-4f) - kf * 7.54978995489188216e-8f;
    const float z = r * r;
    const float sp = r + r * z * (-1.6666654611e-1f + z * (8.3321608736e-3f + z * -1.9515295891e-4f));
    const float cp = (1.0f - 0.5f * z) +
                     z * z * (4.166664568298827e-2f + z * (-1.388731625493765e-3f + z * 2.443315711809948e-5f));
    switch (k & 3) {
    case 0: s = sp; c = cp; break;
    case 1: s = cp; c = -sp; break;
    case 2: s = -sp; c = -cp; break;
    default: s = -cp; c = sp; break;
    }
}

// ---------------------------------------------------------------------------
// counter-based RNG
// ---------------------------------------------------------------------------
OCTPT_LENS_FN uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
OCTPT_LENS_FN uint32_t path_state(uint32_t seed, uint32_t pixel, uint32_t sample) {
    uint32_t h = lowbias32(seed ^ 0xA511E9B3u);
    h = lowbias32(h ^ pixel);
    return lowbias32(h ^ (sample * 0x9E3779B9u));
}
OCTPT_LENS_FN float rng_next(uint32_t &st) {
    const uint32_t s = st * 747796405u + 2891336453u;
    st = s;
    uint32_t w = ((s >> ((s >> 28u) + 4u)) ^ s) * 277803737u;
    w = (w >> 22u) ^ w;
    return (float)(w >> 8) * (1.0f / 16777216.0f);
}

// the lens stream of a path (C37): lowbias32(path_state ^ kLensStream), a stream of its own, so that the path's
// stream is draw for draw what it is without a lens
constexpr uint32_t kLensStream = 0x4C454E53u;

// what lens_ray reads of a frame (DevRender has these fields)
struct LensFrame {
    uint32_t W, H, seed;
    float dim, jlo, jhi;  // max(W, H), -1 / dim, 1 / dim
};
// ... and of a camera (DevCamera has these fields)
struct LensCamera {
    float eye[3], dir[3], right[3], up[3];
    float d_factor;     // 1 / tan(fov / 2)  (camera.rs:79)
    float aperture;     // lens radius; 0 = pinhole
    float focal_scale;  // focal_distance / d_factor, divided once on the host
};
// host: LensCamera as octpt_set_camera derives DevCamera (right = direction x up, camera.rs:80)
inline LensCamera lens_camera(const float eye[3], const float dir[3], const float up[3], float fov, float aperture,
                              float focal_distance) {
    LensCamera L;
    for (int i = 0; i < 3; ++i) {
        L.eye[i] = eye[i];
        L.dir[i] = dir[i];
        L.up[i] = up[i];
    }
    L.right[0] = dir[1] * up[2] - up[1] * dir[2];
    L.right[1] = dir[2] * up[0] - up[2] * dir[0];
    L.right[2] = dir[0] * up[1] - up[0] * dir[1];
    L.d_factor = 1.0f / tanf(fov / 2.0f);
    L.aperture = aperture;
    L.focal_scale = aperture > 0.0f ? focal_distance / L.d_factor : 0.0f;  // aperture 0: focal_distance is not read
    return L;
}
// host: octpt_set_camera's rule for the two lens fields (false on NaN)
inline bool lens_fields_valid(float aperture, float focal_distance) {
    if (!(aperture >= 0.0f && aperture < INFINITY)) return false;
    return aperture == 0.0f || (focal_distance > 0.0f && focal_distance < INFINITY);
}

// The first ray (o, d) of sample `sample` of pixel (x, y); returns the path's RNG state after it (the two jitter
// draws; the same state whatever kLens).  kLens false: the pinhole ray, aperture and focal_scale are not read.
template <bool kLens, class Cam, class Frame>
OCTPT_LENS_FN uint32_t lens_ray(const Cam &C, const Frame &R, uint32_t x, uint32_t y, uint32_t sample, float o[3],
                                float d[3]) {
    const uint32_t st0 = path_state(R.seed, y * R.W + x, sample);
    uint32_t st = st0;
    const float jlo = R.jlo, jhi = R.jhi;  // -1 / dim, 1 / dim
    const float xn = ((float)(2u * x + 1u) - (float)R.W) / R.dim;
    const float yn = ((float)(2u * (R.H - y) - 1u) - (float)R.H) / R.dim;
    const float dx = jlo + (jhi - jlo) * rng_next(st);
    const float dy = jlo + (jhi - jlo) * rng_next(st);
    const float sx = xn + dx, sy = yn + dy;
    float nd[3];
    for (int i = 0; i < 3; ++i) nd[i] = (C.dir[i] * C.d_factor + C.right[i] * sx) + C.up[i] * sy;
    float t[3];
    if (kLens) {
        uint32_t ls = lowbias32(st0 ^ kLensStream);
        const float u1 = rng_next(ls), u2 = rng_next(ls);
        const float r = C.aperture * sqrtf(u1);  // uniform over the disc of radius aperture
        const float phi = (2.0f * 3.14159265358979323846f) * u2;
        float sn, cs;
        dm_sincos(phi, sn, cs);
        const float a = r * cs, b = r * sn;
        for (int i = 0; i < 3; ++i) {
            const float l = C.right[i] * a + C.up[i] * b;  // the point of the lens, relative to the eye
            const float f = nd[i] * C.focal_scale;         // the pinhole ray's point of the focal plane, likewise
            o[i] = C.eye[i] + l;
            t[i] = f - l;
        }
    } else {
        for (int i = 0; i < 3; ++i) {
            o[i] = C.eye[i];
            t[i] = nd[i];
        }
    }
    const float rn = 1.0f / sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    for (int i = 0; i < 3; ++i) d[i] = t[i] * rn;
    return st;
}

// ---------------------------------------------------------------------------
// camera projections: the parallel, fisheye and panoramic first ray
// ---------------------------------------------------------------------------
// octpt_projection::mode (include/octpt.h has the same values); pinhole is lens_ray above, untouched
constexpr uint32_t kProjPinhole = 0u, kProjParallel = 1u, kProjFisheye = 2u, kProjPanoramic = 3u;
constexpr float kProjTwoPi = 6.28318530717958647692f;  // rounds to the f32 above 2 pi: the largest angle accepted

// what projection_ray reads of a camera beside its basis (DevCamera has these fields too)
struct ProjCamera {
    float eye[3], dir[3], right[3], up[3];
    uint32_t proj_mode;  // kProj*, not kProjPinhole
    float proj_half;     // param * 0.5f, multiplied once on the host: half the extent, or half the angle
};
// host: octpt_set_projection's rule for mode and param (kProjPinhole reads no param); false on NaN
inline bool proj_mode_known(uint32_t mode) { return mode <= kProjPanoramic; }
inline bool proj_param_valid(uint32_t mode, float param) {
    if (mode == kProjPinhole) return true;
    if (!(param > 0.0f && param < INFINITY)) return false;
    return mode == kProjParallel || param <= kProjTwoPi;
}

// The first ray of a non-pinhole projection.  The common part -- st0, xn, yn, the two jitter draws, sx, sy, the
// returned state, the final normalisation -- is lens_ray's, so a path's later draws do not depend on the projection.
// kJitter false: the un-jittered ray of the preview and the guide buffers, dx = dy = 0 (no draw; returns st0).
// dm_sincos takes lon, lat in [-pi, pi] and fisheye angles up to pi * sqrt(2) as they are: its three-part pi/2
// reduction is exact for |k| <= 3 quadrants and `k & 3` is the quadrant of a negative k too (C40 has the figures).
template <bool kJitter, class Cam, class Frame>
OCTPT_LENS_FN uint32_t projection_ray(const Cam &C, const Frame &R, uint32_t x, uint32_t y, uint32_t sample,
                                      float o[3], float d[3]) {
    const uint32_t st0 = path_state(R.seed, y * R.W + x, sample);
    uint32_t st = st0;
    const float jlo = R.jlo, jhi = R.jhi;  // -1 / dim, 1 / dim
    const float xn = ((float)(2u * x + 1u) - (float)R.W) / R.dim;
    const float yn = ((float)(2u * (R.H - y) - 1u) - (float)R.H) / R.dim;
    float dx = 0.0f, dy = 0.0f;
    if (kJitter) {
        dx = jlo + (jhi - jlo) * rng_next(st);
        dy = jlo + (jhi - jlo) * rng_next(st);
    }
    const float sx = xn + dx, sy = yn + dy;
    const float hf = C.proj_half;
    float t[3];
    if (C.proj_mode == kProjParallel) {
        const float a = sx * hf, b = sy * hf;
        for (int i = 0; i < 3; ++i) {
            o[i] = (C.eye[i] + C.right[i] * a) + C.up[i] * b;
            t[i] = C.dir[i];
        }
    } else if (C.proj_mode == kProjFisheye) {  // equidistant: the angle from the axis grows with the image radius
        const float ax = sx * hf, ay = sy * hf;
        const float ang = sqrtf(ax * ax + ay * ay);
        float cs = 1.0f, ka = 0.0f, kb = 0.0f;
        if (ang != 0.0f) {
            float sn;
            dm_sincos(ang, sn, cs);
            const float k = sn / ang;
            ka = ax * k;
            kb = ay * k;
        }
        for (int i = 0; i < 3; ++i) {
            o[i] = C.eye[i];
            t[i] = ang != 0.0f ? (C.dir[i] * cs + C.right[i] * ka) + C.up[i] * kb : C.dir[i];
        }
    } else {  // kProjPanoramic, equirectangular: sx is the longitude, sy the latitude
        const float lon = sx * hf, lat = sy * hf;
        float sl, cl, so, co;
        dm_sincos(lat, sl, cl);
        dm_sincos(lon, so, co);
        const float a = cl * co, b = cl * so;
        for (int i = 0; i < 3; ++i) {
            o[i] = C.eye[i];
            t[i] = (C.dir[i] * a + C.right[i] * b) + C.up[i] * sl;
        }
    }
    const float rn = 1.0f / sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    for (int i = 0; i < 3; ++i) d[i] = t[i] * rn;
    return st;
}

// ---------------------------------------------------------------------------
// the ray-list camera: the first ray of every sample read from a buffer the caller fills
// ---------------------------------------------------------------------------
constexpr uint64_t kRayListMaxRays = 1ull << 28;  // width * height * rays_per_pixel at most (octpt_set_ray_source)
constexpr float kRayListUnitBand = 1e-4f;         // a direction's squared length lies within this of 1

// where the ray of sample `sample` of pixel (x, y) starts in the list, in floats: 64-bit, R records per pixel in
// image order, the samples beyond R wrapping round (sample is absolute, spp_start included)
OCTPT_LENS_FN uint64_t ray_list_index(uint32_t W, uint32_t x, uint32_t y, uint32_t rpp, uint32_t sample) {
    return 6ull * ((uint64_t)(y * W + x) * rpp + sample % rpp);
}

// The first ray of a ray-list camera: the six floats of the list as given (origin, direction; not renormalised).  An
// invalid record -- a non-finite float, or a direction whose squared length is not within kRayListUnitBand of 1: the
// negated <= is true for NaN, zero and infinite directions as well -- is replaced whole by the camera's central ray
// (eye, dir), so that no bit pattern in the buffer makes anything but an ordinary path.  st0 and the two jitter draws
// are lens_ray's (drawn and discarded): the returned state is lens_ray's, so a path's later draws are what they are
// under every other camera.  kJitter false: ray 0 of the pixel for the preview and the guide buffers (no draw; st0).
template <bool kJitter, class Cam, class Frame>
OCTPT_LENS_FN uint32_t ray_list_ray(const Cam &C, const Frame &R, const float *rays, uint32_t rpp, uint32_t x, uint32_t y,
                                    uint32_t sample, float o[3], float d[3]) {
    const uint32_t st0 = path_state(R.seed, y * R.W + x, sample);
    uint32_t st = st0;
    if (kJitter) {
        (void)rng_next(st);
        (void)rng_next(st);
    }
    const float *r = rays + ray_list_index(R.W, x, y, rpp, kJitter ? sample : 0u);
    float v[6];
    for (int i = 0; i < 6; ++i) v[i] = r[i];
    const float len2 = (v[3] * v[3] + v[4] * v[4]) + v[5] * v[5];  // (a non-finite direction makes this inf or NaN)
    bool bad = !(fabsf(len2 - 1.0f) <= kRayListUnitBand);
    for (int i = 0; i < 3; ++i) bad = bad || !(fabsf(v[i]) < INFINITY);
    for (int i = 0; i < 3; ++i) {
        o[i] = bad ? C.eye[i] : v[i];
        d[i] = bad ? C.dir[i] : v[3 + i];
    }
    return st;
}

}  // namespace octpt
