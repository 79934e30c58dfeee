// The sky, DESIGN.md C42, stated once for the device (the sky instances of shade, the drain and the preview, and the
// kernel behind octpt_sky_radiance_device) and the host (octpt_sky_radiance): the base colour a ray that leaves the
// world adds before the sun's terms.  Plain f32; both sides compile this text with contraction off, which is what
// makes the host form bit-identical to the device's.
//
// sky_radiance(K, d, out) for a unit direction d in world axes, +y up:
//   DEFAULT   (0.5, 0.7, 1.0), Scene::SKY_COLOR: the state of a new context
//   COLOR     color * scale
//   GRADIENT  (horizon + (zenith - horizon) * max(d.y, 0)) * scale; below the horizon that is horizon * scale
//   MAP       an equirectangular map of W x H texels of four floats (RGBA, 16 bytes: one tap is one 16-byte load),
//             row 0 the zenith:
//               lon = dm_atan2(d.z, d.x) + yaw        u = lon / 2pi + 0.5, wrapped into [0, 1)
//               v   = dm_acos(clamp(d.y, -1, 1)) / pi
//               fx  = u * W - 0.5                      fy = v * H - 0.5
//             taps at floor and floor + 1, wrapped in x and clamped in y; every lerp is a + w * (b - a), x first, then
//             y, then times scale: a map of equal texels returns exactly that texel times scale.
//             At the poles (d.x = d.z = 0, either sign of zero) dm_atan2 gives 0, so lon = yaw: the value is the top
//             (d.y = 1) or bottom (d.y = -1) row's x-lerp at the column of u = yaw / 2pi + 0.5.  Both y taps are that
//             row (fy = -0.5 or H - 0.5 clamps to it), so directions approaching a pole along any meridian approach
//             that row's value at their own longitude.
// Texels are sanitised when a map is set (sky_sanitise: NaN and negative to 0, +inf to FLT_MAX) and a MAP result is
// held at FLT_MAX after the scale, so no bit pattern in a map makes a non-finite lookup.  A direction with a NaN
// component (no path has one: begin_segment replaces it) takes u = 0 and, for a NaN d.y, fy = -0.5 -- the seam's blend of
// columns W - 1 and 0, in the top row then: every index is formed from compared floats, in bounds whatever d holds.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "octpt_math.h"

#if defined(__HIP__)
#define OCTPT_SKY_FN __host__ __device__ inline
#else
#define OCTPT_SKY_FN inline
#endif

namespace octpt {

// octpt_sky::mode (include/octpt.h has the same values)
constexpr uint32_t kSkyDefault = 0u, kSkyColor = 1u, kSkyGradient = 2u, kSkyMap = 3u;
constexpr uint64_t kSkyMaxTexels = 1ull << 26;  // width * height at most (1 GiB of texels)

// the sky as the kernels and the host form take it
struct Sky {
    uint32_t mode, width, height, pad0;
    float color[3], horizon[3], zenith[3];
    float scale, yaw, pad1;
    const float *texels;  // MAP: width * height * 4 floats, 16-byte aligned on the device
};

// what octpt_set_sky makes of one float of a map
OCTPT_SKY_FN float sky_sanitise(float t) {
    if (!(t > 0.0f)) return 0.0f;  // NaN, negative, either zero
    return t < FLT_MAX ? t : FLT_MAX;
}

// octpt_set_sky's rule for the record (false on NaN): every field the mode reads
inline bool sky_mode_known(uint32_t mode) { return mode <= kSkyMap; }
inline bool sky_fields_valid(uint32_t mode, float scale, float yaw, uint32_t width, uint32_t height, bool texels) {
    if (mode == kSkyDefault) return true;
    if (!(scale >= 0.0f && scale < INFINITY)) return false;
    if (!(fabsf(yaw) < INFINITY)) return false;
    if (mode != kSkyMap) return true;
    return texels && width != 0u && height != 0u && (uint64_t)width * height <= kSkyMaxTexels;
}

// one tap: RGB of texel (x, y)
OCTPT_SKY_FN void sky_texel(const Sky &K, uint32_t x, uint32_t y, float t[3]) {
    const size_t i = (size_t)y * K.width + x;
#if defined(__HIP_DEVICE_COMPILE__)
    struct alignas(16) Texel { float r, g, b, a; };  // one 16-byte load
    const Texel v = reinterpret_cast<const Texel *>(K.texels)[i];
    t[0] = v.r; t[1] = v.g; t[2] = v.b;
#else
    t[0] = K.texels[4u * i]; t[1] = K.texels[4u * i + 1u]; t[2] = K.texels[4u * i + 2u];
#endif
}

// the map's lookup position of a direction, in texels (what the CPU test measures against float64)
OCTPT_SKY_FN void sky_map_position(const Sky &K, const float d[3], float &fx, float &fy) {
    const float lon = dm_atan2(d[2], d[0]) + K.yaw;
    float u = lon / 6.28318530717958647692f + 0.5f;
    u = u - floorf(u);
    if (!(u < 1.0f)) u = 0.0f;  // a tiny negative u wraps to the float 1; NaN
    const float dy = d[1] < -1.0f ? -1.0f : (d[1] > 1.0f ? 1.0f : d[1]);
    const float v = dm_acos(dy) / PI_F;
    fx = u * (float)K.width - 0.5f;
    fy = v * (float)K.height - 0.5f;
    if (!(fy >= -0.5f)) fy = -0.5f;  // NaN
}

OCTPT_SKY_FN void sky_radiance(const Sky &K, const float d[3], float out[3]) {
    if (K.mode == kSkyMap) {
        float fx, fy;
        sky_map_position(K, d, fx, fy);
        const float x0f = floorf(fx), y0f = floorf(fy);
        const float wx = fx - x0f, wy = fy - y0f;
        const int32_t W = (int32_t)K.width, H = (int32_t)K.height;
        int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;  // -1 .. W, -1 .. H - 1
        if (x0 < 0) x0 += W;
        if (x0 >= W) x0 -= W;
        int32_t x1 = x0 + 1;
        if (x1 >= W) x1 -= W;
        int32_t y1 = y0 + 1;
        if (y0 < 0) y0 = 0;
        if (y0 > H - 1) y0 = H - 1;
        if (y1 > H - 1) y1 = H - 1;
        float a[3], b[3], c[3], e[3];
        sky_texel(K, (uint32_t)x0, (uint32_t)y0, a);
        sky_texel(K, (uint32_t)x1, (uint32_t)y0, b);
        sky_texel(K, (uint32_t)x0, (uint32_t)y1, c);
        sky_texel(K, (uint32_t)x1, (uint32_t)y1, e);
        for (int i = 0; i < 3; ++i) {
            const float top = a[i] + wx * (b[i] - a[i]);
            const float bot = c[i] + wx * (e[i] - c[i]);
            const float r = (top + wy * (bot - top)) * K.scale;
            out[i] = r < FLT_MAX ? r : FLT_MAX;
        }
    } else if (K.mode == kSkyGradient) {
        const float t = d[1] > 0.0f ? d[1] : 0.0f;
        for (int i = 0; i < 3; ++i) out[i] = (K.horizon[i] + (K.zenith[i] - K.horizon[i]) * t) * K.scale;
    } else if (K.mode == kSkyColor) {
        for (int i = 0; i < 3; ++i) out[i] = K.color[i] * K.scale;
    } else {
        out[0] = 0.5f; out[1] = 0.7f; out[2] = 1.0f;
    }
}

}  // namespace octpt
