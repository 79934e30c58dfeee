// The portable f32 inverse trigonometry of DESIGN.md §3.11 -- dm_asin, dm_acos, dm_atan2 -- stated once for the device
// (the sphere's texture coordinates, the sun, the sky's map lookup) and the host (octpt_sky_radiance, csrc/octpt_sky.h).
// Identical constants and order to the oracle; plain f32, correctly rounded division and sqrtf, and both sides compile
// this text with contraction off.  (dm_sincos: csrc/octpt_lens.h.)
#pragma once
#include <cmath>

#if defined(__HIP__)
#define OCTPT_MATH_FN __host__ __device__ inline
#else
#define OCTPT_MATH_FN inline
#endif

#ifndef PI_F
#define PI_F 3.14159265358979323846f
#endif

namespace octpt {

OCTPT_MATH_FN float dm_asin(float x) {
    const float a = fabsf(x);
    float z, xx;
    bool flag = false;
    if (a > 0.5f) {
        z = 0.5f * (1.0f - a);
        xx = sqrtf(z);
        flag = true;
    } else {
        xx = a;
        z = a * a;
    }
    float r;
    if (a < 1.0e-4f && !flag) {
        r = xx;
    } else {
        r = ((((4.2163199048e-2f * z + 2.4181311049e-2f) * z + 4.5470025998e-2f) * z + 7.4953002686e-2f) * z +
             1.6666752422e-1f) * z * xx + xx;
    }
    if (flag) {
        r = r + r;
        r = 1.5707963267948966f - r;
    }
    return x < 0.0f ? -r : r;
}
OCTPT_MATH_FN float dm_acos(float x) {
    if (x < -0.5f) return PI_F - 2.0f * dm_asin(sqrtf(0.5f * (1.0f + x)));
    if (x > 0.5f) return 2.0f * dm_asin(sqrtf(0.5f * (1.0f - x)));
    return 1.5707963267948966f - dm_asin(x);
}
OCTPT_MATH_FN float dm_atan_core(float x) {
    float sgn = 1.0f, y;
    if (x < 0.0f) { sgn = -1.0f; x = -x; }
    if (x > 2.414213562373095f) {
        y = 1.5707963267948966f;
        x = -1.0f / x;
    } else if (x > 0.4142135623730950f) {
        y = 0.7853981633974483f;
        x = (x - 1.0f) / (x + 1.0f);
    } else {
        y = 0.0f;
    }
    const float z = x * x;
    y = y + ((((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f) * z * x + x);
    return sgn < 0.0f ? -y : y;
}
OCTPT_MATH_FN float dm_atan2(float y, float x) {
    int code = 0;
    if (x < 0.0f) code = 2;
    if (y < 0.0f) code |= 1;
    if (x == 0.0f) {
        if (code & 1) return -1.5707963267948966f;
        if (y == 0.0f) return 0.0f;
        return 1.5707963267948966f;
    }
    if (y == 0.0f) return (code & 2) ? PI_F : 0.0f;
    float w = 0.0f;
    if (code == 2) w = PI_F;
    else if (code == 3) w = -PI_F;
    return w + dm_atan_core(y / x);
}

}  // namespace octpt
