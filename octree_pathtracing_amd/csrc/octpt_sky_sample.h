// The sky map's importance sample, DESIGN.md C43, stated once for the device (the sky-sampling instances of shade and
// the drain, the distribution's builder in octpt_build.hip, and the kernel behind octpt_sky_sample_device) and the host
// (octpt_build_sky_distribution, octpt_sky_sample): the weight of a texel, its quantised integer, the pick of a texel
// from four draws, the direction inside it and the pdf by solid angle.  Plain f32 in this order; both sides compile
// this text with contraction off (octpt_emitter.h is to the emitters what this header is to the map; the RNG is
// octpt_lens.h's).
//
// The distribution is piecewise constant over the texels of the sanitised map and made of integers, so that a device
// build equals the host's whatever order a scan adds in:
//   lum(x, y) = min((0.2126 r + 0.7152 g) + 0.0722 b, FLT_MAX)
//   m(x, y)   = max of lum over the 3 x 3 neighbourhood, wrapped in x and clamped in y: the footprint of the bilinear
//               lookup of any direction that falls into texel (x, y), so the weight is non-zero wherever sky_radiance
//               can be -- what the estimator's unbiasedness rests on
//   w(x, y)   = min(m * row[y], FLT_MAX), row[y] = (float)sin(pi (y + 0.5) / H) from a table the host computes in double
//   q(x, y)   = 0 when w == 0, else clamp((uint32)ceilf((w / wmax) * 65536), 1, 65536), wmax = max w
//   col_cdf[y W + x]  uint32: the inclusive sum of q along row y (W <= 32768, so a row's total fits)
//   row_cdf[y]        uint64: the inclusive sum of the rows' totals;  total = row_cdf[H - 1]
// The quantisation costs efficiency only: the pdf is read from the integers the pick uses.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "octpt_lens.h"
#include "octpt_math.h"
#include "octpt_sky.h"

namespace octpt {

// the sky stream of a hit: lowbias32(path rng state ^ kSkySampleStream), taken from the state before any other draw of
// the hit; the path's own stream is not advanced, so its draws are what they are without sampling
constexpr uint32_t kSkySampleStream = 0x534B5953u;
constexpr uint32_t kSkySampleMaxWidth = 32768u;  // a row's total, at most W * 65536, fits 32 bits
constexpr float kSkyQuantum = 65536.0f;

// the distribution as the sample reads it (device pointers on the device, host arrays in octpt_sky_sample)
struct SkyDist {
    const uint64_t *row_cdf;  // height
    const uint32_t *col_cdf;  // width * height
    uint64_t total;           // row_cdf[height - 1]; 0: an all-black map, nothing to sample
};

struct SkyShot {
    float d[3];  // unit direction in world axes
    float pdf;   // by solid angle
    uint32_t x, y, q;
};

OCTPT_SKY_FN float sky_lum(const float t[3]) {
    const float l = (0.2126f * t[0] + 0.7152f * t[1]) + 0.0722f * t[2];
    return l < FLT_MAX ? l : FLT_MAX;
}

// w(x, y) over the sanitised map K.texels; row = row[y]
OCTPT_SKY_FN float sky_weight(const Sky &K, uint32_t x, uint32_t y, float row) {
    const uint32_t W = K.width, H = K.height;
    const uint32_t xs[3] = {x == 0u ? W - 1u : x - 1u, x, x + 1u == W ? 0u : x + 1u};
    const uint32_t ys[3] = {y == 0u ? 0u : y - 1u, y, y + 1u == H ? y : y + 1u};
    float m = 0.0f;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) {
            float t[3];
            sky_texel(K, xs[i], ys[j], t);
            const float l = sky_lum(t);
            m = l > m ? l : m;
        }
    const float w = m * row;
    return w < FLT_MAX ? w : FLT_MAX;
}

// row[y], on the host in double (both builders take it from the host: no device sine against a host sine)
inline float sky_row_factor(uint32_t y, uint32_t H) {
    return (float)std::sin(3.14159265358979323846 * ((double)y + 0.5) / (double)H);
}

// q of a weight; wmax = the map's largest weight (w <= wmax)
OCTPT_SKY_FN uint32_t sky_quantise(float w, float wmax) {
    if (!(w > 0.0f)) return 0u;
    const float c = ceilf((w / wmax) * kSkyQuantum);
    if (!(c >= 1.0f)) return 1u;
    return c < kSkyQuantum ? (uint32_t)c : 65536u;
}

// The first index i of cdf[0 .. n) with t < cdf[i], for t < cdf[n - 1]: ceil(log2 n) steps whatever t is, so the
// lanes of a wave take the same trip count and their loads stay in step.
template <class T>
OCTPT_SKY_FN uint32_t sky_search(const T *cdf, uint32_t n, T t) {
    uint32_t base = 0u, len = n;
    while (len > 1u) {
        const uint32_t half = len >> 1;
        if (!(t < cdf[base + half - 1u])) base += half;
        len -= half;
    }
    return base;
}

// The sample of draws u[0 .. 4) in [0, 1).  false: there is no sample (an all-black map, a direction at a pole, a pdf
// that is not finite and positive); s.pdf is 0 then.
//   row     t = min((uint64)(u0 * (float)total), total - 1): the first y with t < row_cdf[y]
//   column  s = min((uint32)(u1 * (float)rowsum), rowsum - 1): the first x with s < col_cdf[y W + x]
//   inside  u = (x + u2) / W, v = (y + u3) / H, theta = pi v, lon = 2 pi (u - 0.5) - yaw brought into [-pi, pi]
//   d = (sin theta cos lon, cos theta, sin theta sin lon): the inverse of sky_map_position
//   pdf = (((float)q / (float)total) * ((float)W * (float)H)) / (2 pi^2 * sin theta)
OCTPT_SKY_FN bool sky_sample_draws(const SkyDist &D, const Sky &K, const float u[4], SkyShot &s) {
    s.d[0] = s.d[1] = s.d[2] = 0.0f;
    s.pdf = 0.0f;
    s.x = s.y = s.q = 0u;
    if (D.total == 0ull) return false;
    const uint32_t W = K.width, H = K.height;
    uint64_t t = (uint64_t)(u[0] * (float)D.total);
    if (t > D.total - 1ull) t = D.total - 1ull;
    const uint32_t y = sky_search<uint64_t>(D.row_cdf, H, t);
    const uint32_t *row = D.col_cdf + (size_t)y * W;
    const uint32_t rowsum = row[W - 1u];
    if (rowsum == 0u) return false;  // (no picked row is empty: t lies below its cdf and not below the row's before)
    uint32_t c = (uint32_t)(u[1] * (float)rowsum);
    if (c > rowsum - 1u) c = rowsum - 1u;
    const uint32_t x = sky_search<uint32_t>(row, W, c);
    const uint32_t q = row[x] - (x != 0u ? row[x - 1u] : 0u);
    s.x = x;
    s.y = y;
    s.q = q;
    const float uu = ((float)x + u[2]) / (float)W, vv = ((float)y + u[3]) / (float)H;
    const float theta = PI_F * vv;
    float lon = 6.28318530717958647692f * (uu - 0.5f) - K.yaw;
    lon = lon - 6.28318530717958647692f * floorf(lon / 6.28318530717958647692f + 0.5f);
    lon = lon < -PI_F ? -PI_F : (lon > PI_F ? PI_F : lon);  // dm_sincos's range (octpt_lens.h)
    float st, ct, sl, cl;
    dm_sincos(theta, st, ct);
    dm_sincos(lon, sl, cl);
    if (!(st > 0.0f)) return false;
    const float pdf = (((float)q / (float)D.total) * ((float)W * (float)H)) / (19.7392088021787172376f * st);
    if (!(pdf > 0.0f) || !(pdf < __builtin_inff())) return false;
    s.d[0] = st * cl;
    s.d[1] = ct;
    s.d[2] = st * sl;
    s.pdf = pdf;
    return true;
}

// ... of a hit, from the path's rng state before any draw of the hit (not advanced)
OCTPT_SKY_FN bool sky_sample(const SkyDist &D, const Sky &K, uint32_t rng, SkyShot &s) {
    uint32_t ss = lowbias32(rng ^ kSkySampleStream);
    float u[4];
    u[0] = rng_next(ss);
    u[1] = rng_next(ss);
    u[2] = rng_next(ss);
    u[3] = rng_next(ss);
    return sky_sample_draws(D, K, u, s);
}

// e of the contribution L += (T_before * albedo) * (sky_radiance(d) * e): the diffuse BRDF's cosine over the pdf
OCTPT_SKY_FN float sky_sample_scale(float cosn, float pdf) { return (cosn / PI_F) / pdf; }

// out[8] of octpt_sky_sample and octpt_sky_sample_device: d.xyz, pdf, then the bit patterns of the 32-bit integers
// x, y, q and of 1 (a sample) or 0 (none: d and pdf are 0 then)
OCTPT_SKY_FN void sky_sample_pack(const SkyShot &s, bool ok, float out[8]) {
    uint32_t w[4] = {s.x, s.y, s.q, ok ? 1u : 0u};
    out[0] = s.d[0]; out[1] = s.d[1]; out[2] = s.d[2]; out[3] = s.pdf;
    for (int i = 0; i < 4; ++i) __builtin_memcpy(&out[4 + i], &w[i], 4);
}

}  // namespace octpt
