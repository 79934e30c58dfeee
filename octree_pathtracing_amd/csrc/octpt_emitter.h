// The emitter sample of a diffuse reflection, DESIGN.md C38 (strategy ONE), stated once for the device (shade_segment's
// emitter instances) and the host (octpt_emitter_sample): which emitter of the hit point's grid cell is picked, the
// target in its cube, the shadow segment's direction and the geometric factor, and the contribution's expression.
// Plain f32 in this order, glam's dot-product order, correctly rounded division and sqrtf; both sides compile this
// text with contraction off (octpt_lens.h is to the lens what this header is to the emitter; the RNG is its).
#pragma once
#include "../../include/octpt.h"
#include "octpt_lens.h"

namespace octpt {

// the emitter stream of a hit: lowbias32(path rng state ^ kEmitStream), taken from the state before any other draw
// of the hit; the path's own stream is not advanced, so its draws are what they are without sampling
constexpr uint32_t kEmitStream = 0x454D4954u;
constexpr float kEmitOffset = 0.000001f;   // Ray::OFFSET
constexpr float kEmitEpsilon = 5e-8f;      // Ray::EPSILON

// the grid as the sample reads it (device pointers on the device, host arrays in octpt_emitter_sample)
struct EmitGrid {
    const uint32_t *cell_first, *cell_emitters;
    const octpt_emitter *emitters;
    uint32_t grid_shift;  // log2 grid_size
    uint32_t axis_bits;   // log2 cells per axis
    uint32_t world;       // 2^depth
    float intensity;      // Scene::emmitter_intensity
};

struct EmitShot {
    float p[3];    // the shadow segment's origin: hit point + n * OFFSET
    float dir[3];  // its direction, (t - p) / |t - p|
    float dist;
    float geom;    // |dir . n| / max(dist^2, 1)
    uint32_t K;    // the cell list's length
    uint32_t emitter;
};

// cell coordinate of floor(v), clamped to the world
OCTPT_LENS_FN uint32_t emit_cell_axis(float v, const EmitGrid &G) {
    const float f = floorf(v);
    const float hi = (float)(G.world - 1u);
    const float c = f < 0.0f ? 0.0f : (f > hi ? hi : f);
    return (uint32_t)(c == c ? c : 0.0f) >> G.grid_shift;  // (a NaN takes cell 0)
}

// The sample at hit point o with normal n, from rng state `rng` (not advanced).  false: nothing is traced (an empty
// list, or a target at distance 0 or not finite).  ONE picks one emitter of the K in the cell's list uniformly; the
// contribution carries the factor K, which makes it an unbiased estimate of the sum over the list -- a deliberate
// choice, where Chunky's ONE leaves the pick's probability out.
OCTPT_LENS_FN bool emitter_sample(const EmitGrid &G, const float o[3], const float n[3], uint32_t rng, EmitShot &s) {
    for (int i = 0; i < 3; ++i) s.p[i] = o[i] + n[i] * kEmitOffset;
    const uint32_t cx = emit_cell_axis(s.p[0], G), cy = emit_cell_axis(s.p[1], G), cz = emit_cell_axis(s.p[2], G);
    const uint32_t c = cx + (((cz << G.axis_bits) + cy) << G.axis_bits);
    const uint32_t first = G.cell_first[c];
    const uint32_t K = G.cell_first[c + 1u] - first;
    s.K = K;
    if (K == 0u) return false;
    uint32_t es = lowbias32(rng ^ kEmitStream);
    const float u0 = rng_next(es), u1 = rng_next(es), u2 = rng_next(es), u3 = rng_next(es);
    uint32_t k = (uint32_t)(u0 * (float)K);
    if (k > K - 1u) k = K - 1u;
    s.emitter = G.cell_emitters[first + k];
    const octpt_emitter e = G.emitters[s.emitter];
    const float side = (float)e.s;
    const float t[3] = {(float)e.x + side * u1, (float)e.y + side * u2, (float)e.z + side * u3};
    const float d[3] = {t[0] - s.p[0], t[1] - s.p[1], t[2] - s.p[2]};
    const float dist = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (!(dist > 0.0f) || !(dist < __builtin_inff())) return false;
    s.dist = dist;
    for (int i = 0; i < 3; ++i) s.dir[i] = d[i] / dist;
    const float dn = (s.dir[0] * n[0] + s.dir[1] * n[1]) + s.dir[2] * n[2];
    const float d2 = dist * dist;
    s.geom = fabsf(dn) / (d2 > 1.0f ? d2 : 1.0f);
    return true;
}

// e of the contribution L += T_before * albedo * (col_e^2 * e): geom from the shot, the emitter hit's emittance
OCTPT_LENS_FN float emitter_scale(float geom, float emittance, float intensity, uint32_t K) {
    return ((geom * emittance) * intensity) * (float)K;
}

}  // namespace octpt
