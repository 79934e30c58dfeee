// The emitter sample of a diffuse reflection, DESIGN.md C38 (strategy ONE), stated once for the device (shade_segment's
// emitter instances) and the host (octpt_emitter_sample): which emitter of the hit point's grid cell is picked, the
// target in its cube, the shadow segment's direction and the geometric factor, and the contribution's expression.
// With OCTPT_EMITTERS_MODELS (C39) an emitter may be an emissive block model: the target is a point of one of its quads.
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
    // model emitters (C39): flags = OCTPT_EMITTERS_MODELS or 0 (then nothing below is read); the emissive-model
    // table (octpt_emitter_model_table), and per table entry the quad's (origin, u, v), nine floats
    uint32_t flags;
    uint32_t pad;  // (no padding bytes: the context compares headers bytewise)
    const uint32_t *model_first, *quad_index;
    const float *cum_area, *quad_ouv;
};
constexpr uint32_t kEmitModelBit = 0x80000000u;  // an emitter record's fourth word: kEmitModelBit | model

struct EmitShot {
    float p[3];    // the shadow segment's origin: hit point + n * OFFSET
    float dir[3];  // its direction, (t - p) / |t - p|
    float dist;
    float geom;    // |dir . n| / max(dist^2, 1), for a model emitter times its emissive area A_m
    uint32_t K;    // the cell list's length
    uint32_t emitter;
    uint32_t quad;  // the picked quad of a model emitter (C39), 0xFFFFFFFF for a cube
};

// the area |u x v| of a quad (C39): each cross component a * b - c * d, the length sqrtf((x^2 + y^2) + z^2)
OCTPT_LENS_FN float emit_quad_area(const float u[3], const float v[3]) {
    const float x = u[1] * v[2] - u[2] * v[1], y = u[2] * v[0] - u[0] * v[2], z = u[0] * v[1] - u[1] * v[0];
    return sqrtf((x * x + y * y) + z * z);
}

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
    float t[3], area = 1.0f;
    const bool model = (G.flags & OCTPT_EMITTERS_MODELS) != 0u && (e.s & kEmitModelBit) != 0u;
    s.quad = 0xFFFFFFFFu;
    if (model) {
        // a model emitter (C39): the quad in proportion to its area, the first entry with u1 * A_m < cum_area, the
        // last one else; the target on it, at the leaf's corner
        const uint32_t m = e.s & ~kEmitModelBit;
        const uint32_t hi = G.model_first[m + 1u];
        uint32_t i = G.model_first[m];
        area = G.cum_area[hi - 1u];
        const float x = u1 * area;
        while (i + 1u < hi && !(x < G.cum_area[i])) ++i;
        const float *q = G.quad_ouv + 9u * i;
        const float corner[3] = {(float)e.x, (float)e.y, (float)e.z};
        for (int c = 0; c < 3; ++c) t[c] = ((q[c] + q[3 + c] * u2) + q[6 + c] * u3) + corner[c];
        s.quad = G.quad_index[i];
    } else {
        const float side = (float)e.s;
        t[0] = (float)e.x + side * u1;
        t[1] = (float)e.y + side * u2;
        t[2] = (float)e.z + side * u3;
    }
    const float d[3] = {t[0] - s.p[0], t[1] - s.p[1], t[2] - s.p[2]};
    const float dist = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (!(dist > 0.0f) || !(dist < __builtin_inff())) return false;
    s.dist = dist;
    for (int i = 0; i < 3; ++i) s.dir[i] = d[i] / dist;
    const float dn = (s.dir[0] * n[0] + s.dir[1] * n[1]) + s.dir[2] * n[2];
    const float d2 = dist * dist;
    s.geom = fabsf(dn) / (d2 > 1.0f ? d2 : 1.0f);
    if (model) s.geom = s.geom * area;  // Chunky's face-area form: the area-proportional pick makes the factor A_m
    return true;
}

// e of the contribution L += T_before * albedo * (col_e^2 * e): geom from the shot, the emitter hit's emittance
OCTPT_LENS_FN float emitter_scale(float geom, float emittance, float intensity, uint32_t K) {
    return ((geom * emittance) * intensity) * (float)K;
}

}  // namespace octpt
