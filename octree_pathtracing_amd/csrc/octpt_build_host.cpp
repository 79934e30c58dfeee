// octpt_build_host.cpp -- the host octree builders of the octpt C ABI (include/octpt.h): primitive
// worlds (octpt_build_octree), block cells (octpt_build_block_octree), 16^3 palette sections
// (octpt_sections_to_cells), and the octree handle's view and free.  Pure host code: no context, no device call.
// The GPU builders (octpt_build.hip) produce the same arrays.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "../../include/octpt.h"
#include "octpt_internal.h"
#include "octpt_emitter.h"

using namespace octpt;

namespace {

uint64_t part_by_2(uint64_t v) {  // new_octree.rs:813-822
    uint64_t x = v & 0x1fffff;
    x = (x | x << 32) & 0x1f00000000ffffULL;
    x = (x | x << 16) & 0x1f0000ff0000ffULL;
    x = (x | x << 8) & 0x100f00f00f00f00fULL;
    x = (x | x << 4) & 0x10c30c30c30c30c3ULL;
    x = (x | x << 2) & 0x1249249249249249ULL;
    return x;
}
inline uint64_t morton(uint64_t x, uint64_t y, uint64_t z) { return (part_by_2(z) << 2) + (part_by_2(y) << 1) + part_by_2(x); }

struct CellPrim {
    uint64_t code;
    uint32_t prim;
    bool operator<(const CellPrim &o) const { return code != o.code ? code < o.code : prim < o.prim; }
};

// Pre-order octant emission.  node() returns the child its parent stores: an octant
// id, or with compaction a leaf payload when the octant's eight children are leaves holding the same
// primitive list (Octant::is_compactable, new_octree.rs:227-233, applied bottom-up at every level as
// RegionOctreeBuilder::recursive_build does, :679-690: the octant becomes Lod(get_child(0))).  The
// root is never merged away (a Lod root stays one octant of eight equal leaves, :534-545).
struct Builder {
    octpt_octree *t;
    std::vector<uint64_t> leaf_code;
    uint32_t depth;
    bool compact;
    struct Child {
        bool leaf;
        uint32_t v;
    };
    bool same_leaf(uint32_t a, uint32_t b) const {
        const uint32_t n = t->leaf_count[a];
        return n == t->leaf_count[b] &&
               std::memcmp(&t->leaf_prims[t->leaf_first[a]], &t->leaf_prims[t->leaf_first[b]], n * sizeof(uint32_t)) == 0;
    }
    Child node(uint32_t level, uint32_t lo, uint32_t hi) {
        const uint32_t id = (uint32_t)t->octants.size();
        t->octants.push_back(octpt_octant{0, 0, {0, 0, 0, 0, 0, 0, 0, 0}});
        const uint32_t shift = 3 * (depth - 1 - level);
        uint32_t a = lo;
        for (uint32_t c = 0; c < 8; ++c) {
            uint32_t b = a;
            while (b < hi && ((leaf_code[b] >> shift) & 7u) == c) ++b;
            if (b == a) continue;
            if (level + 1 == depth) {
                t->octants[id].child_mask |= (uint16_t)((1u << c) | (1u << (c + 8)));
                t->octants[id].children[c] = a;
            } else {
                const Child ch = node(level + 1, a, b);
                t->octants[id].child_mask |= (uint16_t)(ch.leaf ? ((1u << c) | (1u << (c + 8))) : (1u << c));
                t->octants[id].children[c] = ch.v;
            }
            a = b;
        }
        if (compact && level > 0 && t->octants[id].child_mask == 0xFFFFu) {
            const uint32_t *ch = t->octants[id].children;
            bool same = true;
            for (int k = 1; k < 8 && same; ++k) same = same_leaf(ch[0], ch[k]);
            if (same) {  // all children are leaves: this octant is the last one emitted
                const uint32_t v = ch[0];
                t->octants.pop_back();
                return Child{true, v};
            }
        }
        return Child{false, id};
    }
};

// Block-value octree (C23): leaf payloads are block ids.  Pre-order emission over the Morton-sorted
// cells as Builder does; with compaction an octant whose eight children are leaves holding the same
// block value becomes one leaf of its parent (Octant::is_compactable, new_octree.rs:227-233: all eight
// leaf bits set and every child value equal -- the reference's rule for leaf children), bottom-up at
// every level as SectionOctantBuilder::insert_child_and_compact / RegionOctreeBuilder::recursive_build
// apply it (:688-709, 582-587).  The root stays an octant.
struct BlockBuilder {
    octpt_octree *t;
    const std::vector<std::pair<uint64_t, uint32_t>> &cells;  // (Morton code, block), sorted
    uint32_t depth;
    bool compact;
    struct Child {
        bool leaf;
        uint32_t v;
    };
    Child node(uint32_t level, size_t lo, size_t hi) {
        const uint32_t id = (uint32_t)t->octants.size();
        t->octants.push_back(octpt_octant{0, 0, {0, 0, 0, 0, 0, 0, 0, 0}});
        const uint32_t shift = 3 * (depth - 1 - level);
        size_t a = lo;
        for (uint32_t c = 0; c < 8; ++c) {
            size_t b = a;
            while (b < hi && ((cells[b].first >> shift) & 7u) == c) ++b;
            if (b == a) continue;
            Child ch{true, cells[a].second};
            if (level + 1 < depth) ch = node(level + 1, a, b);
            t->octants[id].child_mask |= (uint16_t)(ch.leaf ? ((1u << c) | (1u << (c + 8))) : (1u << c));
            t->octants[id].children[c] = ch.v;
            a = b;
        }
        if (compact && level > 0 && t->octants[id].child_mask == 0xFFFFu) {
            const uint32_t *ch = t->octants[id].children;
            bool same = true;
            for (int k = 1; k < 8 && same; ++k) same = ch[k] == ch[0];
            if (same) {  // eight equal leaves: this octant is the last one emitted
                const uint32_t v = ch[0];
                t->octants.pop_back();
                return Child{true, v};
            }
        }
        return Child{false, id};
    }
};

inline int32_t clamp_cell(float f, int32_t hi) {
    if (!(f >= 0.0f)) return 0;  // also NaN
    if (f >= (float)hi) return hi;
    return (int32_t)f;
}

}  // namespace

namespace octpt {

// Upper bound of the (cell, primitive) pairs: the clamped bounding-box cells of every primitive.
// Leaf tables index pairs with uint32, and a scene past 2^31 pairs (>= 32 GiB of pairs) is refused
// up front rather than discovered by allocating until bad_alloc.  Cuboid cells span floor(min) ..
// ceil(max) - 1: a face on an integer plane does not claim the next cell, so a unit block
// [x, x+1) is exactly one cell (the voxel world of C5).
uint64_t pair_bound(const octpt_sphere *spheres, uint32_t ns, const octpt_cuboid *cuboids, uint32_t nc,
                    uint32_t depth) {
    const int32_t N = 1 << depth;
    uint64_t bound = 0;
    auto cub_hi = [](float lo, float hi) { return std::max(floorf(lo), ceilf(hi) - 1.0f); };
    auto add_box = [&](const float *lo_f, const float *hi_f, bool half_open) {
        uint64_t cells = 1;
        for (int a = 0; a < 3; ++a) {
            const float fl = floorf(lo_f[a]), fh = half_open ? cub_hi(lo_f[a], hi_f[a]) : floorf(hi_f[a]);
            if (fh < 0.0f || fl > (float)(N - 1) || hi_f[a] < lo_f[a]) return;
            cells *= (uint64_t)(clamp_cell(fh, N - 1) - clamp_cell(fl, N - 1) + 1);
        }
        bound = std::min<uint64_t>(bound + cells, UINT64_MAX / 2);
    };
    for (uint32_t i = 0; i < ns; ++i) {
        const float *c = spheres[i].center, r = spheres[i].radius;
        if (!(r > 0.0f)) continue;
        const float lo_f[3] = {c[0] - r, c[1] - r, c[2] - r}, hi_f[3] = {c[0] + r, c[1] + r, c[2] + r};
        add_box(lo_f, hi_f, false);
    }
    for (uint32_t i = 0; i < nc; ++i) add_box(cuboids[i].min, cuboids[i].max, true);
    return bound;
}

// the section world's own refusals before any array is read: 0, or the status (the three entries share it)
octpt_status section_world_status(const octpt_section_world *w, uint32_t depth) {
    if (!w || depth < 4 || depth > kMaxDepth) return OCTPT_ERR_INVALID_ARG;
    if ((w->section_count && !w->sections) || (w->palette_size && !w->palette) || (w->index_count && !w->indices))
        return OCTPT_ERR_INVALID_ARG;
    if (w->index_count % 4096u) return OCTPT_ERR_INVALID_ARG;
    if (w->section_count >= kMaxBuildPairs) return OCTPT_ERR_OOM;  // one block of threads per section
    return OCTPT_OK;
}

// the emissive flag of every block (C38): 1 for a block that fills its cell (no model) and has a face material
// with emittance > EPSILON; false: a face material index outside the table
bool block_emissive_flags(const octpt_block *blocks, uint32_t nb, const octpt_material *mats, uint32_t nm,
                          std::vector<uint32_t> &out) {
    out.assign(nb, 0u);
    for (uint32_t b = 0; b < nb; ++b) {
        if (blocks[b].model != OCTPT_MODEL_NONE) continue;
        for (int f = 0; f < 6; ++f) {
            const uint32_t m = blocks[b].face_material[f];
            if (m >= nm) return false;
            if (mats[m].emittance > kEmitterEpsilon) out[b] = 1u;
        }
    }
    return true;
}

// count-then-fill of octpt_emitter_grid_arrays: the counts into *out, then OK when the call only counts or the
// arrays hold them (fill = true), INVALID_ARG (nothing may be written) else
octpt_status emitter_grid_receive(octpt_emitter_grid_arrays *out, uint32_t n_cells, uint32_t n_entries,
                                  uint32_t n_emitters, uint32_t cells_axis, bool &fill) {
    fill = false;
    out->cell_count = n_cells;
    out->entry_count = n_entries;
    out->emitter_count = n_emitters;
    out->cells_per_axis = cells_axis;
    if (!out->cell_first && !out->cell_emitters && !out->emitters) return OCTPT_OK;
    if (!out->cell_first || !out->cell_emitters || !out->emitters) return OCTPT_ERR_INVALID_ARG;
    if (out->cell_first_capacity < (uint64_t)n_cells + 1u || out->cell_emitters_capacity < n_entries ||
        out->emitters_capacity < n_emitters)
        return OCTPT_ERR_INVALID_ARG;
    fill = true;
    return OCTPT_OK;
}

// ---- emissive block models (C39) ----
bool emissive_model_table(const octpt_block_model *models, uint32_t n_models, const octpt_quad *quads, uint32_t n_quads,
                          const octpt_material *mats, uint32_t nm, EmissiveModelTable &out) {
    out.first.assign((size_t)n_models + 1u, 0u);
    out.quad.clear();
    out.cum.clear();
    out.ouv.clear();
    for (uint32_t m = 0; m < n_models; ++m) {
        const uint64_t lo = models[m].first_quad, hi = lo + models[m].quad_count;
        if (hi > n_quads) return false;
        float sum = 0.0f;
        for (uint64_t q = lo; q < hi; ++q) {
            const octpt_quad &Q = quads[q];
            if (Q.material >= nm) return false;
            if (!(mats[Q.material].emittance > kEmitterEpsilon)) continue;
            const float a = emit_quad_area(Q.u, Q.v);
            if (!(a > 0.0f) || !(a < __builtin_inff())) continue;
            sum = sum + a;
            out.quad.push_back((uint32_t)q);
            out.cum.push_back(sum);
            out.ouv.insert(out.ouv.end(), Q.origin, Q.origin + 3);
            out.ouv.insert(out.ouv.end(), Q.u, Q.u + 3);
            out.ouv.insert(out.ouv.end(), Q.v, Q.v + 3);
        }
        out.first[m + 1u] = (uint32_t)out.quad.size();
    }
    return true;
}

octpt_status emitter_models_receive(octpt_emitter_model_arrays *out, uint32_t n_models, uint32_t n_entries, bool &fill) {
    fill = false;
    out->model_count = n_models;
    out->entry_count = n_entries;
    if (!out->model_first && !out->quad_index && !out->cum_area) return OCTPT_OK;
    if (!out->model_first || !out->quad_index || !out->cum_area) return OCTPT_ERR_INVALID_ARG;
    if (out->model_first_capacity < (uint64_t)n_models + 1u || out->quad_index_capacity < n_entries ||
        out->cum_area_capacity < n_entries)
        return OCTPT_ERR_INVALID_ARG;
    fill = true;
    return OCTPT_OK;
}

std::vector<uint8_t> model_emissive_bytes(const EmissiveModelTable &t) {
    std::vector<uint8_t> e(t.first.size() - 1u);
    for (size_t m = 0; m < e.size(); ++m) e[m] = t.first[m + 1] > t.first[m] ? 1u : 0u;
    return e;
}

bool block_emissive_flags_models(const octpt_block *blocks, uint32_t nb, const std::vector<uint8_t> &model_emissive,
                                 std::vector<uint32_t> &flags) {
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t m = blocks[b].model;
        if (m == OCTPT_MODEL_NONE) continue;
        if (m >= model_emissive.size()) return false;
        if (model_emissive[m]) flags[b] = kEmitModelBit | m;
    }
    return true;
}

}  // namespace octpt

namespace {

struct HostEmitter {
    uint64_t code;
    octpt_emitter e;
    bool operator<(const HostEmitter &o) const { return code < o.code; }
};

// the emissive leaves under octant o (corner (x, y, z), side s), in any order
bool collect_emitters(const octpt_octree &t, uint32_t o, uint32_t x, uint32_t y, uint32_t z, uint32_t s,
                      const std::vector<uint32_t> &emissive, std::vector<HostEmitter> &out) {
    const octpt_octant &oc = t.octants[o];
    const uint32_t h = s >> 1;
    for (uint32_t i = 0; i < 8u; ++i) {
        if (!((oc.child_mask >> i) & 1u)) continue;
        const uint32_t cx = x + ((i & 1u) ? h : 0u), cy = y + ((i & 2u) ? h : 0u), cz = z + ((i & 4u) ? h : 0u);
        const uint32_t v = oc.children[i];
        if ((oc.child_mask >> (i + 8u)) & 1u) {
            if (v >= emissive.size()) return false;
            // a full-cell emitter's side, or a model emitter's kEmitModelBit | model (C39)
            if (emissive[v]) out.push_back({morton(cx, cy, cz), {cx, cy, cz, emissive[v] == 1u ? h : emissive[v]}});
        } else if (!collect_emitters(t, v, cx, cy, cz, h, emissive, out)) {
            return false;
        }
    }
    return true;
}

}  // namespace

extern "C" {

octpt_status octpt_emitter_model_table(const octpt_block_model *models, uint32_t n_models, const octpt_quad *quads,
                                       uint32_t n_quads, const octpt_material *mats, uint32_t nm,
                                       octpt_emitter_model_arrays *out) {
    if (!out) return OCTPT_ERR_INVALID_ARG;
    out->model_count = out->entry_count = 0u;
    if ((n_models && !models) || (n_quads && !quads) || (nm && !mats)) return OCTPT_ERR_INVALID_ARG;
    try {
        EmissiveModelTable t;
        if (!emissive_model_table(models, n_models, quads, n_quads, mats, nm, t)) return OCTPT_ERR_INVALID_ARG;
        bool fill = false;
        const octpt_status st = emitter_models_receive(out, n_models, (uint32_t)t.quad.size(), fill);
        if (st != OCTPT_OK || !fill) return st;
        std::copy(t.first.begin(), t.first.end(), out->model_first);
        std::copy(t.quad.begin(), t.quad.end(), out->quad_index);
        std::copy(t.cum.begin(), t.cum.end(), out->cum_area);
        return OCTPT_OK;
    } catch (const std::bad_alloc &) {
        return OCTPT_ERR_OOM;
    }
}

octpt_status octpt_build_emitter_grid(const uint32_t *cells, uint32_t n, const octpt_block *blocks, uint32_t nb,
                                      const octpt_material *mats, uint32_t nm, uint32_t depth, uint32_t flags,
                                      uint32_t grid_size, octpt_emitter_grid_arrays *out) {
    return octpt_build_emitter_grid_models(cells, n, blocks, nb, mats, nm, nullptr, 0u, nullptr, 0u, depth, flags,
                                           grid_size, 0u, out);
}

octpt_status octpt_build_emitter_grid_models(const uint32_t *cells, uint32_t n, const octpt_block *blocks, uint32_t nb,
                                             const octpt_material *mats, uint32_t nm, const octpt_block_model *models,
                                             uint32_t n_models, const octpt_quad *quads, uint32_t n_quads,
                                             uint32_t depth, uint32_t flags, uint32_t grid_size, uint32_t emitter_flags,
                                             octpt_emitter_grid_arrays *out) {
    if (!out) return OCTPT_ERR_INVALID_ARG;
    out->cell_count = out->entry_count = out->emitter_count = out->cells_per_axis = 0u;
    if ((nb && !blocks) || (nm && !mats)) return OCTPT_ERR_INVALID_ARG;
    if (emitter_flags & ~OCTPT_EMITTERS_MODELS) return OCTPT_ERR_INVALID_ARG;
    const bool with_models = (emitter_flags & OCTPT_EMITTERS_MODELS) != 0u;
    if (with_models && ((n_models && !models) || (n_quads && !quads) || n_models > 0x7FFFFFFFu))
        return OCTPT_ERR_INVALID_ARG;
    if (depth < 1 || depth > kMaxDepth) return OCTPT_ERR_INVALID_ARG;
    if (grid_size == 0u || (grid_size & (grid_size - 1u)) || grid_size > (1u << depth)) return OCTPT_ERR_INVALID_ARG;
    octpt_octree *tree = nullptr;
    const octpt_status bst = octpt_build_block_octree(cells, n, depth, flags, &tree);
    if (bst != OCTPT_OK) return bst;
    std::unique_ptr<octpt_octree> hold(tree);
    try {
        std::vector<uint32_t> emissive;
        if (!block_emissive_flags(blocks, nb, mats, nm, emissive)) return OCTPT_ERR_INVALID_ARG;
        if (with_models) {  // C39
            EmissiveModelTable table;
            if (!emissive_model_table(models, n_models, quads, n_quads, mats, nm, table)) return OCTPT_ERR_INVALID_ARG;
            if (!block_emissive_flags_models(blocks, nb, model_emissive_bytes(table), emissive)) return OCTPT_ERR_INVALID_ARG;
        }
        std::vector<HostEmitter> em;
        if (!collect_emitters(*tree, tree->root, 0u, 0u, 0u, 1u << depth, emissive, em)) return OCTPT_ERR_INVALID_ARG;
        if (em.size() > kMaxEmitters) return OCTPT_ERR_OOM;
        std::sort(em.begin(), em.end());
        uint32_t shift = 0;
        while ((1u << shift) < grid_size) ++shift;
        const uint64_t G = (uint64_t)1u << (depth - shift);
        if (G * G * G > kMaxEmitterCells) return OCTPT_ERR_OOM;
        const uint32_t n_cells = (uint32_t)(G * G * G);
        // every emitter into the lists of its home cell's 27-neighbourhood: count, scan, fill in Morton order
        std::vector<uint64_t> first((size_t)n_cells + 1u, 0u);
        auto each_cell = [&](const octpt_emitter &e, auto fn) {
            const int64_t hx = e.x >> shift, hy = e.y >> shift, hz = e.z >> shift;
            for (int64_t dz = -1; dz <= 1; ++dz)
                for (int64_t dy = -1; dy <= 1; ++dy)
                    for (int64_t dx = -1; dx <= 1; ++dx) {
                        const int64_t cx = hx + dx, cy = hy + dy, cz = hz + dz;
                        if (cx < 0 || cy < 0 || cz < 0 || cx >= (int64_t)G || cy >= (int64_t)G || cz >= (int64_t)G)
                            continue;
                        fn((size_t)(cx + (int64_t)G * (cy + (int64_t)G * cz)));
                    }
        };
        for (const HostEmitter &h : em) each_cell(h.e, [&](size_t c) { first[c + 1]++; });
        for (size_t c = 0; c < n_cells; ++c) first[c + 1] += first[c];
        if (first[n_cells] > kMaxEmitterEntries) return OCTPT_ERR_OOM;
        bool fill = false;
        const octpt_status st =
            emitter_grid_receive(out, n_cells, (uint32_t)first[n_cells], (uint32_t)em.size(), (uint32_t)G, fill);
        if (st != OCTPT_OK || !fill) return st;
        std::vector<uint32_t> next(first.begin(), first.end() - 1);
        for (size_t k = 0; k < em.size(); ++k) {
            out->emitters[k] = em[k].e;
            each_cell(em[k].e, [&](size_t c) { out->cell_emitters[next[c]++] = (uint32_t)k; });
        }
        for (size_t c = 0; c <= n_cells; ++c) out->cell_first[c] = (uint32_t)first[c];
        return OCTPT_OK;
    } catch (const std::bad_alloc &) {
        return OCTPT_ERR_OOM;
    } catch (...) {
        return OCTPT_ERR_INTERNAL;
    }
}

octpt_status octpt_build_octree(const octpt_sphere *spheres, uint32_t ns, const octpt_cuboid *cuboids, uint32_t nc,
                                uint32_t depth, octpt_octree **out) {
    return octpt_build_octree_ex(spheres, ns, cuboids, nc, depth, 0u, out);
}

octpt_status octpt_build_octree_ex(const octpt_sphere *spheres, uint32_t ns, const octpt_cuboid *cuboids, uint32_t nc,
                                   uint32_t depth, uint32_t flags, octpt_octree **out) {
    if (!out) return OCTPT_ERR_INVALID_ARG;
    if (flags & ~OCTPT_BUILD_COMPACT) return OCTPT_ERR_INVALID_ARG;
    *out = nullptr;
    if (depth < 1 || depth > kMaxDepth) return OCTPT_ERR_INVALID_ARG;
    if ((ns && !spheres) || (nc && !cuboids)) return OCTPT_ERR_INVALID_ARG;
    try {
        const int32_t N = 1 << depth;
        const uint64_t bound = pair_bound(spheres, ns, cuboids, nc, depth);
        if (bound > kMaxBuildPairs) return OCTPT_ERR_OOM;
        // cuboid cells are half-open at the top (pair_bound)
        auto cub_hi = [](float lo, float hi) { return std::max(floorf(lo), ceilf(hi) - 1.0f); };
        std::vector<CellPrim> cells;
        cells.reserve((size_t)std::min<uint64_t>(bound, 1ull << 24));
        for (uint32_t i = 0; i < ns; ++i) {
            const float *c = spheres[i].center;
            const float r = spheres[i].radius;
            if (!(r > 0.0f)) continue;
            int32_t lo[3], hi[3];
            bool empty = false;
            for (int a = 0; a < 3; ++a) {
                const float fl = floorf(c[a] - r), fh = floorf(c[a] + r);
                if (fh < 0.0f || fl > (float)(N - 1)) empty = true;
                lo[a] = clamp_cell(fl, N - 1);
                hi[a] = clamp_cell(fh, N - 1);
            }
            if (empty) continue;
            const float r2 = r * r;
            for (int32_t z = lo[2]; z <= hi[2]; ++z)
                for (int32_t y = lo[1]; y <= hi[1]; ++y)
                    for (int32_t x = lo[0]; x <= hi[0]; ++x) {
                        const float bl[3] = {(float)x, (float)y, (float)z};
                        float dd[3];
                        for (int a = 0; a < 3; ++a) {
                            const float l = bl[a], h = bl[a] + 1.0f;
                            dd[a] = c[a] < l ? l - c[a] : (c[a] > h ? c[a] - h : 0.0f);
                        }
                        if ((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2] <= r2)
                            cells.push_back(CellPrim{morton((uint64_t)x, (uint64_t)y, (uint64_t)z), i});
                    }
        }
        for (uint32_t i = 0; i < nc; ++i) {
            const octpt_cuboid &b = cuboids[i];
            int32_t lo[3], hi[3];
            bool empty = false;
            for (int a = 0; a < 3; ++a) {
                const float fl = floorf(b.min[a]), fh = cub_hi(b.min[a], b.max[a]);
                if (fh < 0.0f || fl > (float)(N - 1) || b.max[a] < b.min[a]) empty = true;
                lo[a] = clamp_cell(fl, N - 1);
                hi[a] = clamp_cell(fh, N - 1);
            }
            if (empty) continue;
            for (int32_t z = lo[2]; z <= hi[2]; ++z)
                for (int32_t y = lo[1]; y <= hi[1]; ++y)
                    for (int32_t x = lo[0]; x <= hi[0]; ++x)
                        cells.push_back(CellPrim{morton((uint64_t)x, (uint64_t)y, (uint64_t)z), i | kPrimCuboidBit});
        }
        std::sort(cells.begin(), cells.end());
        octpt_octree *t = new octpt_octree();
        t->depth = depth;
        std::vector<uint64_t> codes;
        t->leaf_prims.resize(cells.size());
        for (size_t k = 0; k < cells.size(); ++k) {
            if (k == 0 || cells[k].code != cells[k - 1].code) {
                t->leaf_first.push_back((uint32_t)k);
                t->leaf_count.push_back(0);
                codes.push_back(cells[k].code);
            }
            t->leaf_count.back()++;
            t->leaf_prims[k] = cells[k].prim;
        }
        Builder b{t, std::move(codes), depth, (flags & OCTPT_BUILD_COMPACT) != 0};
        t->root = b.node(0, 0, (uint32_t)b.leaf_code.size()).v;
        *out = t;
        return OCTPT_OK;
    } catch (const std::bad_alloc &) {
        return OCTPT_ERR_OOM;
    } catch (...) {
        return OCTPT_ERR_INTERNAL;
    }
}

octpt_status octpt_build_block_octree(const uint32_t *cells, uint32_t n, uint32_t depth, uint32_t flags,
                                      octpt_octree **out) {
    if (!out) return OCTPT_ERR_INVALID_ARG;
    *out = nullptr;
    if (flags & ~OCTPT_BUILD_COMPACT) return OCTPT_ERR_INVALID_ARG;
    if (depth < 1 || depth > kMaxDepth || (n && !cells)) return OCTPT_ERR_INVALID_ARG;
    try {
        const uint32_t N = 1u << depth;
        std::vector<std::pair<uint64_t, uint32_t>> sorted(n);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t *c = cells + 4 * (size_t)k;
            if (c[0] >= N || c[1] >= N || c[2] >= N || c[3] > kPrimIndexMask) return OCTPT_ERR_INVALID_ARG;
            sorted[k] = {morton(c[0], c[1], c[2]), c[3]};
        }
        std::sort(sorted.begin(), sorted.end());
        for (size_t k = 1; k < sorted.size(); ++k)
            if (sorted[k].first == sorted[k - 1].first) return OCTPT_ERR_INVALID_ARG;  // two blocks in one cell
        std::unique_ptr<octpt_octree> t(new octpt_octree());
        t->depth = depth;
        BlockBuilder b{t.get(), sorted, depth, (flags & OCTPT_BUILD_COMPACT) != 0};
        t->root = b.node(0, 0, sorted.size()).v;
        *out = t.release();
        return OCTPT_OK;
    } catch (const std::bad_alloc &) {
        return OCTPT_ERR_OOM;
    } catch (...) {
        return OCTPT_ERR_INTERNAL;
    }
}

octpt_status octpt_sections_to_cells(const octpt_section_world *w, uint32_t depth, uint32_t *cells, uint32_t capacity,
                                     uint32_t *count) {
    if (!count) return OCTPT_ERR_INVALID_ARG;
    *count = 0u;
    const octpt_status st = section_world_status(w, depth);
    if (st != OCTPT_OK) return st;
    try {
        // validate and count: sections in ascending Morton code of their coordinates
        std::vector<std::pair<uint64_t, uint32_t>> order(w->section_count);
        uint64_t total = 0;
        for (uint32_t s = 0; s < w->section_count; ++s) {
            const octpt_section &sec = w->sections[s];
            if ((sec.x | sec.y | sec.z) >> (depth - 4u)) return OCTPT_ERR_INVALID_ARG;
            if (sec.palette_count == 0u || sec.palette_count > 4096u ||
                (uint64_t)sec.palette_first + sec.palette_count > w->palette_size)
                return OCTPT_ERR_INVALID_ARG;
            const uint32_t *pal = w->palette + sec.palette_first;
            for (uint32_t i = 0; i < sec.palette_count; ++i)
                if (pal[i] > kPrimIndexMask) return OCTPT_ERR_INVALID_ARG;
            if (sec.index_first == OCTPT_SECTION_UNIFORM) {
                if (sec.palette_count != 1u) return OCTPT_ERR_INVALID_ARG;
                total += pal[0] ? 4096u : 0u;
            } else {
                if ((sec.index_first & 4095u) || (uint64_t)sec.index_first + 4096u > w->index_count)
                    return OCTPT_ERR_INVALID_ARG;
                const uint16_t *idx = w->indices + sec.index_first;
                for (uint32_t i = 0; i < 4096u; ++i) {
                    if (idx[i] >= sec.palette_count) return OCTPT_ERR_INVALID_ARG;
                    total += pal[idx[i]] ? 1u : 0u;
                }
            }
            order[s] = {morton(sec.x, sec.y, sec.z), s};
        }
        std::sort(order.begin(), order.end());
        for (size_t k = 1; k < order.size(); ++k)
            if (order[k].first == order[k - 1].first) return OCTPT_ERR_INVALID_ARG;  // two sections at one position
        if (total > kMaxBuildPairs) return OCTPT_ERR_OOM;
        *count = (uint32_t)total;
        if (!cells) return OCTPT_OK;
        if (capacity < total) return OCTPT_ERR_INVALID_ARG;
        uint32_t *out = cells;
        for (const auto &ks : order) {
            const octpt_section &sec = w->sections[ks.second];
            const uint32_t *pal = w->palette + sec.palette_first;
            const bool uniform = sec.index_first == OCTPT_SECTION_UNIFORM;
            const uint16_t *idx = uniform ? nullptr : w->indices + sec.index_first;
            for (uint32_t m = 0; m < 4096u; ++m) {  // local Morton order: x bit 0, y bit 1, z bit 2 per level
                uint32_t x = 0, y = 0, z = 0;
                for (uint32_t b = 0; b < 4u; ++b) {
                    x |= ((m >> (3u * b)) & 1u) << b;
                    y |= ((m >> (3u * b + 1u)) & 1u) << b;
                    z |= ((m >> (3u * b + 2u)) & 1u) << b;
                }
                const uint32_t v = uniform ? pal[0] : pal[idx[y << 8 | z << 4 | x]];
                if (!v) continue;
                out[0] = 16u * sec.x + x;
                out[1] = 16u * sec.y + y;
                out[2] = 16u * sec.z + z;
                out[3] = v;
                out += 4;
            }
        }
        return OCTPT_OK;
    } catch (const std::bad_alloc &) {
        return OCTPT_ERR_OOM;
    } catch (...) {
        return OCTPT_ERR_INTERNAL;
    }
}

octpt_status octpt_octree_get_view(const octpt_octree *t, octpt_octree_view *v) {
    if (!t || !v) return OCTPT_ERR_INVALID_ARG;
    v->octants = t->octants.data();
    v->octant_count = (uint32_t)t->octants.size();
    v->root = t->root;
    v->depth = t->depth;
    v->leaf_first = t->leaf_first.data();
    v->leaf_count = t->leaf_count.data();
    v->leaf_table_size = (uint32_t)t->leaf_first.size();
    v->leaf_prims = t->leaf_prims.data();
    v->leaf_prim_count = (uint32_t)t->leaf_prims.size();
    return OCTPT_OK;
}

void octpt_octree_free(octpt_octree *t) { delete t; }

}  // extern "C"
