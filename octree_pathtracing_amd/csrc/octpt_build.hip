// octpt_build.hip -- the octree builder on the GPU (the reference's
// flattener octree_to_gpu_data, gpu_octree.rs:28-76, is todo!()).
//
// It produces the octree of the host builder (octpt_build_octree) array for array:
// the same (cell, primitive) pairs, the same Morton order (new_octree.rs:752-835), the same leaf
// tables and the same pre-order octant numbering.  All integer / byte work, HBM-bound:
//
//   count  : one thread per primitive counts its cells (sphere: bounding-box cells passing the
//            closest-point test; cuboid: the half-open box)           -> per-primitive counts
//   scan   : exclusive sum                                            -> pair offsets
//   emit   : one thread per primitive writes (Morton code, primitive) in primitive order
//   sort   : stable LSD radix sort on the code (3*depth bits); equal codes keep primitive order,
//            which is the host's (code, prim) order because spheres precede cuboids (bit 31)
//   leaves : head flags + scan -> leaf_first / leaf_count / leaf codes
//   octants: leaf j opens floor(msb(code_j ^ code_j-1) / 3) new octants (depth for j = 0), one
//            per level from the first level where its path leaves its predecessor's; pre-order
//            numbers them consecutively, so ids = exclusive scan of that count.  Each new octant
//            links itself into its parent (found by binary search over the leaf codes when the
//            parent was opened by an earlier leaf), each leaf into its level depth-1 octant.
//
// Block-value octrees (octpt_build_block_octree, C23) take the same path from the sort on
// (build_block_octree_gpu): one thread per cell emits (Morton code, block), every cell is its own
// leaf (no head flags, no leaf tables), and a leaf's payload is its block value.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "../../include/octpt.h"
#include "octpt_internal.h"

namespace octpt {
namespace {

constexpr uint32_t kBuildBlock = 256;

__device__ __forceinline__ uint64_t part_by_2(uint64_t v) {  // new_octree.rs:813-822
    uint64_t x = v & 0x1fffff;
    x = (x | x << 32) & 0x1f00000000ffffULL;
    x = (x | x << 16) & 0x1f0000ff0000ffULL;
    x = (x | x << 8) & 0x100f00f00f00f00fULL;
    x = (x | x << 4) & 0x10c30c30c30c30c3ULL;
    x = (x | x << 2) & 0x1249249249249249ULL;
    return x;
}
__device__ __forceinline__ uint64_t morton(uint32_t x, uint32_t y, uint32_t z) {
    return (part_by_2(z) << 2) + (part_by_2(y) << 1) + part_by_2(x);
}

__device__ __forceinline__ int32_t clamp_cell(float f, int32_t hi) {
    if (!(f >= 0.0f)) return 0;  // also NaN
    if (f >= (float)hi) return hi;
    return (int32_t)f;
}

// the host builder's per-primitive cell box (octpt_build_host.cpp octpt_build_octree); false = no cells
__device__ inline bool prim_box(const octpt_sphere *sp, uint32_t ns, const octpt_cuboid *cb, uint32_t i, int32_t N,
                                int32_t lo[3], int32_t hi[3]) {
    if (i < ns) {
        const octpt_sphere s = sp[i];
        const float r = s.radius;
        if (!(r > 0.0f)) return false;
        bool empty = false;
        for (int a = 0; a < 3; ++a) {
            const float fl = floorf(s.center[a] - r), fh = floorf(s.center[a] + r);
            if (fh < 0.0f || fl > (float)(N - 1)) empty = true;
            lo[a] = clamp_cell(fl, N - 1);
            hi[a] = clamp_cell(fh, N - 1);
        }
        return !empty;
    }
    const octpt_cuboid b = cb[i - ns];
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        const float fl = floorf(b.min[a]), fh = fmaxf(fl, ceilf(b.max[a]) - 1.0f);  // half-open top
        if (fh < 0.0f || fl > (float)(N - 1) || b.max[a] < b.min[a]) empty = true;
        lo[a] = clamp_cell(fl, N - 1);
        hi[a] = clamp_cell(fh, N - 1);
    }
    return !empty;
}

// closest-point test of the host builder: squared distance from the centre to the cell <= r^2
__device__ __forceinline__ bool sphere_keeps(const octpt_sphere &s, int32_t x, int32_t y, int32_t z) {
    const float bl[3] = {(float)x, (float)y, (float)z};
    float dd[3];
    for (int a = 0; a < 3; ++a) {
        const float l = bl[a], h = bl[a] + 1.0f, c = s.center[a];
        dd[a] = c < l ? l - c : (c > h ? c - h : 0.0f);
    }
    return (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2] <= s.radius * s.radius;
}

__global__ __launch_bounds__(kBuildBlock) void count_cells_kernel(const octpt_sphere *__restrict__ sp, uint32_t ns,
                                                                  const octpt_cuboid *__restrict__ cb, uint32_t nc,
                                                                  int32_t N, unsigned long long *__restrict__ counts) {
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= ns + nc) return;
    int32_t lo[3], hi[3];
    unsigned long long n = 0;
    if (prim_box(sp, ns, cb, i, N, lo, hi)) {
        if (i < ns) {
            const octpt_sphere s = sp[i];
            for (int32_t z = lo[2]; z <= hi[2]; ++z)
                for (int32_t y = lo[1]; y <= hi[1]; ++y)
                    for (int32_t x = lo[0]; x <= hi[0]; ++x) n += sphere_keeps(s, x, y, z) ? 1u : 0u;
        } else {
            n = (unsigned long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
        }
    }
    counts[i] = n;
}

__global__ __launch_bounds__(kBuildBlock) void emit_pairs_kernel(const octpt_sphere *__restrict__ sp, uint32_t ns,
                                                                 const octpt_cuboid *__restrict__ cb, uint32_t nc,
                                                                 int32_t N, const unsigned long long *__restrict__ offs,
                                                                 uint64_t *__restrict__ codes,
                                                                 uint32_t *__restrict__ prims) {
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= ns + nc) return;
    int32_t lo[3], hi[3];
    if (!prim_box(sp, ns, cb, i, N, lo, hi)) return;
    unsigned long long o = offs[i];
    const bool sphere = i < ns;
    const uint32_t prim = sphere ? i : ((i - ns) | kPrimCuboidBit);
    const octpt_sphere s = sphere ? sp[i] : octpt_sphere{};
    for (int32_t z = lo[2]; z <= hi[2]; ++z)
        for (int32_t y = lo[1]; y <= hi[1]; ++y)
            for (int32_t x = lo[0]; x <= hi[0]; ++x) {
                if (sphere && !sphere_keeps(s, x, y, z)) continue;
                codes[o] = morton((uint32_t)x, (uint32_t)y, (uint32_t)z);
                prims[o] = prim;
                ++o;
            }
}

// block-value cells (C23): one thread per cell (x, y, z, block) writes (Morton code, block) and ORs what the
// host builder refuses into *err (kCellErr*; a coordinate out of range is masked by morton(), so nothing
// is written out of bounds before the host reads the word).  aligned: `cells` is 16-byte aligned
__global__ __launch_bounds__(kBuildBlock) void emit_cells_kernel(const uint32_t *__restrict__ cells, uint32_t n,
                                                                 uint32_t depth, uint32_t block_count, bool aligned,
                                                                 uint64_t *__restrict__ codes,
                                                                 uint32_t *__restrict__ blks,
                                                                 uint32_t *__restrict__ err) {
    const uint32_t k = blockIdx.x * kBuildBlock + threadIdx.x;
    if (k >= n) return;
    uint4 c;
    if (aligned) {
        c = reinterpret_cast<const uint4 *>(cells)[k];
    } else {
        const uint32_t *p = cells + 4u * (size_t)k;
        c = make_uint4(p[0], p[1], p[2], p[3]);
    }
    uint32_t e = 0u;
    if ((c.x | c.y | c.z) >> depth) e |= kCellErrRange;
    if (c.w > kPrimIndexMask) e |= kCellErrBlockId;
    if (block_count && c.w >= block_count) e |= kCellErrBlockTable;
    if (e) atomicOr(err, e);
    codes[k] = morton(c.x, c.y, c.z);
    blks[k] = c.w;
}

// ---------------------------------------------------------------------------
// 16^3 palette sections (octpt_build_block_octree_sections_device): the front end that writes the cell builder's
// (Morton code, block) streams already sorted.  One 256-thread block per section stages the section's palette
// slice (<= 16 KB) and its 4096 16-bit palette indices (8 KB) in LDS.
// ---------------------------------------------------------------------------
constexpr uint32_t kSectionCells = 4096;
// LDS position of index i = y<<8 | z<<4 | x: 4 pad entries (2 dwords) per y-plane, so the 4x4x4 cube a wave reads
// per emit step (x: 2 dwords, z: stride 8 dwords, y: stride 128 + 2 dwords) covers 32 distinct banks
__device__ __forceinline__ uint32_t index_slot(uint32_t i) { return i + ((i >> 8) << 2); }
constexpr uint32_t kSectionIndexSlots = kSectionCells + 16 * 4;

// the struct-level refusals (octpt_sections_to_cells): 0 = the palette slice and the index block may be read
__device__ inline uint32_t section_errors(const octpt_section &s, uint32_t depth, uint32_t palette_size,
                                          uint32_t index_count) {
    uint32_t e = 0u;
    if ((s.x | s.y | s.z) >> (depth - 4u)) e |= kCellErrRange;
    if (s.palette_count == 0u || s.palette_count > kSectionCells ||
        (uint64_t)s.palette_first + s.palette_count > palette_size)
        e |= kCellErrPalette;
    if (s.index_first == OCTPT_SECTION_UNIFORM) {
        if (s.palette_count != 1u) e |= kCellErrUniform;
    } else if ((s.index_first & (kSectionCells - 1u)) || (uint64_t)s.index_first + kSectionCells > index_count) {
        e |= kCellErrIndexBlock;
    }
    return e;
}

// what a block value raises (the cell builder's checks)
__device__ __forceinline__ uint32_t value_errors(uint32_t v, uint32_t block_count) {
    uint32_t e = 0u;
    if (v > kPrimIndexMask) e |= kCellErrBlockId;
    if (block_count && v >= block_count) e |= kCellErrBlockTable;
    return e;
}

// the section's 4096 indices into LDS (index_slot positions); aligned: 16-byte loads, else 2-byte loads
__device__ inline void stage_indices(const uint16_t *__restrict__ g, bool aligned, uint16_t *s_idx) {
    if (aligned) {
        const uint4 *g4 = reinterpret_cast<const uint4 *>(g);
        for (uint32_t q = threadIdx.x; q < kSectionCells / 8u; q += kBuildBlock) {
            const uint4 v = g4[q];
            uint2 *d = reinterpret_cast<uint2 *>(s_idx + index_slot(8u * q));  // 8-byte aligned: 16 q + 8 (q >> 5)
            d[0] = make_uint2(v.x, v.y);
            d[1] = make_uint2(v.z, v.w);
        }
    } else {
        for (uint32_t i = threadIdx.x; i < kSectionCells; i += kBuildBlock) s_idx[index_slot(i)] = g[i];
    }
}

// bits 0, 3, 6, 9 of v gathered into bits 0..3 (a coordinate of a 12-bit local Morton code)
__device__ __forceinline__ uint32_t compact_4(uint32_t v) {
    v &= 0x249u;
    v = (v | v >> 2) & 0x0C3u;
    v = (v | v >> 4) & 0x00Fu;
    return v;
}

// Count: block s validates section s and writes its Morton key, its id and its number of non-air cells (0 when
// the section is refused; every refusal is ORed into *err and nothing out of bounds is read)
__global__ __launch_bounds__(kBuildBlock) void section_count_kernel(
    const octpt_section *__restrict__ secs, const uint32_t *__restrict__ palette, uint32_t palette_size,
    const uint16_t *__restrict__ indices, uint32_t index_count, bool aligned, uint32_t depth, uint32_t block_count,
    uint64_t *__restrict__ keys, uint32_t *__restrict__ ids, uint32_t *__restrict__ counts,
    uint32_t *__restrict__ err) {
    __shared__ uint32_t s_pal[kSectionCells];
    __shared__ __attribute__((aligned(16))) uint16_t s_idx[kSectionIndexSlots];
    __shared__ uint32_t s_wave[kBuildBlock / 64];
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const octpt_section sec = secs[s];
    if (tid == 0u) {
        keys[s] = morton(sec.x, sec.y, sec.z);
        ids[s] = s;
    }
    uint32_t e = section_errors(sec, depth, palette_size, index_count);
    if (e) {  // uniform over the block
        if (tid == 0u) {
            atomicOr(err, e);
            counts[s] = 0u;
        }
        return;
    }
    if (sec.index_first == OCTPT_SECTION_UNIFORM) {  // 0 or 4096 cells, no index read
        if (tid == 0u) {
            const uint32_t v = palette[sec.palette_first];
            e = value_errors(v, block_count);
            if (e) atomicOr(err, e);
            counts[s] = v ? kSectionCells : 0u;
        }
        return;
    }
    for (uint32_t i = tid; i < sec.palette_count; i += kBuildBlock) {
        const uint32_t v = palette[sec.palette_first + i];
        e |= value_errors(v, block_count);
        s_pal[i] = v;
    }
    stage_indices(indices + sec.index_first, aligned, s_idx);
    __syncthreads();
    uint32_t n = 0u;  // the wave's non-air cells (the same in every lane)
#pragma unroll
    for (uint32_t k = 0; k < kSectionCells / kBuildBlock; ++k) {
        const uint32_t idx = s_idx[index_slot(k * kBuildBlock + tid)];
        const bool ok = idx < sec.palette_count;
        if (!ok) e |= kCellErrPaletteIndex;
        const bool solid = ok && s_pal[ok ? idx : 0u] != 0u;
        n += (uint32_t)__popcll(__ballot(solid));
    }
    if (e) atomicOr(err, e);
    if ((tid & 63u) == 0u) s_wave[tid >> 6] = n;
    __syncthreads();
    if (tid == 0u) counts[s] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// Order: the counts in sorted section order (entry n_sec = 0: the exclusive scan's last input); two equal
// neighbours among the sorted keys are two sections at one position
__global__ __launch_bounds__(kBuildBlock) void section_order_kernel(const uint64_t *__restrict__ keys_s,
                                                                    const uint32_t *__restrict__ ids_s,
                                                                    const uint32_t *__restrict__ counts,
                                                                    uint32_t n_sec,
                                                                    unsigned long long *__restrict__ cnt_s,
                                                                    uint32_t *__restrict__ err) {
    const uint32_t j = blockIdx.x * kBuildBlock + threadIdx.x;
    if (j > n_sec) return;
    cnt_s[j] = j < n_sec ? counts[ids_s[j]] : 0u;
    if (j > 0u && j < n_sec && keys_s[j] == keys_s[j - 1u]) atomicOr(err, kCellErrDuplicate);
}

// Emit: block j writes the cells of the j-th section in Morton order from offs[j]: code = key << 12 | m for the
// local Morton codes m in ascending order, the block value beside it.  Wave w takes m in [1024 w, 1024 w + 1024),
// 64 consecutive codes per step; a cell's rank is the wave's running count + the ballot's prefix count, and the
// waves' bases come from their totals through LDS -- no atomics.  Runs only after the count raised no error.
__global__ __launch_bounds__(kBuildBlock) void section_emit_kernel(
    const octpt_section *__restrict__ secs, const uint32_t *__restrict__ palette,
    const uint16_t *__restrict__ indices, bool aligned, const uint64_t *__restrict__ keys_s,
    const uint32_t *__restrict__ ids_s, const unsigned long long *__restrict__ offs, uint32_t n_cells,
    uint64_t *__restrict__ codes, uint32_t *__restrict__ blks) {
    __shared__ uint32_t s_pal[kSectionCells];
    __shared__ __attribute__((aligned(16))) uint16_t s_idx[kSectionIndexSlots];
    __shared__ uint32_t s_wave[kBuildBlock / 64];
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const unsigned long long base = offs[j];
    if (offs[j + 1u] == base) return;  // all air
    const octpt_section sec = secs[ids_s[j]];
    const uint64_t hi = keys_s[j] << 12;
    if (sec.index_first == OCTPT_SECTION_UNIFORM) {
        const uint32_t v = palette[sec.palette_first];
        for (uint32_t m = tid; m < kSectionCells; m += kBuildBlock) {
            const unsigned long long o = base + m;
            if (o < n_cells) {
                codes[o] = hi | m;
                blks[o] = v;
            }
        }
        return;
    }
    for (uint32_t i = tid; i < sec.palette_count; i += kBuildBlock) s_pal[i] = palette[sec.palette_first + i];
    stage_indices(indices + sec.index_first, aligned, s_idx);
    __syncthreads();
    constexpr uint32_t kSteps = kSectionCells / kBuildBlock;  // 16 steps of 64 codes per wave
    const uint32_t wave = tid >> 6, lane = tid & 63u, m0 = wave * (kSectionCells / 4u) + lane;
    uint32_t val[kSteps], rank[kSteps], run = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kSteps; ++k) {
        const uint32_t m = m0 + k * 64u;
        const uint32_t i = compact_4(m >> 1) << 8 | compact_4(m >> 2) << 4 | compact_4(m);  // y<<8 | z<<4 | x
        const uint32_t idx = s_idx[index_slot(i)];
        val[k] = idx < sec.palette_count ? s_pal[idx] : 0u;
        const unsigned long long b = __ballot(val[k] != 0u);
        rank[k] = run + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        run += (uint32_t)__popcll(b);
    }
    if (lane == 0u) s_wave[wave] = run;
    __syncthreads();
    unsigned long long o0 = base;
    for (uint32_t w = 0; w < wave; ++w) o0 += s_wave[w];
#pragma unroll
    for (uint32_t k = 0; k < kSteps; ++k) {
        const unsigned long long o = o0 + rank[k];
        if (val[k] != 0u && o < n_cells) {
            codes[o] = hi | (m0 + k * 64u);
            blks[o] = val[k];
        }
    }
}

__global__ __launch_bounds__(kBuildBlock) void leaf_heads_kernel(const uint64_t *__restrict__ codes, uint32_t n,
                                                                 uint32_t *__restrict__ head) {
    const uint32_t k = blockIdx.x * kBuildBlock + threadIdx.x;
    if (k >= n) return;
    head[k] = (k == 0u || codes[k] != codes[k - 1]) ? 1u : 0u;
}

// leaf index of pair k = inclusive scan of heads - 1
__global__ __launch_bounds__(kBuildBlock) void leaf_tables_kernel(const uint64_t *__restrict__ codes,
                                                                  const uint32_t *__restrict__ head,
                                                                  const uint32_t *__restrict__ incl, uint32_t n,
                                                                  uint32_t *__restrict__ leaf_first,
                                                                  uint64_t *__restrict__ leaf_code) {
    const uint32_t k = blockIdx.x * kBuildBlock + threadIdx.x;
    if (k >= n || !head[k]) return;
    const uint32_t l = incl[k] - 1u;
    leaf_first[l] = k;
    leaf_code[l] = codes[k];
}

// leaf_count and the number of octants leaf j opens (pre-order ids follow by an exclusive scan).
// kCells (block-value build): every cell is a leaf, leaf_code = the sorted cell codes and there are no
// leaf tables; two equal neighbours are two blocks in one cell (kCellErrDuplicate, opens nothing)
template <bool kCells>
__global__ __launch_bounds__(kBuildBlock) void leaf_count_kernel(const uint32_t *__restrict__ leaf_first,
                                                                 const uint64_t *__restrict__ leaf_code, uint32_t L,
                                                                 uint32_t n_pairs, uint32_t depth,
                                                                 uint32_t *__restrict__ leaf_count,
                                                                 uint32_t *__restrict__ opens,
                                                                 uint32_t *__restrict__ err) {
    const uint32_t j = blockIdx.x * kBuildBlock + threadIdx.x;
    if (j >= L) return;
    if (!kCells) leaf_count[j] = (j + 1u < L ? leaf_first[j + 1u] : n_pairs) - leaf_first[j];
    if (j == 0u) {
        opens[j] = depth;
    } else {
        const uint64_t d = leaf_code[j] ^ leaf_code[j - 1u];  // != 0: codes are unique
        if (kCells && d == 0ull) {
            atomicOr(err, kCellErrDuplicate);
            opens[j] = 0u;
            return;
        }
        opens[j] = (63u - (uint32_t)__clzll((long long)d)) / 3u;
    }
}

// id of the level-`level` octant containing leaf code `code`: opened by the first leaf whose
// code shares the level's prefix
__device__ inline uint32_t octant_at(const uint64_t *__restrict__ leaf_code, const uint32_t *__restrict__ base,
                                     const uint32_t *__restrict__ opens, uint32_t L, uint32_t depth, uint32_t level,
                                     uint64_t code) {
    const uint32_t sh = 3u * (depth - level);
    const uint64_t start = sh >= 64u ? 0ull : (code >> sh) << sh;
    uint32_t lo = 0u, hi = L;  // lower_bound(leaf_code, start)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (leaf_code[mid] < start) lo = mid + 1u; else hi = mid;
    }
    return base[lo] + (level - (depth - opens[lo]));
}

// kBlockValues: leaf j's payload is value[j] (its block), else its leaf table index j
template <bool kBlockValues>
__global__ __launch_bounds__(kBuildBlock) void link_kernel(const uint64_t *__restrict__ leaf_code,
                                                           const uint32_t *__restrict__ base,
                                                           const uint32_t *__restrict__ opens, uint32_t L,
                                                           uint32_t depth, const uint32_t *__restrict__ value,
                                                           uint32_t *__restrict__ child,
                                                           uint32_t *__restrict__ mask, uint32_t *__restrict__ up,
                                                           uint8_t *__restrict__ lvl) {
    const uint32_t j = blockIdx.x * kBuildBlock + threadIdx.x;
    if (j >= L) return;
    const uint64_t code = leaf_code[j];
    const uint32_t nj = opens[j], first_level = depth - nj;
    for (uint32_t t = 0; t < nj; ++t) {  // octants opened by this leaf, top down
        const uint32_t level = first_level + t, id = base[j] + t;
        if (level == 0u) continue;  // the root has no parent
        const uint32_t parent = t ? id - 1u : octant_at(leaf_code, base, opens, L, depth, level - 1u, code);
        const uint32_t c = (uint32_t)(code >> (3u * (depth - level))) & 7u;
        child[8u * parent + c] = id;
        atomicOr(&mask[parent], 1u << c);
        if (up) {  // compaction: parent slot and level
            up[id] = 8u * parent + c;
            lvl[id] = (uint8_t)level;
        }
    }
    const uint32_t p = nj ? base[j] + nj - 1u : octant_at(leaf_code, base, opens, L, depth, depth - 1u, code);
    const uint32_t c = (uint32_t)code & 7u;
    child[8u * p + c] = kBlockValues ? value[j] : j;  // leaf payload = block value / leaf table index
    atomicOr(&mask[p], (1u << c) | (1u << (c + 8u)));
}

// Compaction (OCTPT_BUILD_COMPACT), one launch per level bottom-up: a level-`level` octant whose
// eight children are leaves holding the same primitive list becomes a leaf of its parent with child
// 0's payload (Octant::is_compactable, new_octree.rs:227-233; RegionOctreeBuilder::recursive_build
// :679-690).  Parents are one level up, handled by the next launch; siblings touch distinct slots.
// up[o] = the parent slot (8 * parent + child index), lvl[o] its level; the root (level 0) stays.
// kBlockValues (C23): leaf payloads are block values and "the same" is value equality; the mask alone
// says what a leaf is (block 0 is a value like any other, and the child array is zero-filled).
template <bool kBlockValues>
__global__ __launch_bounds__(kBuildBlock) void compact_level_kernel(const uint32_t *__restrict__ up,
                                                                    const uint8_t *__restrict__ lvl, uint32_t n_oct,
                                                                    uint32_t level, const uint32_t *__restrict__ leaf_first,
                                                                    const uint32_t *__restrict__ leaf_count,
                                                                    const uint32_t *__restrict__ prims,
                                                                    uint32_t *__restrict__ child,
                                                                    uint32_t *__restrict__ mask,
                                                                    uint32_t *__restrict__ keep) {
    const uint32_t o = blockIdx.x * kBuildBlock + threadIdx.x;
    if (o == 0u || o >= n_oct) return;  // octant 0 is the root
    if (lvl[o] != level || mask[o] != 0xFFFFu) return;
    const uint32_t c0 = child[8u * o];
    if (kBlockValues) {
        for (int k = 1; k < 8; ++k)
            if (child[8u * o + k] != c0) return;
    } else {
        const uint32_t f0 = leaf_first[c0], n0 = leaf_count[c0];
        for (int k = 1; k < 8; ++k) {
            const uint32_t ck = child[8u * o + k];
            if (leaf_count[ck] != n0) return;
            const uint32_t fk = leaf_first[ck];
            for (uint32_t e = 0; e < n0; ++e)
                if (prims[fk + e] != prims[f0 + e]) return;
        }
    }
    keep[o] = 0u;
    const uint32_t slot = up[o];
    child[slot] = c0;
    atomicOr(&mask[slot >> 3], 1u << ((slot & 7u) + 8u));
}

// surviving octants in pre-order: new id = exclusive scan of keep; octant children renumbered
__global__ __launch_bounds__(kBuildBlock) void pack_compacted_kernel(const uint32_t *__restrict__ child,
                                                                     const uint32_t *__restrict__ mask,
                                                                     const uint32_t *__restrict__ keep,
                                                                     const uint32_t *__restrict__ new_id, uint32_t n,
                                                                     octpt_octant *__restrict__ out) {
    const uint32_t o = blockIdx.x * kBuildBlock + threadIdx.x;
    if (o >= n || !keep[o]) return;
    octpt_octant v;
    const uint32_t m = mask[o];
    v.child_mask = (uint16_t)m;
    v.reserved = 0;
    for (int c = 0; c < 8; ++c) {
        const uint32_t x = child[8u * o + c];
        v.children[c] = ((m >> c) & 1u) && !((m >> (c + 8)) & 1u) ? new_id[x] : x;
    }
    out[new_id[o]] = v;
}

// keep[i] = 1 for i < n_ones, 0 for the scan's trailing entry
__global__ __launch_bounds__(kBuildBlock) void fill_u32_kernel(uint32_t *__restrict__ a, uint32_t n, uint32_t n_ones) {
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i < n) a[i] = i < n_ones ? 1u : 0u;
}

__global__ __launch_bounds__(kBuildBlock) void pack_octants_kernel(const uint32_t *__restrict__ child,
                                                                   const uint32_t *__restrict__ mask, uint32_t n,
                                                                   octpt_octant *__restrict__ out) {
    const uint32_t o = blockIdx.x * kBuildBlock + threadIdx.x;
    if (o >= n) return;
    octpt_octant v;
    v.child_mask = (uint16_t)mask[o];
    v.reserved = 0;
    for (int c = 0; c < 8; ++c) v.children[c] = child[8u * o + c];
    out[o] = v;
}

inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + kBuildBlock - 1) / kBuildBlock); }

// The slot map of the context's grow-only scratch (BuildScratch): a region is slots [first, end), and a cursor takes
// its region's slots in a fixed order per build, so a rebuild finds every buffer where the last one left it.
//   kBuildSlots    a builder's own buffers; its result (DeviceOctree) points into them until the next build.
//                  The emitter grid's builder (build_emitter_grid_gpu, C38) counts as a build: it takes these slots
//                  for its temporaries, so a scene entry's or octpt_set_emitter_sampling's grid build ends the
//                  lifetime of an earlier DeviceOctree (the scene entries have packed theirs by then).
//                  build_octree_gpu takes up to 0..25.
//   kCellSlots     the block-value builds' part of it: 0 the uploaded input, 1 the error word, 2..5 the (Morton code,
//                  block) streams and their sorted copies, 6..8 the tail's scan, 9..16 the octants.  The section
//                  build writes its streams sorted, so it takes 2 and 4 and leaves 3 and 5 unused: its large
//                  buffers share the cell build's slots, and a context that builds both ways does not hold them
//                  twice.
//   kSectionSlots  the section build's per-section arrays (keys, ids, counts, offsets, their sort's storage)
//   kBaseSlots     slot_bases_gpu: the scene packing's child counts, slot bases and scan storage
//   kFlagSlots     fill_block_scene_gpu: the block table's slot flags
// Slots 26 and 31 are free.  The packing regions lie past kBuildSlots because they are filled while the octree in
// it is still read.
struct SlotRegion {
    int first, end;
};
constexpr SlotRegion kBuildSlots{0, 26}, kCellSlots{0, 17}, kSectionSlots{17, 25}, kBaseSlots{27, 30}, kFlagSlots{30, 31};
static_assert(kCellSlots.end <= kSectionSlots.first && kSectionSlots.end <= kBuildSlots.end &&
                  kBuildSlots.end <= kBaseSlots.first && kBaseSlots.end <= kFlagSlots.first &&
                  kFlagSlots.end <= BuildScratch::kSlots,
              "scratch regions that are live together do not overlap");

struct ScratchCursor {
    BuildScratch &s;
    int next, end;
    ScratchCursor(BuildScratch &scratch, SlotRegion r) : s(scratch), next(r.first), end(r.end) {}
    // leaves n slots untaken, for a build that shares another's slot order but not all its buffers (the section
    // build); not bounded itself: the next get() refuses a cursor that left its region
    void skip(int n) { next += n; }
    template <class T>
    hipError_t get(T **ptr, size_t n) {
        const int k = next++;
        if (k >= end) return hipErrorInvalidValue;  // a buffer too many would alias the next region's
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        if (s.cap[k] < bytes) {
            if (s.dev[k]) (void)hipFree(s.dev[k]);
            s.dev[k] = nullptr;
            s.cap[k] = 0;
            const size_t want = (bytes + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);  // whole MiB
            const hipError_t e = hipMalloc(&s.dev[k], want);
            if (e != hipSuccess) return e;
            s.cap[k] = want;
        }
        *ptr = static_cast<T *>(s.dev[k]);
        return hipSuccess;
    }
};

}  // namespace

#define BTRY(expr)                                 \
    do {                                           \
        const hipError_t _e = (expr);              \
        if (_e != hipSuccess) return _e;           \
    } while (0)

void BuildScratch::release() {
    for (int k = 0; k < kSlots; ++k) {
        if (dev[k]) (void)hipFree(dev[k]);
        dev[k] = nullptr;
        cap[k] = 0;
    }
}

namespace {

// The octants of L Morton-sorted leaves (codes d_lcode; d_opens / d_base = the octants each leaf opens and
// their exclusive scan, n_oct = its total): link, with `compact` one merge pass per level bottom-up and the
// pre-order renumbering, and the packed octpt_octant array *d_oct; n_oct becomes the surviving count.
// kBlockValues: leaf j's payload is d_value[j] and leaves merge by value (C23); else the payload is j and
// leaves merge by primitive list (d_first / d_count / d_prims).
template <bool kBlockValues>
hipError_t octants_gpu(hipStream_t stream, ScratchCursor &pool, const uint64_t *d_lcode, const uint32_t *d_base,
                       const uint32_t *d_opens, uint32_t L, uint32_t depth, bool compact, const uint32_t *d_value,
                       const uint32_t *d_first, const uint32_t *d_count, const uint32_t *d_prims, uint32_t &n_oct,
                       octpt_octant **d_oct_out) {
    uint32_t *d_child, *d_mask, *d_up = nullptr, *d_keep = nullptr, *d_newid = nullptr;
    uint8_t *d_lvl = nullptr;
    octpt_octant *d_oct;
    BTRY(pool.get(&d_child, (size_t)n_oct * 8));
    BTRY(pool.get(&d_mask, n_oct));
    BTRY(pool.get(&d_oct, n_oct));
    if (compact) {
        BTRY(pool.get(&d_up, n_oct));
        BTRY(pool.get(&d_lvl, n_oct));
        BTRY(pool.get(&d_keep, n_oct + 1));  // entry n_oct = 0: the exclusive scan's last input
        BTRY(pool.get(&d_newid, n_oct + 1));
    }
    BTRY(hipMemsetAsync(d_child, 0, (size_t)n_oct * 8 * sizeof(uint32_t), stream));
    BTRY(hipMemsetAsync(d_mask, 0, (size_t)n_oct * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(link_kernel<kBlockValues>, dim3(blocks(L)), dim3(kBuildBlock), 0, stream, d_lcode, d_base, d_opens,
                       L, depth, d_value, d_child, d_mask, d_up, d_lvl);
    BTRY(hipGetLastError());
    if (compact) {
        // keep = 1 per octant, then one pass per level, bottom-up
        hipLaunchKernelGGL(fill_u32_kernel, dim3(blocks(n_oct + 1)), dim3(kBuildBlock), 0, stream, d_keep, n_oct + 1,
                           n_oct);
        BTRY(hipGetLastError());
        for (uint32_t level = depth - 1; level >= 1; --level) {
            hipLaunchKernelGGL(compact_level_kernel<kBlockValues>, dim3(blocks(n_oct)), dim3(kBuildBlock), 0, stream, d_up,
                               d_lvl, n_oct, level, d_first, d_count, d_prims, d_child, d_mask, d_keep);
            BTRY(hipGetLastError());
        }
        size_t id_bytes = 0;
        BTRY(hipcub::DeviceScan::ExclusiveSum(nullptr, id_bytes, d_keep, d_newid, n_oct + 1, stream));
        char *d_tmp3;
        BTRY(pool.get(&d_tmp3, id_bytes));
        BTRY(hipcub::DeviceScan::ExclusiveSum(d_tmp3, id_bytes, d_keep, d_newid, n_oct + 1, stream));
        hipLaunchKernelGGL(pack_compacted_kernel, dim3(blocks(n_oct)), dim3(kBuildBlock), 0, stream, d_child, d_mask,
                           d_keep, d_newid, n_oct, d_oct);
        BTRY(hipGetLastError());
        BTRY(hipMemcpyAsync(&n_oct, d_newid + n_oct, sizeof n_oct, hipMemcpyDeviceToHost, stream));
        BTRY(hipStreamSynchronize(stream));
    } else {
        hipLaunchKernelGGL(pack_octants_kernel, dim3(blocks(n_oct)), dim3(kBuildBlock), 0, stream, d_child, d_mask,
                           n_oct, d_oct);
        BTRY(hipGetLastError());
    }
    *d_oct_out = d_oct;
    return hipSuccess;
}

// the two events a build's kernel time is taken between
struct BuildEvents {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t create() {
        const hipError_t e = hipEventCreate(&e0);
        return e != hipSuccess ? e : hipEventCreate(&e1);
    }
    ~BuildEvents() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// The ways a build ends.  `t` is the builder's own record of what it has on the device; a build hands it out as
// *dev (the arrays stay in the scratch), or with dev == nullptr downloads the arrays into `out`.
// result_init: out's fields before the octants exist (no leaf tables until a primitive build downloads its own)
void result_init(BuiltOctree &out, uint32_t depth) {
    out.depth = depth;
    out.root = 0u;
    out.leaf_first.clear();
    out.leaf_count.clear();
    out.leaf_prims.clear();
}

// nothing to build from: a childless root, as the host builders emit
hipError_t empty_root(hipStream_t stream, ScratchCursor &pool, DeviceOctree t, BuiltOctree &out, float *ms,
                      DeviceOctree *dev) {
    if (ms) *ms = 0.0f;
    if (dev) {
        octpt_octant *d_root;
        BTRY(pool.get(&d_root, 1));
        BTRY(hipMemsetAsync(d_root, 0, sizeof(octpt_octant), stream));
        BTRY(hipStreamSynchronize(stream));
        t.octants = d_root;
        t.n_octants = 1u;
        *dev = t;
        return hipSuccess;
    }
    out.octants.assign(1, octpt_octant{0, 0, {0, 0, 0, 0, 0, 0, 0, 0}});
    return hipSuccess;
}

// the octants (and a primitive build's leaf tables) are built: the end of the timed region, the hand-over or the
// download, one synchronisation, the kernel time
hipError_t finish_build(hipStream_t stream, const BuildEvents &ev, const DeviceOctree &t, BuiltOctree &out, float *ms,
                        DeviceOctree *dev) {
    BTRY(hipEventRecord(ev.e1, stream));
    if (dev) {
        *dev = t;
    } else {
        out.octants.resize(t.n_octants);
        out.leaf_first.resize(t.n_leaves);
        out.leaf_count.resize(t.n_leaves);
        out.leaf_prims.resize(t.n_leaf_prims);
        BTRY(hipMemcpyAsync(out.octants.data(), t.octants, (size_t)t.n_octants * sizeof(octpt_octant),
                            hipMemcpyDeviceToHost, stream));
        if (t.n_leaves) {
            BTRY(hipMemcpyAsync(out.leaf_first.data(), t.leaf_first, (size_t)t.n_leaves * 4, hipMemcpyDeviceToHost, stream));
            BTRY(hipMemcpyAsync(out.leaf_count.data(), t.leaf_count, (size_t)t.n_leaves * 4, hipMemcpyDeviceToHost, stream));
            BTRY(hipMemcpyAsync(out.leaf_prims.data(), t.leaf_prims, (size_t)t.n_leaf_prims * 4, hipMemcpyDeviceToHost,
                                stream));
        }
    }
    BTRY(hipStreamSynchronize(stream));
    if (ms) BTRY(hipEventElapsedTime(ms, ev.e0, ev.e1));
    return hipSuccess;
}

}  // namespace

// Builds on `stream` into `out`, or leaves the arrays in the scratch as *dev.  too_many = the pair count exceeded
// max_pairs (nothing else is built then).
hipError_t build_octree_gpu(hipStream_t stream, BuildScratch &scratch, const octpt_sphere *spheres, uint32_t ns,
                            const octpt_cuboid *cuboids, uint32_t nc, uint32_t depth, bool compact,
                            uint64_t max_pairs, BuiltOctree &out, bool &too_many, float *ms,
                            DeviceOctree *dev) {
    too_many = false;
    const int32_t N = 1 << depth;
    const uint32_t np = ns + nc;
    ScratchCursor pool{scratch, kBuildSlots};
    BuildEvents ev;
    BTRY(ev.create());
    octpt_sphere *d_sp;
    octpt_cuboid *d_cb;
    unsigned long long *d_cnt, *d_off;
    BTRY(pool.get(&d_sp, ns));
    BTRY(pool.get(&d_cb, nc));
    BTRY(pool.get(&d_cnt, np));
    BTRY(pool.get(&d_off, np + 1));
    if (ns) BTRY(hipMemcpyAsync(d_sp, spheres, ns * sizeof(octpt_sphere), hipMemcpyHostToDevice, stream));
    if (nc) BTRY(hipMemcpyAsync(d_cb, cuboids, nc * sizeof(octpt_cuboid), hipMemcpyHostToDevice, stream));
    BTRY(hipEventRecord(ev.e0, stream));
    unsigned long long total = 0;
    if (np) {
        hipLaunchKernelGGL(count_cells_kernel, dim3(blocks(np)), dim3(kBuildBlock), 0, stream, d_sp, ns, d_cb, nc, N,
                           d_cnt);
        BTRY(hipGetLastError());
        size_t tmp_bytes = 0;
        BTRY(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_bytes, d_cnt, d_off + 1, np, stream));
        void *d_tmp;
        BTRY(pool.get(reinterpret_cast<char **>(&d_tmp), tmp_bytes));
        BTRY(hipMemsetAsync(d_off, 0, sizeof(unsigned long long), stream));
        BTRY(hipcub::DeviceScan::InclusiveSum(d_tmp, tmp_bytes, d_cnt, d_off + 1, np, stream));
        BTRY(hipMemcpyAsync(&total, d_off + np, sizeof total, hipMemcpyDeviceToHost, stream));
        BTRY(hipStreamSynchronize(stream));
    }
    if (total > max_pairs) {
        too_many = true;
        return hipSuccess;
    }
    const uint32_t n = (uint32_t)total;
    result_init(out, depth);
    DeviceOctree t;
    t.spheres = d_sp;
    t.cuboids = d_cb;
    t.ns = ns;
    t.nc = nc;
    t.depth = depth;
    if (n == 0u) return empty_root(stream, pool, t, out, ms, dev);  // empty world
    uint64_t *d_code, *d_code_s;
    uint32_t *d_prim, *d_prim_s, *d_head, *d_incl;
    BTRY(pool.get(&d_code, n));
    BTRY(pool.get(&d_code_s, n));
    BTRY(pool.get(&d_prim, n));
    BTRY(pool.get(&d_prim_s, n));
    BTRY(pool.get(&d_head, n));
    BTRY(pool.get(&d_incl, n));
    hipLaunchKernelGGL(emit_pairs_kernel, dim3(blocks(np)), dim3(kBuildBlock), 0, stream, d_sp, ns, d_cb, nc, N, d_off,
                       d_code, d_prim);
    BTRY(hipGetLastError());
    size_t sort_bytes = 0, scan_bytes = 0;
    BTRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_code, d_code_s, d_prim, d_prim_s, n, 0,
                                            (int)(3u * depth), stream));
    BTRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, d_head, d_incl, n, stream));
    char *d_tmp;
    BTRY(pool.get(&d_tmp, std::max(sort_bytes, scan_bytes)));
    BTRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, sort_bytes, d_code, d_code_s, d_prim, d_prim_s, n, 0,
                                            (int)(3u * depth), stream));
    hipLaunchKernelGGL(leaf_heads_kernel, dim3(blocks(n)), dim3(kBuildBlock), 0, stream, d_code_s, n, d_head);
    BTRY(hipGetLastError());
    BTRY(hipcub::DeviceScan::InclusiveSum(d_tmp, scan_bytes, d_head, d_incl, n, stream));
    uint32_t L = 0;
    BTRY(hipMemcpyAsync(&L, d_incl + (n - 1), sizeof L, hipMemcpyDeviceToHost, stream));
    BTRY(hipStreamSynchronize(stream));
    uint32_t *d_first, *d_count, *d_opens, *d_base;
    uint64_t *d_lcode;
    BTRY(pool.get(&d_first, L));
    BTRY(pool.get(&d_count, L));
    BTRY(pool.get(&d_opens, L + 1));  // entry L = 0: the exclusive scan's last input
    BTRY(pool.get(&d_base, L + 1));
    BTRY(pool.get(&d_lcode, L));
    BTRY(hipMemsetAsync(d_opens + L, 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL(leaf_tables_kernel, dim3(blocks(n)), dim3(kBuildBlock), 0, stream, d_code_s, d_head, d_incl, n,
                       d_first, d_lcode);
    BTRY(hipGetLastError());
    hipLaunchKernelGGL(leaf_count_kernel<false>, dim3(blocks(L)), dim3(kBuildBlock), 0, stream, d_first, d_lcode, L, n,
                       depth, d_count, d_opens, (uint32_t *)nullptr);
    BTRY(hipGetLastError());
    size_t base_bytes = 0;
    BTRY(hipcub::DeviceScan::ExclusiveSum(nullptr, base_bytes, d_opens, d_base, L + 1, stream));
    // exclusive sum over L + 1 entries: d_base[L] = octant count
    char *d_tmp2;
    BTRY(pool.get(&d_tmp2, base_bytes));
    BTRY(hipcub::DeviceScan::ExclusiveSum(d_tmp2, base_bytes, d_opens, d_base, L + 1, stream));
    uint32_t n_oct = 0;
    BTRY(hipMemcpyAsync(&n_oct, d_base + L, sizeof n_oct, hipMemcpyDeviceToHost, stream));
    BTRY(hipStreamSynchronize(stream));
    octpt_octant *d_oct;
    BTRY(octants_gpu<false>(stream, pool, d_lcode, d_base, d_opens, L, depth, compact, nullptr, d_first, d_count,
                            d_prim_s, n_oct, &d_oct));
    t.octants = d_oct;
    t.leaf_first = d_first;
    t.leaf_count = d_count;
    t.leaf_prims = d_prim_s;
    t.n_octants = n_oct;
    t.n_leaves = L;
    t.n_leaf_prims = n;
    return finish_build(stream, ev, t, out, ms, dev);
}

namespace {

// a block-value build's record of its result: no leaf tables, no primitives
DeviceOctree block_tree(uint32_t depth) {
    DeviceOctree t;
    t.depth = depth;
    return t;
}

// The tail of the block-value builds, from n >= 1 Morton-sorted (code, block) pairs: every cell is a leaf -- the
// octants it opens and equal neighbours (two blocks in one cell) -- the scan, one readback (the error word d_err[0]
// with the octant count beside it), then the octants.  d_opens / d_base: n + 1 entries; d_tmp: base_bytes, the
// scan's temporary storage.
hipError_t block_tail_gpu(hipStream_t stream, ScratchCursor &pool, const BuildEvents &ev, const uint64_t *d_code_s,
                          const uint32_t *d_blk_s, uint32_t n, uint32_t depth, bool compact, uint32_t *d_err,
                          uint32_t *d_opens, uint32_t *d_base, char *d_tmp, size_t base_bytes, BuiltOctree &out,
                          uint32_t &errors, float *ms, DeviceOctree *dev) {
    BTRY(hipMemsetAsync(d_opens + n, 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL(leaf_count_kernel<true>, dim3(blocks(n)), dim3(kBuildBlock), 0, stream, (const uint32_t *)nullptr,
                       d_code_s, n, n, depth, (uint32_t *)nullptr, d_opens, d_err);
    BTRY(hipGetLastError());
    BTRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, base_bytes, d_opens, d_base, n + 1, stream));
    BTRY(hipMemcpyAsync(d_err + 1, d_base + n, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    uint32_t head[2] = {0u, 0u};
    BTRY(hipMemcpyAsync(head, d_err, sizeof head, hipMemcpyDeviceToHost, stream));
    BTRY(hipStreamSynchronize(stream));
    if (head[0]) {
        errors = head[0];
        return hipSuccess;
    }
    uint32_t n_oct = head[1];
    octpt_octant *d_oct;
    BTRY(octants_gpu<true>(stream, pool, d_code_s, d_base, d_opens, n, depth, compact, d_blk_s, nullptr, nullptr, nullptr,
                           n_oct, &d_oct));
    DeviceOctree t = block_tree(depth);
    t.octants = d_oct;
    t.n_octants = n_oct;
    return finish_build(stream, ev, t, out, ms, dev);
}

}  // namespace

// The block-value builder (octpt_internal.h): the cell front end -- emit and radix sort -- and block_tail_gpu.
hipError_t build_block_octree_gpu(hipStream_t stream, BuildScratch &scratch, const uint32_t *cells, uint32_t n,
                                  bool cells_on_device, uint32_t depth, bool compact, uint32_t block_count,
                                  BuiltOctree &out, uint32_t &errors, float *ms, DeviceOctree *dev) {
    errors = 0u;
    ScratchCursor pool{scratch, kCellSlots};
    BuildEvents ev;
    BTRY(ev.create());
    uint32_t *d_cells, *d_err;
    BTRY(pool.get(&d_cells, cells_on_device ? 0u : (size_t)n * 4));
    BTRY(pool.get(&d_err, 2));  // the error word, and beside it the octant count (one readback)
    const uint32_t *d_in = cells;
    if (!cells_on_device) {
        if (n) BTRY(hipMemcpyAsync(d_cells, cells, (size_t)n * 16, hipMemcpyHostToDevice, stream));
        d_in = d_cells;
    }
    BTRY(hipEventRecord(ev.e0, stream));
    result_init(out, depth);
    if (n == 0u) return empty_root(stream, pool, block_tree(depth), out, ms, dev);
    uint64_t *d_code, *d_code_s;
    uint32_t *d_blk, *d_blk_s, *d_opens, *d_base;
    BTRY(pool.get(&d_code, n));
    BTRY(pool.get(&d_code_s, n));
    BTRY(pool.get(&d_blk, n));
    BTRY(pool.get(&d_blk_s, n));
    BTRY(pool.get(&d_opens, (size_t)n + 1));  // entry n = 0: the exclusive scan's last input
    BTRY(pool.get(&d_base, (size_t)n + 1));
    BTRY(hipMemsetAsync(d_err, 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL(emit_cells_kernel, dim3(blocks(n)), dim3(kBuildBlock), 0, stream, d_in, n, depth, block_count,
                       (reinterpret_cast<uintptr_t>(d_in) & 15u) == 0u, d_code, d_blk, d_err);
    BTRY(hipGetLastError());
    size_t sort_bytes = 0, base_bytes = 0;
    BTRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_code, d_code_s, d_blk, d_blk_s, n, 0,
                                            (int)(3u * depth), stream));
    BTRY(hipcub::DeviceScan::ExclusiveSum(nullptr, base_bytes, d_opens, d_base, n + 1, stream));
    char *d_tmp;
    BTRY(pool.get(&d_tmp, std::max(sort_bytes, base_bytes)));
    BTRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, sort_bytes, d_code, d_code_s, d_blk, d_blk_s, n, 0,
                                            (int)(3u * depth), stream));
    return block_tail_gpu(stream, pool, ev, d_code_s, d_blk_s, n, depth, compact, d_err, d_opens, d_base, d_tmp,
                          base_bytes, out, errors, ms, dev);
}

// The section front end (octpt_internal.h) and block_tail_gpu.  The streams come out of the emit sorted: running the
// cell build's radix sort over them anyway was measured and rejected (tools/rejected/section_sort.patch).
hipError_t build_section_octree_gpu(hipStream_t stream, BuildScratch &scratch, const octpt_section_world &world,
                                    bool on_device, uint32_t depth, bool compact, uint32_t block_count,
                                    uint64_t max_cells, BuiltOctree &out, uint32_t &errors, bool &too_many, float *ms,
                                    DeviceOctree *dev) {
    errors = 0u;
    too_many = false;
    ScratchCursor pool{scratch, kCellSlots}, small{scratch, kSectionSlots};
    BuildEvents ev;
    BTRY(ev.create());
    const uint32_t n_sec = world.section_count;
    // host arrays: one upload each into slot 0, at 16-byte aligned offsets
    const size_t sec_bytes = (size_t)n_sec * sizeof(octpt_section), pal_bytes = (size_t)world.palette_size * 4,
                 idx_bytes = (size_t)world.index_count * 2;
    const size_t pal_at = (sec_bytes + 15) & ~(size_t)15, idx_at = (pal_at + pal_bytes + 15) & ~(size_t)15;
    char *d_in;
    uint32_t *d_err;
    BTRY(pool.get(&d_in, on_device ? 0u : idx_at + idx_bytes));
    BTRY(pool.get(&d_err, 4));  // the error word, the octant count, and the 64-bit cell count (8-byte aligned)
    const octpt_section *d_secs = world.sections;
    const uint32_t *d_pal = world.palette;
    const uint16_t *d_idx = world.indices;
    if (!on_device) {
        if (sec_bytes) BTRY(hipMemcpyAsync(d_in, world.sections, sec_bytes, hipMemcpyHostToDevice, stream));
        if (pal_bytes) BTRY(hipMemcpyAsync(d_in + pal_at, world.palette, pal_bytes, hipMemcpyHostToDevice, stream));
        if (idx_bytes) BTRY(hipMemcpyAsync(d_in + idx_at, world.indices, idx_bytes, hipMemcpyHostToDevice, stream));
        d_secs = reinterpret_cast<const octpt_section *>(d_in);
        d_pal = reinterpret_cast<const uint32_t *>(d_in + pal_at);
        d_idx = reinterpret_cast<const uint16_t *>(d_in + idx_at);
    }
    BTRY(hipEventRecord(ev.e0, stream));
    result_init(out, depth);
    if (n_sec == 0u) return empty_root(stream, pool, block_tree(depth), out, ms, dev);
    // count, order
    uint64_t *d_key, *d_key_s;
    uint32_t *d_id, *d_id_s, *d_cnt;
    unsigned long long *d_cnt_s, *d_off;
    BTRY(small.get(&d_key, n_sec));
    BTRY(small.get(&d_id, n_sec));
    BTRY(small.get(&d_key_s, n_sec));
    BTRY(small.get(&d_id_s, n_sec));
    BTRY(small.get(&d_cnt, n_sec));
    BTRY(small.get(&d_cnt_s, (size_t)n_sec + 1));  // entry n_sec = 0: the exclusive scan's last input
    BTRY(small.get(&d_off, (size_t)n_sec + 1));
    const bool aligned = (reinterpret_cast<uintptr_t>(d_idx) & 15u) == 0u;
    const int key_bits = std::max(1, (int)(3u * (depth - 4u)));
    BTRY(hipMemsetAsync(d_err, 0, 4 * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(section_count_kernel, dim3(n_sec), dim3(kBuildBlock), 0, stream, d_secs, d_pal,
                       world.palette_size, d_idx, world.index_count, aligned, depth, block_count, d_key, d_id, d_cnt,
                       d_err);
    BTRY(hipGetLastError());
    size_t key_sort_bytes = 0, off_bytes = 0;
    BTRY(hipcub::DeviceRadixSort::SortPairs(nullptr, key_sort_bytes, d_key, d_key_s, d_id, d_id_s, n_sec, 0, key_bits,
                                            stream));
    BTRY(hipcub::DeviceScan::ExclusiveSum(nullptr, off_bytes, d_cnt_s, d_off, n_sec + 1, stream));
    char *d_tmp_s;
    BTRY(small.get(&d_tmp_s, std::max(key_sort_bytes, off_bytes)));
    BTRY(hipcub::DeviceRadixSort::SortPairs(d_tmp_s, key_sort_bytes, d_key, d_key_s, d_id, d_id_s, n_sec, 0, key_bits,
                                            stream));
    hipLaunchKernelGGL(section_order_kernel, dim3(blocks((uint64_t)n_sec + 1)), dim3(kBuildBlock), 0, stream, d_key_s,
                       d_id_s, d_cnt, n_sec, d_cnt_s, d_err);
    BTRY(hipGetLastError());
    BTRY(hipcub::DeviceScan::ExclusiveSum(d_tmp_s, off_bytes, d_cnt_s, d_off, n_sec + 1, stream));
    BTRY(hipMemcpyAsync(d_err + 2, d_off + n_sec, sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
    uint32_t head[4] = {0u, 0u, 0u, 0u};
    BTRY(hipMemcpyAsync(head, d_err, sizeof head, hipMemcpyDeviceToHost, stream));
    BTRY(hipStreamSynchronize(stream));
    if (head[0]) {  // nothing is emitted from a refused world
        errors = head[0];
        return hipSuccess;
    }
    const uint64_t total = (uint64_t)head[2] | (uint64_t)head[3] << 32;
    if (total > max_cells) {
        too_many = true;
        return hipSuccess;
    }
    const uint32_t n = (uint32_t)total;
    if (n == 0u) return empty_root(stream, pool, block_tree(depth), out, ms, dev);  // every cell is air
    // emit: the streams come out sorted, in the slots of the cell build's unsorted ones (its sorted copies' stay free)
    uint64_t *d_code;
    uint32_t *d_blk, *d_opens, *d_base;
    BTRY(pool.get(&d_code, n));
    pool.skip(1);
    BTRY(pool.get(&d_blk, n));
    pool.skip(1);
    BTRY(pool.get(&d_opens, (size_t)n + 1));  // entry n = 0: the exclusive scan's last input
    BTRY(pool.get(&d_base, (size_t)n + 1));
    hipLaunchKernelGGL(section_emit_kernel, dim3(n_sec), dim3(kBuildBlock), 0, stream, d_secs, d_pal, d_idx, aligned,
                       d_key_s, d_id_s, d_off, n, d_code, d_blk);
    BTRY(hipGetLastError());
    size_t base_bytes = 0;
    BTRY(hipcub::DeviceScan::ExclusiveSum(nullptr, base_bytes, d_opens, d_base, n + 1, stream));
    char *d_tmp;
    BTRY(pool.get(&d_tmp, base_bytes));
    return block_tail_gpu(stream, pool, ev, d_code, d_blk, n, depth, compact, d_err, d_opens, d_base, d_tmp, base_bytes,
                          out, errors, ms, dev);
}

// ---------------------------------------------------------------------------
// device-resident scene packing (octpt_scene_build_device): the slots octpt_scene_upload packs on
// the host (octpt_api.cpp), from a DeviceOctree, with no round trip through host memory
// ---------------------------------------------------------------------------
namespace {

// present children per octant (the exclusive scan's trailing entry n = 0)
__global__ __launch_bounds__(kBuildBlock) void slot_count_kernel(const octpt_octant *__restrict__ oct, uint32_t n,
                                                                 uint32_t *__restrict__ cnt) {
    const uint32_t o = blockIdx.x * kBuildBlock + threadIdx.x;
    if (o > n) return;
    cnt[o] = o < n ? (uint32_t)__popc(oct[o].child_mask & 0xFFu) : 0u;
}

// octant o's present children from base[o] in child order: octant child = (its base, its mask),
// single-primitive leaf = (prim id, 1), else (first list index, count); sphere-only scenes also get
// the single-sphere leaf's sphere beside the slot (leaf_sph, zero elsewhere)
__global__ __launch_bounds__(kBuildBlock) void slot_fill_kernel(const octpt_octant *__restrict__ oct, uint32_t n,
                                                                const uint32_t *__restrict__ base,
                                                                const uint32_t *__restrict__ first,
                                                                const uint32_t *__restrict__ count,
                                                                const uint32_t *__restrict__ prims,
                                                                const octpt_sphere *__restrict__ sp,
                                                                uint2 *__restrict__ child, float4 *__restrict__ leaf_sph) {
    const uint32_t o = blockIdx.x * kBuildBlock + threadIdx.x;
    if (o >= n) return;
    const octpt_octant v = oct[o];
    const uint32_t m = v.child_mask;
    uint32_t k = base[o];
    for (int i = 0; i < 8; ++i) {
        if (!((m >> i) & 1u)) continue;
        const uint32_t c = v.children[i];
        if (!((m >> (i + 8)) & 1u)) {
            child[k] = make_uint2(base[c], oct[c].child_mask);
        } else if (count[c] == 1u) {
            const uint32_t p = prims[first[c]];
            child[k] = make_uint2(p, 1u);
            if (leaf_sph) {
                const octpt_sphere s = sp[p];
                leaf_sph[k] = make_float4(s.center[0], s.center[1], s.center[2], s.radius);
            }
        } else {
            child[k] = make_uint2(first[c], count[c]);
        }
        ++k;
    }
}

// the slots of a block-value octree (C23): octant child = (its base, its mask), leaf child = (block value,
// the block's slot flags); a leaf value is < the block count (emit_cells_kernel's check)
__global__ __launch_bounds__(kBuildBlock) void block_slot_fill_kernel(const octpt_octant *__restrict__ oct, uint32_t n,
                                                                      const uint32_t *__restrict__ base,
                                                                      const uint32_t *__restrict__ bflags,
                                                                      uint2 *__restrict__ child) {
    const uint32_t o = blockIdx.x * kBuildBlock + threadIdx.x;
    if (o >= n) return;
    const octpt_octant v = oct[o];
    const uint32_t m = v.child_mask;
    uint32_t k = base[o];
    for (int i = 0; i < 8; ++i) {
        if (!((m >> i) & 1u)) continue;
        const uint32_t c = v.children[i];
        child[k++] = ((m >> (i + 8)) & 1u) ? make_uint2(c, bflags[c]) : make_uint2(base[c], oct[c].child_mask);
    }
}

__global__ __launch_bounds__(kBuildBlock) void prim_tables_kernel(const octpt_sphere *__restrict__ sp, uint32_t ns,
                                                                  const octpt_cuboid *__restrict__ cb, uint32_t nc,
                                                                  float4 *__restrict__ sph, uint32_t *__restrict__ sph_mat,
                                                                  float4 *__restrict__ cub_a, float2 *__restrict__ cub_b,
                                                                  uint32_t *__restrict__ cub_mat) {
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i < ns) {
        const octpt_sphere s = sp[i];
        sph[i] = make_float4(s.center[0], s.center[1], s.center[2], s.radius);
        sph_mat[i] = s.material;
    } else if (i < ns + nc) {
        const uint32_t c = i - ns;
        const octpt_cuboid b = cb[c];
        cub_a[c] = make_float4(b.min[0], b.min[1], b.min[2], b.max[0]);
        cub_b[c] = make_float2(b.max[1], b.max[2]);
        for (int f = 0; f < 6; ++f) cub_mat[6u * c + f] = b.face_material[f];
    }
}

}  // namespace

hipError_t slot_bases_gpu(hipStream_t stream, BuildScratch &scratch, const DeviceOctree &t, uint32_t **d_base,
                          uint32_t &n_slots) {
    ScratchCursor pool{scratch, kBaseSlots};
    const uint32_t n = t.n_octants;
    uint32_t *d_cnt;
    BTRY(pool.get(&d_cnt, n + 1));
    BTRY(pool.get(d_base, n + 1));
    hipLaunchKernelGGL(slot_count_kernel, dim3(blocks(n + 1)), dim3(kBuildBlock), 0, stream, t.octants, n, d_cnt);
    BTRY(hipGetLastError());
    size_t bytes = 0;
    BTRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_cnt, *d_base, n + 1, stream));
    char *d_tmp;
    BTRY(pool.get(&d_tmp, bytes));
    BTRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, d_cnt, *d_base, n + 1, stream));
    BTRY(hipMemcpyAsync(&n_slots, *d_base + n, sizeof n_slots, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t fill_scene_gpu(hipStream_t stream, const DeviceOctree &t, const uint32_t *d_base,
                          const ScenePrimTables &out) {
    if (t.n_octants) {
        hipLaunchKernelGGL(slot_fill_kernel, dim3(blocks(t.n_octants)), dim3(kBuildBlock), 0, stream, t.octants,
                           t.n_octants, d_base, t.leaf_first, t.leaf_count, t.leaf_prims, t.spheres, out.node_child,
                           out.leaf_sph);
        BTRY(hipGetLastError());
    }
    if (t.n_leaf_prims)
        BTRY(hipMemcpyAsync(out.leaf_prims, t.leaf_prims, (size_t)t.n_leaf_prims * 4, hipMemcpyDeviceToDevice, stream));
    if (t.ns + t.nc) {
        hipLaunchKernelGGL(prim_tables_kernel, dim3(blocks((uint64_t)t.ns + t.nc)), dim3(kBuildBlock), 0, stream,
                           t.spheres, t.ns, t.cuboids, t.nc, out.spheres, out.sphere_mat, out.cub_a, out.cub_b,
                           out.cub_mat);
        BTRY(hipGetLastError());
    }
    return hipStreamSynchronize(stream);
}

hipError_t fill_block_scene_gpu(hipStream_t stream, BuildScratch &scratch, const DeviceOctree &t,
                                const uint32_t *d_base, const uint32_t *bflags, uint32_t n_blocks, uint2 *node_child) {
    ScratchCursor pool{scratch, kFlagSlots};
    uint32_t *d_bflags;
    BTRY(pool.get(&d_bflags, n_blocks));
    BTRY(hipMemcpyAsync(d_bflags, bflags, (size_t)n_blocks * 4, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(block_slot_fill_kernel, dim3(blocks(t.n_octants)), dim3(kBuildBlock), 0, stream, t.octants,
                       t.n_octants, d_base, d_bflags, node_child);
    BTRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

// ---------------------------------------------------------------------------
// The emitter grid from a resident block-value scene's node slots.  An octant is (base, mask):
// mask bit i = child i present, bit i + 8 = it is a leaf, its slot node_child[base + rank of i] = (block, flags)
// for a leaf and the child octant's own (base, mask) else.  Every store is a plain vector store, and positions
// come from exclusive scans: no atomics.
// ---------------------------------------------------------------------------
namespace {

__device__ __forceinline__ uint32_t compact_by_2(uint64_t v) {  // part_by_2's inverse, 21 bits
    uint64_t x = v & 0x1249249249249249ULL;
    x = (x | x >> 2) & 0x10c30c30c30c30c3ULL;
    x = (x | x >> 4) & 0x100f00f00f00f00fULL;
    x = (x | x >> 8) & 0x1f0000ff0000ffULL;
    x = (x | x >> 16) & 0x1f00000000ffffULL;
    x = (x | x >> 32) & 0x1fffffULL;
    return (uint32_t)x;
}

// The walk's octant table: entry k = (base, mask | level << 16, Morton code of its corner); the root is entry 0 at
// level 0.  Level l's entries are [lo, hi); cnt[k - lo] = its octant children (cnt[hi - lo] = 0: the scan's total).
__global__ __launch_bounds__(kBuildBlock) void walk_count_kernel(const uint32_t *__restrict__ oc_mask, uint32_t lo,
                                                                 uint32_t hi, uint32_t *__restrict__ cnt) {
    const uint32_t k = lo + blockIdx.x * kBuildBlock + threadIdx.x;
    if (k > hi) return;
    const uint32_t m = k < hi ? oc_mask[k] : 0u;
    cnt[k - lo] = (uint32_t)__popc(m & ~(m >> 8) & 0xFFu);
}

// ... and its octant children, in child order, to entries hi + offs[k - lo] ..; cap = the table's size (never
// exceeded: the host compared hi + total with it)
__global__ __launch_bounds__(kBuildBlock) void walk_fill_kernel(const uint2 *__restrict__ node_child,
                                                                uint32_t *__restrict__ oc_base,
                                                                uint32_t *__restrict__ oc_mask,
                                                                uint64_t *__restrict__ oc_code, uint32_t lo, uint32_t hi,
                                                                const uint32_t *__restrict__ offs, uint32_t depth,
                                                                uint32_t cap) {
    const uint32_t k = lo + blockIdx.x * kBuildBlock + threadIdx.x;
    if (k >= hi) return;
    const uint32_t mw = oc_mask[k], m = mw & 0xFFFFu, lv = mw >> 16, base = oc_base[k];
    const uint64_t code = oc_code[k];
    const uint32_t shift = 3u * (depth - 1u - lv);
    uint32_t dst = hi + offs[k - lo], rank = 0u;
    for (uint32_t i = 0; i < 8u; ++i) {
        if (!((m >> i) & 1u)) continue;
        const uint32_t r = rank++;
        if ((m >> (i + 8u)) & 1u) continue;
        const uint2 slot = node_child[base + r];
        if (dst < cap) {
            oc_base[dst] = slot.x;
            oc_mask[dst] = (slot.y & 0xFFFFu) | ((lv + 1u) << 16);
            oc_code[dst] = code | ((uint64_t)i << shift);
        }
        ++dst;
    }
}

// emissive leaf children of table entry k (cnt[n] = 0), or with kFill their (Morton code, level) from offs[k].
// kModels (C39, OCTPT_EMITTERS_MODELS): a leaf whose block has a model with its emissive byte set is an emitter too,
// and carries kModelRecord | model in place of its level: the record's fourth word, through the sort.
constexpr uint32_t kModelRecord = 0x80000000u;
template <bool kFill, bool kModels>
__global__ __launch_bounds__(kBuildBlock) void leaf_emitters_kernel(const uint2 *__restrict__ node_child,
                                                                    const uint32_t *__restrict__ oc_base,
                                                                    const uint32_t *__restrict__ oc_mask,
                                                                    const uint64_t *__restrict__ oc_code, uint32_t n,
                                                                    const uint32_t *__restrict__ emissive,
                                                                    uint32_t n_blocks, uint32_t depth,
                                                                    uint32_t *__restrict__ cnt,
                                                                    const uint32_t *__restrict__ offs,
                                                                    uint64_t *__restrict__ keys,
                                                                    uint32_t *__restrict__ levels, uint32_t n_keys,
                                                                    const uint32_t *__restrict__ blk_model,
                                                                    const uint8_t *__restrict__ model_emissive,
                                                                    uint32_t n_models) {
    const uint32_t k = blockIdx.x * kBuildBlock + threadIdx.x;
    if (k > n || (kFill && k == n)) return;
    uint32_t found = 0u;
    if (k < n) {
        const uint32_t mw = oc_mask[k], m = mw & 0xFFFFu, lv = mw >> 16, base = oc_base[k];
        const uint32_t shift = 3u * (depth - 1u - lv);
        uint32_t rank = 0u;
        for (uint32_t i = 0; i < 8u; ++i) {
            if (!((m >> i) & 1u)) continue;
            const uint32_t r = rank++;
            if (!((m >> (i + 8u)) & 1u)) continue;
            const uint32_t block = node_child[base + r].x;
            if (block >= n_blocks) continue;
            uint32_t word = lv + 1u;
            if (!emissive[block]) {
                if (!kModels) continue;
                const uint32_t mdl = blk_model[block];  // (OCTPT_MODEL_NONE is no index of the table)
                if (mdl >= n_models || !model_emissive[mdl]) continue;
                word = kModelRecord | mdl;
            }
            if (kFill) {
                const uint32_t dst = offs[k] + found;
                if (dst < n_keys) {
                    keys[dst] = oc_code[k] | ((uint64_t)i << shift);
                    levels[dst] = word;
                }
            }
            ++found;
        }
    }
    if (!kFill) cnt[k] = found;
}

template <bool kModels>
__global__ __launch_bounds__(kBuildBlock) void emitter_records_kernel(const uint64_t *__restrict__ keys,
                                                                      const uint32_t *__restrict__ levels, uint32_t n,
                                                                      uint32_t depth, octpt_emitter *__restrict__ out) {
    const uint32_t k = blockIdx.x * kBuildBlock + threadIdx.x;
    if (k >= n) return;
    const uint64_t c = keys[k];
    octpt_emitter e;
    e.x = compact_by_2(c);
    e.y = compact_by_2(c >> 1);
    e.z = compact_by_2(c >> 2);
    const uint32_t word = levels[k];
    e.s = (kModels && (word & kModelRecord)) ? word : 1u << (depth - word);
    out[k] = e;
}

// first sorted key >= code
__device__ inline uint32_t key_lower_bound(const uint64_t *__restrict__ keys, uint32_t n, uint64_t code) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < code) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// The emitters of a home cell are one run of the sorted keys: those with the cell's Morton code above bit
// 3 * gshift.  Cell c's list is the runs of its 27-neighbourhood in ascending cell code.  kFill false: cnt[c] = the
// list's length (cnt[n_cells] = 0); true: the list from first[c].
template <bool kFill>
__global__ __launch_bounds__(kBuildBlock) void grid_cells_kernel(const uint64_t *__restrict__ keys, uint32_t n_keys,
                                                                 uint32_t axis_bits, uint32_t gshift, uint32_t n_cells,
                                                                 uint32_t *__restrict__ cnt,
                                                                 const uint32_t *__restrict__ first,
                                                                 uint32_t *__restrict__ list, uint32_t n_entries) {
    const uint32_t c = blockIdx.x * kBuildBlock + threadIdx.x;
    if (c > n_cells || (kFill && c == n_cells)) return;
    if (c == n_cells) {
        cnt[c] = 0u;
        return;
    }
    const uint32_t G = 1u << axis_bits, am = G - 1u;
    const int32_t cx = (int32_t)(c & am), cy = (int32_t)((c >> axis_bits) & am), cz = (int32_t)(c >> (2u * axis_bits));
    uint32_t run_lo[27], run_n[27];
    uint32_t runs = 0u, total = 0u;
    for (int32_t dz = -1; dz <= 1; ++dz)
        for (int32_t dy = -1; dy <= 1; ++dy)
            for (int32_t dx = -1; dx <= 1; ++dx) {
                const int32_t x = cx + dx, y = cy + dy, z = cz + dz;
                if (x < 0 || y < 0 || z < 0 || x >= (int32_t)G || y >= (int32_t)G || z >= (int32_t)G) continue;
                const uint64_t mc = morton((uint32_t)x, (uint32_t)y, (uint32_t)z);
                const uint32_t lo = key_lower_bound(keys, n_keys, mc << (3u * gshift));
                const uint32_t hi = key_lower_bound(keys, n_keys, (mc + 1ull) << (3u * gshift));
                if (hi == lo) continue;
                total += hi - lo;
                if (kFill) {  // insertion by run start: the non-empty runs are disjoint, so their starts ascend with the cell code
                    uint32_t j = runs;
                    while (j > 0u && run_lo[j - 1u] > lo) {
                        run_lo[j] = run_lo[j - 1u];
                        run_n[j] = run_n[j - 1u];
                        --j;
                    }
                    run_lo[j] = lo;
                    run_n[j] = hi - lo;
                }
                ++runs;
            }
    if (!kFill) {
        cnt[c] = total;
        return;
    }
    uint32_t dst = first[c];
    for (uint32_t j = 0; j < runs; ++j)
        for (uint32_t k = 0; k < run_n[j]; ++k, ++dst)
            if (dst < n_entries) list[dst] = run_lo[j] + k;
}

hipError_t scan_u32(hipStream_t stream, char *d_tmp, size_t tmp_bytes, const uint32_t *in, uint32_t *out, uint32_t n) {
    size_t bytes = tmp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, in, out, n, stream);
}

}  // namespace

hipError_t build_emitter_grid_gpu(hipStream_t stream, BuildScratch &scratch, const DevScene &S,
                                  const uint32_t *emissive, uint32_t grid_shift, DeviceEmitterGrid &out,
                                  octpt_status &refusal, const uint8_t *model_emissive, uint32_t n_models) {
    out = DeviceEmitterGrid{};
    refusal = OCTPT_OK;
    const uint32_t depth = S.depth, axis_bits = depth - grid_shift;
    if (3ull * axis_bits > 28ull) {  // more than kMaxEmitterCells cells
        refusal = OCTPT_ERR_OOM;
        return hipSuccess;
    }
    const uint32_t n_cells = 1u << (3u * axis_bits);
    const uint32_t cap = std::max(S.n_octants, 1u);  // the walk's table: every octant once
    ScratchCursor pool{scratch, kBuildSlots};
    uint32_t *d_emissive, *oc_base, *oc_mask, *d_cnt, *d_offs;
    uint64_t *oc_code;
    const size_t n_scan = (size_t)std::max(cap, n_cells) + 1u;
    BTRY(pool.get(&d_emissive, S.n_blocks));
    const bool with_models = model_emissive != nullptr && n_models != 0u && S.blk_model != nullptr;  // C39
    uint8_t *d_model_emissive = nullptr;
    if (with_models) BTRY(pool.get(&d_model_emissive, n_models));
    BTRY(pool.get(&oc_base, cap));
    BTRY(pool.get(&oc_mask, cap));
    BTRY(pool.get(&oc_code, cap));
    BTRY(pool.get(&d_cnt, n_scan));
    BTRY(pool.get(&d_offs, n_scan));
    size_t scan_bytes = 0;
    BTRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_cnt, d_offs, (int)n_scan, stream));
    char *d_tmp;
    BTRY(pool.get(&d_tmp, scan_bytes));
    if (S.n_blocks)
        BTRY(hipMemcpyAsync(d_emissive, emissive, (size_t)S.n_blocks * 4, hipMemcpyHostToDevice, stream));
    if (with_models) BTRY(hipMemcpyAsync(d_model_emissive, model_emissive, n_models, hipMemcpyHostToDevice, stream));
    // the root, then level after level
    const uint32_t root_mask = S.root_mask & 0xFFFFu;
    const uint64_t zero = 0ull;
    BTRY(hipMemcpyAsync(oc_base, &S.root, 4, hipMemcpyHostToDevice, stream));
    BTRY(hipMemcpyAsync(oc_mask, &root_mask, 4, hipMemcpyHostToDevice, stream));
    BTRY(hipMemcpyAsync(oc_code, &zero, 8, hipMemcpyHostToDevice, stream));
    BTRY(hipStreamSynchronize(stream));  // the three words above are read from this frame
    uint32_t lo = 0u, hi = 1u;
    for (uint32_t lv = 0; lv + 1u < depth && hi > lo; ++lv) {  // an octant at level depth - 1 has leaf children only
        const uint32_t n = hi - lo;
        hipLaunchKernelGGL(walk_count_kernel, dim3(blocks((uint64_t)n + 1)), dim3(kBuildBlock), 0, stream, oc_mask, lo, hi,
                           d_cnt);
        BTRY(hipGetLastError());
        BTRY(scan_u32(stream, d_tmp, scan_bytes, d_cnt, d_offs, n + 1u));
        uint32_t total = 0u;
        BTRY(hipMemcpyAsync(&total, d_offs + n, 4, hipMemcpyDeviceToHost, stream));
        BTRY(hipStreamSynchronize(stream));
        if ((uint64_t)hi + total > cap) {
            refusal = OCTPT_ERR_INTERNAL;
            return hipSuccess;
        }
        if (total) {
            hipLaunchKernelGGL(walk_fill_kernel, dim3(blocks(n)), dim3(kBuildBlock), 0, stream, S.node_child, oc_base,
                               oc_mask, oc_code, lo, hi, d_offs, depth, cap);
            BTRY(hipGetLastError());
        }
        lo = hi;
        hi += total;
    }
    const uint32_t n_oct = hi;
    // the emissive leaves: mark and scan, emit (Morton code, level), sort
    // (the instances without model emitters are the kernels they were)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(with_models ? leaf_emitters_kernel<false, true> : leaf_emitters_kernel<false, false>),
                       dim3(blocks((uint64_t)n_oct + 1)), dim3(kBuildBlock), 0, stream,
                       S.node_child, oc_base, oc_mask, oc_code, n_oct, d_emissive, S.n_blocks, depth, d_cnt,
                       (const uint32_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, 0u, S.blk_model,
                       (const uint8_t *)d_model_emissive, n_models);
    BTRY(hipGetLastError());
    BTRY(scan_u32(stream, d_tmp, scan_bytes, d_cnt, d_offs, n_oct + 1u));
    uint32_t n_em = 0u;
    BTRY(hipMemcpyAsync(&n_em, d_offs + n_oct, 4, hipMemcpyDeviceToHost, stream));
    BTRY(hipStreamSynchronize(stream));
    if (n_em > kMaxEmitters) {
        refusal = OCTPT_ERR_OOM;
        return hipSuccess;
    }
    uint64_t *d_keys, *d_keys_s;
    uint32_t *d_lv, *d_lv_s;
    BTRY(pool.get(&d_keys, n_em));
    BTRY(pool.get(&d_keys_s, n_em));
    BTRY(pool.get(&d_lv, n_em));
    BTRY(pool.get(&d_lv_s, n_em));
    if (n_em) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(with_models ? leaf_emitters_kernel<true, true> : leaf_emitters_kernel<true, false>),
                           dim3(blocks(n_oct)), dim3(kBuildBlock), 0, stream, S.node_child,
                           oc_base, oc_mask, oc_code, n_oct, d_emissive, S.n_blocks, depth, (uint32_t *)nullptr, d_offs,
                           d_keys, d_lv, n_em, S.blk_model, (const uint8_t *)d_model_emissive, n_models);
        BTRY(hipGetLastError());
        size_t sort_bytes = 0;
        BTRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_keys, d_keys_s, d_lv, d_lv_s, n_em, 0,
                                                (int)(3u * depth), stream));
        char *d_sort;
        BTRY(pool.get(&d_sort, sort_bytes));
        BTRY(hipcub::DeviceRadixSort::SortPairs(d_sort, sort_bytes, d_keys, d_keys_s, d_lv, d_lv_s, n_em, 0,
                                                (int)(3u * depth), stream));
    }
    // count the 27-neighbourhood per cell, scan into cell_first, fill
    DeviceEmitterGrid g;
    auto drop = [&](hipError_t e) {
        if (g.cell_first) (void)hipFree(g.cell_first);
        if (g.cell_emitters) (void)hipFree(g.cell_emitters);
        if (g.emitters) (void)hipFree(g.emitters);
        return e;
    };
#define GTRY(expr)                                   \
    do {                                             \
        const hipError_t _e = (expr);                \
        if (_e != hipSuccess) return drop(_e);       \
    } while (0)
    GTRY(hipMalloc(&g.cell_first, ((size_t)n_cells + 1u) * 4));
    GTRY(hipMalloc(&g.emitters, std::max<size_t>(n_em, 1) * sizeof(octpt_emitter)));
    hipLaunchKernelGGL(grid_cells_kernel<false>, dim3(blocks((uint64_t)n_cells + 1)), dim3(kBuildBlock), 0, stream,
                       d_keys_s, n_em, axis_bits, grid_shift, n_cells, d_cnt, (const uint32_t *)nullptr,
                       (uint32_t *)nullptr, 0u);
    GTRY(hipGetLastError());
    GTRY(scan_u32(stream, d_tmp, scan_bytes, d_cnt, g.cell_first, n_cells + 1u));
    uint32_t n_entries = 0u;
    GTRY(hipMemcpyAsync(&n_entries, g.cell_first + n_cells, 4, hipMemcpyDeviceToHost, stream));
    GTRY(hipStreamSynchronize(stream));
    if (n_entries > kMaxEmitterEntries) {
        refusal = OCTPT_ERR_OOM;
        return drop(hipSuccess);
    }
    GTRY(hipMalloc(&g.cell_emitters, std::max<size_t>(n_entries, 1) * 4));
    if (n_em) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(with_models ? emitter_records_kernel<true> : emitter_records_kernel<false>),
                           dim3(blocks(n_em)), dim3(kBuildBlock), 0, stream, d_keys_s, d_lv_s, n_em, depth, g.emitters);
        GTRY(hipGetLastError());
        hipLaunchKernelGGL(grid_cells_kernel<true>, dim3(blocks(n_cells)), dim3(kBuildBlock), 0, stream, d_keys_s, n_em,
                           axis_bits, grid_shift, n_cells, (uint32_t *)nullptr, g.cell_first, g.cell_emitters, n_entries);
        GTRY(hipGetLastError());
    }
    GTRY(hipStreamSynchronize(stream));
#undef GTRY
    g.n_cells = n_cells;
    g.n_entries = n_entries;
    g.n_emitters = n_em;
    g.cells_axis = 1u << axis_bits;
    g.grid_shift = grid_shift;
    out = g;
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// The sky map's distribution (csrc/octpt_sky_sample.h is its definition and the host builder's text):
//   weight    one thread per texel: the 3 x 3 maximum of the luminance times the row's factor       -> w
//   max       hipcub::DeviceReduce::Max over w (a maximum is the same in every order)               -> wmax
//   quantise  one thread per texel: q = sky_quantise(w, wmax), an integer                           -> q
//   row scan  one block per row: the inclusive sum of q along the row, 256 texels per step with the
//             block's running total carried over                                                    -> col_cdf
//   marginal  the rows' totals (col_cdf's last column) widened to 64 bits, then their inclusive sum  -> row_cdf
// Positions and sums come from scans and reductions alone; every store is a plain vector store; the sums are integer,
// so no order of addition shows in them.
namespace {

__global__ __launch_bounds__(kBuildBlock) void sky_weight_kernel(Sky K, const float *__restrict__ row,
                                                                 float *__restrict__ w, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t y = (uint32_t)(i / K.width), x = (uint32_t)(i - (uint64_t)y * K.width);
    w[i] = sky_weight(K, x, y, row[y]);
}

__global__ __launch_bounds__(kBuildBlock) void sky_quantise_kernel(const float *__restrict__ w,
                                                                   const float *__restrict__ wmax,
                                                                   uint32_t *__restrict__ q, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= n) return;
    q[i] = sky_quantise(w[i], *wmax);
}

// in place: q of row blockIdx.x becomes its inclusive sum (a row's total is at most 32768 * 65536 = 2^31)
__global__ __launch_bounds__(kBuildBlock) void sky_row_scan_kernel(uint32_t *__restrict__ q, uint32_t W) {
    using Scan = hipcub::BlockScan<uint32_t, kBuildBlock>;
    __shared__ typename Scan::TempStorage tmp;
    uint32_t *row = q + (size_t)blockIdx.x * W;
    uint32_t carry = 0u;
    for (uint32_t x0 = 0u; x0 < W; x0 += kBuildBlock) {  // (block-uniform trip count)
        const uint32_t x = x0 + threadIdx.x;
        const uint32_t v = x < W ? row[x] : 0u;
        uint32_t incl, sum;
        Scan(tmp).InclusiveSum(v, incl, sum);
        if (x < W) row[x] = carry + incl;
        carry += sum;
        __syncthreads();  // tmp is used again
    }
}

__global__ __launch_bounds__(kBuildBlock) void sky_row_totals_kernel(const uint32_t *__restrict__ col_cdf, uint32_t W,
                                                                     uint32_t H, uint64_t *__restrict__ totals) {
    const uint32_t y = blockIdx.x * kBuildBlock + threadIdx.x;
    if (y >= H) return;
    totals[y] = col_cdf[(size_t)y * W + (W - 1u)];
}

__global__ __launch_bounds__(kBuildBlock) void sky_sample_kernel(Sky K, SkyDist D, const float *__restrict__ u,
                                                                 uint32_t n, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= n) return;
    const float uu[4] = {u[4u * (size_t)i], u[4u * (size_t)i + 1u], u[4u * (size_t)i + 2u], u[4u * (size_t)i + 3u]};
    SkyShot s;
    const bool ok = sky_sample_draws(D, K, uu, s);
    float o[8];
    sky_sample_pack(s, ok, o);
    for (int k = 0; k < 8; ++k) out[8u * (size_t)i + k] = o[k];
}

}  // namespace

hipError_t build_sky_distribution_gpu(hipStream_t stream, const Sky &sky, const float *row, DeviceSkyDist &out) {
    out = DeviceSkyDist{};
    const uint32_t W = sky.width, H = sky.height;
    const uint64_t n = (uint64_t)W * H;
    float *d_row = nullptr, *d_w = nullptr, *d_max = nullptr;
    uint64_t *d_tot = nullptr, *d_rowcdf = nullptr;
    uint32_t *d_col = nullptr;
    char *d_tmp = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto drop = [&](hipError_t e) {
        for (void *p : {(void *)d_row, (void *)d_w, (void *)d_max, (void *)d_tot, (void *)d_tmp})
            if (p) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (e != hipSuccess) {
            if (d_col) (void)hipFree(d_col);
            if (d_rowcdf) (void)hipFree(d_rowcdf);
        }
        return e;
    };
#define STRY(expr)                             \
    do {                                       \
        const hipError_t _e = (expr);          \
        if (_e != hipSuccess) return drop(_e); \
    } while (0)
    STRY(hipMalloc(&d_row, (size_t)H * sizeof(float)));
    STRY(hipMalloc(&d_w, n * sizeof(float)));
    STRY(hipMalloc(&d_max, sizeof(float)));
    STRY(hipMalloc(&d_tot, (size_t)H * sizeof(uint64_t)));
    STRY(hipMalloc(&d_rowcdf, (size_t)H * sizeof(uint64_t)));
    STRY(hipMalloc(&d_col, n * sizeof(uint32_t)));
    size_t max_bytes = 0, scan_bytes = 0;
    STRY(hipcub::DeviceReduce::Max(nullptr, max_bytes, d_w, d_max, (int)n, stream));
    STRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, d_tot, d_rowcdf, (int)H, stream));
    const size_t tmp_bytes = std::max<size_t>(std::max(max_bytes, scan_bytes), 1);
    STRY(hipMalloc(&d_tmp, tmp_bytes));
    STRY(hipEventCreate(&e0));
    STRY(hipEventCreate(&e1));
    STRY(hipMemcpyAsync(d_row, row, (size_t)H * sizeof(float), hipMemcpyHostToDevice, stream));
    STRY(hipEventRecord(e0, stream));
    hipLaunchKernelGGL(sky_weight_kernel, dim3(blocks(n)), dim3(kBuildBlock), 0, stream, sky, d_row, d_w, n);
    STRY(hipGetLastError());
    size_t bytes = tmp_bytes;
    STRY(hipcub::DeviceReduce::Max(d_tmp, bytes, d_w, d_max, (int)n, stream));
    hipLaunchKernelGGL(sky_quantise_kernel, dim3(blocks(n)), dim3(kBuildBlock), 0, stream, d_w, d_max, d_col, n);
    STRY(hipGetLastError());
    hipLaunchKernelGGL(sky_row_scan_kernel, dim3(H), dim3(kBuildBlock), 0, stream, d_col, W);
    STRY(hipGetLastError());
    hipLaunchKernelGGL(sky_row_totals_kernel, dim3(blocks(H)), dim3(kBuildBlock), 0, stream, d_col, W, H, d_tot);
    STRY(hipGetLastError());
    bytes = tmp_bytes;
    STRY(hipcub::DeviceScan::InclusiveSum(d_tmp, bytes, d_tot, d_rowcdf, (int)H, stream));
    STRY(hipEventRecord(e1, stream));
    uint64_t total = 0;
    STRY(hipMemcpyAsync(&total, d_rowcdf + (H - 1u), sizeof total, hipMemcpyDeviceToHost, stream));
    STRY(hipStreamSynchronize(stream));
    float ms = 0.0f;
    STRY(hipEventElapsedTime(&ms, e0, e1));
#undef STRY
    out.row_cdf = d_rowcdf;
    out.col_cdf = d_col;
    out.total = total;
    out.width = W;
    out.height = H;
    out.build_ms = ms;
    return drop(hipSuccess);
}

hipError_t launch_sky_sample(const Sky &sky, const SkyDist &dist, const float *u, uint32_t n, float *out,
                             hipStream_t stream) {
    hipLaunchKernelGGL(sky_sample_kernel, dim3(blocks(n)), dim3(kBuildBlock), 0, stream, sky, dist, u, n, out);
    return hipGetLastError();
}

}  // namespace octpt
