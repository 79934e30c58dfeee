// octpt_resolve_map.h -- resolve's wave-cooperative read of a grouped chunk's colour records.
//
// In a chunk whose item order puts G = 1 << g samples of a pixel into one wave (item_split), the records of one 8x8
// tile and one sample group are one contiguous span of 64 * G records: the pixel with group key q (0 .. 63) owns
// records q * G .. q * G + G - 1 of it, in sample order.  A resolve wave holds the tile's 64 pixels, one per lane,
// and takes the span in batches of K samples per pixel (K a power of two, K <= G): the batch at in-group sample j0
// is the 64 segments [q * G + j0, q * G + j0 + K) of K * 16 B each.  The wave numbers the batch's 64 * K records
// r = 0 .. 64 * K - 1 segment by segment (r = q * K + k) and loads them in K wave-wide loads, lane l of load i taking
// r = i * 64 + l: 64 consecutive r are 64 / K whole segments, so at K = 8 every load reads eight whole 128-B lines and
// at K = G the load is one contiguous 1 KB.  Record r is staged in the wave's LDS region at 16-B slot
// q * (K + 1) + k -- a segment padded by one slot, so the lane that owns q reads its K samples at an odd slot stride
// and the four 16-lane groups of a 16-B LDS read each fall on 16 distinct 16-B bank columns (tools/resolve_map_check.cpp).
//
// Host-compilable: the kernel (octpt_kernels.hip, resolve_pixel_wide) and the host check share these functions.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define OCTPT_MAP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define OCTPT_MAP_FN inline
#endif

namespace octpt {

// The item order's group key (octpt_kernels.hip, item_split): group_swap swaps the two fields of the three middle
// bits of a pixel-in-tile index, which start at bit pos = 3 - g / 2 either way; low is the width of the lower one:
// 3 - g / 2 for q -> w, g / 2 for w -> q.
OCTPT_MAP_FN uint32_t group_swap(uint32_t v, uint32_t pos, uint32_t low) {
    const uint32_t mid = (v >> pos) & 7u;
    return (v & ~(7u << pos)) | ((((mid & ((1u << low) - 1u)) << (3u - low)) | (mid >> low)) << pos);
}

// samples of a pixel per batch in chunks of G >= 16 (G = 4 takes its whole run, K = 4)
#ifndef OCTPT_RESOLVE_BATCH
#define OCTPT_RESOLVE_BATCH 8
#endif
constexpr uint32_t kResolveBatch = OCTPT_RESOLVE_BATCH;
static_assert(kResolveBatch == 4u || kResolveBatch == 8u || kResolveBatch == 16u, "a power of two, at most G = 16");

// 16-B slots of one wave's staging region
OCTPT_MAP_FN constexpr uint32_t resolve_wave_slots(uint32_t K) { return 64u * (K + 1u); }

// load i (0 .. K - 1) of lane l: the record's offset in the span, for the batch at in-group sample 0 (add j0)
OCTPT_MAP_FN uint32_t resolve_load_record(uint32_t i, uint32_t lane, uint32_t K, uint32_t g) {
    const uint32_t r = i * 64u + lane;
    return ((r / K) << g) + (r & (K - 1u));
}
// ... and the slot it is staged in
OCTPT_MAP_FN uint32_t resolve_load_slot(uint32_t i, uint32_t lane, uint32_t K) {
    const uint32_t r = i * 64u + lane;
    return (r / K) * (K + 1u) + (r & (K - 1u));
}
// the slot of sample j0 + k of the pixel whose group key is q
OCTPT_MAP_FN uint32_t resolve_read_slot(uint32_t q, uint32_t k, uint32_t K) { return q * (K + 1u) + k; }

}  // namespace octpt
