// Check of octpt_resolve_map.h, the lane -> (record, LDS slot) mapping of resolve's wave-cooperative read of a grouped
// chunk's colour records (resolve_pixel_wide).  For G in {4, 16, 64} and every batch size K the kernel can be built
// with (4 at G = 4; 4, 8 or 16 above, K <= G), over one wave (one 8x8 tile) and every batch of a sample group:
//  - the K wave-wide loads of all batches read every record of the tile's span of 64 * G records exactly once, and a
//    load's 64 lanes read whole segments of K consecutive records (whole 128-B lines at K = 8);
//  - no two lanes of a batch share a staging slot, and every slot lies inside the wave's region;
//  - the lane of pixel w reads, as its k-th sample of the batch at j0, the record that item_of gives sample j0 + k of
//    the pixel (key q = group_swap(w)): ((sg * total_items + tile * 64 + q) << g) + j0 + k, relative to the span;
//  - the 16-B reads of a sample are conflict-free: in each of the four 16-lane groups a 16-B LDS read is served in
//    ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32), the 16 lanes fall on 16 distinct 16-B columns of the
//    256-B bank row.
// Host code (tests/test_resolve_map_cpu.py builds and runs this).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../octree_pathtracing_amd/csrc/octpt_resolve_map.h"

using namespace octpt;

int main() {
    static const int kGroups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                       {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                       {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                       {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    unsigned long long checks = 0, bad = 0;
    auto fail = [&](const char *what, uint32_t G, uint32_t K, uint32_t a, uint32_t b) {
        if (++bad < 10) std::printf("G=%u K=%u: %s (%u, %u)\n", G, K, what, a, b);
    };
    for (uint32_t g : {2u, 4u, 6u}) {
        const uint32_t G = 1u << g, gh = g >> 1;
        for (uint32_t K : {4u, 8u, 16u}) {
            if (K > G || (g == 2u && K != 4u)) continue;
            std::vector<uint32_t> reads(64u * G, 0u);
            for (uint32_t j0 = 0; j0 < G; j0 += K) {
                std::vector<int> owner(resolve_wave_slots(K), -1);   // slot -> record staged there
                for (uint32_t i = 0; i < K; ++i)
                    for (uint32_t lane = 0; lane < 64u; ++lane) {
                        const uint32_t rec = resolve_load_record(i, lane, K, g) + j0, slot = resolve_load_slot(i, lane, K);
                        ++checks;
                        if (rec >= 64u * G) { fail("record outside the span", G, K, i, lane); continue; }
                        ++reads[rec];
                        if (slot >= resolve_wave_slots(K)) { fail("slot outside the region", G, K, i, lane); continue; }
                        if (owner[slot] != -1) fail("two lanes share a slot", G, K, i, lane);
                        owner[slot] = (int)rec;
                        // a load's lanes read whole segments: lane and lane ^ 1 .. within K are neighbours
                        if ((lane & (K - 1u)) != 0u &&
                            rec != resolve_load_record(i, lane - 1u, K, g) + j0 + 1u)
                            fail("a segment's records are not consecutive", G, K, i, lane);
                    }
                for (uint32_t w = 0; w < 64u; ++w) {  // the lane's pixel-in-tile index (px_item & 63)
                    const uint32_t q = group_swap(w, 3u - gh, gh) & 63u;
                    if (group_swap(q, 3u - gh, 3u - gh) != w) fail("group_swap is not its own inverse pair", G, K, w, q);
                    for (uint32_t k = 0; k < K; ++k) {
                        const uint32_t slot = resolve_read_slot(q, k, K);
                        ++checks;
                        if (slot >= resolve_wave_slots(K) || owner[slot] != (int)((q << g) + j0 + k))
                            fail("a lane reads another record than its pixel's sample", G, K, w, k);
                    }
                }
                for (uint32_t k = 0; k < K; ++k)
                    for (const auto &grp : kGroups) {
                        uint32_t cols = 0u;
                        for (int lane : grp) {
                            const uint32_t q = group_swap((uint32_t)lane, 3u - gh, gh) & 63u;
                            cols |= 1u << (resolve_read_slot(q, k, K) & 15u);  // 16-B column of the 256-B bank row
                        }
                        ++checks;
                        if (cols != 0xFFFFu) fail("bank conflict in a 16-lane read group", G, K, k, cols);
                    }
            }
            for (uint32_t r = 0; r < 64u * G; ++r)
                if (reads[r] != 1u) fail("a record is not read exactly once", G, K, r, reads[r]);
        }
    }
    std::printf("resolve_map_check: %llu checks, %llu mismatches\n", checks, bad);
    return bad ? 1 : 0;
}
