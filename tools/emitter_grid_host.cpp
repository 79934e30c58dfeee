// emitter_grid_host -- a stand-alone host program over octpt_build_emitter_grid, for sanitizer runs of
// the host builder (tests/test_emitter_cpu.py compiles it with octpt_build_host.cpp under -fsanitize=address,undefined).
// Reads worlds from the file named by argv[1] and prints each world's grid:
//   in:  depth flags grid_size n_blocks n_materials n_cells
//        n_blocks rows of six face materials and the model, n_materials emittances, n_cells rows (x y z block)
//   out: "grid <status> <cells_per_axis> <n_cells> <n_entries> <n_emitters>", then the three arrays, one per line
// Every world is also run through the count-then-fill misuses, which must write nothing.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/octpt.h"

static int fail(const char *what) {
    std::fprintf(stderr, "emitter_grid_host: %s\n", what);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: emitter_grid_host WORLDS");
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return fail("cannot open the worlds file");
    unsigned depth, flags, grid_size, nb, nm, nc;
    while (std::fscanf(f, "%u %u %u %u %u %u", &depth, &flags, &grid_size, &nb, &nm, &nc) == 6) {
        std::vector<octpt_block> blocks(nb);
        std::vector<octpt_material> mats(nm);
        std::vector<uint32_t> cells(4 * (size_t)nc);
        for (auto &b : blocks) {
            b.reserved = 0;
            for (int k = 0; k < 6; ++k)
                if (std::fscanf(f, "%u", &b.face_material[k]) != 1) return fail("bad block row");
            if (std::fscanf(f, "%u", &b.model) != 1) return fail("bad block row");
        }
        for (auto &m : mats) {
            m = octpt_material{};
            if (std::fscanf(f, "%f", &m.emittance) != 1) return fail("bad material");
        }
        for (auto &c : cells)
            if (std::fscanf(f, "%u", &c) != 1) return fail("bad cell row");
        octpt_emitter_grid_arrays g{};
        octpt_status st = octpt_build_emitter_grid(cells.data(), nc, blocks.data(), nb, mats.data(), nm, depth, flags,
                                                   grid_size, &g);
        if (st != OCTPT_OK) {
            std::printf("grid %d 0 0 0 0\n\n\n\n", st);
            continue;
        }
        // exact-size arrays: a write past any of them is the sanitizer's to report
        std::vector<uint32_t> first((size_t)g.cell_count + 1), list(g.entry_count);
        std::vector<octpt_emitter> em(g.emitter_count);
        // misuse: one pointer missing, then each capacity one short -- INVALID_ARG and nothing written
        const uint32_t mark = 0xA5A5A5A5u;
        uint32_t mark_entry = mark;
        octpt_emitter mark_emitter{};
        for (auto &v : first) v = mark;
        for (int bad = 0; bad < 4; ++bad) {
            octpt_emitter_grid_arrays m{};
            m.cell_first = first.data();
            m.cell_first_capacity = (uint32_t)first.size() - (bad == 1 ? 1u : 0u);
            m.cell_emitters = bad == 0 ? nullptr : (list.empty() ? &mark_entry : list.data());
            m.cell_emitters_capacity = (uint32_t)list.size() - (bad == 2 ? 1u : 0u);
            m.emitters = em.empty() ? &mark_emitter : em.data();
            m.emitters_capacity = (uint32_t)em.size() - (bad == 3 ? 1u : 0u);
            if ((bad == 2 && list.empty()) || (bad == 3 && em.empty())) continue;
            if (octpt_build_emitter_grid(cells.data(), nc, blocks.data(), nb, mats.data(), nm, depth, flags, grid_size,
                                         &m) != OCTPT_ERR_INVALID_ARG)
                return fail("count-then-fill misuse was not INVALID_ARG");
            for (uint32_t v : first)
                if (v != mark) return fail("count-then-fill misuse wrote cell_first");
        }
        // (an empty array still needs an address: the three pointers are set or the call only counts)
        uint32_t no_entry = 0;
        octpt_emitter no_emitter{};
        g.cell_first = first.data();
        g.cell_first_capacity = (uint32_t)first.size();
        g.cell_emitters = list.empty() ? &no_entry : list.data();
        g.cell_emitters_capacity = (uint32_t)list.size();
        g.emitters = em.empty() ? &no_emitter : em.data();
        g.emitters_capacity = (uint32_t)em.size();
        st = octpt_build_emitter_grid(cells.data(), nc, blocks.data(), nb, mats.data(), nm, depth, flags, grid_size, &g);
        std::printf("grid %d %u %u %u %u\n", st, g.cells_per_axis, g.cell_count, g.entry_count, g.emitter_count);
        for (uint32_t v : first) std::printf("%u ", v);
        std::printf("\n");
        for (uint32_t v : list) std::printf("%u ", v);
        std::printf("\n");
        for (const octpt_emitter &e : em) std::printf("%u %u %u %u ", e.x, e.y, e.z, e.s);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
