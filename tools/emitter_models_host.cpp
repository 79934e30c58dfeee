// emitter_models_host -- a stand-alone host program over octpt_emitter_model_table and octpt_build_emitter_grid_models
// (DESIGN.md C39), for sanitizer runs of the host builders (tests/test_emitter_models_cpu.py compiles it with
// octpt_build_host.cpp under -fsanitize=address,undefined), in the manner of tools/emitter_grid_host.cpp.
// Reads worlds from the file named by argv[1] and prints each world's table and grid:
//   in:  depth flags grid_size n_blocks n_materials n_models n_quads n_cells
//        n_blocks rows of six face materials and the model, n_materials emittances, n_models rows (first_quad
//        quad_count), n_quads rows (origin u v material), n_cells rows (x y z block)
//   out: "table <status> <n_models> <n_entries>", model_first, quad_index, cum_area (one array per line), then
//        "grid <status> <cells_per_axis> <n_cells> <n_entries> <n_emitters>" and the grid's three arrays
// Every world is also run through the count-then-fill misuses of both entries, which must write nothing.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/octpt.h"

static int fail(const char *what) {
    std::fprintf(stderr, "emitter_models_host: %s\n", what);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: emitter_models_host WORLDS");
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return fail("cannot open the worlds file");
    unsigned depth, flags, grid_size, nb, nm, nmod, nq, nc;
    while (std::fscanf(f, "%u %u %u %u %u %u %u %u", &depth, &flags, &grid_size, &nb, &nm, &nmod, &nq, &nc) == 8) {
        std::vector<octpt_block> blocks(nb);
        std::vector<octpt_material> mats(nm);
        std::vector<octpt_block_model> models(nmod);
        std::vector<octpt_quad> quads(nq);
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
        for (auto &m : models) {
            m = octpt_block_model{};
            if (std::fscanf(f, "%u %u", &m.first_quad, &m.quad_count) != 2) return fail("bad model row");
        }
        for (auto &q : quads) {
            q = octpt_quad{};
            if (std::fscanf(f, "%f %f %f %f %f %f %f %f %f %u", &q.origin[0], &q.origin[1], &q.origin[2], &q.u[0],
                            &q.u[1], &q.u[2], &q.v[0], &q.v[1], &q.v[2], &q.material) != 10)
                return fail("bad quad row");
        }
        for (auto &c : cells)
            if (std::fscanf(f, "%u", &c) != 1) return fail("bad cell row");
        const uint32_t mark = 0xA5A5A5A5u;
        // ---- the table: exact-size arrays, so that a write past any of them is the sanitizer's to report
        octpt_emitter_model_arrays t{};
        octpt_status st = octpt_emitter_model_table(models.data(), nmod, quads.data(), nq, mats.data(), nm, &t);
        if (st != OCTPT_OK) {
            std::printf("table %d 0 0\n\n\n\ngrid %d 0 0 0 0\n\n\n\n", st, st);
            continue;
        }
        std::vector<uint32_t> mfirst((size_t)t.model_count + 1, mark), qidx(t.entry_count);
        std::vector<float> cum(t.entry_count);
        uint32_t no_index = 0;
        float no_area = 0.0f;
        for (int bad = 0; bad < 4; ++bad) {  // one pointer missing, then each capacity one short
            if ((bad == 2 || bad == 3) && qidx.empty()) continue;
            octpt_emitter_model_arrays m{};
            m.model_first = mfirst.data();
            m.model_first_capacity = (uint32_t)mfirst.size() - (bad == 1 ? 1u : 0u);
            m.quad_index = bad == 0 ? nullptr : (qidx.empty() ? &no_index : qidx.data());
            m.quad_index_capacity = (uint32_t)qidx.size() - (bad == 2 ? 1u : 0u);
            m.cum_area = cum.empty() ? &no_area : cum.data();
            m.cum_area_capacity = (uint32_t)cum.size() - (bad == 3 ? 1u : 0u);
            if (octpt_emitter_model_table(models.data(), nmod, quads.data(), nq, mats.data(), nm, &m) != OCTPT_ERR_INVALID_ARG)
                return fail("table: count-then-fill misuse was not INVALID_ARG");
            for (uint32_t v : mfirst)
                if (v != mark) return fail("table: count-then-fill misuse wrote model_first");
        }
        t.model_first = mfirst.data();
        t.model_first_capacity = (uint32_t)mfirst.size();
        t.quad_index = qidx.empty() ? &no_index : qidx.data();
        t.quad_index_capacity = (uint32_t)qidx.size();
        t.cum_area = cum.empty() ? &no_area : cum.data();
        t.cum_area_capacity = (uint32_t)cum.size();
        st = octpt_emitter_model_table(models.data(), nmod, quads.data(), nq, mats.data(), nm, &t);
        std::printf("table %d %u %u\n", st, t.model_count, t.entry_count);
        for (uint32_t v : mfirst) std::printf("%u ", v);
        std::printf("\n");
        for (uint32_t v : qidx) std::printf("%u ", v);
        std::printf("\n");
        for (float v : cum) std::printf("%.9g ", v);
        std::printf("\n");
        // ---- the grid with the model emitters
        auto build = [&](octpt_emitter_grid_arrays *g) {
            return octpt_build_emitter_grid_models(cells.data(), nc, blocks.data(), nb, mats.data(), nm, models.data(), nmod,
                                                   quads.data(), nq, depth, flags, grid_size, OCTPT_EMITTERS_MODELS, g);
        };
        octpt_emitter_grid_arrays g{};
        st = build(&g);
        if (st != OCTPT_OK) {
            std::printf("grid %d 0 0 0 0\n\n\n\n", st);
            continue;
        }
        std::vector<uint32_t> first((size_t)g.cell_count + 1, mark), list(g.entry_count);
        std::vector<octpt_emitter> em(g.emitter_count);
        uint32_t no_entry = 0;
        octpt_emitter no_emitter{};
        for (int bad = 0; bad < 4; ++bad) {
            if ((bad == 2 && list.empty()) || (bad == 3 && em.empty())) continue;
            octpt_emitter_grid_arrays m{};
            m.cell_first = first.data();
            m.cell_first_capacity = (uint32_t)first.size() - (bad == 1 ? 1u : 0u);
            m.cell_emitters = bad == 0 ? nullptr : (list.empty() ? &no_entry : list.data());
            m.cell_emitters_capacity = (uint32_t)list.size() - (bad == 2 ? 1u : 0u);
            m.emitters = em.empty() ? &no_emitter : em.data();
            m.emitters_capacity = (uint32_t)em.size() - (bad == 3 ? 1u : 0u);
            if (build(&m) != OCTPT_ERR_INVALID_ARG) return fail("grid: count-then-fill misuse was not INVALID_ARG");
            for (uint32_t v : first)
                if (v != mark) return fail("grid: count-then-fill misuse wrote cell_first");
        }
        g.cell_first = first.data();
        g.cell_first_capacity = (uint32_t)first.size();
        g.cell_emitters = list.empty() ? &no_entry : list.data();
        g.cell_emitters_capacity = (uint32_t)list.size();
        g.emitters = em.empty() ? &no_emitter : em.data();
        g.emitters_capacity = (uint32_t)em.size();
        st = build(&g);
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
