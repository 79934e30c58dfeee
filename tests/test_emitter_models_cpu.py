"""Emissive block models as emitters on the host: octpt_emitter_model_table and
octpt_build_emitter_grid_models against the numpy restatement of tests/emitter_models_ref.py, their refusals, the
sample entry against float64, and a stand-alone program over the same worlds under AddressSanitizer and UBSan
(tools/emitter_models_host.cpp; nothing is loaded into Python under a sanitizer)."""
import ctypes as C
import functools
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import emitter_models_ref as M
from tests import emitter_ref as E

ROOT = Path(__file__).resolve().parents[1]
INVALID_ARG = 1
GRID_SIZES = (1, 4, 32)


@functools.lru_cache(maxsize=None)
def _world(seed):
    return M.random_world(seed)


@functools.lru_cache(maxsize=None)
def _ref(seed, grid_size, compact):
    return M.grid(M.make_scene(_world(seed)), M.DEPTH, grid_size, compact)


def test_model_table_equals_the_definition():
    """A table with the torch, a model without an emissive quad, one with zero-area quads beside a real one, one of
    mixed materials and one whose only emissive quad has no area: exactly the restatement's, f32 sums included."""
    from octree_pathtracing_amd import scene as S

    sc = M.make_scene([])
    got, want = S.emitter_model_table(sc), M.model_table(sc)
    M.assert_same_table(got, want)
    first = want["model_first"].tolist()
    assert first == [0, 5, 5, 6, 8, 8]  # torch 5, dull 0, zero-area 1 of 3, mixed 2 of 5, only-zero 0
    assert want["quad_index"].tolist() == [0, 1, 2, 3, 4, 8, 11, 13]
    # the torch's areas are exact in f32: four sides of 20/256, the top 4/256
    assert got["cum_area"][:5].tolist() == [20 / 256, 40 / 256, 60 / 256, 80 / 256, 84 / 256]
    assert got["cum_area"][7] > got["cum_area"][6] == 1.0  # the mixed model's running sum starts again


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("grid_size", GRID_SIZES)
@pytest.mark.parametrize("seed", range(M.RANDOM_WORLDS))
def test_host_grid_with_models_equals_the_definition(seed, grid_size, compact):
    from octree_pathtracing_amd import scene as S

    sc = M.make_scene(_world(seed))
    got = S.build_emitter_grid(sc, M.DEPTH, grid_size, compact=compact, models=True)
    want = _ref(seed, grid_size, compact)
    E.assert_same_grid(got, want)
    s = want["emitters"][:, 3]
    assert (s & M.MODEL_BIT).any() and (~s & M.MODEL_BIT).any()  # both kinds
    assert set((s[(s & M.MODEL_BIT) != 0] & 0x7FFFFFFF).tolist()) <= {M.M_TORCH, M.M_ZERO_AREA, M.M_MIXED}
    if compact:  # the 2^3 groups are one leaf each: a model emitter of a level above the voxels, a cube of side 2
        rows = want["emitters"].tolist()
        assert [4, 8, 12, M.MODEL_BIT | M.M_TORCH] in rows and [20, 2, 6, 2] in rows
        assert [5, 8, 12, M.MODEL_BIT | M.M_TORCH] not in rows


@pytest.mark.parametrize("compact", [False, True])
def test_flag_off_is_the_old_builder(compact):
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S

    lib = _lib.load()
    for seed in range(3):
        sc = M.make_scene(_world(seed))
        cells, blocks, mats = sc.cells_array(), sc.block_structs(), sc.material_structs()

        def call(g):
            # flag 0: the model and quad tables are not read (NULL)
            _lib.check(lib, None, lib.octpt_build_emitter_grid_models(
                cells.ctypes.data_as(C.c_void_p), len(cells), C.cast(blocks, C.c_void_p), len(sc.blocks),
                C.cast(mats, C.c_void_p), len(sc.materials), None, 0, None, 0, M.DEPTH,
                _lib.BUILD_COMPACT if compact else 0, 4, 0, C.byref(g)))

        new = S.take_emitter_grid(call)
        old = S.build_emitter_grid(sc, M.DEPTH, 4, compact=compact)
        E.assert_same_grid(new, old)
        E.assert_same_grid(old, M.grid(sc, M.DEPTH, 4, compact, models=False))
        assert not (old["emitters"][:, 3] & M.MODEL_BIT).any()


def _table_call(sc, arrays, models=None, n_models=None, n_quads=None, nm=None):
    from octree_pathtracing_amd import _lib

    lib = _lib.load()
    mdl = sc.model_structs() if models is None else models
    quads, mats = np.ascontiguousarray(sc.quads), sc.material_structs()
    return lib.octpt_emitter_model_table(C.cast(mdl, C.c_void_p), len(sc.models) if n_models is None else n_models,
                                         quads.ctypes.data_as(C.c_void_p), len(quads) if n_quads is None else n_quads,
                                         C.cast(mats, C.c_void_p), len(sc.materials) if nm is None else nm,
                                         C.byref(arrays) if arrays is not None else None)


def test_table_refusals_write_nothing():
    from octree_pathtracing_amd import _lib

    sc = M.make_scene([])
    fresh = _lib.EmitterModelArrays
    assert _table_call(sc, None) == INVALID_ARG
    # a quad material outside the material table, a model whose quad range leaves the quad table
    for kw in ({"nm": 2}, {"n_quads": 10}):
        t = fresh()
        t.model_count = t.entry_count = 77
        assert _table_call(sc, t, **kw) == INVALID_ARG, kw
        assert (t.model_count, t.entry_count) == (0, 0)
    over = (_lib.BlockModel * 1)(_lib.BlockModel(0, 0xFFFFFFFF, 2, 0))  # first + count wraps in 32 bits
    assert _table_call(sc, fresh(), models=over, n_models=1) == INVALID_ARG
    # count-then-fill misuse
    t = fresh()
    assert _table_call(sc, t) == 0 and (t.model_count, t.entry_count) == (5, 8)
    first = np.full(6, 0xA5A5A5A5, np.uint32)
    quad = np.full(8, 0xA5A5A5A5, np.uint32)
    cum = np.full(8, 7.0, np.float32)
    for missing, short in ((0, None), (1, None), (2, None), (None, 0), (None, 1), (None, 2)):
        m = fresh()
        ptrs, caps = [first.ctypes.data, quad.ctypes.data, cum.ctypes.data], [6, 8, 8]
        if missing is not None:
            ptrs[missing] = None
        if short is not None:
            caps[short] -= 1
        m.model_first, m.quad_index, m.cum_area = ptrs
        m.model_first_capacity, m.quad_index_capacity, m.cum_area_capacity = caps
        assert _table_call(sc, m) == INVALID_ARG, (missing, short)
        assert (m.model_count, m.entry_count) == (5, 8)  # the counts still arrive
        assert (first == 0xA5A5A5A5).all() and (quad == 0xA5A5A5A5).all() and (cum == 7.0).all()


def test_grid_refusals_write_nothing():
    from octree_pathtracing_amd import _lib

    lib = _lib.load()
    sc = M.make_scene(_world(0))
    cells, blocks, mats = sc.cells_array(), sc.block_structs(), sc.material_structs()
    mdl, quads = sc.model_structs(), np.ascontiguousarray(sc.quads)

    def call(g, emitter_flags=1, n_models=len(sc.models), n_quads=len(quads), nm=len(sc.materials), models=mdl):
        return lib.octpt_build_emitter_grid_models(
            cells.ctypes.data_as(C.c_void_p), len(cells), C.cast(blocks, C.c_void_p), len(sc.blocks),
            C.cast(mats, C.c_void_p), nm, C.cast(models, C.c_void_p) if models is not None else None, n_models,
            quads.ctypes.data_as(C.c_void_p), n_quads, M.DEPTH, 0, 4, emitter_flags, C.byref(g))

    # an unknown flag; a block's model outside the model table; a quad range outside the quad table; a quad material
    # outside the material table; the model table missing; more than 2^31 - 1 models
    for kw in ({"emitter_flags": 2}, {"emitter_flags": 3}, {"n_models": 2}, {"n_quads": 10}, {"nm": 2},
               {"models": None}, {"n_models": 0x80000000}):
        g = _lib.EmitterGridArrays()
        g.cell_count = g.emitter_count = 77
        assert call(g, **kw) == INVALID_ARG, kw
        assert (g.cell_count, g.entry_count, g.emitter_count, g.cells_per_axis) == (0, 0, 0, 0)
    g = _lib.EmitterGridArrays()
    assert call(g) == 0
    want = _ref(0, 4, False)
    assert (g.cell_count, g.entry_count, g.emitter_count) == (512, len(want["cell_emitters"]), len(want["emitters"]))
    first = np.full(g.cell_count + 1, 0xA5A5A5A5, np.uint32)
    lst = np.full(g.entry_count, 0xA5A5A5A5, np.uint32)
    em = np.full((g.emitter_count, 4), 0xA5A5A5A5, np.uint32)
    for missing, short in ((0, None), (1, None), (2, None), (None, 0), (None, 1), (None, 2)):
        m = _lib.EmitterGridArrays()
        ptrs, caps = [first.ctypes.data, lst.ctypes.data, em.ctypes.data], [len(first), len(lst), len(em)]
        if missing is not None:
            ptrs[missing] = None
        if short is not None:
            caps[short] -= 1
        m.cell_first, m.cell_emitters, m.emitters = ptrs
        m.cell_first_capacity, m.cell_emitters_capacity, m.emitters_capacity = caps
        assert call(m) == INVALID_ARG, (missing, short)
        assert (first == 0xA5A5A5A5).all() and (lst == 0xA5A5A5A5).all() and (em == 0xA5A5A5A5).all()


@pytest.mark.parametrize("seed,grid_size,compact", [(0, 4, False), (1, 32, False), (2, 4, True), (3, 1, False)])
def test_sample_against_float64(seed, grid_size, compact):
    """octpt_emitter_sample_models against the float64 restatement: the cell's K, the picked emitter and the picked
    quad exactly; p, dir, dist and the factor to f32 rounding -- tests/test_emitter_cpu.py's bounds (a few ulp of
    the operations of csrc/octpt_emitter.h, the target's cancellation against p bounded by the world's 32 voxels); the
    factor's product with A_m adds one rounding, inside the 1e-5.  A cube emitter must be sampled as octpt_emitter_sample
    samples it, draw for draw: on a grid without the flag both entries agree bit for bit."""
    from octree_pathtracing_amd import scene as S

    sc = M.make_scene(_world(seed))
    grid = S.build_emitter_grid(sc, M.DEPTH, grid_size, compact=compact, models=True)
    cubes = S.build_emitter_grid(sc, M.DEPTH, grid_size, compact=compact)
    table = S.emitter_model_table(sc)
    rng = np.random.default_rng(21 + seed)
    normals = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    cells = _world(seed)
    picked_model = picked_cube = 0
    quads_seen = set()
    for i in range(300):
        hit = (rng.random(3) * 32).astype(np.float32)
        if i % 3 == 0:  # beside a block of the world, so that the cell lists are not empty at small grid sizes
            hit = (np.array(cells[i % len(cells)][:3], np.float32) + (rng.random(3) * 3 - 1).astype(np.float32))
        n, st = normals[i % 6], int(rng.integers(0, 1 << 32))
        got = S.emitter_sample(grid, M.DEPTH, grid_size, hit, n, st, table=table, quads=sc.quads)
        want = M.sample_ref(grid, table, sc.quads, M.DEPTH, grid_size, hit, n, st)
        assert got["K"] == want["K"] and got["emitter"] == want["emitter"] and got["quad"] == want["quad"], (i, got, want)
        assert np.array_equal(got["p"].astype(np.float64), want["p"])
        old, new = (S.emitter_sample(cubes, M.DEPTH, grid_size, hit, n, st),
                    S.emitter_sample(cubes, M.DEPTH, grid_size, hit, n, st, table=table, quads=sc.quads))
        assert old["emitter"] == new["emitter"] and new["quad"] is None
        assert all(np.array_equal(np.float32(old[k]).view(np.uint32), np.float32(new[k]).view(np.uint32))
                   for k in ("p", "dir", "dist", "geom"))
        if want["emitter"] is None:
            assert got["dist"] == 0.0 and got["geom"] == 0.0
            continue
        if want["quad"] is None:
            picked_cube += 1
        else:
            picked_model += 1
            quads_seen.add(want["quad"])
        assert abs(got["dist"] - want["dist"]) <= 4e-6 * want["dist"] + 32 * 2.0 ** -23
        assert np.abs(got["dir"] - want["dir"]).max() <= 4e-6 + 32 * 2.0 ** -22 / want["dist"]
        # (the absolute term is |dir . n|'s, scaled by what multiplies it: 1 / max(dist^2, 1) and, for a model, A_m)
        assert abs(got["geom"] - want["geom"]) <= (want["geom"] * 1e-5 +
                                                   want["area"] * (32 * 2.0 ** -21 / want["dist"]) / max(want["dist"] ** 2, 1.0))
    assert picked_model > 20 and picked_cube > 5 and len(quads_seen) >= 5


def test_scene_and_params_defaults():
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S

    assert S.Scene().emitter_models is False
    p = _lib.EmitterParams(1, 8, 1.0)
    assert C.sizeof(p) == 32 and p.flags == 0 and _lib.EmitterParams.flags.offset == 12
    p.flags = _lib.EMITTERS_MODELS
    assert list(p.reserved) == [1, 0, 0, 0, 0]  # the first of the five words that were reserved
    assert C.sizeof(_lib.EmitterModelArrays) == 56


def test_host_builders_under_sanitizers(tmp_path):
    """The table and the grid builder in a program of its own with -fsanitize=address,undefined, over the random worlds
    of this file at every grid size, with and without compaction, count-then-fill misuse included: clean, and the arrays
    it prints are the definition's."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "emitter_models_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    f"-I{os.environ.get('ROCM_PATH', '/opt/rocm')}/include", str(ROOT / "tools" / "emitter_models_host.cpp"),
                    str(ROOT / "octree_pathtracing_amd" / "csrc" / "octpt_build_host.cpp"), "-o", str(exe)], check=True)
    cases, lines = [], []
    for seed in range(M.RANDOM_WORLDS):
        sc = M.make_scene(_world(seed))
        for gs in GRID_SIZES:
            for compact in (False, True):
                cases.append((seed, gs, compact))
                lines.append(f"{M.DEPTH} {1 if compact else 0} {gs} {len(sc.blocks)} {len(sc.materials)} "
                             f"{len(sc.models)} {len(sc.quads)} {len(sc.cells)}")
                for b in range(len(sc.blocks)):
                    lines.append(" ".join(str(int(v)) for v in sc.blocks[b]) + f" {int(sc.block_model[b])}")
                lines.append(" ".join(repr(float(np.float32(m.emittance))) for m in sc.materials))
                lines += [f"{int(a)} {int(n)}" for a, n in sc.models]
                for q in sc.quads:
                    lines.append(" ".join(repr(float(v)) for f in ("origin", "u", "v") for v in q[f]) + f" {int(q['material'])}")
                lines += [" ".join(str(int(v)) for v in row) for row in sc.cells]
    worlds = tmp_path / "worlds.txt"
    worlds.write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(worlds)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    out = run.stdout.split("\n")
    assert len(out) >= 8 * len(cases)
    table = M.model_table(M.make_scene([]))
    for k, (seed, gs, compact) in enumerate(cases):
        thead, mfirst, qidx, cum, head, first, lst, em = out[8 * k:8 * k + 8]
        assert thead.split() == ["table", "0", "5", "8"]
        M.assert_same_table({"model_first": np.array(mfirst.split(), np.uint32), "quad_index": np.array(qidx.split(), np.uint32),
                             "cum_area": np.array(cum.split(), np.float64).astype(np.float32)}, table)
        want = _ref(seed, gs, compact)
        assert head.split() == ["grid", "0", str(want["cells_per_axis"]), str(len(want["cell_first"]) - 1),
                                str(len(want["cell_emitters"])), str(len(want["emitters"]))], (seed, gs, compact)
        got = {"cells_per_axis": want["cells_per_axis"], "cell_first": np.array(first.split(), np.uint32),
               "cell_emitters": np.array(lst.split(), np.uint32),
               "emitters": np.array(em.split(), np.uint32).reshape(-1, 4)}
        E.assert_same_grid(got, want)
