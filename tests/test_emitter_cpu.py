"""The emitter grid's host builder (octpt_build_emitter_grid) against the numpy restatement of its
definition in tests/emitter_ref.py, its refusals, and a stand-alone program over the same worlds under
AddressSanitizer and UBSan (tools/emitter_grid_host.cpp; nothing is loaded into Python under a sanitizer)."""
import ctypes as C
import functools
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import emitter_ref as E

ROOT = Path(__file__).resolve().parents[1]
INVALID_ARG, OOM = 1, 2


@functools.lru_cache(maxsize=None)
def _ref(name, grid_size):
    cells, compact = E.WORLDS[name]
    return E.grid(E.make_scene(cells), E.DEPTH, grid_size, compact)


@pytest.mark.parametrize("grid_size", E.GRID_SIZES)
@pytest.mark.parametrize("name", sorted(E.WORLDS))
def test_host_grid_equals_the_definition(name, grid_size):
    from octree_pathtracing_amd import scene as S

    cells, compact = E.WORLDS[name]
    got = S.build_emitter_grid(E.make_scene(cells), E.DEPTH, grid_size, compact=compact)
    E.assert_same_grid(got, _ref(name, grid_size))


def test_the_worlds_hold_what_their_names_say():
    from octree_pathtracing_amd import scene as S

    def lib_grid(name, gs=4):
        cells, compact = E.WORLDS[name]
        return S.build_emitter_grid(E.make_scene(cells), E.DEPTH, gs, compact=compact)

    n = {name: len(lib_grid(name)["emitters"]) for name in E.WORLDS}  # the library's counts, and the reference's
    assert n == {name: len(_ref(name, 4)["emitters"]) for name in E.WORLDS}
    assert lib_grid("group_compact")["emitters"].tolist() == [[12, 4, 20, 2]]
    assert n["no_emitters"] == 0 and n["empty"] == 0 and n["corners"] == 8 and n["two_in_cell"] == 2
    assert n["group_plain"] == 8 and n["group_compact"] == 1 and n["one_face"] == 1 and n["model_block"] == 1
    assert _ref("group_compact", 4)["emitters"].tolist() == [[12, 4, 20, 2]]
    assert sorted(_ref("big_compact", 4)["emitters"][:, 3].tolist()) == [1, 8]
    # both sides of a cell border: at grid_size 4 the emitters at x = 15 and x = 16 have different home cells and
    # each other's cell lists both
    g = _ref("border", 4)
    cell = lambda x, y, z: (x // 4) + 8 * ((y // 4) + 8 * (z // 4))  # noqa: E731
    for c in (cell(15, 7, 7), cell(16, 7, 7)):
        lst = g["cell_emitters"][g["cell_first"][c]:g["cell_first"][c + 1]]
        assert {tuple(g["emitters"][k][:3]) for k in lst} >= {(15, 7, 7), (16, 7, 7)}


def _call(cells, blocks, mats, depth, flags, grid_size, arrays, nb=None, nm=None):
    from octree_pathtracing_amd import _lib

    lib = _lib.load()
    cells = np.ascontiguousarray(cells, np.uint32).reshape(-1, 4)
    return lib.octpt_build_emitter_grid(cells.ctypes.data_as(C.c_void_p) if len(cells) else None, len(cells),
                                        C.cast(blocks, C.c_void_p), len(blocks) if nb is None else nb,
                                        C.cast(mats, C.c_void_p), len(mats) if nm is None else nm, depth, flags,
                                        grid_size, C.byref(arrays) if arrays is not None else None)


def test_bad_arguments_are_invalid_and_write_nothing():
    from octree_pathtracing_amd import _lib

    sc = E.make_scene(E.WORLDS["two_in_cell"][0])
    blocks, mats = sc.block_structs(), sc.material_structs()
    fresh = _lib.EmitterGridArrays
    assert _call(sc.cells, blocks, mats, 5, 0, 4, None) == INVALID_ARG
    for depth, flags, gs in ((5, 0, 0), (5, 0, 3), (5, 0, 64), (0, 0, 1), (22, 0, 1), (5, 2, 4), (5, 8, 4)):
        g = fresh()
        g.cell_count = g.emitter_count = 77
        assert _call(sc.cells, blocks, mats, depth, flags, gs, g) == INVALID_ARG, (depth, flags, gs)
        assert (g.cell_count, g.entry_count, g.emitter_count, g.cells_per_axis) == (0, 0, 0, 0)
    # a block id outside the block table, a face material outside the material table, a cell outside the world, two
    # cells at one position
    assert _call(sc.cells, blocks, mats, 5, 0, 4, fresh(), nb=2) == INVALID_ARG
    assert _call(sc.cells, blocks, mats, 5, 0, 4, fresh(), nm=2) == INVALID_ARG
    assert _call([(32, 0, 0, E.GLOW)], blocks, mats, 5, 0, 4, fresh()) == INVALID_ARG
    assert _call([(1, 2, 3, E.GLOW), (1, 2, 3, E.STONE)], blocks, mats, 5, 0, 4, fresh()) == INVALID_ARG
    # more than 2^28 cells: depth 10 at grid_size 1
    assert _call(sc.cells, blocks, mats, 10, 0, 1, fresh()) == OOM
    # count-then-fill misuse: a pointer missing, or a capacity one short
    g = fresh()
    assert _call(sc.cells, blocks, mats, 5, 0, 4, g) == 0
    assert (g.cell_count, g.entry_count, g.emitter_count, g.cells_per_axis) == (512, 54, 2, 8)
    first = np.full(g.cell_count + 1, 0xA5A5A5A5, np.uint32)
    lst = np.full(g.entry_count, 0xA5A5A5A5, np.uint32)
    em = np.full((g.emitter_count, 4), 0xA5A5A5A5, np.uint32)
    for missing, short in ((0, None), (1, None), (2, None), (None, 0), (None, 1), (None, 2)):
        m = fresh()
        ptrs = [first.ctypes.data, lst.ctypes.data, em.ctypes.data]
        caps = [len(first), len(lst), len(em)]
        if missing is not None:
            ptrs[missing] = None
        if short is not None:
            caps[short] -= 1
        m.cell_first, m.cell_emitters, m.emitters = ptrs
        m.cell_first_capacity, m.cell_emitters_capacity, m.emitters_capacity = caps
        assert _call(sc.cells, blocks, mats, 5, 0, 4, m) == INVALID_ARG, (missing, short)
        assert m.cell_count == 512 and m.entry_count == 54 and m.emitter_count == 2  # the counts still arrive
        assert (first == 0xA5A5A5A5).all() and (lst == 0xA5A5A5A5).all() and (em == 0xA5A5A5A5).all()


@pytest.mark.parametrize("name,grid_size", [("corners", 32), ("two_in_cell", 4), ("border", 4), ("big_compact", 4),
                                            ("group_plain", 1), ("no_emitters", 4)])
def test_emitter_sample_against_float64(name, grid_size):
    """octpt_emitter_sample, the text the emitter instances compile, against the float64 restatement: the cell's K and
    the picked emitter exactly, p, dir, dist and the geometric factor to f32 rounding (a few ulp of the operations of
    csrc/octpt_emitter.h: 4e-6 relative, the target's cancellation against p bounded by the world's 32 voxels)."""
    from octree_pathtracing_amd import scene as S

    cells, compact = E.WORLDS[name]
    grid = S.build_emitter_grid(E.make_scene(cells), E.DEPTH, grid_size, compact=compact)
    rng = np.random.default_rng(11)
    normals = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    traced = 0
    for i in range(200):
        hit = (rng.random(3) * 32).astype(np.float32)
        if i % 10 == 0:
            hit = np.array(cells[i % len(cells)][:3], np.float32) if len(cells) else hit  # on a block's corner
        if i % 25 == 1:
            hit = np.array([-3.0, 40.0, 31.999998], np.float32)  # outside the world: the cell is clamped
        n, st = normals[i % 6], int(rng.integers(0, 1 << 32))
        got, want = S.emitter_sample(grid, E.DEPTH, grid_size, hit, n, st), E.emitter_sample_ref(grid, E.DEPTH, grid_size, hit, n, st)
        assert got["K"] == want["K"] and got["emitter"] == want["emitter"], (i, got, want)
        assert np.array_equal(got["p"].astype(np.float64), want["p"])
        if want["emitter"] is None:
            assert got["dist"] == 0.0 and got["geom"] == 0.0
            continue
        traced += 1
        assert abs(got["dist"] - want["dist"]) <= 4e-6 * want["dist"] + 32 * 2.0 ** -23
        assert np.abs(got["dir"] - want["dir"]).max() <= 4e-6 + 32 * 2.0 ** -22 / want["dist"]
        assert abs(got["geom"] - want["geom"]) <= want["geom"] * 1e-5 + (32 * 2.0 ** -21 / want["dist"]) / max(want["dist"] ** 2, 1.0)
    assert traced > 0 or name == "no_emitters"


def test_scene_defaults_leave_sampling_off():
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S

    sc = S.Scene()
    assert sc.emitter_sampling == _lib.EMITTERS_NONE == 0 and sc.emitter_intensity == 1.0
    assert C.sizeof(_lib.EmitterParams) == 32 and C.sizeof(_lib.EmitterGridArrays) == 64


def test_host_builder_under_sanitizers(tmp_path):
    """The host builder in a program of its own with -fsanitize=address,undefined, on every world and grid size of
    this file, count-then-fill misuse included: clean, and the arrays it prints are the definition's."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "emitter_grid_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", f"-I{os.environ.get('ROCM_PATH', '/opt/rocm')}/include", str(ROOT / "tools" / "emitter_grid_host.cpp"),
                    str(ROOT / "octree_pathtracing_amd" / "csrc" / "octpt_build_host.cpp"), "-o", str(exe)], check=True)
    cases, lines = [], []
    for name in sorted(E.WORLDS):
        cells, compact = E.WORLDS[name]
        sc = E.make_scene(cells)
        for gs in E.GRID_SIZES:
            cases.append((name, gs))
            lines.append(f"{E.DEPTH} {1 if compact else 0} {gs} {len(sc.blocks)} {len(sc.materials)} {len(sc.cells)}")
            for b in range(len(sc.blocks)):
                lines.append(" ".join(str(int(v)) for v in sc.blocks[b]) + f" {int(sc.block_model[b])}")
            lines.append(" ".join(repr(float(np.float32(m.emittance))) for m in sc.materials))
            lines += [" ".join(str(int(v)) for v in row) for row in sc.cells]
    worlds = tmp_path / "worlds.txt"
    worlds.write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(worlds)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    out = run.stdout.split("\n")
    assert len(out) >= 4 * len(cases)
    for k, (name, gs) in enumerate(cases):
        head, first, lst, em = out[4 * k:4 * k + 4]
        want = _ref(name, gs)
        assert head.split() == ["grid", "0", str(want["cells_per_axis"]), str(len(want["cell_first"]) - 1),
                                str(len(want["cell_emitters"])), str(len(want["emitters"]))], (name, gs)
        got = {"cells_per_axis": want["cells_per_axis"], "cell_first": np.array(first.split(), np.uint32),
               "cell_emitters": np.array(lst.split(), np.uint32),
               "emitters": np.array(em.split(), np.uint32).reshape(-1, 4)}
        E.assert_same_grid(got, want)
