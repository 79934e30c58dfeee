"""Section worlds without a GPU: the ctypes mirrors of octpt_section / octpt_section_world match
the C layouts, octpt_sections_to_cells equals a numpy restatement of its definition (sections in ascending Morton
code, cells in ascending local Morton code, palette value 0 = air) and refuses what the header lists, the cells of
a section build the octree the restated SectionOctantBuilder gives, and SectionWorld.from_cells round-trips.

The block configs number their blocks from 0, and palette value 0 is air: they are packed through
Scene.with_air_block() (block b becomes value b + 1)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd import scene as S
from tests import reference_builders as RB

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "octpt.h"
BAD, OOM, OK = _lib.ERR_INVALID_ARG, _lib.ERR_OOM, _lib.OK
UNIFORM = _lib.SECTION_UNIFORM

# local Morton code m -> (x, y, z) and the linear index y<<8 | z<<4 | x (new_octree.rs:838-850)
_M = np.arange(4096)
_LX = sum(((_M >> (3 * b)) & 1) << b for b in range(4))
_LY = sum(((_M >> (3 * b + 1)) & 1) << b for b in range(4))
_LZ = sum(((_M >> (3 * b + 2)) & 1) << b for b in range(4))
_LIN = (_LY << 8) | (_LZ << 4) | _LX


def world(sections, palette, indices, depth=6):
    """SectionWorld from rows (x, y, z, palette_first, palette_count, index_first)."""
    secs = np.zeros(len(sections), _lib.SECTION_DTYPE)
    for k, row in enumerate(sections):
        secs[k] = tuple(row)
    return S.SectionWorld(secs, np.asarray(palette, np.uint32), np.asarray(indices, np.uint16), depth)


def np_cells(w):
    """The definition of octpt_sections_to_cells, restated."""
    secs = sorted(w.sections.tolist(), key=lambda s: RB.encode_morton(s[0], s[1], s[2]))
    out = [np.zeros((0, 4), np.uint32)]
    for x, y, z, pf, pc, first in secs:
        pal = w.palette[pf:pf + pc]
        val = np.full(4096, pal[0]) if first == UNIFORM else pal[w.indices[first:first + 4096][_LIN]]
        keep = val != 0
        out.append(np.stack([16 * x + _LX[keep], 16 * y + _LY[keep], 16 * z + _LZ[keep], val[keep]], 1))
    return np.concatenate(out).astype(np.uint32)


def call(w, depth=None, capacity=None, count_only=False):
    """(status, count, cells) of octpt_sections_to_cells."""
    lib = _lib.load()
    st, n = w.struct(), C.c_uint32(12345)
    depth = w.depth if depth is None else depth
    if count_only:
        return lib.octpt_sections_to_cells(C.byref(st), depth, None, 0, C.byref(n)), n.value, None
    cap = len(np_cells(w)) if capacity is None else capacity
    cells = np.full((max(cap, 1), 4), 0xABABABAB, np.uint32)
    status = lib.octpt_sections_to_cells(C.byref(st), depth, cells.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return status, n.value, cells[:cap]


def index_block(grid):
    """grid[x, y, z] of palette indices -> the 4096 indices in y<<8 | z<<4 | x order."""
    return np.ascontiguousarray(np.transpose(grid, (1, 2, 0))).reshape(-1).astype(np.uint16)


# ------------------------------------------------------------------ layouts
def test_struct_layouts(tmp_path):
    assert C.sizeof(_lib.Section) == 24 and C.sizeof(_lib.SectionWorld) == 48
    assert np.dtype(_lib.SECTION_DTYPE).itemsize == 24
    fields = {"octpt_section": (_lib.Section, ["x", "y", "z", "palette_first", "palette_count", "index_first"]),
              "octpt_section_world": (_lib.SectionWorld, ["sections", "section_count", "palette", "palette_size",
                                                          "indices", "index_count"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for c_name, (_, names) in fields.items():
        lines.append(f'    printf("{c_name} . %zu\\n", sizeof({c_name}));')
        for f in names:
            lines.append(f'    printf("{c_name} {f} %zu\\n", offsetof({c_name}, {f}));')
    lines.append("    return 0;\n}")
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                   check=True)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        name, f, value = line.split()
        mirror = fields[name][0]
        assert (C.sizeof(mirror) if f == "." else getattr(mirror, f).offset) == int(value), line
        if f != "." and name == "octpt_section":
            assert np.dtype(_lib.SECTION_DTYPE).fields[f][1] == int(value), line
        seen += 1
    assert seen == 14
    assert _lib.SECTION_UNIFORM == 0xFFFFFFFF and _lib.BUILD_SECTIONS_ON_DEVICE == 0x4


# ------------------------------------------------------------------ octpt_sections_to_cells
def _one_voxel(lx, ly, lz, value=5, pos=(1, 2, 3)):
    g = np.zeros((16, 16, 16), np.uint16)
    g[lx, ly, lz] = 1
    return world([(*pos, 0, 2, 0)], [0, value], index_block(g))


def _cases():
    rng = np.random.default_rng(11)
    cases = {"voxel-lo": _one_voxel(0, 0, 0), "voxel-hi": _one_voxel(15, 15, 15),
             "uniform-flag": world([(1, 0, 2, 0, 1, UNIFORM)], [7], []),
             "uniform-indices": world([(1, 0, 2, 0, 1, 0)], [7], np.zeros(4096, np.uint16)),
             "all-air-indices": world([(0, 0, 0, 0, 1, 0)], [0], np.zeros(4096, np.uint16)),
             "all-air-flag": world([(0, 0, 0, 0, 1, UNIFORM)], [0], []),
             "empty": world([], [], [])}
    # a palette with 0 in the middle and repeated values
    cases["zero-in-the-middle"] = world([(3, 3, 3, 0, 5, 0)], [4, 9, 0, 4, 9], rng.integers(0, 5, 4096))
    # two sections sharing one palette slice (and a third sharing an index block with the first)
    idx = rng.integers(0, 3, 2 * 4096)
    cases["shared-palette"] = world([(0, 1, 0, 1, 3, 0), (2, 1, 1, 1, 3, 4096), (1, 1, 1, 1, 3, 0)], [8, 0, 6, 2], idx)
    # sections given in shuffled order, mixed forms
    secs, pal, blocks = [], [0, 1, 2, 3], []
    pos = [(x, y, z) for x in range(4) for y in range(4) for z in range(4)]
    for k in rng.permutation(len(pos))[:24]:
        if k % 5 == 0:
            secs.append((*pos[k], 1 + k % 3, 1, UNIFORM))
        else:
            secs.append((*pos[k], 0, 4, 4096 * len(blocks)))
            blocks.append(rng.integers(0, 4, 4096) * (rng.random(4096) < (k % 7) / 6.0))
    cases["shuffled"] = world(secs, pal, np.concatenate(blocks))
    return cases


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_sections_to_cells_equals_restatement(name):
    w = CASES[name]
    want = np_cells(w)
    st, n, cells = call(w)
    assert st == OK and n == len(want)
    assert np.array_equal(cells, want), name
    st, n, _ = call(w, count_only=True)
    assert st == OK and n == len(want)
    assert np.array_equal(w.to_cells(), want)
    # ascending Morton order of the world, no air
    codes = [RB.encode_morton(*map(int, c[:3])) for c in want[:: max(1, len(want) // 512)]]
    assert codes == sorted(codes) and (len(want) == 0 or want[:, 3].min() > 0)


def test_expected_cells():
    assert np.array_equal(CASES["voxel-lo"].to_cells(), [[16, 32, 48, 5]])
    assert np.array_equal(CASES["voxel-hi"].to_cells(), [[31, 47, 63, 5]])
    a, b = CASES["uniform-flag"].to_cells(), CASES["uniform-indices"].to_cells()
    assert len(a) == 4096 and np.array_equal(a, b) and np.all(a[:, 3] == 7)
    assert np.array_equal(a[:3, :3], [[16, 0, 32], [17, 0, 32], [16, 1, 32]])  # x, then y, then z
    for name in ("all-air-indices", "all-air-flag", "empty"):
        assert len(CASES[name].to_cells()) == 0


def test_capacity_and_count_only():
    w = CASES["shared-palette"]
    n_want = len(np_cells(w))
    st, n, cells = call(w, capacity=n_want - 1)
    assert st == BAD and n == n_want and np.all(cells == 0xABABABAB)  # nothing written, the count returned
    st, n, cells = call(w, capacity=n_want + 3)
    assert st == OK and n == n_want and np.all(cells[n_want:] == 0xABABABAB)
    lib, s = _lib.load(), w.struct()
    assert lib.octpt_sections_to_cells(C.byref(s), w.depth, None, 0, None) == BAD
    assert lib.octpt_sections_to_cells(None, w.depth, None, 0, C.byref(C.c_uint32())) == BAD


def _refusals():
    air = np.zeros(4096, np.uint16)
    bad_index = air.copy()
    bad_index[4095] = 2
    return {
        "depth-3": (world([(0, 0, 0, 0, 1, 0)], [1], air), 3),
        "depth-22": (world([(0, 0, 0, 0, 1, 0)], [1], air), 22),
        "outside-x": (world([(4, 0, 0, 0, 1, 0)], [1], air), 6),
        "outside-y": (world([(0, 4, 0, 0, 1, 0)], [1], air), 6),
        "outside-z": (world([(0, 0, 1, 0, 1, 0)], [1], air), 4),
        "duplicate": (world([(1, 1, 1, 0, 1, 0), (2, 1, 1, 0, 1, 0), (1, 1, 1, 0, 1, UNIFORM)], [1], air), 6),
        "palette-past-end": (world([(0, 0, 0, 1, 2, 0)], [0, 1], air), 6),
        "palette-count-0": (world([(0, 0, 0, 0, 0, 0)], [0, 1], air), 6),
        "palette-count-4097": (world([(0, 0, 0, 0, 4097, 0)], np.ones(5000), air), 6),
        "index-first-unaligned": (world([(0, 0, 0, 0, 1, 2048)], [1], np.zeros(8192, np.uint16)), 6),
        "index-first-past-end": (world([(0, 0, 0, 0, 1, 4096)], [1], air), 6),
        "uniform-two-entries": (world([(0, 0, 0, 0, 2, UNIFORM)], [1, 2], air), 6),
        "index-ge-palette-count": (world([(0, 0, 0, 0, 2, 0)], [0, 1, 3], bad_index), 6),
        "value-2^27": (world([(0, 0, 0, 0, 2, 0)], [1, 1 << 27], air), 6),
        "value-2^27-uniform": (world([(0, 0, 0, 0, 1, UNIFORM)], [1 << 27], []), 6),
    }


REFUSALS = _refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    w, depth = REFUSALS[name]
    st, n, _ = call(w, depth=depth, count_only=True)
    assert (st, n) == (BAD, 0), name


def test_refusal_neighbours_pass():
    """The largest valid value, palette, position and the last index block pass."""
    idx = np.zeros(8192, np.uint16)
    idx[4096:] = 4095
    w = world([(3, 3, 3, 0, 4096, 4096)], np.concatenate([np.arange(1, 4096), [(1 << 27) - 1]]), idx)
    st, n, cells = call(w, capacity=4096)
    assert st == OK and n == 4096 and np.all(cells[:, 3] == (1 << 27) - 1)
    st, n, _ = call(world([((1 << 17) - 1,) * 3 + (0, 1, UNIFORM)], [3], []), depth=21, count_only=True)
    assert st == OK and n == 4096
    # index_count not a multiple of 4096
    st, n, _ = call(world([(0, 0, 0, 0, 1, 0)], [1], np.zeros(4097, np.uint16)), count_only=True)
    assert st == BAD


# ------------------------------------------------------------------ section semantics
def test_section_octree_equals_restated_section_builder():
    """One random 16^3 section, values {0, 1, 2}, with solid 8^3 and 4^3 sub-blocks: the compacted octree of its
    cells decodes to the grid and has the octant count of the restated SectionOctantBuilder."""
    rng = np.random.default_rng(3)
    grid = rng.integers(0, 3, (16, 16, 16)).astype(np.uint32)
    grid[8:16, 0:8, 8:16] = 2
    grid[0:4, 4:8, 12:16] = 1
    w = world([(0, 0, 0, 0, 3, 0)], [0, 1, 2], index_block(grid), depth=4)
    cells = w.to_cells()
    assert len(cells) == np.count_nonzero(grid)
    sc = S.Scene(blocks=np.zeros((3, 6), np.uint32), cells=cells)
    t = sc.build_octree(4, compact=True)
    for x, y, z in np.ndindex(16, 16, 16):
        assert RB.decode_cell(t.octant_mask, t.octant_children, t.root, 4, x, y, z) == grid[x, y, z], (x, y, z)
    kind, masks, _ = RB.section_octants(grid)
    assert kind == "subtree" and t.octant_count == len(masks)
    # the same octree through build_octree(sections=...) on the host
    t2 = S.Scene(blocks=np.zeros((3, 6), np.uint32)).build_octree(4, compact=True, sections=w)
    assert np.array_equal(t2.octant_mask, t.octant_mask) and np.array_equal(t2.octant_children, t.octant_children)


@pytest.mark.parametrize("name", ["blocks-b", "cap"])
@pytest.mark.parametrize("uniform", [True, False])
def test_from_cells_round_trip(name, uniform):
    sc = S.make_config(name, build=False)[0].with_air_block()
    cells = sc.cells_array()
    w = S.SectionWorld.from_cells(cells, sc._depth, uniform=uniform)
    back = w.to_cells()
    assert len(back) == len(cells)
    assert {tuple(r) for r in back.tolist()} == {tuple(r) for r in cells.tolist()}
    assert np.array_equal(back, np_cells(w))
    flagged = int(np.count_nonzero(w.sections["index_first"] == UNIFORM))
    assert flagged == 0 if not uniform else True
    assert len(w.indices) == 4096 * (len(w.sections) - flagged)
    with pytest.raises(ValueError):
        S.SectionWorld.from_cells(np.array([[0, 0, 0, 0]], np.uint32), 4)  # block 0 is air
