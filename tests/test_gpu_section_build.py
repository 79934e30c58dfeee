"""The block-value builds from 16^3 palette sections on the device.
octpt_build_block_octree_sections_device must return octpt_build_block_octree of octpt_sections_to_cells' cells,
array for array, with and without compaction, from host arrays and from arrays already on the GPU
(OCTPT_BUILD_SECTIONS_ON_DEVICE, also with 2-byte aligned indices), and refuse what the host entry refuses;
octpt_scene_build_sections_device must leave the device scene octpt_scene_upload makes from that host octree --
renders bit-identical in radiance, per-pixel segment counts and statistics, closest-hit queries identical -- also
between cell builds on one context, after an edit, and on a multi-device context.

The block configs number their blocks from 0 and palette value 0 is air: they are packed through
Scene.with_air_block() (block b becomes value b + 1)."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from tests.test_gpu_block_build import _same_shot, _same_tree, _shot
from tests.test_gpu_parity import gpu_render, renderer, torch_cuda  # noqa: F401
from tests.test_sections_cpu import index_block, world

pytestmark = pytest.mark.gpu

STAT_KEYS = ("segments", "esvo_steps", "block_tests", "shade_events", "texel_reads")
SCENES = [("blocks-b", None), ("cap", None), ("C5s-small", (160, 90, 2))]
UNIFORM = 0xFFFFFFFF


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _config(name):
    """(scene with the air block, camera, settings, its SectionWorld) of a block config."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config(name, build=False)
    sc = sc.with_air_block()
    return sc, cam, rs, S.SectionWorld.from_cells(sc.cells_array(), sc._depth)


def _voxel(lx, ly, lz, pos, depth, value=5):
    g = np.zeros((16, 16, 16), np.uint16)
    g[lx, ly, lz] = 1
    return world([(*pos, 0, 2, 0)], [0, value], index_block(g), depth)


def _eight_uniform(other=False):
    """depth 5: eight full sections of one value (the merge cascade); other: one voxel of another value."""
    secs = [(x, y, z, 0, 1, UNIFORM) for x in range(2) for y in range(2) for z in range(2)]
    if not other:
        return world(secs, [3], [], 5)
    g = np.zeros((16, 16, 16), np.uint16)
    g[5, 2, 6] = 1
    secs[5] = secs[5][:3] + (0, 2, 0)
    return world(secs, [3, 4], index_block(g), 5)


def _random_world(rng, depth=7, n=300):
    """n sections at random positions: densities 0..100 %, some uniform, some all air, shuffled, shared slices."""
    side = 1 << (depth - 4)
    pos = [(x, y, z) for x in range(side) for y in range(side) for z in range(side)]
    palette = np.concatenate([[0, 1, 2, 3, 0, 7, 7, 9], rng.integers(0, 50, 56)]).astype(np.uint32)
    secs, blocks = [], []
    for k, p in enumerate(rng.permutation(len(pos))[:n]):
        first, count = [(0, 4), (3, 5), (8, 56), (1, 1)][k % 4]  # shared slices; (1, 1): the single value 1
        kind = k % 10
        if kind == 0:
            secs.append((*pos[p], first, 1, UNIFORM))  # uniform (value 0 at slice 0: all air)
            continue
        if kind == 1:
            idx = np.zeros(4096, np.int64)  # all air through indices when the slice starts with 0
        else:
            density = (kind - 2) / 7.0
            idx = np.where(rng.random(4096) < density, rng.integers(0, count, 4096), 0)
        if kind == 9 and blocks:  # an index block shared with an earlier section (the widest slice fits any)
            secs.append((*pos[p], 8, 56, 4096 * int(rng.integers(0, len(blocks)))))
            continue
        secs.append((*pos[p], first, count, 4096 * len(blocks)))
        blocks.append(idx % count)
    return world(secs, palette, np.concatenate(blocks), depth)


@functools.lru_cache(maxsize=None)
def _case(name):
    rng = np.random.default_rng(17)
    top = (1 << 17) - 1
    if name == "empty":
        return world([], [], [], 4)
    if name == "all-air":
        return world([(1, 1, 0, 0, 1, 0), (0, 1, 0, 0, 1, UNIFORM)], [0], np.zeros(4096, np.uint16), 5)
    if name == "voxel-lo":
        return _voxel(0, 0, 0, (1, 2, 3), 6)
    if name == "voxel-hi":
        return _voxel(15, 15, 15, (1, 2, 3), 6)
    if name == "d4-uniform-flag":
        return world([(0, 0, 0, 0, 1, UNIFORM)], [6], [], 4)
    if name == "d4-uniform-indices":
        return world([(0, 0, 0, 0, 1, 0)], [6], np.zeros(4096, np.uint16), 4)
    if name == "d5-eight-uniform":
        return _eight_uniform()
    if name == "d5-eight-one-other":
        return _eight_uniform(other=True)
    if name == "d21-far-corner":  # 63-bit codes
        return _voxel(15, 15, 15, (top, top, top), 21)
    if name == "palette-4096":
        pal = rng.permutation(4096).astype(np.uint32)  # one entry is 0
        return world([(2, 0, 1, 0, 4096, 0)], pal, rng.integers(0, 4096, 4096), 6)
    if name == "d7-random-300":
        return _random_world(rng)
    return _config(name)[3]


CASES = ["empty", "all-air", "voxel-lo", "voxel-hi", "d4-uniform-flag", "d4-uniform-indices", "d5-eight-uniform",
         "d5-eight-one-other", "d21-far-corner", "palette-4096", "d7-random-300", "blocks-b", "cap", "C5s-small"]

_HOST = {}


def _cell_scene(cells=None):
    from octree_pathtracing_amd import scene as S

    return S.Scene(blocks=np.zeros((1, 6), np.uint32), cells=cells)


def _host_octree(name, compact):
    """octpt_build_block_octree of octpt_sections_to_cells' cells, once per (case, compact)."""
    if (name, compact) not in _HOST:
        w = _case(name)
        _HOST[(name, compact)] = _cell_scene(w.to_cells()).build_octree(w.depth, compact=compact)
    return _HOST[(name, compact)]


# ------------------------------------------------------------------ the builder entry
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_section_octree_device_equals_host(renderer, name, compact):
    w = _case(name)
    host = _host_octree(name, compact)
    dev = _cell_scene().build_octree(w.depth, renderer=renderer, compact=compact, sections=w)
    _same_tree(dev, host, name)
    if name in ("empty", "all-air"):
        assert dev.octant_count == 1 and dev.octant_mask[0] == 0
    if name.startswith("d4-uniform"):  # the root stays an octant of eight leaves
        flag, idx = (_cell_scene().build_octree(4, renderer=renderer, compact=compact, sections=_case(n))
                     for n in ("d4-uniform-flag", "d4-uniform-indices"))
        _same_tree(flag, idx, "flag form against index form")
        if compact:
            assert dev.octant_count == 1 and dev.octant_mask[0] == 0xFFFF and np.all(dev.octant_children[0] == 6)
    if name == "d5-eight-uniform" and compact:
        assert dev.octant_count == 1 and dev.octant_mask[0] == 0xFFFF and np.all(dev.octant_children[0] == 3)
    if name == "d5-eight-one-other" and compact:
        assert 1 < dev.octant_count <= 1 + 4  # the root and the path to the voxel: seven sections merge
    if name == "d7-random-300":
        kinds = w.sections["index_first"] == UNIFORM
        assert 0 < kinds.sum() < len(kinds) and len(w.to_cells()) > 100_000


def _device_world(torch, w, offset_indices=False):
    """The world's three arrays as torch tensors on the GPU: (tensors to keep alive, device addresses)."""
    secs = torch.as_tensor(w.sections.view(np.uint32).view(np.int32).copy(), device="cuda")
    pal = torch.as_tensor(w.palette.view(np.int32).copy(), device="cuda")
    idx = torch.empty(len(w.indices) + 1, dtype=torch.int16, device="cuda")
    at = 1 if offset_indices else 0
    idx[at:at + len(w.indices)] = torch.as_tensor(w.indices.view(np.int16).copy(), device="cuda")
    torch.cuda.synchronize()
    ptrs = (secs.data_ptr(), pal.data_ptr(), idx.data_ptr() + 2 * at)
    return (secs, pal, idx), ptrs


@pytest.mark.parametrize("name", ["d7-random-300", "C5s-small"])
def test_device_resident_sections(torch_cuda, renderer, name):
    w = _case(name)
    keep, ptrs = _device_world(torch_cuda, w)
    assert ptrs[2] % 16 == 0
    for compact in (False, True):
        dev = _cell_scene().build_octree(w.depth, renderer=renderer, compact=compact, sections=w, device_sections=ptrs)
        _same_tree(dev, _host_octree(name, compact), f"device sections, compact={compact}")
    keep2, ptrs2 = _device_world(torch_cuda, w, offset_indices=True)  # indices only 2-byte aligned
    assert ptrs2[2] % 16 == 2
    dev = _cell_scene().build_octree(w.depth, renderer=renderer, compact=True, sections=w, device_sections=ptrs2)
    _same_tree(dev, _host_octree(name, True), "2-byte aligned device indices")


# ------------------------------------------------------------------ the scene entry
def _settings(name, res):
    sc, cam, rs, w = _config(name)
    rs = dataclasses.replace(rs)
    if res:
        rs.width, rs.height, rs.spp = res
    return sc, cam, rs, w


_UPLOADED = {}


def _uploaded_shot(torch, r, name, res, compact):
    """The reference side, once per (name, compact): the host octree through octpt_scene_upload."""
    if (name, compact) not in _UPLOADED:
        sc, cam, rs, w = _settings(name, res)
        host = dataclasses.replace(sc, octree=_host_octree(name, compact))
        _UPLOADED[(name, compact)] = _shot(torch, r, host, cam, rs, sc._depth, True)
    return _UPLOADED[(name, compact)]


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("name,res", SCENES)
def test_scene_build_sections_device_equals_upload(torch_cuda, renderer, name, res, compact):
    sc, cam, rs, w = _settings(name, res)
    a = _uploaded_shot(torch_cuda, renderer, name, res, compact)
    assert a[2]["block_tests"] > 0
    renderer.set_scene_built_sections(sc, sc._depth, w, compact=compact)
    assert renderer.stats()["build_ms"] > 0.0
    _same_shot(_shot(torch_cuda, renderer, sc, cam, rs, sc._depth, False), a, name)


def test_scene_build_sections_on_device(torch_cuda, renderer):
    name, res = "C5s-small", (160, 90, 2)
    sc, cam, rs, w = _settings(name, res)
    a = _uploaded_shot(torch_cuda, renderer, name, res, True)
    keep, ptrs = _device_world(torch_cuda, w, offset_indices=True)
    renderer.set_scene_built_sections(sc, sc._depth, w, compact=True, on_device=ptrs)
    _same_shot(_shot(torch_cuda, renderer, sc, cam, rs, sc._depth, False), a, "device sections")


# ------------------------------------------------------------------ refusals on the device
def test_section_build_device_errors(torch_cuda, renderer):
    """Every refusal comes back INVALID_ARG from both device entries as from the host entry, and the context
    builds and renders a valid world right after each."""
    from octree_pathtracing_amd import _lib

    lib, ctx = renderer._lib, renderer._ctx
    bad = _lib.ERR_INVALID_ARG
    name = "blocks-b"
    sc, cam, rs, good = _settings(name, None)
    want = _uploaded_shot(torch_cuda, renderer, name, None, False)
    desc, keep = sc.to_desc(octree=False, depth=6)
    air = np.zeros(4096, np.uint16)
    two = air.copy()
    two[77] = 2
    n_blocks = len(sc.blocks)
    refused = {
        "range": world([(0, 0, 0, 0, 1, 0), (4, 0, 0, 0, 1, 0)], [1], air),
        "duplicate": world([(1, 1, 1, 0, 1, 0), (2, 1, 1, 0, 1, 0), (1, 1, 1, 0, 1, UNIFORM)], [1], air),
        "index >= palette_count": world([(0, 0, 0, 0, 2, 0)], [0, 1, 3], two),
        "value >= 2^27": world([(0, 0, 0, 0, 2, 0)], [1, 1 << 27], air),
        "palette slice": world([(0, 0, 0, 1, 2, 0)], [0, 1], air),
        "index block": world([(0, 0, 0, 0, 1, 4096)], [1], air),
        "uniform": world([(0, 0, 0, 0, 2, UNIFORM)], [1, 2], air),
    }

    def recovers(tag):
        renderer.set_scene_built_sections(sc, sc._depth, good)
        _same_shot(_shot(torch_cuda, renderer, sc, cam, rs, sc._depth, False), want, f"after {tag}")

    for tag, w in refused.items():
        s, out, n = w.struct(), C.c_void_p(), C.c_uint32()
        assert lib.octpt_sections_to_cells(C.byref(s), 6, None, 0, C.byref(n)) == bad, tag
        assert lib.octpt_build_block_octree_sections_device(ctx, C.byref(s), 6, 0, C.byref(out)) == bad, tag
        assert not out.value and lib.octpt_last_error(ctx)
        assert lib.octpt_scene_build_sections_device(ctx, C.byref(desc), C.byref(s), 0) == bad, tag
        recovers(tag)
    # a value beyond the block table: the scene entry alone
    w = world([(0, 0, 0, 0, 2, 0)], [1, n_blocks], air)
    s, out = w.struct(), C.c_void_p()
    assert lib.octpt_build_block_octree_sections_device(ctx, C.byref(s), 6, 0, C.byref(out)) == _lib.OK
    lib.octpt_octree_free(out)
    assert lib.octpt_scene_build_sections_device(ctx, C.byref(desc), C.byref(s), 0) == bad
    assert b"block" in lib.octpt_last_error(ctx)
    recovers("value >= block_count")
    # flags on the wrong entry, unknown flags, depth, NULL arguments
    s, out = good.struct(), C.c_void_p()
    cells = sc.cells_array()
    p = cells.ctypes.data_as(C.c_void_p)
    desc_b, keep_b = sc.to_desc(octree=False, depth=sc._depth)
    for flag in (_lib.BUILD_CELLS_ON_DEVICE, 0x100):
        assert lib.octpt_build_block_octree_sections_device(ctx, C.byref(s), sc._depth, flag, C.byref(out)) == bad
        assert lib.octpt_scene_build_sections_device(ctx, C.byref(desc_b), C.byref(s), flag) == bad
    flag = _lib.BUILD_SECTIONS_ON_DEVICE
    assert lib.octpt_build_block_octree_device(ctx, p, len(cells), sc._depth, flag, C.byref(out)) == bad
    assert lib.octpt_scene_build_blocks_device(ctx, C.byref(desc_b), p, len(cells), flag) == bad
    assert lib.octpt_build_block_octree(p, len(cells), sc._depth, flag, C.byref(out)) == bad
    recovers("flags on the wrong entry")
    for depth in (3, 22):
        assert lib.octpt_build_block_octree_sections_device(ctx, C.byref(s), depth, 0, C.byref(out)) == bad
    assert lib.octpt_build_block_octree_sections_device(ctx, None, 6, 0, C.byref(out)) == bad
    assert lib.octpt_build_block_octree_sections_device(ctx, C.byref(s), 6, 0, None) == bad
    assert lib.octpt_scene_build_sections_device(ctx, None, C.byref(s), 0) == bad
    assert lib.octpt_scene_build_sections_device(ctx, C.byref(desc_b), None, 0) == bad
    assert lib.octpt_scene_build_sections_device(None, C.byref(desc_b), C.byref(s), 0) == bad
    saved = desc_b.blocks, desc_b.block_count
    desc_b.blocks, desc_b.block_count = None, 0  # a descriptor without blocks
    assert lib.octpt_scene_build_sections_device(ctx, C.byref(desc_b), C.byref(s), 0) == bad
    desc_b.blocks, desc_b.block_count = saved
    recovers("argument errors")


# ------------------------------------------------------------------ sequences on one context
def test_cell_and_section_builds_alternate(torch_cuda, renderer):
    """A cell build, a section build and a cell build again share the context's scratch."""
    from tests.test_gpu_block_build import _case as cell_case

    depth, cells = cell_case("d12-random")
    cell_sc = _cell_scene(cells)
    cell_host = dataclasses.replace(cell_sc).build_octree(depth, compact=True)
    w = _case("C5s-small")
    for step in range(3):
        if step == 1:
            dev = _cell_scene().build_octree(w.depth, renderer=renderer, compact=True, sections=w)
            _same_tree(dev, _host_octree("C5s-small", True), "section build between cell builds")
        else:
            dev = dataclasses.replace(cell_sc).build_octree(depth, renderer=renderer, compact=True)
            _same_tree(dev, cell_host, f"cell build {step}")
    # the scene entries the same way
    name, res = "C5s-small", (160, 90, 2)
    sc, cam, rs, world_s = _settings(name, res)
    a = _uploaded_shot(torch_cuda, renderer, name, res, True)
    small = _config("blocks-b")[0]
    renderer.set_scene_built(small, small._depth, compact=True)
    renderer.set_scene_built_sections(sc, sc._depth, world_s, compact=True)
    _same_shot(_shot(torch_cuda, renderer, sc, cam, rs, sc._depth, False), a, "sections after cells")
    renderer.set_scene_built(sc, sc._depth, compact=True)
    _same_shot(_shot(torch_cuda, renderer, sc, cam, rs, sc._depth, False), a, "cells after sections")


def _cell_keys(cells):
    """the cells as sorted 64-bit keys (coordinates < 2^12, values < 2^27): set equality without Python tuples"""
    c = cells.astype(np.uint64)
    return np.sort(c[:, 0] << np.uint64(51) | c[:, 1] << np.uint64(39) | c[:, 2] << np.uint64(27) | c[:, 3])


def test_section_edit_and_rebuild(torch_cuda, renderer):
    """One voxel of one section changes (the top block of a column becomes stone), then a rebuild."""
    from octree_pathtracing_amd import scene as S

    name, res = "C5s-small", (160, 90, 2)
    sc, cam, rs, w = _settings(name, res)
    cells = sc.cells_array()
    x, z = 24 + 64, 24 + 40
    col = np.flatnonzero((cells[:, 0] == x) & (cells[:, 2] == z))
    k = col[np.argmax(cells[col, 1])]
    y, before, stone = int(cells[k, 1]), int(cells[k, 3]), 3  # block 2 = stone, value 3
    assert before != stone
    down = np.array([[x + 0.5, 300.0, z + 0.5, 0.0, -1.0, 0.0]], np.float32)  # straight down onto the column
    renderer.set_scene_built_sections(sc, sc._depth, w, compact=True)
    t, prim, _, _ = renderer.intersect(down)
    assert prim[0] == before and abs(t[0] - (300.0 - (y + 1.0))) < 1e-2
    # the edit, in the section's own arrays: a palette slice of its own with stone in it, one index changed
    s = int(np.flatnonzero((w.sections["x"] == x >> 4) & (w.sections["y"] == y >> 4) & (w.sections["z"] == z >> 4))[0])
    sec = w.sections[s]
    assert sec["index_first"] != UNIFORM
    pal = np.concatenate([w.palette[sec["palette_first"]:sec["palette_first"] + sec["palette_count"]], [stone]])
    secs, idx = w.sections.copy(), w.indices.copy()
    secs["palette_first"][s], secs["palette_count"][s] = len(w.palette), len(pal)
    at = int(sec["index_first"]) + ((y & 15) << 8 | (z & 15) << 4 | (x & 15))
    assert pal[idx[at]] == before
    idx[at] = len(pal) - 1
    edited = S.SectionWorld(secs, np.concatenate([w.palette, pal.astype(np.uint32)]), idx, w.depth)
    want = cells.copy()
    want[k, 3] = stone
    assert np.array_equal(_cell_keys(edited.to_cells()), _cell_keys(want))
    host = dataclasses.replace(sc, cells=want, octree=None)
    host.build_octree(sc._depth, compact=True)
    b = _shot(torch_cuda, renderer, host, cam, rs, sc._depth, True)
    renderer.set_scene_built_sections(sc, sc._depth, edited, compact=True)
    _same_shot(_shot(torch_cuda, renderer, sc, cam, rs, sc._depth, False), b, "edit")
    t, prim, _, _ = renderer.intersect(down)
    assert prim[0] == stone and abs(t[0] - (300.0 - (y + 1.0))) < 1e-2


# ------------------------------------------------------------------ multi-device
@pytest.fixture(scope="module")
def multi2(torch_cuda):
    from octree_pathtracing_amd.renderer import HipRenderer

    r = HipRenderer(devices=[0, 0])
    assert r.device_entries == 2
    yield r
    r.close()


def test_multi_device(torch_cuda, renderer, multi2):
    """Every entry of a multi-device context builds its own replica; device sections are refused there."""
    from octree_pathtracing_amd import _lib

    sc, cam, rs, w = _settings("blocks-b", None)
    renderer.set_scene_built_sections(sc, sc._depth, w, compact=True)
    one = gpu_render(torch_cuda, renderer, sc, cam, rs, upload=False)
    multi2.set_scene_built_sections(sc, sc._depth, w, compact=True)
    two = gpu_render(torch_cuda, multi2, sc, cam, rs, upload=False)
    assert np.array_equal(one[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(one[1], two[1])
    for k in STAT_KEYS:
        assert one[2][k] == two[2][k], k
    _same_tree(_cell_scene().build_octree(w.depth, renderer=multi2, compact=True, sections=w),
               _host_octree("blocks-b", True), "multi")
    keep, ptrs = _device_world(torch_cuda, w)
    s, out = w.struct(ptrs), C.c_void_p()
    desc, keep_d = sc.to_desc(octree=False, depth=sc._depth)
    flag = _lib.BUILD_SECTIONS_ON_DEVICE
    lib = multi2._lib
    assert lib.octpt_scene_build_sections_device(multi2._ctx, C.byref(desc), C.byref(s), flag) == _lib.ERR_UNSUPPORTED
    st = lib.octpt_build_block_octree_sections_device(multi2._ctx, C.byref(s), w.depth, flag, C.byref(out))
    assert st == _lib.ERR_UNSUPPORTED and not out.value
