"""The device block builds at the C-ABI boundary, without a GPU: octpt_build_block_octree_device
and octpt_scene_build_blocks_device refuse a NULL context, with host cells and with the device-cells flag;
the block scene's build descriptor; the flag constant."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from octree_pathtracing_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "octpt.h"


def test_null_context_calls_fail_cleanly():
    lib = _lib.load()
    out = C.c_void_p()
    cells = np.array([[0, 0, 0, 1]], np.uint32)
    p = cells.ctypes.data_as(C.c_void_p)
    assert lib.octpt_build_block_octree_device(None, p, 1, 4, 0, C.byref(out)) == _lib.ERR_INVALID_ARG
    assert not out.value
    assert lib.octpt_build_block_octree_device(None, None, 0, 4, _lib.BUILD_CELLS_ON_DEVICE, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_scene_build_blocks_device(None, None, None, 0, 0) == _lib.ERR_INVALID_ARG
    desc = _lib.SceneDesc()
    assert lib.octpt_scene_build_blocks_device(None, C.byref(desc), p, 1, _lib.BUILD_COMPACT) == _lib.ERR_INVALID_ARG


def test_host_builder_still_refuses_the_device_flag():
    lib = _lib.load()
    out = C.c_void_p()
    cells = np.array([[0, 0, 0, 1]], np.uint32)
    st = lib.octpt_build_block_octree(cells.ctypes.data_as(C.c_void_p), 1, 4, _lib.BUILD_CELLS_ON_DEVICE, C.byref(out))
    assert st == _lib.ERR_INVALID_ARG and not out.value


def test_block_build_descriptor():
    """Scene.to_desc(octree=False, depth=...) of a block-value scene: the block table and the build depth,
    no octree and no primitives (what octpt_scene_build_blocks_device takes)."""
    from octree_pathtracing_amd import scene as S

    sc, _, _ = S.make_config("blocks-b", build=False)
    d, keep = sc.to_desc(octree=False, depth=5)
    assert d.blocks and d.block_count == len(sc.blocks) > 0 and d.depth == 5
    assert not d.octants and d.octant_count == 0 and d.root == 0
    assert not d.leaf_first and not d.leaf_count and d.leaf_table_size == 0
    assert not d.leaf_prims and d.leaf_prim_count == 0
    assert not d.spheres and d.sphere_count == 0 and not d.cuboids and d.cuboid_count == 0
    assert not d.cuboid_model
    assert d.material_count == len(sc.materials) and d.texture_count == len(sc.textures)
    cells = sc.cells_array()
    assert cells.dtype == np.uint32 and cells.ndim == 2 and cells.shape[1] == 4 and cells.flags.c_contiguous


def test_flag_constant_matches_header():
    m = re.search(r"#define\s+OCTPT_BUILD_CELLS_ON_DEVICE\s+0x([0-9a-fA-F]+)u", HEADER.read_text())
    assert m and int(m.group(1), 16) == _lib.BUILD_CELLS_ON_DEVICE == 0x2
    assert _lib.BUILD_CELLS_ON_DEVICE & _lib.BUILD_COMPACT == 0
