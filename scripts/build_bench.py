"""Octree build time: host builder (octpt_build_octree) vs the GPU builder
(octpt_build_octree_device).  Prints the library call's wall time (the device call includes the
primitive upload and the result download) and the GPU time of the build kernels.

Block-value configs (C5b, C5s) run the block legs instead: octpt_build_block_octree against
octpt_build_block_octree_device (end to end: cell upload, build, octant download), the build kernels alone,
and scene set-up through octpt_scene_build_blocks_device against the host build + octpt_scene_upload.  C5s is
built compacted (as it is rendered), C5b not (nothing merges there).

`--sections` runs the sections leg for them instead: the world packed once into a SectionWorld
(outside the timed region), scene set-up through octpt_scene_build_sections_device from host arrays and from
arrays on the device, against the cell path in the same run, the bytes each path uploads, and the build kernels'
time."""
import ctypes as C
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from octree_pathtracing_amd import _lib, scene as S  # noqa: E402
from octree_pathtracing_amd.renderer import HipRenderer  # noqa: E402

r = HipRenderer(0)
lib = _lib.load()


def call(sc, depth, ctx=None, reps=3):
    sph, cub = sc.sphere_structs(), sc.cuboid_structs()
    args = (C.cast(sph, C.c_void_p) if len(sc.spheres) else None, len(sc.spheres),
            C.cast(cub, C.c_void_p) if len(sc.cuboids) else None, len(sc.cuboids), depth)
    best = 1e9
    for _ in range(reps):
        h = C.c_void_p()
        t = time.perf_counter()
        st = lib.octpt_build_octree(*args, C.byref(h)) if ctx is None else \
            lib.octpt_build_octree_device(ctx, *args, C.byref(h))
        best = min(best, time.perf_counter() - t)
        _lib.check(lib, ctx, st)
        lib.octpt_octree_free(h)
    return best


def best_of(fn, reps):
    best = 1e9
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


def block_leg(name, sc, depth):
    compact = name.startswith("C5s")
    flags = _lib.BUILD_COMPACT if compact else 0
    cells = sc.cells_array()
    p, n = cells.ctypes.data_as(C.c_void_p), len(cells)
    reps = 3 if n < 10_000_000 else 1  # the host builder sorts C5s's 110 M cells on one core
    octants = [0]

    def build(ctx):
        h = C.c_void_p()
        st = lib.octpt_build_block_octree(p, n, depth, flags, C.byref(h)) if ctx is None else \
            lib.octpt_build_block_octree_device(ctx, p, n, depth, flags, C.byref(h))
        _lib.check(lib, ctx, st)
        v = _lib.OctreeView()
        lib.octpt_octree_get_view(h, C.byref(v))
        octants[0] = v.octant_count
        lib.octpt_octree_free(h)

    print(f"{name}: {n} cells, depth {depth}, compact={compact}", flush=True)
    th = best_of(lambda: build(None), reps)
    print(f"{name}: host builder {th * 1e3:.1f} ms ({octants[0]} octants)", flush=True)
    build(r._ctx)  # warm: scratch and code objects
    tg = best_of(lambda: build(r._ctx), 3)
    kms = r.stats()["build_ms"]
    print(f"{name}: GPU builder {tg * 1e3:.1f} ms end to end ({th / tg:.1f}x), build kernels {kms:.2f} ms "
          f"({th * 1e3 / kms:.0f}x)", flush=True)

    def setup_host():
        sc.build_octree(depth, compact=compact)
        r.set_scene(sc)

    r.set_scene_built(sc, depth, compact=compact)  # warm
    td = best_of(lambda: r.set_scene_built(sc, depth, compact=compact), 3)
    kms2 = r.stats()["build_ms"]
    tu = best_of(setup_host, reps)
    print(f"{name}: scene set-up on the device {td * 1e3:.1f} ms (build kernels {kms2:.2f} ms) against host build + "
          f"octpt_scene_upload {tu * 1e3:.1f} ms ({tu / td:.1f}x)", flush=True)


def section_leg(name, sc, depth):
    import numpy as np
    import torch

    compact = name.startswith("C5s")
    sc = sc.with_air_block()  # palette value 0 is air: block b becomes value b + 1
    cells = sc.cells_array()
    t = time.perf_counter()
    w = S.SectionWorld.from_cells(cells, depth)
    uniform = int((w.sections["index_first"] == _lib.SECTION_UNIFORM).sum())
    print(f"{name}: {len(cells)} cells in {len(w.sections)} sections ({uniform} uniform), {len(w.palette)} palette "
          f"entries, packed in {time.perf_counter() - t:.1f} s (not timed below); uploads: cells {cells.nbytes / 1e6:.1f} MB, "
          f"sections {w.nbytes / 1e6:.1f} MB ({cells.nbytes / w.nbytes:.1f}x fewer)", flush=True)
    keep = [torch.as_tensor(a.view(np.uint8).copy(), device="cuda") for a in (w.sections, w.palette, w.indices)]
    d_cells = torch.as_tensor(cells.view(np.int32), device="cuda")
    torch.cuda.synchronize()
    ptrs = tuple(k.data_ptr() for k in keep)
    legs = {"cells, host array": lambda rr: rr.set_scene_built(sc, depth, compact=compact),
            "cells, device array": lambda rr: rr.set_scene_built_cells(sc, depth, d_cells.data_ptr(), len(cells),
                                                                       compact=compact),
            "sections, host arrays": lambda rr: rr.set_scene_built_sections(sc, depth, w, compact=compact),
            "sections, device arrays": lambda rr: rr.set_scene_built_sections(sc, depth, w, compact=compact,
                                                                              on_device=ptrs)}
    times = {}
    for tag, fn in legs.items():
        fn(r)  # warm: scratch and code objects
        times[tag] = best_of(lambda: fn(r), 5)
        kms = r.stats()["build_ms"]
        times[tag + " kernels"] = kms
        print(f"{name}: scene set-up from {tag}: {times[tag] * 1e3:.2f} ms (build kernels {kms:.2f} ms)", flush=True)
    print(f"{name}: set-up from host arrays, sections against cells: {times['cells, host array'] / times['sections, host arrays']:.2f}x "
          f"({(times['cells, host array'] - times['sections, host arrays']) * 1e3:.2f} ms less); from device arrays "
          f"{times['cells, device array'] / times['sections, device arrays']:.2f}x; build kernels "
          f"{times['cells, device array kernels'] / times['sections, device arrays kernels']:.2f}x", flush=True)


args = [a for a in sys.argv[1:] if a != "--sections"]
sections = "--sections" in sys.argv[1:]
for name in args or ["C3", "C4", "C5", "C5b", "C5s"]:
    print(f"{name}: generating the scene", flush=True)
    sc, _, _ = S.make_config(name, build=False)
    d = sc._depth
    if sc.blocks is not None:
        (section_leg if sections else block_leg)(name, sc, d)
        continue
    th = call(sc, d)
    tg = call(sc, d, r._ctx)
    kms = r.stats()["build_ms"]
    n = sc.build_octree(d)
    print(f"{name}: {n.octant_count} octants, {len(n.leaf_first)} leaves, {len(n.leaf_prims)} pairs; host builder "
          f"{th * 1e3:.1f} ms, GPU builder {tg * 1e3:.1f} ms end to end ({th / tg:.1f}x), build kernels "
          f"{kms:.2f} ms ({th * 1e3 / kms:.0f}x)", flush=True)
