"""GPU traversal at octree depths 12-21 against the oracle (worlds of tests/deep_worlds.py).

Everything that walks an octree on the device -- the wavefront with and without the camera rays' beam start, the
megakernel, the drain, the preview, the guide buffers, octpt_intersect, tile-list and adaptive renders -- on trees
deeper than the configs' 11, up to kMaxDepth = 21: the LDS stack at twice the size the other tests launch, the push
and pop slots of levels 12-21, the depth-indexed occupancy caches, and world coordinates near 2^20.  The bar is
tests/test_gpu_parity.py's, imported unchanged; tests/test_deep_cpu.py shows on every machine that each case
compares something."""
import dataclasses
import os

import numpy as np
import pytest

from tests import deep_worlds as DW
from tests import intersect_rays as IR
from tests.adaptive_ref import adaptive_loop, tile_grid, tile_mask
from tests.test_gpu_beam import _same as same_but_iterations
from tests.test_gpu_beam import assert_parity_shipped
from tests.test_gpu_block_build import _same_shot
from tests.test_gpu_intersect_edges import assert_rays_equal
from tests import test_gpu_parity as parity
from tests.test_gpu_parity import (REL_TOL_FORWARD, REL_TOL_RECURSIVE, assert_parity, gpu_render, rel_err,  # noqa: F401
                                   renderer, torch_cuda)

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = DW.NONE
STATS = ("paths", "segments", "sphere_tests", "cuboid_tests", "shade_events", "texel_reads", "block_tests")


def _renderer_with(env):
    from octree_pathtracing_amd.renderer import HipRenderer

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # read when the context is created
    try:
        return HipRenderer(device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _context(env):
    def make(torch_cuda):
        r = _renderer_with(env)
        yield r
        r.close()

    return pytest.fixture(scope="module")(make)


# `renderer` (tests/conftest.py: OCTPT_BEAM=0) is the context whose ESVO iteration total the oracle restates
beam = _context({"OCTPT_BEAM": "1"})  # the shipped default
small_pool = _context({"OCTPT_BEAM": "1", "OCTPT_POOL": "100", "OCTPT_REFILL": "1", "OCTPT_CHUNK": "2000"})
no_drain = _context({"OCTPT_BEAM": "1", "OCTPT_DRAIN_RAYS": "0"})
# the drain takes over as soon as every item is claimed, whatever the queue's length (its default bound is 4096 rays)
pool_drain = _context({"OCTPT_BEAM": "1", "OCTPT_DRAIN_RAYS": "1000000"})


def _identical(a, b, tag, stats=STATS + ("esvo_steps",)):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{tag}: radiance"
    assert np.array_equal(a[1], b[1]), f"{tag}: segment counts"
    for k in stats:
        assert a[2][k] == b[2][k], (tag, k, a[2][k], b[2][k])


# ---------------------------------------------------------------------------------------------- renders
@pytest.mark.parametrize("name", list(DW.CASES))
def test_deep_render_parity(torch_cuda, renderer, beam, name):
    """Every generator at every depth through octpt_render_device.  With the beam on (the shipped default) against
    the oracle: everything of assert_parity but the ESVO iteration total, which the beam can only lower
    (assert_parity_shipped); with the beam off assert_parity itself, the iteration total included; the two renders
    equal bit for bit; the recursive oracle within its tolerance."""
    sc, cam, tag = DW.case(name)
    rs = DW.settings()
    ref = DW.reference(name)
    on = gpu_render(torch_cuda, beam, sc, cam, rs)
    exact = assert_parity_shipped(on, ref, f"{tag}, beam on")
    assert exact > 0.999, f"{tag}: only {exact:.4%} of channels bit-identical"
    off = gpu_render(torch_cuda, renderer, sc, cam, rs)
    assert assert_parity(off, ref, tag) > 0.999
    same_but_iterations(on, off)
    assert rel_err(on[0], DW.reference(name, False)[0]).max() <= REL_TOL_RECURSIVE
    if name.startswith("forms16"):  # the reader form of the same tree renders bit-identically
        reader = DW.case("blocks16c" if name.endswith("lifted") else "blocks16")[0]
        _identical(gpu_render(torch_cuda, renderer, reader, cam, rs), off, tag)


@pytest.mark.parametrize("name", ["blocks21", "prims21"])
def test_deep_variants_identical(torch_cuda, renderer, beam, small_pool, no_drain, pool_drain, name):
    from octree_pathtracing_amd.renderer import shard_pixels

    torch = torch_cuda
    sc, cam, tag = DW.case(name)
    rs = DW.settings()
    default = gpu_render(torch, beam, sc, cam, rs)
    off = gpu_render(torch, renderer, sc, cam, rs)
    same_but_iterations(default, off)
    assert off[2]["esvo_steps"] == DW.reference(name)[2]["esvo_steps"]
    mega = gpu_render(torch, beam, sc, cam, rs, megakernel=True)
    _identical(mega, default, f"{tag} megakernel", STATS)
    assert mega[2]["esvo_steps"] in (default[2]["esvo_steps"], off[2]["esvo_steps"])
    for ctx, what in ((small_pool, "100-slot pool, 2000-item chunks"), (no_drain, "no drain"),
                      (pool_drain, "the drain from the first exhausted queue on")):
        _identical(gpu_render(torch, ctx, sc, cam, rs), default, f"{tag} {what}")
    assert gpu_render(torch, pool_drain, sc, cam, rs)[2]["drain"]["segments"] > 0
    # branch count 10 over 20 samples (passes of weight 1, 1, 1, 1, 6, 10)
    from oracle import cpu_ref

    rb = DW.settings(spp=20)
    b_on = gpu_render(torch, beam, sc, cam, rb, branch_count=10)
    b_off = gpu_render(torch, renderer, sc, cam, rb, branch_count=10)
    same_but_iterations(b_on, b_off)
    racc, rsegs, _ = cpu_ref.render(sc, cam, rb.width, rb.height, rb.spp, max_depth=rb.max_depth, seed=rb.seed,
                                    forward=True, branch_count=10)
    assert np.array_equal(b_on[1], rsegs)
    assert rel_err(b_on[0], racc).max() <= REL_TOL_FORWARD and (b_on[0] == racc).mean() > 0.999
    # three compact shards of a frame whose tiles overhang both edges, gathered by the unshard kernel
    rr = DW.settings(37, 21)
    full = gpu_render(torch, beam, sc, cam, rr)[0]
    N = 3
    stride = max(shard_pixels(rr.width, rr.height, i, N) for i in range(N))
    buf = torch.zeros((N * stride, 4), dtype=torch.float32, device="cuda")
    for i in range(N):
        a = gpu_render(torch, beam, sc, cam, rr, shard=(i, N), compact=True)[0]
        buf[i * stride:i * stride + len(a)] = torch.as_tensor(a, device="cuda")
    frame = torch.zeros((rr.height * rr.width, 4), dtype=torch.float32, device="cuda")
    beam.unshard_device(rr.width, rr.height, N, buf.data_ptr(), stride, frame.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().reshape(rr.height, rr.width, 4), full)
    ref37 = cpu_ref.render(sc, cam, 37, 21, rr.spp, max_depth=rr.max_depth, seed=rr.seed, forward=True)[0]
    assert rel_err(full, ref37).max() <= REL_TOL_FORWARD


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("name", ["blocks21", "prims21", "corner21-inside", "models16"])
def test_deep_preview_and_aov(torch_cuda, renderer, name):
    """The preview bit-exact to the oracle's; the guide buffers by tests/test_gpu_aov.py's rule: on every pixel whose
    preview chain is one segment prim, normal and depth equal the oracle's Scene::hit of the pixel's camera ray, depth
    by its bits, and the material is set; octpt_intersect answers the camera rays as the oracle does."""
    from oracle import cpu_ref

    sc, cam, tag = DW.case(name)
    rs = DW.settings()
    W, H = rs.width, rs.height
    pre = np.random.default_rng(3).random((H, W, 4), dtype=np.float32)
    acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, rs, accum=pre, preview=True)
    racc, rsegs, rst = cpu_ref.render(sc, cam, W, H, 1, max_depth=rs.max_depth, seed=rs.seed, accum=pre.copy(),
                                      preview=True)
    assert np.array_equal(segs, rsegs) and np.array_equal(acc, racc), tag
    assert st["segments"] == rst["segments"] and st["esvo_steps"] == rst["esvo_steps"]
    assert st["texel_reads"] == rst["texel_reads"] and st["shade_events"] == 0
    rays = renderer.camera_rays(W, H).reshape(-1, 6)
    ref = cpu_ref.intersect(sc, rays)
    assert_rays_equal(renderer.intersect(rays), ref, rays, f"{tag} camera rays")
    rt, rprim, rn = ref[0].reshape(H, W), ref[1].reshape(H, W), ref[2].reshape(H, W, 3)
    renderer.reset_stats()
    a = renderer.render_aov(rs)
    ast = renderer.stats()
    one = rsegs == 1
    hit, miss = one & np.isfinite(rt), one & ~np.isfinite(rt)
    assert hit.mean() > 0.2, tag
    assert np.array_equal(a["prim"][hit], rprim[hit])
    assert np.array_equal(_bits(a["normal"][..., :3][hit]), _bits(rn[hit]))
    assert np.array_equal(_bits(a["depth"][hit]), _bits(rt[hit]))
    assert np.all(a["material"][hit] != 0) and np.all(a["albedo"][..., 3][hit] > 0)
    assert np.all(np.isposinf(a["depth"][miss])) and np.all(a["prim"][miss] == NONE)
    assert not a["albedo"][miss].any() and not a["normal"][miss].any() and not a["material"][miss].any()
    assert ast["segments"] == rst["segments"] and ast["esvo_steps"] == rst["esvo_steps"]


@pytest.mark.parametrize("name", ["blocks21", "blocks21c", "prims21", "corner21-outside"])
def test_deep_intersect(renderer, name):
    """octpt_intersect against cpu_ref.intersect: the case's 4096 random rays, the edge families of
    tests/intersect_rays.py built from the deep geometry (once per corner in a corner world), the exact axis rays of tests/test_deep_cpu.py, and second
    segments with the self-hit key sent with key and normal, with the key alone and unkeyed."""
    from oracle import cpu_ref

    sc, _, tag = DW.case(name)
    renderer.set_scene(sc)
    rays, ref = DW.ray_batch(name)
    assert_rays_equal(renderer.intersect(rays), ref, rays, f"{tag} random")
    if name.startswith(("blocks21", "corner21")):
        ax = (DW.axis_rays_corner if name.startswith("corner") else DW.axis_rays_blocks)(21)
        assert_rays_equal(renderer.intersect(ax), cpu_ref.intersect(sc, ax), ax, f"{tag} axis")
    for ci, g in enumerate(DW.cluster_geometries(sc)):  # a corner world: the families once per corner
        ctag = f"{tag} cluster {ci}"
        first, fam = IR.first_pass(g, IR.SEED, primitive_scene=sc.blocks is None)
        fref = cpu_ref.intersect(sc, first)
        for f, sl in fam.items():
            if f != "zero":
                assert 0.02 < (fref[1][sl] != NONE).mean() < 0.98, (ctag, f)
        assert_rays_equal(renderer.intersect(first), fref, first, ctag, fam)
        b = IR.bounce(first, fref[0], fref[1], fref[2], IR.SEED + 1, block_values=sc.blocks is not None)
        kinds = {d: b["dir"] == j for j, d in enumerate(IR.BOUNCE_DIRS)}
        answers = []
        for mode, lp, ln in (("key+normal", b["last_prim"], b["last_normal"]), ("key", b["last_prim"], None),
                             ("unkeyed", None, None)):
            want = cpu_ref.intersect(sc, b["rays"], lp, ln)
            answers.append(want)
            assert_rays_equal(renderer.intersect(b["rays"], lp, ln), want, b["rays"], f"{ctag}/bounce {mode}", kinds, lp)
        if sc.blocks is None:  # the key changes the answer of enough rays to be seen
            assert (answers[0][1] != answers[2][1]).sum() >= 100


# ---------------------------------------------------------------------------------------------- device-built scenes
def _shot(torch, r, sc, cam, rays, upload):
    return gpu_render(torch, r, sc, cam, DW.settings(), upload=upload) + (r.intersect(rays),)


@pytest.mark.parametrize("compact", [False, True])
def test_deep_device_built_scene(torch_cuda, renderer, compact):
    """The three device scene builds at depth 21 leave the scene octpt_scene_upload makes of the host-built tree:
    renders and closest-hit queries bit-identical (tests/test_gpu_block_build.py's _same_shot)."""
    from octree_pathtracing_amd import scene as S
    from tests.test_gpu_section_build import _device_world

    torch = torch_cuda
    D = 21
    name = "blocks21c" if compact else "blocks21"
    sc, cam, tag = DW.case(name)
    rays = DW.ray_batch(name)[0]
    want = _shot(torch, renderer, sc, cam, rays, True)
    assert want[2]["block_tests"] > 0 and (want[3][1] != NONE).mean() > 0.05
    bare = dataclasses.replace(sc, octree=None)
    renderer.set_scene_built(bare, D, compact=compact)
    _same_shot(_shot(torch, renderer, sc, cam, rays, False), want, f"{tag}: host cells")
    cells = sc.cells_array()
    t = torch.as_tensor(cells.view(np.int32), device="cuda").contiguous()
    torch.cuda.synchronize()
    renderer.set_scene_built_cells(dataclasses.replace(bare, cells=None), D, t.data_ptr(), len(cells), compact=compact)
    _same_shot(_shot(torch, renderer, sc, cam, rays, False), want, f"{tag}: device cells")
    # sections: palette value 0 is air, so the block table gains an unused block 0 (Scene.with_air_block)
    air = sc.with_air_block()
    world = S.SectionWorld.from_cells(air.cells_array(), D)
    air.build_octree(D, compact=compact)
    want_s = _shot(torch, renderer, air, cam, rays, True)
    assert np.array_equal(want_s[1], want[1]) and want_s[2]["esvo_steps"] == want[2]["esvo_steps"]
    renderer.set_scene_built_sections(air, D, world, compact=compact)
    _same_shot(_shot(torch, renderer, air, cam, rays, False), want_s, f"{tag}: host sections")
    keep, ptrs = _device_world(torch, world)
    renderer.set_scene_built_sections(air, D, world, compact=compact, on_device=ptrs)
    _same_shot(_shot(torch, renderer, air, cam, rays, False), want_s, f"{tag}: device sections")
    del keep
    # primitives: octpt_scene_build_device
    pname = "prims21c" if compact else "prims21"
    ps, pcam, ptag = DW.case(pname)
    prays = DW.ray_batch(pname)[0]
    pwant = _shot(torch, renderer, ps, pcam, prays, True)
    assert pwant[2]["sphere_tests"] > 0 and pwant[2]["cuboid_tests"] > 0
    renderer.set_scene_built(dataclasses.replace(ps, octree=None), D, compact=compact)
    _same_shot(_shot(torch, renderer, ps, pcam, prays, False), pwant, ptag)
    assert pwant[2]["sphere_tests"] == _shot(torch, renderer, ps, pcam, prays, False)[2]["sphere_tests"]


@pytest.mark.parametrize("beam_on", [False, True])
def test_deep_then_shallow_same_context(torch_cuda, beam_on):
    """One context renders depth 21, then depth 5, then depth 21 again: the occupancy caches indexed by depth and the
    grow-only wavefront state across a 4x change of the LDS per block.  First and third render bit-identical, and
    both the oracle's; the depth-5 render between them is the `tiny` golden fixture's."""
    from octree_pathtracing_amd import scene as S

    r = _renderer_with({"OCTPT_BEAM": "1" if beam_on else "0"})
    try:
        sc, cam, tag = DW.case("blocks21")
        rs = DW.settings()
        first = gpu_render(torch_cuda, r, sc, cam, rs)
        if beam_on:
            tsc, tcam, trs = S.make_config("tiny")
            tiny = gpu_render(torch_cuda, r, tsc, tcam, trs)
            g = np.load(parity.GOLDEN / "tiny.npz", allow_pickle=False)
            assert np.array_equal(tiny[1], g["segcount"])
            assert rel_err(tiny[0], g["accum"]).max() <= REL_TOL_FORWARD and (tiny[0] == g["accum"]).mean() > 0.999
        else:
            parity.test_render_matches_golden_fixture(torch_cuda, r, "tiny")
        third = gpu_render(torch_cuda, r, sc, cam, rs)
        _identical(first, third, tag)
        (assert_parity_shipped if beam_on else assert_parity)(third, DW.reference("blocks21"), tag)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- tile lists, adaptive
class _Frames:
    def __init__(self, torch, W, H, accum=None, moments=None, seg=None):
        black = np.zeros((H, W, 4), F32)
        black[..., 3] = 1.0
        self.torch = torch
        self.acc = torch.from_numpy(np.ascontiguousarray(black if accum is None else accum, F32)).cuda()
        self.mom = torch.from_numpy(np.ascontiguousarray(np.zeros((H, W, 2), F32) if moments is None else moments)).cuda()
        s = np.zeros((H, W), np.uint32) if seg is None else np.ascontiguousarray(seg, np.uint32)
        self.seg = torch.from_numpy(s.view(np.int32)).cuda()

    def host(self):
        self.torch.cuda.synchronize()
        return self.acc.cpu().numpy(), self.mom.cpu().numpy(), self.seg.cpu().numpy().view(np.uint32)


def test_deep_tile_list_and_adaptive(torch_cuda, beam):
    """octpt_render_tiles_device over half of deep_blocks(21)'s tiles: the listed tiles hold the full render's pixels,
    the others come back untouched (tests/test_gpu_adaptive.py's rule).  octpt_render_adaptive_device with
    min_spp 2, step_spp 2, max_spp 6 equals tests/adaptive_ref.py's loop composed of tile-list renders."""
    from octree_pathtracing_amd import _lib
    from tests.test_gpu_adaptive import FLOOR, half_list, same, sentinel

    torch, r = torch_cuda, beam
    sc, cam, tag = DW.case("blocks21")
    rs = DW.settings()
    W, H = rs.width, rs.height
    full = gpu_render(torch, r, sc, cam, rs)  # uploads the scene and sets the camera
    r.branch_count = 1

    def params(start, count):
        return r.params(W, H, start, count)

    lst = half_list(W, H)
    inside = tile_mask(W, H, lst)
    assert inside.any() and (~inside).any()
    sa, sm, ss = sentinel(W, H)
    black = np.zeros((H, W, 4), F32)
    black[..., 3] = 1.0
    f = _Frames(torch, W, H, np.where(inside[..., None], black, sa), np.where(inside[..., None], F32(0), sm),
                np.where(inside, np.uint32(0), ss))
    r.render_tiles_device(params(0, rs.spp), lst, f.acc.data_ptr(), f.mom.data_ptr(), f.seg.data_ptr())
    a, m, s = f.host()
    assert same(a[inside], full[0][inside]) and np.array_equal(s[inside], full[1][inside])
    assert same(a[~inside], sa[~inside]) and same(m[~inside], sm[~inside]) and np.array_equal(s[~inside], ss[~inside])
    assert np.all(np.isfinite(m[inside])) and (m[inside][..., 0] > 0).mean() > 0.5

    # the adaptive driver against the composed loop
    T = int(np.prod(tile_grid(W, H)))
    d_err = torch.zeros(T, dtype=torch.float32, device="cuda")

    def errors(frames, tile_spp):
        d_spp = torch.from_numpy(np.ascontiguousarray(tile_spp).view(np.int32)).cuda()
        r.tile_error_device(_lib.TileErrorParams(W, H, FLOOR), frames.mom.data_ptr(), d_spp.data_ptr(), d_err.data_ptr())
        torch.cuda.synchronize()
        return d_err.cpu().numpy()

    f0 = _Frames(torch, W, H)
    r.render_tiles_device(params(0, 2), None, f0.acc.data_ptr(), f0.mom.data_ptr(), None)
    e1 = errors(f0, np.full(T, 2, np.uint32))
    threshold = float(np.median(e1[np.isfinite(e1)]))
    assert threshold > 0
    fc = _Frames(torch, W, H)

    def render(active, start, count):
        r.render_tiles_device(params(start, count), np.asarray(active, np.uint32), fc.acc.data_ptr(),
                              fc.mom.data_ptr(), None)

    tile_spp, err, rounds = adaptive_loop(T, render, lambda n: errors(fc, n), 2, 2, 6, threshold)
    ca, cm, _ = fc.host()
    assert (tile_spp == 2).any() and (tile_spp > 2).any(), "tiles that stopped at 2 and tiles that went on"
    fd = _Frames(torch, W, H, sa, sm)
    d_spp, res = r.render_adaptive_device(params(0, 6), _lib.AdaptiveParams(2, 2, threshold, FLOOR), fd.acc.data_ptr(),
                                          fd.mom.data_ptr())
    da, dm, _ = fd.host()
    assert same(da, ca) and same(dm, cm) and np.array_equal(d_spp, tile_spp)
    assert res == dict(rounds=rounds, tile_samples=int(tile_spp.sum()), converged_tiles=int((err <= threshold).sum()),
                       total_tiles=T)
    at6 = tile_mask(W, H, np.flatnonzero(tile_spp == 6))
    six = gpu_render(torch, r, sc, cam, DW.settings(spp=6))[0]
    assert at6.any() and same(da[at6], six[at6])


# ---------------------------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("name", ["deep_blocks21_small", "deep_blocks12_small", "deep_prims21_small",
                                  "deep_blocks21_preview", "deep_blocks21_rays"])
def test_deep_golden_fixture(torch_cuda, renderer, name):
    """The GPU reproduces the deep fixtures under test_render_matches_golden_fixture's and
    test_intersect_matches_golden_rays' own rules."""
    if name.endswith("_rays"):
        parity.test_intersect_matches_golden_rays(renderer, name)
    else:
        parity.test_render_matches_golden_fixture(torch_cuda, renderer, name)
