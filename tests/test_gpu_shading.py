"""Shading on the device across the material, alpha, ior, emission and sun parameter space.

The cases are tests/shading_cases.py's; each has finished in the CPU oracle and reached the branches it exists
for (tests/test_shading_cpu.py) before it is rendered here.  The device keeps no branch counters: the parity
bar (per-pixel segment counts, ESVO-step, primitive-test and shade totals equal, radiance within
REL_TOL_FORWARD) makes the oracle's branch counts the kernel's.  The furnace is held against its closed form
directly, not against the oracle.
"""
import os

import numpy as np
import pytest

from tests import shading_cases as C
from tests.test_gpu_beam import _same as beam_same, beam  # noqa: F401
from tests.test_gpu_lean import _same as lean_same, full_state  # noqa: F401
from tests.test_gpu_parity import REL_TOL_FORWARD, assert_parity, gpu_render, oracle, renderer, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


# -------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(C.CASES))
def test_case_parity(torch_cuda, renderer, name):
    sc, cam, rs, _ = C.built(name)
    assert_parity(gpu_render(torch_cuda, renderer, sc, cam, rs), C.oracle_of(name), name)


@pytest.mark.parametrize("seed", C.FUZZ_SEEDS)
def test_fuzz_parity(torch_cuda, renderer, seed):
    sc, cam, rs, tag = C.fuzz_built(seed)
    assert_parity(gpu_render(torch_cuda, renderer, sc, cam, rs), C.fuzz_oracle_of(seed), tag)


# ------------------------------------------------------------------------------------------------- furnace
@pytest.mark.parametrize("shape", ["sphere", "cuboid"])
@pytest.mark.parametrize("name", list(C.FURNACE))
def test_furnace_matches_closed_form(torch_cuda, renderer, name, shape):
    """the assertions of tests/test_shading_cpu.py's furnace on the device's render: the closed form, not the oracle"""
    kw = C.FURNACE[name]
    spp = 32
    sc, cam, rs = C.furnace_scene(shape, spp=spp, **kw)
    acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, rs)
    mask_segs = None
    if C.furnace_mask_kw(kw) is not kw:  # a partial-alpha case takes its pixels from the opaque twin's render
        mask_segs = gpu_render(torch_cuda, renderer, *C.furnace_scene(shape, spp=spp, **C.furnace_mask_kw(kw)))[1]
    n_pix, worst = C.furnace_check(acc, segs, spp, kw, REL_TOL_FORWARD, mask_segs=mask_segs)
    print(f"furnace {name}/{shape}: {n_pix} pixels, worst deviation / allowance {worst:.3f}")


# ---------------------------------------------------------------------------------------------- megakernel
@pytest.mark.parametrize("name", [names[0] for names in C.GROUPS.values()] + ["alpha_tinted_glass_hq",
                                                                              "ior_overlap_unequal"])
def test_megakernel_equals_wavefront(torch_cuda, renderer, name):
    sc, cam, rs, _ = C.built(name)
    a = gpu_render(torch_cuda, renderer, sc, cam, rs, megakernel=False)
    b = gpu_render(torch_cuda, renderer, sc, cam, rs, megakernel=True)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    for k in ("paths", "segments", "esvo_steps", "sphere_tests", "cuboid_tests", "shade_events"):
        assert a[2][k] == b[2][k], k


# ------------------------------------------------------------------------------------ lean vs full path state
def lean_rule(sc):
    """enqueue_wavefront's rule, scene part (octpt_api.cpp): the lean state applies when nothing adds light before
    a path's end -- no material with emittance > RAY_EPSILON while emitters are enabled, and no sun sampling"""
    emissive = sc.emitters_enabled and any(np.float32(m.emittance) > np.float32(C.RAY_EPSILON) for m in sc.materials)
    return not emissive and not sc.strategy.sun_sampling


@pytest.mark.parametrize("name", C.EMITTER_CASES)
def test_lean_equals_full(torch_cuda, renderer, full_state, name):
    """The emitter cases through the lean mechanism (OCTPT_LEAN=0 forces the 40-B state): bit-identical, statistics
    included.  Which state the default context chose is not observable through the C ABI; what is pinned is that
    a scene on either side of the rule renders the same in both, and against the oracle (test_case_parity): a
    lean instance chosen for a scene that adds light mid-path would drop that light (kLean shade_segment has no
    emission term) and fail both."""
    sc, cam, rs, _ = C.built(name)
    assert lean_rule(sc) == (name in ("emit_disabled", "eps_at"))
    lean_same(gpu_render(torch_cuda, renderer, sc, cam, rs), gpu_render(torch_cuda, full_state, sc, cam, rs), name)


# ------------------------------------------------------------------------------------- sun cases across modes
@pytest.mark.parametrize("name", C.SUN_CASES)
def test_sun_preview(torch_cuda, renderer, name):
    """the preview's flat shading uses the sun direction and emittance: bit-exact against the oracle's preview"""
    sc, cam, rs, _ = C.built(name)
    pre = np.random.default_rng(3).random((rs.height, rs.width, 4), dtype=np.float32)
    acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, rs, accum=pre, preview=True)
    racc, rsegs, rst = oracle(sc, cam, rs, accum=pre.copy(), preview=True)
    assert np.array_equal(segs, rsegs)
    assert st["segments"] == rst["segments"] and st["esvo_steps"] == rst["esvo_steps"]
    assert np.array_equal(acc, racc), f"{name}: max abs diff {np.abs(acc - racc).max()}"
    assert np.array_equal(acc[..., 3], pre[..., 3])


@pytest.mark.parametrize("name", C.SUN_CASES)
def test_sun_branch_count(torch_cuda, renderer, name):
    """branch_count = 4 over 8 spp (passes 1, 1, 1, 1, 4) against the oracle's schedule"""
    from dataclasses import replace

    sc, cam, rs, _ = C.built(name)
    rs = replace(rs, spp=8)
    acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, rs, branch_count=4)
    racc, rsegs, rst = oracle(sc, cam, rs, forward=True, branch_count=4)
    assert np.array_equal(segs, rsegs), f"{name}: segment counts differ at {np.argwhere(segs != rsegs)[:5]}"
    assert st["paths"] >= rst["paths"] and st["segments"] >= rst["segments"]
    assert np.all(np.isfinite(acc))
    e = np.abs(acc - racc) / np.maximum(np.abs(racc), 1e-3)
    assert e.max() <= REL_TOL_FORWARD, f"{name}: max rel err {e.max()}"


@pytest.mark.parametrize("name", C.SUN_CASES)
def test_sun_beam(torch_cuda, renderer, beam, name):
    sc, cam, rs, _ = C.built(name)
    beam_same(gpu_render(torch_cuda, beam, sc, cam, rs), gpu_render(torch_cuda, renderer, sc, cam, rs))


# ---------------------------------------------------------------------------------------------- small pool
@pytest.fixture(scope="module")
def small_pool(torch_cuda):
    """a 100-path pool, refill at 1, 2000-item chunks (tests/test_gpu_parity.py's small-pool settings)"""
    from octree_pathtracing_amd.renderer import HipRenderer

    env = {"OCTPT_POOL": "100", "OCTPT_REFILL": "1", "OCTPT_CHUNK": "2000"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # read when the context is created
    try:
        r = HipRenderer(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    yield r
    r.close()


@pytest.mark.parametrize("name", C.PARTIAL_ALPHA_HQ)
def test_partial_alpha_small_pool(torch_cuda, renderer, small_pool, name):
    """A path waits in a shadow chain through partial-alpha occluders across refills and chunks, its saved
    bounce state packed and unpacked: bit-identical to the whole-frame pool."""
    sc, cam, rs, _ = C.built(name)
    a = gpu_render(torch_cuda, renderer, sc, cam, rs)
    b = gpu_render(torch_cuda, small_pool, sc, cam, rs)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    for k in ("paths", "segments", "esvo_steps", "shade_events"):
        assert a[2][k] == b[2][k], k
