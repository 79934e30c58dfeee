"""The chunk's item order (item_split): a wave of a chunk's first launch holds G samples of each of
64 / G pixels of one tile (OCTPT_SAMPLE_GROUP gives the largest G allowed; each chunk takes the largest allowed G
that divides its sample count; 1 is one sample of the whole 8x8 tile).  A path's random numbers are keyed by
(seed, pixel, sample), resolve folds a pixel's samples in sample order and every statistic is a sum over rays, so a
render at any G equals the render at G = 1 bit for bit: radiance, per-pixel segment counts and every statistic.

Small frames, seconds each, at 16 samples (G = 16 at most) and at 64 (every G in effect; the G each chunk ran at is
read from the library's OCTPT_DEBUG line and asserted): the direct seed with its 16-B camera records (64 x 48),
overhanging tiles (60 x 44), sample counts that lower G (20 -> 4, 5 -> 1), regeneration from a pool smaller than the
chunk, a progressive split, a shard with and without compact buffers, a tile list, sun sampling (the 40-B state),
block values and a branch schedule (which keeps G = 1).

Without the variable the order is grouped (G = 4 at most) only in sphere / cuboid scenes and in chunks of at least
2^27 items (enqueue_wavefront's rule): test_default_rule."""
import os
import re

import numpy as np
import pytest

from tests.test_gpu_parity import gpu_render, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

GROUPS = (4, 16, 64)
SAME = ("paths", "segments", "esvo_steps", "sphere_tests", "cuboid_tests", "block_tests", "shade_events",
        "texel_reads", "beam_restarts")
SMALL_POOL = {"OCTPT_POOL": "4096"}  # the knob of tests/test_gpu_drain.py's small-pool context, below these chunks


@pytest.fixture(scope="module")
def contexts(torch_cuda):
    """renderer(G, extra environment) -> a context created under OCTPT_SAMPLE_GROUP=G, made once per module"""
    from octree_pathtracing_amd.renderer import HipRenderer

    made = {}

    def get(group, extra=()):
        key = (group, tuple(sorted(dict(extra).items())))
        if key not in made:
            env = {"OCTPT_SAMPLE_GROUP": "" if group is None else str(group), **dict(extra)}  # "": as unset
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)  # read when the context is created
            try:
                made[key] = HipRenderer(device=0)
            finally:
                for k, v in old.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
        return made[key]

    yield get
    for r in made.values():
        r.close()


def config(name, size=None, spp=None, variant=None):
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config(name)
    if size:
        rs.width, rs.height = size
    if spp:
        rs.spp = spp
    if variant:
        S.with_sun_variant(sc, variant)
    return sc, cam, rs


def assert_same(a, b, tag):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{tag}: radiance"
    assert np.array_equal(a[1], b[1]), f"{tag}: segment counts"
    for k in SAME:
        assert a[2][k] == b[2][k], (tag, k, a[2][k], b[2][k])


def effective(most, spp, branch_count=1):
    """the G a chunk of spp samples runs at under OCTPT_SAMPLE_GROUP=most (enqueue_wavefront's choice, restated)"""
    if branch_count > 1:
        return 1
    return max(g for g in (1, 4, 16, 64) if g <= most and spp % g == 0)


def ran_at(capfd, render):
    """render() -> (its result, the G of every chunk it ran: the library's OCTPT_DEBUG line per chunk)"""
    os.environ["OCTPT_DEBUG"] = "1"  # read at every render call
    try:
        capfd.readouterr()
        out = render()
        err = capfd.readouterr().err
    finally:
        del os.environ["OCTPT_DEBUG"]
    return out, [int(g) for g in re.findall(r"sample group (\d+)", err)]


def check_all_groups(torch, capfd, contexts, sc, cam, rs, extra=(), branch_count=1, **kw):
    """every G against G = 1; each render ran one chunk, at the G its sample count allows"""
    kw["branch_count"] = branch_count
    ref, ran = ran_at(capfd, lambda: gpu_render(torch, contexts(1, extra), sc, cam, rs, **kw))
    assert ran == [1], ran
    assert ref[2]["paths"] > 0 and ref[2]["segments"] >= ref[2]["paths"]
    for g in GROUPS:
        got, ran = ran_at(capfd, lambda: gpu_render(torch, contexts(g, extra), sc, cam, rs, **kw))
        assert ran == [effective(g, rs.spp, branch_count)], (g, ran)
        assert_same(got, ref, f"G={g}")
    return ref


@pytest.mark.parametrize("size,spp", [((64, 48), 16), ((64, 48), 64), ((64, 48), 20), ((64, 48), 5), ((60, 44), 16),
                                      ((60, 44), 64)],
                         ids=["64x48x16", "64x48x64-G64", "64x48x20-G4", "64x48x5-G1", "60x44x16-partial-tiles",
                              "60x44x64-partial-tiles-G64"])
def test_sphere_scene(torch_cuda, capfd, contexts, size, spp):
    sc, cam, rs = config("C2", size, spp)
    check_all_groups(torch_cuda, capfd, contexts, sc, cam, rs)


@pytest.mark.parametrize("spp", [16, 64])
def test_regeneration_from_a_small_pool(torch_cuda, capfd, contexts, spp):
    sc, cam, rs = config("C2", (64, 48), spp)
    ref = check_all_groups(torch_cuda, capfd, contexts, sc, cam, rs, extra=SMALL_POOL)
    assert ref[2]["pool_slots"] < rs.width * rs.height * rs.spp, "the pool held the chunk: no regeneration"
    assert_same(gpu_render(torch_cuda, contexts(64), sc, cam, rs), ref, "whole-chunk pool against the small pool")


@pytest.mark.parametrize("half", [8, 64])
def test_progressive_split(torch_cuda, capfd, contexts, half):
    """half + half samples in two calls against both halves in one call at G = 1 (8 + 8: the chunks allow G <= 4;
    64 + 64: every G in effect)"""
    sc, cam, rs = config("C2", (64, 48), 2 * half)
    ref = gpu_render(torch_cuda, contexts(1), sc, cam, rs)
    rs.spp = half
    for g in GROUPS:
        r = contexts(g)
        a, ran_a = ran_at(capfd, lambda: gpu_render(torch_cuda, r, sc, cam, rs))
        b, ran_b = ran_at(capfd, lambda: gpu_render(torch_cuda, r, sc, cam, rs, spp_start=half, accum=a[0]))
        assert ran_a == ran_b == [effective(g, half)], (g, ran_a, ran_b)
        both = (b[0], a[1] + b[1], {k: a[2][k] + b[2][k] for k in SAME})
        assert_same(both, ref, f"G={g}")


@pytest.mark.parametrize("compact", [False, True], ids=["frame", "compact"])
@pytest.mark.parametrize("spp", [16, 64])
def test_shard_one_of_three(torch_cuda, capfd, contexts, compact, spp):
    sc, cam, rs = config("C2", (64, 48), spp)
    check_all_groups(torch_cuda, capfd, contexts, sc, cam, rs, shard=(1, 3), compact=compact)


@pytest.mark.parametrize("spp", [16, 64])
def test_tile_list(torch_cuda, contexts, spp):
    sc, cam, rs = config("C2", (64, 48), spp)
    tiles = np.array([17, 3, 40, 8, 47], np.uint32)  # of the 8 x 6 tile grid, in no order

    def render(r):
        r.set_scene(sc)
        r.set_camera(cam)
        r.reset_stats()
        acc, mom, seg = r.render_tiles(rs, tiles)
        return (acc, seg, r.stats()), mom

    ref, ref_mom = render(contexts(1))
    assert ref[2]["paths"] == len(tiles) * 64 * rs.spp
    for g in GROUPS:
        got, mom = render(contexts(g))
        assert_same(got, ref, f"G={g}")
        assert np.array_equal(mom.view(np.uint32), ref_mom.view(np.uint32)), f"G={g}: moments"


@pytest.mark.parametrize("spp", [16, 64])
def test_sun_sampling(torch_cuda, capfd, contexts, spp):
    sc, cam, rs = config("C2", (64, 48), spp, variant="nee_importance")
    check_all_groups(torch_cuda, capfd, contexts, sc, cam, rs)


@pytest.mark.parametrize("spp", [16, 64])
def test_block_values(torch_cuda, capfd, contexts, spp):
    sc, cam, rs = config("blocks-b", (64, 48), spp)
    ref = check_all_groups(torch_cuda, capfd, contexts, sc, cam, rs)
    assert ref[2]["block_tests"] > 0


def test_branch_schedule_keeps_one_sample_per_wave(torch_cuda, capfd, contexts):
    sc, cam, rs = config("tiny", (64, 48), 8)
    check_all_groups(torch_cuda, capfd, contexts, sc, cam, rs, branch_count=4)


def test_default_rule(torch_cuda, capfd, contexts):
    """OCTPT_SAMPLE_GROUP unset: G = 4 in a sphere scene's chunk of >= 2^27 items, 1 in a smaller chunk and in a
    block-value scene; the large frame equals its G = 1 render"""
    auto = contexts(None)
    sc, cam, rs = config("C2", (64, 48), 16)
    _, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, auto, sc, cam, rs))
    assert ran == [1], ran
    sb, camb, rsb = config("blocks-b", (64, 48), 16)
    _, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, auto, sb, camb, rsb))
    assert ran == [1], ran
    rs.width, rs.height, rs.spp = 1280, 720, 148  # 136.4 M items >= 2^27, 148 = 4 * 37: G = 4
    got, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, auto, sc, cam, rs))
    assert ran == [4], ran
    assert_same(got, gpu_render(torch_cuda, contexts(1), sc, cam, rs), "default against G = 1")
