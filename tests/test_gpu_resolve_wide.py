"""Resolve's wave-cooperative read of a grouped chunk's colour records (resolve_pixel_wide): a wave loads
its tile's span of 64 * G records with whole-line loads, K samples per pixel at a time, stages the batch in LDS and
hands each lane its pixel's samples in sample order; the fold is resolve_pixel's.  So a render under
OCTPT_SAMPLE_GROUP = 4 / 16 / 64 still equals the render at G = 1 bit for bit: radiance, per-pixel segment counts,
moments and every statistic of tests/test_gpu_sample_group.py's SAME, whose helpers these tests use.  The G of every
chunk is read from the library's OCTPT_DEBUG line and asserted.

Frames the read can get wrong: 8 x 8 (one tile: one wave of a 256-thread block, three waves past the items), 24 x 8
(three tiles, one idle wave), 60 x 44 (partial tiles: lanes outside the image inside cooperating waves) and 64 x 48.
Sample counts that walk the batch loop: 64, 128 and 192 (one to three sample groups at G = 64), 80 (five groups at
G = 16), 20 (G = 4) and 8 (G = 4 in two groups, runs shorter than the batch of the larger groups); one seed each.
Paths: a progressive continuation, shard 1 of 3 with and without compact buffers, regeneration from a small pool, a
tile list, the moments, clamp and moments + clamp instances and a branch schedule (which stays at G = 1)."""
import numpy as np
import pytest

from tests.adaptive_ref import luminance
from tests.test_gpu_adaptive import _renderer_with, render_full, render_tiles, same
from tests.test_gpu_final import clamped
from tests.test_gpu_parity import gpu_render
from tests.test_gpu_sample_group import (GROUPS, SAME, SMALL_POOL, assert_same, check_all_groups, config,  # noqa: F401
                                         contexts, effective, ran_at, torch_cuda)

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (24, 8), (60, 44), (64, 48)]
SPPS = {64: 11, 128: 12, 192: 13, 80: 14, 20: 15, 8: 16}  # samples -> the seed of its renders


def scene(size, spp):
    sc, cam, rs = config("C2", size, spp)
    rs.seed = SPPS[spp]
    return sc, cam, rs


@pytest.mark.parametrize("spp", list(SPPS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_and_sample_counts(torch_cuda, capfd, contexts, size, spp):
    check_all_groups(torch_cuda, capfd, contexts, *scene(size, spp))


@pytest.mark.parametrize("half", [64, 80, 20])
def test_progressive_continuation(torch_cuda, capfd, contexts, half):
    """two calls of `half` samples, the second from spp_start = half, against one call of both at G = 1"""
    sc, cam, rs = scene((60, 44), half)
    rs.spp = 2 * half
    ref = gpu_render(torch_cuda, contexts(1), sc, cam, rs)
    rs.spp = half
    for g in GROUPS:
        r = contexts(g)
        a, ran_a = ran_at(capfd, lambda: gpu_render(torch_cuda, r, sc, cam, rs))
        b, ran_b = ran_at(capfd, lambda: gpu_render(torch_cuda, r, sc, cam, rs, spp_start=half, accum=a[0]))
        assert ran_a == ran_b == [effective(g, half)], (g, ran_a, ran_b)
        assert_same((b[0], a[1] + b[1], {k: a[2][k] + b[2][k] for k in SAME}), ref, f"G={g}")


@pytest.mark.parametrize("compact", [False, True], ids=["frame", "compact"])
@pytest.mark.parametrize("size,spp", [((60, 44), 128), ((24, 8), 80)], ids=["60x44x128", "24x8x80"])
def test_shard_one_of_three(torch_cuda, capfd, contexts, size, spp, compact):
    check_all_groups(torch_cuda, capfd, contexts, *scene(size, spp), shard=(1, 3), compact=compact)


@pytest.mark.parametrize("spp", [128, 80])
def test_records_of_regenerated_paths(torch_cuda, capfd, contexts, spp):
    sc, cam, rs = scene((60, 44), spp)
    ref = check_all_groups(torch_cuda, capfd, contexts, sc, cam, rs, extra=SMALL_POOL)
    assert ref[2]["pool_slots"] < rs.width * rs.height * rs.spp, "the pool held the chunk: no regeneration"


@pytest.mark.parametrize("spp", [128, 80, 20])
def test_tile_list_and_moments(torch_cuda, capfd, contexts, spp):
    """a tile-list render (the moments instance): the list's tiles in no order, the last column and row overhanging"""
    sc, cam, rs = scene((60, 44), spp)
    tiles = np.array([17, 3, 47, 40, 8, 7], np.uint32)  # of the 8 x 6 tile grid

    def render(r):
        r.set_scene(sc)
        r.set_camera(cam)
        r.reset_stats()
        acc, mom, seg = r.render_tiles(rs, tiles)
        return (acc, seg, r.stats()), mom

    (ref, ref_mom), ran = ran_at(capfd, lambda: render(contexts(1)))
    assert ran == [1], ran
    assert ref[2]["paths"] > 0
    for g in GROUPS:
        (got, mom), ran = ran_at(capfd, lambda: render(contexts(g)))
        assert ran == [effective(g, spp)], (g, ran)
        assert_same(got, ref, f"G={g}")
        assert same(mom, ref_mom), f"G={g}: moments"


@pytest.fixture(scope="module")
def c3_renderers(torch_cuda):
    """G -> a context with tests/test_gpu_adaptive.py's scene, created under OCTPT_SAMPLE_GROUP=G"""
    made = {g: _renderer_with({"OCTPT_SAMPLE_GROUP": str(g)}) for g in (1,) + GROUPS}
    yield made
    for r in made.values():
        r.close()


@pytest.mark.parametrize("spp", [128, 80, 20])
def test_clamp_instances(torch_cuda, capfd, c3_renderers, spp):
    """octpt_render_device under a sample clamp (the clamp instance) and octpt_render_tiles_device with moments under
    it (moments + clamp), on the frame with partial tiles; the clamp is the median pixel luminance of the unclamped
    render, so it acts on some samples and not on others"""
    W, H = 60, 44
    base = c3_renderers[1]
    plain, _ = render_full(torch_cuda, base, W, H, spp)
    l = luminance(plain[..., :3])
    clamp = float(np.float32(np.median(l[l > 0])))
    with clamped(base, clamp):
        (ref_a, ref_s), ran = ran_at(capfd, lambda: render_full(torch_cuda, base, W, H, spp))
        assert ran == [1], ran
        ref_t = render_tiles(torch_cuda, base, W, H, spp, None)
    assert not same(ref_a, plain), "the clamp acted"
    for g in GROUPS:
        r = c3_renderers[g]
        with clamped(r, clamp):
            (a, s), ran = ran_at(capfd, lambda: render_full(torch_cuda, r, W, H, spp))
            assert ran == [effective(g, spp)], (g, ran)
            t, ran = ran_at(capfd, lambda: render_tiles(torch_cuda, r, W, H, spp, None))
            assert ran == [effective(g, spp)], (g, ran)
        assert same(a, ref_a) and np.array_equal(s, ref_s), f"G={g}: clamp"
        assert same(t[0], ref_t[0]) and same(t[1], ref_t[1]) and np.array_equal(t[2], ref_t[2]), f"G={g}: moments + clamp"


def test_branch_schedule_stays_ungrouped(torch_cuda, capfd, contexts):
    sc, cam, rs = config("tiny", (60, 44), 8)
    check_all_groups(torch_cuda, capfd, contexts, sc, cam, rs, branch_count=4)
