"""The first-launch refill threshold of a grouped chunk (OCTPT_REFILL_FIRST): when a chunk runs grouped
(G > 1), its queue holds the seed's camera records (no partial tiles, a pool that holds the chunk) and the launch is
the chunk's first, extend refills a wave once that many lanes are idle instead of by the adaptive rule (0); at 64 a
wave whose lanes are all idle takes a whole claim of 64 positions in lane order (the in-phase path).  Radiance,
per-pixel segment counts and every statistic are sums over rays and a ray's walk is the same whatever lane runs it, so
every threshold renders the adaptive rule's frame bit for bit.

Small frames, seconds each: 64 x 64 at 64 samples (G = 64) and at 16 (G = 16), a scene of 300 spheres and one of 300
cuboids, the beam start on and off.  The policy each chunk's first launch ran is read from the library's OCTPT_DEBUG
line, as tests/test_gpu_sample_group.py reads G, and asserted: the threshold where the three conditions hold, 0 (the
adaptive rule) in a frame with partial tiles, with a pool smaller than the chunk and in a G = 1 chunk.  Each chunk of
a two-chunk render seeds its own camera records, so each one's first launch is a first launch under the rule and runs
the threshold; the frame equals the adaptive one.  A shard of 21 tiles at 16 samples gives segments of 336 positions,
5 claims of 64 and one of 16: the in-phase path must leave the cut claim to the partial refill."""
import os
import re

import numpy as np
import pytest

from tests.test_gpu_parity import REL_TOL_FORWARD, gpu_render, oracle, rel_err, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

THRESHOLDS = (16, 48, 64)
SAME = ("paths", "segments", "esvo_steps", "sphere_tests", "cuboid_tests", "beam_restarts")
SEGS = 64  # the queue's segments (kSegs): segment k holds positions [k * items / 64, (k + 1) * items / 64) of the chunk


@pytest.fixture(scope="module")
def contexts(torch_cuda):
    """renderer(first, beam, extra environment) -> a context created under OCTPT_SAMPLE_GROUP=64 (these chunks are far
    below the size at which the order is grouped by default) and OCTPT_REFILL_FIRST=first, made once per module"""
    from octree_pathtracing_amd.renderer import HipRenderer

    made = {}

    def get(first, beam=True, extra=()):
        key = (first, beam, tuple(sorted(dict(extra).items())))
        if key not in made:
            env = {"OCTPT_SAMPLE_GROUP": "64", "OCTPT_REFILL_FIRST": str(first), "OCTPT_BEAM": "1" if beam else "0",
                   **dict(extra)}
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


@pytest.fixture(scope="module")
def scenes():
    """300 spheres (the sphere extend instance) and 300 cuboids (the cuboid one) in a 64^3 world, C2's view"""
    from octree_pathtracing_amd import scene as S

    out = {}
    for kind in ("spheres", "cuboids"):
        sc = S.Scene()
        ids = S.primitive_materials(sc)
        if kind == "spheres":
            sc.spheres = S.random_spheres(3, 300, 64.0, 0.5, 3.0)
            sc.sphere_material = S._assign_materials(ids, 3, 300)
        else:
            sc.cuboids = S.random_cuboids(3, 300, 64.0, 1.0, 4.0)
            sc.cuboid_material = S._assign_materials(ids, 8, 6 * 300, stream=21).reshape(300, 6)
        sc.build_octree(6)
        out[kind] = (sc, S.Camera.look_at((32.0, 38.0, -28.0), (32.0, 32.0, 32.0)))
    return out


def settings(size, spp):
    from octree_pathtracing_amd.scene import RenderSettings

    return RenderSettings(size[0], size[1], spp, seed=1)


def assert_same(a, b, tag):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{tag}: radiance"
    assert np.array_equal(a[1], b[1]), f"{tag}: segment counts"
    for k in SAME:
        assert a[2][k] == b[2][k], (tag, k, a[2][k], b[2][k])


def ran_at(capfd, render):
    """render() -> (its result, the (G, first-launch threshold) of every chunk it ran: the OCTPT_DEBUG line per chunk)"""
    os.environ["OCTPT_DEBUG"] = "1"  # read at every render call
    try:
        capfd.readouterr()
        out = render()
        err = capfd.readouterr().err
    finally:
        del os.environ["OCTPT_DEBUG"]
    return out, [(int(g), int(f)) for g, f in re.findall(r"sample group (\d+), first-launch refill (\d+)", err)]


@pytest.mark.parametrize("beam", [True, False], ids=["beam", "no-beam"])
@pytest.mark.parametrize("spp", [64, 16], ids=["64spp-G64", "16spp-G16"])
@pytest.mark.parametrize("kind", ["spheres", "cuboids"])
def test_policies_render_the_same_frame(torch_cuda, capfd, contexts, scenes, kind, spp, beam):
    sc, cam = scenes[kind]
    rs = settings((64, 64), spp)
    ref, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(0, beam), sc, cam, rs))
    assert ran == [(spp, 0)], ran
    assert ref[2]["paths"] == 64 * 64 * spp and ref[2]["segments"] > ref[2]["paths"]
    assert ref[2]["sphere_tests" if kind == "spheres" else "cuboid_tests"] > 0
    assert (ref[2]["beam_restarts"] == 0) or beam
    for thr in THRESHOLDS:
        got, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(thr, beam), sc, cam, rs))
        assert ran == [(spp, thr)], (thr, ran)
        assert_same(got, ref, f"{kind} first-launch refill {thr}")


@pytest.mark.parametrize("case,size,spp,extra,group", [
    ("partial-tiles", (60, 44), 64, {}, 64),            # no camera records: tiles overhang the image
    ("small-pool", (64, 64), 64, {"OCTPT_POOL": "4096"}, 64),  # regeneration: the queue holds 48-B ray records
    ("G1-5spp", (64, 64), 5, {}, 1),                    # 5 samples: no G > 1 divides them
])
def test_policy_boundaries(torch_cuda, capfd, contexts, scenes, case, size, spp, extra, group):
    """the threshold is not in effect (the chunk's line reports 0) and the frame is the adaptive rule's"""
    sc, cam = scenes["spheres"]
    rs = settings(size, spp)
    ref, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(0, True, extra), sc, cam, rs))
    assert ran == [(group, 0)], ran
    for thr in (48, 64):
        got, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(thr, True, extra), sc, cam, rs))
        assert ran == [(group, 0)], (case, thr, ran)
        assert_same(got, ref, f"{case} at {thr}")
    if case == "small-pool":
        assert ref[2]["pool_slots"] < rs.width * rs.height * rs.spp, "the pool held the chunk: no regeneration"


def test_two_chunks(torch_cuda, capfd, contexts, scenes):
    """128 samples in two chunks of 64 (OCTPT_CHUNK = 64 x 64 x 64 items): the second chunk continues the first's
    running mean; each chunk's first launch reads that chunk's camera records and runs the threshold, every later
    launch of either chunk the adaptive rule"""
    sc, cam = scenes["spheres"]
    rs = settings((64, 64), 128)
    chunked = {"OCTPT_CHUNK": str(64 * 64 * 64)}
    ref, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(0, True, chunked), sc, cam, rs))
    assert ran == [(64, 0), (64, 0)], ran
    got, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(64, True, chunked), sc, cam, rs))
    assert ran == [(64, 64), (64, 64)], ran
    assert_same(got, ref, "two chunks at 64")
    one, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(0), sc, cam, rs))
    assert ran == [(64, 0)], ran
    assert np.array_equal(one[1], got[1]), "segment counts of one chunk and of two"


def test_claim_cut_by_the_segment_end(torch_cuda, capfd, contexts, scenes):
    """shard 1 of 3 of the 64-tile frame holds 21 tiles: at 16 samples its 64 segments hold 16 x 21 = 336 positions
    each, five claims of 64 and one of 16, and no segment but the first starts on a multiple of 64 items"""
    from octree_pathtracing_amd.renderer import shard_pixels

    sc, cam = scenes["cuboids"]
    rs = settings((64, 64), 16)
    items = shard_pixels(64, 64, 1, 3) * rs.spp
    assert items % SEGS == 0 and items // SEGS == 336 and 336 % 64 == 16, items
    ref, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(0), sc, cam, rs, shard=(1, 3)))
    assert ran == [(16, 0)], ran
    for thr in (48, 64):
        got, ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(thr), sc, cam, rs, shard=(1, 3)))
        assert ran == [(16, thr)], ran
        assert_same(got, ref, f"cut claim at {thr}")


def test_threshold_64_against_the_oracle(torch_cuda, capfd, contexts, scenes):
    sc, cam = scenes["spheres"]
    rs = settings((64, 64), 64)
    (acc, segs, st), ran = ran_at(capfd, lambda: gpu_render(torch_cuda, contexts(64), sc, cam, rs))
    assert ran == [(64, 64)], ran
    racc, rsegs, rst = oracle(sc, cam, rs, forward=True)
    assert np.array_equal(segs, rsegs)
    assert st["segments"] == rst["segments"]
    assert st["esvo_steps"] <= rst["esvo_steps"]  # the beam start skips iterations over empty cells
    assert np.all(np.isfinite(acc))
    e = rel_err(acc, racc)
    assert e.max() <= REL_TOL_FORWARD, f"max rel err {e.max()} at {np.unravel_index(e.argmax(), e.shape)}"
