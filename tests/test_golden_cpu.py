"""The oracle reproduces the committed golden fixtures (tests/golden/, written by make_golden.py)
bit for bit: renders (float radiance, per-pixel segment counts, work counters) and closest-hit
queries.  A change of the oracle's arithmetic shows up here before it reaches a parity claim."""
import json
from pathlib import Path

import numpy as np
import pytest

from oracle import cpu_ref
from octree_pathtracing_amd import scene as S

GOLDEN = Path(__file__).resolve().parent / "golden"
RENDERS = ["c1_as_is", "c1", "tiny", "c2_small", "c3_small", "c4_small", "c5_small", "c3_preview", "c4_preview",
           "c5_preview", "tiny_fast", "c2_hq", "c4_hq_sss", "c5_nee_importance", "blocks_small", "blocks_preview", "tiny_branch10",
           "blocks_branch10",
           # octree depths 12 and 21 (tests/deep_worlds.py): their metadata names a generator case, not a config
           "deep_blocks21_small", "deep_blocks12_small", "deep_prims21_small", "deep_blocks21_preview"]
STAT_KEYS = ("paths", "segments", "esvo_steps", "node_fetches", "prim_tests", "leaf_visits", "shade_events",
             "texel_reads", "max_path_segs")


def load(name):
    return np.load(GOLDEN / f"{name}.npz", allow_pickle=False)


def fixture_scene(m):
    """(scene, camera) of a fixture's metadata: a make_config name under "config", or a tests/deep_worlds.py case
    under "generator" (the worlds at octree depths 12-21, which are no configs)."""
    if "generator" in m:
        from tests import deep_worlds as DW

        return DW.case(m["generator"])[:2]
    sc, cam, _ = S.make_config(m["config"])
    if "sun_variant" in m:
        S.with_sun_variant(sc, m["sun_variant"])
    return sc, cam


@pytest.mark.parametrize("name", RENDERS)
def test_oracle_reproduces_render_fixture(name):
    g = load(name)
    m = json.loads(str(g["meta"]))
    sc, cam = fixture_scene(m)
    acc, seg, st = cpu_ref.render(sc, cam, m["width"], m["height"], m["spp"], max_depth=m["max_depth"],
                                  seed=m["seed"], forward=m["forward"], threads=8, preview=m.get("preview", False),
                                  branch_count=m.get("branch_count", 1))
    assert np.array_equal(seg, g["segcount"])
    assert np.array_equal(acc, g["accum"])
    assert [st[k] for k in STAT_KEYS] == g["stats"].tolist()


def test_c1_as_is_is_sky_only():
    g = load("c1_as_is")
    st = dict(zip(STAT_KEYS, g["stats"].tolist()))
    assert st["prim_tests"] == 0 and st["leaf_visits"] == 0  # empty octree: every primary ray misses
    assert np.all(g["segcount"] == 1)
    acc = g["accum"]
    assert np.all(acc[..., 3] == 1.0) and np.all(acc[..., :3] > 0)


@pytest.mark.parametrize("name", ["c3_rays", "deep_blocks21_rays"])
def test_oracle_reproduces_ray_fixture(name):
    g = load(name)
    sc = fixture_scene(json.loads(str(g["meta"])) if "meta" in g else {"config": "C3"})[0]
    t, prim, nrm, steps = cpu_ref.intersect(sc, g["rays"])
    assert np.array_equal(prim, g["prim"]) and np.array_equal(t, g["t"])
    assert np.array_equal(nrm, g["normal"]) and np.array_equal(steps, g["steps"])
    assert 0.2 < (prim != 0xFFFFFFFF).mean() < 0.95  # a mix of hits and misses
