"""octpt_intersect against the oracle on the batteries of tests/intersect_rays.py: degenerate rays (axis-aligned
with +-0 components, either side of ESVO's direction clamp, tying diagonals from lattice origins, rays in face
planes, sphere limbs, box corners and edges, origins inside primitives and cells, zero directions) and second
segments with the self-intersection key, each sent with key and normal, with the key
alone, and unkeyed.  The bar is this query's own: prim, steps and normal equal, t bit-equal on hits and +inf
on misses.  tests/test_intersect_edges_cpu.py shows on every machine that the batteries hit and miss in every
family and that the key changes the oracle's answer for hundreds of their rays."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import intersect_rays as IR
from tests.test_gpu_multi import multi2  # noqa: F401
from tests.test_gpu_parity import renderer, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

NONE = IR.NONE


def _k_block() -> int:
    src = (Path(__file__).resolve().parents[1] / "octree_pathtracing_amd" / "csrc" / "octpt_internal.h").read_text()
    return int(re.search(r"constexpr\s+uint32_t\s+kBlock\s*=\s*(\d+)\s*;", src).group(1))


def _differ(got, ref):
    t, prim, nrm, steps = got
    rt, rprim, rnrm, rsteps = ref
    return ((prim != rprim) | (steps != rsteps) | (t.view(np.uint32) != rt.view(np.uint32))
            | np.any(nrm != rnrm, axis=1))


def assert_rays_equal(got, ref, rays, tag, families=None, last_prim=None):
    """exact parity per family, the first differing rays spelled out"""
    miss = ref[1] == NONE
    assert np.all(np.isposinf(ref[0][miss])) and np.all(np.isposinf(got[0][got[1] == NONE])), tag
    bad = _differ(got, ref)
    if not bad.any():
        return
    lines = []
    for fam, sl in (families or {"all": slice(0, len(rays))}).items():
        idx = np.flatnonzero(bad[sl]) + sl.start if isinstance(sl, slice) else np.flatnonzero(bad & sl)
        if not len(idx):
            continue
        lines.append(f"{tag}/{fam}: {len(idx)} rays differ")
        for i in idx[:4]:
            key = "" if last_prim is None else f" key {int(last_prim[i]):#x}"
            lines.append(f"  ray {i} o {rays[i, :3].tolist()} d {rays[i, 3:].tolist()}{key}\n"
                         f"    gpu    t {got[0][i]!r} prim {int(got[1][i]):#x} n {got[2][i].tolist()} steps {got[3][i]}\n"
                         f"    oracle t {ref[0][i]!r} prim {int(ref[1][i]):#x} n {ref[2][i].tolist()} steps {ref[3][i]}")
    raise AssertionError("\n".join(lines))


@pytest.mark.parametrize("name", IR.SCENES)
def test_intersect_edge_parity(renderer, name):
    B = IR.battery(name)
    renderer.set_scene(B["scene"])
    assert_rays_equal(renderer.intersect(B["rays"]), B["ref"], B["rays"], name, B["fam"])
    b = B["b"]
    kinds = {d: b["dir"] == j for j, d in enumerate(IR.BOUNCE_DIRS)}
    for mode, lp, ln in (("key+normal", b["last_prim"], b["last_normal"]), ("key", b["last_prim"], None),
                         ("unkeyed", None, None)):
        got = renderer.intersect(b["rays"], lp, ln)
        ref = B[{"key+normal": "ref_kn", "key": "ref_k", "unkeyed": "ref_u"}[mode]]
        assert_rays_equal(got, ref, b["rays"], f"{name}/bounce {mode}", kinds, lp)


@pytest.fixture(scope="module")
def keyed_tiny(renderer):
    """tiny's keyed bounce battery and the device's answers to the whole batch"""
    B = IR.battery("tiny")
    b = B["b"]
    renderer.set_scene(B["scene"])
    full = renderer.intersect(b["rays"], b["last_prim"], b["last_normal"])
    assert_rays_equal(full, B["ref_kn"], b["rays"], "tiny keyed", last_prim=b["last_prim"])
    return b["rays"], b["last_prim"], b["last_normal"], full


def test_batch_size_does_not_change_a_ray(renderer, keyed_tiny):
    """n = 1, kBlock - 1, kBlock + 1 and a prime above 4 k: the bounds guard of the last, partial block"""
    rays, lp, ln, full = keyed_tiny
    kb = _k_block()
    assert kb >= 64 and len(rays) > 4099
    for n in (1, kb - 1, kb + 1, 4099):
        got = renderer.intersect(rays[:n], lp[:n], ln[:n])
        assert_rays_equal(got, tuple(x[:n] for x in full), rays[:n], f"first {n}", last_prim=lp[:n])


def test_lane_and_neighbours_do_not_change_a_ray(renderer, keyed_tiny):
    """reversed and randomly permuted: the LDS stack is indexed by the thread, so a ray's answer must not depend
    on its lane, its block or the rays beside it"""
    rays, lp, ln, full = keyed_tiny
    for tag, perm in (("reversed", np.arange(len(rays))[::-1]),
                      ("permuted", np.random.default_rng(9).permutation(len(rays)))):
        got = renderer.intersect(rays[perm], lp[perm], ln[perm])
        assert_rays_equal(got, tuple(x[perm] for x in full), rays[perm], tag, last_prim=lp[perm])


def test_nullable_arguments(renderer, keyed_tiny):
    """normal = NULL and steps = NULL leave t and prim as they are; last_prim without last_normal and the reverse
    equal the oracle given the same; n = 0 is OK and touches nothing"""
    from octree_pathtracing_amd import _lib
    from oracle import cpu_ref

    rays, lp, ln, full = keyed_tiny
    renderer.set_scene(IR.scene("tiny"))
    n = 3001
    rays, lp, ln = (np.ascontiguousarray(x[:n]) for x in (rays, lp, ln))
    lib, ctx = renderer._lib, renderer._ctx

    def P(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(lp_, ln_, want_normal, want_steps, count=n):
        t, prim = np.full(n, 7.5, np.float32), np.full(n, 0x1234, np.uint32)
        nrm = np.full((n, 3), 7.5, np.float32) if want_normal else None
        steps = np.full(n, 0x1234, np.uint32) if want_steps else None
        assert lib.octpt_intersect(ctx, P(rays), P(lp_), P(ln_), count, P(t), P(prim), P(nrm), P(steps)) == _lib.OK
        return t, prim, nrm, steps

    want = tuple(x[:n] for x in full)
    for want_normal, want_steps in ((False, False), (True, False), (False, True)):
        t, prim, nrm, steps = call(lp, ln, want_normal, want_steps)
        assert np.array_equal(t.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(prim, want[1])
        assert nrm is None or np.array_equal(nrm, want[2])
        assert steps is None or np.array_equal(steps, want[3])
    sc = IR.scene("tiny")
    for lp_, ln_, tag in ((lp, None, "key only"), (None, ln, "normal only")):
        got = call(lp_, ln_, True, True)
        assert_rays_equal(got, cpu_ref.intersect(sc, rays, lp_, ln_), rays, tag, last_prim=lp_)
    t, prim, nrm, steps = call(lp, ln, True, True, count=0)
    assert (t == 7.5).all() and (prim == 0x1234).all() and (nrm == 7.5).all() and (steps == 0x1234).all()
    assert lib.octpt_intersect(ctx, None, None, None, 0, None, None, None, None) == _lib.OK


def test_multi_device_context_keyed(renderer, multi2, keyed_tiny):
    """a two-entry context (octpt_create_multi over [0, 0]) answers the keyed bounce battery as one device does"""
    rays, lp, ln, full = keyed_tiny
    renderer.set_scene(IR.scene("tiny"))
    multi2.set_scene(IR.scene("tiny"))
    assert_rays_equal(multi2.intersect(rays, lp, ln), full, rays, "multi2 keyed", last_prim=lp)
    assert_rays_equal(multi2.intersect(rays, lp), renderer.intersect(rays, lp), rays, "multi2 key only", last_prim=lp)
