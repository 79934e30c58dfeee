"""GPU parity: liboctpt (gfx950) vs the CPU oracle on identical scenes and seeds.

Bar: control flow is compared exactly (per-pixel ray-segment counts and the
ESVO step / primitive-test totals are integers and must be equal); radiance is compared with
max relative error <= 1e-5 per channel against the oracle's forward-accumulation mode (the
kernel's order) and <= 1e-4 against the recursive (reference-order) mode.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL_FORWARD = 1e-5
REL_TOL_RECURSIVE = 1e-4


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd.renderer import HipRenderer

    r = HipRenderer(device=0)
    yield r
    r.close()


def rel_err(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-3)


def gpu_render(torch, r, sc, cam, rs, spp_start=0, accum=None, shard=(0, 1), compact=False, megakernel=False,
               preview=False, branch_count=1, upload=True):
    """Device render through octpt_render_device; returns (accum[H,W,4] or compact, seg_count, stats).
    upload=False: render the scene already on the context (octpt_scene_build_device)."""
    from octree_pathtracing_amd.renderer import shard_pixels

    if upload:
        r.set_scene(sc)
    r.set_camera(cam)
    r.max_depth, r.seed = rs.max_depth, rs.seed
    r.branch_count = branch_count
    r.reset_stats()
    W, H = rs.width, rs.height
    n = shard_pixels(W, H, *shard) if compact else W * H
    if accum is None:
        acc = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        acc[:, 3] = 1.0
    else:
        acc = torch.as_tensor(accum.reshape(-1, 4), device="cuda").clone()
    segs = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = r.params(W, H, spp_start, rs.spp, shard[0], shard[1], compact, megakernel, preview=preview)
    stream = torch.cuda.current_stream().cuda_stream
    r.render_device(p, acc.data_ptr(), segs.data_ptr(), stream)
    torch.cuda.synchronize()
    st = r.stats()
    a = acc.cpu().numpy()
    s = segs.cpu().numpy().view(np.uint32)
    if not compact:
        a = a.reshape(H, W, 4)
        s = s.reshape(H, W)
    return a, s, st


def oracle(sc, cam, rs, **kw):
    from oracle import cpu_ref

    return cpu_ref.render(sc, cam, rs.width, rs.height, rs.spp, max_depth=rs.max_depth, seed=rs.seed, **kw)


def assert_parity(gpu, ref, tag):
    acc, segs, st = gpu
    racc, rsegs, rst = ref
    assert np.array_equal(segs, rsegs), f"{tag}: per-pixel segment counts differ at {np.argwhere(segs != rsegs)[:5]}"
    assert st["segments"] == rst["segments"], tag
    assert st["esvo_steps"] == rst["esvo_steps"], tag
    assert st["sphere_tests"] + st["cuboid_tests"] == rst["prim_tests"], tag
    assert st.get("block_tests", 0) == rst.get("block_tests", 0), tag  # block-value leaves (C23)
    assert st["shade_events"] == rst["shade_events"], tag
    assert np.all(np.isfinite(acc)), tag
    e = rel_err(acc, racc)
    assert e.max() <= REL_TOL_FORWARD, f"{tag}: max rel err {e.max()} at {np.unravel_index(e.argmax(), e.shape)}"
    return float((acc == racc).mean())


@pytest.mark.parametrize("name,res", [("tiny", None), ("C1", None), ("C1-as-is", None), ("C2", (160, 90, 8)),
                                      ("C3", (192, 108, 2)), ("C4", (128, 72, 2)), ("C5", (192, 108, 2)),
                                      ("blocks", None)])
def test_render_parity(torch_cuda, renderer, name, res):
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config(name)
    if res:
        rs.width, rs.height, rs.spp = res
    gpu = gpu_render(torch_cuda, renderer, sc, cam, rs)
    ref = oracle(sc, cam, rs, forward=True)
    exact = assert_parity(gpu, ref, name)
    assert exact > 0.999, f"{name}: only {exact:.4%} of channels bit-identical"
    rec = oracle(sc, cam, rs, forward=False)
    assert rel_err(gpu[0], rec[0]).max() <= REL_TOL_RECURSIVE


def test_c1_as_is_is_sky_only(torch_cuda, renderer):
    """With Scene::hit stubbed (reference today) every pixel is sky (0.5, 0.7, 1.0) + optional sun."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config("C1-as-is")
    acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, rs)
    assert np.all(segs == 1)
    sky = np.array([0.5, 0.7, 1.0], np.float32)
    diff = acc[..., :3] - sky
    assert np.all((np.abs(diff).max(-1) == 0) | (diff.min(-1) > 1.0))  # sun adds > 1


def test_progressive_split_is_identical(torch_cuda, renderer):
    """Two calls of 2 spp == one call of 4 spp, bit for bit (per-pixel running mean order)."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config("tiny")
    full = gpu_render(torch_cuda, renderer, sc, cam, rs)[0]
    rs.spp = 2
    half = gpu_render(torch_cuda, renderer, sc, cam, rs)[0]
    two = gpu_render(torch_cuda, renderer, sc, cam, rs, spp_start=2, accum=half)[0]
    assert np.array_equal(full, two)


def test_shards_union_equals_full(torch_cuda, renderer):
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import shard_pixels

    torch = torch_cuda
    sc, cam, rs = S.make_config("tiny")
    rs.width, rs.height = 70, 45  # ragged tiles on both axes
    full = gpu_render(torch, renderer, sc, cam, rs)[0]
    N = 3
    stride = max(shard_pixels(rs.width, rs.height, i, N) for i in range(N))
    buf = torch.zeros((N * stride, 4), dtype=torch.float32, device="cuda")
    for i in range(N):
        a = gpu_render(torch, renderer, sc, cam, rs, shard=(i, N), compact=True)[0]
        buf[i * stride:i * stride + len(a)] = torch.as_tensor(a, device="cuda")
    frame = torch.zeros((rs.height * rs.width, 4), dtype=torch.float32, device="cuda")
    renderer.unshard_device(rs.width, rs.height, N, buf.data_ptr(), stride, frame.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().reshape(rs.height, rs.width, 4), full)


def test_intersect_parity(renderer):
    from octree_pathtracing_amd import scene as S
    from oracle import cpu_ref

    for name in ("tiny", "C3", "blocks"):
        sc, cam, rs = S.make_config(name)
        renderer.set_scene(sc)
        rng = np.random.default_rng(7)
        n = 20000
        world = float(2 ** sc.octree.depth)
        o = rng.uniform(-0.2 * world, 1.2 * world, (n, 3)).astype(np.float32)
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.concatenate([o, d], 1).astype(np.float32)
        t, prim, nrm, steps = renderer.intersect(rays)
        rt, rprim, rnrm, rsteps = cpu_ref.intersect(sc, rays)
        assert np.array_equal(prim, rprim), name
        assert np.array_equal(steps, rsteps), name
        hit = prim != 0xFFFFFFFF
        assert hit.mean() > 0.05, name
        assert np.array_equal(t[hit], rt[hit]) and np.array_equal(nrm, rnrm), name


def test_intersect_unsupported_rays_are_misses(renderer):
    """A ray with a non-finite component or a direction component above 2^126 is a miss, and the batch's other
    rays are traced exactly as without it.  Non-finite rays miss in the reference too; a finite component above
    2^126 missing is a deliberate deviation (the reference would walk on a subnormal t_coef,
    octree_traversal.rs:95, and might hit): parity unpinned, no reference fixture covers it."""
    from octree_pathtracing_amd import scene as S
    from oracle import cpu_ref

    sc, _, _ = S.make_config("C3")
    renderer.set_scene(sc)
    rng = np.random.default_rng(11)
    n = 4096
    world = float(2 ** sc.octree.depth)
    o = rng.uniform(0.1 * world, 0.9 * world, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], 1).astype(np.float32)
    want = cpu_ref.intersect(sc, rays)
    bad = rays.copy()
    bad_rows = [3, 100, 101, 2000, n - 1]
    bad[3, 0] = np.nan
    bad[100, 4] = np.inf
    bad[101, 5] = -np.inf
    bad[2000, 3] = 2.0 ** 127
    bad[n - 1, 1] = -np.inf
    t, prim, nrm, steps = renderer.intersect(bad)
    keep = np.setdiff1d(np.arange(n), bad_rows)
    assert np.all(np.isposinf(t[bad_rows])) and np.all(prim[bad_rows] == 0xFFFFFFFF)
    assert np.all(nrm[bad_rows] == 0) and np.all(steps[bad_rows] == 0)
    assert np.array_equal(prim[keep], want[1][keep]) and np.array_equal(steps[keep], want[3][keep])
    hit = keep[want[1][keep] != 0xFFFFFFFF]
    assert len(hit) > 100 and np.array_equal(t[hit], want[0][hit]) and np.array_equal(nrm[keep], want[2][keep])


def test_tonemap_parity(torch_cuda, renderer):
    from oracle import cpu_ref

    torch = torch_cuda
    rng = np.random.default_rng(3)
    acc = rng.uniform(-0.5, 3.0, (4096, 4)).astype(np.float32)
    acc[:5] = [[np.nan, 0, 1, 1], [np.inf, -np.inf, 0.5, 2], [1e-9, 254.9 / 255, 255 / 255, 0], [0, 0, 0, 1],
               [0.0039, 0.5, 0.99, 0.5]]
    a = torch.as_tensor(acc, device="cuda")
    out = torch.zeros((4096, 4), dtype=torch.uint8, device="cuda")
    renderer.tonemap_device(a.data_ptr(), out.data_ptr(), 4096, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), cpu_ref.tonemap(acc))


def test_async_frame_and_cancel(renderer):
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import FrameInFlightPoll

    sc, cam, rs = S.make_config("tiny")
    renderer.set_scene(sc)
    renderer.set_camera(cam)
    renderer.set_resolution((rs.width, rs.height))
    renderer.max_depth, renderer.seed = rs.max_depth, rs.seed
    f = renderer.render_frame(spp_count=rs.spp)
    while True:
        state, payload = f.poll()
        if state is not FrameInFlightPoll.NotReady:
            break
    assert state is FrameInFlightPoll.Ready
    assert renderer.get_current_spp() == rs.spp
    sync, rgba = renderer.render(rs, with_rgba=True)
    assert np.array_equal(payload, rgba)
    assert np.array_equal(renderer.get_float_image(), sync)
    f2 = renderer.render_frame(spp_count=64)
    f2.cancel()
    while True:
        state, payload = f2.poll()
        if state is not FrameInFlightPoll.NotReady:
            break
    assert state is FrameInFlightPoll.Cancelled and payload is None
    assert renderer.get_current_spp() == rs.spp  # a cancelled frame does not advance the render


def test_validation_errors(renderer):
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config("tiny")
    bad = S.make_config("tiny")[0]
    bad.octree.octant_children = bad.octree.octant_children.copy()
    leafy = np.argwhere((bad.octree.octant_mask >> 8) != 0)[0][0]
    c = int(np.argwhere((bad.octree.octant_mask[leafy] >> (8 + np.arange(8))) & 1)[0][0])
    bad.octree.octant_children[leafy, c] = 10 ** 8
    with pytest.raises(_lib.OctptError) as e:
        renderer.set_scene(bad)
    assert e.value.status == _lib.ERR_INVALID_ARG
    for fault in ("stretched", "model_index"):  # block-model instances (C19)
        blk = S.make_config("blocks")[0]
        mi = int(np.nonzero(blk.cuboid_model != _lib.MODEL_NONE)[0][0])
        if fault == "stretched":
            blk.cuboids = blk.cuboids.copy()
            blk.cuboids[mi, 4] += 0.5  # a model instance must be a unit voxel
        else:
            blk.cuboid_model = blk.cuboid_model.copy()
            blk.cuboid_model[mi] = len(blk.models)
        with pytest.raises(_lib.OctptError) as e:
            renderer.set_scene(blk)
        assert e.value.status == _lib.ERR_INVALID_ARG, fault
    renderer.set_scene(sc)  # branch-count validation: test_branch_count_validation


@pytest.mark.parametrize("case", ["one_pixel", "ragged", "empty_scene", "inside_sphere", "glass_only",
                                  "cuboids_textured", "emitters"])
def test_edge_cases(torch_cuda, renderer, case):
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config("tiny")
    if case == "one_pixel":
        rs.width = rs.height = 1
        rs.spp = 16
    elif case == "ragged":
        rs.width, rs.height = 37, 19
    elif case == "empty_scene":
        sc.spheres = sc.spheres[:0]
        sc.sphere_material = sc.sphere_material[:0]
        sc.cuboids = sc.cuboids[:0]
        sc.cuboid_material = sc.cuboid_material[:0]
        sc.build_octree(5)
    elif case == "inside_sphere":
        cam = S.Camera.look_at(tuple(map(float, sc.spheres[0, :3])), (16.0, 16.0, 16.0))
    elif case == "glass_only":
        ids = S.primitive_materials(sc)
        sc.sphere_material[:] = ids["glass"]
        sc.cuboid_material[:] = ids["glass"]
        rs.max_depth = 8
    elif case == "cuboids_textured":
        tex = np.random.default_rng(5).integers(0, 256, (16, 16, 4), dtype=np.uint8)
        tex[..., 3] = np.where(tex[..., 3] < 40, 0, 255)  # transparent texels exercise the skip rule
        sc.textures.append(S.Texture.image(tex))
        sc.materials.append(S.Material(texture_index=len(sc.textures) - 1))
        sc.cuboid_material[:] = len(sc.materials) - 1
        sc.sphere_material[::3] = len(sc.materials) - 1
    elif case == "emitters":
        sc.materials[1].emittance = 5.0
    gpu = gpu_render(torch_cuda, renderer, sc, cam, rs)
    ref = oracle(sc, cam, rs, forward=True)
    assert_parity(gpu, ref, case)


@pytest.mark.parametrize("name,spp", [("C3", 2), ("C4", 1), ("C5", 1)])
def test_fullframe_oracle(torch_cuda, renderer, name, spp):
    """The benchmark configs at full size (C3 1920x1080, C4 / C5 3840x2160) against the oracle over the
    WHOLE frame: per-pixel segment counts and the ESVO / primitive-test / shade totals exact, radiance
    within the forward tolerance on every channel (the oracle takes a few seconds per frame on the
    box's 16-thread CPU share)."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config(name)
    assert (rs.width, rs.height) == ((1920, 1080) if name == "C3" else (3840, 2160))
    rs.spp = spp
    gpu = gpu_render(torch_cuda, renderer, sc, cam, rs)
    assert gpu[2]["paths"] == rs.width * rs.height * spp
    assert gpu[0][..., :3].min() >= 0
    exact = assert_parity(gpu, oracle(sc, cam, rs, forward=True, threads=16), name)
    assert exact > 0.999, f"{name}: only {exact:.4%} of channels bit-identical"


def test_c3_fullframe_repeatable(torch_cuda, renderer):
    """The whole headline frame is deterministic: the wavefront's atomics decide only the order in
    which rays are traced, never a value (RNG streams are keyed by pixel and sample), so two renders
    of C3 at full size are bit-identical, and so is the frame rendered as two progressive halves."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config("C3")
    rs.spp = 8
    a = gpu_render(torch_cuda, renderer, sc, cam, rs)
    b = gpu_render(torch_cuda, renderer, sc, cam, rs)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    assert a[2]["segments"] == b[2]["segments"] and a[2]["esvo_steps"] == b[2]["esvo_steps"]
    rs.spp = 4
    h1 = gpu_render(torch_cuda, renderer, sc, cam, rs)
    h2 = gpu_render(torch_cuda, renderer, sc, cam, rs, spp_start=4, accum=h1[0])
    assert np.array_equal(h2[0].view(np.uint32), a[0].view(np.uint32))
    assert np.array_equal(h1[1] + h2[1], a[1])


def test_c3_grazing_self_hit_regression(torch_cuda, renderer):
    """C3 pixel (269, 770), sample 22: a grazing ray re-hits its own sphere at a chord that rounds
    to zero and the transparent-skip `continue` (path_tracer.rs:52-54) never ends.  Contract C15
    caps a path at 64 next_intersection calls; GPU and oracle must agree on the capped path."""
    from octree_pathtracing_amd import scene as S
    from oracle import cpu_ref

    sc, cam, rs = S.make_config("C3")
    rs.spp = 1
    acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, rs, spp_start=22)
    r0, r1 = 768, 772
    racc, rsegs, rst = cpu_ref.render(sc, cam, rs.width, rs.height, 1, spp_start=22, max_depth=5, seed=rs.seed,
                                      forward=True, rows=(r0, r1))
    assert rst["max_path_segs"] == 64  # the capped path is in this band
    assert segs[770, 269] >= 64
    assert np.array_equal(segs[r0:r1], rsegs[r0:r1])
    assert rel_err(acc[r0:r1], racc[r0:r1]).max() <= REL_TOL_FORWARD


@pytest.mark.parametrize("name,res", [("tiny", None), ("C3", (256, 144, 4)), ("blocks", None)])
def test_megakernel_equals_wavefront(torch_cuda, renderer, name, res):
    """Both GPU strategies compute every path with the same device functions: bit-identical."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config(name)
    if res:
        rs.width, rs.height, rs.spp = res
    a = gpu_render(torch_cuda, renderer, sc, cam, rs, megakernel=False)
    b = gpu_render(torch_cuda, renderer, sc, cam, rs, megakernel=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in ("paths", "segments", "esvo_steps", "sphere_tests", "shade_events"):
        assert a[2][k] == b[2][k], k


def test_wavefront_small_pool_many_chunks(torch_cuda, renderer):
    """Pool much smaller than the work (path regeneration), 3 chunks (OCTPT_CHUNK) and ragged tiles."""
    import os
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import HipRenderer

    sc, cam, rs = S.make_config("tiny")
    rs.width, rs.height, rs.spp = 37, 19, 6
    ref = gpu_render(torch_cuda, renderer, sc, cam, rs)
    os.environ["OCTPT_POOL"] = "100"
    os.environ["OCTPT_REFILL"] = "1"
    os.environ["OCTPT_CHUNK"] = "2000"  # 960 tile pixels: 2 spp per chunk
    try:
        small = HipRenderer(0)
        out = gpu_render(torch_cuda, small, sc, cam, rs)
        small.close()
    finally:
        del os.environ["OCTPT_POOL"], os.environ["OCTPT_REFILL"], os.environ["OCTPT_CHUNK"]
    assert np.array_equal(ref[0], out[0]) and np.array_equal(ref[1], out[1])


@pytest.mark.parametrize("config", ["C2", "C5"])
def test_refill_schedules_identical(torch_cuda, renderer, config):
    """The extend schedule is invisible in the results: fixed refill thresholds 1 / 7 / 32 / 64 and the
    adaptive default, with a pool small enough that waves cross many 64-ray claim
    chunks and drain segments, give the same radiance, per-pixel segment counts and statistics."""
    import os
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import HipRenderer

    sc, cam, rs = S.make_config(config)
    rs.width, rs.height, rs.spp = 96, 40, 2
    ref = gpu_render(torch_cuda, renderer, sc, cam, rs)
    for refill in ("1", "7", "32", "64", ""):
        os.environ["OCTPT_POOL"] = "3000"
        if refill:
            os.environ["OCTPT_REFILL"] = refill
        try:
            r = HipRenderer(0)
            out = gpu_render(torch_cuda, r, sc, cam, rs)
            r.close()
        finally:
            os.environ.pop("OCTPT_POOL", None)
            os.environ.pop("OCTPT_REFILL", None)
        assert np.array_equal(ref[0], out[0]), refill
        assert np.array_equal(ref[1], out[1]), refill
        for k in ("paths", "segments", "esvo_steps", "sphere_tests", "cuboid_tests", "shade_events"):
            assert ref[2][k] == out[2][k], (refill, k)


GOLDEN = __import__("pathlib").Path(__file__).resolve().parent / "golden"


@pytest.mark.parametrize("name", ["c1_as_is", "c1", "tiny", "c2_small", "c3_small", "c4_small", "c5_small",
                                  "c3_preview", "c4_preview", "c5_preview", "tiny_fast", "c2_hq", "c4_hq_sss",
                                  "c5_nee_importance", "blocks_small", "blocks_preview"])
def test_render_matches_golden_fixture(torch_cuda, renderer, name):
    """GPU render vs the committed oracle fixture (tests/golden/make_golden.py): exact per-pixel
    segment counts and work totals, radiance within REL_TOL_FORWARD."""
    import json

    from octree_pathtracing_amd import scene as S

    from tests.test_golden_cpu import fixture_scene

    g = np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
    m = json.loads(str(g["meta"]))
    sc, cam = fixture_scene(m)  # a make_config name, or a tests/deep_worlds.py case under "generator"
    rs = S.RenderSettings(m["width"], m["height"], m["spp"], max_depth=m["max_depth"], seed=m["seed"])
    bc = m.get("branch_count", 1)
    acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, rs, preview=m.get("preview", False), branch_count=bc)
    keys = ("paths", "segments", "esvo_steps", "node_fetches", "prim_tests", "leaf_visits", "shade_events",
            "texel_reads", "max_path_segs")
    ref = dict(zip(keys, g["stats"].tolist()))
    assert np.array_equal(segs, g["segcount"])
    if bc > 1:  # GPU totals also count the replayed camera rays of branches > 0 (C20)
        e = rel_err(acc, g["accum"])
        assert e.max() <= REL_TOL_FORWARD, (name, e.max())
        return
    assert st["segments"] == ref["segments"] and st["esvo_steps"] == ref["esvo_steps"]
    assert st["sphere_tests"] + st["cuboid_tests"] == ref["prim_tests"]
    assert st["shade_events"] == ref["shade_events"] and st["paths"] == ref["paths"]
    e = rel_err(acc, g["accum"])
    assert e.max() <= REL_TOL_FORWARD, (name, e.max())
    assert (acc == g["accum"]).mean() > 0.999


def test_intersect_matches_golden_rays(renderer, name="c3_rays"):
    """octpt_intersect on a committed ray fixture (the C3 one; tests/test_gpu_deep.py passes the depth-21 one): prim
    ids, t, normals and ESVO step counts all bit-exact."""
    import json

    from tests.test_golden_cpu import fixture_scene

    g = np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
    sc = fixture_scene(json.loads(str(g["meta"])) if "meta" in g else {"config": "C3"})[0]
    renderer.set_scene(sc)
    t, prim, nrm, steps = renderer.intersect(g["rays"])
    assert np.array_equal(prim, g["prim"]) and np.array_equal(steps, g["steps"])
    assert np.array_equal(t, g["t"]) and np.array_equal(nrm, g["normal"])


# ---------------------------------------------------------------------------- preview mode (C16)
@pytest.mark.parametrize("name,res", [("tiny", None), ("C1", None), ("C2", (160, 90)), ("C3", (256, 144)),
                                      ("C4", (160, 90)), ("C5", (320, 180)), ("blocks", (160, 120))])
def test_preview_parity(torch_cuda, renderer, name, res):
    """RendererMode::Preview (preview_kernel) vs the oracle: segment counts, work totals and the
    flat-shaded radiance bit-exact; alpha of the incoming buffer untouched."""
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config(name)
    if res:
        rs.width, rs.height = res
    pre = np.random.default_rng(3).random((rs.height, rs.width, 4), dtype=np.float32)
    acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, rs, accum=pre, preview=True)
    racc, rsegs, rst = oracle(sc, cam, rs, accum=pre.copy(), preview=True)
    assert np.array_equal(segs, rsegs)
    assert st["paths"] == rst["paths"] == rs.width * rs.height
    assert st["segments"] == rst["segments"] and st["esvo_steps"] == rst["esvo_steps"]
    assert st["sphere_tests"] + st["cuboid_tests"] == rst["prim_tests"] and st["shade_events"] == 0
    assert st["texel_reads"] == rst["texel_reads"]
    assert np.array_equal(acc, racc), f"{name}: max abs diff {np.abs(acc - racc).max()}"
    assert np.array_equal(acc[..., 3], pre[..., 3])


def test_preview_shards_union_equals_full(torch_cuda, renderer):
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import shard_pixels

    torch = torch_cuda
    sc, cam, rs = S.make_config("C4")
    rs.width, rs.height = 70, 45
    full = gpu_render(torch, renderer, sc, cam, rs, preview=True)[0]
    N = 3
    stride = max(shard_pixels(rs.width, rs.height, i, N) for i in range(N))
    buf = torch.zeros((N * stride, 4), dtype=torch.float32, device="cuda")
    for i in range(N):
        a = gpu_render(torch, renderer, sc, cam, rs, shard=(i, N), compact=True, preview=True)[0]
        buf[i * stride:i * stride + len(a)] = torch.as_tensor(a, device="cuda")
    frame = torch.zeros((rs.height * rs.width, 4), dtype=torch.float32, device="cuda")
    renderer.unshard_device(rs.width, rs.height, N, buf.data_ptr(), stride, frame.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().reshape(rs.height, rs.width, 4), full)


def test_renderer_preview_mode(renderer):
    """HipRenderer.set_mode(Preview) + render_frame (TileRenderer::render_preview): one replacing
    pass, current spp stays 0, the frame equals the oracle's preview."""
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import RendererMode
    from oracle import cpu_ref

    sc, cam, rs = S.make_config("C4")
    W, H = 96, 64
    renderer.set_scene(sc)
    renderer.set_camera(cam)
    renderer.set_resolution((W, H))
    renderer.set_mode(RendererMode.Preview)
    try:
        assert renderer.get_mode() is RendererMode.Preview
        renderer.render_frame().wait_for()
        assert renderer.get_current_spp() == 0
        ref = cpu_ref.render(sc, cam, W, H, 1, preview=True)[0]
        assert np.array_equal(renderer.get_float_image(), ref)
    finally:
        renderer.set_mode(RendererMode.PathTraced)


# ---------------------------------------------------------------------------------------------
# sun sampling (next-event estimation): shadow segments between a diffuse hit and
# its bounce, through the kNee shade / megakernel instances
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant,res", [("tiny", "fast", None), ("tiny", "hq_sss", None),
                                              ("C2", "hq", (160, 90, 4)), ("C3", "fast", (192, 108, 2)),
                                              ("C4", "hq_sss", (128, 72, 2)), ("C5", "nee_importance", (192, 108, 2)),
                                              ("blocks", "hq", None)])
def test_sun_sampling_parity(torch_cuda, renderer, name, variant, res):
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config(name)
    S.with_sun_variant(sc, variant)
    if res:
        rs.width, rs.height, rs.spp = res
    gpu = gpu_render(torch_cuda, renderer, sc, cam, rs)
    ref = oracle(sc, cam, rs, forward=True)
    exact = assert_parity(gpu, ref, f"{name}/{variant}")
    assert exact > 0.999, f"{name}/{variant}: only {exact:.4%} of channels bit-identical"
    rec = oracle(sc, cam, rs, forward=False)
    assert rel_err(gpu[0], rec[0]).max() <= REL_TOL_RECURSIVE


@pytest.mark.parametrize("variant", ["fast", "hq_sss"])
def test_sun_sampling_megakernel_and_small_pool(torch_cuda, renderer, variant):
    """The megakernel keeps the waiting bounce in registers, the wavefront in the slot's NEE planes:
    both bit-identical, also when slots are recycled across 3 chunks with a 100-path pool."""
    import os
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import HipRenderer

    sc, cam, rs = S.make_config("tiny")
    S.with_sun_variant(sc, variant)
    rs.width, rs.height, rs.spp = 37, 19, 6
    a = gpu_render(torch_cuda, renderer, sc, cam, rs)
    b = gpu_render(torch_cuda, renderer, sc, cam, rs, megakernel=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    os.environ["OCTPT_POOL"] = "100"
    os.environ["OCTPT_REFILL"] = "1"
    os.environ["OCTPT_CHUNK"] = "2000"
    try:
        small = HipRenderer(0)
        c = gpu_render(torch_cuda, small, sc, cam, rs)
        small.close()
    finally:
        del os.environ["OCTPT_POOL"], os.environ["OCTPT_REFILL"], os.environ["OCTPT_CHUNK"]
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


# ---------------------------------------------------------------------------------------------
# TileRenderer branch count: the first reflection splits into branch_count branches,
# each branch a wavefront path of its own (the camera ray replayed), folded per pass in resolve
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,res,variant", [("tiny", (64, 48, 20), None), ("C2", (160, 90, 20), None),
                                              ("blocks", (64, 48, 20), "fast"), ("C4", (96, 54, 10), None)])
def test_branch_count_parity(torch_cuda, renderer, name, res, variant):
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config(name)
    if variant:
        S.with_sun_variant(sc, variant)
    rs.width, rs.height, rs.spp = res
    acc, segs, st = gpu_render(torch_cuda, renderer, sc, cam, rs, branch_count=10)
    racc, rsegs, rst = oracle(sc, cam, rs, forward=True, branch_count=10)
    assert np.array_equal(segs, rsegs), f"{name}: segment counts differ at {np.argwhere(segs != rsegs)[:5]}"
    assert st["paths"] >= rst["paths"] and st["segments"] >= rst["segments"]
    e = rel_err(acc, racc)
    assert e.max() <= REL_TOL_FORWARD, f"{name}: max rel err {e.max()}"
    assert (acc == racc).mean() > 0.999
    rec = oracle(sc, cam, rs, forward=False, branch_count=10)
    assert rel_err(acc, rec[0]).max() <= REL_TOL_RECURSIVE


def test_branch_count_progressive_and_chunked(torch_cuda, renderer):
    """[0, 10) + [10, 40) == [0, 40) on the GPU, and == a render chunked into pass-aligned chunks
    of a 100-slot pool (OCTPT_CHUNK, OCTPT_POOL)."""
    import os
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import HipRenderer

    sc, cam, rs = S.make_config("tiny")
    rs.width, rs.height, rs.spp = 37, 19, 40
    whole = gpu_render(torch_cuda, renderer, sc, cam, rs, branch_count=10)
    rs.spp = 10
    a = gpu_render(torch_cuda, renderer, sc, cam, rs, branch_count=10)
    rs.spp = 30
    b = gpu_render(torch_cuda, renderer, sc, cam, rs, spp_start=10, accum=a[0], branch_count=10)
    assert np.array_equal(whole[0], b[0]) and np.array_equal(whole[1], a[1] + b[1])
    # 100 spp = passes 1, 1, 1, 1, 6, 10 x 9; a 65-sub-sample chunk cap (960 tile pixels) makes the
    # host pull the first chunk back to the pass boundary at 60
    rs.spp = 100
    full = gpu_render(torch_cuda, renderer, sc, cam, rs, branch_count=10)
    os.environ.update({"OCTPT_POOL": "100", "OCTPT_CHUNK": str(65 * 960)})
    try:
        small = HipRenderer(0)
        c = gpu_render(torch_cuda, small, sc, cam, rs, branch_count=10)
        small.close()
    finally:
        del os.environ["OCTPT_POOL"], os.environ["OCTPT_CHUNK"]
    assert np.array_equal(full[0], c[0]) and np.array_equal(full[1], c[1])


def test_branch_count_validation(renderer):
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config("tiny")
    renderer.set_scene(sc)
    renderer.set_camera(cam)
    acc = np.zeros((rs.height, rs.width, 4), np.float32)
    renderer.branch_count = 10
    try:
        for start, count, flags, want in [(0, 5, 0, _lib.ERR_INVALID_ARG),   # 5 is inside the 6-pass [4, 10)
                                          (5, 5, 0, _lib.ERR_INVALID_ARG),   # 5 is not a pass start
                                          (0, 10, _lib.RENDER_MEGAKERNEL, _lib.ERR_UNSUPPORTED),
                                          (0, 10, 0, _lib.OK)]:
            p = renderer.params(rs.width, rs.height, start, count)
            p.flags = flags
            st = renderer._lib.octpt_render(renderer._ctx, C.byref(p), acc.ctypes.data_as(C.c_void_p), None)
            assert st == want, (start, count, flags, st)
        p = renderer.params(rs.width, rs.height, 0, 10)
        p.branch_count = 65
        st = renderer._lib.octpt_render(renderer._ctx, C.byref(p), acc.ctypes.data_as(C.c_void_p), None)
        assert st == _lib.ERR_INVALID_ARG
    finally:
        renderer.branch_count = 1
