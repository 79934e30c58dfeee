"""First-hit guide buffers (octpt_render_aov, gbuffer_kernel) on the GPU.

Pinned exactly, without a new oracle: octpt_camera_rays gives the device's own camera rays, the oracle's
Scene::hit of those rays gives t, primitive and normal of every pixel whose preview chain is one segment
(bit-equal depth, prim, normal), and the preview identity -- preview rgb == albedo * (sun emittance *
max(0.3, n . sun)) -- pins the albedo, the material and the chained pixels against the bit-exact preview."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
PRIM_NONE = 0xFFFFFFFF
# the project's small configs at crop sizes (C2's 37x21 has edge tiles that are no multiple of 8), plus the block-value
# form of the blocks world, which is the one scene kind (gbuffer_kernel<kPrimsBlocks>) the others do not launch
CONFIGS = [("tiny", None), ("C3", (256, 144)), ("C4", (160, 90)), ("C2", (37, 21)), ("blocks", (160, 120)),
           ("blocks-b", (64, 48))]
NAMES = [c[0] for c in CONFIGS]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    from octree_pathtracing_amd.renderer import HipRenderer

    r = HipRenderer(device=0)
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def config(name):
    from octree_pathtracing_amd import scene as S

    sc, cam, rs = S.make_config(name)
    res = dict(CONFIGS)[name]
    if res:
        rs.width, rs.height = res
    return sc, cam, rs


@pytest.fixture(scope="module")
def case(renderer):
    """name -> everything the tests compare, computed once per config: the oracle's preview and Scene::hit
    of the camera rays, the GPU's guide buffers (with the pass's statistics) and its preview frame."""
    from octree_pathtracing_amd import _lib
    from oracle import cpu_ref

    done = {}

    def get(name):
        if name in done:
            return done[name]
        sc, cam, rs = config(name)
        W, H = rs.width, rs.height
        renderer.set_scene(sc)
        renderer.set_camera(cam)
        rays = renderer.camera_rays(W, H)
        rt, rprim, rn, _ = cpu_ref.intersect(sc, rays.reshape(-1, 6))
        racc, rsegs, rst = cpu_ref.render(sc, cam, W, H, 1, preview=True)
        renderer.reset_stats()
        aov = renderer.render_aov(rs)
        st = renderer.stats()
        pre = np.zeros((H, W, 4), F32)
        pre[..., 3] = 1.0
        p = renderer.params(W, H, 0, 0, preview=True)
        renderer._check(renderer._lib.octpt_render(renderer._ctx, C.byref(p), pre.ctypes.data_as(C.c_void_p), None))
        done[name] = dict(sc=sc, cam=cam, rs=rs, rt=rt.reshape(H, W), rprim=rprim.reshape(H, W),
                          rn=rn.reshape(H, W, 3), rsegs=rsegs, rst=rst, racc=racc, aov=aov, stats=st, preview=pre)
        return done[name]

    return get


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("name", NAMES)
def test_single_segment_pixels_equal_scene_hit(case, name):
    """Every pixel whose oracle preview chain is one segment: prim, normal and depth equal the oracle's
    Scene::hit of the pixel's camera ray (depth bit for bit), misses are +inf / 0xFFFFFFFF / zeros; the pass
    counts paths, segments and ESVO iterations as the preview does.

    The `blocks` view (160x120, alpha-0 texels and model quads): 6992 single-segment hit pixels and 1494
    chained pixels by the oracle alone, so single-segment pixels are at least 82.4 % of the hit pixels."""
    c = case(name)
    a, one = c["aov"], c["rsegs"] == 1
    hit, miss = one & np.isfinite(c["rt"]), one & ~np.isfinite(c["rt"])
    assert hit.any()
    assert np.array_equal(a["prim"][hit], c["rprim"][hit])
    assert np.array_equal(bits(a["normal"][..., :3][hit]), bits(c["rn"][hit]))
    assert np.array_equal(bits(a["depth"][hit]), bits(c["rt"][hit]))
    assert np.all(a["normal"][..., 3] == 0)
    assert np.all(a["material"][hit] != 0) and np.all(a["albedo"][..., 3][hit] > 0)
    assert np.all(np.isposinf(a["depth"][miss])) and np.all(a["prim"][miss] == PRIM_NONE)
    assert not a["albedo"][miss].any() and not a["normal"][miss].any() and not a["material"][miss].any()
    st, rst, rs = c["stats"], c["rst"], c["rs"]
    assert st["paths"] == rs.width * rs.height == rst["paths"]
    assert st["segments"] == rst["segments"] == int(c["rsegs"].sum())
    assert st["esvo_steps"] == rst["esvo_steps"]
    if name.startswith("blocks"):
        gpu_hits = int((a["prim"] != PRIM_NONE).sum())
        assert 2 * int(hit.sum()) >= gpu_hits, (int(hit.sum()), gpu_hits)
        assert (c["rsegs"] > 1).any()  # the pass-through chain is exercised


def sun_vectors(sun):
    """Sun::new (scene/mod.rs:321-383) in f32: the sun direction sw and the emittance colour *
    INTENSITY^GAMMA, with the C library's cosf / sinf / powf as the host side of the library uses them."""
    m = C.CDLL("libm.so.6")
    for f in (m.cosf, m.sinf):
        f.restype, f.argtypes = C.c_float, [C.c_float]
    m.powf.restype, m.powf.argtypes = C.c_float, [C.c_float, C.c_float]
    theta, phi = F32(sun.azimuth), F32(sun.altitude)
    r = np.abs(F32(m.cosf(phi)))
    sw = np.array([F32(m.cosf(theta)) * r, F32(m.sinf(phi)), F32(m.sinf(theta)) * r], F32)
    emit = np.asarray(sun.color[:3], F32) * F32(m.powf(F32(1.25), F32(2.2)))
    return sw, emit


@pytest.mark.parametrize("name", NAMES)
def test_preview_identity(case, name):
    """All pixels: a guide-buffer hit has material != 0 and albedo alpha > 0, and there the preview's rgb is
    albedo.rgb * (emittance * max(0.3, n . sw)) (Sun::flat_shading, scene/mod.rs:447-452) -- bit for bit: the
    sun vectors come from the same libm calls in f32 and numpy's f32 products round as the kernel's.  The
    preview itself equals the oracle's (checked here too), so this pins albedo, normal and material of
    the chained pixels as well.  A miss pixel holds the miss values in all five buffers."""
    c = case(name)
    a, pre = c["aov"], c["preview"]
    assert np.array_equal(pre, c["racc"])
    hit = a["prim"] != PRIM_NONE
    assert np.array_equal(hit, np.isfinite(a["depth"])) and np.array_equal(hit, a["material"] != 0)
    assert np.all(a["albedo"][..., 3][hit] > 0)
    assert np.all(a["depth"][hit] > 0)
    miss = ~hit
    assert not a["albedo"][miss].any() and not a["normal"][miss].any()
    # a chained pixel is at least as far as the first thing its ray meets
    chained = hit & (c["rsegs"] > 1)
    assert np.all(a["depth"][chained] >= c["rt"][chained])
    sw, emit = sun_vectors(c["sc"].sun)
    n = a["normal"]
    shading = np.maximum(F32(0.3), (n[..., 0] * sw[0] + n[..., 1] * sw[1]) + n[..., 2] * sw[2])
    want = a["albedo"][..., :3] * (emit[None, None, :] * shading[..., None])
    assert np.array_equal(bits(pre[..., :3][hit]), bits(want[hit])), np.abs(pre[..., :3][hit] - want[hit]).max()


def gather_shards(renderer, rs, N, order=None):
    """The full-frame buffers from N compact shards: shard i's local tile u sits at dealing position
    i + u * N, which holds frame tile order[position] (the position itself without an order)."""
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd.renderer import shard_pixels

    W, H = rs.width, rs.height
    tx = (W + 7) // 8
    T = tx * ((H + 7) // 8)
    full = {k: None for k in _lib.AOV_NAMES}
    for i in range(N):
        part = renderer.render_aov(rs, shard=(i, N), compact=True)
        n = shard_pixels(W, H, i, N)
        assert all(len(v) == n for v in part.values())
        tiles = np.arange(i, T, N)
        if order is not None:
            tiles = np.asarray(order)[tiles]
        k = np.arange(64)
        x = ((tiles % tx) * 8)[:, None] + (k % 8)[None, :]
        y = ((tiles // tx) * 8)[:, None] + (k // 8)[None, :]
        ok = (x < W) & (y < H)
        for name, v in part.items():
            if full[name] is None:
                full[name] = np.zeros((H, W) + v.shape[1:], v.dtype)
            full[name][y[ok], x[ok]] = v.reshape((len(tiles), 64) + v.shape[1:])[ok]
    return full


def test_shards_union_equals_full(renderer):
    sc, cam, rs0 = config("C4")
    from octree_pathtracing_amd.scene import RenderSettings

    rs = RenderSettings(70, 45, 1)
    renderer.set_scene(sc)
    renderer.set_camera(cam)
    full = renderer.render_aov(rs)
    assert np.isfinite(full["depth"]).any() and np.isinf(full["depth"]).any()
    got = gather_shards(renderer, rs, 3)
    for k, v in full.items():
        assert np.array_equal(bits(v) if v.dtype == F32 else v, bits(got[k]) if v.dtype == F32 else got[k]), k
    T = ((rs.width + 7) // 8) * ((rs.height + 7) // 8)
    order = np.arange(T, dtype=np.uint32)[::-1].copy()
    renderer.set_tile_order(rs.width, rs.height, order)
    try:
        again = renderer.render_aov(rs)
        got = gather_shards(renderer, rs, 3, order)
    finally:
        renderer.set_tile_order(rs.width, rs.height, None)
    for k, v in full.items():
        same = (lambda p, q: np.array_equal(bits(p), bits(q))) if v.dtype == F32 else np.array_equal
        assert same(v, again[k]) and same(v, got[k]), k


def test_selective_outputs(case, renderer):
    """Only `depth` requested: the same depth as with all five; arrays that were not requested stay as they
    were; no output requested: OK and nothing runs."""
    c = case("tiny")
    rs = c["rs"]
    renderer.set_scene(c["sc"])
    renderer.set_camera(c["cam"])
    W, H = rs.width, rs.height
    out = {"albedo": np.full((H, W, 4), 7.5, F32), "normal": np.full((H, W, 4), -3.25, F32),
           "depth": np.full((H, W), -1.0, F32), "prim": np.full((H, W), 12345, np.uint32),
           "material": np.full((H, W), 54321, np.uint32)}
    got = renderer.render_aov(rs, which=("depth",), out=out)
    assert set(got) == {"depth"} and got["depth"] is out["depth"]
    assert np.array_equal(bits(out["depth"]), bits(c["aov"]["depth"]))
    assert np.all(out["albedo"] == 7.5) and np.all(out["normal"] == -3.25)
    assert np.all(out["prim"] == 12345) and np.all(out["material"] == 54321)
    renderer.reset_stats()
    assert renderer.render_aov(rs, which=()) == {}
    st = renderer.stats()
    assert st["paths"] == 0 and st["launches"] == 0


def test_device_entry_on_a_stream(case, renderer, torch_cuda):
    torch = torch_cuda
    c = case("C2")
    rs = c["rs"]
    renderer.set_scene(c["sc"])
    renderer.set_camera(c["cam"])
    n = rs.width * rs.height
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = {"albedo": torch.full((n, 4), 9.0, device="cuda"), "normal": torch.full((n, 4), 9.0, device="cuda"),
             "depth": torch.full((n,), 9.0, device="cuda"),
             "prim": torch.full((n,), 9, dtype=torch.int32, device="cuda"),
             "material": torch.full((n,), 9, dtype=torch.int32, device="cuda")}
        p = renderer.params(rs.width, rs.height, 0, 0)
        renderer.render_aov_device(p, {k: v.data_ptr() for k, v in t.items()}, s.cuda_stream)
    s.synchronize()
    for k, v in c["aov"].items():
        got = t[k].cpu().numpy().reshape(v.shape)
        assert np.array_equal(got.view(np.uint32), v.view(np.uint32)), k


def test_invalid_arguments(case, renderer, torch_cuda):
    """Each INVALID_ARG of the new context entry points, with its octpt_last_error text."""
    from octree_pathtracing_amd import _lib

    lib, ctx = renderer._lib, renderer._ctx
    c = case("tiny")
    renderer.set_scene(c["sc"])
    renderer.set_camera(c["cam"])

    def err():
        return lib.octpt_last_error(ctx).decode()

    b = _lib.AovBuffers()
    p = renderer.params(8, 8, 0, 0)
    assert lib.octpt_render_aov(ctx, None, C.byref(b)) == _lib.ERR_INVALID_ARG and "params NULL" in err()
    assert lib.octpt_render_aov(ctx, C.byref(p), None) == _lib.ERR_INVALID_ARG and "guide buffers NULL" in err()
    assert lib.octpt_render_aov_device(ctx, None, C.byref(b), None) == _lib.ERR_INVALID_ARG and "params NULL" in err()
    assert lib.octpt_render_aov_device(ctx, C.byref(p), None, None) == _lib.ERR_INVALID_ARG
    z = renderer.params(0, 8, 0, 0)
    assert lib.octpt_render_aov(ctx, C.byref(z), C.byref(b)) == _lib.ERR_INVALID_ARG and "resolution" in err()
    # spp, depth and seed are ignored: a params block a render would refuse (max_depth 0) is fine here
    q = _lib.RenderParams(8, 8, 0, 0, 0, 0, 0, 0, 1, 0)
    assert lib.octpt_render_aov(ctx, C.byref(q), C.byref(b)) == _lib.OK

    torch = torch_cuda
    col = torch.zeros((64, 4), device="cuda")
    nrm = torch.zeros((64, 4), device="cuda")
    dep = torch.ones(64, device="cuda")
    g = _lib.AovBuffers(normal=nrm.data_ptr(), depth=dep.data_ptr())

    def dn(params, guides=g, color=col.data_ptr(), out=col.data_ptr()):
        return lib.octpt_denoise_device(ctx, C.byref(params) if params else None, C.c_void_p(color),
                                        C.byref(guides) if guides else None, C.c_void_p(out), None)

    ok = _lib.DenoiseParams(8, 8, 1, 1.0, 1.0, 1.0, 0)
    assert dn(ok) == _lib.OK
    assert dn(None) == _lib.ERR_INVALID_ARG and "params NULL" in err()
    assert dn(_lib.DenoiseParams(0, 8, 1, 1.0, 1.0, 1.0, 0)) == _lib.ERR_INVALID_ARG and "zero frame size" in err()
    for it in (0, 6):
        assert dn(_lib.DenoiseParams(8, 8, it, 1.0, 1.0, 1.0, 0)) == _lib.ERR_INVALID_ARG and "iterations" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for k in range(3):
            sig = [1.0, 1.0, 1.0]
            sig[k] = bad
            assert dn(_lib.DenoiseParams(8, 8, 1, *sig, 0)) == _lib.ERR_INVALID_ARG and "sigma" in err()
    assert dn(ok, guides=None) == _lib.ERR_INVALID_ARG and "normal and depth" in err()
    assert dn(ok, guides=_lib.AovBuffers(normal=nrm.data_ptr())) == _lib.ERR_INVALID_ARG and "normal and depth" in err()
    assert dn(ok, guides=_lib.AovBuffers(depth=dep.data_ptr())) == _lib.ERR_INVALID_ARG
    demod = _lib.DenoiseParams(8, 8, 1, 1.0, 1.0, 1.0, _lib.DENOISE_DEMODULATE)
    assert dn(demod) == _lib.ERR_INVALID_ARG and "albedo" in err()
    assert dn(_lib.DenoiseParams(8, 8, 1, 1.0, 1.0, 1.0, 0x2)) == _lib.ERR_INVALID_ARG and "compact" in err()
    assert dn(ok, color=0) == _lib.ERR_INVALID_ARG and dn(ok, out=0) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
