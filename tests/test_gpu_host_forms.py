"""The host-pointer forms of the post-processing entries against their device forms (csrc/octpt_post.cpp, staged
through csrc/octpt_stage.h): bit-identical outputs on the same inputs, with every optional buffer supplied and with
each one absent, on a 70 x 50 frame of the tiny scene -- not a multiple of the 8 x 8 tile, so that the per-pixel
(n = 3500) and per-tile (T = 63) buffer sizes differ and a mixed-up size shows as a mismatch.  A failed call leaves
the caller's buffers alone, a partial guide-buffer shard keeps the caller's values in the pixels it does not write,
and a two-entry context answers as one device does."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP = 70, 50, 4
N, T = W * H, ((W + 7) // 8) * ((H + 7) // 8)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def tiny_renderer(**kw):
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import HipRenderer

    sc, cam, _ = S.make_config("tiny")
    r = HipRenderer(**(kw or {"device": 0}))
    r.set_scene(sc)
    r.set_camera(cam)
    return r


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    r = tiny_renderer()
    yield r
    r.close()


@pytest.fixture(scope="module")
def frames(renderer):
    """The inputs every test shares, computed once: guides, a noisy frame, an adaptive render's moments and tile_spp,
    a temporal history with moments, and a variance plane."""
    from octree_pathtracing_amd.scene import RenderSettings

    r, rs = renderer, RenderSettings(W, H, SPP)
    f = {"rs": rs, "aov": r.render_aov(rs), "color": r.render(rs)[0]}
    f["accum"], f["moments"], f["tile_spp"], _ = r.render_adaptive(RenderSettings(W, H, 8), 2, 2, 0.05)
    f["history"] = r.temporal(f["color"], f["aov"], moments=True, demodulate=True)
    f["variance"] = r.variance(f["history"], f["aov"], min_history=1)
    f["error"] = r.tile_error(f["moments"], f["tile_spp"])
    return f


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def same(host, dev, what):
    assert host.shape == dev.shape and np.array_equal(bits(host), bits(dev)), f"{what}: host form != device form"


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def dptrs(torch, aov, names):
    keep = {k: dev(torch, aov[k]) for k in names}
    return keep, {k: v.data_ptr() for k, v in keep.items()}


def test_intersect_optional_buffers(renderer, frames):
    """normal and steps NULL, with and without last_prim and last_normal: t and prim as with every buffer supplied"""
    rays = np.ascontiguousarray(renderer.camera_rays(W, H).reshape(-1, 6))
    t_all, prim_all, _, _ = renderer.intersect(rays)
    t, prim = np.full(N, -7.0, np.float32), np.full(N, 7, np.uint32)
    renderer._check(renderer._lib.octpt_intersect(renderer._ctx, ptr(rays), None, None, N, ptr(t), ptr(prim), None, None))
    same(t, t_all, "t")
    same(prim, prim_all, "prim")
    ln = np.zeros((N, 3), np.float32)
    keyed = renderer.intersect(rays, last_prim=prim_all, last_normal=ln)
    renderer._check(renderer._lib.octpt_intersect(renderer._ctx, ptr(rays), ptr(prim_all), ptr(ln), N, ptr(t), ptr(prim), None,
                                                  None))
    same(t, keyed[0], "keyed t")
    same(prim, keyed[1], "keyed prim")


@pytest.mark.parametrize("which", [("albedo", "normal", "depth", "prim", "material"), ("depth",), ("normal", "prim")])
def test_render_aov(torch_cuda, renderer, frames, which):
    from octree_pathtracing_amd import _lib

    got = renderer.render_aov(frames["rs"], which=which)
    d = {k: torch_cuda.zeros((H, W, 4) if k in ("albedo", "normal") else (H, W),
                             dtype=torch_cuda.float32 if k in ("albedo", "normal", "depth") else torch_cuda.int32,
                             device="cuda") for k in which}
    renderer.render_aov_device(renderer.params(W, H, 0, 0), {k: v.data_ptr() for k, v in d.items()})
    torch_cuda.cuda.synchronize()
    assert set(got) == set(which) and set(which) <= set(_lib.AOV_NAMES)
    for k in which:
        same(got[k], host(d[k]), k)


def test_render_aov_partial_shard_keeps_the_callers_values(renderer, frames):
    """shard 0 of 2 and shard 1 of 2 of a full frame, each into sentinel-filled buffers: every pixel is written by
    exactly one of them, with the full frame's value, and keeps the sentinel in the other"""
    sentinel = np.float32(-123.0)
    shards = []
    for s in (0, 1):
        out = {"depth": np.full((H, W), sentinel, np.float32), "normal": np.full((H, W, 4), sentinel, np.float32)}
        renderer.render_aov(frames["rs"], which=("depth", "normal"), shard=(s, 2), out=out)
        shards.append(out)
    wrote = [o["depth"] != sentinel for o in shards]
    assert wrote[0].any() and wrote[1].any() and not (wrote[0] & wrote[1]).any() and (wrote[0] | wrote[1]).all()
    for o, m in zip(shards, wrote):
        assert np.array_equal(bits(o["depth"][m]), bits(frames["aov"]["depth"][m]))
        assert np.array_equal(bits(o["normal"][m]), bits(frames["aov"]["normal"][m]))
        assert (o["normal"][~m] == sentinel).all()


@pytest.mark.parametrize("demodulate", [False, True], ids=["no_albedo", "albedo"])
def test_denoise(torch_cuda, renderer, frames, demodulate):
    from octree_pathtracing_amd import _lib

    got = renderer.denoise(frames["color"], frames["aov"], iterations=2, demodulate=demodulate)
    keep, g = dptrs(torch_cuda, frames["aov"], ("normal", "depth") + (("albedo",) if demodulate else ()))
    c = dev(torch_cuda, frames["color"])
    p = _lib.DenoiseParams(W, H, 2, 0.6, 0.3, 0.1, _lib.DENOISE_DEMODULATE if demodulate else 0)
    renderer.denoise_device(p, c.data_ptr(), g, c.data_ptr())
    torch_cuda.cuda.synchronize()
    same(got, host(c), "denoise")


@pytest.mark.parametrize("moments", [False, True], ids=["temporal", "temporal_moments"])
@pytest.mark.parametrize("with_prev", [False, True], ids=["no_prev", "prev"])
def test_temporal(torch_cuda, renderer, frames, moments, with_prev):
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd.renderer import _c_camera

    torch, aov, hist = torch_cuda, frames["aov"], frames["history"] if with_prev else None
    got = renderer.temporal(frames["color"], aov, history=hist, moments=moments, demodulate=moments)
    cam = _c_camera(renderer.get_camera())
    flags = _lib.TEMPORAL_MATCH_PRIM | (_lib.TEMPORAL_DEMODULATE if moments else 0)
    p = _lib.TemporalParams(W, H, cam, cam, 32, 0.1, 0.9, flags)
    keep, g = dptrs(torch, aov, ("normal", "depth", "prim") + (("albedo",) if moments else ()))
    keep_h, prev = dptrs(torch, hist, ("color", "normal", "depth", "prim", "length")) if with_prev else (None, None)
    c = dev(torch, frames["color"])
    length = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    if moments:
        pm = dev(torch, hist["moments"]) if with_prev else None
        om = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
        renderer.temporal_moments_device(p, c.data_ptr(), g, prev, pm.data_ptr() if with_prev else None, c.data_ptr(),
                                         length.data_ptr(), om.data_ptr())
    else:
        renderer.temporal_device(p, c.data_ptr(), g, prev, c.data_ptr(), length.data_ptr())
    torch.cuda.synchronize()
    same(got["color"], host(c), "colour")
    same(got["length"], host(length, np.uint32), "length")
    if moments:
        same(got["moments"], host(om), "moments")


def test_variance(torch_cuda, renderer, frames):
    from octree_pathtracing_amd import _lib

    hist = frames["history"]
    keep, g = dptrs(torch_cuda, frames["aov"], ("normal", "depth"))
    m, ln = dev(torch_cuda, hist["moments"]), dev(torch_cuda, hist["length"])
    out = torch_cuda.zeros((H, W), dtype=torch_cuda.float32, device="cuda")
    renderer.variance_device(_lib.VarianceParams(W, H, 1, 0.3, 0.1), m.data_ptr(), ln.data_ptr(), g, out.data_ptr())
    torch_cuda.cuda.synchronize()
    same(frames["variance"], host(out), "variance")


@pytest.mark.parametrize("demodulate", [False, True], ids=["no_albedo", "albedo"])
@pytest.mark.parametrize("with_out_variance", [False, True], ids=["no_out_variance", "out_variance"])
def test_denoise_variance(torch_cuda, renderer, frames, demodulate, with_out_variance):
    from octree_pathtracing_amd import _lib

    aov, names = frames["aov"], ("normal", "depth") + (("albedo",) if demodulate else ())
    p = _lib.DenoiseVarianceParams(W, H, 2, 4.0, 1e-2, 0.3, 0.1, _lib.DENOISE_DEMODULATE if demodulate else 0)
    b = _lib.AovBuffers(**{k: aov[k].ctypes.data for k in names})
    out = np.zeros((H, W, 4), np.float32)
    out_var = np.zeros((H, W), np.float32) if with_out_variance else None
    renderer._check(renderer._lib.octpt_denoise_variance(renderer._ctx, C.byref(p), ptr(frames["color"]),
                                                         ptr(frames["variance"]), C.byref(b), ptr(out), ptr(out_var)))
    keep, g = dptrs(torch_cuda, aov, names)
    c, v = dev(torch_cuda, frames["color"]), dev(torch_cuda, frames["variance"])
    renderer.denoise_variance_device(p, c.data_ptr(), v.data_ptr(), g, c.data_ptr(),
                                     v.data_ptr() if with_out_variance else None)
    torch_cuda.cuda.synchronize()
    same(out, host(c), "filtered frame")
    if with_out_variance:
        same(out_var, host(v), "filtered variance")


def test_tile_error_and_spread(torch_cuda, renderer, frames):
    from octree_pathtracing_amd import _lib

    torch = torch_cuda
    m, n = dev(torch, frames["moments"]), dev(torch, frames["tile_spp"])
    e, s = (torch.zeros(T, dtype=torch.float32, device="cuda") for _ in range(2))
    renderer.tile_error_device(_lib.TileErrorParams(W, H, 1e-2), m.data_ptr(), n.data_ptr(), e.data_ptr())
    renderer.tile_error_spread_device(W, H, 0.5, e.data_ptr(), s.data_ptr())
    torch.cuda.synchronize()
    err = renderer.tile_error(frames["moments"], frames["tile_spp"], luminance_floor=1e-2)
    assert err.shape == (T,) and T != N // 64
    same(err, host(e), "tile error")
    same(renderer.tile_error_spread(err, W, H, 0.5), host(s), "spread")


@pytest.mark.parametrize("demodulate", [False, True], ids=["no_albedo", "albedo"])
def test_sample_variance(torch_cuda, renderer, frames, demodulate):
    from octree_pathtracing_amd import _lib

    got = renderer.sample_variance(frames["moments"], frames["tile_spp"], frames["aov"], demodulate=demodulate)
    keep, g = dptrs(torch_cuda, frames["aov"], ("depth",) + (("albedo",) if demodulate else ()))
    m, n = dev(torch_cuda, frames["moments"]), dev(torch_cuda, frames["tile_spp"])
    out = torch_cuda.zeros((H, W), dtype=torch_cuda.float32, device="cuda")
    p = _lib.SampleVarianceParams(W, H, _lib.DENOISE_DEMODULATE if demodulate else 0)
    renderer.sample_variance_device(p, m.data_ptr(), n.data_ptr(), g, out.data_ptr())
    torch_cuda.cuda.synchronize()
    same(got, host(out), "sample variance")


def adaptive_params(ex):
    from octree_pathtracing_amd import _lib

    return _lib.AdaptiveParamsEx(2, 2, 0.05, 1e-2, 0.5) if ex else _lib.AdaptiveParams(2, 2, 0.05, 1e-2)


@pytest.mark.parametrize("ex", [False, True], ids=["adaptive", "adaptive_ex"])
@pytest.mark.parametrize("optional", [False, True], ids=["accum_only", "all_buffers"])
def test_render_adaptive(torch_cuda, renderer, frames, ex, optional):
    """moments, tile_spp and out_rgba8 NULL, and all three supplied"""
    torch, r, a = torch_cuda, renderer, adaptive_params(ex)
    p = r.params(W, H, 0, 8)
    accum = np.zeros((H, W, 4), np.float32)
    moments, tile_spp, rgba = ((np.zeros((H, W, 2), np.float32), np.zeros(T, np.uint32), np.zeros((H, W, 4), np.uint8))
                               if optional else (None, None, None))
    entry = r._lib.octpt_render_adaptive_ex if ex else r._lib.octpt_render_adaptive
    r._check(entry(r._ctx, C.byref(p), C.byref(a), ptr(accum), ptr(moments), ptr(tile_spp), ptr(rgba), None))
    d_acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    d_mom = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    d_rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    spp, _ = (r.render_adaptive_ex_device if ex else r.render_adaptive_device)(p, a, d_acc.data_ptr(), d_mom.data_ptr())
    r.tonemap_device(d_acc.data_ptr(), d_rgba.data_ptr(), N)
    torch.cuda.synchronize()
    same(accum, host(d_acc), "accum")
    if optional:
        same(moments, host(d_mom), "moments")
        same(tile_spp, spp, "tile_spp")
        same(rgba, host(d_rgba), "rgba8")


@pytest.mark.parametrize("optional", [False, True], ids=["out_only", "all_buffers"])
def test_render_final(torch_cuda, renderer, frames, optional):
    """accum, moments, out_variance, tile_spp and out_rgba8 NULL, and all five supplied"""
    from octree_pathtracing_amd import _lib

    torch, r = torch_cuda, renderer
    p = r.params(W, H, 0, 8)
    f = _lib.FinalParams(adaptive_params(True),
                         _lib.DenoiseVarianceParams(W, H, 2, 4.0, 1e-2, 0.3, 0.1, _lib.DENOISE_DEMODULATE))
    out = np.zeros((H, W, 4), np.float32)
    opt = ({"accum": np.zeros((H, W, 4), np.float32), "moments": np.zeros((H, W, 2), np.float32),
            "out_variance": np.zeros((H, W), np.float32), "tile_spp": np.zeros(T, np.uint32),
            "rgba": np.zeros((H, W, 4), np.uint8)} if optional else {})
    r._check(r._lib.octpt_render_final(r._ctx, C.byref(p), C.byref(f), ptr(opt.get("accum")), ptr(opt.get("moments")),
                                       ptr(out), ptr(opt.get("out_variance")), ptr(opt.get("tile_spp")),
                                       ptr(opt.get("rgba")), None))
    d = {k: torch.zeros(s, dtype=torch.float32, device="cuda")
         for k, s in (("accum", (H, W, 4)), ("moments", (H, W, 2)), ("out", (H, W, 4)), ("out_variance", (H, W)))}
    d_rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    spp, _ = r.render_final_device(p, f, d["accum"].data_ptr(), d["moments"].data_ptr(), d["out"].data_ptr(),
                                   d["out_variance"].data_ptr())
    r.tonemap_device(d["out"].data_ptr(), d_rgba.data_ptr(), N)
    torch.cuda.synchronize()
    same(out, host(d["out"]), "out")
    for k in ("accum", "moments", "out_variance"):
        if optional:
            same(opt[k], host(d[k]), k)
    if optional:
        same(opt["tile_spp"], spp, "tile_spp")
        same(opt["rgba"], host(d_rgba), "rgba8")


def test_refused_call_leaves_the_buffers_alone(renderer, frames):
    """check_denoise's refusal of iterations = 6: the status, its message, and an untouched output"""
    from octree_pathtracing_amd import _lib

    aov = frames["aov"]
    p = _lib.DenoiseParams(W, H, 6, 0.6, 0.3, 0.1, 0)
    b = _lib.AovBuffers(normal=aov["normal"].ctypes.data, depth=aov["depth"].ctypes.data)
    color = frames["color"].copy()
    out = np.full((H, W, 4), -5.0, np.float32)
    st = renderer._lib.octpt_denoise(renderer._ctx, C.byref(p), ptr(color), C.byref(b), ptr(out))
    assert st == _lib.ERR_INVALID_ARG
    assert renderer._lib.octpt_last_error(renderer._ctx).decode() == "denoise: iterations must be 1..5"
    assert (out == -5.0).all() and np.array_equal(bits(color), bits(frames["color"]))


def test_two_entry_context_answers_as_one_device(torch_cuda, renderer, frames):
    """octpt_create_multi over [0, 0]: a host entry forwarded to the first entry's replica"""
    r2 = tiny_renderer(devices=[0, 0])
    try:
        assert r2.device_entries == 2
        same(r2.variance(frames["history"], frames["aov"], min_history=1), frames["variance"], "variance")
        same(r2.tile_error(frames["moments"], frames["tile_spp"]), frames["error"], "tile error")
        same(r2.render_aov(frames["rs"], which=("depth",))["depth"], frames["aov"]["depth"], "depth guide")
    finally:
        r2.close()
