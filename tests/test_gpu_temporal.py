"""Temporal reprojection of the preview history (octpt_temporal, temporal_kernel) against the f32
numpy restatement of the contract (tests/temporal_ref.py), the host mirror of its mapping, and the properties the
contract promises: the running mean under a static camera, the rejections, the call forms and the refusals that
need a context."""
import ctypes as C

import numpy as np
import pytest

from tests.temporal_ref import temporal_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
REL, ABS = 1e-5, 1e-6  # the project's forward tolerance, as tests/test_gpu_denoise.py


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


def close(got, ref):
    return np.abs(got - ref) <= REL * np.abs(ref) + ABS


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def moved(cam, right=0.0, up=0.0, forward=0.0, yaw=0.0):
    """cam translated along its own axes and turned by `yaw` radians towards its right."""
    from octree_pathtracing_amd.scene import Camera

    d, u = np.asarray(cam.direction, np.float64), np.asarray(cam.up, np.float64)
    r = np.cross(d, u)
    eye = np.asarray(cam.eye, np.float64) + right * r + up * u + forward * d
    c = Camera.look_at(tuple(eye), tuple(eye + np.cos(yaw) * d + np.sin(yaw) * r), up=tuple(u))
    c.fov = cam.fov
    return c


@pytest.fixture(scope="module")
def frames(renderer):
    """(W, H) -> the C3 frames of a camera move, computed once: `prev` (colour at 4 spp, guides, camera) and `cur`
    (2 spp, guides, camera: translated by 3 to the right, 1 down, 2 forward and yawed by 0.02 rad -- about a pixel
    at these sizes, the scene 150 to 400 away and its spheres a pixel or two across, so that some pixels keep their
    surface and many do not)."""
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.scene import RenderSettings

    sc, cam0, _ = S.make_config("C3")
    cam1 = moved(cam0, right=3.0, up=-1.0, forward=2.0, yaw=0.02)
    renderer.set_scene(sc)
    out = {}
    for W, H in [(64, 64), (37, 21)]:
        f = {}
        for name, cam, spp in (("prev", cam0, 4), ("cur", cam1, 2)):
            renderer.set_camera(cam)
            rs = RenderSettings(W, H, spp)
            color, _ = renderer.render(rs)
            f[name] = (color, renderer.render_aov(rs), cam)
        out[(W, H)] = f
    return out


def two_frame_history(renderer, f):
    """The history after two static frames at the previous camera (lengths 2 on hits)."""
    color, aov, cam = f["prev"]
    renderer.set_camera(cam)
    h = renderer.temporal(color, aov)
    return renderer.temporal(color[::-1, ::-1].copy(), aov, h)


@pytest.mark.parametrize("match_prim", [True, False], ids=["match_prim", "any_prim"])
@pytest.mark.parametrize("size", [(64, 64), (37, 21)], ids=["64x64", "37x21"])
def test_moving_camera_matches_restatement(renderer, frames, size, match_prim):
    """Lengths equal the restatement's exactly, colour within 1e-5 relative + 1e-6 absolute; alpha and miss
    pixels bit-identical to the input; pixels with history, disoccluded pixels and misses all occur."""
    f = frames[size]
    hist = two_frame_history(renderer, f)
    color, aov, cam = f["cur"]
    renderer.set_camera(cam)
    kw = dict(max_history=32, depth_tolerance=0.1, normal_threshold=0.9, match_prim=match_prim)
    got = renderer.temporal(color, aov, hist, **kw)
    assert got["camera"] is cam and got["depth"] is aov["depth"]
    ref, ref_len = temporal_ref(color, aov, hist, cam, f["prev"][2], **kw)
    hit = np.isfinite(aov["depth"])
    n_bad = int((got["length"] != ref_len).sum())
    err = np.abs(got["color"] - ref)
    print(f"{size} match_prim={match_prim}: length mismatches {n_bad}, max colour error {err.max():.3e}, "
          f"history {int((ref_len > 1).sum())}, disoccluded {int(((ref_len == 1) & hit).sum())}, "
          f"misses {int((~hit).sum())}")
    assert (ref_len[hit] == 3).any(), "no pixel carries its history"
    assert (ref_len[hit] == 1).any(), "no disoccluded pixel"
    assert (~hit).any() and np.all(ref_len[~hit] == 0), "no miss"
    assert n_bad == 0
    assert np.all(np.isfinite(got["color"]))
    bad = ~close(got["color"], ref)
    assert not bad.any(), (int(bad.sum()), float(err.max()))
    assert np.array_equal(bits(got["color"][~hit]), bits(color[~hit]))
    assert np.array_equal(bits(got["color"][..., 3]), bits(color[..., 3]))
    # the blend does something: a pixel with history is not the input
    assert np.abs(got["color"][ref_len == 3] - color[ref_len == 3]).max() > 1e-3


def flat_guides(H, W, depth=10.0):
    normal = np.zeros((H, W, 4), F32)
    normal[..., 2] = 1.0
    return {"normal": normal, "depth": np.full((H, W), depth, F32), "prim": np.zeros((H, W), np.uint32)}


def test_device_mapping_matches_the_host_mirror(renderer):
    """A previous frame whose colour holds its own pixel coordinates, every tap valid (flat guides, the depth
    tolerance wide open), a translated camera, current colour 0 and history length 1: out = h + (0 - h) / 2 =
    h / 2 exactly, and h, the bilinear mean of a linear function, is (fx, fy).  Where all four taps lie in the
    image the kernel reproduces octpt_reproject_coords' (fx, fy) to the colour tolerance: terms of one sign, a
    handful of roundings of 2^-24 each."""
    from octree_pathtracing_amd.renderer import reproject_coords
    from octree_pathtracing_amd.scene import Camera

    W, H = 70, 45
    cur = Camera.look_at((3.0, 2.0, -1.0), (3.5, 2.5, 9.0))
    prev = moved(cur, right=0.8, up=-0.45, forward=0.3)
    g = flat_guides(H, W)
    X, Y = np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32))
    hist = dict(g, color=np.stack([X, Y, np.zeros_like(X), np.ones_like(X)], -1).astype(F32),
                length=np.ones((H, W), np.uint32))
    renderer.set_camera(cur)
    got = renderer.temporal(np.zeros((H, W, 4), F32), g, hist, prev_camera=prev, max_history=2, depth_tolerance=1e3,
                            normal_threshold=-1.0, match_prim=False)
    xy, _ = reproject_coords(cur, prev, W, H, g["depth"])
    inner = (xy[..., 0] >= 0) & (xy[..., 0] < W - 1) & (xy[..., 1] >= 0) & (xy[..., 1] < H - 1)
    assert inner.sum() > W * H // 2 and (~inner).any()
    assert np.all(got["length"][inner] == 2)
    h = F32(2.0) * got["color"][..., :2]
    assert np.abs(xy[inner] - np.stack([X, Y], -1)[inner]).max() > 1.0  # the move is more than a pixel
    bad = ~close(h[inner], xy[inner])
    assert not bad.any(), (int(bad.sum()), float(np.abs(h[inner] - xy[inner]).max()))


@pytest.mark.parametrize("max_history", [32, 3])
def test_static_camera_accumulates_the_running_mean(renderer, frames, max_history):
    """K = 6 frames of constant colours over real guides: after frame k the history is the running mean of the
    constants (1e-5 relative) and every hit pixel's length is min(k, max_history); with max_history = 3 the
    blend is the exponential one, weight 1/3, from frame 3 on."""
    _, aov, cam = frames[(64, 64)]["prev"]
    renderer.set_camera(cam)
    hit = np.isfinite(aov["depth"])
    hist, mean = None, np.zeros(3)
    for k in range(1, 7):
        c = np.array([0.05 + 0.1 * k, 0.9 / k, 0.3 + 0.07 * (k % 3)])
        color = np.empty((64, 64, 4), F32)
        color[...] = (*c, 1.0)
        hist = renderer.temporal(color, aov, hist, max_history=max_history)
        n = min(k, max_history)
        mean = mean + (c - mean) / n
        assert np.array_equal(hist["length"][hit], np.full(int(hit.sum()), n, np.uint32)), k
        assert np.all(hist["length"][~hit] == 0)
        assert np.all(np.abs(hist["color"][hit][:, :3] - mean) <= 1e-5 * np.abs(mean)), k
        assert np.array_equal(bits(hist["color"][~hit]), bits(color[~hit]))


def test_a_far_move_resets_every_pixel(renderer, frames):
    """The previous camera turned by 2 rad: no pixel lands in its frame (part of the scene is behind it)."""
    f = frames[(64, 64)]
    hist = two_frame_history(renderer, f)
    color, aov, cam = f["cur"]
    renderer.set_camera(cam)
    got = renderer.temporal(color, aov, hist, prev_camera=moved(f["prev"][2], yaw=2.0))
    hit = np.isfinite(aov["depth"])
    assert np.array_equal(bits(got["color"]), bits(color))
    assert np.array_equal(got["length"], hit.astype(np.uint32))


def test_prim_mismatch_resets_only_with_match_prim(renderer, frames):
    f = frames[(64, 64)]
    color, aov, cam = f["prev"]
    renderer.set_camera(cam)
    hist = renderer.temporal(color, aov)
    hist["prim"] = aov["prim"] ^ np.uint32(1)
    hit = np.isfinite(aov["depth"])
    other = (color * F32(0.5)).astype(F32)
    got = renderer.temporal(other, aov, hist, match_prim=True)
    assert np.array_equal(bits(got["color"]), bits(other))
    assert np.array_equal(got["length"], hit.astype(np.uint32))
    kept = renderer.temporal(other, aov, hist, match_prim=False)
    assert np.array_equal(kept["length"], 2 * hit.astype(np.uint32))


def step_case(kind):
    """Left of column 20 one colour, right of it another, in the history and the current frame alike; across
    the column either the depth steps (10 | 20) or the normal does (+Z | +X).  The previous camera is the
    current one turned by 0.01 rad about its own eye -- a third of a pixel, so each pixel's taps straddle its
    neighbour and zp is the pixel's depth again."""
    from octree_pathtracing_amd.scene import Camera

    H, W, X = 33, 45, 20
    g = flat_guides(H, W)
    if kind == "depth":
        g["depth"][:, X:] = 20.0
    else:
        g["normal"][:, X:] = (1.0, 0.0, 0.0, 0.0)
    color = np.empty((H, W, 4), F32)
    color[:, :X] = (0.9, 0.2, 0.1, 1.0)
    color[:, X:] = (0.1, 0.3, 0.8, 1.0)
    cur = Camera(eye=(0.0, 0.0, 0.0))
    return color, g, cur, moved(cur, yaw=0.01)


@pytest.mark.parametrize("kind", ["depth", "normal"])
def test_the_two_sides_of_a_step_do_not_mix(renderer, kind):
    """depth_tolerance = 1e-6 across a depth step, normal_threshold = 0.999 across a normal step: every counted
    tap holds the pixel's own colour, so the result is that colour to the tolerance.  (zp is the stored depth to
    3 roundings, 4e-7 relative, inside 1e-6.)  With the test wide open the columns at the step mix."""
    color, g, cur, prev = step_case(kind)
    hist = dict(g, color=color, length=np.full(color.shape[:2], 5, np.uint32))
    renderer.set_camera(cur)
    strict = dict(depth_tolerance=1e-6, normal_threshold=-1.0) if kind == "depth" else \
        dict(depth_tolerance=1e3, normal_threshold=0.999)
    got = renderer.temporal(color, g, hist, prev_camera=prev, match_prim=False, **strict)
    assert (got["length"] == 6).sum() > color.shape[0] * color.shape[1] * 3 // 4
    assert close(got["color"], color).all(), float(np.abs(got["color"] - color).max())
    loose = renderer.temporal(color, g, hist, prev_camera=prev, match_prim=False, depth_tolerance=1e3,
                              normal_threshold=-1.0)
    assert np.abs(loose["color"] - color).max() > 0.05


def device_call(renderer, torch, p, color, aov, hist, in_place):
    """octpt_temporal_device over torch tensors -> (out, length) as numpy."""
    def dev(a):  # u32 planes travel as i32 bits
        a = np.ascontiguousarray(a)
        return torch.as_tensor(a.view(np.int32) if a.dtype == np.uint32 else a, device="cuda")

    g = {k: dev(aov[k]) for k in ("normal", "depth", "prim")}
    h = {k: dev(hist[k]) for k in ("color", "normal", "depth", "prim", "length")} if hist is not None else None
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = dev(color)
        out = c if in_place else torch.zeros_like(c)
        length = torch.zeros(color.shape[:2], dtype=torch.int32, device="cuda")
        renderer.temporal_device(p, c.data_ptr(), {k: v.data_ptr() for k, v in g.items()},
                                 {k: v.data_ptr() for k, v in h.items()} if h is not None else None, out.data_ptr(),
                                 length.data_ptr(), s.cuda_stream)
    s.synchronize()
    if not in_place:
        assert np.array_equal(c.cpu().numpy(), color)  # the out-of-place input is left alone
    return out.cpu().numpy(), length.cpu().numpy().view(np.uint32)


def test_call_forms_agree(renderer, frames, torch_cuda):
    """First frame (d_prev = NULL); in place = out of place; host form = device form; a two-entry context."""
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd.renderer import HipRenderer, _c_camera

    f = frames[(64, 64)]
    hist = two_frame_history(renderer, f)
    color, aov, cam = f["cur"]
    hit = np.isfinite(aov["depth"])
    renderer.set_camera(cam)
    first = renderer.temporal(color, aov)
    assert np.array_equal(bits(first["color"]), bits(color))
    assert np.array_equal(first["length"], hit.astype(np.uint32))
    p = _lib.TemporalParams(64, 64, _c_camera(cam), _c_camera(f["prev"][2]), 32, 0.1, 0.9, _lib.TEMPORAL_MATCH_PRIM)
    d_first = device_call(renderer, torch_cuda, p, color, aov, None, False)
    assert np.array_equal(bits(d_first[0]), bits(color)) and np.array_equal(d_first[1], first["length"])
    host = renderer.temporal(color, aov, hist)
    oop = device_call(renderer, torch_cuda, p, color, aov, hist, False)
    inp = device_call(renderer, torch_cuda, p, color, aov, hist, True)
    assert (host["length"] > 1).any()
    for out, length in (oop, inp):
        assert np.array_equal(bits(out), bits(host["color"])) and np.array_equal(length, host["length"])
    with HipRenderer(devices=[0, 0]) as r2:
        assert r2.device_entries == 2
        r2.set_camera(cam)
        multi = r2.temporal(color, aov, hist)
        m_dev = device_call(r2, torch_cuda, p, color, aov, hist, False)
    assert np.array_equal(bits(multi["color"]), bits(host["color"])) and np.array_equal(multi["length"], host["length"])
    assert np.array_equal(bits(m_dev[0]), bits(host["color"])) and np.array_equal(m_dev[1], host["length"])


def test_refusals(renderer):
    """Every argument check that needs a context: INVALID_ARG (UNSUPPORTED for an aperture, octpt_set_camera's
    rule) with a message, and nothing written."""
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd.renderer import _c_camera
    from octree_pathtracing_amd.scene import Camera

    lib, ctx = renderer._lib, renderer._ctx
    W = H = 4
    g = flat_guides(H, W)
    color = np.full((H, W, 4), 0.25, F32)
    h_color, h_len = np.full((H, W, 4), 0.5, F32), np.ones((H, W), np.uint32)
    out, out_len = np.full((H, W, 4), 7.0, F32), np.full((H, W), 7, np.uint32)
    cam = Camera.look_at((3.0, 2.0, -1.0), (3.5, 2.5, 9.0))
    ptr = lambda a: a.ctypes.data  # noqa: E731

    def call(params=None, color_p=ptr(color), guides=None, prev="default", out_p=ptr(out), len_p=ptr(out_len), **over):
        f = dict(width=W, height=H, camera=_c_camera(cam), prev_camera=_c_camera(cam), max_history=32,
                 depth_tolerance=0.1, normal_threshold=0.9, flags=_lib.TEMPORAL_MATCH_PRIM)
        f.update(over)
        p = _lib.TemporalParams(*(f[k] for k, _ in _lib.TemporalParams._fields_))
        gd = dict(normal=ptr(g["normal"]), depth=ptr(g["depth"]), prim=ptr(g["prim"]))
        gd.update(guides or {})
        hd = dict(color=ptr(h_color), normal=ptr(g["normal"]), depth=ptr(g["depth"]), prim=ptr(g["prim"]),
                  length=ptr(h_len))
        if isinstance(prev, dict):
            hd.update(prev)
        b, h = _lib.AovBuffers(**gd), _lib.TemporalHistory(**hd)
        st = lib.octpt_temporal(ctx, None if params == "null" else C.byref(p), color_p, C.byref(b),
                                None if prev is None else C.byref(h), out_p, len_p)
        if st != _lib.OK:
            assert lib.octpt_last_error(ctx).decode().startswith("temporal"), st
        return st

    def c_cam(**over):
        c = _c_camera(cam)
        for k, v in over.items():
            setattr(c, k, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
        return c

    d, u = np.asarray(cam.direction), np.asarray(cam.up)
    refused = [
        dict(params="null"), dict(color_p=None), dict(out_p=None), dict(len_p=None),
        dict(guides=dict(normal=None)), dict(guides=dict(depth=None)), dict(guides=dict(prim=None)),
        dict(prev=dict(color=None)), dict(prev=dict(normal=None)), dict(prev=dict(depth=None)),
        dict(prev=dict(prim=None)), dict(prev=dict(length=None)),
        dict(width=0), dict(height=0), dict(width=1 << 16, height=1 << 15),
        dict(max_history=0), dict(max_history=65536),
        dict(depth_tolerance=0.0), dict(depth_tolerance=-1.0), dict(depth_tolerance=float("inf")),
        dict(depth_tolerance=float("nan")),
        dict(normal_threshold=1.5), dict(normal_threshold=-1.5), dict(normal_threshold=float("nan")),
        dict(flags=2), dict(flags=_lib.TEMPORAL_MATCH_PRIM | 0x10),
        dict(camera=c_cam(fov=0.0)), dict(prev_camera=c_cam(fov=3.2)),
        dict(prev_camera=c_cam(direction=tuple(d * 1.001))), dict(prev_camera=c_cam(up=tuple(u + 0.001 * d))),
        dict(prev_camera=c_cam(up=tuple(u * 0.999))),
        # the forbidden aliases
        dict(out_p=ptr(h_color)), dict(len_p=ptr(h_len)),
    ]
    for kw in refused:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert call(camera=c_cam(aperture=0.1)) == _lib.ERR_UNSUPPORTED
    assert call(prev_camera=c_cam(aperture=0.1)) == _lib.ERR_UNSUPPORTED
    assert np.all(out == 7.0) and np.all(out_len == 7)
    # what is allowed: no prim without the flag, no history, the output aliasing the current colour
    assert call(flags=0, guides=dict(prim=None), prev=dict(prim=None)) == _lib.OK
    assert call(prev=None) == _lib.OK
    assert np.array_equal(out, color) and np.all(out_len == 1)
    assert call(out_p=ptr(color)) == _lib.OK
    assert np.all(out_len == 2) and np.allclose(color[..., :3], 0.375)
