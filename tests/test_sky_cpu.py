"""The sky without a GPU: octpt_sky_radiance, the host's statement of the colour a render adds where a
ray leaves the world -- the text the kernels compile (csrc/octpt_sky.h) -- against the float64 restatement of
tests/sky_ref.py; the exact statements of the contract (COLOR, GRADIENT, a map of equal texels); continuity across the
seam and at the poles; the refusals of the host form (a context needs a device: tests/test_gpu_sky.py holds the
context's refusals and that the previous sky stays in force); the Python surface; and the Radiance .hdr reader and
writer of octree_pathtracing_amd/sky.py."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd import sky as hdr
from octree_pathtracing_amd.scene import Sky
from tests import sky_ref as R

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
W, H = 32, 16
YAWS = [0.0, 0.7, -2.5, math.pi, 100.0]

# The largest lookup-position error of the host text against float64, |dx| + |dy| in texels (dx taken round the map),
# measured per map size and yaw over direction_set of that size (test_map_position_error prints the figures and holds
# the code to them; DESIGN.md C42 records them).  The error grows with the map's width (texels per radian) and with
# |yaw|: the f32 sum lon + yaw rounds at the yaw's scale (half an ulp of 100 is 3.8e-6 rad, 32 / 2 pi = 5.1 texels per
# radian, and the division and the product by W round at that scale too).  Each case is bounded by its own figure.
POSITION_ERROR = {
    (32, 16): {0.0: 2.8e-6, 0.7: 3.95e-6, -2.5: 3.96e-6, math.pi: 5.37e-6, 100.0: 7.81e-5},
    (8, 4): {0.0: 6.99e-7, 0.7: 9.88e-7, -2.5: 9.91e-7, math.pi: 1.34e-6, 100.0: 1.95e-5},
}
ROUND_UP = 1.005  # the figures above are printed to three digits


def lookup_bound(t, size, yaw, scale=1.0):
    """What a MAP lookup may differ from float64 by: the case's measured position error with the 2x margin for
    directions outside the measured set, times the largest difference between neighbouring texels (the bilinear
    surface's slope per texel, in x plus in y), plus 8 ulp of the largest value for the three lerps and the scale."""
    e = POSITION_ERROR[size][yaw] * ROUND_UP
    return (2.0 * e * R.neighbour_difference(t) + 8.0 * float(np.finfo(F32).eps) * float(t.max())) * scale


def c_sky(sky: dict) -> "_lib.SkyDesc":
    d = _lib.SkyDesc()
    d.mode = sky.get("mode", 0)
    d.color[:] = sky.get("color", (0, 0, 0))
    d.horizon[:] = sky.get("horizon", (0, 0, 0))
    d.zenith[:] = sky.get("zenith", (0, 0, 0))
    d.scale = sky.get("scale", 1.0)
    d.yaw = sky.get("yaw", 0.0)
    if "texels" in sky:
        d.height, d.width = sky["texels"].shape[:2]
    return d


def rgba(texels):
    t = np.ones(texels.shape[:2] + (4,), F32)
    t[..., :texels.shape[2]] = texels
    return np.ascontiguousarray(t)


def host_radiance(sky: dict, dirs, desc=None, out=None):
    """(status, out): octpt_sky_radiance."""
    dirs = np.ascontiguousarray(dirs, F32).reshape(-1, 3)
    out = np.zeros_like(dirs) if out is None else out
    tex = rgba(sky["texels"]) if "texels" in sky else None
    d = desc if desc is not None else c_sky(sky)
    st = _lib.load().octpt_sky_radiance(C.byref(d), tex.ctypes.data if tex is not None else None, dirs.ctypes.data,
                                        len(dirs), out.ctypes.data)
    return st, out


def sample_map(w=W, h=H, seed=3):
    """A map with structure at every scale the lookup sees: smooth gradients plus per-texel noise, HDR range."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    t = np.stack([0.5 + 0.5 * np.sin(2 * np.pi * x / w), (y + 0.5) / h, 0.25 + 0.0 * x], -1)
    t = t + rng.uniform(0.0, 0.5, t.shape)
    t[h // 4, w // 3] = (40.0, 30.0, 20.0)  # one bright texel
    return t.astype(F32)


def test_color_and_gradient_are_exact():
    dirs = R.direction_set(W, H)
    col, sc = (0.3, 1.7, 0.05), 2.5
    st, got = host_radiance(dict(mode=R.COLOR, color=col, scale=sc), dirs)
    assert st == _lib.OK
    want = np.asarray(col, F32) * F32(sc)
    assert np.array_equal(got.view(np.uint32), np.broadcast_to(want, got.shape).view(np.uint32))
    hz, ze = np.asarray((0.9, 0.8, 0.7), F32), np.asarray((0.1, 0.3, 1.5), F32)
    st, got = host_radiance(dict(mode=R.GRADIENT, horizon=hz, zenith=ze, scale=sc), dirs)
    assert st == _lib.OK
    t = np.maximum(dirs[:, 1], F32(0.0))[:, None]
    want = (hz + (ze - hz) * t) * F32(sc)  # the contract's expression in numpy f32: every operation rounds once
    assert want.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    below = dirs[:, 1] <= 0
    assert below.any() and np.array_equal(got[below], np.broadcast_to(hz * F32(sc), got[below].shape))
    # DEFAULT is the constant, whatever the other fields hold
    st, got = host_radiance(dict(mode=R.DEFAULT, color=col, scale=9.0), dirs)
    assert st == _lib.OK and np.array_equal(got, np.broadcast_to(np.asarray((0.5, 0.7, 1.0), F32), got.shape))


def position_error(w, h, yaw, dirs):
    d = c_sky(dict(mode=R.MAP, yaw=yaw))
    d.width, d.height = w, h
    xy = np.zeros((len(dirs), 2), F32)
    assert _lib.load().octpt_sky_map_position(C.byref(d), dirs.ctypes.data, len(dirs), xy.ctypes.data) == _lib.OK
    fx, fy = R.map_position(dirs, w, h, float(F32(yaw)))
    dx = (xy[:, 0].astype(np.float64) - fx + w / 2.0) % w - w / 2.0
    dy = xy[:, 1].astype(np.float64) - fy
    return np.abs(dx) + np.abs(dy)


def test_map_position_error():
    """The measurement behind POSITION_ERROR: printed, and each case held to its own figure (the bound
    test_map_against_float64 uses carries a further 2x for directions outside this set)."""
    worst = {}
    for (w, h) in ((32, 16), (8, 4)):
        dirs = R.direction_set(w, h)
        for yaw in YAWS:
            worst[(w, h, yaw)] = float(position_error(w, h, yaw, dirs).max())
    print({k: f"{v:.3g}" for k, v in worst.items()})
    for (w, h, yaw), v in worst.items():
        assert v <= POSITION_ERROR[(w, h)][yaw] * ROUND_UP, (w, h, yaw)


@pytest.mark.parametrize("size", [(32, 16), (8, 4)])
@pytest.mark.parametrize("yaw", YAWS)
def test_map_against_float64(size, yaw):
    """MAP differs from float64 only through the f32 atan2 / acos (the position) and the lerps: lookup_bound, per map
    size and yaw."""
    w, h = size
    t = sample_map(w, h)
    sky = dict(mode=R.MAP, texels=t, yaw=yaw, scale=1.5)
    dirs = R.direction_set(w, h)
    st, got = host_radiance(sky, dirs)
    assert st == _lib.OK and np.isfinite(got).all()
    want = R.radiance(dict(sky, yaw=float(F32(yaw)), scale=1.5), dirs)
    bound = lookup_bound(t, size, yaw, 1.5)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"{w}x{h} yaw {yaw}: max err {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_texel_centres_return_the_texels():
    """The arithmetic puts a texel centre's direction on its texel: within the same bound of the map itself."""
    t = sample_map()
    dirs = R.texel_centre_dirs(W, H).reshape(-1, 3).astype(F32)
    st, got = host_radiance(dict(mode=R.MAP, texels=t), dirs)
    assert st == _lib.OK
    assert np.abs(got.astype(np.float64) - t.reshape(-1, 3)).max() <= lookup_bound(t, (W, H), 0.0)


@pytest.mark.parametrize("size", [(32, 16), (8, 4), (1, 1), (2, 1), (1, 3)])
def test_uniform_map_is_its_texel_times_scale(size):
    w, h = size
    texel = np.asarray((0.37, 11.5, 1e-3), F32)
    t = np.broadcast_to(texel, (h, w, 3)).astype(F32)
    dirs = R.direction_set(W, H)
    for yaw in YAWS:
        st, got = host_radiance(dict(mode=R.MAP, texels=t, yaw=yaw, scale=3.0), dirs)
        assert st == _lib.OK
        want = np.broadcast_to(texel * F32(3.0), got.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_continuity_across_the_seam_and_at_the_poles():
    t = sample_map()
    D = R.neighbour_difference(t)
    sky = dict(mode=R.MAP, texels=t)

    def look(d):
        return host_radiance(sky, np.asarray(d, F32))[1].astype(np.float64)

    # the seam lon = +-pi at yaw 0: directions a small angle either side of -x see nearly the same colour
    for y in (-0.8, 0.0, 0.5):
        r = math.sqrt(1.0 - y * y)
        for eps in (1e-6, 1e-4):
            a, b = look([[-r * math.cos(eps), y, r * math.sin(eps)]]), look([[-r * math.cos(eps), y, -r * math.sin(eps)]])
            step = 2.0 * eps / (2.0 * math.pi) * W  # texels between the two
            assert np.abs(a - b).max() <= (step + 2.0 * POSITION_ERROR[(W, H)][0.0] * ROUND_UP) * D + 1e-5
    # the poles: along the meridian of longitude 0 (+x) the value tends to the pole's, which is the row's at lon = yaw
    for sgn in (1.0, -1.0):
        pole = look([[0.0, sgn, 0.0]])
        assert np.array_equal(pole, look([[-0.0, sgn, 0.0]])) and np.array_equal(pole, look([[0.0, sgn, -0.0]]))
        for eps in (1e-3, 1e-5):
            near = look([[math.sin(eps), sgn * math.cos(eps), 0.0]])
            step = eps / math.pi * H
            assert np.abs(near - pole).max() <= (step + 2.0 * POSITION_ERROR[(W, H)][0.0] * ROUND_UP) * D + 1e-5
        row = t[0 if sgn > 0 else H - 1].astype(np.float64)
        # u = 0.5 at yaw 0: fx = W / 2 - 0.5, half way between columns W/2 - 1 and W/2
        assert np.allclose(pole[0], 0.5 * (row[W // 2 - 1] + row[W // 2]), rtol=1e-6, atol=0)


def test_sanitised_texels():
    """NaN and negative texels read as 0, +inf as FLT_MAX, and the result stays finite under a scale above 1."""
    t = np.zeros((4, 8, 3), F32)
    t[..., 0] = np.nan
    t[..., 1] = -5.0
    t[..., 2] = np.inf
    dirs = R.direction_set(8, 4, n_random=200)
    st, got = host_radiance(dict(mode=R.MAP, texels=t, scale=2.0), dirs)
    assert st == _lib.OK and np.isfinite(got).all()
    assert (got[:, :2] == 0.0).all() and (got[:, 2] == np.finfo(F32).max).all()


def test_host_form_refusals_write_nothing():
    t = sample_map(8, 4)
    dirs = R.direction_set(8, 4, n_random=10)
    nan, inf = float("nan"), float("inf")
    good = dict(mode=R.MAP, texels=t, scale=1.0, yaw=0.0)
    assert host_radiance(good, dirs)[0] == _lib.OK

    def refused(desc, sky=good):
        out = np.full((len(dirs), 3), 123.25, F32)
        st, out = host_radiance(sky, dirs, desc=desc, out=out)
        assert st == _lib.ERR_INVALID_ARG and (out == 123.25).all()

    for field, bad in (("mode", 4), ("mode", 0xFFFFFFFF), ("scale", nan), ("scale", -1.0), ("scale", inf),
                       ("yaw", nan), ("yaw", inf), ("yaw", -inf), ("width", 0), ("height", 0)):
        d = c_sky(good)
        setattr(d, field, bad)
        refused(d)
    d = c_sky(good)
    d.width, d.height = 1 << 14, (1 << 12) + 1  # over the 2^26-texel cap (checked before any texel is read)
    refused(d)
    d = c_sky(good)
    d.reserved[1] = 1
    refused(d)
    refused(c_sky(good), sky=dict(mode=R.MAP))  # MAP with NULL texels
    for mode in (R.COLOR, R.GRADIENT):  # scale and yaw are checked in every mode but DEFAULT
        d = c_sky(dict(mode=mode, scale=nan))
        refused(d, sky=dict(mode=mode))
    lib = _lib.load()
    assert lib.octpt_sky_radiance(None, None, dirs.ctypes.data, 1, dirs.ctypes.data) == _lib.ERR_INVALID_ARG
    assert lib.octpt_sky_radiance(C.byref(c_sky(dict(mode=R.COLOR))), None, None, 1, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_set_sky(None, C.byref(c_sky(good)), None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_clear_sky(None) == _lib.ERR_INVALID_ARG


def test_python_sky():
    t = sample_map(8, 4)
    dirs = R.direction_set(8, 4, n_random=50)
    for sky, ref in ((Sky(), dict(mode=R.DEFAULT)),
                     (Sky.color((0.1, 0.2, 0.3), 2.0), dict(mode=R.COLOR, color=(0.1, 0.2, 0.3), scale=2.0)),
                     (Sky.gradient((1, 1, 1), (0, 0, 1), 0.5), dict(mode=R.GRADIENT, horizon=(1, 1, 1), zenith=(0, 0, 1), scale=0.5)),
                     (Sky.map(t, yaw=0.3, scale=2.0), dict(mode=R.MAP, texels=t, yaw=0.3, scale=2.0)),
                     (Sky.map(rgba(t)), dict(mode=R.MAP, texels=t))):
        got = sky.radiance(dirs)
        assert np.array_equal(got.view(np.uint32), host_radiance(ref, dirs)[1].view(np.uint32))
    assert Sky.map(t).texels.shape == (4, 8, 4) and Sky.map(t).texels.dtype == F32
    with pytest.raises(ValueError):
        Sky.map(np.zeros((4, 8), F32))
    with pytest.raises(ValueError):
        Sky.color((1, 1, 1), float("nan")).radiance(dirs)


# ------------------------------------------------------------------ Radiance .hdr
def rgbe_bound(img):
    """RGBE's quantisation: 1/256 of the pixel's largest channel."""
    return img.max(axis=2, keepdims=True) / 256.0


@pytest.mark.parametrize("rle", [True, False], ids=["rle", "flat"])
@pytest.mark.parametrize("size", [(32, 16), (8, 4), (7, 3), (200, 2)])
def test_hdr_round_trip(tmp_path, size, rle):
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    img = np.exp(rng.uniform(-12.0, 12.0, (h, w, 3))).astype(F32)  # 1e-5 .. 1e5
    img[0, :, :] = 0.75                       # a run the encoder packs
    img[-1, : w // 2] = 0.0                   # black: e = 0
    img[h // 2, w // 2] = (255.9 / 256.0, 0.1, 0.1)  # a mantissa that rounds up to the next exponent
    p = tmp_path / "m.hdr"
    hdr.write_hdr(p, img, rle=rle)
    raw = p.read_bytes()
    body = raw[raw.index(b"+X") :].split(b"\n", 1)[1]
    assert (len(body) == w * h * 4) == (not (rle and w >= 8))  # flat is flat; 7 wide cannot be run-length encoded
    back = hdr.read_hdr(p)
    assert back.shape == (h, w, 3) and back.dtype == F32
    assert (np.abs(back.astype(np.float64) - img) <= rgbe_bound(img.astype(np.float64))).all()
    assert np.array_equal(back[0], np.full((w, 3), 0.75, F32)) and (back[-1, : w // 2] == 0.0).all()


def test_hdr_golden_file():
    """A hand-made 8 x 2 file, its first scanline run-length encoded (a run, then literals) and its second flat."""
    got = hdr.read_hdr(ROOT / "tests" / "golden" / "sky_8x2.hdr")
    assert got.shape == (2, 8, 3)
    # row 0: r = 128 at e = 129 (= 1.0) in all eight, g = 0..7 literals (x / 128), b = 64 (= 0.5)
    assert np.array_equal(got[0, :, 0], np.full(8, 1.0, F32))
    assert np.array_equal(got[0, :, 1], (np.arange(8) / 128.0).astype(F32))
    assert np.array_equal(got[0, :, 2], np.full(8, 0.5, F32))
    # row 1, flat: pixel x = (x, 2x, 3x) at e = 136 (byte values themselves); the last pixel has e = 0: black
    want = np.stack([np.arange(8), 2 * np.arange(8), 3 * np.arange(8)], -1).astype(F32)
    want[7] = 0.0
    assert np.array_equal(got[1], want)
    with pytest.raises(ValueError):
        hdr.read_hdr(ROOT / "tests" / "golden" / "c3_rays.npz")
