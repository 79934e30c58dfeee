"""Importance sampling of the sky map without a GPU: octpt_build_sky_distribution against the numpy
restatement of tests/sky_sample_ref.py, integer for integer; the coverage the estimator's unbiasedness rests on;
octpt_sky_sample -- the text the kernels compile (csrc/octpt_sky_sample.h) -- against float64; the unbiasedness of that
text against a quadrature of the bilinear map; the refusals that need no device; and the host builder and sample in a
stand-alone program under AddressSanitizer and UBSan (tools/sky_sample_host.cpp; nothing is loaded into Python under a
sanitizer)."""
import ctypes as C
import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd import scene as S
from octree_pathtracing_amd.scene import Sky
from tests import sky_ref as R
from tests import sky_sample_ref as SS
from tests.test_sky_cpu import POSITION_ERROR, ROUND_UP, YAWS, c_sky, rgba

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
SIZES = [(8, 4), (32, 16), (33, 17), (1, 1), (5, 1)]  # (W, H)

# The largest relative error of the host sample's pdf against the float64 expression, measured over 4000 draw tuples per
# map of SIZES and yaw of YAWS (test_host_sample_against_float64 prints the figure; DESIGN.md C43 records it).  It is
# the relative error of the sine of theta = pi v next to the nadir: the f32 product pi * v rounds at half an ulp of pi
# (1.2e-7 rad) and dm_sincos reduces by its own pi, against a sine that is as small as pi (1 - v).  The one-row maps
# (1 x 1, 5 x 1) set it, where v is the draw itself and 4000 draws reach 1 - v of a few 1e-4; the relative error of a
# sample is about 2.4e-7 / sin theta, so it stays below 1e-5 for every direction more than 1.4 degrees from the nadir.
PDF_REL_ERROR = 4.78e-4
PDF_MARGIN = 2.0


def random_map(w, h, seed=7):
    return np.random.default_rng(seed + 31 * w + h).uniform(0.5, 2.0, (h, w, 3)).astype(F32)


def bright_map(w=32, h=16):
    t = np.zeros((h, w, 3), F32)
    t[h // 4, w // 3] = (2000.0, 1500.0, 900.0)
    return t


def hostile_map(w=33, h=17):
    t = random_map(w, h)
    t[0, 0] = (np.nan, -1.0, np.inf)
    t[3, 5] = (FLT_MAX, FLT_MAX, FLT_MAX)
    t[h - 1, w - 1] = (-np.inf, 0.0, -0.0)
    return t


def draws(n, seed=11):
    return np.random.default_rng(seed).random((n, 4), dtype=F32)


def assert_equal_dist(got, want):
    assert np.array_equal(got["col_cdf"], want["col_cdf"])
    assert np.array_equal(got["row_cdf"], want["row_cdf"])
    assert got["total"] == want["total"]


# ------------------------------------------------------------------ the host builder is the definition
@pytest.mark.parametrize("size", SIZES)
def test_host_builder_against_the_restatement(size):
    t = random_map(*size)
    got, want = S.build_sky_distribution(t), SS.distribution(t)
    assert want["total"] > 0 and got["col_cdf"].dtype == np.uint32 and got["row_cdf"].dtype == np.uint64
    assert_equal_dist(got, want)
    assert SS.q_of(got).max() == 65536  # the largest weight takes the whole quantum


@pytest.mark.parametrize("name", ["hostile", "bright", "black", "flt_max"])
def test_host_builder_on_edge_maps(name):
    t = {"hostile": hostile_map(), "bright": bright_map(), "black": np.zeros((4, 8, 3), F32),
         "flt_max": np.full((4, 8, 3), FLT_MAX, F32)}[name]
    got, want = S.build_sky_distribution(t), SS.distribution(t)
    assert_equal_dist(got, want)
    if name == "black":
        assert got["total"] == 0 and not got["col_cdf"].any()
    if name == "bright":  # the texel and its eight neighbours, nothing else
        q = SS.q_of(got)
        assert (q > 0).sum() == 9 and q[3:6, 9:12].all()
    if name == "flt_max":  # weights held at FLT_MAX where the product overflows: finite, every texel sampled
        assert (SS.q_of(got) > 0).all()


@pytest.mark.parametrize("t", [random_map(33, 17), hostile_map(), bright_map(), bright_map(5, 1)], ids=range(4))
def test_coverage(t):
    """q > 0 wherever any texel of the 3 x 3 neighbourhood has lum > 0: the footprint of every bilinear lookup that can
    be non-zero."""
    q = SS.q_of(S.build_sky_distribution(t))
    lit = SS.neighbourhood_max(SS.lum32(SS.sanitise(t))) > 0
    assert lit.any() and (q[lit] > 0).all() and (q[~lit] == 0).all()


# ------------------------------------------------------------------ the host sample against float64
def test_host_sample_against_float64():
    worst_pdf, worst_pos = 0.0, {}
    for (w, h) in SIZES:
        t = random_map(w, h)
        dist = S.build_sky_distribution(t)
        u = draws(4000, seed=w + h)
        for yaw in YAWS:
            got = S.sky_samples(dist, u, yaw)
            d64, pdf64, x, y = SS.sample64(dist, u, yaw)
            ok = got["ok"]
            assert ok.mean() > 0.99
            assert np.array_equal(got["x"][ok], x[ok]) and np.array_equal(got["y"][ok], y[ok])
            assert np.array_equal(got["q"][ok], SS.q_of(dist)[y, x][ok])
            d = got["d"][ok].astype(np.float64)
            assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 4 * np.finfo(F32).eps
            rel = np.abs(got["pdf"][ok] / pdf64[ok] - 1.0)
            worst_pdf = max(worst_pdf, float(rel.max()))
            if (w, h) in POSITION_ERROR:
                # the lookup's own position of the sampled direction falls into the picked texel, to within the error
                # C42 records for this size and yaw, with its 2x margin
                desc = c_sky(dict(mode=R.MAP, yaw=yaw))
                desc.width, desc.height = w, h
                xy = np.zeros((int(ok.sum()), 2), F32)
                dirs = np.ascontiguousarray(got["d"][ok])
                assert _lib.load().octpt_sky_map_position(C.byref(desc), dirs.ctypes.data, len(dirs), xy.ctypes.data) == _lib.OK
                tol = 2.0 * POSITION_ERROR[(w, h)][yaw] * ROUND_UP
                dx = (xy[:, 0].astype(np.float64) - x[ok] + w / 2.0) % w - w / 2.0  # texel x covers fx in [x - 0.5, x + 0.5)
                dy = xy[:, 1].astype(np.float64) - y[ok]
                out = np.maximum(np.maximum(np.abs(dx), np.abs(dy)) - 0.5, 0.0)
                worst_pos[(w, h, yaw)] = float(out.max())
                assert out.max() <= tol, (w, h, yaw, out.max(), tol)
    print(f"pdf relative error {worst_pdf:.3g}; position overshoot {worst_pos}")
    assert worst_pdf <= PDF_MARGIN * PDF_REL_ERROR


@pytest.mark.parametrize("name", ["random", "bright"])
def test_the_text_is_unbiased(name):
    """The mean of lum(sky_radiance(d)) / pdf over 2^18 draws against the float64 quadrature of the bilinear map over
    the sphere, within 5 standard errors of the sample's own mean."""
    t = random_map(32, 16) if name == "random" else bright_map()
    yaw = 0.7
    dist = S.build_sky_distribution(t)
    got = S.sky_samples(dist, draws(1 << 18, seed=23), yaw)
    lum = SS.lum64(Sky.map(t, yaw=yaw).radiance(got["d"]).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        est = np.where(got["ok"], lum / got["pdf"].astype(np.float64), 0.0)
    mean, se = est.mean(), est.std(ddof=1) / math.sqrt(len(est))
    want = SS.sphere_integral(t)
    print(f"{name}: estimate {mean:.6g} +- {se:.3g}, quadrature {want:.6g}")
    assert want > 0 and abs(mean - want) <= 5.0 * se


# ------------------------------------------------------------------ refusals that need no device
def test_refusals_of_the_host_entries():
    lib = _lib.load()
    t = rgba(random_map(8, 4))
    row, col = np.full(4, 7, np.uint64), np.full((4, 8), 7, np.uint32)
    for args, status in (((None, 8, 4, row.ctypes.data, col.ctypes.data), _lib.ERR_INVALID_ARG),
                         ((t.ctypes.data, 0, 4, row.ctypes.data, col.ctypes.data), _lib.ERR_INVALID_ARG),
                         ((t.ctypes.data, 8, 0, row.ctypes.data, col.ctypes.data), _lib.ERR_INVALID_ARG),
                         ((t.ctypes.data, 8, 4, None, col.ctypes.data), _lib.ERR_INVALID_ARG),
                         ((t.ctypes.data, 1 << 14, (1 << 12) + 1, row.ctypes.data, col.ctypes.data), _lib.ERR_INVALID_ARG),
                         ((t.ctypes.data, 32769, 1, row.ctypes.data, col.ctypes.data), _lib.ERR_UNSUPPORTED)):
        assert lib.octpt_build_sky_distribution(*args) == status
    assert (row == 7).all() and (col == 7).all()
    with pytest.raises(ValueError):
        S.build_sky_distribution(np.ones((1, 32769, 3), F32))
    # the setter's own rules, on a NULL context: INVALID_ARG before anything is read
    p = _lib.SkySampling()
    assert lib.octpt_set_sky_sampling(None, C.byref(p)) == _lib.ERR_INVALID_ARG
    assert lib.octpt_get_sky_sampling(None, C.byref(p)) == _lib.ERR_INVALID_ARG
    assert C.sizeof(_lib.SkySampling) == 32 and _lib.SKY_SAMPLING_NONE == 0 and _lib.SKY_SAMPLING_MAP == 1
    # the host sample: a distribution of another size than the sky's, a mode that is not MAP
    dist = S.build_sky_distribution(random_map(8, 4))
    a = _lib.SkyDistributionArrays(dist["row_cdf"].ctypes.data, 4, dist["col_cdf"].ctypes.data, 32, 8, 4, 0.0, 0)
    u, out = draws(4), np.full((4, 8), 7.0, F32)
    for w, h, mode in ((8, 5, R.MAP), (9, 4, R.MAP), (8, 4, R.COLOR)):
        d = c_sky(dict(mode=mode))
        d.width, d.height = w, h
        assert lib.octpt_sky_sample(C.byref(a), C.byref(d), 4, u.ctypes.data, out.ctypes.data) == _lib.ERR_INVALID_ARG
    assert (out == 7.0).all()


def test_all_black_map_has_no_sample():
    dist = S.build_sky_distribution(np.zeros((4, 8, 3), F32))
    got = S.sky_samples(dist, draws(64))
    assert not got["ok"].any() and not got["pdf"].any() and not got["d"].any()


# ------------------------------------------------------------------ the host entries under sanitizers
def test_host_entries_under_sanitizers(tmp_path):
    """octpt_build_sky_distribution and octpt_sky_sample in a program of their own with -fsanitize=address,undefined
    over the edge maps (1 x 1, 5 x 1, all-black, FLT_MAX, non-finite texels, one bright texel) into exact-size arrays,
    draws of 0 and of the largest float below 1 among them: clean, and every picked texel and pdf in range."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "sky_sample_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    f"-I{os.environ.get('ROCM_PATH', '/opt/rocm')}/include",
                    str(ROOT / "tools" / "sky_sample_host.cpp"),
                    str(ROOT / "octree_pathtracing_amd" / "csrc" / "octpt_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "refusals ok" and len(lines) == 13
    totals = {tuple(map(int, ln.split()[:2])): int(ln.split()[2]) for ln in lines[:-1]}
    assert int(lines[4].split()[2]) == 0  # the all-black map
    assert totals[(8, 4)] == SS.distribution(np.full((4, 8, 3), FLT_MAX, F32))["total"]  # (the FLT_MAX map, the later one)
    assert totals[(1, 1)] == 65536
    assert totals[(32, 16)] == SS.distribution(bright_line_map())["total"]


def bright_line_map():
    """tools/sky_sample_host.cpp's one-bright-texel map."""
    t = np.zeros((16, 32, 3), F32)
    t[4, 7, 1] = 2000.0
    return t
