"""Luminance moments, variance and the variance-guided filter without a GPU: the new structs'
ctypes mirrors against the header, the entries' NULL-context refusals, and the numpy restatements of the three rows
(tests/svgf_ref.py) on cases whose answers are known in closed form."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from octree_pathtracing_amd.scene import Camera
from tests.svgf_ref import denoise_variance_ref, luminance, temporal_moments_ref, variance_ref

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "octpt.h"
F32 = np.float32
F64 = np.float64

NEW_STRUCTS = {"octpt_variance_params": "VarianceParams", "octpt_denoise_variance_params": "DenoiseVarianceParams"}


def test_new_struct_layouts_match_gcc(tmp_path):
    """Sizes, alignments and every field offset, by the compiler probe of tests/test_abi_cpu.py."""
    probe = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for c_name, mirror in NEW_STRUCTS.items():
        lines.append(f'    printf("{c_name} %zu %zu\\n", sizeof({c_name}), _Alignof({c_name}));')
        for field, _ in getattr(_lib, mirror)._fields_:
            lines.append(f'    printf("{c_name}.{field} %zu 0\\n", offsetof({c_name}, {field}));')
    lines.append('    printf("OCTPT_TEMPORAL_DEMODULATE %u 0\\n", OCTPT_TEMPORAL_DEMODULATE);')
    lines.append("    return 0;\n}")
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        name, size, align = line.split()
        if name == "OCTPT_TEMPORAL_DEMODULATE":
            assert int(size) == _lib.TEMPORAL_DEMODULATE == 2
        elif "." in name:
            c_name, field = name.split(".")
            assert getattr(getattr(_lib, NEW_STRUCTS[c_name]), field).offset == int(size), name
        else:
            mirror = getattr(_lib, NEW_STRUCTS[name])
            assert C.sizeof(mirror) == int(size), (name, C.sizeof(mirror), size)
            assert C.alignment(mirror) == int(align)
        seen += 1
    assert seen == 2 + 5 + 8 + 1


def test_abi_version_is_still_4():
    assert _lib.load().octpt_abi_version() == _lib.OCTPT_ABI_VERSION == 4


def test_null_context_calls_fail_cleanly():
    lib = _lib.load()
    assert lib.octpt_temporal_moments(None, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_temporal_moments_device(None, None, None, None, None, None, None, None, None, None) == \
        _lib.ERR_INVALID_ARG
    assert lib.octpt_variance(None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_variance_device(None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_denoise_variance(None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.octpt_denoise_variance_device(None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG


def flat_guides(H, W, depth=10.0):
    normal = np.zeros((H, W, 4), F32)
    normal[..., 2] = 1.0
    return {"normal": normal, "depth": np.full((H, W), depth, F32), "prim": np.zeros((H, W), np.uint32),
            "albedo": np.full((H, W, 4), 0.5, F32)}


COLOURS = [np.array([0.05 + 0.1 * k, 0.9 / k, 0.3 + 0.07 * (k % 3)]) for k in range(1, 7)]


def constant_frames(H, W):
    for c in COLOURS:
        color = np.empty((H, W, 4), F32)
        color[...] = (*c, 1.0)
        yield color


@pytest.mark.parametrize("max_history", [32, 3])
def test_static_frames_give_the_running_means_and_the_population_variance(max_history):
    """K = 6 static frames of per-frame constant colours over flat guides with a miss column.  With identical
    cameras a pixel maps onto itself to a few 1e-2 of a pixel (tests/test_temporal_cpu.py), and every tap holds the
    same moments, so the history moments are the previous frame's constants whatever the bilinear weights: after
    frame k the moments are the running means of l and l^2 (the exponential blend with weight 1 / max_history from
    there on), and with min_history = 1 C28's variance is m2 - m1^2, the population variance of the l sequence
    while the mean is the running one.  1e-5 relative on the moments (a handful of f32 roundings per frame); the
    variance is a difference of them, so its bound is relative to its terms, 1e-5 (m2 + m1^2)."""
    H, W = 12, 20
    g = flat_guides(H, W)
    g["depth"][:, 7] = np.inf
    hit = np.isfinite(g["depth"])
    cam = Camera.look_at((3.0, 2.0, -1.0), (3.5, 2.5, 9.0))
    hist, m1, m2, ls = None, 0.0, 0.0, []
    for k, color in enumerate(constant_frames(H, W), 1):
        m, length = temporal_moments_ref(color, g, hist, cam, cam, max_history=max_history)
        assert m.dtype == F32
        hist = dict(g, color=color, length=length, moments=m)
        l = float(luminance(color[0, 0, :3].astype(F64), F64))
        ls.append(l)
        n = min(k, max_history)
        m1, m2 = m1 + (l - m1) / n, m2 + (l * l - m2) / n
        assert np.all(length[hit] == n) and np.all(length[~hit] == 0), k
        assert np.all(np.abs(m[hit] - (m1, m2)) <= 1e-5 * np.abs((m1, m2))), k
        assert np.all(m[~hit] == 0)
        v = variance_ref(m, length, g["normal"], g["depth"], min_history=1)
        assert np.all(np.abs(v[hit] - (m2 - m1 * m1)) <= 1e-5 * (m2 + m1 * m1) + 1e-6), k
        assert np.all(v[~hit] == 0) and np.all(v >= 0)
        if k <= max_history:
            assert abs((m2 - m1 * m1) - np.var(ls)) <= 1e-12
    assert np.var(ls) > 1e-3  # the sequence does vary


def test_first_frame_and_demodulation():
    """No history: out_m = mu = (l(s), l(s)^2) on hits and (0, 0) on misses, s = color / max(albedo, 1e-3) with
    demodulate; an albedo below the floor divides by the floor."""
    H, W = 5, 6
    g = flat_guides(H, W)
    g["depth"][2, 3] = np.inf
    g["albedo"][0, 0] = (1e-6, 0.25, 2.0, 1.0)
    color = np.random.default_rng(3).uniform(0.0, 2.0, (H, W, 4)).astype(F32)
    cam = Camera.look_at((3.0, 2.0, -1.0), (3.5, 2.5, 9.0))
    for demodulate in (False, True):
        m, length = temporal_moments_ref(color, g, None, cam, cam, demodulate=demodulate, dtype=F64)
        s = color[..., :3].astype(F64)
        if demodulate:
            s = s / np.maximum(g["albedo"][..., :3], F32(1e-3)).astype(F64)
        l = 0.2126 * s[..., 0] + 0.7152 * s[..., 1] + 0.0722 * s[..., 2]
        hit = np.isfinite(g["depth"])
        assert np.allclose(m[..., 0][hit], l[hit], rtol=1e-6) and np.allclose(m[..., 1][hit], (l * l)[hit], rtol=1e-6)
        assert np.all(m[~hit] == 0) and np.array_equal(length, hit.astype(np.uint32))
    assert abs(m[0, 0, 0] - (0.2126 * color[0, 0, 0] / 1e-3 + 0.7152 * color[0, 0, 1] / 0.25 +
                             0.0722 * color[0, 0, 2] / 2.0)) <= 1e-5 * m[0, 0, 0]


@pytest.mark.parametrize("min_history,N", [(4, 1), (4, 3), (100, 7)])
def test_spatial_branch_over_a_flat_plane(min_history, N):
    """Flat guides: every edge weight is expf(-0) = 1, so M is the plain mean of the window's moments.  With the
    same moments (M1, M2) everywhere the mean is (M1, M2) to a few roundings and v = (M2 - M1^2) min_history / N.
    A pixel with N >= min_history beside them takes its own moments instead, and a length-0 or miss tap is
    skipped: its (huge) moments leave no trace."""
    H, W = 11, 13
    g = flat_guides(H, W)
    M1, M2 = 0.75, 0.9
    m = np.empty((H, W, 2), F32)
    m[...] = (M1, M2)
    length = np.full((H, W), N, np.uint32)
    length[5, 6] = min_history  # long enough: the temporal estimate of its own moments
    m[5, 6] = (0.5, 0.75)
    length[2, 2] = 0  # skipped, and 0 itself
    m[2, 2] = (1e6, 1e12)
    g["depth"][8, 9] = np.inf
    m[8, 9] = (1e6, 1e12)
    v = variance_ref(m, length, g["normal"], g["depth"], min_history=min_history)
    want = (M2 - M1 * M1) * min_history / N
    # the pixels whose 7 x 7 window does not hold (5, 6), whose moments differ, and which are not skipped themselves
    far = ~((np.abs(np.arange(H)[:, None] - 5) <= 3) & (np.abs(np.arange(W)[None, :] - 6) <= 3))
    far[2, 2] = far[8, 9] = False
    assert far.sum() > 20 and (far[:, :3].any() and far[7:, 7:].any())  # windows that hold the skipped taps
    assert np.all(np.abs(v[far] - want) <= 1e-5 * (M2 + M1 * M1) * min_history / N)
    assert abs(v[5, 6] - (0.75 - 0.25)) <= 1e-6
    assert v[2, 2] == 0 and v[8, 9] == 0
    assert np.all(np.isfinite(v)) and np.all(v >= 0) and v.max() < 10 * want + 1
    v64 = variance_ref(m, length, g["normal"], g["depth"], min_history=min_history, dtype=F64)
    assert v64.dtype == F64 and np.all(np.abs(v64[far] - want) <= 1e-6 * want)


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulate", "plain"])
def test_zero_variance_and_a_tiny_floor_return_the_input(demodulate):
    """v = 0 and luminance_floor = 1e-30: k = 1e30, so a tap whose luminance differs from the centre's by more than
    1e-28 weighs expf(-huge) = 0.  On a random frame every tap differs, only the centre is left, and the output is
    the working signal re-modulated: the input to the rounding of the division and multiplication by the albedo.
    The variance stays 0, the alpha and the miss pixels are the input's."""
    H, W = 19, 23
    g = flat_guides(H, W)
    g["depth"][4, 5] = np.inf
    g["albedo"][..., :3] = np.random.default_rng(5).uniform(0.1, 1.0, (H, W, 3)).astype(F32)
    color = np.random.default_rng(4).uniform(0.1, 2.0, (H, W, 4)).astype(F32)
    out, v = denoise_variance_ref(color, np.zeros((H, W), F32), g["normal"], g["depth"], g["albedo"], iterations=5,
                                  sigma_luminance=4.0, luminance_floor=1e-30, demodulate=demodulate)
    assert out.dtype == F32 and v.dtype == F32
    assert np.all(np.abs(out - color) <= 2e-7 * np.abs(color))
    assert np.all(v == 0)
    assert np.array_equal(out[4, 5], color[4, 5]) and np.array_equal(out[..., 3], color[..., 3])


def test_constant_frame_and_variance_decay():
    """A constant frame over flat guides is unchanged whatever the variance; a constant variance v then falls to
    v sum(h^2)^2 per pass in the interior, where sum(w^2) / sum(w)^2 = (sum h^2)^2 = (35/128)^2."""
    H, W = 40, 44
    g = flat_guides(H, W)
    color = np.empty((H, W, 4), F32)
    color[...] = (0.25, 0.5, 0.75, 1.0)
    out, v = denoise_variance_ref(color, np.full((H, W), 0.3, F32), g["normal"], g["depth"], g["albedo"], iterations=2,
                                  demodulate=False)
    assert np.abs(out - color).max() <= 1e-6
    ratio = (35.0 / 128.0) ** 2
    assert np.all(np.abs(v[8:-8, 8:-8] - 0.3 * ratio * ratio) <= 1e-5 * 0.3)
