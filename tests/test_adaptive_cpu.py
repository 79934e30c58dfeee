"""Adaptive sampling without a GPU (octpt_render_tiles_device, octpt_tile_error, octpt_render_adaptive; DESIGN.md
C30-C32): the new symbols are declared, exported and bound, the three structs match a gcc probe of the header, the
entries refuse a NULL context and NULL params, and the numpy restatement (tests/adaptive_ref.py) has the properties
the rows promise."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from octree_pathtracing_amd import _lib
from tests.adaptive_ref import adaptive_loop, sample_moments_ref, tile_error_ref, tile_mask, tile_pixels
from tests.test_abi_cpu import exported_symbols, header_functions

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "octpt.h"
NEW = ("octpt_render_tiles_device", "octpt_tile_error_device", "octpt_tile_error", "octpt_render_adaptive_device",
       "octpt_render_adaptive")
STRUCTS = {"octpt_tile_error_params": "TileErrorParams", "octpt_adaptive_params": "AdaptiveParams",
           "octpt_adaptive_result": "AdaptiveResult"}
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    declared = header_functions()
    exported = exported_symbols(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
        assert hasattr(lib, name)
    assert lib.octpt_abi_version() == 4  # entries are only added


def test_struct_layouts_match_gcc(tmp_path):
    probe = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for c_name in STRUCTS:
        lines.append(f'    printf("{c_name} %zu %zu\\n", sizeof({c_name}), _Alignof({c_name}));')
    lines.append('    printf("tile_samples %zu 0\\n", offsetof(octpt_adaptive_result, tile_samples));')
    lines.append("    return 0;\n}")
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        name, size, align = line.split()
        if name == "tile_samples":
            assert _lib.AdaptiveResult.tile_samples.offset == int(size)
            continue
        mirror = getattr(_lib, STRUCTS[name])
        assert C.sizeof(mirror) == int(size), (name, C.sizeof(mirror), size)
        assert C.alignment(mirror) <= int(align)
        seen += 1
    assert seen == len(STRUCTS)


def test_null_context_and_params_are_refused(lib):
    p = _lib.RenderParams(64, 64, 0, 4, 5, 1, 1, 0, 1, 0)
    a = _lib.AdaptiveParams(4, 4, 0.1, 1e-2)
    e = _lib.TileErrorParams(64, 64, 1e-2)
    # a NULL context, with and without the parameters
    for pp, aa, ee in ((None, None, None), (C.byref(p), C.byref(a), C.byref(e))):
        assert lib.octpt_render_tiles_device(None, pp, None, 0, None, None, None, None) == _lib.ERR_INVALID_ARG
        assert lib.octpt_tile_error_device(None, ee, None, None, None, None) == _lib.ERR_INVALID_ARG
        assert lib.octpt_tile_error(None, ee, None, None, None) == _lib.ERR_INVALID_ARG
        assert lib.octpt_render_adaptive_device(None, pp, aa, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
        assert lib.octpt_render_adaptive(None, pp, aa, None, None, None, None, None) == _lib.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------- the reference's properties
def _moments_of(samples):
    return sample_moments_ref(samples).astype(F32)


def test_error_is_zero_for_constant_samples():
    W, H = 24, 16
    rng = np.random.default_rng(1)
    colour = rng.random((H, W, 3)) * 0.5  # per pixel, the same in every sample: m2 = m1^2 up to the f32 rounding
    m = np.empty((H, W, 2), F32)
    l = (F32(0.2126) * colour[..., 0].astype(F32) + F32(0.7152) * colour[..., 1].astype(F32)) \
        + F32(0.0722) * colour[..., 2].astype(F32)
    m[..., 0], m[..., 1] = l, l * l
    err = tile_error_ref(m, np.full(6, 8), 1e-2)
    assert err.shape == (6,) and np.all(err == 0.0)


def test_error_is_inf_below_two_samples_and_for_nan():
    W, H = 16, 8
    m = np.zeros((H, W, 2), F32)
    m[..., 0], m[..., 1] = 0.5, 0.5
    err = tile_error_ref(m, [0, 1], 1e-2)
    assert np.all(np.isposinf(err))
    m[3, 3, 1] = np.nan
    err = tile_error_ref(m, [4, 4], 1e-2)
    assert np.isposinf(err[0]) and np.isfinite(err[1]) and err[1] > 0


def test_error_scales_with_the_sample_count():
    W, H = 16, 16
    rng = np.random.default_rng(2)
    m = np.empty((H, W, 2), F32)
    m[..., 0] = rng.random((H, W)) + 0.1
    m[..., 1] = m[..., 0] ** 2 + rng.random((H, W))
    e2, e5, e17 = (tile_error_ref(m, np.full(4, n), 1e-2) for n in (2, 5, 17))
    assert np.all(e2 > 0)
    np.testing.assert_allclose(e5, e2 / np.sqrt(4.0), rtol=1e-12)
    np.testing.assert_allclose(e17, e2 / np.sqrt(16.0), rtol=1e-12)


def test_overhanging_tiles_use_their_own_pixel_count():
    """At 37 x 21 (5 x 3 tiles) the last column holds 5 and the last row 5 pixels per side: a frame of uniform
    moments gives every tile the same error only if each divides by its own P, and what lies outside is not read."""
    W, H = 37, 21
    m = np.empty((H, W, 2), F32)
    m[..., 0], m[..., 1] = 0.25, 0.25  # v = 0.1875 everywhere
    err = tile_error_ref(m, np.full(15, 4), 1e-2)
    expect = np.sqrt(0.1875 / 3.0) / (0.25 + np.float64(F32(1e-2)))
    np.testing.assert_allclose(err, expect, rtol=1e-12)
    ys, xs = tile_pixels(W, H, 14)
    assert (ys.stop - ys.start, xs.stop - xs.start) == (5, 5)
    assert tile_mask(W, H, [14]).sum() == 25 and tile_mask(W, H, range(15)).all()
    # a tile's error follows its own pixels: doubling the corner tile's variance moves that tile alone
    m2 = m.copy()
    m2[ys, xs, 1] = 0.25 ** 2 + 2 * 0.1875
    err2 = tile_error_ref(m2, np.full(15, 4), 1e-2)
    assert np.all(err2[:14] == err[:14])
    np.testing.assert_allclose(err2[14], expect * np.sqrt(2.0), rtol=1e-6)


def test_sample_moments_are_the_weighted_means():
    rng = np.random.default_rng(3)
    s = rng.random((5, 4, 3))
    m = sample_moments_ref(s)
    l = 0.2126 * s[..., 0] + 0.7152 * s[..., 1] + 0.0722 * s[..., 2]
    np.testing.assert_allclose(m[..., 0], l.mean(0), rtol=1e-12)
    np.testing.assert_allclose(m[..., 1], (l * l).mean(0), rtol=1e-12)
    w = [1, 1, 2, 3, 5]
    mw = sample_moments_ref(s, w)
    np.testing.assert_allclose(mw[..., 0], np.average(l, 0, w), rtol=1e-12)


def test_adaptive_loop_steps():
    """The seven steps on a synthetic error: tile t converges once it holds >= 4 * (t + 1) samples; the cap is 12."""
    calls = []
    spp = np.zeros(4, int)

    def render(active, start, count):
        assert all(spp[t] == start for t in active)
        calls.append((tuple(active), start, count))
        spp[list(active)] += count

    def error(tile_spp):
        return np.where(np.asarray(tile_spp) >= 4 * (np.arange(4) + 1), 0.05, 1.0).astype(F32)

    tile_spp, err, rounds = adaptive_loop(4, render, error, 4, 3, 12, 0.1)
    assert calls == [((0, 1, 2, 3), 0, 4), ((1, 2, 3), 4, 3), ((1, 2, 3), 7, 3), ((2, 3), 10, 2)]
    assert rounds == 4 and list(tile_spp) == [4, 10, 12, 12]
    assert list(err <= 0.1) == [True, True, True, False]
