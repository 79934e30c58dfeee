"""The final-frame rows without a GPU: the new structs' layouts against gcc, the new entries'
NULL-context refusals, and self-checks of the numpy restatement (tests/final_ref.py) the GPU tests compare with."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from octree_pathtracing_amd import _lib
from tests.adaptive_ref import luminance, tile_error_ref, tile_grid, tile_mask
from tests.final_ref import clamp_samples, neighbours, sample_variance_ref, spread_ref

F32 = np.float32
F64 = np.float64
REL, ABS = 1e-5, 1e-6
HEADER = Path(__file__).resolve().parents[1] / "include" / "octpt.h"
STRUCTS = {"octpt_adaptive_params_ex": "AdaptiveParamsEx", "octpt_sample_variance_params": "SampleVarianceParams",
           "octpt_final_params": "FinalParams"}
GRIDS = [(64, 64), (37, 21)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_new_struct_layouts_match_gcc(tmp_path):
    probe = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for c_name in STRUCTS:
        lines.append(f'    printf("{c_name} %zu %zu\\n", sizeof({c_name}), _Alignof({c_name}));')
    lines.append('    printf("filter %zu 0\\n", offsetof(octpt_final_params, filter));')
    lines.append('    printf("weight %zu 0\\n", offsetof(octpt_adaptive_params_ex, neighbour_weight));')
    lines.append("    return 0;\n}")
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = {}
    for line in out.splitlines():
        name, size, align = line.split()
        seen[name] = int(size)
        if name in STRUCTS:
            mirror = getattr(_lib, STRUCTS[name])
            assert C.sizeof(mirror) == int(size), (name, C.sizeof(mirror), size)
            assert C.alignment(mirror) <= int(align)
    assert set(STRUCTS) <= set(seen)
    assert seen["filter"] == _lib.FinalParams.filter.offset
    assert seen["weight"] == _lib.AdaptiveParamsEx.neighbour_weight.offset
    assert C.sizeof(_lib.AdaptiveParamsEx) == 32


def test_null_context_is_invalid_arg():
    lib = _lib.load()
    inv = _lib.ERR_INVALID_ARG
    assert lib.octpt_set_sample_clamp(None, 1.0) == inv
    assert lib.octpt_tile_error_spread_device(None, 8, 8, 0.5, None, None, None) == inv
    assert lib.octpt_tile_error_spread(None, 8, 8, 0.5, None, None) == inv
    assert lib.octpt_render_adaptive_ex_device(None, None, None, None, None, None, None, None, None) == inv
    assert lib.octpt_render_adaptive_ex(None, None, None, None, None, None, None, None) == inv
    assert lib.octpt_sample_variance_device(None, None, None, None, None, None, None) == inv
    assert lib.octpt_sample_variance(None, None, None, None, None, None) == inv
    assert lib.octpt_render_final_device(None, None, None, None, None, None, None, None, None, None) == inv
    assert lib.octpt_render_final(None, None, None, None, None, None, None, None, None, None) == inv


def plane(W, H, seed):
    T = int(np.prod(tile_grid(W, H)))
    e = np.random.default_rng(seed).random(T, F32)
    e[[0, T // 2, T - 1]] = np.inf
    return e


def test_spread_ref():
    for W, H in GRIDS:
        tx, ty = tile_grid(W, H)
        e = plane(W, H, 3)
        assert np.array_equal(bits(spread_ref(e, W, H, 0.0)), bits(e)), "w = 0 is the identity, +inf included"
        grid = e.reshape(ty, tx)
        pad = np.full((ty + 2, tx + 2), -np.inf, F32)
        pad[1:-1, 1:-1] = grid
        box = np.max([pad[1 + dy:1 + dy + ty, 1 + dx:1 + dx + tx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
        assert np.array_equal(bits(spread_ref(e, W, H, 1.0)), bits(box.reshape(-1))), "w = 1 is the 3 x 3 max"
        half = spread_ref(e, W, H, 0.5)
        assert np.all(half >= e) and np.all(half <= spread_ref(e, W, H, 1.0))
        # the corners have three neighbours, the other border tiles five, the rest eight
        counts = np.array([len(neighbours(W, H, t)) for t in range(tx * ty)]).reshape(ty, tx)
        assert counts[0, 0] == counts[-1, -1] == 3 and counts[0, 1] == counts[1, 0] == 5 and counts[1, 1] == 8
    assert np.array_equal(spread_ref(np.asarray([2.0], F32), 8, 8, 1.0), [F32(2.0)]), "one tile has no neighbour"


def test_clamp_ref():
    rng = np.random.default_rng(11)
    c = (rng.random((8, 21, 37, 3), F32) * F32(4) + F32(0.01)).astype(F32)
    c[0, 0, 0] = (np.nan, 1.0, 1.0)
    clamp = F32(np.median(luminance(c, F32)[np.isfinite(luminance(c, F32))]))
    out = clamp_samples(c, clamp, F32)
    assert out.dtype == F32
    l = luminance(c, F32)
    over = l > clamp
    assert over.any() and (~over).any()
    assert np.array_equal(bits(out[~over]), bits(c[~over])), "samples at or below the clamp pass bit for bit, a NaN too"
    lo = luminance(out[over].astype(F64))
    assert np.all(np.abs(lo - F64(clamp)) <= REL * F64(clamp) + ABS), "clamped samples have luminance clamp"
    # the hue is kept: the three components share one factor
    k = out[over].astype(F64) / c[over].astype(F64)
    assert np.all(np.abs(k - k[:, :1]) <= 1e-6)
    # the f64 form agrees
    assert np.allclose(clamp_samples(c[1:], clamp, F64), out[1:], rtol=1e-6, atol=0)


def test_sample_variance_ref():
    W, H = 37, 21
    T = int(np.prod(tile_grid(W, H)))
    rng = np.random.default_rng(7)
    m = np.empty((H, W, 2), F32)
    m[..., 0] = rng.random((H, W), F32) + F32(0.1)
    m[..., 1] = m[..., 0] * m[..., 0] + rng.random((H, W), F32)
    m[3, 3, 1] = np.nan
    m[4, 4, 1] = F32(0.0)  # m2 < m1^2
    depth = np.full((H, W), 5.0, F32)
    depth[:, :5] = np.inf
    spp = np.full(T, 6, np.uint32)
    spp[1], spp[2] = 0, 1
    v = sample_variance_ref(m, spp, depth)
    assert v.dtype == F32 and np.all(v >= 0) and np.all(np.isfinite(v))
    assert np.all(v[:, :5] == 0), "misses"
    assert np.all(v[tile_mask(W, H, [1, 2])] == 0), "n < 2"
    assert v[3, 3] == 0 and v[4, 4] == 0, "a NaN moment and a negative difference give 0"
    inner = (12, 12)  # a hit pixel of tile 6, n = 6
    d = F64(m[inner][1]) - F64(m[inner][0]) ** 2
    assert abs(v[inner] - d / 5) <= 1e-6
    # demodulation: a grey albedo g divides the variance by g^2; components below the floor are raised to it
    alb = np.zeros((H, W, 4), F32)
    alb[..., :3] = F32(0.5)
    alb[10, 20, :3] = F32(1e-5)
    vd = sample_variance_ref(m, spp, depth, alb)
    assert np.allclose(vd[12, 12], v[12, 12] / 0.25, rtol=1e-6)
    assert np.allclose(vd[10, 20], v[10, 20] / 1e-6, rtol=1e-5)
    # the firefly mechanism of C33: one pixel with a huge second moment holds its tile's error up
    spp8 = np.full(T, 8, np.uint32)
    calm = np.empty((H, W, 2), F32)
    calm[..., 0] = F32(0.5)
    calm[..., 1] = F32(0.25 + 1e-4)
    hot = calm.copy()
    hot[9, 9] = (F32(0.5 + 1000 / 8), F32(0.25 + 1000.0 ** 2 / 8))
    t = (9 // 8) * tile_grid(W, H)[0] + 9 // 8
    assert tile_error_ref(hot, spp8, 1e-2)[t] > 10 * tile_error_ref(calm, spp8, 1e-2)[t]
