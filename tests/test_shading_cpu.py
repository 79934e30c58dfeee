"""Shading across the material, alpha, ior, emission and sun parameter space, on the CPU (no GPU).

tests/shading_cases.py holds the cases.  Here: every case and fuzz seed finishes in the oracle and reaches the
branches it exists for (the oracle's branch counters, oracle/cpu_ref.h REF_SHADE_COUNTERS); the closed-form
furnace holds the oracle against numbers derived without it; the `> RAY_EPSILON` thresholds are read from the
counters, from bit-identical renders and from the furnace.  tests/test_gpu_shading.py renders the same cases
on the device against the oracle, and the furnace against the closed form directly.
"""
import numpy as np
import pytest

from oracle.cpu_ref import SHADE_COUNTERS
from tests import shading_cases as C

REL_TOL_FORWARD = 1e-5  # tests/test_gpu_parity.py's bar (that module needs no GPU to import, but marks itself gpu)
MIN_COUNT = 16          # a case reaches each branch it exists for at least this often
MIN_SEEDS = 3           # every reachable counter is non-zero in at least this many fuzz seeds

# Counters no valid scene reaches, with the reason (read from oracle/cpu_ref.c, the same code as the kernel's).
UNREACHABLE = {
    "signum_diffuse":
        "diffuse_reflection leaves on the normal's side (tz >= 0), so the correction needs a diffuse scatter at a "
        "hit whose normal points along the ray.  Such hits are exit hits, which carry material 0 with colour 0 "
        "(commit_hit), alpha 0, diffuse probability 0; quads are back-face culled (quad_hit) and block faces are "
        "entry faces.",
    "signum_refract":
        "entering (cos_theta > 0) the refracted direction has n.d = -sqrt(radicand) < 0, the incoming side's sign, "
        "and radicand >= RAY_EPSILON leaves no room for rounding to flip it; with cos_theta <= 0 the Fresnel term "
        "is r0 + (1 - r0)(1 - cos_theta)^5 >= 1, so the draw always reflects and the refraction arm is not reached.",
    "is_chance_clamp":
        "the horizon branch scales chance by seg / cr^2 with seg = (max_r^2 - min_r^2) cr / pi and "
        "max_r^2 - min_r^2 = sin(2 alt) sin(2 cr) <= 2 cr, so the scaled chance is at most chance * 2 / pi < 0.9 = "
        "SUN_MAX_CHANCE for every importance_sample_chance <= 1.",
}


# ------------------------------------------------------------------------------------- termination + coverage
@pytest.mark.parametrize("name", list(C.CASES))
def test_case_finishes_and_reaches_its_branches(name):
    sc, cam, rs, expects = C.built(name)
    assert sc.octree.depth <= 6 and rs.width <= 64 and rs.height <= 48 and 1 <= rs.spp <= 8 and rs.max_depth <= 8
    acc, segs, st = C.oracle_of(name)  # raises TimeoutError past the wall limit
    assert np.all(np.isfinite(acc))
    assert expects <= set(SHADE_COUNTERS)
    low = {k: st[k] for k in expects if st[k] < MIN_COUNT}
    assert not low, f"{name}: counters below {MIN_COUNT}: {low}"


def test_fuzz_finishes_and_covers_every_counter():
    seeds = {k: 0 for k in SHADE_COUNTERS}
    strategies = set()
    for seed in C.FUZZ_SEEDS:
        acc, segs, st = C.fuzz_oracle_of(seed)  # raises TimeoutError past the wall limit
        assert np.all(np.isfinite(acc)), seed
        strategies.add(C.fuzz_built(seed)[3].split()[-1])
        for k in SHADE_COUNTERS:
            seeds[k] += st[k] > 0
    assert len(strategies) == 7, strategies
    low = {k: n for k, n in seeds.items() if n < MIN_SEEDS and k not in UNREACHABLE}
    assert not low, f"counters non-zero in fewer than {MIN_SEEDS} seeds: {low}"


def test_unreachable_counters_stay_zero():
    """A counter declared unreachable is zero over every case and seed; one that turns up is a finding."""
    for k in UNREACHABLE:
        assert k in SHADE_COUNTERS
        assert sum(C.oracle_of(n)[2][k] for n in C.CASES) == 0, k
        assert sum(C.fuzz_oracle_of(s)[2][k] for s in C.FUZZ_SEEDS) == 0, k


def test_every_counter_is_named_by_a_case():
    named = set().union(*(C.built(n)[3] for n in C.CASES))
    assert named | set(UNREACHABLE) == set(SHADE_COUNTERS) and not named & set(UNREACHABLE)


def test_fuzz_is_seeded():
    a, b = C.shading_fuzz(3003), C.shading_fuzz(3003)
    assert a[3] == b[3] and a[2] == b[2] and a[1] == b[1]
    assert [vars(m) for m in a[0].materials] == [vars(m) for m in b[0].materials] and a[0].sun == b[0].sun


# ------------------------------------------------------------------------------------ what the arms must do
def test_emitters_disabled_adds_nothing():
    on, off = C.oracle_of("emit_metal_glossy_glass_partial"), C.oracle_of("emit_disabled")
    assert off[2]["emission_added"] == 0 and on[2]["emission_added"] >= MIN_COUNT
    assert np.array_equal(on[1], off[1])  # the same paths ...
    assert np.all(on[0][..., :3] >= off[0][..., :3]) and (on[0] > off[0]).any()  # ... with light added only


def test_ior_below_outer_never_reflects_totally():
    """radicand = 1 - (ior_cur / ior_prev)^2 sin^2 > 0 whenever ior_cur < ior_prev: entering a medium of ior 0.8
    from the outer 1.000293 refracts or Fresnel-reflects and never reflects totally; entering ior 2.4 does beyond
    asin(1.000293 / 2.4) = 24.6 degrees.  (ior_prev / ior_cur, the swapped ratio, turns both around.)"""
    low, high = C.oracle_of("ior_below_outer")[2], C.oracle_of("ior_diamond")[2]
    assert low["tir"] == 0 and low["refract"] >= MIN_COUNT
    assert high["tir"] > high["refract"] >= MIN_COUNT


def test_ior_threshold():
    """outer +- 1e-8 is the outer ior in float32: transmission only.  One ulp above it: refraction only."""
    same, ulp = C.oracle_of("ior_outer_pm_1e8")[2], C.oracle_of("ior_one_ulp_above_outer")[2]
    assert same["refract"] == same["refract_straight"] == same["fresnel_reflect"] == same["tir"] == 0
    assert same["transmission"] >= MIN_COUNT and ulp["refract"] >= MIN_COUNT


def test_overlapping_media():
    """equal iors: crossing from one glass into the other is a transmission; unequal: never"""
    assert C.oracle_of("ior_overlap_equal")[2]["transmission"] >= MIN_COUNT
    assert C.oracle_of("ior_overlap_unequal")[2]["transmission"] == 0


def test_alpha_zero_with_specular_is_shaded():
    """[C4] fires at alpha + specular < RAY_EPSILON only: the four alpha-0 materials with specular 0.2 are shaded"""
    st = C.oracle_of("alpha_zero_specular")[2]
    assert st["c4_pass"] >= MIN_COUNT and st["lobe_specular"] >= MIN_COUNT and st["transmission"] >= MIN_COUNT
    assert st["lobe_diffuse"] < st["lobe_specular"]  # alpha 0 never scatters diffusely; only metal/glossy/glass mats


def test_f_sub_surface_zero_casts_no_subsurface_shadow():
    assert C.oracle_of("sun_f_sub_surface_zero")[2]["shadow_cast_sss"] == 0
    one = C.oracle_of("sun_f_sub_surface_one")[2]
    assert one["shadow_cast_sss"] >= MIN_COUNT
    assert one["shadow_cast_front"] == C.oracle_of("sun_f_sub_surface_zero")[2]["shadow_cast_front"]


def test_strategies_switch_their_arms():
    off, nl = C.oracle_of("sun_strategy_off")[2], C.oracle_of("sun_strategy_non_luminous")[2]
    for st in (off, nl):
        assert st["is_disc_sample"] + st["is_disc_reject"] + st["is_horizon_sample"] + st["is_horizon_reject"] == 0
        assert st["shadow_cast_front"] + st["shadow_cast_sss"] == 0
    assert off["sky_sun_diffuse"] >= MIN_COUNT and nl["sky_sun_diffuse"] == 0
    assert C.oracle_of("sun_no_texture")[2]["sky_sun_textured"] == 0
    # the apparent colour and the sun's own colour scale the disc, they do not move it
    a, b = C.oracle_of("sun_apparent_color"), C.oracle_of("sun_colored")
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[0], b[0])


def test_sun_direction_folds_above_half_pi():
    """altitude a > pi/2: sw = (cos(az) |cos a|, sin a, sin(az) |cos a|) and the sampling direction folds to
    pi - a, so both are the sun of altitude pi - a: the two renders are equal up to sin/cos rounding of a."""
    from dataclasses import replace
    from oracle import cpu_ref

    sc, cam, rs, _ = C.built("sun_altitude_folded")
    twin = replace(sc, sun=replace(sc.sun, altitude=float(np.float32(np.pi) - np.float32(sc.sun.altitude))))
    a = C.oracle_of("sun_altitude_folded")
    b = cpu_ref.render(twin, cam, rs.width, rs.height, rs.spp, max_depth=rs.max_depth, seed=rs.seed, forward=True)
    same = (a[1] == b[1]).mean()
    assert same > 0.98, same  # a path differs only where a 1e-7 shift of the sun flips a branch
    m = a[1] == b[1]
    assert np.median(np.abs(a[0][m] - b[0][m]) / np.maximum(np.abs(b[0][m]), 1e-3)) < 1e-5


# --------------------------------------------------------------------------------------- threshold edges
def test_thresholds_at_and_above_epsilon():
    """metalness, specular, emittance and roughness equal to RAY_EPSILON behave as 0: the render is bit-identical
    to the one with zeros, no draw is made for the lobe, the mirror arm runs.  The next float above switches
    each on: the metal and specular draws shift the stream (the image changes although neither lobe is ever
    chosen at probability 6e-8), the rough arm runs, emission is added."""
    from oracle import cpu_ref

    sc, cam, rs, _ = C.built("eps_at")
    zero = C._eps(0.0)[0]
    ref = cpu_ref.render(zero, cam, rs.width, rs.height, rs.spp, max_depth=rs.max_depth, seed=rs.seed, forward=True)
    at, above = C.oracle_of("eps_at"), C.oracle_of("eps_above")
    assert np.array_equal(at[0], ref[0]) and np.array_equal(at[1], ref[1])
    assert all(at[2][k] == ref[2][k] for k in SHADE_COUNTERS)
    assert at[2]["reflect_rough"] == 0 and at[2]["emission_added"] == 0
    assert above[2]["emission_added"] >= MIN_COUNT and above[2]["reflect_rough"] >= MIN_COUNT
    assert not np.array_equal(above[0], ref[0])
    # one threshold at a time: each alone changes the stream or the arm
    for field in ("metalness", "specular"):
        one = C._eps(0.0)[0]
        for m in C.DIFFUSE:
            setattr(one.materials[m], field, C.EPS_ABOVE)
        r = cpu_ref.render(one, cam, rs.width, rs.height, rs.spp, max_depth=rs.max_depth, seed=rs.seed, forward=True)
        assert not np.array_equal(r[0], ref[0]), field


# ----------------------------------------------------------------------------------- the closed-form furnace
@pytest.mark.parametrize("shape", ["sphere", "cuboid"])
@pytest.mark.parametrize("name", list(C.FURNACE))
def test_furnace_matches_closed_form(name, shape):
    """E[radiance] = [m c + (1-m)(s_p + (1-s_p) c)] * s + (1-m)(1-s_p) c^2 e over the pixels every sample of
    which hit once and escaped (shading_cases.furnace_check), evaluated in float64 from the byte LUT and the
    material alone.  The oracle's per-pixel error on the deterministic cases is about 7e-7 relative; the mixed
    cases land within about 1.5 of the 5 sigma allowed."""
    kw = C.FURNACE[name]
    spp = 32
    sc, cam, rs = C.furnace_scene(shape, spp=spp, **kw)
    acc, segs, st = C.run_oracle(sc, cam, rs, forward=True)
    mask_segs = None
    if C.furnace_mask_kw(kw) is not kw:
        mask_segs = C.run_oracle(*C.furnace_scene(shape, spp=spp, **C.furnace_mask_kw(kw)), forward=True)[1]
        assert st["transmission"] >= MIN_COUNT and st["c4_pass"] == st["transmission"]
    n_pix, worst = C.furnace_check(acc, segs, spp, kw, REL_TOL_FORWARD, mask_segs=mask_segs)
    print(f"furnace {name}/{shape}: {n_pix} pixels, worst deviation / allowance {worst:.3f}")
    # the arms the parameters switch, read from the counters
    on = lambda v: np.float32(v) > np.float32(C.RAY_EPSILON)  # noqa: E731
    m, sp, e, rough = kw.get("m", 0.0), kw.get("sp", 0.0), kw.get("e", 0.0), kw.get("rough", 0.0)
    assert (st["lobe_metal"] > 0) == bool(on(m))
    assert (st["lobe_specular"] > 0) == bool(on(sp) and m < 1.0)
    assert (st["emission_added"] > 0) == bool(on(e) and kw.get("emitters", True) and m < 1.0 and sp < 1.0)
    if st["lobe_metal"] + st["lobe_specular"]:
        assert (st["reflect_rough"] > 0) == bool(on(rough)) and (st["reflect_mirror"] > 0) == (not on(rough))
    # recursive (reference-order) accumulation gives the same numbers within its own bar
    if name in ("metal_03_specular_06", "emit_mixed") and shape == "sphere":
        rec = C.run_oracle(sc, cam, rs, forward=False)
        assert np.abs(rec[0] - acc).max() <= 1e-4 * max(1.0, float(np.abs(acc).max()))
