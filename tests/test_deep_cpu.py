"""The oracle at octree depths 12-21 (tests/deep_worlds.py), on every machine: each deep case
compares something (the conditions the GPU tests of tests/test_gpu_deep.py rely on), the oracle's closest hit of
axis-parallel rays through cell centres at depth 21 equals an integer walk of the cells bit for bit, and the oracle
reproduces the deep golden fixtures (the deep_* cases of tests/test_golden_cpu.py)."""
import bisect

import numpy as np
import pytest

from tests import deep_worlds as DW

F32 = np.float32
NONE = DW.NONE


@pytest.mark.parametrize("name", list(DW.CASES))
def test_case_is_not_vacuous(name):
    DW.assert_not_vacuous(name)


# ---------------------------------------------------------------------------------------------- the exact axis rays
def _lines(cells):
    """per axis k: {(the two other coordinates): (sorted coordinates along k, their blocks)}; and the cell set"""
    out = []
    for k in range(3):
        a, b = [x for x in range(3) if x != k]
        d = {}
        for row in cells:
            d.setdefault((row[a], row[b]), []).append((row[k], row[3]))
        out.append({key: tuple(zip(*sorted(v))) for key, v in d.items()})
    return out


def grid_walk(lines, o, k, sgn):
    """The first cell strictly beyond the origin's own cell on the line through o along sgn * e_k, in plain ints (o =
    integer + 0.5 on every axis): (2 * t, block) or None.  A ray that starts inside a cell passes it (C23)."""
    a, b = [x for x in range(3) if x != k]
    c0 = (int(o[k] * 2) - 1) // 2  # floor of integer + 0.5
    line = lines[k].get(((int(o[a] * 2) - 1) // 2, (int(o[b] * 2) - 1) // 2))
    if line is None:
        return None
    coords, blocks = line
    if sgn > 0:
        i = bisect.bisect_right(coords, c0)
        return None if i == len(coords) else (2 * (coords[i] - c0) - 1, blocks[i])
    i = bisect.bisect_left(coords, c0) - 1
    return None if i < 0 else (2 * (c0 - coords[i] - 1) + 1, blocks[i])


def passes_beside(lines, o, k, sgn, t2, depth):
    """Does the ray, before its hit face (the cube's face on a miss), pass within 2 units of a cell off its own line?
    Those are the cells of the 24 lines 1 or 2 cells off in the perpendicular directions, anywhere along the way."""
    a, b = [x for x in range(3) if x != k]
    c = [(int(v * 2) - 1) // 2 for v in o]
    if t2 is None:
        last = (1 << depth) - 1 if sgn > 0 else 0
    else:
        last = c[k] + sgn * ((t2 - 1) // 2)  # the last cell before the hit cell
    lo, hi = min(c[k], last), max(c[k], last)
    for da in range(-2, 3):
        for db in range(-2, 3):
            line = lines[k].get((c[a] + da, c[b] + db)) if (da, db) != (0, 0) else None
            if line is not None:
                i = bisect.bisect_left(line[0], lo)
                if i < len(line[0]) and line[0][i] <= hi:
                    return True
    return False


AXIS = [("blocks21", DW.axis_rays_blocks), ("corner21-outside", DW.axis_rays_corner)]


@pytest.mark.parametrize("name,make", AXIS, ids=[a[0] for a in AXIS])
def test_axis_rays_equal_integer_grid_walk(name, make):
    """Axis-parallel rays through cell centres at depth 21.  Every coordinate, every normalised position
    (c + 0.5) * 2^-21 + 1 and every plane distance is a float32, so the oracle's block, normal and t must equal the
    integer walk's, t by its bits.  Rays that pass within 2 units of a cell beside their line are left out (the
    reference clamps a zero direction component to 2^-23, so its path is not exactly axial).

    Measured: deep_blocks(21) 1210 rays, 11 left out (0.91 %); deep_corner(21) 288 rays, 12 left out (4.17 %).
    Every other ray is exact."""
    from oracle import cpu_ref

    sc = DW.case(name)[0]
    D = sc._depth
    rays = make(D)
    assert np.all((rays[:, :3].astype(np.float64) * 2) % 2 == 1), "origins are integer + 0.5"
    assert np.all(np.abs(rays[:, 3:]).sum(1) == 1) and np.all(np.abs(rays[:, 3:]).max(1) == 1)
    cells = [tuple(int(v) for v in row) for row in np.asarray(sc.cells)]
    lines = _lines(cells)
    t, prim, nrm, steps = cpu_ref.intersect(sc, rays)
    left_out = hits = misses = inside = 0
    occupied = set(c[:3] for c in cells)
    for i, r in enumerate(rays.astype(np.float64)):
        o, d = r[:3], r[3:]
        k = int(np.flatnonzero(d)[0])
        sgn = int(d[k])
        want = grid_walk(lines, o, k, sgn)
        if passes_beside(lines, o, k, sgn, None if want is None else want[0], D):
            left_out += 1
            continue
        inside += tuple((int(v * 2) - 1) // 2 for v in o) in occupied
        tag = f"{name} ray {i} {r.tolist()}: oracle t {t[i]!r} prim {prim[i]:#x} n {nrm[i].tolist()}, walk {want}"
        n_want = np.zeros(3, F32)
        if want is None:
            misses += 1
            assert prim[i] == NONE and np.isposinf(t[i]) and np.array_equal(nrm[i], n_want), tag
            continue
        hits += 1
        n_want[k] = -sgn
        assert prim[i] == want[1], tag
        assert F32(want[0] / 2.0).view(np.uint32) == t[i].view(np.uint32), tag
        assert np.array_equal(nrm[i], n_want), tag
    print(f"{name}: {len(rays)} axis rays, {left_out} left out ({left_out / len(rays):.2%}), {hits} hits, "
          f"{misses} misses, {inside} from inside a cell; most ESVO iterations {int(steps.max())}")
    assert left_out < 0.10 * len(rays), (left_out, len(rays))
    assert hits >= 100 and misses >= 20 and inside >= 4, (hits, misses, inside)
    assert int(steps.max()) >= D  # a descent of the tree's whole height
