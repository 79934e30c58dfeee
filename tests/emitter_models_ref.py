"""Emissive block models as emitters restated in numpy, and the worlds its tests share.

The emissive-model table (include/octpt.h, octpt_emitter_model_table): the emissive quads of a model are those of its
range whose material has emittance > EPSILON and whose area |u x v| -- plain f32, each cross component a * b - c * d,
the length sqrt((x^2 + y^2) + z^2) -- is finite and > 0, in table order; cum_area is the running f32 sum within the
model.  The grid with OCTPT_EMITTERS_MODELS: the grid of tests/emitter_ref.py, where a leaf at any level whose block
has an emissive model is an emitter too, its record (x, y, z, 0x80000000 | model).  The sample: a model emitter's
target is ((origin + u * u2) + v * u3) + corner on the first quad i with u1 * A_m < cum_area[i] (the last one else),
and the geometric factor carries A_m.

With them the room of tests/emitter_ref.py with a torch standing on its floor, and the float64 statement of the
one-target estimator over the torch's quads."""
import numpy as np

from tests import emitter_ref as E

EPSILON = E.EPSILON
MODEL_NONE = E.MODEL_NONE
MODEL_BIT = 0x80000000
DEPTH = E.DEPTH

# materials: 0 air, 1 stone, 2 glow (emittance 1), 3 faint (emittance below EPSILON)
# blocks: 0 unused, 1 stone, 2 glow cube, 3 torch, 4 a dull model (nothing emits), 5 a model with a zero-area glowing
# quad beside a real one, 6 a model of mixed materials, 7 a model whose only glowing quad has no area
STONE, GLOW, TORCH, DULL, ZERO_AREA, MIXED, ONLY_ZERO = 1, 2, 3, 4, 5, 6, 7
# models, in table order
M_TORCH, M_DULL, M_ZERO_AREA, M_MIXED, M_ONLY_ZERO = 0, 1, 2, 3, 4

S = 1.0 / 16.0
# the torch: a 2/16 x 10/16 x 2/16 post on the middle of its voxel's floor, four sides and the top, normals (u x v)
# outward: (origin, u, v)
TORCH_QUADS = [
    ((9 * S, 0, 7 * S), (0, 10 * S, 0), (0, 0, 2 * S)),   # +X
    ((7 * S, 0, 7 * S), (0, 0, 2 * S), (0, 10 * S, 0)),   # -X
    ((7 * S, 0, 9 * S), (2 * S, 0, 0), (0, 10 * S, 0)),   # +Z
    ((7 * S, 0, 7 * S), (0, 10 * S, 0), (2 * S, 0, 0)),   # -Z
    ((7 * S, 10 * S, 7 * S), (0, 0, 2 * S), (2 * S, 0, 0)),  # top
]
TORCH_BOX = (np.array([7 * S, 0.0, 7 * S]), np.array([9 * S, 10 * S, 9 * S]))  # the post, voxel-local


def _quad_rows():
    """(origin, u, v, material) of every quad, and (first, count) of every model."""
    rows = [(o, u, v, 2) for o, u, v in TORCH_QUADS]
    models = [(0, 5)]
    # dull: two stone quads
    models.append((len(rows), 2))
    rows += [((0, 0.5, 0), (1, 0, 0), (0, 0, 1), 1), ((0, 0.25, 0), (0, 0, 1), (1, 0, 0), 3)]
    # zero area: a glowing quad with v parallel to u, then a real glowing quad, then a glowing quad with u = 0
    models.append((len(rows), 3))
    rows += [((0, 0, 0), (1, 0, 0), (0.5, 0, 0), 2), ((0.25, 0.5, 0.125), (0.5, 0, 0.25), (0, 0.375, 0), 2),
             ((0, 0, 0), (0, 0, 0), (0, 1, 0), 2)]
    # mixed: stone, glow, faint, glow (a slanted one, whose area rounds), stone
    models.append((len(rows), 5))
    rows += [((0, 0, 0), (1, 0, 0), (0, 1, 0), 1), ((0, 0, 1), (0, 1, 0), (1, 0, 0), 2),
             ((0, 0, 0.5), (1, 0, 0), (0, 1, 0), 3), ((0.1, 0.2, 0.3), (0.7, 0.1, 0.3), (0.2, 0.6, 0.1), 2),
             ((1, 0, 0), (0, 1, 0), (0, 0, 1), 1)]
    # only zero: one glowing quad without area
    models.append((len(rows), 1))
    rows += [((0, 0, 0), (0, 1, 0), (0, 2, 0), 2)]
    return rows, models


def make_scene(cells):
    """A block-value scene of the tables above with the given (x, y, z, block) rows."""
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as Sc

    sc = Sc.Scene()
    sc.materials = [Sc.air_material(), Sc.Material(), Sc.Material(emittance=1.0), Sc.Material(emittance=1e-9)]
    sc.blocks = np.array([[1] * 6, [1] * 6, [2] * 6] + [[1] * 6] * 5, np.uint32)
    sc.block_model = np.array([MODEL_NONE] * 3 + [M_TORCH, M_DULL, M_ZERO_AREA, M_MIXED, M_ONLY_ZERO], np.uint32)
    rows, models = _quad_rows()
    sc.models = np.array(models, np.uint32)
    q = np.zeros(len(rows), _lib.QUAD_DTYPE)
    for k, (o, u, v, m) in enumerate(rows):
        q["origin"][k], q["u"][k], q["v"][k], q["material"][k] = o, u, v, m
    q["texture_u_range"] = q["texture_v_range"] = (0, 1)
    sc.quads = q
    sc.cells = np.asarray(cells, np.uint32).reshape(-1, 4)
    sc._depth = DEPTH
    return sc


def random_world(seed):
    """Cube and torch blocks (and the other kinds) scattered in the 32^3 world, with a 2^3 group of torches and one of
    glow cubes that compaction merges into leaves of side 2."""
    rng = np.random.default_rng(1000 + seed)
    cells = {}
    for gx, gy, gz, b in ((4, 8, 12, TORCH), (20, 2, 6, GLOW)):
        for c in E._cube(gx, gy, gz, 2, b):
            cells[c[:3]] = b
    for _ in range(40):
        p = tuple(int(v) for v in rng.integers(0, 32, 3))
        cells.setdefault(p, int(rng.choice([STONE, GLOW, TORCH, TORCH, DULL, ZERO_AREA, MIXED, ONLY_ZERO])))
    return [(x, y, z, b) for (x, y, z), b in cells.items()]


RANDOM_WORLDS = 10
NO_EMISSIVE_MODEL = [(8, 8, 8, GLOW), (9, 10, 11, GLOW), (20, 3, 3, STONE), (10, 8, 8, DULL), (12, 9, 9, ONLY_ZERO),
                     (6, 7, 8, DULL)]


# ------------------------------------------------------------------ the table and the grid
def f32_area(u, v):
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    x = u[1] * v[2] - u[2] * v[1]
    y = u[2] * v[0] - u[0] * v[2]
    z = u[0] * v[1] - u[1] * v[0]
    return np.sqrt((x * x + y * y) + z * z)


def model_table(scene):
    """model_first, quad_index, cum_area as the library returns them."""
    e = np.array([m.emittance for m in scene.materials], np.float32)
    first, quad, cum = [0], [], []
    for a, n in np.asarray(scene.models, np.int64).reshape(-1, 2):
        s = np.float32(0.0)
        for q in range(a, a + n):
            if not e[scene.quads["material"][q]] > np.float32(EPSILON):
                continue
            area = f32_area(scene.quads["u"][q], scene.quads["v"][q])
            assert area.dtype == np.float32
            if not (np.isfinite(area) and area > 0):
                continue
            s = np.float32(s + area)
            quad.append(q)
            cum.append(s)
        first.append(len(quad))
    return {"model_first": np.array(first, np.uint32), "quad_index": np.array(quad, np.uint32),
            "cum_area": np.array(cum, np.float32)}


def assert_same_table(got, want):
    for k in ("model_first", "quad_index", "cum_area"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k], want[k]), k


def grid(scene, depth, grid_size, compact, models=True):
    """tests/emitter_ref.py's grid with the model emitters listed."""
    cube = E.emissive_blocks(scene)
    t = model_table(scene)
    emissive_model = np.diff(t["model_first"].astype(np.int64)) > 0
    em = []
    for x, y, z, s, b in E.leaves(scene.cells, depth, compact):
        m = int(scene.block_model[b])
        if cube[b]:
            em.append((E.morton(x, y, z), (x, y, z, s)))
        elif models and m != MODEL_NONE and emissive_model[m]:
            em.append((E.morton(x, y, z), (x, y, z, MODEL_BIT | m)))
    em.sort()
    emitters = np.array([e for _, e in em], np.uint32).reshape(-1, 4)
    G = (1 << depth) // grid_size
    first, entries = [0], []
    home = emitters[:, :3].astype(np.int64) // grid_size
    for cz in range(G):
        for cy in range(G):
            for cx in range(G):
                near = np.abs(home - np.array([cx, cy, cz])).max(axis=1) <= 1 if len(home) else np.zeros(0, bool)
                entries += list(np.nonzero(near)[0])
                first.append(len(entries))
    return {"cell_first": np.array(first, np.uint32), "cell_emitters": np.array(entries, np.uint32),
            "emitters": emitters, "cells_per_axis": G}


# ------------------------------------------------------------------ one sample, float64
def sample_ref(grid, table, quads, depth, grid_size, hit, normal, rng_state):
    """tests/emitter_ref.py's emitter_sample_ref over a grid with model emitters: also the picked quad.  The quad pick
    compares u1 * A_m with cum_area in f32, as the library does (u1 has 24 bits: the product rounds, and the rounding
    is the definition's)."""
    n = np.asarray(normal, np.float32).astype(np.float64)
    p32 = (np.asarray(hit, np.float32) + np.asarray(normal, np.float32) * np.float32(1e-6)).astype(np.float64)
    G = (1 << depth) // grid_size
    cell = np.clip(np.floor(p32), 0, (1 << depth) - 1).astype(np.int64) // grid_size
    c = int(cell[0] + G * (cell[1] + G * cell[2]))
    first, K = int(grid["cell_first"][c]), int(grid["cell_first"][c + 1] - grid["cell_first"][c])
    if K == 0:
        return {"K": 0, "emitter": None, "quad": None, "p": p32}
    es = E._lowbias32(rng_state ^ E.EMIT_STREAM)
    u = []
    for _ in range(4):
        es, v = E._rng_next(es)
        u.append(v)
    k = min(int(np.float32(u[0]) * np.float32(K)), K - 1)
    e = int(grid["cell_emitters"][first + k])
    x, y, z, s = (int(v) for v in grid["emitters"][e])
    quad, area = None, 1.0
    if s & MODEL_BIT:
        m = s & ~MODEL_BIT
        lo, hi = int(table["model_first"][m]), int(table["model_first"][m + 1])
        A = np.float32(table["cum_area"][hi - 1])
        xa = np.float32(u[1]) * A
        i = lo
        while i + 1 < hi and not xa < np.float32(table["cum_area"][i]):
            i += 1
        quad = int(table["quad_index"][i])
        o, qu, qv = (np.asarray(quads[f][quad], np.float32).astype(np.float64) for f in ("origin", "u", "v"))
        t = o + qu * u[2] + qv * u[3] + np.array([x, y, z], np.float64)
        area = float(A)
    else:
        t = np.array([x + s * u[1], y + s * u[2], z + s * u[3]], np.float64)
    d = t - p32
    dist = float(np.sqrt((d * d).sum()))
    dirv = d / dist
    return {"K": K, "emitter": e, "quad": quad, "p": p32, "dir": dirv, "dist": dist, "area": area,
            "geom": abs(float(dirv @ n)) / max(dist * dist, 1.0) * area}


# ------------------------------------------------------------------ the estimator's room with a torch
# the torch's voxel: it hangs over the floor beside the view, behind z = 14, where tests/emitter_ref.py's room has its
# cube emitter.  (Not on the floor: from there a bounce off the floor meets the post at grazing angles only, about
# 6e-5 of the bounces by its solid angle, and a 16 x 16, 64 spp render without sampling would see it about once --
# no variance to compare with.  From y = 8 the post's sides face the floor at cosines near 0.5.)
ROOM_TORCH = (12, 8, 16)
ROOM_CUBE = E.ROOM_EMITTER_2


def room_scene(wall=False, cube=False, torch=True, hole=False):
    """tests/emitter_ref.py's room (its walls, its camera) over the block table of this module: a torch on the floor at
    ROOM_TORCH, with cube a glow cube at ROOM_CUBE too."""
    from octree_pathtracing_amd import scene as Sc

    shell = E.room_scene(wall=wall, emitter=False, hole=hole)
    cells = [tuple(int(v) for v in row) for row in shell.cells]
    if torch:
        cells.append((*ROOM_TORCH, TORCH))
    if cube:
        cells.append((*ROOM_CUBE, GLOW))
    sc = make_scene(cells)
    sc.textures = [Sc.Texture(), Sc.Texture(rgba=(200, 200, 200, 255)), Sc.Texture(rgba=(255, 255, 255, 255))]
    sc.materials[1].texture_index, sc.materials[2].texture_index = 1, 2
    sc.strategy = Sc.STRATEGY_IMPORTANCE
    return sc


def torch_moments(p, n, corner, points, emittance=1.0, intensity=1.0):
    """Per point of p [m, 3]: E[f] and E[f^2] (float64) of f = |dir . n| / max(dist^2, 1) * A_m * emittance * intensity
    at p + n * OFFSET over the torch at `corner`: the quad in proportion to its area, the target uniform on it, each quad
    by midpoint quadrature with points^2 points.  Visibility: the post is a convex box whose five quads face outward
    and emit alike, and whose base is open.  A shadow segment that enters the box through one of the five meets an
    emissive quad from its front and contributes the shot's value, whichever quad the target is on; one that enters
    through the open base sees every quad from behind, meets none of them, and contributes nothing (p is outside the
    box: asserted).  The face entered is the slab test's: the axis of the largest near t."""
    n = np.asarray(n, np.float64)
    p = np.asarray(p, np.float64).reshape(-1, 3) + n * 1e-6
    lo, hi = np.asarray(corner, np.float64) + TORCH_BOX[0], np.asarray(corner, np.float64) + TORCH_BOX[1]
    assert ((p < lo) | (p > hi)).any(axis=1).all()
    areas = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in TORCH_QUADS])
    A = areas.sum()
    g = (np.arange(points) + 0.5) / points
    a, b = (x.reshape(-1, 1) for x in np.meshgrid(g, g, indexing="ij"))
    mean, m2 = np.zeros(len(p)), np.zeros(len(p))
    for (o, u, v), area in zip(TORCH_QUADS, areas):
        t = np.asarray(o, np.float64) + a * np.asarray(u, np.float64) + b * np.asarray(v, np.float64) + np.asarray(corner, np.float64)
        d = t[None, :, :] - p[:, None, :]
        d2 = (d * d).sum(-1)
        f = np.abs(d @ n) / np.sqrt(d2) / np.maximum(d2, 1.0) * (A * emittance * intensity)
        with np.errstate(divide="ignore", invalid="ignore"):
            near = np.fmin((lo - p[:, None, :]) / d, (hi - p[:, None, :]) / d)
        through_base = (near.argmax(-1) == 1) & (d[..., 1] > 0.0)
        f = np.where(through_base, 0.0, f)
        mean += area / A * f.mean(1)
        m2 += area / A * (f * f).mean(1)
    return mean, m2
