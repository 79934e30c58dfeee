"""The emitter grid of DESIGN.md C38 restated in numpy, and the worlds its tests share.

The definition (include/octpt.h, octpt_build_emitter_grid): an emitter is a leaf of the block octree, at any level,
whose block fills its cell (model == MODEL_NONE) and has a face material with emittance > EPSILON; record
(x, y, z, s).  Cell (cx, cy, cz) of the grid, index cx + G * (cy + G * cz) with G = 2^depth / grid_size, lists every
emitter whose home cell (x, y, z) // grid_size is within Chebyshev distance 1, in ascending Morton code of (x, y, z).

With it the room the estimator's GPU tests render (room_scene) and the float64 statement of the one-target estimator
at a point of its floor (estimator_moments)."""
import numpy as np

EPSILON = 5e-8
MODEL_NONE = 0xFFFFFFFF
DEPTH = 5

# materials: 0 air, 1 stone, 2 glow (emittance 1), 3 faint (emittance below EPSILON)
# blocks: 0 unused (palette value 0 is air in section worlds), 1 stone, 2 glow on every face, 3 glow on the top face
# alone, 4 a block model whose quad glows (not listed), 5 faint
STONE, GLOW, TOP_GLOW, MODEL_GLOW, FAINT = 1, 2, 3, 4, 5


def make_scene(cells):
    """A block-value scene of the block table above with the given (x, y, z, block) rows."""
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S

    sc = S.Scene()
    sc.materials = [S.air_material(), S.Material(), S.Material(emittance=1.0), S.Material(emittance=1e-9)]
    sc.blocks = np.array([[1] * 6, [1] * 6, [2] * 6, [1, 1, 1, 2, 1, 1], [1] * 6, [3] * 6], np.uint32)
    sc.block_model = np.array([MODEL_NONE] * 4 + [0, MODEL_NONE], np.uint32)
    sc.models = np.array([[0, 1]], np.uint32)
    q = np.zeros(1, _lib.QUAD_DTYPE)
    q["origin"], q["u"], q["v"], q["material"] = (0, 0, 0.5), (1, 0, 0), (0, 1, 0), 2
    q["texture_u_range"] = q["texture_v_range"] = (0, 1)
    sc.quads = q
    sc.cells = np.asarray(cells, np.uint32).reshape(-1, 4)
    sc._depth = DEPTH
    return sc


def _cube(x0, y0, z0, side, block):
    return [(x0 + x, y0 + y, z0 + z, block) for z in range(side) for y in range(side) for x in range(side)]


N = (1 << DEPTH) - 1
# name -> (cells, compact); every world at depth 5
WORLDS = {
    "no_emitters": ([(3, 4, 5, STONE), (9, 9, 9, FAINT), (1, 1, 1, MODEL_GLOW)], False),
    "empty": ([], False),
    "corners": ([(x, y, z, GLOW) for x in (0, N) for y in (0, N) for z in (0, N)], False),
    "two_in_cell": ([(8, 8, 8, GLOW), (9, 10, 11, GLOW), (20, 3, 3, STONE)], False),
    "border": ([(15, 7, 7, GLOW), (16, 7, 7, GLOW), (7, 15, 16, GLOW), (3, 3, 3, STONE)], False),
    "group_plain": (_cube(12, 4, 20, 2, GLOW) + [(2, 2, 2, STONE)], False),
    "group_compact": (_cube(12, 4, 20, 2, GLOW) + [(2, 2, 2, STONE)], True),
    "big_compact": (_cube(16, 0, 8, 8, GLOW) + _cube(0, 0, 0, 4, STONE) + [(31, 31, 31, TOP_GLOW)], True),
    "one_face": ([(5, 6, 7, TOP_GLOW), (5, 7, 7, STONE)], False),
    "model_block": ([(10, 10, 10, MODEL_GLOW), (11, 10, 10, GLOW)], False),
}
GRID_SIZES = (1, 4, 32)


def morton(x, y, z):
    c = 0
    for b in range(21):
        c |= ((int(x) >> b) & 1) << (3 * b) | ((int(y) >> b) & 1) << (3 * b + 1) | ((int(z) >> b) & 1) << (3 * b + 2)
    return c


def leaves(cells, depth, compact):
    """The leaves (x, y, z, s, block) of the block octree: the cells, or with compact eight sibling leaves of one
    value merged bottom-up at every level below the root (the root is never merged away)."""
    level = {(int(x), int(y), int(z)): int(b) for x, y, z, b in np.asarray(cells, np.int64).reshape(-1, 4)}
    out = []
    if not compact:
        return [(x, y, z, 1, b) for (x, y, z), b in level.items()]
    s = 1
    while (s << 1) < (1 << depth):  # parents of side 2s, strictly below the root's side
        parents = {}
        for (x, y, z), b in level.items():
            parents.setdefault((x // (2 * s), y // (2 * s), z // (2 * s)), []).append(((x, y, z), b))
        merged = {}
        for (px, py, pz), kids in parents.items():
            if len(kids) == 8 and len({b for _, b in kids}) == 1:
                merged[(px * 2 * s, py * 2 * s, pz * 2 * s)] = kids[0][1]
            else:
                out += [(x, y, z, s, b) for (x, y, z), b in kids]
        level, s = merged, s << 1
    return out + [(x, y, z, s, b) for (x, y, z), b in level.items()]


def emissive_blocks(scene):
    e = np.array([m.emittance for m in scene.materials])
    model = (np.asarray(scene.block_model) if scene.block_model is not None
             else np.full(len(scene.blocks), MODEL_NONE, np.uint32))
    return [(model[b] == MODEL_NONE) and bool((e[np.asarray(scene.blocks[b])] > EPSILON).any())
            for b in range(len(scene.blocks))]


def grid(scene, depth, grid_size, compact):
    """The grid as the library returns it: cell_first, cell_emitters, emitters (n, 4), cells_per_axis."""
    em_block = emissive_blocks(scene)
    em = sorted((morton(x, y, z), (x, y, z, s)) for x, y, z, s, b in leaves(scene.cells, depth, compact) if em_block[b])
    emitters = np.array([e for _, e in em], np.uint32).reshape(-1, 4)
    G = (1 << depth) // grid_size
    first, entries = [0], []
    home = emitters[:, :3].astype(np.int64) // grid_size
    for cz in range(G):
        for cy in range(G):
            for cx in range(G):
                near = np.abs(home - np.array([cx, cy, cz])).max(axis=1) <= 1 if len(home) else np.zeros(0, bool)
                entries += list(np.nonzero(near)[0])  # emitters[] is in ascending Morton code
                first.append(len(entries))
    return {"cell_first": np.array(first, np.uint32), "cell_emitters": np.array(entries, np.uint32),
            "emitters": emitters, "cells_per_axis": G}


def assert_same_grid(got, want):
    assert got["cells_per_axis"] == want["cells_per_axis"]
    for k in ("emitters", "cell_first", "cell_emitters"):
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------ the estimator's room
# A closed room of opaque diffuse stone, interior (5, 19) x (5, 12) x (5, 19), its floor's top at y = 5; the camera
# hangs under the ceiling and looks straight down, so every pixel of a 16 x 16 frame meets the floor top; the emitter
# block(s) float beside the view, inside the room.  ROOM_GRID = 16: two cells per axis, every cell in every other's reach.
ROOM_GRID = 16
ROOM_EMITTER, ROOM_EMITTER_2 = (12, 8, 16), (8, 8, 16)
ROOM_EYE = (11.5, 10.5, 11.5)


def room_scene(wall=False, second=False, emitter=True, hole=False):
    """wall: a full wall at z = 14 between the floor under the camera (z < 14) and the emitter (z >= 16).
    hole: the ceiling is open over 6 <= x, z <= 17, so that the sun reaches the floor under the camera."""
    from octree_pathtracing_amd import scene as S

    cells = []
    for x in range(4, 20):
        for z in range(4, 20):
            for y in range(4, 13):
                shell = x in (4, 19) or z in (4, 19) or y in (4, 12)
                if hole and y == 12 and 6 <= x <= 17 and 6 <= z <= 17:
                    continue
                if shell or (wall and z == 14):
                    cells.append((x, y, z, STONE))
    if emitter:
        cells.append((*ROOM_EMITTER, GLOW))
    if second:
        cells.append((*ROOM_EMITTER_2, GLOW))
    sc = make_scene(cells)
    sc.textures = [S.Texture(), S.Texture(rgba=(200, 200, 200, 255)), S.Texture(rgba=(255, 255, 255, 255))]
    sc.materials[1].texture_index, sc.materials[2].texture_index = 1, 2
    sc.strategy = S.STRATEGY_IMPORTANCE
    return sc


def room_camera():
    from octree_pathtracing_amd import scene as S

    return S.Camera.look_at(ROOM_EYE, (ROOM_EYE[0], 5.0, ROOM_EYE[2]), up=(0.0, 0.0, 1.0))


def estimator_moments(p, n, cubes, points, emittance=1.0, intensity=1.0):
    """Per point of p [m, 3]: mean and second moment (float64) of the one-target estimator |dir . n| / max(dist^2, 1) *
    emittance * intensity * K at p + n * OFFSET over K = len(cubes) emitters (x, y, z, s), each cube integrated by
    midpoint quadrature with points^3 points.  The pick is uniform and the estimator carries K, so the mean is the sum
    of the cubes' means and the second moment K times the sum of theirs."""
    n = np.asarray(n, np.float64)
    p = np.asarray(p, np.float64).reshape(-1, 3) + n * 1e-6
    K = len(cubes)
    g = (np.arange(points) + 0.5) / points
    mean, m2 = np.zeros(len(p)), np.zeros(len(p))
    for x, y, z, s in cubes:
        t = np.stack(np.meshgrid(x + s * g, y + s * g, z + s * g, indexing="ij"), -1).reshape(-1, 3)
        for a in range(0, len(p), 16):
            d = t[None, :, :] - p[a:a + 16, None, :]
            d2 = (d * d).sum(-1)
            f = np.abs(d @ n) / np.sqrt(d2) / np.maximum(d2, 1.0) * (emittance * intensity)
            mean[a:a + 16] += f.mean(1)
            m2[a:a + 16] += K * (f * f).mean(1)
    return mean, m2


# ------------------------------------------------------------------ one sample, float64 (csrc/octpt_emitter.h restated)
EMIT_STREAM = 0x454D4954
_M = 0xFFFFFFFF


def _lowbias32(x):
    x &= _M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M
    x ^= x >> 16
    return x


def _rng_next(st):
    """PCG-RXS-M-XS: (new state, the float's exact value (w >> 8) * 2^-24)."""
    s = (st * 747796405 + 2891336453) & _M
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & _M
    w = (w >> 22) ^ w
    return s, (w >> 8) / 16777216.0


def emitter_sample_ref(grid, depth, grid_size, hit, normal, rng_state):
    """The sample of one hit in float64 from the f32 inputs: p, the cell's K, the picked index (exact: the draws are
    exact binary fractions and K < 2^24, so u0 * K has no rounding to decide), dir, dist, geom."""
    hit, n = np.asarray(hit, np.float32).astype(np.float64), np.asarray(normal, np.float32).astype(np.float64)
    p32 = (np.asarray(hit, np.float32) + np.asarray(normal, np.float32) * np.float32(1e-6)).astype(np.float64)  # f32's p
    G = (1 << depth) // grid_size
    cell = np.clip(np.floor(p32), 0, (1 << depth) - 1).astype(np.int64) // grid_size
    c = int(cell[0] + G * (cell[1] + G * cell[2]))
    first, K = int(grid["cell_first"][c]), int(grid["cell_first"][c + 1] - grid["cell_first"][c])
    if K == 0:
        return {"K": 0, "emitter": None, "p": p32}
    es = _lowbias32(rng_state ^ EMIT_STREAM)
    u = []
    for _ in range(4):
        es, v = _rng_next(es)
        u.append(v)
    k = min(int(np.float32(u[0]) * np.float32(K)), K - 1)
    e = int(grid["cell_emitters"][first + k])
    x, y, z, s = (float(v) for v in grid["emitters"][e])
    t = np.array([x + s * u[1], y + s * u[2], z + s * u[3]])
    d = t - p32
    dist = float(np.sqrt((d * d).sum()))
    dirv = d / dist
    return {"K": K, "emitter": e, "p": p32, "dir": dirv, "dist": dist,
            "geom": abs(float(dirv @ n)) / max(dist * dist, 1.0)}
