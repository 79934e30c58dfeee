"""Which texel appears where on a surface: a float64 reference of the texture chain -- hit point, face,
(u, v), the flip of v, the clamp, the (i, j) texel, the row-major address and the LUT -- written from the
reference's text, not from oracle/cpu_ref.c or the kernels:

  texture.rs:64-93            Texture::value: a height-0 image is white; u clamped, v clamped and flipped,
                              i = (u * width) as u32, j = (v * height) as u32, pixel_data(i, j) (clamped to the
                              image, row-major, rtw_image.rs:234-237, with the RGBA stride of C9), rgb through
                              LUT_TABLE_FLOAT = (byte / 255)^2.2 (:51-54), alpha = byte / 255
  sphere.rs:60-69             Sphere::get_uv of the unit outward normal: theta = acos(-y), phi = atan2(-z, x) + pi,
                              u = phi / 2pi, v = theta / pi
  octree_traversal.rs:159-190 a leaf cell's face = the axis of the largest entry t; uv = the entry point's other
                              two coordinates over the cell: X (z, y), Y (x, z), Z (x, y); u -> 1 - u where the ray
                              runs negative on X and Z, v -> 1 - v on Y; face id 2 * axis + (ray negative), the
                              pattern of :173 / :182 taken for X too (C23)
  cuboid.rs:73-90             Cuboid::intersect_texture: Texture::value at (|u|, |v|); alpha > EPSILON is a hit;
                              Face order W, E, Bottom, Top, South, North (:9-29), South = +Z (:20-29)
  quad.rs:172-200             Quad::hit: back faces culled (d . n >= -EPSILON), t > 0, alpha = w . (p x v),
                              beta = w . (u x p) in [0, 1], uv = the texture ranges at (alpha, beta)

and, where the reference is undefined, the contract rows of DESIGN.md section 3: C3 (a cuboid is the slab test,
the face is the entry axis, uv per face as the leaf cell's over the box's extents), C9 (RGBA stride), C19 (a
block model's quads in voxel-local coordinates; a transparent texel continues to the next quad) and C23 (a
block-value leaf is the box [c, c + 2^l); a face texel with alpha <= EPSILON passes the ray on).

The input is the f32 camera rays of octpt_camera_rays (a host function), widened to float64; everything after
is float64 and analytic, in world space, brute force over the scene's handful of primitives.

`sure`.  A pixel is `sure` when no f32 evaluation of the same chain could legitimately land in a neighbouring
texel, on another face or on another primitive.  It is not sure when u * W (v * H) lies within delta * W
(delta * H) of an integer, when the hit lies within delta (in u/v units) of a face or quad edge, when the ray
passes within delta of a silhouette of any primitive, or when two surfaces along the ray are closer than delta.

  flat surfaces   DELTA_FLAT = 2^-13 = 1.22e-4.  Coordinates and t stay below 128, so p = o + d * t carries
                  about 3 * 2^-24 * 128 = 2.3e-5 of rounding; extents are >= 1 (quads: voxel-local coordinates
                  below 1, so 3 * 2^-24 = 1.8e-7 over extents >= 1/8); 2^-13 is about 4 x the former.
  spheres         two terms.  (a) dm_acos and dm_atan2 are within 4 ulp of libm (tests/test_oracle_cpu.py
                  test_math_unary_accuracy, test_math_atan2_hypot).  theta lies in [0, pi], where an f32 ulp is
                  2^-22: 4 * 2^-22 = 9.5e-7 rad, / pi = 3.0e-7 in v.  phi = atan2 + pi: 9.5e-7 plus half an ulp of
                  [4, 8), 2.4e-7, = 1.19e-6 rad, / 2 pi = 1.9e-7 in u.  The larger, 3.0e-7, times 4:
                  DELTA_SPHERE_FN = 1.25e-6 in u/v units.  (b) the hit point: DELTA_FLAT world units, times the
                  conditioning of the quadratic's near root r / sqrt(r^2 - b^2) (b = the ray's impact parameter),
                  over r for the unit normal, over sin(theta) for both angles (d phi = d n / sin theta, d theta =
                  d n / sin theta), over 2 pi (u) or pi (v).  delta_u and delta_v are (a) + (b) per pixel; they
                  grow without bound towards the poles and the silhouette, which makes those pixels unsure.
                  (c) the silhouette band of a sphere: the same conditioning carries the hit point's rounding
                  (3 * 2^-24 * 32 = 5.7e-6 at the sphere case's coordinates, below 32) into the unit normal as
                  5.7e-6 * cond / r; beyond cond = SPHERE_COND_MAX = 4 (b > 0.968 r, 6 % of the disc) that passes
                  half of the 1e-5 which the shading and the normal checks allow, so those pixels are unsure.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

F32 = np.float32
DELTA_FLAT = 2.0 ** -13
DELTA_SPHERE_FN = 1.25e-6
SPHERE_COND_MAX = 4.0
RAY_EPSILON = 0.00000005  # Ray::EPSILON (ray/mod.rs:26)
W, H = 96, 72             # every case's frame
MODEL_NONE = 0xFFFFFFFF
PRIM_NONE = 0xFFFFFFFF
PRIM_CUBOID_BIT = 0x80000000
QUAD_KEY = 0x40000000
MISS, BOX, BLOCK, SPHERE, QUAD = range(5)
KIND_NAMES = ("miss", "box", "block", "sphere", "quad")
FACE_NORMALS = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
# texture.rs:51-54 in float64 by the formula of tests/test_oracle_cpu.py::test_luts: the f32 quotient and the f32 exponent
# 2.2 widened (the exponent's rounding alone is 5e-8 * ln x, four f32 spacings at x = 1 / 255)
LUT64 = np.array([math.pow(float(F32(i) / F32(255.0)), float(F32(2.2))) for i in range(256)])


def _S():
    from octree_pathtracing_amd import scene as S
    return S


# ------------------------------------------------------------------------------------- identity textures
def identity_texture(w: int, h: int, number: int, alpha=None) -> np.ndarray:
    """(h, w, 4) RGBA8 whose texel (i, j) (column i, row j) holds R = i, G = j, B = 8 * number + 7 and A = 255
    (or alpha[j, i]): one byte through the inverse LUT names the texel, the texture and the channel order."""
    assert w <= 32 and h <= 32 and number < 31
    px = np.empty((h, w, 4), np.uint8)
    px[..., 0] = np.arange(w)[None, :]
    px[..., 1] = np.arange(h)[:, None]
    px[..., 2] = 8 * number + 7
    px[..., 3] = 255 if alpha is None else alpha
    return px


def checker_alpha(w: int, h: int, sparse: bool = False) -> np.ndarray:
    """alpha bytes [h, w]: 0 on the even texels of a checkerboard (`sparse`: only where i and j are both multiples
    of 3), 1 -- 1/255 > EPSILON, opaque -- on those of them in every third column plus one, 255 elsewhere."""
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    hole = ((i % 3 == 0) & (j % 3 == 0)) if sparse else ((i + j) % 2 == 0)
    a = np.where(hole, 0, 255)
    a[hole & (i % 3 == 1 if not sparse else (i % 6 == 3))] = 1
    return a.astype(np.uint8)


# ----------------------------------------------------------------------------------------------- geometry
def block_leaves(tree):
    """[(corner xyz, size, payload)] of every leaf child of a block-value octree, decoded from the octant
    arrays alone: child i of a cell sits at bit 0 -> x, bit 1 -> y, bit 2 -> z (new_octree.rs:753-755), mask bit
    i = present, bit i + 8 = leaf (:84-100)."""
    out = []
    stack = [(int(tree.root), np.zeros(3, np.int64), 1 << tree.depth)]
    while stack:
        node, corner, size = stack.pop()
        m = int(tree.octant_mask[node])
        half = size // 2
        for i in range(8):
            if not (m >> i) & 1:
                continue
            c = corner + half * np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1])
            v = int(tree.octant_children[node, i])
            if (m >> (i + 8)) & 1:
                out.append((c, half, v))
            else:
                stack.append((v, c, half))
    return out


@dataclass
class Candidate:
    """one primitive's surface against every ray: arrays over the rays"""
    hit: np.ndarray
    t: np.ndarray
    kind: int
    face: np.ndarray       # face 0..5, quad index, or the sphere's quadrant (n.y > 0) | (n.x > 0) << 1
    prim: int
    material: np.ndarray
    normal: np.ndarray     # [n, 3]
    u: np.ndarray
    v: np.ndarray
    du: np.ndarray         # the pixel's delta in u and v units
    dv: np.ndarray
    shaky: np.ndarray      # within delta of an edge or a silhouette (hit or near miss)
    segment: bool          # a pass-through is a segment of its own (a committed quad hit), not a traversal step
    normal_f32: object = None  # the normal as f32 holds it: [n, 3] or [3], None on the sphere


def _slab(o, d, lo, hi):
    ta, tb = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(ta, tb), np.maximum(ta, tb)
    return tn, tn.max(-1), tf.min(-1)


def box_candidate(o, d, lo, hi, face_material, kind, prim):
    """slabs (aabb.rs:172-191, C3 / C23): the face is the entry axis, uv as octree_traversal.rs:163-189"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    tn, tin, tout = _slab(o, d, lo, hi)
    hit = (tin < tout) & (tin > 0)
    axis = tn.argmax(-1)
    neg = np.take_along_axis(d, axis[:, None], 1)[:, 0] < 0
    p = o + d * tin[:, None]
    a = (p - lo) / ext                                  # the hit point over the extent, per axis
    ua = np.array([2, 0, 0])[axis]                      # X: (z, y), Y: (x, z), Z: (x, y)
    va = np.array([1, 2, 1])[axis]
    u = np.take_along_axis(a, ua[:, None], 1)[:, 0]
    v = np.take_along_axis(a, va[:, None], 1)[:, 0]
    edge = np.minimum(np.minimum(u, 1 - u), np.minimum(v, 1 - v))
    u = np.where(neg & (axis != 1), 1 - u, u)           # :169-171, :187-189
    v = np.where(neg & (axis == 1), 1 - v, v)           # :178-180
    u, v = np.abs(u), np.abs(v)                         # cuboid.rs:75
    face = 2 * axis + neg                               # 2 * axis + sign bit: W/E, Bottom/Top
    face = np.where(axis == 2, np.where(neg, 4, 5), face)  # rd.z < 0 enters the +Z face: South = 4 (cuboid.rs:9-29)
    # a silhouette within delta: the box grown by delta (world units, extents >= 1) is hit where the box is not
    _, gin, gout = _slab(o, d, lo - DELTA_FLAT, hi + DELTA_FLAT)
    near_miss = ~hit & (gin < gout) & (gout > 0)
    shaky = near_miss | (hit & (edge < DELTA_FLAT))
    n = len(o)
    dl = np.full(n, DELTA_FLAT)
    return Candidate(hit, np.where(hit, tin, np.inf), kind, face, prim, np.asarray(face_material)[face],
                     FACE_NORMALS[face], u, v, dl, dl, shaky, False, FACE_NORMALS[face].astype(F32))


def sphere_candidate(o, d, c, r, material, prim):
    """the near root (sphere.rs:33-47) and get_uv of the unit normal (:60-69), with math.acos / math.atan2"""
    oc = np.asarray(c, np.float64) - o
    a = (d * d).sum(-1)
    h = (d * oc).sum(-1)
    b2 = np.maximum((oc * oc).sum(-1) - h * h / a, 0.0)  # squared impact parameter
    b = np.sqrt(b2)
    disc = h * h - a * ((oc * oc).sum(-1) - r * r)
    hit = (disc > 0) & (h > 0)
    root = (h - np.sqrt(np.maximum(disc, 0.0))) / a
    hit &= root > 0
    p = o + d * root[:, None]
    nrm = (p - np.asarray(c, np.float64)) / r
    n = len(o)
    u, v = np.zeros(n), np.zeros(n)
    for k in np.flatnonzero(hit):
        x, y, z = nrm[k]
        theta = math.acos(max(-1.0, min(1.0, -y)))
        phi = math.atan2(-z, x) + math.pi
        u[k], v[k] = phi / (2.0 * math.pi), theta / math.pi
    sin_t = np.sqrt(np.maximum(1.0 - nrm[:, 1] ** 2, 1e-300))
    cond = r / np.sqrt(np.maximum(r * r - b2, 1e-300))
    dn = DELTA_FLAT * cond / r / sin_t
    du = DELTA_SPHERE_FN + dn / (2.0 * math.pi)
    dv = DELTA_SPHERE_FN + dn / math.pi
    shaky = ((np.abs(b - r) < DELTA_FLAT) & (h > 0)) | (hit & (cond > SPHERE_COND_MAX))
    face = (nrm[:, 1] > 0).astype(np.int64) | ((nrm[:, 0] > 0).astype(np.int64) << 1)
    return Candidate(hit, np.where(hit, root, np.inf), SPHERE, face, prim, np.full(n, material), nrm, u, v, du, dv,
                     shaky, False, None)


def quad_normal_f32(q):
    """Quad::new's normal (quad.rs:98-99) as f32 evaluates it, in glam's operation order: cross = (a.y * b.z -
    b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y), dot = (x * x + y * y) + z * z, normalize = self *
    (1 / sqrt(dot)), every operation rounded to f32 and none fused.  A rotated element's top gives 0.99999994."""
    a, b = np.asarray(q["u"], F32), np.asarray(q["v"], F32)
    n = np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]], F32)
    return n * (F32(1.0) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))


def quad_candidate(o, d, voxel, q, index, kind_prim):
    """Quad::new (quad.rs:90-114) and Quad::hit (:172-200) with the quad moved to its voxel's world corner"""
    origin = np.asarray(q["origin"], np.float64) + np.asarray(voxel, np.float64)
    qu, qv = np.asarray(q["u"], np.float64), np.asarray(q["v"], np.float64)
    nn = np.cross(qu, qv)
    normal = nn / np.linalg.norm(nn)
    w = nn / nn.dot(nn)
    denom = d @ normal
    front = denom < -RAY_EPSILON                        # :176
    t = (normal.dot(origin) - o @ normal) / np.where(front, denom, 1.0)
    planar = (o + d * t[:, None]) - origin
    alpha = np.cross(planar, qv) @ w
    beta = np.cross(qu, planar) @ w
    inside = (alpha >= 0) & (alpha <= 1) & (beta >= 0) & (beta <= 1)
    hit = front & (t > 0) & inside
    edge = np.minimum(np.minimum(alpha, 1 - alpha), np.minimum(beta, 1 - beta))
    shaky = front & (t > 0) & (np.abs(edge) < DELTA_FLAT)
    tu, tv = np.asarray(q["texture_u_range"], np.float64), np.asarray(q["texture_v_range"], np.float64)
    u = tu[0] + alpha * (tu[1] - tu[0])                 # :194-197
    v = tv[0] + beta * (tv[1] - tv[0])
    n = len(o)
    dl = np.full(n, DELTA_FLAT)
    return Candidate(hit, np.where(hit, t, np.inf), QUAD, np.full(n, index), kind_prim,
                     np.full(n, int(q["material"])), np.broadcast_to(normal, (n, 3)), u, v, dl, dl, shaky, True,
                     quad_normal_f32(q))


def candidates(scene, o, d):
    """every primitive of the scene against the rays, from the scene's own arrays (block-value scenes: from
    the octree's leaves, so that an LOD leaf is the box of its cell)"""
    out = []
    if scene.blocks is not None:
        model = (np.asarray(scene.block_model) if scene.block_model is not None
                 else np.full(len(scene.blocks), MODEL_NONE, np.uint32))
        for corner, size, block in block_leaves(scene.octree):
            if model[block] != MODEL_NONE:
                assert size == 1
                first, count = (int(x) for x in np.asarray(scene.models).reshape(-1, 2)[model[block]])
                for qi in range(first, first + count):
                    out.append(quad_candidate(o, d, corner, scene.quads[qi], qi, QUAD_KEY | qi))
            else:
                out.append(box_candidate(o, d, corner, corner + size, np.asarray(scene.blocks)[block], BLOCK, block))
        return out
    for i, s in enumerate(np.asarray(scene.spheres).reshape(-1, 4)):
        out.append(sphere_candidate(o, d, s[:3], float(s[3]), int(scene.sphere_material[i]), i))
    for i, c in enumerate(np.asarray(scene.cuboids).reshape(-1, 6)):
        mdl = MODEL_NONE if scene.cuboid_model is None else int(scene.cuboid_model[i])
        if mdl == MODEL_NONE:
            out.append(box_candidate(o, d, c[:3], c[3:], scene.cuboid_material[i], BOX, PRIM_CUBOID_BIT | i))
        else:
            first, count = (int(x) for x in np.asarray(scene.models).reshape(-1, 2)[mdl])
            for qi in range(first, first + count):
                out.append(quad_candidate(o, d, c[:3], scene.quads[qi], qi, PRIM_CUBOID_BIT | i))
    return out


# ------------------------------------------------------------------------------------------ Texture::value
def texture_value(scene, material, u, v, du, dv):
    """Texture::value (texture.rs:64-93) of the materials' textures at (u, v): (texture index, i, j, rgba bytes,
    white flag, near flag); near = u * W or v * H within du * W (dv * H) of an integer."""
    n = len(u)
    tex = np.array([scene.materials[int(m)].texture_index for m in material], np.int64)
    ti, tj = np.zeros(n, np.int64), np.zeros(n, np.int64)
    rgba = np.zeros((n, 4), np.uint8)
    white, near = np.zeros(n, bool), np.zeros(n, bool)
    for t in np.unique(tex):
        sel = tex == t
        tx = scene.textures[t]
        if tx.kind == 0:                                # Texture::Color: no addressing
            rgba[sel] = np.asarray(tx.rgba, np.uint8)
            continue
        th, tw = tx.pixels.shape[:2]
        if th == 0:                                     # :71-73
            white[sel] = True
            rgba[sel] = 255
            continue
        uu = np.clip(u[sel], 0.0, 1.0) * tw             # :75, :78
        vv = (1.0 - np.clip(v[sel], 0.0, 1.0)) * th     # :76, :79
        i = np.minimum(np.trunc(uu).astype(np.int64), tw - 1)  # pixel_data's clamp (rtw_image.rs:235-236)
        j = np.minimum(np.trunc(vv).astype(np.int64), th - 1)
        ti[sel], tj[sel] = i, j
        rgba[sel] = tx.pixels[j, i]                     # row j, column i
        near[sel] = (np.abs(uu - np.rint(uu)) < du[sel] * tw) | (np.abs(vv - np.rint(vv)) < dv[sel] * th)
    return tex, ti, tj, rgba, white, near


def albedo_of(rgba, white):
    """((R/255)^2.2, (G/255)^2.2, (B/255)^2.2, A/255) in float64 (LUT64); a height-0 image is (1, 1, 1, 1)"""
    out = np.concatenate([LUT64[rgba[:, :3]], rgba[:, 3:4] / 255.0], 1)
    out[white] = 1.0
    return out


# -------------------------------------------------------------------------------------------- the reference
def reference(scene, camera, width=W, height=H):
    """Per pixel [height, width]: hit, kind, face (face / quad / sphere quadrant), prim (the guide buffers'
    encoding), material, texture, u, v, i, j, rgba (the texel's bytes), albedo, normal, t, segments (1 + the
    committed pass-through hits before it), through (the ray passed an alpha-0 texel first), sure, d (the ray),
    normal_f32 (faces: the axis normal; quads: Quad::new's normal evaluated in f32; NaN on the sphere), order (the
    hit's place among the surfaces along the ray, 0 = the nearest) and along (how many surfaces the ray meets),
    last_albedo / last_normal (the last committed pass-through hit: what the preview shades when the chain then
    misses, C16)."""
    from octree_pathtracing_amd.renderer import camera_rays

    rays = camera_rays(camera, width, height).reshape(-1, 6).astype(np.float64)
    o, d = rays[:, :3], rays[:, 3:]
    n = len(o)
    cands = candidates(scene, o, d)
    tv = [texture_value(scene, c.material, c.u, c.v, c.du, c.dv) for c in cands]
    ts = np.stack([c.t for c in cands])                 # [K, n]
    order = np.argsort(ts, axis=0, kind="stable")
    res = dict(hit=np.zeros(n, bool), kind=np.zeros(n, np.int64), face=np.zeros(n, np.int64),
               prim=np.full(n, PRIM_NONE, np.uint32), material=np.zeros(n, np.uint32), texture=np.zeros(n, np.int64),
               u=np.zeros(n), v=np.zeros(n), i=np.zeros(n, np.int64), j=np.zeros(n, np.int64),
               rgba=np.zeros((n, 4), np.uint8), albedo=np.zeros((n, 4)), normal=np.zeros((n, 3)),
               t=np.full(n, np.inf), segments=np.ones(n, np.int64), through=np.zeros(n, bool),
               last_albedo=np.zeros((n, 4)), last_normal=np.zeros((n, 3)),
               normal_f32=np.full((n, 3), np.nan, F32), order=np.zeros(n, np.int64),
               along=np.isfinite(ts).sum(0))
    unsure = np.zeros(n, bool)
    for c in cands:
        unsure |= c.shaky
    # two surfaces along the ray closer than delta: their order is not f32's to keep
    st = np.sort(ts, axis=0)
    if len(cands) > 1:
        with np.errstate(invalid="ignore"):
            gap = np.diff(st, axis=0)
        unsure |= (np.isfinite(st[1:]) & (gap < DELTA_FLAT)).any(0)
    open_ = np.ones(n, bool)
    idx = np.arange(n)
    for k in range(len(cands)):
        which = order[k]
        for ci, c in enumerate(cands):
            sel = open_ & (which == ci) & c.hit
            if not sel.any():
                continue
            tex, ti, tj, rgba, white, near = tv[ci]
            unsure |= sel & near
            opaque = sel & ((rgba[:, 3] / 255.0 > RAY_EPSILON) | white)   # cuboid.rs:77; C19 / C23
            passed = sel & ~opaque
            res["through"] |= passed
            if c.segment:  # a committed hit (C19): the preview keeps it as its last hit record (C16)
                res["segments"] += passed
                g = idx[passed]
                res["last_albedo"][g] = albedo_of(rgba[g], white[g])
                res["last_normal"][g] = c.normal[g]
            s = idx[opaque]
            res["hit"][s] = True
            res["kind"][s] = c.kind
            res["face"][s] = c.face[s]
            res["prim"][s] = c.prim
            res["material"][s] = c.material[s]
            res["texture"][s] = tex[s]
            res["u"][s], res["v"][s], res["i"][s], res["j"][s] = c.u[s], c.v[s], ti[s], tj[s]
            res["rgba"][s] = rgba[s]
            res["albedo"][s] = albedo_of(rgba[s], white[s])
            res["normal"][s] = c.normal[s]
            if c.normal_f32 is not None:
                res["normal_f32"][s] = c.normal_f32[s] if c.normal_f32.ndim == 2 else c.normal_f32
            res["order"][s] = k
            res["t"][s] = c.t[s]
            open_ &= ~opaque
    res["sure"] = ~unsure
    res["d"] = d
    shape = (height, width)
    return {k: v.reshape(shape + v.shape[1:]) for k, v in res.items()}


def sun_f64(sun):
    """Sun::new (scene/mod.rs:321-383) in float64: the direction sw and the emittance colour * 1.25^2.2"""
    az, alt = float(F32(sun.azimuth)), float(F32(sun.altitude))
    r = abs(math.cos(alt))
    sw = np.array([math.cos(az) * r, math.sin(alt), math.sin(az) * r])
    return sw, np.array([float(F32(c)) for c in sun.color[:3]]) * 1.25 ** 2.2


def flat_shaded(ref, sun):
    """the preview's colour of every pixel that is not sky (C16): albedo.rgb * (emittance * max(0.3, n . sw)), float64"""
    sw, emit = sun_f64(sun)
    ghost = ~ref["hit"] & (ref["segments"] > 1)  # a miss after committed pass-through hits keeps the last one
    normal = np.where(ghost[..., None], ref["last_normal"], ref["normal"])
    albedo = np.where(ghost[..., None], ref["last_albedo"], ref["albedo"])
    shade = np.maximum(0.3, normal @ sw)
    return albedo[..., :3] * (emit[None, None, :] * shade[..., None])


# ------------------------------------------------------------------------------------------------- cases
SIZES = {1: (1, 1), 2: (1, 7), 3: (7, 1), 4: (5, 3), 5: (3, 5), 6: (16, 16), 7: (17, 4), 8: (32, 32)}  # number -> (w, h)
ALPHA_A, ALPHA_B = 9, 10  # the alpha cases' textures: a 16 x 16 checkerboard, a 5 x 3 with sparse holes


@dataclass
class View:
    scene: object
    camera: object
    tag: str


@dataclass
class Case:
    name: str
    views: list
    targets: list                      # (kind, face / quad / quadrant) that must each cover >= 100 sure pixels
    textures: list                     # texture numbers whose texels must appear
    alpha: bool = False


def base_scene(order=None, white=False):
    """A scene whose pool holds every identity texture (and the two alpha textures), after the colour texture of
    material 0: material m (1-based) carries texture number m.  `order` permutes the pool: the images are stored
    in that order of numbers, so a texture's index and byte offset move while the materials keep their numbers.
    `white`: one more material on a height-0 image (texture.rs:71-73)."""
    S = _S()
    numbers = list(SIZES) + [ALPHA_A, ALPHA_B]
    order = list(order) if order is not None else numbers
    assert sorted(order) == sorted(numbers)
    sc = S.Scene()
    sc.textures = [S.Texture()]
    sc.materials = [S.air_material(0)] + [None] * len(numbers)
    for num in order:
        if num == ALPHA_A:
            px = identity_texture(16, 16, num, checker_alpha(16, 16))
        elif num == ALPHA_B:
            px = identity_texture(5, 3, num, checker_alpha(5, 3, sparse=True))
        else:
            px = identity_texture(*SIZES[num], num)
        sc.textures.append(S.Texture.image(px))
        sc.materials[num] = S.Material(texture_index=len(sc.textures) - 1)
    if white:
        sc.textures.append(S.Texture(kind=1, rgba=(0, 0, 0, 0), pixels=np.zeros((0, 4, 4), np.uint8)))
        sc.materials.append(S.Material(texture_index=len(sc.textures) - 1))
    return sc


PERMUTED = [7, 4, 10, 8, 1, 6, 3, 9, 5, 2]  # block_faces' pool order (box_faces and the rest: by number)


def number_of(scene, texture_index):
    """the identity number in a texture's blue byte"""
    return (int(scene.textures[texture_index].pixels[0, 0, 2]) - 7) // 8


def _look(eye, at, fov=None):
    return _S().Camera.look_at(tuple(map(float, eye)), tuple(map(float, at)), fov=fov)


def _faces_targets(kind):
    return [(kind, f) for f in range(6)]


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return CASES[name]()


def box_faces(order=None):
    """one cuboid of extents 3 x 5 x 2 off the lattice, six face textures, seen from two opposite corners"""
    sc = base_scene(order)
    lo = np.array([13.3, 11.6, 14.7])
    sc.cuboids = np.array([[*lo, *(lo + [3.0, 5.0, 2.0])]], F32)
    sc.cuboid_material = np.array([[6, 7, 3, 4, 8, 5]], np.uint32)  # W 16x16, E 17x4, Bottom 7x1, Top 5x3, S 32x32, N 3x5
    sc.build_octree(5)
    views = [View(sc, _look((18.07, 17.71, 20.49), (16.19, 15.52, 17.3), 1.07), "east-top-south"),
             View(sc, _look((11.35, 10.0, 11.94), (13.36, 12.59, 13.81), 1.18), "west-bottom-north")]
    return Case("box_faces", views, _faces_targets(BOX), [6, 7, 3, 4, 8, 5])


def block_faces():
    """a block-value world: one level-0 block and one level-2 LOD leaf (a solid 4^3 of one value through the
    compacting build), six face materials each, the pool in PERMUTED order"""
    sc = base_scene(PERMUTED)
    sc.blocks = np.array([[2, 3, 1, 4, 5, 2], [3, 6, 8, 5, 4, 2]], np.uint32)
    sc.block_model = np.full(2, MODEL_NONE, np.uint32)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3) + 12
    cells = [(x, y, z, 1) for x, y, z in g] + [(16, 11, 13, 0)]
    sc.cells = np.array(cells, np.uint32)
    sc.build_octree(5, compact=True)
    views = [View(sc, _look((21.72, 19.74, 18.34), (18.59, 16.78, 16.66), 0.72), "east-top-south"),
             View(sc, _look((11.61, 7.93, 8.72), (13.11, 10.85, 11.83), 0.72), "west-bottom-north"),
             # the level-0 block is a sixteenth of the LOD leaf's face: two more views of the same pair of corners, close up
             View(sc, _look((17.75, 12.6, 14.95), (16.45, 11.5, 13.5)), "unit-east-top-south"),
             View(sc, _look((15.2, 10.35, 12.2), (16.55, 11.5, 13.5)), "unit-west-bottom-north")]
    targets = [(BLOCK, f, b) for b in range(2) for f in range(6)]
    return Case("block_faces", views, targets, [1, 2, 3, 4, 5, 6, 8])


def sphere():
    """one sphere seen from above its seam side and from below the other, on a 17 x 4 and on a 5 x 3 texture"""
    views = []
    for num in (7, 4):
        sc = base_scene()
        sc.spheres = np.array([[15.6, 16.3, 15.9, 4.0]], F32)
        sc.sphere_material = np.array([num], np.uint32)
        sc.build_octree(5)
        size = f"{SIZES[num][0]}x{SIZES[num][1]}"
        views += [View(sc, _look((10.92, 23.75, 18.41), (13.95, 19.78, 17.55), 1.28), size + "-top-seam"),
                  View(sc, _look((21.16, 8.63, 12.7), (17.68, 12.77, 14.05), 1.16), size + "-bottom")]
        if num == 7:  # two opposite views leave the great circle between them to the silhouette band: two side views
            views += [View(sc, _look((17.2, 17.6, 25.0), (15.7, 16.2, 15.9), 1.0), size + "-south"),
                      View(sc, _look((14.1, 14.9, 6.9), (15.5, 16.4, 15.9), 1.0), size + "-north")]
    return Case("sphere", views, [(SPHERE, q) for q in range(4)], [7, 4])


def _model_scene(elements, voxel=(14, 13, 15)):
    """a scene with one block model (element_quads rows) as one unit-voxel cuboid, and its block-value twin"""
    S = _S()
    from octree_pathtracing_amd import _lib

    sc = base_scene()
    rows = [q for e in elements for q in e]
    quads = np.zeros(len(rows), _lib.QUAD_DTYPE)
    for k, (o, m, u, v, tu, tv, _) in enumerate(rows):
        quads[k] = (o, m, u, v, tu, tv, (0, 0))
    sc.quads = quads
    sc.models = np.array([[0, len(rows)]], np.uint32)
    lo = np.asarray(voxel, F32)
    sc.cuboids = np.concatenate([lo, lo + F32(1.0)])[None, :].astype(F32)
    sc.cuboid_material = np.full((1, 6), 1, np.uint32)
    sc.cuboid_model = np.array([0], np.uint32)
    sb = S.voxels_to_blocks(sc)
    sc.build_octree(5)
    sb.build_octree(5)
    return sc, sb


def quads():
    """one block model -- a slab element with full-range and sub-range faces and a rotated post on it -- as a
    block-model cuboid and as a block-value leaf"""
    S = _S()
    sub = (4.0, 2.0, 12.0, 10.0)   # tu0 = 0.25, tu1 = 0.75, tv0 = 0.125, tv1 = 0.625
    slab = S.element_quads((1, 0, 2), (15, 7, 14), {"down": 4, "up": (4, sub), "east": 5, "west": (5, sub), "south": 3,
                                                    "north": (3, sub)})
    post = S.element_quads((4, 7, 4), (12, 15, 12), {"east": 2, "west": (2, sub), "south": (7, sub), "north": (6, sub),
                                                     "up": (4, sub)}, ((8, 8, 8), "y", 22.5))
    sc, sb = _model_scene([slab, post])
    cams = [(_look((15.46, 14.15, 16.25), (12.82, 12.2, 13.71), 1.28), "east-up-south"),
            (_look((12.62, 12.13, 14.22), (15.33, 14.49, 16.47), 0.71), "west-down-north")]
    views = [View(s, cam, f"{form}-{tag}") for s, form in ((sc, "cuboid"), (sb, "block")) for cam, tag in cams]
    # quads 0-5: the slab's west, east, down, up, north, south; 6-10: the post's west, east, up, north, south
    return Case("quads", views, [(QUAD, k) for k in range(len(sc.quads))], [4, 5, 3, 2])


def alpha_faces():
    """two block-value cells in a row along the view: a checkerboard of alpha-0 texels on the one, sparse holes
    on the other; the expected texel is the first opaque one along the ray"""
    sc = base_scene()
    sc.blocks = np.array([[ALPHA_A] * 6, [ALPHA_B] * 6], np.uint32)
    sc.block_model = np.full(2, MODEL_NONE, np.uint32)
    sc.cells = np.array([(14, 13, 16, 0), (14, 13, 14, 1)], np.uint32)
    sc.build_octree(5)
    views = [View(sc, _look((14.48, 13.63, 18.33), (14.25, 13.5, 15.03), 1.21), "checker-first"),
             View(sc, _look((14.48, 12.77, 12.58), (14.95, 13.63, 16.05), 1.15), "sparse-first")]
    return Case("alpha_faces", views, [], [], alpha=True)


def alpha_quads():
    """the same for two model quads, one behind the other (each plane has a south and a north face), as a
    block-model cuboid and as a block-value leaf"""
    S = _S()
    a = S.element_quads((1, 1, 11), (15, 15, 11), {"south": ALPHA_A, "north": ALPHA_A})
    b = S.element_quads((1, 1, 4), (15, 15, 4), {"south": ALPHA_B, "north": ALPHA_B})
    sc, sb = _model_scene([a, b])
    near, far = _look((15.06, 14.15, 16.46), (13.79, 12.93, 12.87), 1.3), _look((14.23, 13.49, 14.5), (14.78, 14.59, 17.43), 1.17)
    views = [View(sc, near, "cuboid-checker-first"), View(sb, near, "block-checker-first"),
             View(sc, far, "cuboid-sparse-first"), View(sb, far, "block-sparse-first")]
    return Case("alpha_quads", views, [], [], alpha=True)


def white_image():
    """box_faces with the top face on a height-0 image, which reads as white (texture.rs:71-73).  The product's
    octpt_scene_upload refuses such a texture (INVALID_ARG), so only the oracle renders this one."""
    sc = base_scene(white=True)
    lo = np.array([13.3, 11.6, 14.7])
    sc.cuboids = np.array([[*lo, *(lo + [3.0, 5.0, 2.0])]], F32)
    sc.cuboid_material = np.array([[7, 4, 3, len(sc.materials) - 1, 8, 5]], np.uint32)
    sc.build_octree(5)
    mid = lo + [1.5, 2.5, 1.0]
    return Case("white_image", [View(sc, _look(mid + [3.1, 3.4, 4.6], mid + [0.2, 0.1, 0.0]), "east-top-south")], [], [])


CASES = {"box_faces": box_faces, "block_faces": block_faces, "sphere": sphere, "quads": quads,
         "alpha_faces": alpha_faces, "alpha_quads": alpha_quads}
VIEWS = [(name, k) for name, n in (("box_faces", 2), ("block_faces", 4), ("sphere", 6), ("quads", 4),
                                   ("alpha_faces", 2), ("alpha_quads", 4)) for k in range(n)]
VIEW_IDS = [f"{n}-{k}" for n, k in VIEWS]


@functools.lru_cache(maxsize=None)
def expected(name, k):
    """the reference of view k of a case, computed once; read-only"""
    v = case(name).views[k]
    return reference(v.scene, v.camera)


# -------------------------------------------------------------------------------- each case's own conditions
def coverage(name):
    """The non-vacuity figures of a case, from the reference alone.  Per view: the unsure share and the hit share.
    Per scene form (the views of one scene: a case's block-model cuboid and its block-value twin trace the same
    rays through different code, so each must meet the caps by itself), the smallest over the forms: the sure
    pixels per target, the share of each texture's texels that appear on sure pixels, and for the alpha cases
    the sure pixels that see a surface through an alpha-0 texel, that stop on the near one of two surfaces along
    the ray, and that stop on an alpha-1 texel.  Over all views: the ray signs per axis."""
    c = case(name)
    refs = [expected(name, k) for k in range(len(c.views))]
    out = dict(unsure=[float((~r["sure"]).mean()) for r in refs], hit=[float(r["hit"].mean()) for r in refs])
    forms = {}
    for r, v in zip(refs, c.views):
        forms.setdefault(id(v.scene), []).append(r)
    forms = list(forms.values())
    out["forms"] = len(forms)

    def count(rs, mask):
        return sum(int((r["sure"] & r["hit"] & mask(r)).sum()) for r in rs)

    def target(t):
        return lambda r: (r["kind"] == t[0]) & (r["face"] == t[1]) & ((r["prim"] == t[2]) if len(t) > 2 else True)

    out["targets"] = {t: min(count(rs, target(t)) for rs in forms) for t in c.targets}
    tex = {}
    for num in c.textures:
        w, h = SIZES[num]
        shares = []
        for rs in forms:
            seen = np.zeros((h, w), bool)
            for r in rs:
                m = r["sure"] & r["hit"] & (r["rgba"][..., 2] == 8 * num + 7)
                seen[r["j"][m], r["i"][m]] = True
            if seen.any():  # a form that carries the texture at all (the sphere's two scenes carry one each)
                shares.append(float(seen.mean()))
        tex[num] = min(shares) if shares else 0.0
    out["texels"] = tex
    d = np.concatenate([r["d"].reshape(-1, 3) for r in refs])
    out["signs"] = [(bool((d[:, a] < 0).any()), bool((d[:, a] > 0).any())) for a in range(3)]
    if c.alpha:
        out["through"] = min(count(rs, lambda r: r["through"]) for rs in forms)
        out["stopped"] = min(count(rs, lambda r: (r["along"] >= 2) & (r["order"] == 0)) for rs in forms)
        out["alpha_one"] = min(count(rs, lambda r: r["rgba"][..., 3] == 1) for rs in forms)
    return out
