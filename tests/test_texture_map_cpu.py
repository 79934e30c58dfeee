"""The oracle's texture mapping against the float64 reference of tests/texture_map_ref.py: which texel appears
where on cuboid faces, block-value faces (a level-0 cell and an LOD leaf), a sphere and block-model quads, on
identity textures whose bytes name the texel, the texture and the channel order.  Also each case's own
non-vacuity conditions, from the reference alone."""
import numpy as np
import pytest

from tests import texture_map_ref as T
from tests.test_gpu_parity import REL_TOL_FORWARD, rel_err

SKY = np.array([0.5, 0.7, 1.0], np.float32)


def check_preview(rgb, ref, sun, tag):
    """A preview frame against the reference: every sure hit pixel is albedo * (Sun emittance * max(0.3, n . sun))
    (C16) within REL_TOL_FORWARD -- distinct bytes differ by far more, so this pins the texel -- a chain that
    misses after committed alpha-0 quad hits keeps the last of them as its hit record (C16), and every other sure
    miss pixel is exactly sky (+ sun), as tests/test_gpu_parity.py::test_c1_as_is_is_sky_only has it."""
    ghost = ~ref["hit"] & (ref["segments"] > 1)  # a miss after committed alpha-0 quads: shaded as the last of them
    hit, miss = ref["sure"] & (ref["hit"] | ghost), ref["sure"] & ~ref["hit"] & ~ghost
    want = T.flat_shaded(ref, sun)
    e = rel_err(rgb[..., :3][hit].astype(np.float64), want[hit])
    bad = np.argwhere(hit)[np.unique(np.argwhere(e > REL_TOL_FORWARD)[:, 0])]
    assert e.size and e.max() <= REL_TOL_FORWARD, (
        f"{tag}: {len(bad)} of {int(hit.sum())} sure hit pixels off, max rel err {e.max()}, first (y, x): {bad[:5].tolist()}; "
        f"expected texel (i, j) {[(int(ref['i'][y, x]), int(ref['j'][y, x])) for y, x in bad[:5]]}")
    diff = rgb[..., :3][miss] - SKY
    assert np.all((np.abs(diff).max(-1) == 0) | (diff.min(-1) > 1.0)), tag


@pytest.mark.parametrize("name,k", T.VIEWS, ids=T.VIEW_IDS)
def test_oracle_preview_matches_reference(name, k):
    from oracle import cpu_ref

    v = T.case(name).views[k]
    ref = T.expected(name, k)
    acc, _, _ = cpu_ref.render(v.scene, v.camera, T.W, T.H, 1, preview=True)
    check_preview(acc, ref, v.scene.sun, f"{name} {v.tag}")


def test_height_zero_image_is_white():
    """texture.rs:71-73: an image of height 0 reads as (1, 1, 1, 1).  Only the oracle takes such a texture: the
    product's scene upload refuses an image without pixels."""
    from oracle import cpu_ref

    c = T.white_image()
    v = c.views[0]
    ref = T.reference(v.scene, v.camera)
    top = ref["sure"] & ref["hit"] & (ref["face"] == 3)
    assert top.sum() >= 100 and np.all(ref["albedo"][top] == 1.0)
    acc, _, _ = cpu_ref.render(v.scene, v.camera, T.W, T.H, 1, preview=True)
    check_preview(acc, ref, v.scene.sun, "white_image")


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_is_not_vacuous(name):
    """From the reference alone: unsure share <= 5 % and hit share >= 25 % of every frame; both ray signs on each
    axis; and in each scene form by itself (a block-model cuboid and its block-value twin see the same rays, which
    are not counted twice): every face, quad or sphere quadrant the case exists for on >= 100 sure pixels; every
    texel of the textures up to 5 x 3 and >= 90 % of the larger ones' on a sure pixel; in the alpha cases >= 100 sure
    pixels that see a surface through an alpha-0 texel, >= 100 that stop on the near one of the two surfaces their
    ray meets, and some that stop on an alpha-1 texel."""
    c = T.case(name)
    cov = T.coverage(name)
    print(name, cov)
    assert max(cov["unsure"]) <= 0.05, cov["unsure"]
    assert min(cov["hit"]) >= 0.25, cov["hit"]
    for t, n in cov["targets"].items():
        assert n >= 100, (t, n)
    for num, share in cov["texels"].items():
        w, h = T.SIZES[num]
        assert share == 1.0 if w * h <= 15 else share >= 0.9, (num, share)
    assert all(neg and pos for neg, pos in cov["signs"]), cov["signs"]
    if c.alpha:
        assert cov["through"] >= 100 and cov["stopped"] >= 100 and cov["alpha_one"] >= 10, cov
    if name in ("alpha_quads", "quads"):
        assert len(c.views) == 4 and cov["forms"] == 2  # each camera on the block-model cuboid and on the block-value leaf
    if name == "alpha_quads":
        assert any((T.expected(name, k)["segments"] > 1).any() for k in range(4))


def test_cases_follow_the_issue():
    """the properties the cases are built to have: three or more images in every pool and the texture under test
    not the first; the pool order differs between box_faces and block_faces, so offsets are non-zero and move;
    block_faces holds a level-0 and a level-2 leaf; textures separate width from height"""
    from tests.octree_forms import leaf_levels

    for name in T.CASES:
        for k, v in enumerate(T.case(name).views):
            images = [t for t in v.scene.textures if t.kind == 1]
            assert len(images) >= 3
            ref = T.expected(name, k)
            used = np.unique(ref["texture"][ref["hit"]])
            assert used.min() > 1, (name, used)  # index 0 is material 0's colour, index 1 the pool's first image
    a = [T.number_of(T.case("box_faces").views[0].scene, i) for i in range(1, 11)]
    b = [T.number_of(T.case("block_faces").views[0].scene, i) for i in range(1, 11)]
    assert a != b and sorted(a) == sorted(b)
    assert leaf_levels(T.case("block_faces").views[0].scene.octree) == {0: 1, 2: 1}
    assert {(1, 1), (1, 7), (7, 1), (5, 3), (3, 5), (16, 16), (17, 4), (32, 32)} == set(T.SIZES.values())
    for name in ("alpha_faces", "alpha_quads"):
        px = T.case(name).views[0].scene
        for num in (T.ALPHA_A, T.ALPHA_B):
            al = px.textures[px.materials[num].texture_index].pixels[..., 3]
            assert (al == 0).any() and (al == 1).any() and (al == 255).any()


def test_reference_separates_the_mistakes():
    """The reference is only worth its name if the mistakes it is meant to catch move the expected bytes: on
    box_faces a u/v swap, a missing v flip and a wrong u flip each change the expected texel on most sure pixels."""
    ref = T.expected("box_faces", 0)
    sc = T.case("box_faces").views[0].scene
    m = ref["sure"] & ref["hit"]
    u, v, mat = ref["u"][m], ref["v"][m], ref["material"][m]
    dl = np.full(u.shape, T.DELTA_FLAT)
    base = T.texture_value(sc, mat, u, v, dl, dl)[3]
    assert np.array_equal(base, ref["rgba"][m])
    for tag, (uu, vv) in {"swap": (v, u), "no v flip": (u, 1 - v), "u flip": (1 - u, v)}.items():
        other = T.texture_value(sc, mat, uu, vv, dl, dl)[3]
        assert (other != base).any(-1).mean() > 0.5, tag
