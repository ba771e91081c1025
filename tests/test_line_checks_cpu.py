"""tests/helpers/line_checks.py on its own: the line rule against a pixel set known in advance, direction independence, each check against a
renderer that breaks the rule it checks, the near-tie cap on every scene of the winner check, and the new entry points.  No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import line_checks as lc
from .helpers import raster_checks as rc


def _reference(sc, **kw):
    X, Y, z, _, _ = rc.setup(sc["verts"], sc["faces"], sc["cam"], sc["M"], sc["H"], sc["W"])
    return lc.rasterise_lines(X, Y, z, sc["faces"], sc["H"], sc["W"], **kw)


@pytest.fixture(scope="module")
def references():
    """One int64 / float64 wireframe of every scene of the winner check, shared by the tests below; nothing modifies it."""
    return {name: _reference(sc) for name, sc in lc.winner_scenes().items()}


def test_square_outline_is_the_closed_form_set(references):
    """Pinned without any line code: the outline and the diagonal of a square with corners on pixel centres, every segment half-open at its
    upper end along its major axis."""
    want = np.zeros((48, 64), bool)
    want[7, 5:29] = True
    want[31, 5:29] = True
    want[8:32, 5] = True
    want[8:32, 29] = True
    k = np.arange(24)
    want[31 - k, 5 + k] = True
    assert want.sum() == 118
    win = references["square_outline"][0]
    assert np.array_equal(win >= 0, want)
    # the diagonal belongs to both faces, as edge 2 -> 0 of face 0 and edge 0 -> 2 of face 1: the lower index holds it
    inner = want.copy()
    inner[[7, 31], :] = False
    inner[:, [5, 29]] = False
    assert inner.sum() == 23 and (win[inner] == 3 * 0 + 2).all()


MIRROR_SCENES = ("fan_16", "through_image", "negative_sx_12x8", "torus_12x8", "triangle_64x48", "triangle_97x61")


def test_direction_independence(references):
    """Reversing every face's winding together with the sign of sx draws the mirror image with every edge walked the other way round: pixel i
    becomes W - 1 - i and no pixel is gained or lost.  The depth of a fragment is then 1 - t along the edge from the other end: equal up to
    float64 rounding.  (A mirror image swaps the open and the closed side of every half-open choice, so the scenes here are those in which
    no line passes exactly between two pixels at a major centre; walking an edge the other way WITHOUT mirroring is the next test.)"""
    for name in MIRROR_SCENES:
        sc = lc.winner_scenes()[name]
        H, W = sc["H"], sc["W"]
        X, Y, z, _, _ = rc.setup(sc["verts"], sc["faces"], sc["cam"], sc["M"], H, W)
        Xm, Ym, zm, _, _ = rc.setup(sc["verts"], sc["faces"], sc["cam"] * np.array([-1, 1, 1, 1], np.float32), sc["M"], H, W)
        assert np.array_equal(Xm, 256 * W - X) and np.array_equal(Ym, Y), name
        ref, d1, _ = references[name]
        win, e1, _ = lc.rasterise_lines(Xm, Ym, zm, sc["faces"][:, ::-1], H, W)
        assert (ref >= 0).any() and np.array_equal(win[:, ::-1] >= 0, ref >= 0), name
        assert np.allclose(e1[:, ::-1][ref >= 0], d1[ref >= 0], rtol=0, atol=1e-12), name


def test_an_edge_walked_either_way_is_the_same_fragments(references):
    """Everything is computed from (lo, hi): with the cull off, the faces listed the other way round give the same pixels and the same depths
    BIT FOR BIT."""
    for name in MIRROR_SCENES + ("equal_depth", "square_outline", "on_pixel_boundaries", "sub_pixel"):
        sc = lc.winner_scenes()[name]
        X, Y, z, _, _ = rc.setup(sc["verts"], sc["faces"], sc["cam"], sc["M"], sc["H"], sc["W"])
        a = lc.rasterise_lines(X, Y, z, sc["faces"], sc["H"], sc["W"], cull=False)
        b = lc.rasterise_lines(X, Y, z, sc["faces"][:, [0, 2, 1]], sc["H"], sc["W"], cull=False)
        assert np.array_equal(a[0] >= 0, b[0] >= 0) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), name
        assert (a[0] >= 0).any() and np.array_equal(a[0] // 3, b[0] // 3), name


def test_closed_upper_end_fails_the_cover_check(references):
    ref = references["square_outline"][0]
    wrong = _reference(lc.winner_scenes()["square_outline"], upper="closed")[0]
    assert (wrong >= 0).sum() > (ref >= 0).sum()
    with pytest.raises(AssertionError, match="coverage"):
        rc.check_cover(wrong, ref)
    rc.check_cover(ref.copy(), ref)


def test_missing_cull_fails_the_checks(references):
    """A lone clockwise triangle must draw nothing; and on a closed surface the back faces' edges show between the front faces' lines."""
    ref = references["back_facing"][0]
    wrong = _reference(lc.winner_scenes()["back_facing"], cull=False)[0]
    assert set(np.unique(ref) // 3) == {-1, 1} and set(np.unique(wrong) // 3) == {-1, 0, 1}
    with pytest.raises(AssertionError, match="coverage"):
        rc.check_cover(wrong, ref)
    with pytest.raises(AssertionError, match="coverage"):
        rc.check_cover(_reference(lc.winner_scenes()["torus_12x8"], cull=False)[0], references["torus_12x8"][0])


def test_higher_index_winning_fails_the_winner_check(references):
    """At equal depth the lower 3 face + k wins: on the shared diagonal of the square, at the crossings of the two equal-depth triangles and at
    every corner, where two edges of one face meet."""
    for name in ("square_outline", "equal_depth", "equal_depth_swapped", "fan_16"):
        ref, d1, d2 = references[name]
        wrong = _reference(lc.winner_scenes()[name], tie="higher")[0]
        assert np.array_equal(wrong >= 0, ref >= 0) and (wrong > ref).any() and not (wrong < ref).any(), name
        assert not (rc.near_ties(d1, d2) & (wrong != ref)).any()             # equal depths are decided by the rule, not excused
        with pytest.raises(AssertionError, match="wrong face"):
            rc.check_winner(wrong, ref, d1, d2)
        rc.check_winner(ref.copy(), ref, d1, d2)
    for name in ("equal_depth", "equal_depth_swapped"):                      # where the two outlines cross: the lower FACE, whichever carries it
        sc = lc.winner_scenes()[name]
        masks = [_reference(dict(sc, faces=sc["faces"][k:k + 1]))[0] >= 0 for k in (0, 1)]
        cross = masks[0] & masks[1]
        assert cross.sum() >= 4 and (references[name][0][cross] // 3 == 0).all()


def test_round_half_down_fails_the_cover_check(references):
    """A line that runs exactly between two pixels at a major centre belongs to the upper one: n = floor, not ceil - 1."""
    ref = references["on_pixel_boundaries"][0]
    wrong = _reference(lc.winner_scenes()["on_pixel_boundaries"], minor="half_down")[0]
    assert (ref[47 - 10, 10:40] >= 0).all() and not (ref[47 - 9] >= 0).any()         # the horizontal edge y = 10: GL row 10, not 9
    assert (ref[47 - 29:47 - 9, 10] >= 0).all() and not (ref[:, 9] >= 0).any()       # the vertical edge x = 10: column 10, not 9
    with pytest.raises(AssertionError, match="coverage"):
        rc.check_cover(wrong, ref)
    # away from exact boundaries the two agree
    rc.check_cover(_reference(lc.winner_scenes()["through_image"], minor="half_down")[0], references["through_image"][0])


def test_near_tie_cap_on_every_scene_of_the_winner_check(references):
    sizes = {name: rc.check_near_tie_cap(ref, d1, d2) for name, (ref, d1, d2) in references.items()}
    assert sizes["torus_320x240"][1] > 5000 and sizes["fan_16"][1] > 100
    small = [n for n in sizes if not n.startswith("torus_320x240")]
    assert all(sizes[n][0] == 0 for n in small), {n: sizes[n] for n in small if sizes[n][0]}
    ties, covered = rc.check_near_tie_cap(*_reference(rc.scene_1080p()))
    assert covered > 100000


def test_scenes_do_what_their_names_say(references):
    sc = lc.line_scenes()["fan_16"]
    X, Y, _, _, _ = rc.setup(sc["verts"], sc["faces"], sc["cam"], None, sc["H"], sc["W"])
    f = sc["faces"]
    dx = np.concatenate([X[f[:, (k + 1) % 3]] - X[f[:, k]] for k in range(3)])
    dy = np.concatenate([Y[f[:, (k + 1) % 3]] - Y[f[:, k]] for k in range(3)])
    octant = (dx > 0).astype(int) * 4 + (dy > 0).astype(int) * 2 + (np.abs(dx) > np.abs(dy)).astype(int)
    generic = (dx != 0) & (dy != 0) & (np.abs(dx) != np.abs(dy))
    assert set(octant[generic]) == set(range(8))
    assert ((dy == 0) & (dx > 0)).any() and ((dy == 0) & (dx < 0)).any() and ((dx == 0) & (dy > 0)).any() and ((dx == 0) & (dy < 0)).any()
    assert sum(((np.abs(dx) == np.abs(dy)) & (np.sign(dx) == a) & (np.sign(dy) == b)).any() for a in (-1, 1) for b in (-1, 1)) == 4
    through = references["through_image"][0]
    assert ((through >= 0).sum(0) >= 1).all()                                # one edge crosses all 64 columns
    assert set(np.unique(references["sub_pixel"][0]) // 3) == {-1, 0} and 0 < (references["sub_pixel"][0] >= 0).sum() <= 3
    assert references["triangle_1x1"][0].shape == (1, 1)
    for name in ("crossing_far", "crossing_near"):                           # the end beyond z = +-1 is clipped
        whole = dict(lc.winner_scenes()[name])
        whole["verts"] = whole["verts"] * np.array([1, 1, 0.1], np.float32)
        assert 0 < (references[name][0] >= 0).sum() < (_reference(whole)[0] >= 0).sum()
    assert set(np.unique(references["zero_area"][0]) // 3) == {-1, 1}
    neg, pos = references["negative_sx_12x8"][0], references["torus_12x8"][0]
    assert (neg >= 0).sum() > 200 and not (set(np.unique(neg // 3)) & set(np.unique(pos // 3))) - {-1}      # the mirror image shows the other side's faces
    for name in lc.COVER_ONLY:
        assert name in lc.all_scenes() and name not in references


def test_shading_formula_on_a_facing_triangle():
    """A triangle in the plane z_q = 0 facing +z: the formula by hand at the middle of its bottom edge."""
    sc = rc._scene(rc._from_window([(8.5, 8.5), (56.5, 8.5), (32.5, 60.5)], 64, 64), [(0, 1, 2)], 64, 64)
    X, Y, z, n, q = rc.setup(sc["verts"], sc["faces"], sc["cam"], None, 64, 64)
    win = lc.rasterise_lines(X, Y, z, sc["faces"], 64, 64)[0]
    lv = lc.shade_lines(q, n, X, Y, sc["faces"], win, (1.0, 0.5, 0.25))
    r, i = 63 - 8, 32                                                     # centre (32.5, 8.5) in GL pixels: p = (1/64, -47/64, 0), n = (0, 0, 1)
    assert win[r, i] == 0
    p = np.array([1 / 64, -47 / 64, 0.0])
    want = 0.3 + sum(L[2] / np.linalg.norm(L - p) ** 3 / np.pi for L in rc.LIGHTS)
    assert np.allclose(lv[r, i], 255 * np.minimum(1, np.array([1.0, 0.5, 0.25]) * want), rtol=1e-12)
    assert np.isnan(lv[0, 0]).all() and np.isnan(lv[63 - 20, 32]).all()   # nothing is filled


def test_entry_points_are_declared_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    for name in ("grnet_render_meshes_ex", "grnet_op_raster_lines"):
        assert name + "(" in hdr, name
        assert name in pkg._lib.EXPORTS, name
    assert "#define GRNET_RENDER_WIREFRAME 1" in hdr and pkg.GRNet.RENDER_WIREFRAME == 1
    assert len(pkg._lib.EXPORTS["grnet_render_meshes"][1]) == 12 and len(pkg._lib.EXPORTS["grnet_render_meshes_ex"][1]) == 13
    assert pkg._lib.EXPORTS["grnet_op_raster_lines"] == pkg._lib.EXPORTS["grnet_op_raster"]


def test_demo_wireframe_refusals():
    sys.path.insert(0, ROOT)
    demo = importlib.import_module("demo")
    p = demo.parser()
    assert demo.refusal(p.parse_args(["--mesh_render", "--wireframe"])) is None
    assert demo.refusal(p.parse_args(["--mesh_render", "--wireframe", "--sideview", "--save_obj"])) is None
    alone = demo.refusal(p.parse_args(["--wireframe"]))
    assert "line" in alone and "--mesh_render" in alone and "\n" not in alone
    assert demo.refusal(p.parse_args(["--mesh_render", "--wireframe", "--display"])) and "--display" in demo.refusal(p.parse_args(["--display"]))
