"""tests/helpers/raster_checks.py on its own: the fill rule against a pixel set known in advance, each check against a renderer that breaks
the rule it checks, and the near-tie cap on every scene the GPU tests draw.  No GPU, no library call beyond the export table."""
import os

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import raster_checks as rc


def _reference(sc, **kw):
    X, Y, z, _, _ = rc.setup(sc["verts"], sc["faces"], sc["cam"], sc["M"], sc["H"], sc["W"])
    return rc.rasterise(X, Y, z, sc["faces"], sc["H"], sc["W"], **kw)


@pytest.fixture(scope="module")
def references():
    """One float64 / int64 rendering of every scene, shared by the tests below; nothing modifies it."""
    return {name: _reference(sc) for name, sc in rc.scenes().items()}


@pytest.mark.parametrize("other", (False, True))
@pytest.mark.parametrize("box", ((5, 41, 7, 30), (0, 63, 0, 47), (10, 11, 20, 21), (3, 9, 40, 47)))
def test_fill_rule_on_a_split_rectangle(box, other):
    """(a) Pinned without any triangle code: a rectangle with its corners on pixel centres, split along either diagonal, covers exactly
    [c0,c1) x [r0,r1) in image space -- the left column and the top row in, the right column and the bottom row out -- and the pixels on the
    diagonal belong to exactly one half."""
    c0, c1, r0, r1 = box
    sc = rc.split_rectangle(c0, c1, r0, r1, 48, 64, other_diagonal=other)
    X, Y, z, _, _ = rc.setup(sc["verts"], sc["faces"], sc["cam"], None, 48, 64)
    assert np.array_equal(X, (np.array([c0, c1, c1, c0]) * 256 + 128)) and np.array_equal(Y, (47 - np.array([r1, r1, r0, r0])) * 256 + 128)
    want = np.zeros((48, 64), bool)
    want[r0:r1, c0:c1] = True
    halves = [rc.rasterise(X, Y, z, sc["faces"][k:k + 1], 48, 64)[0] >= 0 for k in (0, 1)]
    assert np.array_equal(halves[0] | halves[1], want)
    assert not (halves[0] & halves[1]).any()                 # each pixel once
    assert (halves[0].any() and halves[1].any()) or (c1 - c0, r1 - r0) == (1, 1)      # one pixel has one owner


def test_wrong_fill_rule_fails_the_cover_check(references):
    sc = rc.scenes()["split_rectangle"]
    wrong = _reference(sc, fill="inclusive")[0]
    with pytest.raises(AssertionError, match="coverage"):
        rc.check_cover(wrong, references["split_rectangle"][0])
    rc.check_cover(references["split_rectangle"][0].copy(), references["split_rectangle"][0])


def test_missing_cull_fails_the_checks(references):
    """A closed surface seen from outside hides its back faces behind its front faces, so a renderer that does not cull draws the same picture
    of it.  Two scenes tell: a lone clockwise triangle (coverage), and the torus under a negative sx, whose mirror image turns every face over,
    so that culling keeps the FAR side of the surface and no culling the near one (coverage alike, other winners)."""
    ref = references["back_facing"][0]
    wrong = _reference(rc.scenes()["back_facing"], cull=False)[0]
    assert set(np.unique(ref)) == {-1, 1} and set(np.unique(wrong)) == {-1, 0, 1}
    with pytest.raises(AssertionError, match="coverage"):
        rc.check_cover(wrong, ref)
    ref, d1, d2 = references["negative_sx"]
    wrong = _reference(rc.scenes()["negative_sx"], cull=False)[0]
    with pytest.raises(AssertionError, match="wrong face"):
        rc.check_winner(wrong, ref, d1, d2)
    closed = rc.scenes()["torus_97x61"]
    assert np.array_equal(_reference(closed, cull=False)[0], references["torus_97x61"][0])


def test_lequal_fails_the_winner_check(references):
    for name in ("equal_depth", "equal_depth_swapped"):
        ref, d1, d2 = references[name]
        overlap = np.isfinite(d2)
        assert overlap.sum() > 100 and (ref[overlap] == 0).all()          # the lower index wins, whichever triangle carries it
        assert not rc.near_ties(d1, d2).any()                             # equal depths are decided by the rule, not excused
        wrong = _reference(rc.scenes()[name], depth="lequal")[0]
        assert (wrong[overlap] == 1).all()
        with pytest.raises(AssertionError, match="wrong face"):
            rc.check_winner(wrong, ref, d1, d2)
        rc.check_winner(ref.copy(), ref, d1, d2)


def test_near_tie_cap_on_every_scene(references):
    """(c) Near-ties stay under 0.5 % of the covered pixels in every scene, so the excuse of the winner check cannot hide a wrong depth test."""
    sizes = {}
    for name, (ref, d1, d2) in references.items():
        sizes[name] = rc.check_near_tie_cap(ref, d1, d2)
    assert sizes["torus_320x240"][1] > 5000 and sizes["zero_area"][1] > 0
    ref, d1, d2 = _reference(rc.scene_1080p())
    ties, covered = rc.check_near_tie_cap(ref, d1, d2)
    assert covered > 100000


def test_scenes_do_what_their_names_say(references):
    sc = rc.scenes()
    assert references["triangle_1x1"][0].shape == (1, 1) and references["triangle_1x1"][0][0, 0] == 0
    assert (references["larger_than_image"][0] == 0).all()
    off = references["off_each_side"][0]
    assert set(np.unique(off)) == {-1, 0, 2, 4, 6, 8}                      # the partly visible ones; 1, 3, 5, 7 are wholly outside
    assert set(np.unique(references["zero_area"][0])) == {-1, 1}
    for name, lo in (("crossing_far", 1), ("crossing_near", -1)):
        whole = sc[name].copy()
        whole["verts"] = whole["verts"] * np.array([1, 1, 0.1], np.float32)
        part, full = (references[name][0] >= 0).sum(), (_reference(whole)[0] >= 0).sum()
        assert 0 < part < full
    assert sc["torus_97x61"]["verts"].shape == (6890, 3) and sc["torus_97x61"]["faces"].shape == (13780, 3)
    main, side = references["torus_97x61"][0], references["torus_97x61_side"][0]
    assert (main >= 0).sum() > 500 and (side >= 0).sum() > 500 and not np.array_equal(main >= 0, side >= 0)
    neg = references["negative_sx"][0]
    assert (neg >= 0).sum() > 500 and not set(np.unique(neg)) & set(np.unique(main)) - {-1}     # the mirror image shows the other side's faces


def test_shading_formula_on_a_facing_triangle():
    """A triangle in the plane z_q = 0 facing +z, lit by the three lights: the formula by hand at one pixel."""
    sc = rc._scene(rc._from_window([(8.0, 8.0), (56.0, 8.0), (32.5, 60.0)], 64, 64), [(0, 1, 2)], 64, 64)
    X, Y, z, n, q = rc.setup(sc["verts"], sc["faces"], sc["cam"], None, 64, 64)
    assert np.allclose(n, [0, 0, 1])
    win = rc.rasterise(X, Y, z, sc["faces"], 64, 64)[0]
    lv = rc.shade(q, n, X, Y, sc["faces"], win, (1.0, 0.5, 0.25))
    r, i = 31, 32                                                         # centre (32.5, 32.5) in GL pixels: p = (1/64, 1/64, 0), n = (0, 0, 1)
    p = np.array([1 / 64, 1 / 64, 0.0])
    want = 0.3 + sum(L[2] / np.linalg.norm(L - p) ** 3 / np.pi for L in np.array([[0.0, -1, 1], [0, 1, 1], [1, 1, 2]]))
    assert np.allclose(lv[r, i], 255 * np.minimum(1, np.array([1.0, 0.5, 0.25]) * want), rtol=1e-12)
    assert np.isnan(lv[0, 0]).all()


def test_entry_points_are_declared_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    for name in ("grnet_load_faces", "grnet_render_meshes", "grnet_op_raster_setup", "grnet_op_raster"):
        assert name + "(" in hdr, name
        assert name in pkg._lib.EXPORTS, name
    assert len(pkg._lib.EXPORTS["grnet_render_meshes"][1]) == 12
    f = pkg.synth.make_faces()
    assert f.shape == (13780, 3) and f.dtype == np.int32 and f.min() == 0 and f.max() == 6889
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()    # closed: every edge has two faces
    assert np.array_equal(f, pkg.synth.make_faces())


def test_prepare_rendering_results_orders_far_to_near(pkg):
    """demo_utils.py:212-247, non-concat: per frame, the persons present, sorted by the y-scale of their camera ascending; 'row' is the frame's index
    in the person's own arrays."""
    mk = lambda frames, sy: {"frame_ids": np.asarray(frames), "verts": np.arange(len(frames))[:, None, None] * np.ones((1, 4, 3)),
                             "orig_cam": np.stack([np.array([1.0, s, 0.0, 0.0]) for s in sy]), "joints3d": np.zeros((len(frames), 2, 3)),
                             "joints2d": np.zeros((len(frames), 2, 2))}
    res = {7: mk([0, 1, 2], [0.5, 0.9, 0.2]), 3: mk([1, 2, 4], [0.6, 0.3, 0.1])}
    fr = pkg.pipeline.prepare_rendering_results(res, list(range(5)))
    assert [list(fr[i]) for i in range(5)] == [[7], [3, 7], [7, 3], [], [3]]
    assert fr[2][3]["row"] == 1 and fr[2][3]["verts"][0, 0] == 1 and fr[1][7]["cam"][1] == 0.9
    with pytest.raises(TypeError):
        pkg.pipeline.prepare_rendering_results(res, 5)


def test_write_obj_round_trip(pkg, tmp_path):
    v = np.array([[0.1, 0.2, 0.3], [-1.5, 2.5, -3.5], [4.0, 0.0, -0.0]], np.float32)
    pkg.pipeline.write_obj(str(tmp_path / "m.obj"), v, [(0, 1, 2)])
    lines = open(tmp_path / "m.obj").read().split("\n")
    got = np.array([l.split()[1:] for l in lines if l.startswith("v ")], np.float64)
    assert np.allclose(got, v.astype(np.float64) * [1, -1, -1], atol=1e-7) and [l for l in lines if l.startswith("f ")] == ["f 1 2 3"]


def test_demo_refusals():
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    demo = importlib.import_module("demo")
    p = demo.parser()
    assert "line" in demo.refusal(p.parse_args(["--wireframe"])) and "--display" in demo.refusal(p.parse_args(["--display"]))
    assert demo.refusal(p.parse_args(["--mesh_render", "--sideview", "--save_obj"])) is None
    assert p.parse_args([]).save_vid is True and p.parse_args(["--save_vid"]).save_vid is False
