"""tests/helpers/segment_checks.py on its own: the wide-line rule against pixel sets written out by hand and against the wireframe's rule at
width 1, direction independence, each check against a renderer that breaks the rule it checks, and the near-tie cap on every scene of the
winner check.  No GPU."""
import numpy as np
import pytest

from .helpers import line_checks as lc
from .helpers import raster_checks as rc
from .helpers import segment_checks as sg


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


@pytest.fixture(scope="module")
def bones(pipe):
    return pipe.skeleton_bones("spin")[0]


@pytest.fixture(scope="module")
def references(pipe, bones):
    """One int64 / float64 picture of every scene, shared by the tests below; nothing modifies it."""
    view = pipe.skeleton_view()
    out = {}
    for name, sc in sg.scenes(bones).items():
        xy, d = sg.resolve(sc, view)
        out[name] = sg.rasterise_segments(xy, d, sc["segments"], sc["widths"], sc["H"], sc["W"])
    return out


def _draw(pts, seg, widths, H, W, d=None, **kw):
    sc = sg._scene(pts, seg, widths, H, W, d=d)
    return sg.rasterise_segments(sc["xy"], sc["d"], sc["segments"], sc["widths"], H, W, **kw)


def test_width_1_is_the_wireframe_rule():
    """The same edges through line_checks.rasterise_lines (cull=False): segment 3 f + k is edge k of face f."""
    for name in ("fan_16", "through_image", "square_outline", "on_pixel_boundaries", "torus_12x8", "sub_pixel"):
        sc = lc.all_scenes()[name]
        X, Y, z, _, _ = rc.setup(sc["verts"], sc["faces"], sc["cam"], sc["M"], sc["H"], sc["W"])
        assert (z >= -1).all() and (z <= 1).all()
        f = np.asarray(sc["faces"], np.int64)
        seg = np.stack([f, f[:, [1, 2, 0]]], -1).reshape(-1, 2)
        want = lc.rasterise_lines(X, Y, z, sc["faces"], sc["H"], sc["W"], cull=False)
        got = sg.rasterise_segments(np.stack([X, Y], 1), z, seg, np.ones(len(seg), np.int64), sc["H"], sc["W"])
        assert (want[0] >= 0).any(), name
        for a, b in zip(got, want):
            assert np.array_equal(a, b), name


def test_hand_written_pixel_sets():
    H, W = 12, 16
    # horizontal, width 3, ends on the centres of columns 2 and 10 at y = 5.5: columns 2 .. 9 (half-open), the column of 3 about GL row 5
    win = _draw([(2.5, 5.5), (10.5, 5.5)], [(0, 1)], 3, H, W)[0]
    want = np.zeros((H, W), bool)
    want[[H - 1 - 4, H - 1 - 5, H - 1 - 6], 2:10] = True
    assert want.sum() == 24 and np.array_equal(win >= 0, want)
    # vertical, width 2, at x = 7.75 from the centre of row 1 to that of row 9: rows 1 .. 8; the line covers [6.75, 8.75): centres 7.5, 8.5
    win = _draw([(7.75, 1.5), (7.75, 9.5)], [(0, 1)], 2, H, W)[0]
    want = np.zeros((H, W), bool)
    want[H - 1 - 8:H - 1, 7:9] = True
    assert want.sum() == 16 and np.array_equal(win >= 0, want)
    # width 16 at the lower edge: the column n0 = floor(2.3 - 7.5) = -6 .. 9 is cut to GL rows 0 .. 9
    win = _draw([(-5.0, 2.3), (30.0, 2.3)], [(0, 1)], 16, H, W)[0]
    want = np.zeros((H, W), bool)
    want[H - 10:, :] = True
    assert np.array_equal(win >= 0, want)


def test_both_directions_give_identical_fragments(references):
    for name in ("horizontal", "vertical", "diagonal", "antidiagonal", "slanted"):
        a, b = references[name + "_fwd"], references[name + "_back"]
        assert (a[0] >= 0).sum() > 90, name
        for x, y in zip(a, b):
            assert np.array_equal(x, y), name
    # |dx| == |dy| is x-major: 35 columns of 3
    assert (references["diagonal_fwd"][0] >= 0).sum() == 35 * 3 and (references["diagonal_fwd"][0] >= 0).sum(0).max() == 3


def test_scenes_do_what_they_are_for(references):
    zero = references["zero_length"][0]
    assert set(np.unique(zero)) == {-1, 2}                                 # a point draws nothing, whatever its width
    assert not (references["wholly_outside"][0] >= 0).any()
    through = references["through_image"][0]
    assert ((through == 0).sum(0) == 2).all() and ((through == 1).sum(1).max() == 3) and (through == 2).any()
    ends = references["ends_on_centres"][0]
    assert (ends == 0).sum() == 16 and (ends == 1).sum() == 2 * 22         # columns 4 .. 19; rows 8 .. 29, two wide
    edge = references["wide_at_edges"][0]
    assert (edge[-1] >= 0).all() and (edge[:, -1] >= 0).all() and (edge[0, 5:55] >= 0).all() and (edge[5:40, 0] >= 0).all()
    for name, near in (("crossing_gap", 1), ("crossing_gap_swapped", 0)):   # the nearer segment on top, whichever id it has
        win = references[name][0]
        both = (_one(name, 0) >= 0) & (_one(name, 1) >= 0)
        assert both.sum() >= 9 and (win[both] == near).all(), name
    co = references["coincident_equal_depth"][0]
    assert (co == 0).sum() > 100 and not (co == 1).any() and (co == 2).any()      # equal depth: the lower id holds every pixel of both
    assert ((_one("long_97x61", 0) >= 0).sum(0) == 2).all() and (references["long_97x61"][0] >= 0).any(0).all()   # all 97 columns: lanes step by 64
    assert references["one_pixel_1x1"][0].tolist() == [[1]]


def _one(name, s):
    sc = sg.scenes([(0, 1)])[name]
    return sg.rasterise_segments(sc["xy"], sc["d"], sc["segments"][s:s + 1], sc["widths"][s:s + 1], sc["H"], sc["W"])[0]


def test_wrong_variants_are_caught(references, bones):
    """Every wrong variant fails the check meant for it, and the right rule passes the same check."""
    def fails(check):
        with pytest.raises(AssertionError):
            check()
    sc = sg.scenes(bones)
    draw = lambda name, **kw: sg.rasterise_segments(sc[name]["xy"], sc[name]["d"], sc[name]["segments"], sc[name]["widths"], sc[name]["H"], sc[name]["W"], **kw)
    # the half pixel of an even width rounded the other way, and the symmetric column: coverage
    for variant in ("up", "symmetric"):
        fails(lambda: rc.check_cover(draw("widths_1_2_3_16", offset=variant)[0], references["widths_1_2_3_16"][0]))
        fails(lambda: rc.check_cover(draw("wide_at_edges", offset=variant)[0], references["wide_at_edges"][0]))
        assert np.array_equal(draw("horizontal_fwd", offset=variant)[0] >= 0, references["horizontal_fwd"][0] >= 0)      # an odd width is the same column
    # the closed upper end: one more column where an end is on a centre
    fails(lambda: rc.check_cover(draw("ends_on_centres", upper="closed")[0], references["ends_on_centres"][0]))
    # later-wins ties: the coincident pair
    ref = references["coincident_equal_depth"]
    rc.check_winner(draw("coincident_equal_depth")[0], *ref)
    fails(lambda: rc.check_winner(draw("coincident_equal_depth", tie="higher")[0], *ref))
    # one depth buffer per skeleton: two skeletons, the first drawn nearer where they cross
    xy, d, seg, wid = shared_buffer_scene()
    ref = sg.rasterise_segments(xy, d, seg, wid, 48, 64)
    rc.check_winner(sg.rasterise_segments(xy, d, seg, wid, 48, 64)[0], *ref)
    fails(lambda: rc.check_winner(sg.rasterise_segments(xy, d, seg, wid, 48, 64, buffers="per_skeleton")[0], *ref))
    cross = (sg.rasterise_segments(xy[0], d[0], seg, wid, 48, 64)[0] >= 0) & (sg.rasterise_segments(xy[1], d[1], seg, wid, 48, 64)[0] >= 0)
    assert cross.sum() >= 9 and (ref[0][cross] == 0).all()


def shared_buffer_scene():
    """Two one-segment skeletons that cross; the first is nearer."""
    a = sg._scene([(5.0, 5.0), (58.0, 42.0)], [(0, 1)], 5, 48, 64, d=[0.3, 0.3])
    b = sg._scene([(6.0, 41.0), (57.0, 7.0)], [(0, 1)], 5, 48, 64, d=[0.4, 0.4])
    return np.stack([a["xy"], b["xy"]]), np.stack([a["d"], b["d"]]), a["segments"], a["widths"]


def test_near_tie_cap_on_the_winner_scenes(references, bones, pipe):
    for name in sg.winner_scenes(bones):
        rc.check_near_tie_cap(*references[name])
    for name in ("spin_k0_64x48_w2", "spin_k2_64x48_w1", "spin_k0_97x61_w5", "spin_k2_97x61_w3"):
        assert (references[name][0] >= 0).sum() > 100, name
    # the cover-only scene is over the cap, which is why it is cover-only
    with pytest.raises(AssertionError):
        rc.check_near_tie_cap(*references["spin_k1_97x61_w2"])
    sc = sg.scene_1080p(bones)
    xy, d = sg.resolve(sc, pipe.skeleton_view())
    ref = sg.rasterise_segments(xy, d, sc["segments"], sc["widths"], sc["H"], sc["W"])
    ties, covered = rc.check_near_tie_cap(*ref)
    assert covered > 30000


def test_compose_and_project(pipe):
    back = np.random.Generator(np.random.Philox(key=[3, 3])).integers(0, 256, (12, 16, 3), dtype=np.uint8)
    win = _draw([(2.5, 5.5), (10.5, 5.5), (7.75, 1.5), (7.75, 9.5)], [(0, 1), (2, 3)], [3, 2], 12, 16, d=[0.5, 0.5, 0.2, 0.2])[0]
    cols = np.array([(1, 2, 3), (200, 100, 50)], np.uint8)
    out = sg.compose(back, win, cols)
    assert np.array_equal(out[win < 0], back[win < 0]) and (out[win == 0] == (1, 2, 3)).all() and (out[win == 1] == (200, 100, 50)).all()
    assert (win == 1).sum() == 16                                          # the nearer vertical holds its whole column over the horizontal
    # invalid points: not finite, behind the eye, 2^21 pixels away
    view = pipe.skeleton_view()
    P = view[0]
    eye = -P[3, :3] * (P[3, 3] + 1.0) / (P[3, :3] @ P[3, :3])              # hw = -1
    pts = np.array([(0, 0, 0), (np.nan, 0, 0), (0, np.inf, 0), eye, (0.1, 0.2, -0.3)])
    xy, d, valid = sg.project(pts, 61, 97, view)
    assert valid.tolist() == [True, False, False, False, True] and (xy[~valid] == sg.SENTINEL).all()
    narrow = (P, (-0.095, -0.095 + 0.185 * 2.0**-22, -0.095, 0.09))        # a window so narrow that the point is more than 2^20 pixels away
    assert sg.project([(0.3, 0.2, 0.1)], 61, 97, view)[2][0] and not sg.project([(0.3, 0.2, 0.1)], 61, 97, narrow)[2][0]
