"""The 3D skeleton view on the device (csrc/skeleton_kernels.hip; grnet_render_segments, grnet_op_segments_setup, grnet_op_raster_segments,
grnet_spin_joints; the rules: DESIGN.md 4.6) against tests/helpers/segment_checks.py: the setup against float64, coverage bit for bit and the
winning segment against the integer reference fed the device's own snapped points, the composite byte for byte, one depth buffer per image,
one call against one call per image, spin_joints against smooth_pose's joints, refusals, and demo.py --skeleton_view."""
import ctypes as C
import importlib
import os
import sys

import joblib
import numpy as np
import pytest
import torch

from .conftest import ROOT
from .helpers import raster_checks as rc
from .helpers import segment_checks as sg

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (7, 5), (64, 48), (97, 61), (1920, 1080))         # (W, H)
XY_BAR, DEPTH_BAR = 1, 2e-6


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=2, with_gru=False)
    yield m
    m.close()


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


@pytest.fixture(scope="module")
def view(pipe):
    return pipe.skeleton_view()


@pytest.fixture(scope="module")
def bones(pipe):
    return pipe.skeleton_bones("spin")


def unproject(xw, yw, d, H, W, view):
    """The point that the view puts at window position (xw, yw) pixels (GL rows) with depth d."""
    P, (x0, x1, y0, y1) = view
    S = min(H, W)
    xs, ys = x0 + (xw - (W - S) / 2) / S * (x1 - x0), y0 + (yw - (H - S) / 2) / S * (y1 - y0)
    hw = d + P[3, 3]
    p = np.linalg.solve(P, np.array([hw * xs, hw * ys, P[2, 3], hw]))           # the third row of P is the constant P[2,3]
    assert abs(p[3] - 1.0) < 1e-9
    return p[:3]


def _draw(model, sc, view):
    """The line stage alone on one scene, and the reference it is held against: the integer rule on the DEVICE's snapped points and depths."""
    if "points" in sc:
        xy, d = model.op_segments_setup(sc["points"], sc["H"], sc["W"], view=view)
    else:
        xy, d = sc["xy"], sc["d"]
    winner = model.op_raster_segments(xy, d, sc["segments"], sc["widths"], sc["H"], sc["W"]).cpu().numpy()
    xy = xy.cpu().numpy() if torch.is_tensor(xy) else np.asarray(xy)
    d = d.cpu().numpy() if torch.is_tensor(d) else np.asarray(d, np.float32)
    ref, d1, d2 = sg.rasterise_segments(xy, d, sc["segments"], sc["widths"], sc["H"], sc["W"])
    return dict(xy=xy, d=d, winner=winner, ref=ref, d1=d1, d2=d2)


@pytest.fixture(scope="module")
def scenes(bones):
    return sg.scenes(bones[0])


@pytest.fixture(scope="module")
def drawn(model, scenes, view):
    """Every scene drawn once by the stage hooks, shared by the tests below; nothing modifies it."""
    return {name: _draw(model, sc, view) for name, sc in scenes.items()}


# ------------------------------------------------------------------ 1. setup
@pytest.mark.parametrize("W,H", SIZES)
def test_setup_against_float64(model, view, W, H):
    g = np.random.Generator(np.random.Philox(key=[W, H]))
    pts = np.concatenate([sg.spin_points((0, 7)), (g.uniform(-1, 1, (200, 3)) * (0.6, 1.0, 1.0)).astype(np.float32)])
    xy, d = model.op_segments_setup(pts, H, W, view=view)
    xy, d = xy.cpu().numpy(), d.cpu().numpy()
    want_xy, want_d, valid = sg.project(pts, H, W, view)
    assert valid.all() and (xy != sg.SENTINEL).all()
    dxy, dd = np.abs(xy - want_xy).max(), np.abs(d - want_d).max()
    print(f"{W}x{H}: xy off by {dxy} snapped units, depth by {dd:.2e}")
    assert dxy <= XY_BAR and dd <= DEPTH_BAR
    # R: the same as points turned on the host
    a = 0.7
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    R32 = R.astype(np.float32)
    xyr, dr = model.op_segments_setup(pts, H, W, R=R32, view=view)
    want_xy, want_d, valid = sg.project(pts, H, W, view, R=R32)
    assert valid.all()
    assert np.abs(xyr.cpu().numpy() - want_xy).max() <= XY_BAR and np.abs(dr.cpu().numpy() - want_d).max() <= DEPTH_BAR
    turned = (pts.astype(np.float64) @ R32.astype(np.float64).T).astype(np.float32)
    xyt, dt = model.op_segments_setup(turned, H, W, view=view)
    assert np.abs(xyr.cpu().numpy().astype(np.int64) - xyt.cpu().numpy()).max() <= 2 * XY_BAR and np.abs(dr.cpu().numpy() - dt.cpu().numpy()).max() <= 2 * DEPTH_BAR


@pytest.mark.parametrize("W,H", SIZES)
def test_setup_centres_and_invalid_points(model, view, W, H):
    P = view[0]
    cells = sorted({(0, 0), (W - 1, H - 1), (W // 2, H // 3), (W // 3, H - 1)})
    centres = np.array([unproject(i + 0.5, j + 0.5, dd, H, W, view) for (i, j), dd in zip(cells, (-0.3, 0.0, 0.4, 0.7))]).astype(np.float32)
    eye = -P[3, :3] * (P[3, 3] + 1.0) / (P[3, :3] @ P[3, :3])              # homogeneous coordinate -1: behind the eye
    on_eye = -P[3, :3] * P[3, 3] / (P[3, :3] @ P[3, :3])                   # homogeneous coordinate 0 up to rounding: behind or invalid by its window
    far = unproject(2.0**21, 0.5, 0.0, H, W, view)                         # 2^21 pixels to the right
    far_y = unproject(0.5, -2.0**21, 0.0, H, W, view)
    bad = np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), eye, far, far_y], np.float32)
    pts = np.concatenate([centres, bad, on_eye[None].astype(np.float32)])
    xy, d = model.op_segments_setup(pts, H, W, view=view)
    xy, d = xy.cpu().numpy(), d.cpu().numpy()
    n = len(cells)
    assert np.array_equal(xy[:n], [(256 * i + 128, 256 * j + 128) for i, j in cells])      # a pixel centre snaps exactly
    assert (xy[n:n + len(bad)] == sg.SENTINEL).all()
    assert sg.project(bad, H, W, view)[2].tolist() == [False] * len(bad)
    assert np.isfinite(d).all()


# ------------------------------------------------------------------ 2. coverage and the winning segment
def test_scene_names(scenes, bones):
    assert set(scenes) == set(sg.winner_scenes(bones[0])) | set(sg.COVER_ONLY)


@pytest.mark.parametrize("name", sorted(sg.scenes([(0, 1)])))
def test_cover(drawn, name):
    rc.check_cover(drawn[name]["winner"], drawn[name]["ref"])


@pytest.mark.parametrize("name", sorted(sg.winner_scenes([(0, 1)])))
def test_winner(drawn, name):
    d = drawn[name]
    rc.check_winner(d["winner"], d["ref"], d["d1"], d["d2"])


def test_rules_by_name(drawn, scenes):
    """What the scenes are for, read off the DEVICE's pictures."""
    for name in ("horizontal", "vertical", "diagonal", "antidiagonal", "slanted"):
        a, b = drawn[name + "_fwd"]["winner"], drawn[name + "_back"]["winner"]
        assert (a >= 0).sum() > 90 and np.array_equal(a, b), name
    assert (drawn["diagonal_fwd"]["winner"] >= 0).sum() == 35 * 3
    assert set(np.unique(drawn["zero_length"]["winner"])) == {-1, 2}
    assert not (drawn["wholly_outside"]["winner"] >= 0).any()
    through = drawn["through_image"]["winner"]
    assert ((through == 0).sum(0) == 2).all() and (through == 1).sum(1).max() == 3
    ends = drawn["ends_on_centres"]["winner"]
    assert (ends == 0).sum() == 16 and (ends == 1).sum() == 44
    edge = drawn["wide_at_edges"]["winner"]
    assert (edge[-1] >= 0).all() and (edge[:, -1] >= 0).all()
    one = lambda name, s: sg.rasterise_segments(scenes[name]["xy"], scenes[name]["d"], scenes[name]["segments"][s:s + 1], scenes[name]["widths"][s:s + 1], 48, 64)[0] >= 0
    for name, near in (("crossing_gap", 1), ("crossing_gap_swapped", 0)):
        both = one(name, 0) & one(name, 1)
        assert both.sum() >= 9 and (drawn[name]["winner"][both] == near).all(), name
    co = drawn["coincident_equal_depth"]["winner"]
    assert (co == 0).sum() > 100 and not (co == 1).any() and (co == 2).any()
    assert (drawn["long_97x61"]["winner"] >= 0).any(0).all()               # 97 covered major indices: every lane steps by 64
    assert drawn["one_pixel_1x1"]["winner"].tolist() == [[1]]
    widths = drawn["widths_1_2_3_16"]["winner"]
    assert [(widths == s).sum(0).max() for s in range(4)] == [1, 2, 3, 16]
    for name in ("spin_k0_64x48_w2", "spin_k2_97x61_w3"):
        assert (drawn[name]["winner"] >= 0).sum() > 100


# ------------------------------------------------------------------ 3. render_segments end to end
GUARD = 4096


def _canvas(F, H, W, seed):
    g = np.random.Generator(np.random.Philox(key=[seed, F * H * W]))
    flat = torch.from_numpy(g.integers(0, 256, F * H * W * 3 + 2 * GUARD, dtype=np.uint8)).cuda()
    return flat, flat[GUARD:GUARD + F * H * W * 3].view(F, H, W, 3), flat.cpu().numpy().copy()


def _guards_unchanged(flat, before):
    after = flat.cpu().numpy()
    assert np.array_equal(after[:GUARD], before[:GUARD]) and np.array_equal(after[-GUARD:], before[-GUARD:]), "a guard region changed"


@pytest.mark.parametrize("name", ("spin_k0_64x48_w2", "spin_k2_64x48_w1", "spin_k0_97x61_w5", "spin_k2_97x61_w3", "spin_k1_97x61_w2"))
def test_render_against_compose(model, drawn, scenes, bones, view, name):
    sc, d = scenes[name], drawn[name]
    H, W = sc["H"], sc["W"]
    flat, img, before = _canvas(1, H, W, 5)
    model.render_segments(img, sc["points"][None], sc["segments"], bones[1], sc["widths"], [0], view=view, rgb=True)
    _guards_unchanged(flat, before)
    was = before[GUARD:GUARD + H * W * 3].reshape(H, W, 3)
    want = sg.compose(was, d["ref"], bones[1])
    got = img.cpu().numpy()[0]
    tie = rc.near_ties(d["d1"], d["d2"])
    assert np.array_equal(got[~tie], want[~tie])                           # byte for byte: the covered in their colour, every other byte as it was
    assert (d["ref"] >= 0).sum() > 100 and (got != was).any()
    # rgb=False: the triple goes down reversed
    flat2, img2, _ = _canvas(1, H, W, 5)
    model.render_segments(img2, sc["points"][None], sc["segments"], bones[1], sc["widths"], [0], view=None, rgb=False)
    got2 = img2.cpu().numpy()[0]
    on = (d["winner"] >= 0) & ~tie
    assert np.array_equal(got2[on], got[on][:, ::-1]) and np.array_equal(got2[d["winner"] < 0], was[d["winner"] < 0])


def _two_skeletons(view, H=48, W=64):
    """Two skeletons of 4 points and 2 segments each, aimed at one image: the first draws only segment 0, the second only segment 1 (the other is
    a point), and where they cross the FIRST is nearer by 0.4."""
    a = [unproject(5.0, 5.0, -0.2, H, W, view), unproject(58.0, 42.0, -0.2, H, W, view)]
    b = [unproject(6.0, 41.0, 0.2, H, W, view), unproject(57.0, 7.0, 0.2, H, W, view)]
    pts = np.array([a + [a[0], a[0]], [b[0], b[0]] + b], np.float32)
    return pts, np.array([(0, 1), (2, 3)]), np.array([(250, 10, 20), (10, 20, 250)], np.uint8), np.array([5, 5])


def test_skeletons_of_one_image_share_the_depth_buffer(model, view):
    H, W = 48, 64
    pts, seg, cols, wid = _two_skeletons(view)
    flat, img, before = _canvas(1, H, W, 6)
    model.render_segments(img, pts, seg, cols, wid, [0, 0], view=view)
    _guards_unchanged(flat, before)
    was = before[GUARD:GUARD + H * W * 3].reshape(H, W, 3)
    xy, d = zip(*[[t.cpu().numpy() for t in model.op_segments_setup(p, H, W, view=view)] for p in pts])
    xy, d = np.stack(xy), np.stack(d)
    ref, d1, d2 = sg.rasterise_segments(xy, d, seg, wid, H, W)
    assert not rc.near_ties(d1, d2).any()
    got = img.cpu().numpy()[0]
    assert np.array_equal(got, sg.compose(was, ref, cols))
    cross = (sg.rasterise_segments(xy[0], d[0], seg, wid, H, W)[0] >= 0) & (sg.rasterise_segments(xy[1], d[1], seg, wid, H, W)[0] >= 0)
    assert cross.sum() >= 9 and (ref[cross] == 0).all() and (got[cross] == cols[0]).all()      # the first-drawn is nearer and stays on top
    assert set(np.unique(ref)) == {-1, 0, 3}                                # ids are rank * S + segment
    wrong = sg.rasterise_segments(xy, d, seg, wid, H, W, buffers="per_skeleton")[0]
    assert not np.array_equal(got, sg.compose(was, wrong, cols))           # a depth buffer per skeleton paints the second over the first
    with pytest.raises(AssertionError):
        rc.check_winner(wrong, ref, d1, d2)


def test_five_skeletons_three_images_equal_one_call_each(model, bones, view):
    H, W = 61, 97
    pts = np.stack([sg.placed_skeleton(k, place) for k, place in enumerate((1, 1, 3, 2, 3))])      # side by side: no near-ties in float64
    where = [0, 1, 0, 2, 1]                                                # images 0 and 1 hold two skeletons
    wid = np.full(len(bones[0]), 3)
    runs = []
    for _ in range(2):
        flat, img, before = _canvas(3, H, W, 7)
        model.render_segments(img, pts, bones[0], bones[1], wid, where, view=view)
        _guards_unchanged(flat, before)
        runs.append(img.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
    for _ in range(2):
        flat, each, before = _canvas(3, H, W, 7)
        for f in range(3):
            mine = [k for k in range(5) if where[k] == f]
            model.render_segments(each, pts[mine], bones[0], bones[1], wid, [f] * len(mine), view=view)
        assert np.array_equal(runs[0], each.cpu().numpy())
    was = before[GUARD:GUARD + 3 * H * W * 3].reshape(3, H, W, 3)
    for f in range(3):                                                     # and each image is the model's composition of its skeletons
        mine = [k for k in range(5) if where[k] == f]
        xy, d = zip(*[[t.cpu().numpy() for t in model.op_segments_setup(pts[k], H, W, view=view)] for k in mine])
        ref, d1, d2 = sg.rasterise_segments(np.stack(xy), np.stack(d), bones[0], wid, H, W)
        tie = rc.near_ties(d1, d2)
        print(f"image {f}: {int(tie.sum())} near-ties among {int((ref >= 0).sum())} covered pixels")
        rc.check_near_tie_cap(ref, d1, d2)                                 # the project's cap: what the comparison below leaves out is at most that
        assert np.array_equal(runs[0][f][~tie], sg.compose(was[f], ref, bones[1])[~tie]), f
        assert (ref >= len(bones[0])).any() == (len(mine) == 2)            # the second skeleton of an image holds pixels of its own


def _model_image(model, view, pts, seg, wid, cols, was, H, W, R=None):
    """The numpy model's picture of the skeletons pts aimed at one image, fed the device's own snapped points; the near-tie mask, capped."""
    xy, d = zip(*[[t.cpu().numpy() for t in model.op_segments_setup(p, H, W, R=R, view=view)] for p in pts])
    ref, d1, d2 = sg.rasterise_segments(np.stack(xy), np.stack(d), seg, wid, H, W)
    rc.check_near_tie_cap(ref, d1, d2)
    return sg.compose(was, ref, cols), rc.near_ties(d1, d2), ref


def test_more_images_than_a_launch_group(model, bones, view):
    """24 images of 97 x 61 in one call: two launch groups (16 + 8 images), the first with 80 skeletons = two launches of setup and of cover.
    Every image against the model and against one call per image."""
    H, W, F = 61, 97, 24
    pts, where = sg.many_images(F, 5)
    wid = np.full(len(bones[0]), 3)
    flat, img, before = _canvas(F, H, W, 9)
    model.render_segments(img, pts, bones[0], bones[1], wid, where, view=view)
    _guards_unchanged(flat, before)
    got = img.cpu().numpy()
    was = before[GUARD:GUARD + F * H * W * 3].reshape(F, H, W, 3)
    for f in range(F):
        want, tie, ref = _model_image(model, view, pts[where == f], bones[0], wid, bones[1], was[f], H, W)
        assert np.array_equal(got[f][~tie], want[~tie]), f
        assert (ref >= 4 * len(bones[0])).any() and (ref >= 0).sum() > 400, f          # the fifth skeleton of the image holds pixels
    flat, each, _ = _canvas(F, H, W, 9)
    order = np.random.Generator(np.random.Philox(key=[9, 1])).permutation(F)            # and the images in another order, one call each
    for f in order:
        model.render_segments(each, pts[where == f], bones[0], bones[1], wid, [int(f)] * 5, view=view)
    assert np.array_equal(got, each.cpu().numpy())
    # the same call with the images named in another order: the slots change, the pictures do not
    perm = np.concatenate([np.nonzero(where == f)[0] for f in order])
    flat, again, _ = _canvas(F, H, W, 9)
    model.render_segments(again, pts[perm], bones[0], bones[1], wid, where[perm], view=view)
    assert np.array_equal(got, again.cpu().numpy())


def test_more_points_than_the_workspace_holds(model, view):
    """70 skeletons of 1024 points aimed at one image (and 3 at another): 71 680 points against the 65 536 the record area holds, so the group
    goes through in two passes over a depth image cleared as a whole."""
    H, W = 61, 97
    pts, where, seg, wid = sg.many_points(70, 3, 1024)
    cols = np.array([(250, 10, 20), (10, 20, 250)], np.uint8)
    flat, img, before = _canvas(2, H, W, 10)
    dev = torch.from_numpy(pts).cuda()
    model.render_segments(img, dev, seg, cols, wid, where, view=view)
    _guards_unchanged(flat, before)
    got = img.cpu().numpy()
    was = before[GUARD:GUARD + 2 * H * W * 3].reshape(2, H, W, 3)
    for f in range(2):
        want, tie, ref = _model_image(model, view, pts[where == f], seg, wid, cols, was[f], H, W)
        assert np.array_equal(got[f][~tie], want[~tie]), f
        assert ref.max() >= (2 * 65 if f == 0 else 2), f                   # skeletons of the second pass hold pixels
    # the other order of the two images: image 1's skeletons first, so that the large image is the second slot
    flip = np.r_[np.nonzero(where == 1)[0], np.nonzero(where == 0)[0]]
    flat, again, _ = _canvas(2, H, W, 10)
    model.render_segments(again, dev[torch.from_numpy(flip).cuda()], seg, cols, wid, where[flip], view=view)
    assert np.array_equal(got, again.cpu().numpy())


def test_render_with_R_equals_points_turned_on_the_host(model, bones, view):
    H, W = 61, 97
    pts = np.stack([sg.placed_skeleton(0, 1), sg.placed_skeleton(2, 3)])
    wid = np.full(len(bones[0]), 3)
    # a quarter turn about z is exact in fp32 on both sides: the same bytes
    Q = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    small = (pts * np.float32(0.5)).astype(np.float32)
    flat, a, before = _canvas(1, H, W, 11)
    model.render_segments(a, small, bones[0], bones[1], wid, [0, 0], R=Q, view=view)
    _guards_unchanged(flat, before)
    flat, b, _ = _canvas(1, H, W, 11)
    model.render_segments(b, small @ Q.T, bones[0], bones[1], wid, [0, 0], view=view)
    was = before[GUARD:GUARD + H * W * 3].reshape(H, W, 3)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and (a.cpu().numpy()[0] != was).any(-1).sum() > 100
    # a general rotation: against the model fed the setup hook's points for the same R, and within the setup bar of the points turned on the host
    t = 0.7
    R = (np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]]) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])).astype(np.float32)
    flat, c, _ = _canvas(1, H, W, 11)
    model.render_segments(c, pts, bones[0], bones[1], wid, [0, 0], R=R, view=view)
    want, tie, ref = _model_image(model, view, pts, bones[0], wid, bones[1], was, H, W, R=R)
    assert np.array_equal(c.cpu().numpy()[0][~tie], want[~tie]) and (ref >= 0).sum() > 200
    turned = (pts.astype(np.float64) @ R.astype(np.float64).T).astype(np.float32)
    for p, q in zip(pts, turned):
        (xy_r, d_r), (xy_t, d_t) = model.op_segments_setup(p, H, W, R=R, view=view), model.op_segments_setup(q, H, W, view=view)
        assert (xy_r.long() - xy_t.long()).abs().max().item() <= 2 * XY_BAR and (d_r - d_t).abs().max().item() <= 2 * DEPTH_BAR


# ------------------------------------------------------------------ 4. spin_joints
@pytest.mark.parametrize("T", (1, 3, 5))
def test_spin_joints_equal_smooth_pose(model, T):
    """max_frames = 2: T = 3 = max_frames + 1 crosses a chunk boundary, T = 5 two."""
    assert model.max_frames == 2
    g = np.random.Generator(np.random.Philox(key=[T, 11]))
    pose = (g.standard_normal((T, 72)) * 0.3).astype(np.float32)
    betas = np.repeat((g.standard_normal((1, 10)) * 0.5).astype(np.float32), T, 0)
    verts, _, j29 = model.smooth_pose(pose, betas, joints="spin2")
    for kind, nj in (("spin49", 49), ("spin2", 29), ("kinectv2", 25)):
        want = model.smooth_pose(pose, betas, joints=kind)[2].cpu().numpy()
        got = model.spin_joints(j29, verts, joints=kind).cpu().numpy()
        assert got.shape == (T, nj, 3) and np.array_equal(got, want), kind
    with pytest.raises(ValueError):
        model.spin_joints(j29, verts, joints="common")


# ------------------------------------------------------------------ 5. refusals
def test_refusals(pkg, model, view, bones):
    lib, L = model._lib, pkg._lib
    H, W, F, n, P = 48, 64, 2, 2, 49
    S = len(bones[0])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pts = torch.from_numpy(np.stack([sg.spin_points((0, 7)), sg.spin_points((2, 7))])).cuda()
    back = np.random.Generator(np.random.Philox(key=[8, 8])).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    img = torch.from_numpy(back.copy()).cuda()
    good = dict(points=pts.data_ptr(), n=n, P=P, seg=np.ascontiguousarray(bones[0], np.int32), S=S, col=np.ascontiguousarray(bones[1]), wid=np.full(S, 2, np.int32),
                idx=np.array([0, 1], np.int32), R=np.eye(3, dtype=np.float32).reshape(9), proj=np.ascontiguousarray(view[0].reshape(16)),
                window=np.array(view[1], np.float64), images=img.data_ptr(), F=F, H=H, W=W)

    def call(**kw):
        a = dict(good, **kw)
        ptr = lambda v: None if v is None else (v if isinstance(v, int) else p(v))
        r = lib.grnet_render_segments(model._h, ptr(a["points"]), a["n"], a["P"], ptr(a["seg"]), a["S"], ptr(a["col"]), ptr(a["wid"]), ptr(a["idx"]), ptr(a["R"]),
                                      ptr(a["proj"]), ptr(a["window"]), ptr(a["images"]), a["F"], a["H"], a["W"], None)
        torch.cuda.synchronize()
        return r, lib.grnet_last_error(model._h)

    def changed(v, at, value):
        v = v.copy()
        v.reshape(-1)[at] = value
        return v

    cases = [(dict(n=-1), b"n -1 < 0"), (dict(P=0), b"P 0 outside [1, 1024]"), (dict(P=1025), b"P 1025 outside"), (dict(S=-1), b"S -1 outside [0, 4096]"),
             (dict(S=4097), b"S 4097 outside"), (dict(H=0), b"image 0 x 64 outside [1, 4096]"), (dict(W=4097), b"image 48 x 4097 outside"), (dict(F=0), b"F 0 < 1"),
             (dict(seg=changed(good["seg"], 3, 49)), b"segment 1 names point 49, outside [0, 49)"), (dict(seg=changed(good["seg"], 0, -1)), b"names point -1"),
             (dict(wid=changed(good["wid"], 2, 0)), b"widths[2] = 0 outside [1, 16]"), (dict(wid=changed(good["wid"], 0, 17)), b"widths[0] = 17"),
             (dict(idx=changed(good["idx"], 1, 2)), b"image_index[1] = 2 outside [0, 2)"), (dict(idx=changed(good["idx"], 0, -1)), b"image_index[0] = -1"),
             (dict(R=changed(good["R"], 4, np.nan)), b"R has a non-finite"), (dict(proj=changed(good["proj"], 7, np.inf)), b"proj has a non-finite"),
             (dict(window=changed(good["window"], 1, np.nan)), b"window has a non-finite"), (dict(window=changed(good["window"], 1, good["window"][0])), b"is empty"),
             (dict(window=changed(good["window"], 3, -1.0)), b"is empty")]
    cases += [(dict(**{k: None}), b"null pointer") for k in ("points", "seg", "col", "wid", "idx", "proj", "window", "images")]
    # an empty call with a bad size is still refused
    cases += [(dict(n=0, P=0), b"P 0 outside"), (dict(n=0, H=5000), b"image 5000 x 64"), (dict(n=0, F=0), b"F 0 < 1"), (dict(n=0, S=5000), b"S 5000 outside")]
    for kw, text in cases:
        r, msg = call(**kw)
        assert r == L.EINVAL and msg.startswith(b"grnet_render_segments: ") and text in msg, (kw.keys(), msg)
    # more skeletons aimed at one image than rank * S + segment holds in 31 bits: checked on the host, before anything is read on the device
    big = 2**31 // 4096 + 1
    r, msg = call(n=big, P=1, S=4096, seg=np.zeros((4096, 2), np.int32), col=np.zeros((4096, 3), np.uint8), wid=np.ones(4096, np.int32), idx=np.zeros(big, np.int32))
    assert r == L.EINVAL and b"31 bits" in msg
    assert lib.grnet_render_segments(None, None, 0, 1, None, 0, None, None, None, None, None, None, None, 1, 1, 1, None) == L.EINVAL
    assert np.array_equal(img.cpu().numpy(), back)                         # no refusal touched the images
    # n == 0 reads no pointer; S == 0 draws nothing; R == NULL is the identity
    assert call(n=0, points=None, seg=None, col=None, wid=None, idx=None, proj=None, window=None, images=None)[0] == 0
    assert call(S=0)[0] == 0 and np.array_equal(img.cpu().numpy(), back)
    assert call()[0] == 0
    first = img.cpu().numpy()
    img.copy_(torch.from_numpy(back))
    assert call(R=None)[0] == 0 and np.array_equal(img.cpu().numpy(), first) and not np.array_equal(first, back)
    # the hooks
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    one = np.zeros((1, 2), np.int32)
    w1 = np.ones(1, np.int32)
    hook = lambda *a: lib.grnet_op_raster_segments(model._h, *a)
    assert hook(out.data_ptr(), out.data_ptr(), 0, p(one), 1, p(w1), 8, 8, out.data_ptr(), None) == L.EINVAL and b"grnet_op_raster_segments: P 0" in lib.grnet_last_error(model._h)
    assert hook(out.data_ptr(), out.data_ptr(), 2, p(one), 1, p(w1), 8, 4097, out.data_ptr(), None) == L.EINVAL
    assert hook(None, out.data_ptr(), 2, p(one), 1, p(w1), 8, 8, out.data_ptr(), None) == L.EINVAL and b"null pointer" in lib.grnet_last_error(model._h)
    assert hook(out.data_ptr(), out.data_ptr(), 2, p(changed(one, 1, 2)), 1, p(w1), 8, 8, out.data_ptr(), None) == L.EINVAL
    assert hook(out.data_ptr(), out.data_ptr(), 2, p(one), 1, p(changed(w1, 0, 17)), 8, 8, out.data_ptr(), None) == L.EINVAL
    assert lib.grnet_op_segments_setup(model._h, pts.data_ptr(), 0, None, p(good["proj"]), p(good["window"]), 8, 8, out.data_ptr(), out.data_ptr(), None) == L.EINVAL
    assert lib.grnet_op_segments_setup(model._h, pts.data_ptr(), 2, None, p(good["proj"]), p(changed(good["window"], 0, 1.0)), 8, 8, out.data_ptr(), out.data_ptr(), None) == L.EINVAL
    assert b"is empty" in lib.grnet_last_error(model._h)
    # spin_joints
    v = torch.zeros(1, 6890, 3, device="cuda")
    k = torch.zeros(1, 29, 3, device="cuda")
    o = torch.zeros(1, 49, 3, device="cuda")
    assert lib.grnet_spin_joints(model._h, k.data_ptr(), v.data_ptr(), -1, 0, o.data_ptr(), None) == L.EINVAL
    assert lib.grnet_spin_joints(model._h, k.data_ptr(), v.data_ptr(), 1, 3, o.data_ptr(), None) == L.EINVAL and b"joints_kind" in lib.grnet_last_error(model._h)
    assert lib.grnet_spin_joints(model._h, None, v.data_ptr(), 1, 0, o.data_ptr(), None) == L.EINVAL
    assert lib.grnet_spin_joints(model._h, None, None, 0, 0, None, None) == 0
    bare = pkg.GRNet(max_frames=1)                                         # no SMPL tables
    try:
        assert lib.grnet_spin_joints(bare._h, k.data_ptr(), v.data_ptr(), 1, 0, o.data_ptr(), None) == L.ESTATE
        assert b"SMPL tables were not loaded" in lib.grnet_last_error(bare._h)
        with pytest.raises(L.GrnetError, match="SMPL tables"):
            bare.spin_joints(k, v)
    finally:
        bare.close()


# ------------------------------------------------------------------ 6. demo.py
def _panel_model(model, pipe, demo, view, H, W, persons, rot, joint_type):
    """The numpy model's panel: white, the grid, then the persons (their joints in joint_type's skeleton, call order) in one depth buffer -- fed
    the device's own snapped points from the setup hook."""
    bone_w, grid_w = demo.skeleton_widths(H, W)
    panel = np.full((H, W, 3), 255, np.uint8)
    gp, gs = pipe.skeleton_grid()
    xy, d = [t.cpu().numpy() for t in model.op_segments_setup(gp, H, W, view=view)]
    gw = np.full(len(gs), grid_w)
    ref = sg.rasterise_segments(xy, d, gs, gw, H, W)[0]
    panel = sg.compose(panel, ref, [pipe.GRID_COLOUR] * len(gs))
    tie = np.zeros((H, W), bool)                                           # one colour: a near-tie between grid lines changes no byte
    if persons:
        bones, cols = pipe.skeleton_bones(joint_type)
        xy, d = zip(*[[t.cpu().numpy() for t in model.op_segments_setup(j, H, W, R=rot, view=view)] for j in persons])
        ref, d1, d2 = sg.rasterise_segments(np.stack(xy), np.stack(d), bones, np.full(len(bones), bone_w), H, W)
        panel = sg.compose(panel, ref, cols)
        tie = rc.near_ties(d1, d2)
        assert (ref >= 0).sum() > 20
    return panel, tie


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """160 x 120, 30 frames, two persons, frames 28 and 29 empty; the plain run's pickle, shared by the cases below; nothing modifies it."""
    from PIL import Image
    sys.path.insert(0, ROOT)
    demo = importlib.import_module("demo")
    tmp = tmp_path_factory.mktemp("skeleton_demo")
    H, W, T = 120, 160, 30
    g = np.random.Generator(np.random.Philox(key=[21, 21]))
    img_dir = str(tmp / "vid")
    os.makedirs(img_dir)
    frames = g.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(img_dir, f"{i:06d}.png"))
    box = lambda n, cx: np.tile(np.array([[cx, 60.0, 90.0, 90.0]], np.float32), (n, 1))
    tp = str(tmp / "tracking.pkl")
    # person 1: frames 0..25, person 2: frames 2..27 -- both in 2..25, nobody in 28, 29
    joblib.dump({1: {"bbox": box(26, 60.0), "frames": np.arange(0, 26)}, 2: {"bbox": box(26, 100.0), "frames": np.arange(2, 28)}}, tp)
    base = ["--img_folder", img_dir, "--tracking_path", tp, "--synthetic_weights", "--grnet_batch_size", "16", "--max_frames", "16", "--save_vid"]
    run = lambda name, *flags: demo.main(demo.parser().parse_args(base + ["--output_folder", str(tmp / name)] + list(flags)))
    plain = run("plain")
    assert not [x for x in os.listdir(os.path.dirname(plain)) if x.endswith("_output")]      # without the flag no folder
    return dict(demo=demo, tmp=tmp, H=H, W=W, T=T, frames=frames, base=base, run=run, plain=joblib.load(plain))


@pytest.mark.parametrize("case", ("spin", "smooth", "kinectv2"))
def test_demo_skeleton_view(model, pipe, view, clip, case):
    from PIL import Image
    demo, H, W, T, frames, run, ref = (clip[k] for k in ("demo", "H", "W", "T", "frames", "run", "plain"))
    flags = {"spin": [], "smooth": ["--smooth"], "kinectv2": ["--joint_type", "kinectv2"]}[case]
    against = ref if case == "spin" else joblib.load(run(case + "_plain", *flags))
    out = run(case, "--skeleton_view", *flags)
    res = joblib.load(out)
    assert set(res) == set(against) == {1, 2}
    for pid in res:                                                                      # the pickle is what it is without the flag
        assert set(res[pid]) == set(against[pid])
        for k in res[pid]:
            assert np.array_equal(res[pid][k], against[pid][k]) and res[pid][k].dtype == against[pid][k].dtype, (pid, k)
    folder = out[:-len(".pkl")] + "_output"
    pngs = sorted(os.listdir(folder))
    assert pngs == [f"{i:06d}.png" for i in range(T)]
    pics = np.stack([np.asarray(Image.open(os.path.join(folder, x))) for x in pngs])
    assert pics.shape == (T, H, 2 * W, 3)
    assert np.array_equal(pics[:, :, :W], frames)                                        # the left half is the input, untouched
    empty, _ = _panel_model(model, pipe, demo, view, H, W, [], None, "spin")
    assert (empty != 255).any()
    for i in (28, 29):                                                                   # nobody there: the grid alone
        assert np.array_equal(pics[i, :, W:], empty), i
    # the 49 joints the view is defined on: --smooth stores them; a plain forward's are formed from its 29 joints and its vertices
    if case == "smooth":
        j49 = {pid: against[pid]["joints3d"] for pid in against}
    else:
        j49 = {pid: model.spin_joints(ref[pid]["joints3d"], ref[pid]["verts"]).cpu().numpy() for pid in ref}
    assert all(v.shape[1:] == (49, 3) for v in j49.values())
    joint_type = "kinectv2" if case == "kinectv2" else "spin"
    shown = {pid: (v if joint_type == "spin" else pipe.convert_kps(v, "spin", joint_type)) for pid, v in j49.items()}
    rot = pipe.body_rotation(j49[2][10])                                                 # frame 10 of the last person processed
    for i in (0, 10, 27):
        order = pipe.prepare_rendering_results(res, list(range(T)))[i]
        persons = [shown[pid][pd["row"]] for pid, pd in order.items()]
        assert len(persons) == (2 if i == 10 else 1)
        want, tie = _panel_model(model, pipe, demo, view, H, W, persons, rot, joint_type)
        got = pics[i, :, W:]
        print(f"{case} frame {i}: {int(tie.sum())} near-ties")
        assert np.array_equal(got[~tie], want[~tie]) and tie.sum() <= 4, i               # (the count: so that the comparison is not empty-handed)
        assert not np.array_equal(got, empty)


def test_demo_refuses_both_outputs(clip):
    """The two outputs are alternatives: one line, no traceback, nothing written."""
    import subprocess
    demo, tmp = clip["demo"], clip["tmp"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py")] + clip["base"] + ["--output_folder", str(tmp / "both"), "--skeleton_view", "--mesh_render"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stderr.strip() == demo.refusal(demo.parser().parse_args(["--skeleton_view", "--mesh_render"]))
    assert not os.path.exists(tmp / "both")


# ------------------------------------------------------------------ 7. one production-size frame
def test_one_1080p_frame(model, bones, view):
    sc = sg.scene_1080p(bones[0])
    d = _draw(model, sc, view)
    rc.check_cover(d["winner"], d["ref"])
    rc.check_winner(d["winner"], d["ref"], d["d1"], d["d2"])
    assert (d["winner"] >= 0).sum() > 30000
    # the same four skeletons as four skeletons of one image, through the entry point
    H, W = sc["H"], sc["W"]
    img = torch.full((1, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    model.render_segments(img, sc["points"].reshape(4, 49, 3), bones[0], bones[1], np.full(len(bones[0]), 13), [0, 0, 0, 0], view=view)
    want = sg.compose(np.full((H, W, 3), 255, np.uint8), d["ref"], np.tile(bones[1], (4, 1)))
    tie = rc.near_ties(d["d1"], d["d2"])
    assert np.array_equal(img.cpu().numpy()[0][~tie], want[~tie])
