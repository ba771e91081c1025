"""The host side of demo.py --skeleton_view against tests/golden/skeleton_view.npz, which tools/make_goldens_skeleton.py wrote from
matplotlib, scipy and the reference's skeleton tables: the view matrix and window by the project's closed formula, the bone tables, the body
rotation, the grid's panes, the new flag and its refusals.  No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import segment_checks as sg


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "skeleton_view.npz"))


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


@pytest.fixture(scope="module")
def demo():
    sys.path.insert(0, ROOT)
    return importlib.import_module("demo")


def _projected(P, points):
    hom = points @ P[:, :3].T + P[:, 3]
    return hom[:, :2] / hom[:, 3:]


def test_view_is_matplotlibs(pipe, gold):
    P, window = pipe.skeleton_view()
    assert P.shape == (4, 4) and P.dtype == np.float64 and len(window) == 4
    assert np.abs(P - gold["P"]).max() < 1e-12
    assert np.abs(np.asarray(window) - gold["window"]).max() < 1e-12
    assert np.abs(P[3] - (0.830627, -0.253935, 0.152688, 10.0)).max() < 1e-6
    assert np.abs(_projected(P, gold["points"]) - gold["proj"]).max() < 1e-12
    # the model the GPU tests are held against maps the window's corners onto the corners of the centred square
    # (points with homogeneous coordinate 10, the eye distance; the third row of P is the constant -10)
    corners = np.linalg.lstsq(P, 10.0 * np.array([(window[0], window[2], -1.0, 1.0), (window[1], window[3], -1.0, 1.0)]).T, rcond=None)[0].T
    assert np.allclose(corners[:, 3], 1.0)
    xw, yw, _, valid = sg.window_coords(corners[:, :3], 61, 97, (P, window))
    assert valid.all() and np.allclose(xw, [18.0, 79.0], atol=1e-9) and np.allclose(yw, [0.0, 61.0], atol=1e-9)


def test_view_is_matplotlibs_live(pipe):
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig = plt.figure()
    fig.add_subplot(1, 2, 1)
    ax = fig.add_subplot(1, 2, 2, projection="3d")
    ax.view_init(elev=pipe.SKELETON_ELEV, azim=pipe.SKELETON_AZIM)
    (x0, x1), (y0, y1), (z0, z1) = pipe.SKELETON_LIMITS
    ax.set_xlim3d([x0, x1]), ax.set_ylim3d([y0, y1]), ax.set_zlim3d([z0, z1])
    fig.canvas.draw()
    P, window = pipe.skeleton_view()
    assert np.abs(P - ax.get_proj()).max() < 1e-12
    (a0, b0), (a1, b1) = ax.transData.inverted().transform(ax.bbox.get_points())
    assert np.abs(np.asarray(window) - (a0, a1, b0, b1)).max() < 1e-12
    plt.close(fig)


def test_bone_tables(pipe, gold):
    for name, joints in (("spin", 49), ("kinectv2", 25)):
        bones, colours = pipe.skeleton_bones(name)
        assert bones.dtype == np.int64 and np.array_equal(bones, gold["bones_" + name])
        assert bones.min() >= 0 and bones.max() < joints
        assert colours.dtype == np.uint8 and colours.shape == (len(bones), 3)
        assert (colours[0::2] == (215, 48, 39)).all() and (colours[1::2] == (69, 117, 180)).all()
    for name in ("common", "spin2", "coco", ""):
        with pytest.raises(NameError):
            pipe.skeleton_bones(name)


def test_body_rotation(pipe, gold):
    for j, want in zip(gold["joints"], gold["ex_R"]):
        R = pipe.body_rotation(j)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12
        assert np.abs(R[0] - want).max() < 1e-9
        h, v = j[28] - j[27], j[40] - j[39]
        c = np.cross(h / np.linalg.norm(h), v / np.linalg.norm(v))
        assert np.abs(R[0] - c / np.linalg.norm(c)).max() < 1e-12         # the determined part: e_x R
    assert np.array_equal(pipe.body_rotation(gold["joints"][0].astype(np.float32)), pipe.body_rotation(gold["joints"][0].astype(np.float32).astype(np.float64)))


def test_grid_is_on_the_far_panes(pipe):
    P, _ = pipe.skeleton_view()
    pts, seg = pipe.skeleton_grid()
    assert pts.shape == (116, 3) and seg.shape == (58, 2) and np.array_equal(seg, np.arange(116).reshape(58, 2))
    lim = np.array(pipe.SKELETON_LIMITS)
    panes = []
    for axis in range(3):
        centres = np.zeros((2, 3))
        centres[:, axis] = lim[axis]
        far = lim[axis][np.argmax(centres @ P[3, :3] + P[3, 3])]          # the pane with the larger homogeneous coordinate is further from the eye
        panes.append(far)
    assert panes == [0.6, -1.0, 1.0]
    a, b = pts[seg[:, 0]], pts[seg[:, 1]]
    ticks = [np.linspace(lo, hi, k) for (lo, hi), k in zip(lim, (7, 11, 11))]
    count = [0, 0, 0]
    for p, q in zip(a, b):
        fixed = [k for k in range(3) if p[k] == q[k]]
        assert len(fixed) == 2                                             # a line along one axis ...
        on = [k for k in fixed if p[k] == panes[k]]
        assert on, (p, q)                                                  # ... on a far pane ...
        along = [k for k in range(3) if k not in fixed][0]
        assert {p[along], q[along]} == set(lim[along])                     # ... across the whole pane ...
        tick = [k for k in fixed if k != on[0]] if len(on) == 1 else [fixed[1]]
        assert np.isclose(ticks[tick[0]], p[tick[0]]).any()                # ... at a tick
        count[on[0]] += 1
    assert sum(count) == 58


def test_npy_folder_is_refused_before_the_model_runs(demo, tmp_path):
    np.save(str(tmp_path / "000000.npy"), np.zeros((3, 224, 224), np.float32))
    with pytest.raises(SystemExit) as e:
        demo.main(demo.parser().parse_args(["--img_folder", str(tmp_path), "--tracking_path", "none.pkl", "--synthetic_weights", "--skeleton_view",
                                            "--output_folder", str(tmp_path / "out")]))
    assert isinstance(e.value.code, str) and "\n" not in e.value.code and "--skeleton_view" in e.value.code and ".npy crops" in e.value.code
    assert not os.path.exists(tmp_path / "out")


def test_flag_and_refusals(demo):
    p = demo.parser()
    assert p.parse_args([]).skeleton_view is False and p.parse_args(["--skeleton_view"]).skeleton_view is True
    assert demo.refusal(p.parse_args(["--skeleton_view"])) is None
    assert demo.refusal(p.parse_args(["--skeleton_view", "--joint_type", "kinectv2"])) is None
    line = demo.refusal(p.parse_args(["--skeleton_view", "--mesh_render"]))
    assert line and "\n" not in line and "--skeleton_view and --mesh_render" in line and "alternative" in line
    line = demo.refusal(p.parse_args(["--skeleton_view", "--joint_type", "common"]))
    assert line and "\n" not in line and "no bone table for --joint_type common" in line
    line = demo.refusal(p.parse_args(["--skeleton_view", "--display"]))
    assert line and "--display" in line
    assert demo.refusal(p.parse_args(["--mesh_render"])) is None and demo.refusal(p.parse_args(["--joint_type", "common"])) is None
    assert demo.skeleton_widths(480, 640) == (6, 2) and demo.skeleton_widths(120, 160) == (2, 1) and demo.skeleton_widths(1080, 1920) == (13, 5)
