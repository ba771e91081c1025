"""The per-frame boxes from 2D joints on the host: pipeline.track_boxes, the numpy float64 statement, and its two filters against the
golden values the reference's lib/utils/smooth_bbox.py gave (tests/golden/track_boxes.npz; the bars: tests/helpers/track_checks.py); the rules the
goldens do not reach (pad = edge, status 3, a NaN joint, sequences lying back to back); csrc/track_boxes.h, the arithmetic the kernels run, through
tests/helpers/track_boxes_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly; and the C
exports.  Every worst ratio is printed before it is asserted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import track_checks as tk


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


@pytest.fixture(scope="module")
def g():
    return tk.golden()


def test_golden_file_is_what_the_tool_states(g):
    for name in tk.CASES:
        kp = g[name + "_kp"]
        start, end = (int(v) for v in g[name + "_range"])
        assert kp.shape == (tk.FRAMES[name], 25, 3) and kp.dtype == np.float64
        det = tk.detected(kp)
        if name == "dead":
            assert not det.any() and (start, end) == (-1, 0) and g[name + "_params"].shape == (0, 3)
            continue
        assert (start, end) == (np.flatnonzero(det)[0], np.flatnonzero(det)[-1] + 1)
        for key in ("_params", "_median", "_smooth"):
            assert g[name + key].shape == (end - start, 3) and g[name + key].dtype == np.float64
    assert np.flatnonzero(~tk.detected(g["t26gaps_kp"])).tolist() == [0, 1, 7, 13, 14, 15, 24, 25]
    assert g["t26gaps_kp"][0, 4, 2] == tk.VIS_THRESH             # a score exactly at the threshold, in a dead frame
    assert 0.2 < (~tk.detected(g["t70_kp"])).mean() < 0.4
    assert np.flatnonzero(~tk.detected(g["point_kp"])).tolist() == [3]
    assert float(g["t5_sigma"]) == float(g["t70_sigma"]) == 8.0 and float(g["t12_sigma"]) == 3.0


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_track_boxes", 13), ("grnet_op_median1d", 8), ("grnet_op_gauss1d", 7)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    assert lib.grnet_track_boxes(None, None, 25, None, 1, 0.3, 11, 3.0, 0, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_median1d(None, None, None, 1, 11, 0, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gauss1d(None, None, None, 1, 3.0, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("track_boxes", "op_median1d", "op_gauss1d"))


@pytest.mark.parametrize("name", tk.CASES)
def test_statement_against_get_all_bbox_params(pipe, g, name):
    out = pipe.track_boxes(g[name + "_kp"], vis_thresh=tk.VIS_THRESH, return_params=True)
    assert out["range"].tolist() == [g[name + "_range"].tolist()] and out["range"].dtype == np.int32 and out["status"].dtype == np.int32
    ratio = tk.check_unsmoothed(out, g, name)
    print(f"{name}: worst scale error / (8 u) = {ratio:.3g}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", [n for n in tk.CASES if n != "dead"])
def test_filters_against_the_reference_stage_by_stage(pipe, g, name):
    params, median, smooth, sigma = g[name + "_params"], g[name + "_median"], g[name + "_smooth"], float(g[name + "_sigma"])
    for c in range(3):
        got = pipe.median_filter1d(params[:, c], tk.KERNEL, "zero")
        assert np.array_equal(got.view(np.int64), median[:, c].view(np.int64)), f"{name}: the median of column {c} differs in some bit"
        got = pipe.gauss_filter1d(median[:, c], sigma)
        bar = tk.gauss_bar(median[:, c], sigma)
        ratio = np.abs(got - smooth[:, c]).max() / bar if bar > 0 else float(np.abs(got - smooth[:, c]).max() > 0)
        print(f"{name} column {c}: worst Gaussian error / ((2 r + 8) u max|x|) = {ratio:.3g}")
        assert ratio <= 1.0


@pytest.mark.parametrize("name", [n for n in tk.CASES if n != "dead"])
def test_statement_against_smooth_bbox_params(pipe, g, name):
    out = pipe.track_boxes(g[name + "_kp"], vis_thresh=tk.VIS_THRESH, kernel_size=tk.KERNEL, sigma=float(g[name + "_sigma"]))
    ratio = tk.check_smoothed(out, g, name)
    print(f"{name}: worst error / the chain's bar = {ratio:.3g}")
    assert ratio <= 1.0
    if name in ("t1", "t2", "t5"):                               # more than half of every window is padding: scipy's zeros, status 3 everywhere
        assert (out["status"] == 3).all() and (out["boxes"] == 0).all()


def test_reflect_index(pipe):
    for n in range(1, 6):
        want = np.pad(np.arange(n), 32, mode="symmetric")
        assert np.array_equal(pipe.track_reflect(np.arange(-32, n + 32), n), want)


def test_pad_edge_has_no_status_3(pipe, g):
    for name in ("t12", "t26gaps", "t2", "t1"):
        out = pipe.track_boxes(g[name + "_kp"], vis_thresh=tk.VIS_THRESH, kernel_size=tk.KERNEL, sigma=3.0, pad="edge", return_params=True)
        start, end = out["range"][0]
        assert (out["status"][start:end] < 2).all() and (out["boxes"][start:end, 2] > 0).all()
        col = g[name + "_params"][:, 0]
        want = np.array([np.median(np.pad(col, 5, mode="edge")[i:i + 11]) for i in range(col.size)])
        assert np.array_equal(pipe.median_filter1d(col, 11, "edge"), want)


def test_sequences_do_not_see_each_other(pipe, g):
    order = ("t26gaps", "t5", "dead", "t70", "t1", "point")
    kp = np.concatenate([g[n + "_kp"] for n in order])
    for kw in (dict(), dict(kernel_size=11, sigma=8.0), dict(kernel_size=11, sigma=3.0, pad="edge")):
        whole = pipe.track_boxes(kp, lengths=[tk.FRAMES[n] for n in order], vis_thresh=tk.VIS_THRESH, **kw)
        a = 0
        for q, n in enumerate(order):
            alone = pipe.track_boxes(g[n + "_kp"], vis_thresh=tk.VIS_THRESH, **kw)
            T = tk.FRAMES[n]
            assert np.array_equal(whole["boxes"][a:a + T].view(np.int64), alone["boxes"].view(np.int64)), (n, kw)
            assert np.array_equal(whole["status"][a:a + T], alone["status"]) and whole["range"][q].tolist() == alone["range"][0].tolist()
            a += T


def test_nan_joint_makes_its_frame_interpolated(pipe, g):
    kp = g["t12_kp"].copy()
    clean = pipe.track_boxes(kp, vis_thresh=tk.VIS_THRESH)
    j = int(np.flatnonzero(kp[5, :, 2] > tk.VIS_THRESH)[0])
    kp[5, j, 0] = np.nan
    out = pipe.track_boxes(kp, vis_thresh=tk.VIS_THRESH)
    assert out["status"].tolist() == [0] * 5 + [1] + [0] * 6 and np.isfinite(out["boxes"]).all()
    rest = np.arange(12) != 5
    assert np.array_equal(out["boxes"][rest].view(np.int64), clean["boxes"][rest].view(np.int64))
    assert out["boxes"][5, 0] == np.linspace(clean["boxes"][4, 0], clean["boxes"][6, 0], 3)[1]
    kp[5, j] = (np.nan, np.nan, 0.0)                            # beside a dead score the NaN is not looked at
    assert pipe.track_boxes(kp, vis_thresh=tk.VIS_THRESH)["status"][5] == 0


def test_gap_across_a_64_frame_boundary(pipe):
    kp = np.tile(tk.golden()["t70_kp"][:1], (130, 1, 1))
    kp[:, :, 0] += 3.0 * np.arange(130)[:, None]
    kp[60:71, :, 2] = 0.0
    out = pipe.track_boxes(kp, vis_thresh=tk.VIS_THRESH, return_params=True)
    assert out["range"].tolist() == [[0, 130]] and out["status"].tolist() == [0] * 60 + [1] * 11 + [0] * 59
    for c in (0, 1, 2):
        assert np.array_equal(out["params"][60:71, c], np.linspace(out["params"][59, c], out["params"][71, c], 13)[1:-1])
    assert np.array_equal(out["boxes"][:, 0], out["params"][:, 0]) and np.array_equal(out["boxes"][:, 3], 150.0 / out["params"][:, 2])


def test_bad_arguments_are_refused(pipe, g):
    kp = g["t12_kp"]
    for kw, word in ((dict(kernel_size=10), "kernel_size"), (dict(kernel_size=33), "kernel_size"), (dict(kernel_size=0), "kernel_size"),
                     (dict(sigma=-1.0), "sigma"), (dict(sigma=np.nan), "sigma"), (dict(sigma=16.5), "sigma"), (dict(vis_thresh=np.inf), "vis_thresh"),
                     (dict(pad="wrap"), "pad"), (dict(lengths=[5, 6]), "lengths"), (dict(lengths=[12, 0]), "lengths")):
        with pytest.raises(ValueError, match=word):
            pipe.track_boxes(kp, **kw)
    with pytest.raises(ValueError, match="joints2d"):
        pipe.track_boxes(np.zeros((3, 65, 3)))


def test_header_on_the_host_under_sanitizers(tmp_path):
    """csrc/track_boxes.h itself: the reflect index for n = 1 .. 5 with r = 32 against a table written out by hand, the previous / next search
    across 64-frame word boundaries, the selection median with ties against a sort, the Gaussian's order, the frame rule with NaN and infinities."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "track_boxes_check.cpp")
    exe = str(tmp_path / "track_boxes_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]


def test_header_includes_only_the_fill_statement():
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "track_boxes.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "translation3.h"']
    assert "translation3_fill(" in src
