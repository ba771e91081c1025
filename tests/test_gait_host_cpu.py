"""Gait events and parameters on the host: pipeline.gait_parameters, the numpy float64 statement, on the synthetic walker of
tests/helpers/gait_checks.py, whose events and parameters are known analytically; the events rule on a hand-made integer signal whose events are
written out here; sequences lying back to back; csrc/gait_events.h, the arithmetic the kernels run, through tests/helpers/gait_events_check.cpp: a
stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on files this test writes; the C exports and
every refusal.  Every figure is printed before it is asserted.

The issue holds the step length to A (1 - cos(2 pi / P)) of 2 A |sin| at the strike for sigma 0 and 2 alike, but a Gaussian of sigma 2 frames
makes of a sinusoid of period 21.7 one of 0.846 times the amplitude (0.506 m against 0.598 m), so with sigma > 0 the test takes for A the
amplitude of the SMOOTHED sinusoid, A g with g = w0 + 2 sum w_i cos(2 pi i / P) of the Gaussian's own weights: the same bound, now tighter."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import gait_checks as gc

FPS, W, EXC, A, P, T = 20.0, 5, 0.05, 0.3, 21.7, 130
HAND = np.array([0, 1, 3, 3, -2, -4, -1, -4, -6, -2, 0, 4, 2], np.float64)       # 13 frames, window 2
# the plateau 3, 3: the earlier frame (2); -1 at frame 6 is a maximum of its window but negative: no heel strike; 4 at frame 11 is one frame from the
# end of what has a whole window: no event; -4 at frames 5 and 7: the earlier one is a toe-off, -6 at frame 8 another
HAND_HEEL, HAND_TOE = [2], [5, 8]


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def hand_signals():
    """(13,4) = [s, -s, s, -s]: the left foot's events are those of s, the right foot's those of -s."""
    return np.stack([HAND, -HAND, HAND, -HAND], axis=1)


def hand_events():
    ev = np.zeros(13, np.int32)
    ev[HAND_HEEL] |= gc.HEEL_L | gc.TOE_R                       # a maximum of s is a minimum of -s
    ev[HAND_TOE] |= gc.TOE_L | gc.HEEL_R
    return ev


def both_feet_events():
    """Of the signals [s, s, s, s]: both feet strike at the maxima of s and both leave at its minima."""
    ev = np.zeros(13, np.int32)
    ev[HAND_HEEL] |= gc.HEEL_L | gc.HEEL_R
    ev[HAND_TOE] |= gc.TOE_L | gc.TOE_R
    return ev


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_parameters", 15), ("grnet_op_gait_events", 8)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    assert lib.grnet_gait_parameters(None, None, 25, None, 1, None, None, 20.0, 2.0, 5, 0.05, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_events(None, None, None, 1, 5, 0.05, None, None) == pkg._lib.EINVAL
    # without a handle every call is refused, whatever else is wrong with it
    for kw in (dict(J=0), dict(n_seq=0), dict(fps=0.0), dict(fps=float("nan")), dict(sigma=-1.0), dict(sigma=16.5), dict(sigma=float("inf")), dict(window=0),
               dict(window=33), dict(exc=-0.1), dict(exc=float("nan"))):
        a = dict(J=25, n_seq=1, fps=20.0, sigma=2.0, window=5, exc=0.05)
        a.update(kw)
        assert lib.grnet_gait_parameters(None, None, a["J"], None, a["n_seq"], None, None, a["fps"], a["sigma"], a["window"], a["exc"], None, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_parameters", "op_gait_events"))
    assert pkg.pipeline.GAIT_JOINTS_KINECTV2 == gc.KINECTV2 and len(pkg.pipeline.GAIT_COLUMNS) == 18 and len(set(pkg.pipeline.GAIT_COLUMNS)) == 18


@pytest.mark.parametrize("sigma", (0.0, 2.0))
@pytest.mark.parametrize("theta", (0.0, np.deg2rad(40.0), np.pi))
def test_statement_on_the_walker(pipe, theta, sigma):
    joints, trans = gc.walker(T, theta=theta, A=A, P=P)
    out = pipe.gait_parameters(joints, trans=trans, fps=FPS, sigma=sigma, window=W, min_excursion=EXC)
    margin = gc.assert_margin(out["per_frame"], [T], W, EXC)
    print(f"theta {theta:.3f} sigma {sigma:g}: decision margin {margin:.3g} m")
    want = gc.expected_events(T, W, P=P)
    taken = np.zeros(T, np.int32)
    for bit, frames in want.items():
        found = np.flatnonzero(out["events"] & bit)
        print(f"  bit {bit}: expected {frames}, found {found.tolist()}")
        assert len(found) == len(frames) and all(abs(int(a) - b) <= 1 for a, b in zip(found, frames))       # each within one frame, and no others
        taken[found] |= bit
    assert np.array_equal(taken, out["events"])
    row = dict(zip(pipe.GAIT_COLUMNS, out["per_sequence"][0]))
    strikes = sorted([(t, 0) for t in want[gc.HEEL_L]] + [(t, 1) for t in want[gc.HEEL_R]])
    n = sum(a[1] != b[1] for a, b in zip(strikes, strikes[1:]))
    assert row["steps"] == n == 10 and [row[k] for k in pipe.GAIT_COLUMNS[:4]] == [len(want[b]) for b in (1, 2, 4, 8)]
    shift = 1.0 / (FPS * n)                                    # one frame over the n intervals
    print(f"  step time {row['step_time_mean']:.5f} s against {P / 2 / FPS:.5f} +- {shift:.5f}; cadence {row['cadence']:.3f} against {120 * FPS / P:.3f}")
    assert abs(row["step_time_mean"] - P / 2 / FPS) <= shift
    assert abs(row["cadence"] - 120 * FPS / P) <= (120 * FPS / P) * shift / (P / 2 / FPS - shift)
    n_strides = len(want[gc.HEEL_L]) - 1 + len(want[gc.HEEL_R]) - 1
    print(f"  stride time {row['stride_time_mean']:.5f} s against {P / FPS:.5f} +- {1.0 / (FPS * n_strides):.5f}, SD {row['stride_time_sd']:.5f} s")
    assert abs(row["stride_time_mean"] - P / FPS) <= 1.0 / (FPS * n_strides)
    assert row["stride_time_sd"] <= 1.0 / FPS and row["step_time_sd"] <= 1.0 / FPS
    assert row["stride_time_cv"] == 100.0 * row["stride_time_sd"] / row["stride_time_mean"]
    gain = 1.0
    if sigma > 0:
        wts = pipe.gauss_weights(sigma)
        r = wts.size // 2
        gain = float(np.dot(wts, np.cos(2 * np.pi * np.arange(-r, r + 1) / P)))
    bound = A * gain * (1 - np.cos(2 * np.pi / P))
    seconds = [t for (t, f), (_, g) in zip(strikes[1:], strikes[:-1]) if f != g]
    ideal = np.mean([2 * A * gain * abs(np.sin(2 * np.pi * (t - 3.02) / P)) for t in seconds])    # phi = -3.02
    print(f"  step length {row['step_length_mean']:.5f} m against {ideal:.5f} +- {bound:.5f} (gain {gain:.4f}); width {row['step_width_mean']:.5f}")
    assert abs(row["step_length_mean"] - ideal) <= bound and abs(row["step_width_mean"] - 0.2) <= 1e-6
    assert abs(row["speed"] - row["step_length_mean"] * row["cadence"] / 60) <= 1e-12
    print(f"  trajectory speed {row['trajectory_speed']:.5f} m/s against {gc.walker_speed(A, P, FPS):.5f}; stance {row['stance_share']:.2f} %")
    assert abs(row["trajectory_speed"] - gc.walker_speed(A, P, FPS)) <= A * (1 - np.cos(2 * np.pi / P))
    assert abs(row["stance_share"] - 100 * (0.5 + 2.64 / P)) <= 100 * 1.0 / (P - 1)     # toe-off and strike each within half a frame of a stride of P frames
    at = (out["events"] & (gc.HEEL_L | gc.HEEL_R)) != 0
    assert np.isnan(out["per_frame"][~at, 5:]).all() and np.isfinite(out["per_frame"][at, 5:]).all()
    no_trans = pipe.gait_parameters(joints, fps=FPS, sigma=sigma, window=W, min_excursion=EXC)
    assert np.isnan(no_trans["per_sequence"][0, 17]) and gc.same_bits(no_trans["per_sequence"][0, :17], out["per_sequence"][0, :17])


def test_hand_made_signal(pipe):
    ev = pipe.gait_events(hand_signals(), window=2, min_excursion=1.0)
    print(ev.tolist())
    assert ev.dtype == np.int32 and ev.tolist() == hand_events().tolist()
    assert pipe.gait_events(hand_signals(), window=2, min_excursion=9.5).tolist() == [0] * 13       # the largest excursion is 9: -6 under 3
    assert pipe.gait_events(hand_signals()[:4], window=2).tolist() == [0] * 4                        # no frame has a whole window


def test_both_feet_strike_in_one_frame(pipe):
    """A hopper -- the walker with the right ankle 0.8 times the LEFT one's swing, in phase -- strikes with both feet in the same frames: the row holds
    the left foot's step length (positive: the left ankle is further ahead), the frame counts as a left strike, then a right one (a step of 0 s),
    and the next left strike a period later closes another step."""
    both = np.stack([HAND, HAND, HAND, HAND], axis=1)
    assert pipe.gait_events(both, window=2, min_excursion=1.0).tolist() == both_feet_events().tolist()
    joints, trans = gc.walker(T, theta=0.5, right=0.8)
    for sigma in (0.0, 2.0):
        out = pipe.gait_parameters(joints, trans=trans, fps=FPS, sigma=sigma, window=W, min_excursion=EXC)
        gc.assert_margin(out["per_frame"], [T], W, EXC)
        want = gc.expected_events(T, W, P=P)[gc.HEEL_L]
        at = np.flatnonzero(out["events"] & gc.HEEL_L)
        assert at.tolist() == want and np.flatnonzero(out["events"] & gc.HEEL_R).tolist() == want
        rows, seq = out["per_frame"], out["per_sequence"][0]
        assert gc.same_bits(rows[at, 5], rows[at, 0] - rows[at, 1]) and (rows[at, 5] > 0).all() and gc.same_bits(rows[at, 6], rows[at, 4])
        n = len(want)
        assert seq[0] == seq[1] == n and seq[4] == 2 * n - 1            # (L, R) in every frame, (R, L) between two frames
        times = [x for a, b in zip(want[:-1], want[1:]) for x in (0.0, (b - a) / FPS)] + [0.0]
        lengths = [rows[want[0], 1] - rows[want[0], 0]] + [x for t in want[1:] for x in (rows[t, 0] - rows[t, 1], rows[t, 1] - rows[t, 0])]     # second strikes: R, then L and R of each later frame
        assert abs(seq[5] - np.mean(times)) <= 1e-12 and abs(seq[11] - np.mean(lengths)) <= 1e-12
        assert seq[8] == np.cumsum([(b - a) / FPS for a, b in zip(want[:-1], want[1:])] * 2)[-1] / (2 * n - 2)


def test_floor_cases(pipe):
    joints, trans = gc.walker(64, A=0.02, theta=2.0)
    for sigma in (0.0, 2.0):
        out = pipe.gait_parameters(joints, trans=trans, fps=FPS, sigma=sigma, window=W, min_excursion=EXC)
        gc.assert_margin(out["per_frame"], [64], W, EXC)
        assert not out["events"].any() and (out["per_sequence"][0, :5] == 0).all() and np.isnan(out["per_sequence"][0, 5:]).all()
        assert np.isnan(out["per_frame"][:, 5:]).all() and np.isfinite(out["per_frame"][:, :5]).all()
    clean_j, trans = gc.walker(T, theta=0.3)
    bad_j, _ = gc.walker(T, theta=0.3, degenerate=(60,))
    for sigma, reach in ((0.0, W), (2.0, W + 8)):              # the frame itself, the Gaussian's radius int(4 sigma + 0.5), the window
        clean = pipe.gait_parameters(clean_j, trans=trans, fps=FPS, sigma=sigma, window=W, min_excursion=EXC)
        bad = pipe.gait_parameters(bad_j, trans=trans, fps=FPS, sigma=sigma, window=W, min_excursion=EXC)
        near = np.abs(np.arange(T) - 60) <= reach
        assert np.isnan(bad["per_frame"][60, :5]).all()
        assert np.array_equal(bad["events"][~near], clean["events"][~near]) and not bad["events"][near].any() and clean["events"][near].any()
        far = np.abs(np.arange(T) - 60) > reach - W
        assert gc.same_bits(bad["per_frame"][far, :5], clean["per_frame"][far, :5])


def test_sequences_do_not_see_each_other(pipe):
    for window, sigma in ((5, 0.0), (5, 2.0), (1, 2.0), (32, 0.0)):
        joints, trans, lengths, names = gc.build_call(window)
        exc = 0.005 if window == 1 else EXC
        whole = pipe.gait_parameters(joints, lengths=lengths, trans=trans, fps=FPS, sigma=sigma, window=window, min_excursion=exc)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_parameters(joints[a:a + n], trans=trans[a:a + n], fps=FPS, sigma=sigma, window=window, min_excursion=exc)
            assert np.array_equal(whole["events"][a:a + n], alone["events"]), names[q]
            assert gc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]) and gc.same_bits(whole["per_sequence"][q], alone["per_sequence"][0]), names[q]
            a += n
        counts = dict(zip(names, whole["per_sequence"][:, :4].sum(axis=1)))
        print(f"window {window} sigma {sigma:g}: events per sequence {counts}")
        assert counts["one"] == counts["two_w"] == counts["standing64"] == 0
        if window == 5:
            assert whole["events"][lengths[0] + 1 + 2 * window + window] & gc.HEEL_L      # 2 w + 1 frames hold an event on their one eligible frame
            assert counts["walk130"] >= 20 and counts["degenerate65"] >= 4


def test_bad_arguments_are_refused(pipe):
    joints, trans = gc.walker(30)
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 20, 12, 16, 14, 18, -1, 19)), "joints"), (dict(joints=(0, 1, 2)), "joints"),
                     (dict(lengths=[10, 19]), "lengths"), (dict(lengths=[30, 0]), "lengths"), (dict(fps=0.0), "fps"), (dict(fps=-20.0), "fps"), (dict(fps=nan), "fps"),
                     (dict(fps=inf), "fps"), (dict(sigma=-1.0), "sigma"), (dict(sigma=nan), "sigma"), (dict(sigma=16.5), "sigma"), (dict(window=0), "window"),
                     (dict(window=33), "window"), (dict(min_excursion=-0.01), "min_excursion"), (dict(min_excursion=inf), "min_excursion"),
                     (dict(trans=trans[:-1]), "trans")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_parameters(joints, **kw)
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_parameters(np.zeros((3, 25, 2)))
    assert pipe.gait_parameters(joints, window=32)["events"].tolist() == [0] * 30              # a window longer than the sequence is no error


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_events.h itself against the statement, one file per sequence of the calls of the device tests: with sigma = 0 every bit, with
    sigma = 2 within the bars of gait_checks.py (the program adds the Gaussian's pairs from the outside in, numpy by np.dot)."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_events_check.cpp")
    exe = str(tmp_path / "gait_events_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for window, sigma, J, table, with_trans in ((5, 0.0, 25, gc.KINECTV2, True), (5, 2.0, 25, gc.KINECTV2, True), (1, 0.0, 49, gc.OTHER49, False),
                                                (32, 2.0, 25, gc.KINECTV2, True)):
        joints, trans, lengths, names = gc.build_call(window, J=J, table=table)
        trans = trans.copy()
        trans[[8, 9, 10, 200]] = np.nan                         # the first heel strikes of the first walk have no translation
        exc = 0.005 if window == 1 else EXC
        weights = None if sigma == 0 else pipe.gauss_weights(sigma)[int(4 * sigma + 0.5):]
        a = 0
        for name, n in zip(names, lengths):
            tr = trans[a:a + n] if with_trans else None
            host = pipe.gait_parameters(joints[a:a + n], trans=tr, fps=FPS, sigma=sigma, window=window, min_excursion=exc, joints=table)
            gc.assert_margin(host["per_frame"], [n], window, exc)
            raw = pipe.gait_parameters(joints[a:a + n], fps=FPS, sigma=0.0, window=window, min_excursion=exc, joints=table)["per_frame"][:, :4]
            files.append(gc.write_case(str(tmp_path / f"w{window}_s{sigma:g}_{name}.bin"), joints[a:a + n], tr, table, FPS, sigma, window, exc, host, weights, raw))
            a += n
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]


def test_header_includes_only_the_track_header():
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_events.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "track_boxes.h"']
    assert "track_first(" in src and "hip_runtime" not in src and "__global__" not in src
