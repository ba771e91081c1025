"""Turns and straight-walking gait parameters on the host: pipeline.gait_turns, the numpy float64 statement, on the turning walker of
tests/helpers/turn_checks.py, whose turns are known analytically; a hand-made integer case whose phases, turn rows and counts are written out in
the helper; csrc/gait_turns.h, the arithmetic the kernels run, through tests/helpers/gait_turns_check.cpp: a stand-alone program (its own main, no
HIP) built with AddressSanitizer and UBSan and run directly on files this test writes; the C exports and every refusal.  Every figure is printed
before it is asserted.

The walker's wobble is 0.5 degrees with sigma 0 and 2 and 6 degrees with sigma 8: a raw wobble of 6 degrees is a rate of 35 degrees a second at the
stride's frequency, which only the wide Gaussian takes out (DESIGN 4.13 says why its default is 8 frames).  The turn lasts three strides of the
wobble, so the wobble is the same at both of its ends and the summed angle misses the analytic one by what the run leaves out below the edge rate."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import gait_checks as gc
from .helpers import turn_checks as tc

FPS, P, T = 20.0, 21.7, 400
TURNS = ((170, 65, 180.0),)                                     # one turn to the left of 180 degrees in 3.25 s, three periods of the wobble


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_turns", 21), ("grnet_op_gait_turn_runs", 17)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_turns(None, None, 25, None, 1, None, None, None, 20.0, 8.0, 5.0, 15.0, 45.0, 10, 200, 8, None, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_turn_runs(None, None, None, None, None, 1, 20.0, 5.0, 15.0, 45.0, 10, 200, 8, None, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_turns", "op_gait_turn_runs"))
    cols = pkg.pipeline.TURN_COLUMNS
    assert len(cols) == 24 and len(set(cols)) == 24 and cols[11:] == tuple("straight_" + c for c in pkg.pipeline.GAIT_COLUMNS[4:17])
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_turns.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_angles.h"']
    assert "hip_runtime" not in src and "__global__" not in src


@pytest.mark.parametrize("sigma,wobble", ((0.0, 0.5), (2.0, 0.5), (8.0, 6.0)))
def test_statement_on_the_turning_walker(pipe, sigma, wobble):
    joints, trans = tc.turning_walker(T, TURNS, theta0=0.3, wobble=(wobble, 0.4), P=P)
    gait = pipe.gait_parameters(joints, trans=trans, fps=FPS, sigma=2.0)
    out = pipe.gait_turns(joints, gait["events"], gait["per_frame"], fps=FPS, sigma=sigma)
    margin = tc.assert_margin(out["per_frame"], [T])
    row, whole = dict(zip(pipe.TURN_COLUMNS, out["per_sequence"][0])), dict(zip(pipe.GAIT_COLUMNS, gait["per_sequence"][0]))
    want = tc.expected_turns(T, TURNS, 0.3)
    found = out["turns"][0][np.isfinite(out["turns"][0, :, 0])]
    print(f"sigma {sigma:g} wobble {wobble:g}: decision margin {margin:.3g}; expected {want}, found {found.tolist()}")
    assert row["n_turns"] == len(want) == len(found) == 1 and row["n_turns_left"] == 1 and row["n_turns_right"] == 0      # every expected turn and no other
    reach = int(4 * sigma + 0.5)
    core = tc.core_window(TURNS[0], FPS, 5.0 + wobble * 2 * np.pi / P * FPS)      # where the turn alone is faster than the edge and the wobble's largest rate together
    for (first, last, direction, angle), got in zip(want, found):
        print(f"  frames {got[0]:g} .. {got[1]:g}; the window {first} .. {last}, its core {core[0]} .. {core[1]}, the Gaussian's reach {reach}")
        assert first - reach <= got[0] <= core[0] + reach and core[1] - reach <= got[1] <= last + reach      # no further out than the Gaussian reaches, no further in either
        assert got[2] == direction == 1
        print(f"  angle {got[3]:.4f} against {angle:.4f} +- {wobble:g}; peak {got[5]:.2f} deg/s, {got[4]:.2f} s, {got[6]:g} steps")
        assert abs(got[3] - angle) <= wobble
        assert got[4] == (got[1] - got[0] + 1) / FPS and np.array_equal(out["phase"][int(got[0]):int(got[1]) + 1], np.full(int(got[1] - got[0]) + 1, 1))
    assert row["turn_frames"] == np.count_nonzero(out["phase"]) and row["unknown_frames"] == 0 and row["straight_bouts"] == 2
    assert row["straight_frames"] + row["turn_frames"] == T
    print(f"  stride time straight {row['straight_stride_time_mean']:.5f} s against {P / FPS:.5f} +- {1 / FPS:.3f}; CV straight {row['straight_stride_time_cv']:.3f} % "
          f"against {whole['stride_time_cv']:.3f} % over the whole clip; speed {row['straight_speed']:.4f} against {whole['speed']:.4f} m/s")
    assert abs(row["straight_stride_time_mean"] - P / FPS) <= 1.0 / FPS
    assert row["straight_stride_time_cv"] < whole["stride_time_cv"]              # the reason for the feature
    assert whole["stride_time_cv"] >= 2.0 * row["straight_stride_time_cv"]       # the walker's slow-down is chosen for it
    assert 0 < row["straight_steps"] < whole["steps"]


def test_a_walker_without_a_turn(pipe):
    joints, trans = tc.turning_walker(130, theta0=0.7)
    same_j, _ = gc.walker(130, theta=0.7)
    assert np.array_equal(joints, same_j)                       # without a turn it is gait_checks' walker
    gait = pipe.gait_parameters(joints, trans=trans, fps=FPS, sigma=2.0)
    for sigma in (0.0, 2.0, 8.0):
        out = pipe.gait_turns(joints, gait["events"], gait["per_frame"], fps=FPS, sigma=sigma)
        row = out["per_sequence"][0]
        print(f"sigma {sigma:g}: largest |rate| {np.abs(out['per_frame'][:, 1]).max():.3g} deg/s")
        assert row[:7].tolist() == [0, 0, 0, 0, 0, 1, 130] and np.isnan(row[7:11]).all() and not out["phase"].any() and np.isnan(out["turns"]).all()
        assert gait["per_sequence"][0, 4] >= 9 and tc.same_bits(row[11:24], gait["per_sequence"][0, 4:17])       # every bit


def test_hand_made_case(pipe):
    rates, events, rows = tc.hand_case()
    for max_turns in (8, 1):
        out = pipe.gait_turn_runs(rates, events, rows, max_turns=max_turns, **tc.HAND_RULE)
        print(out["phase"].tolist(), out["turns"][0, :2].tolist(), out["per_sequence"][0].tolist())
        assert out["phase"].dtype == np.int32 and out["phase"].tolist() == tc.HAND_PHASE
        assert out["turns"].shape == (1, max_turns, 7) and out["turns"][0, :2].tolist() == tc.HAND_TURNS[:max_turns] and np.isnan(out["turns"][0, 2:]).all()
        assert out["per_sequence"][0, :11].tolist() == tc.HAND_COUNTS            # two turns counted, whatever is stored
        assert all(abs(out["per_sequence"][0, c] - v) <= 1e-12 for c, v in tc.HAND_STRAIGHT.items())
    assert tc.decision_margin(rates, 5.0, 15.0, 45.0) == 3.0    # |2 - 5|: the hand-made case decides nothing narrowly


def test_a_degenerate_frame_is_unknown_and_costs_nothing_else(pipe):
    turns = ((20, 30, 120.0),)
    clean_j, _ = tc.turning_walker(130, turns, theta0=0.3)
    bad_j, _ = tc.turning_walker(130, turns, theta0=0.3, degenerate=(90,))
    gait = pipe.gait_parameters(clean_j, fps=FPS, sigma=0.0)
    for sigma, reach in ((0.0, 0), (2.0, 8)):
        clean = pipe.gait_turns(clean_j, gait["events"], gait["per_frame"], fps=FPS, sigma=sigma)
        bad = pipe.gait_turns(bad_j, gait["events"], gait["per_frame"], fps=FPS, sigma=sigma)
        unknown = np.flatnonzero(bad["phase"] == 3)
        assert unknown.tolist() == list(range(90 - reach, 92 + reach))             # the steps into and out of the frame, as far as the Gaussian reaches
        far = np.ones(130, bool)
        far[unknown] = False
        assert np.array_equal(bad["phase"][far], clean["phase"][far]) and tc.same_bits(bad["per_frame"][far], clean["per_frame"][far])
        assert tc.same_bits(bad["turns"], clean["turns"]) and bad["per_sequence"][0, 4] == unknown.size and bad["per_sequence"][0, 5] == clean["per_sequence"][0, 5] + 1


def test_sequences_do_not_see_each_other(pipe):
    from .test_gpu_turns import LENGTHS, NAMES, call
    joints, table = call(25)
    gait = pipe.gait_parameters(joints, lengths=LENGTHS, fps=FPS, sigma=2.0)
    for sigma in (0.0, 8.0):
        whole = pipe.gait_turns(joints, gait["events"], gait["per_frame"], lengths=LENGTHS, fps=FPS, sigma=sigma)
        a = 0
        for q, n in enumerate(LENGTHS):
            alone = pipe.gait_turns(joints[a:a + n], gait["events"][a:a + n], gait["per_frame"][a:a + n], fps=FPS, sigma=sigma)
            assert np.array_equal(whole["phase"][a:a + n], alone["phase"]) and tc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]), NAMES[q]
            assert tc.same_bits(whole["turns"][q], alone["turns"][0]) and tc.same_bits(whole["per_sequence"][q], alone["per_sequence"][0]), NAMES[q]
            a += n


def test_bad_arguments_are_refused(pipe):
    joints, _ = gc.walker(30)
    ev, rows = np.zeros(30, np.int32), np.zeros((30, 7))
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(fps=0.0), "fps"),
                     (dict(fps=nan), "fps"), (dict(sigma=-1.0), "sigma"), (dict(sigma=nan), "sigma"), (dict(sigma=16.5), "sigma"), (dict(edge_rate=-1.0), "edge_rate"),
                     (dict(edge_rate=nan), "edge_rate"), (dict(edge_rate=inf), "edge_rate"), (dict(peak_rate=4.0), "peak_rate"), (dict(peak_rate=nan), "peak_rate"),
                     (dict(min_angle=-1.0), "min_angle"), (dict(min_angle=inf), "min_angle"), (dict(min_frames=0), "min_frames"), (dict(max_frames=9), "max_frames"),
                     (dict(max_turns=0), "max_turns"), (dict(max_turns=65), "max_turns"), (dict(min_frames=2.5), "whole")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_turns(joints, ev, rows, **kw)
    for args, word in (((np.zeros((3, 25, 2)), ev, rows), "joints3d"), ((joints, ev[:-1], rows), "events"), ((joints, ev, rows[:, :6]), "gait_rows")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_turns(*args)
    with pytest.raises(ValueError, match="rates"):
        pipe.gait_turn_runs(np.zeros((30, 3)), ev, rows)


def write_case(path, joints, table, events, gait_rows, rule, max_turns, host):
    """The file tests/helpers/gait_turns_check.cpp reads: ONE sequence, sigma = 0."""
    T, J = joints.shape[:2]
    with open(path, "wb") as f:
        f.write(np.array([T, J, rule["min_frames"], rule["max_frames"], max_turns], "<i4").tobytes() + np.asarray(table, "<i4").tobytes())
        f.write(np.array([rule["fps"], rule["edge_rate"], rule["peak_rate"], rule["min_angle"]], "<f8").tobytes())
        f.write(np.ascontiguousarray(joints, "<f4").tobytes() + np.ascontiguousarray(events, "<i4").tobytes() + np.ascontiguousarray(gait_rows, "<f8").tobytes())
        f.write(np.ascontiguousarray(host["per_frame"], "<f8").tobytes() + np.ascontiguousarray(host["phase"], "<i4").tobytes())
        f.write(np.ascontiguousarray(host["turns"][0], "<f8").tobytes() + np.ascontiguousarray(host["per_sequence"][0], "<f8").tobytes())
    return path


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_turns.h itself against the statement with sigma = 0, one file per sequence of the device tests' call and the walker of this file:
    every bit equal."""
    from .test_gpu_turns import LENGTHS, NAMES, call
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_turns_check.cpp")
    exe = str(tmp_path / "gait_turns_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for J, max_turns in ((25, 8), (49, 1)):
        joints, table = call(J)
        gait = pipe.gait_parameters(joints, lengths=LENGTHS, fps=FPS, sigma=2.0, joints=table)
        a = 0
        for name, n in zip(NAMES, LENGTHS):
            ev, rows = gait["events"][a:a + n], gait["per_frame"][a:a + n]
            host = pipe.gait_turns(joints[a:a + n], ev, rows, fps=FPS, sigma=0.0, max_turns=max_turns, joints=table)
            tc.assert_margin(host["per_frame"], [n])
            files.append(write_case(str(tmp_path / f"J{J}_{name}.bin"), joints[a:a + n], table, ev, rows, tc.DEFAULT_RULE, max_turns, host))
            a += n
    joints, trans = tc.turning_walker(T, TURNS, theta0=0.3, wobble=(0.5, 0.4), P=P)
    gait = pipe.gait_parameters(joints, trans=trans, fps=FPS, sigma=2.0)
    host = pipe.gait_turns(joints, gait["events"], gait["per_frame"], fps=FPS, sigma=0.0)
    files.append(write_case(str(tmp_path / "walker400.bin"), joints, gc.KINECTV2, gait["events"], gait["per_frame"], tc.DEFAULT_RULE, 8, host))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
