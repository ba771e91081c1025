"""Foot contact phases and double support on the host: pipeline.gait_contacts, the numpy float64 statement, on the planted-foot walker
of tests/helpers/contact_checks.py, whose double-support and step times are known analytically; a hand-made integer case whose phases, run rows and
row are written out in the helper; the fixed-tree sum against math.fsum and against loops; csrc/gait_contacts.h, the arithmetic the kernels run,
through tests/helpers/gait_contacts_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on
files this test writes; every refusal.  Every figure is printed before it is asserted.

The bars of the walker tests are the issue's: a numpy prototype of the rule recovered the double-support time to 0.38 frames in the mean and 0.54
for a single run, the step time to 0.17 frames and the mean inter-foot speed to 4.7 %, on these inputs without smoothing; the bars are those with a
margin of about 1.4.  What the statement reaches is in profiles/gait_contacts_bounds.txt."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import contact_checks as cc
from .helpers import gait_checks as gc

FPS, T = cc.FPS, 400
PHASES = (0.0, 0.21, 0.43, 0.62, 0.84)                          # phi as a share of the cycle


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def walk(pipe, P, beta, speed, phi, theta, **kw):
    joints = cc.planted_walker(T, P, beta, speed, phi * P, theta)
    gait = pipe.gait_parameters(joints, fps=FPS, sigma=0.0)
    return joints, gait, pipe.gait_contacts(joints, gait["events"], fps=FPS, **kw)


@pytest.mark.parametrize("P,beta,speed", cc.WALKERS)
def test_statement_on_the_planted_walker(pipe, P, beta, speed):
    want = (beta - 0.5) * P
    worst = dict(single=0.0, mean=0.0, step=0.0, speed=0.0, stance=0.0)
    for phi in PHASES:
        for theta in cc.YAWS:
            _, gait, out = walk(pipe, P, beta, speed, phi, theta)
            row = dict(zip(pipe.CONTACT_COLUMNS, out["per_sequence"][0]))
            runs = out["runs"][0][:int(row["static_runs"])]
            strikes = np.flatnonzero(gait["events"] & 3)
            between = runs[np.isfinite(runs[:, 0]) & (runs[:, 0] >= strikes[0]) & (runs[:, 1] <= strikes[-1])]
            assert (between[:, 2] != 0).all(), f"P {P} phi {phi} yaw {theta:.2f}: an unattributed run between the first and the last heel strike: {between}"
            assert (between[1:, 2] == -between[:-1, 2]).all(), "the runs do not alternate"
            assert abs(row["static_runs"] - 2 * T / P) <= 2, f"{row['static_runs']} runs against {2 * T / P:.1f}"
            led = runs[runs[:, 2] != 0]
            frames = (led[:, 1] - led[:, 0])
            assert np.array_equal(frames / FPS, led[:, 4])
            worst["single"] = max(worst["single"], float(np.abs(frames - want).max()))
            worst["mean"] = max(worst["mean"], abs(row["double_support_time_mean"] * FPS - want))
            worst["step"] = max(worst["step"], float(np.abs(np.diff(between[:, 0]) - P / 2).max()))
            worst["speed"] = max(worst["speed"], abs(row["interfoot_speed_mean"] / (2 * speed) - 1))
            worst["stance"] = max(worst["stance"], abs(row["stance_share_mean"] - 100 * beta))
            assert row["strides"] >= 2 * (T / P - 3) and abs(row["stride_time_mean"] * FPS - P) <= 0.25
            assert abs(row["single_support_time_mean"] * FPS - (1 - beta) * P) <= 0.75 and abs(row["swing_time_mean"] + row["stance_time_mean"] - row["stride_time_mean"]) < 1e-12
    print(f"P {P} beta {beta} speed {speed}: double support {want:.3f} frames: worst single run off by {worst['single']:.3f} (bar 0.75), worst mean {worst['mean']:.3f} (0.5); "
          f"step time off by {worst['step']:.3f} (0.25); mean inter-foot speed off by {100 * worst['speed']:.2f} % (8); stance share off by {worst['stance']:.3f} "
          f"({100 / P:.3f})")
    assert worst["single"] <= 0.75 and worst["mean"] <= 0.5 and worst["step"] <= 0.25 and worst["speed"] <= 0.08 and worst["stance"] <= 100 * 1.0 / P


def test_smoothing_shortens_the_runs(pipe):
    P, beta, speed = cc.WALKERS[0]
    means = []
    for sigma in (0.0, 1.0, 2.0):
        _, _, out = walk(pipe, P, beta, speed, 0.21, 0.0, sigma=sigma)
        means.append(out["per_sequence"][0, 6] * FPS)
    print(f"double-support time {(beta - 0.5) * P:.2f} frames: found {means[0]:.2f}, {means[1]:.2f} with sigma 1, {means[2]:.2f} with sigma 2")
    assert means[0] > means[1] > means[2] > 0                   # why the default is no smoothing


def test_hand_made_case(pipe):
    speeds, events = cc.hand_case()
    for max_runs in (128, 2):
        out = pipe.gait_contact_runs(speeds, events, max_runs=max_runs, **cc.HAND_RULE)
        print(out["phase"].tolist(), out["runs"][0, :6].tolist(), out["per_sequence"][0].tolist())
        assert out["phase"].dtype == np.int32 and out["phase"].tolist() == cc.HAND_PHASE
        keep = min(max_runs, 6)
        assert out["runs"].shape == (1, max_runs, 6) and cc.same_bits(out["runs"][0, :keep], cc.HAND_RUNS[:keep]) and np.isnan(out["runs"][0, keep:]).all()
        assert cc.same_bits(out["per_sequence"][0], cc.HAND_ROW)                  # six runs counted, whatever is stored
    assert cc.decision_margin(speeds[:-1], 5.0) == 2.0
    shifted = np.concatenate([speeds, speeds])                  # two sequences: the second one's first run is open again, the entry between them is not read
    both = pipe.gait_contact_runs(shifted, np.concatenate([events, events]), lengths=[22, 22], **cc.HAND_RULE)
    assert both["phase"].tolist() == cc.HAND_PHASE * 2 and cc.same_bits(both["per_sequence"], [cc.HAND_ROW] * 2)
    rel = pipe.gait_contact_runs(speeds, events, fps=20.0, fraction=0.5, reach=1, max_frames=3)        # the relative threshold, half of 4.8: the 3s move
    moving = [0 if k in (6, 14) else p for k, p in enumerate(cc.HAND_PHASE)]
    assert rel["per_sequence"][0, 0] == 0.5 * 4.8 and rel["per_sequence"][0, 2:6].tolist() == [5, 0, 0, 5] and rel["phase"].tolist() == moving


def test_fixed_tree_sum(pipe):
    rng = np.random.default_rng(14)
    x = rng.uniform(0.0, 3.0, 130)
    S, n = pipe.contact_tree_sum(x)
    exact = math.fsum(x)
    print(f"130 intervals: tree sum off by {abs(S - exact):.3g}, bar {130 * cc.U * x.max():.3g}")
    assert n == 130 and abs(S - exact) <= 130 * cc.U * x.max()
    assert (S, n) == cc.tree_sum(x)                             # every bit: floats compare by value, and neither is NaN
    x[[3, 64, 129]] = [np.nan, np.inf, -np.inf]
    assert pipe.contact_tree_sum(x) == cc.tree_sum(x) and pipe.contact_tree_sum(x)[1] == 127
    for size in (0, 1, 63, 64, 65, 128):
        assert pipe.contact_tree_sum(x[:size]) == cc.tree_sum(x[:size])
    out = pipe.gait_contact_runs(np.append(x, 0.0), np.zeros(131, np.int32))
    assert out["per_sequence"][0, 1] == cc.tree_sum(x)[0] / 127 and out["per_sequence"][0, 0] == 0.25 * (cc.tree_sum(x)[0] / 127)


def test_standing_nan_and_short_sequences(pipe):
    still = cc.planted_walker(64, still=True)
    out = pipe.gait_contacts(still, np.zeros(64, np.int32), fps=FPS, speed=0.05)
    assert out["phase"].tolist() == [3] * 63 + [4] and out["per_sequence"][0, 2:6].tolist() == [1, 0, 0, 1] and np.isnan(out["per_sequence"][0, 6:11]).all()
    assert np.isnan(out["runs"][0, 0, [0, 1, 3, 4]]).all() and out["runs"][0, 0, 2] == 0 and out["runs"][0, 0, 5] == 0       # one open run
    rel = pipe.gait_contacts(still, np.zeros(64, np.int32), fps=FPS)                # mean 0: nothing is below a quarter of it
    assert rel["per_sequence"][0, :3].tolist() == [0, 0, 0] and not rel["phase"][:-1].any()
    for n in (1, 2, 3):
        short = pipe.gait_contacts(cc.planted_walker(n), np.zeros(n, np.int32), fps=FPS)
        assert short["phase"][-1] == 4 and short["per_sequence"][0, 3:5].tolist() == [0, 0] and np.isnan(short["per_sequence"][0, 6:11]).all()
        assert np.isnan(short["runs"][0, :, [0, 1, 3, 4]]).all()                  # three frames hold no closed run
    assert np.isnan(pipe.gait_contacts(cc.planted_walker(1), [0], fps=FPS)["per_sequence"][0, :2]).all()          # no interval: a NaN threshold
    P, beta, speed = cc.WALKERS[0]
    clean = cc.planted_walker(130, P, beta, speed, 3.0)
    gait = pipe.gait_parameters(clean, fps=FPS, sigma=0.0)
    a = pipe.gait_contacts(clean, gait["events"], fps=FPS, speed=0.6)
    closed_a = a["runs"][0][np.isfinite(a["runs"][0, :, 0])]
    f = int(np.ceil(closed_a[5, 0]))                            # a frame inside the sixth double support: the intervals f - 1 and f lose their speed
    b = pipe.gait_contacts(cc.planted_walker(130, P, beta, speed, 3.0, nan_frames=(f,)), gait["events"], fps=FPS, speed=0.6)
    assert np.flatnonzero(b["phase"] == 4).tolist() == [f - 1, f, 129]
    lost = [r for r in closed_a if r[0] < f + 1.5 and r[1] > f - 1.5]             # the runs that hold one of the two intervals or end beside one
    kept = [r for r in closed_a if not (r[0] < f + 1.5 and r[1] > f - 1.5)]
    closed_b = b["runs"][0][np.isfinite(b["runs"][0, :, 0])]
    print(f"a NaN ankle in frame {f}: {len(lost)} of {len(closed_a)} closed runs touch it, {len(closed_b)} closed runs are left")
    assert len(lost) == 1 and len(closed_b) == len(kept) and cc.same_bits(closed_b, kept)       # it loses only the runs that touch it


def test_sequences_do_not_see_each_other(pipe):
    from .test_gpu_contacts import call
    joints, table, lengths, names = call(25)
    gait = pipe.gait_parameters(joints, lengths=lengths, fps=FPS, sigma=0.0)
    for sigma in (0.0, 1.0):
        whole = pipe.gait_contacts(joints, gait["events"], lengths=lengths, fps=FPS, sigma=sigma)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_contacts(joints[a:a + n], gait["events"][a:a + n], fps=FPS, sigma=sigma)
            assert np.array_equal(whole["phase"][a:a + n], alone["phase"]) and cc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]), names[q]
            assert cc.same_bits(whole["runs"][q], alone["runs"][0]) and cc.same_bits(whole["per_sequence"][q], alone["per_sequence"][0]), names[q]
            a += n


def test_bad_arguments_are_refused(pipe):
    joints = cc.planted_walker(30)
    ev = np.zeros(30, np.int32)
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(fps=0.0), "fps"),
                     (dict(fps=nan), "fps"), (dict(sigma=-1.0), "sigma"), (dict(sigma=nan), "sigma"), (dict(sigma=16.5), "sigma"), (dict(fraction=-0.1), "fraction"),
                     (dict(fraction=nan), "fraction"), (dict(speed=-1.0), "speed"), (dict(speed=inf), "speed"), (dict(fraction=0.0), "both zero"), (dict(reach=-1), "reach"),
                     (dict(reach=9), "reach"), (dict(max_frames=0), "max_frames"), (dict(max_runs=0), "max_runs"), (dict(max_runs=513), "max_runs"), (dict(reach=1.5), "whole")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_contacts(joints, ev, **kw)
    for args, word in (((np.zeros((3, 25, 2)), ev), "joints3d"), ((joints, ev[:-1]), "events")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_contacts(*args)
    with pytest.raises(ValueError, match="speeds"):
        pipe.gait_contact_runs(np.zeros((30, 2)), ev)


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_contacts.h itself against the statement with sigma = 0: one file per sequence of the device tests' call, with both tables and with a
    table of two rows, the walker of this file, and the hand-made signal through the hook's path.  Every bit equal."""
    from .test_gpu_contacts import call
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_contacts_check.cpp")
    exe = str(tmp_path / "gait_contacts_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    rule = dict(fps=FPS, fraction=0.25, speed=0.0, reach=2, max_frames=20)
    for J, max_runs in ((25, 128), (49, 2)):
        joints, table, lengths, names = call(J)
        gait = pipe.gait_parameters(joints, lengths=lengths, fps=FPS, sigma=0.0, joints=table)
        a = 0
        for name, n in zip(names, lengths):
            ev = gait["events"][a:a + n]
            host = pipe.gait_contacts(joints[a:a + n], ev, fps=FPS, max_runs=max_runs, joints=table)
            files.append(cc.write_case(str(tmp_path / f"J{J}_{name}.bin"), joints[a:a + n], table, None, ev, rule, max_runs, host))
            a += n
    P, beta, speed = cc.WALKERS[1]
    joints, gait, host = walk(pipe, P, beta, speed, 0.43, cc.YAWS[1])
    files.append(cc.write_case(str(tmp_path / "walker400.bin"), joints, gc.KINECTV2, None, gait["events"], rule, 128, host))
    speeds, events = cc.hand_case()
    for max_runs in (128, 2):
        host = pipe.gait_contact_runs(speeds, events, max_runs=max_runs, **cc.HAND_RULE)
        files.append(cc.write_case(str(tmp_path / f"hand{max_runs}.bin"), None, gc.KINECTV2, speeds, events, cc.HAND_RULE, max_runs, host))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
