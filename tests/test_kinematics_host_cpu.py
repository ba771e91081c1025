"""Joint-angle kinematics per gait cycle on the host: pipeline.gait_kinematics, the numpy float64 statement, on the articulated walker of
tests/helpers/kinematics_checks.py, whose angles are known analytically and whose events are given; gait_atan2 against math.atan2; a hand-made
integer case of the cycle stage whose values are written out here by hand and by Fractions; csrc/gait_angles.h, the arithmetic the kernels run,
through tests/helpers/gait_angles_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly
on files this test writes; the C exports and every refusal.  Every figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import kinematics_checks as kc

U = 2.0 ** -53
T = 130
STRIDES_130 = {"left": [(8, 30), (30, 52), (52, 74), (74, 95), (95, 117)], "right": [(19, 41), (41, 63), (63, 84), (84, 106), (106, 128)]}


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def test_exports_and_refusals(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_kinematics", 14), ("grnet_op_gait_cycles", 10)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    for kw in (dict(), dict(J=0), dict(n_seq=0), dict(n_seq=8193), dict(sigma=-1.0), dict(sigma=16.5), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(lo=0),
               dict(lo=9, hi=8), dict(hi=4097)):
        a = dict(J=25, n_seq=1, sigma=2.0, lo=8, hi=60)
        a.update(kw)
        assert lib.grnet_gait_kinematics(None, None, a["J"], None, a["n_seq"], None, None, a["sigma"], a["lo"], a["hi"], None, None, None, None) == pkg._lib.EINVAL
        assert lib.grnet_op_gait_cycles(None, None, None, None, a["n_seq"], a["lo"], a["hi"], None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_kinematics", "op_gait_cycles"))
    p = pkg.pipeline
    assert p.KINEMATICS_JOINTS_KINECTV2 == kc.KINECTV2 == (0, 20, 12, 16, 13, 17, 14, 18, 15, 19, 4, 8, 5, 9, 6, 10)
    assert len(p.KINEMATICS_CHANNELS) == 13 == len(set(p.KINEMATICS_CHANNELS)) and p.KINEMATICS_CHANNELS[4] == "knee_flexion_left" and p.KINEMATICS_CHANNELS[12] == "trunk_inclination"
    assert p.KINEMATICS_COLUMNS == ("strides", "max_mean", "min_mean", "rom_mean", "rom_sd", "symmetry_index")
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_kinematics(" in header and "int grnet_op_gait_cycles(" in header


def atan_arguments():
    """A seeded grid: all octants, near the axes and the diagonals, huge and tiny ratios, exact axes."""
    rng = np.random.default_rng(412)
    ang = rng.uniform(-np.pi, np.pi, 20000)
    r = 10.0 ** rng.uniform(-3, 3, ang.size)
    y, x = [r * np.sin(ang)], [r * np.cos(ang)]
    for centre in np.arange(-4, 5) * (np.pi / 4):              # the axes and the diagonals, from 1e-17 to 1e-2 radians off them
        off = 10.0 ** rng.uniform(-17, -2, 1500) * rng.choice([-1.0, 1.0], 1500)
        y.append(np.sin(centre + off))
        x.append(np.cos(centre + off))
    big, small = 10.0 ** rng.uniform(100, 300, 2000), 10.0 ** rng.uniform(-300, -100, 2000)
    sg = rng.choice([-1.0, 1.0], (4, 2000))
    y += [sg[0] * big, sg[1] * small, sg[0] * small, sg[2] * big]
    x += [sg[2] * small, sg[3] * big, sg[1] * small * 3.0, sg[3] * big * 0.7]
    y += [np.array([0.0, 0.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, -0.0, 5e-324])]
    x += [np.array([1.0, -1.0, 0.0, 0.0, 1.0, 1.0, -1.0, -1.0, 2.0, 5e-324])]
    return np.concatenate(y), np.concatenate(x)


def test_gait_atan2(pipe):
    y, x = atan_arguments()
    got = pipe.gait_atan2(y, x)
    want = np.array([math.atan2(a, b) for a, b in zip(y, x)])
    err = np.abs(got - want)
    worst = float(err.max()) / (U * math.pi)
    i = int(err.argmax())
    print(f"gait_atan2 against math.atan2 over {y.size} arguments: worst error {worst:.3f} u pi at ({y[i]!r}, {x[i]!r})")
    assert np.isfinite(got).all() and worst <= 4.0
    assert float(pipe.gait_atan2(0.0, 1.0)) == 0.0 and float(pipe.gait_atan2(0.0, -1.0)) == math.pi and float(pipe.gait_atan2(1.0, 0.0)) == math.pi / 2
    nan, inf = float("nan"), float("inf")
    for a, b in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, -inf), (inf, inf)):
        assert np.isnan(pipe.gait_atan2(a, b)), (a, b)
    assert pipe.gait_atan2(np.ones((2, 3)), np.ones(3)).shape == (2, 3)


@pytest.mark.parametrize("sigma", (0.0, 2.0))
@pytest.mark.parametrize("theta", (0.0, np.deg2rad(40.0), np.pi))
def test_statement_on_the_walker(pipe, theta, sigma):
    joints, ang, events = kc.walker(T, theta=theta, arm_right=0.6)
    out = pipe.gait_kinematics(joints, events, sigma=sigma)
    bars = kc.analytic_bars(joints)
    want = ang if sigma == 0 else np.stack([kc.gauss64(ang[:, c], sigma) for c in range(13)], axis=1)
    extra = 0.0 if sigma == 0 else 2 * kc.tk.gauss_bar(ang, sigma)     # each side's Gaussian rounds
    err = np.abs(out["per_frame"] - want).max(axis=0)
    for c, name in enumerate(pipe.KINEMATICS_CHANNELS):
        print(f"theta {theta:.3f} sigma {sigma:g} {name}: error {err[c]:.3g} deg against the derived {bars[c] + extra:.3g} deg")
    assert (err <= bars + extra).all()
    # the strides: exactly the walker's, none skipped
    hl, hr = kc.heel_strikes(T)
    assert list(zip(hl[:-1], hl[1:])) == STRIDES_130["left"] and list(zip(hr[:-1], hr[1:])) == STRIDES_130["right"]
    rows = out["per_sequence"][0]
    print(f"  strides used per channel {rows[:, 0].astype(int).tolist()}")
    assert rows[:, 0].tolist() == [5.0] * 13
    # range of motion against the analytic excursion over the same frames; the mean curve at 0 % is the mean over the opening strikes
    for c in range(13):
        strides = STRIDES_130["right" if c < 12 and c & 1 else "left"]
        rom = np.mean([want[a:b + 1, c].max() - want[a:b + 1, c].min() for a, b in strides])
        print(f"  {pipe.KINEMATICS_CHANNELS[c]}: ROM {rows[c, 3]:.4f} against {rom:.4f} deg, SD {rows[c, 4]:.4f}, symmetry {rows[c, 5]:.3f}")
        assert abs(rows[c, 3] - rom) <= 2 * (bars[c] + extra) + 1e-9
        assert abs(out["curves"][0, c, 0, 0] - np.mean([want[a, c] for a, _ in strides])) <= bars[c] + extra + 1e-9
        assert abs(out["curves"][0, c, 100, 0] - np.mean([want[b, c] for _, b in strides])) <= bars[c] + extra + 1e-9
    # the right arm swings 0.6 of the left one's: 100 |1 - 0.6| / 0.8 = 50, to what a sampled maximum allows; the legs are symmetric
    assert abs(rows[8, 5] - 50.0) <= 3.0 and rows[8, 5] == rows[9, 5] and rows[4, 5] == rows[5, 5] <= 3.0 and np.isnan(rows[12, 5])


def fraction_cycles(x, ev, lo, hi):
    """Rules 5 to 7 in exact rational arithmetic on integer angles: {channel: (n, points (101) mean, SD^2, max mean, min mean, ROM mean, ROM SD^2)}."""
    out = {}
    for c in range(13):
        hs = [t for t in range(len(ev)) if ev[t] & (kc.HEEL_R if c < 12 and c & 1 else kc.HEEL_L)]
        used = [(a, b - a) for a, b in zip(hs[:-1], hs[1:]) if lo <= b - a <= hi and all(math.isfinite(v) for v in x[a:b + 1, c])]
        n = len(used)
        if not n:
            out[c] = (0,)
            continue
        col = [Fraction(int(v)) if math.isfinite(v) else None for v in x[:, c]]
        pts = []
        for t0, L in used:
            pts.append([col[t0 + p * L // 100] + ((col[t0 + p * L // 100 + 1] - col[t0 + p * L // 100]) * Fraction(p * L % 100, 100) if p * L % 100 else 0) for p in range(101)])
        mean = [sum(s[p] for s in pts) / n for p in range(101)]
        var = [sum((s[p] - mean[p]) ** 2 for s in pts) / n for p in range(101)]
        top = [max(col[t0:t0 + L + 1]) for t0, L in used]
        low = [min(col[t0:t0 + L + 1]) for t0, L in used]
        rom = [a - b for a, b in zip(top, low)]
        m = sum(rom) / n
        out[c] = (n, mean, var, sum(top) / n, sum(low) / n, m, sum((r - m) ** 2 for r in rom) / n)
    return out


def check_hand_case(result):
    """The hand-made case against what is written out by hand (channel 12, the ramp) and by Fractions (every channel): every value passes fewer than
    eight roundings of numbers below 2 M, so the bar is 16 u M with M = 80, the largest value."""
    x, ev, lo, hi = kc.hand_case()
    curves, rows = result["curves"][0], result["per_sequence"][0]
    print(f"strides used per channel {rows[:, 0].astype(int).tolist()}")
    assert rows[:, 0].tolist() == [3, 2, 3, 2, 2, 2, 3, 2, 3, 2, 3, 2, 3]      # the left foot's 3, the right foot's 2; channel 4 loses the stride with its NaN
    bar = 16 * U * 80
    # channel 12 = t on the strides [0, 10], [10, 30], [65, 75]: point p = (p / 10 + 10 + p / 5 + 65 + p / 10) / 3 = 25 + 2 p / 15
    p = np.arange(101)
    assert np.abs(curves[12, :, 0] - (25 + 2 * p / 15)).max() <= bar
    sd = np.sqrt(((p / 10 - 25 - 2 * p / 15) ** 2 + (10 + p / 5 - 25 - 2 * p / 15) ** 2 + (65 + p / 10 - 25 - 2 * p / 15) ** 2) / 3)
    assert np.abs(curves[12, :, 1] - sd).max() <= bar
    assert curves[12, 0, 0] == 25.0 and curves[12, 100, 0] == 115 / 3                          # whole frames: the mean of 0, 10, 65 and of 10, 30, 75
    assert abs(rows[12, 1] - 115 / 3) <= bar and rows[12, 2] == 25.0 and abs(rows[12, 3] - 40 / 3) <= bar and abs(rows[12, 4] - math.sqrt(200 / 9)) <= bar
    assert np.isnan(rows[12, 5])
    want = fraction_cycles(x, ev, lo, hi)
    worst = 0.0
    for c in range(13):
        n, mean, var, top, low, rom, rom_var = want[c]
        got = np.concatenate([curves[c, :, 0], curves[c, :, 1], rows[c, 1:5]])
        ref = np.array([float(v) for v in mean] + [math.sqrt(v) for v in var] + [float(top), float(low), float(rom), math.sqrt(rom_var)])
        worst = max(worst, float(np.abs(got - ref).max()))
        whole = [q for q in range(101) if all(q * L % 100 == 0 for L in (10, 20))]              # every tenth point falls on a frame in every stride
        assert all(curves[c, q, 0] == float(mean[q] * n) / n for q in whole)                    # a sum of integers is exact: one quotient
    print(f"the hand-made case against Fractions: worst difference {worst:.3g} against the bar {bar:.3g}")
    assert worst <= bar
    for c in range(0, 12, 2):
        L, R = want[c][5], want[c + 1][5]
        si = float(100 * abs(L - R) / ((L + R) / 2))
        assert abs(rows[c, 5] - si) <= 64 * U * max(si, 1.0) + 100 * 4 * bar / float((L + R) / 2) and same(rows[c, 5], rows[c + 1, 5])


def same(a, b):
    return kc.same_bits(np.asarray(a), np.asarray(b))


def test_hand_made_cycles(pipe):
    x, ev, lo, hi = kc.hand_case()
    check_hand_case(pipe.gait_cycles(x, ev, min_stride=lo, max_stride=hi))
    # nothing used: counts 0, NaN everywhere else
    none = pipe.gait_cycles(x, ev, min_stride=31, max_stride=40)
    assert (none["per_sequence"][0, :, 0] == 0).all() and np.isnan(none["per_sequence"][0, :, 1:]).all() and np.isnan(none["curves"]).all()
    only30 = pipe.gait_cycles(x, ev, min_stride=30, max_stride=30)
    assert only30["per_sequence"][0, :, 0].tolist() == [1, 0] * 6 + [1] and only30["curves"][0, 12, 50, 0] == 50.0 and only30["per_sequence"][0, 12, 4] == 0.0


def test_sequences_do_not_see_each_other(pipe):
    for sigma in (0.0, 2.0):
        joints, events, lengths, names = kc.build_call()
        whole = pipe.gait_kinematics(joints, events, lengths=lengths, sigma=sigma)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_kinematics(joints[a:a + n], events[a:a + n], sigma=sigma)
            assert all(same(whole[k][q], alone[k][0]) for k in ("curves", "per_sequence")) and same(whole["per_frame"][a:a + n], alone["per_frame"]), names[q]
            a += n
        used = dict(zip(names, whole["per_sequence"][:, :, 0].astype(int).tolist()))
        print(f"sigma {sigma:g}: strides used per sequence and channel {used}")
        assert used["one"] == used["min"] == used["standing64"] == [0] * 13
        assert used["min_1"] == [1, 0] * 6 + [1]               # one stride of exactly min_stride frames, of the left foot
        assert used["no_right130"][1::2] == [0] * 6 and min(used["no_right130"][0::2]) >= 4 and np.isnan(whole["per_sequence"][6, :, 5]).all()
        lost, kept = used["degenerate65"], used["walk130"]
        assert all(lost[c] == 1 for c in kc.AXIS_CHANNELS) and all(lost[c] == 2 for c in kc.FREE_CHANNELS), lost     # the degenerate frame costs the axis channels a stride
        assert kept == [5] * 13
        assert np.isnan(whole["curves"][4]).all() and np.isnan(whole["per_sequence"][4, :, 1:]).all()


def test_bad_arguments_are_refused(pipe):
    joints, _, events = kc.walker(30)
    nan = float("nan")
    for kw, word in ((dict(joints=kc.KINECTV2[:15] + (25,)), "joints"), (dict(joints=(-1,) + kc.KINECTV2[1:]), "joints"), (dict(joints=(0, 1, 2)), "joints"),
                     (dict(lengths=[10, 19]), "lengths"), (dict(lengths=[30, 0]), "lengths"), (dict(sigma=-1.0), "sigma"), (dict(sigma=nan), "sigma"),
                     (dict(sigma=16.5), "sigma"), (dict(min_stride=0), "min_stride"), (dict(min_stride=9, max_stride=8), "max_stride"), (dict(max_stride=4097), "max_stride"),
                     (dict(min_stride=8.5), "whole")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_kinematics(joints, events, **kw)
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_kinematics(np.zeros((3, 25, 2)), events[:3])
    with pytest.raises(ValueError, match="events"):
        pipe.gait_kinematics(joints, events[:-1])
    with pytest.raises(ValueError, match="angles"):
        pipe.gait_cycles(np.zeros((4, 12)), np.zeros(4, np.int32))


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_angles.h itself against the statement with sigma = 0, one file per sequence of the calls of the device tests, the hand-made case and
    the arctangent's arguments: every bit."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_angles_check.cpp")
    exe = str(tmp_path / "gait_angles_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for J, table, lo, hi in ((25, kc.KINECTV2, 8, 60), (49, kc.OTHER49, 22, 22)):
        joints, events, lengths, names = kc.build_call(J=J, table=table)
        a = 0
        for name, n in zip(names, lengths):
            host = pipe.gait_kinematics(joints[a:a + n], events[a:a + n], sigma=0.0, min_stride=lo, max_stride=hi, joints=table)
            files.append(kc.write_case(str(tmp_path / f"j{J}_{name}.bin"), 0, lo, hi, host, joints=joints[a:a + n], table=table, events=events[a:a + n]))
            a += n
    x, ev, lo, hi = kc.hand_case()
    files.append(kc.write_case(str(tmp_path / "hand.bin"), 2, lo, hi, pipe.gait_cycles(x, ev, min_stride=lo, max_stride=hi), angles=x, events=ev))
    y, xx = atan_arguments()
    y, xx = np.concatenate([y, [0.0, np.nan, np.inf]]), np.concatenate([xx, [0.0, 1.0, 1.0]])
    files.append(kc.write_atan_case(str(tmp_path / "atan.bin"), y, xx, pipe.gait_atan2(y, xx)))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]


def test_header_includes_only_the_gait_header():
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_angles.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_events.h"']
    assert "hip_runtime" not in src and "__global__" not in src
    body = src.split("#pragma once")[1]
    assert not any(word in body for word in ("__builtin_atan", "std::", "sin(", "cos(", "exp(", "tan("))      # + - * / and sqrt alone
