"""Footprints, centre of mass and margin of stability on the host: pipeline.gait_balance, the numpy float64 statement, against the
plain-loop restatement of tests/helpers/balance_checks.py and against csrc/gait_balance.h, the arithmetic the kernels run, through
tests/helpers/gait_balance_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on files
this test writes.  All three agree IN EVERY BIT on every case.  Then the hand-made case whose numbers are written out in the helper, the closed forms
on the clean planted-foot walker within bars derived from the float32 rounding of the joints, the faults compare must catch, and every refusal.
Every figure is printed before it is asserted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import balance_checks as bc
from .helpers import contact_checks as cc
from .helpers import gait_checks as gc

FPS, T = bc.FPS, 400


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


@pytest.fixture(scope="module")
def walkers(pipe):
    """[(name, joints, parameters, events, the statement's result with the one-segment table)] of the twelve clean walkers, computed once."""
    made = []
    for name, joints, par in bc.walker_cases(T):
        events = pipe.gait_parameters(joints, fps=FPS)["events"]
        made.append((name, joints, par, events, pipe.gait_balance(joints, events, fps=FPS, segments=bc.ONE_SEGMENT)))
    return made


def device_cases(pipe):
    """[(name, joints, events, lengths, keywords)] of the GPU tests' calls."""
    from . import test_gpu_balance as g
    cases = []
    for name, (joints, lengths) in (("a", g.case_a()), ("b", g.case_b()), ("c", g.case_c())):
        events = g.statement(PKG_NAME, name)[0]
        cases.append((name, joints, events, lengths, {}))
    joints, lengths = g.case_b()
    cases.append(("e", joints, cases[1][2], lengths, dict(max_steps=4)))
    cases.append(("f", joints, cases[1][2], lengths, dict(segments=bc.ONE_SEGMENT)))
    joints, events = g.case_d()
    cases.append(("d", joints, events, [6000], dict(max_steps=1024)))
    return cases


def test_statement_equals_the_loops(pipe, walkers):
    for name, joints, _, events, host in walkers:
        bc.compare(host, bc.loops_balance(joints, events), name + ": ")
    for name, joints, events, lengths, kw in device_cases(pipe):
        host = pipe.gait_balance(joints, events, lengths=lengths, fps=FPS, **kw)
        loops = bc.loops_balance(joints, events, lengths, **{"segments": pipe.BALANCE_SEGMENTS_KINECTV2, **kw})
        bc.compare(host, loops, f"case {name}: ")
        print(f"case {name}: {int(host['per_sequence'][:, 1].sum())} steps in {int(host['per_sequence'][:, 2].sum())} chains: equal bits")
    rel, events, _ = bc.hand_case()
    for max_steps in (8, 2):
        bc.compare(pipe.gait_balance_steps(rel, events, max_steps=max_steps, **bc.HAND_RULE), bc.loops_steps(rel, events, max_steps=max_steps, **bc.HAND_RULE), "hand: ")


def test_hand_made_case(pipe):
    rel, events, frame = bc.hand_case()
    for max_steps in (8, 2):
        out = pipe.gait_balance_steps(rel, events, max_steps=max_steps, **bc.HAND_RULE)
        print(out["steps"][0, :5].tolist(), out["per_sequence"][0].tolist())
        keep = min(max_steps, 5)
        assert out["steps"].shape == (1, max_steps, 15) and bc.same_bits(out["steps"][0, :keep], bc.HAND_STEPS[:keep]) and np.isnan(out["steps"][0, keep:]).all()
        assert bc.same_bits(out["per_sequence"][0], bc.HAND_ROW)                  # five steps counted, whatever is stored
        assert bc.same_bits(out["per_frame"], frame)
    both = pipe.gait_balance_steps(np.concatenate([rel, rel]), np.concatenate([events, events]), lengths=[32, 32], max_steps=8, **bc.HAND_RULE)
    assert bc.same_bits(both["per_sequence"], [bc.HAND_ROW] * 2) and bc.same_bits(both["per_frame"], np.concatenate([frame, frame]))
    assert len(pipe.BALANCE_FRAME_COLUMNS) == 8 and len(pipe.BALANCE_STEP_COLUMNS) == 15 and len(pipe.BALANCE_COLUMNS) == 24


def test_closed_forms_on_the_clean_walker(pipe, walkers):
    """COM speed = v fps, MoS_ML = 0.09, stride length = v P, lateral and vertical excursion = 0, each within the helper's bar; and the condition that
    keeps the comparison honest: ONE chain and at least floor(2 T / P) - 3 steps."""
    for name, joints, (P, beta, speed, phi, theta), events, host in walkers:
        row = host["per_sequence"][0]
        n = int(row[1])
        steps = host["steps"][0, :n]
        assert row[2] == 1 and n >= int(2 * T / P) - 3, f"{name}: {n} steps in {int(row[2])} chains"
        bars = bc.closed_form_bars(P, beta, speed, n_steps=n)
        strides = steps[1:]
        lifts = np.array([bc.stance_lift(s[0], -s[2], P, beta, speed, phi) for s in steps])
        vertical_bar = bars["vertical"] + lifts[:-1] + lifts[1:]
        miss = {"com_speed": np.abs(steps[:, 10] - speed).max(), "mos_ml": np.abs(steps[:, 12] - 0.09).max(),
                "stride_length": np.abs(strides[:, 7] - speed / FPS * P).max(), "lateral": np.abs(strides[:, 14]).max()}
        print(f"{name}: {n} steps; " + ", ".join(f"{k} off by {v:.3g} (bar {bars[k]:.3g})" for k, v in miss.items()) +
              f"; vertical excursion at most {strides[:, 13].max():.3g} where the stance ankles are lifted by up to {lifts.max():.3g} at their strikes, "
              f"{(strides[:, 13] / vertical_bar).max():.3g} of its bar; {np.count_nonzero(lifts == 0)} of {n} strikes fall on a planted foot")
        assert all(miss[k] <= bars[k] for k in miss), name
        assert (strides[:, 13] <= vertical_bar).all(), name
        planted = (lifts[:-1] == 0) & (lifts[1:] == 0)          # strides whose two strikes fall on planted feet: the bar of the float32 rounding alone
        assert planted.any() and (strides[planted, 13] <= bars["vertical"]).all(), f"{name}: {np.count_nonzero(planted)} strides on planted feet"
        assert np.isfinite(strides[:, 7:10]).all() and np.isnan(steps[0, 7:10]).all() and np.isnan(steps[0, 13:15]).all()
        assert abs(row[11] - speed) <= bars["com_speed"] and abs(row[16] - 0.09) <= bars["mos_ml"] and abs(row[4] - speed / FPS * P) <= bars["stride_length"]


def test_noise_of_the_margins(pipe):
    """What DESIGN 4.22 states: 5 mm of Gaussian joint noise on the first walker, the default table, the gait call's sigma = 2.  Printed, and held only
    to the order of magnitude the issue's prototype found (about 0.02 m a step)."""
    P, beta, speed = cc.WALKERS[0]
    rng = np.random.default_rng(22)
    sd_ap, sd_ml = [], []
    for trial in range(5):
        joints = cc.planted_walker(T, P, beta, speed, 0.3 + trial) + rng.normal(0.0, 0.005, (T, 25, 3)).astype(np.float32)
        events = pipe.gait_parameters(joints, fps=FPS)["events"]
        row = dict(zip(pipe.BALANCE_COLUMNS, pipe.gait_balance(joints, events, fps=FPS)["per_sequence"][0]))
        sd_ap.append(row["mos_ap_sd"]), sd_ml.append(row["mos_ml_sd"])
        print(f"trial {trial}: {int(row['steps'])} steps in {int(row['chains'])} chains, stride {row['stride_length_mean']:.4f} +- {row['stride_length_sd']:.4f} m, COM speed "
              f"{row['com_speed_mean']:.3f} +- {row['com_speed_sd']:.3f} m/s, MoS_AP {row['mos_ap_mean']:.3f} +- {row['mos_ap_sd']:.3f} m, MoS_ML {row['mos_ml_mean']:.3f} +- "
              f"{row['mos_ml_sd']:.3f} m")
    assert 0.005 <= np.mean(sd_ap) <= 0.05 and 0.005 <= np.mean(sd_ml) <= 0.05


@pytest.mark.parametrize("fault", bc.FAULTS)
def test_compare_catches_a_planted_fault(pipe, walkers, fault):
    name, joints, _, events, host = walkers[1]
    rel, hand_events, _ = bc.hand_case()
    hand = pipe.gait_balance_steps(rel, hand_events, max_steps=8, **bc.HAND_RULE)
    bc.compare(bc.loops_balance(joints, events), host)                            # without the fault: equal
    bc.compare(bc.loops_steps(rel, hand_events, max_steps=8, **bc.HAND_RULE), hand)
    caught = []
    for what, got, want in (("walker", bc.loops_balance(joints, events, fault=fault), host),
                            ("hand", bc.loops_steps(rel, hand_events, max_steps=8, fault=fault, **bc.HAND_RULE), hand)):
        try:
            bc.compare(got, want)
        except AssertionError as e:
            caught.append(what)
            print(f"{fault} on the {what} case: {e}")
    assert ("hand" in caught) if fault == "same_foot" else ("walker" in caught), f"{fault}: caught on {caught}"


def test_standing_nan_and_short_sequences(pipe):
    still = cc.planted_walker(64, still=True)
    out = pipe.gait_balance(still, np.zeros(64, np.int32), fps=FPS)
    assert out["per_sequence"][0, :4].tolist() == [0, 0, 0, 0] and np.isnan(out["per_sequence"][0, 4:]).all() and np.isnan(out["steps"]).all()
    assert np.isnan(out["per_frame"][:, 3:6]).all() and (out["per_frame"][:, 6] == 0).all() and np.isnan(out["per_frame"][:, 7]).all()
    assert np.isfinite(out["per_frame"][:, :3]).all()
    ev = np.zeros(64, np.int32)
    ev[[10, 20, 30]] = [1, 2, 1]
    out = pipe.gait_balance(still, ev, fps=FPS, segments=bc.ONE_SEGMENT)        # strikes on a body that does not move: the speed is not positive, no step
    assert out["per_sequence"][0, :3].tolist() == [3, 0, 0]
    for n in (1, 2, 3):
        short = pipe.gait_balance(cc.planted_walker(n), np.ones(n, np.int32), fps=FPS)
        assert short["per_sequence"][0, :3].tolist() == [n, 0, 0] and short["steps"].shape == (1, 256, 15)
    P, beta, speed = cc.WALKERS[0]
    clean = cc.planted_walker(200, P, beta, speed, 0.3)
    events = pipe.gait_parameters(clean, fps=FPS)["events"]
    a = pipe.gait_balance(clean, events, fps=FPS)
    f = int(a["steps"][0, 6, 0]) + 3                             # a frame inside the seventh step, while the stance ankle is read
    side = a["steps"][0, 6, 2]
    hurt = clean.copy()
    hurt[f, gc.KINECTV2[5 if side > 0 else 4]] = np.nan          # the stance ankle: the right one where the left foot lands
    b = pipe.gait_balance(hurt, events, fps=FPS)
    print(f"a NaN stance ankle in frame {f}: {int(a['per_sequence'][0, 1])} steps in {int(a['per_sequence'][0, 2])} chain become {int(b['per_sequence'][0, 1])} in "
          f"{int(b['per_sequence'][0, 2])}")
    assert b["per_sequence"][0, 1] == a["per_sequence"][0, 1] - 1 and b["per_sequence"][0, 2] == 2 and bc.same_bits(b["steps"][0, :6], a["steps"][0, :6])
    assert np.isnan(b["steps"][0, 6, 7:10]).all() and b["steps"][0, 6, 3] == 1 and bc.same_bits(b["steps"][0, 6, 10:13], a["steps"][0, 7, 10:13])


def test_sequences_do_not_see_each_other(pipe):
    from . import test_gpu_balance as g
    joints, lengths = g.case_c()
    events = pipe.gait_parameters(joints, lengths=lengths, fps=FPS)["events"]
    whole = pipe.gait_balance(joints, events, lengths=lengths, fps=FPS)
    a = 0
    for q, n in enumerate(lengths):
        alone = pipe.gait_balance(joints[a:a + n], events[a:a + n], fps=FPS)
        assert bc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]) and bc.same_bits(whole["steps"][q], alone["steps"][0]), q
        assert bc.same_bits(whole["per_sequence"][q], alone["per_sequence"][0]), q
        a += n


def test_bad_arguments_are_refused(pipe):
    joints = cc.planted_walker(30)
    ev = np.zeros(30, np.int32)
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(fps=0.0), "fps"),
                     (dict(fps=nan), "fps"), (dict(gravity=0.0), "gravity"), (dict(gravity=inf), "gravity"), (dict(window=0), "window"), (dict(window=17), "window"),
                     (dict(settle=-1), "settle"), (dict(settle=5), "settle"), (dict(max_step=0), "max_step"), (dict(max_steps=0), "max_steps"), (dict(max_steps=1025), "max_steps"),
                     (dict(window=1.5), "whole"), (dict(segments=()), "segments"), (dict(segments=((0, 20, 1.0),)), "segments"), (dict(segments=((0, 20, 1.0, 0.5),) * 17), "segments"),
                     (dict(segments=((0, 25, 1.0, 0.5),)), "segment joint"), (dict(segments=((0.5, 20, 1.0, 0.5),)), "segment joint"), (dict(segments=((0, 20, 0.0, 0.5),)), "mass"),
                     (dict(segments=((0, 20, nan, 0.5),)), "mass"), (dict(segments=((0, 20, 1.0, inf),)), "fraction")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_balance(joints, ev, **kw)
    for args, word in (((np.zeros((3, 25, 2)), ev), "joints3d"), ((joints, ev[:-1]), "events")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_balance(*args)
    with pytest.raises(ValueError, match="rel"):
        pipe.gait_balance_steps(np.zeros((30, 8)), ev)


def test_header_on_the_host_under_sanitizers(pipe, walkers, tmp_path):
    """csrc/gait_balance.h itself against the statement: one file per sequence of the device tests' calls, two walkers of this file, and the hand-made
    case through the hook's path.  Every bit equal."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_balance_check.cpp")
    exe = str(tmp_path / "gait_balance_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for name, joints, events, lengths, kw in device_cases(pipe):
        segments = kw.get("segments", pipe.BALANCE_SEGMENTS_KINECTV2)
        max_steps = kw.get("max_steps", 256)
        a = 0
        for q, n in enumerate(lengths):
            host = pipe.gait_balance(joints[a:a + n], events[a:a + n], fps=FPS, **kw)
            files.append(bc.write_case(str(tmp_path / f"{name}{q}.bin"), joints[a:a + n], gc.KINECTV2, segments, None, events[a:a + n], bc.DEFAULTS, max_steps, host))
            a += n
    for name, joints, _, events, host in walkers[1::5]:
        files.append(bc.write_case(str(tmp_path / f"{name}.bin"), joints, gc.KINECTV2, bc.ONE_SEGMENT, None, events, bc.DEFAULTS, 256, host))
    rel, events, _ = bc.hand_case()
    for max_steps in (8, 2):
        host = pipe.gait_balance_steps(rel, events, max_steps=max_steps, **bc.HAND_RULE)
        files.append(bc.write_case(str(tmp_path / f"hand{max_steps}.bin"), None, gc.KINECTV2, None, rel, events, bc.HAND_RULE, max_steps, host))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    print(f"{len(files)} files: {r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-200:]}")
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
