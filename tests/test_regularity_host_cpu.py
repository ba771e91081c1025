"""Gait regularity and symmetry on the host: pipeline.gait_regularity and pipeline.gait_autocorr, the numpy float64 statements, against
the yardstick in plain loops of tests/helpers/regularity_checks.py (every bit), against the closed form of the walker's autocorrelation (the bars:
twice the yardstick's own finite-sample error, profiles/gait_regularity_bounds.txt), on a hand-made integer signal whose sums, counts and peaks are
written out in the helper, with an exclude mask, at the edge lengths, on a standing body, without a translation; csrc/gait_regularity.h, the
arithmetic the kernels run, through tests/helpers/gait_regularity_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer
and UBSan and run directly on files this test writes; every refusal.  Every figure is printed before it is asserted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import gait_checks as gc
from .helpers import regularity_checks as rc

FPS = rc.FPS


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def exclude_of(lengths):
    """A mask over a call's frames: frames 60 .. 69 of every sequence that has them, and frame 3."""
    ex = np.zeros(sum(lengths), np.int32)
    a = 0
    for T in lengths:
        ex[a + 60:a + min(T, 70)] = 2
        if T > 3:
            ex[a + 3] = 1
        a += T
    return ex


@pytest.mark.parametrize("J", (25, 49))
def test_statement_against_the_yardstick(pipe, J):
    table = gc.KINECTV2 if J == 25 else gc.OTHER49
    joints, trans, lengths, names = rc.build_call(J, table)
    trans = trans.copy()
    trans[[5, 200]] = np.nan                                   # NaN rows: bob loses the frames, the others do not
    for ex in (None, exclude_of(lengths)):
        for rule in (rc.RULE, dict(max_lag=8, min_lag=2, min_peak=0.1, min_pairs=2), dict(max_lag=255, min_lag=6, min_peak=0.25, min_pairs=20)):
            out = pipe.gait_regularity(joints, lengths, trans, ex, fps=FPS, joints=table, **rule)
            want = rc.signals_of(joints, trans, table)
            assert rc.same_bits(out["per_frame"], want)
            acf, rows = rc.yardstick_call(want, lengths, ex, fps=FPS, **rule)
            assert rc.same_bits(out["acf"], acf) and rc.same_bits(out["per_sequence"], rows), (J, rule)
    assert np.isnan(out["per_frame"][[5, 200], 3]).all() and np.isfinite(out["per_frame"][[5, 200], :3]).all()
    seq = dict(zip(names, out["per_sequence"]))
    assert seq["walk400_back"][0, 5] == 27 and seq["walk400_back"][3, 2] == 14        # the stride of sep and the step of bob with max_lag 255


@pytest.mark.parametrize("T", (400, 130))
def test_statement_against_the_closed_form(pipe, T):
    """The estimator's finite-sample error on the walker, both asymmetries, and the symmetry column of one against the other."""
    lines = []
    for B in (0.0, rc.ASYMMETRY):
        bar = rc.bars(T, B)
        worst = dict(stride_lag=0.0, step_lag=0.0, rho=0.0, symmetry=0.0)
        for P in rc.PERIODS:
            for theta in rc.YAWS:
                for share in rc.PHASES:
                    joints, trans = rc.walker(T, P, B, theta, share * P)
                    out = pipe.gait_regularity(joints, trans=trans, fps=FPS, **rc.RULE)
                    row, acf = out["per_sequence"][0, 0], out["acf"][0, 0]
                    rc.assert_lags(row, P)
                    rc.assert_lags(out["per_sequence"][0, 3], P)                  # bob repeats every step
                    ok = np.isfinite(acf)
                    worst["rho"] = max(worst["rho"], float(np.abs(acf[ok] - rc.closed_form(np.arange(61)[ok], P, B)).max()))
                    worst["stride_lag"] = max(worst["stride_lag"], abs(row[6] - P))
                    worst["step_lag"] = max(worst["step_lag"], abs(row[3] - P / 2))
                    worst["symmetry"] = max(worst["symmetry"], abs(row[8] - rc.closed_symmetry(B)))
                    assert abs(row[9] - 120 * FPS / P) <= 120 * FPS / P * bar["stride_lag"] / (P - bar["stride_lag"])
        lines.append(f"T {T} B {B}: " + ", ".join(f"{k} off by {worst[k]:.4f} (bar {bar[k]:.4f})" for k in worst))
        print(lines[-1])
        assert all(worst[k] <= bar[k] for k in worst), lines[-1]
    # the asymmetric walker's symmetry lies below the symmetric one's by the closed form's amount
    P = rc.PERIODS[0]
    sym = [pipe.gait_regularity(*rc.walker(T, P, B, rc.YAWS[1], 0.37 * P)[:1], fps=FPS, **rc.RULE)["per_sequence"][0, 0, 8] for B in (0.0, rc.ASYMMETRY)]
    gap = (1.0 - rc.closed_symmetry(rc.ASYMMETRY))
    print(f"T {T}: symmetry {sym[0]:.4f} symmetric, {sym[1]:.4f} at B = 0.3; closed form {1.0:.4f} and {rc.closed_symmetry(rc.ASYMMETRY):.4f}")
    assert abs((sym[0] - sym[1]) - gap) <= rc.bars(T, 0.0)["symmetry"] + rc.bars(T, rc.ASYMMETRY)["symmetry"]


def test_white_noise_has_no_first_peak(pipe):
    rng = np.random.default_rng(2004)
    x = rng.standard_normal((200 * 400, 4))
    out = pipe.gait_autocorr(x, lengths=[400] * 200, fps=FPS, **rc.RULE)
    first = np.where(np.arange(4)[None, :] < 3, out["per_sequence"][:, :, 5], out["per_sequence"][:, :, 2])
    print(f"200 x 4 white-noise signals of 400 frames: {int((first >= 0).sum())} with a first peak; largest |rho| past lag 0: {np.nanmax(np.abs(out['acf'][:, :, 1:])):.3f}")
    assert (first == -1).all() and (out["per_sequence"][:, :, [2, 5]] == -1).all() and np.isnan(out["per_sequence"][:, :, [3, 4, 6, 7, 8, 9]]).all()


def test_hand_made_signal(pipe):
    x, acf, rows = rc.hand_case()
    out = pipe.gait_autocorr(x, return_pairs=True, **rc.HAND_RULE)
    print(out["acf"][0, 0].tolist(), out["per_sequence"][0, 0].tolist(), out["per_sequence"][0, 3].tolist())
    assert (out["pairs"][0] == np.array(rc.HAND_N)).all()
    assert rc.same_bits(out["acf"][0], acf) and rc.same_bits(out["per_sequence"][0], rows)
    assert out["acf"][0, 0, 7] > 1.0 and out["acf"][0, 0, 3] == out["acf"][0, 0, 4]          # not clipped; the plateau
    got = rc.yardstick(x[:, 0], True, **rc.HAND_RULE)
    assert rc.same_bits(got[0], acf[0]) and rc.same_bits(got[1], rows[0])
    two = pipe.gait_autocorr(np.concatenate([x, x]), lengths=[31, 31], **rc.HAND_RULE)
    assert rc.same_bits(two["per_sequence"], [rows, rows])
    high = pipe.gait_autocorr(x, **dict(rc.HAND_RULE, min_pairs=17))             # lag 7 has 16 pairs: no neighbour for a peak at 6, none at 7
    assert np.isnan(high["acf"][0, :, 7:]).all() and (high["per_sequence"][0, :, 5] == -1).all() and (high["per_sequence"][0, :3, 2] == -1).all()


def test_exclude_mask(pipe):
    """A walker whose second half has a phase jump behind 50 excluded frames: stride regularity stays, and no pair spans the gap."""
    T, P = 400, rc.PERIODS[0]
    whole, _ = rc.walker(T, P, 0.0, rc.YAWS[1], 0.37 * P)
    late, _ = rc.walker(T, P, 0.0, rc.YAWS[1], 0.37 * P + 8.3)
    joints = np.concatenate([whole[:200], late[200:]])
    ex = np.zeros(T, np.int32)
    ex[175:225] = 1
    a = pipe.gait_regularity(whole, fps=FPS, **rc.RULE)
    b = pipe.gait_regularity(joints, exclude=ex, fps=FPS, **rc.RULE)
    jump = pipe.gait_regularity(joints, fps=FPS, **rc.RULE)
    bar = rc.bars(400, 0.0)
    print(f"stride regularity {a['per_sequence'][0, 0, 7]:.4f} unbroken, {b['per_sequence'][0, 0, 7]:.4f} with the jump excluded, {jump['per_sequence'][0, 0, 7]:.4f} with "
          f"it counted; worst rho difference below lag 50: {np.abs(a['acf'][0, 0, :50] - b['acf'][0, 0, :50]).max():.4f} (bar {bar['rho']:.4f})")
    assert abs(a["per_sequence"][0, 0, 7] - b["per_sequence"][0, 0, 7]) <= bar["rho"] and b["per_sequence"][0, 0, 0] == 350
    assert np.abs(a["acf"][0, 0, :50] - b["acf"][0, 0, :50]).max() <= bar["rho"]
    assert jump["per_sequence"][0, 0, 7] < b["per_sequence"][0, 0, 7] - 0.05                # what the mask is for
    x = pipe.gait_regularity(joints, exclude=ex, fps=FPS, **rc.RULE)["per_frame"]
    x[100, 0] = np.nan
    pairs = pipe.gait_autocorr(x, exclude=ex, fps=FPS, return_pairs=True, **rc.RULE)["pairs"][0]
    valid = (ex == 0)
    assert pairs[1].tolist() == rc.pair_counts(valid.tolist(), 60) and pairs[1][0] == 350 and pairs[1][60] == 175 - 60 + 175 - 60
    valid[100] = False
    assert pairs[0].tolist() == rc.pair_counts(valid.tolist(), 60)


def test_edge_lengths(pipe):
    for T in (1, 19, 20, 64):
        joints, trans = rc.walker(T, 19.3, 0.0, 0.3, 1.1)
        out = pipe.gait_regularity(joints, trans=trans, fps=FPS, **rc.RULE)
        acf, row = out["acf"][0], out["per_sequence"][0]
        assert (row[:, 0] == T).all()
        if T < 20:
            assert np.isnan(acf).all() and np.isnan(row[:, 1:]).all()
        elif T == 20:                                           # only rho(0) = 1 is defined
            assert (acf[:, 0] == 1).all() and np.isnan(acf[:, 1:]).all() and (row[:, 1] > 0).all() and (row[:, [2, 5]] == -1).all() and np.isnan(row[:, [3, 4, 6, 7, 8, 9]]).all()
        else:                                                   # 64 - m >= 20 pairs up to lag 44
            assert np.isfinite(acf[:, :45]).all() and np.isnan(acf[:, 45:]).all()
            assert row[0, 5] == 19 and row[0, 2] in (9, 10) and row[3, 2] in (9, 10) and row[3, 5] == 19
            far = pipe.gait_regularity(joints, trans=trans, fps=FPS, **dict(rc.RULE, min_lag=45))
            assert (far["per_sequence"][0, :, [2, 5]] == -1).all()                  # nothing is found beyond


def test_standing_body_and_no_translation(pipe):
    joints, trans = rc.walker(64, still=True)
    out = pipe.gait_regularity(joints, trans=trans, fps=FPS)
    assert np.isfinite(out["per_frame"]).all() and (out["per_frame"] == out["per_frame"][0]).all()
    assert (out["per_sequence"][0, :, 0] == 64).all() and np.isnan(out["per_sequence"][0, :, 1:]).all() and np.isnan(out["acf"]).all()
    joints, trans = rc.walker(130, 21.7, 0.3, 0.7, 3.0)
    a, b = pipe.gait_regularity(joints, trans=trans, fps=FPS), pipe.gait_regularity(joints, fps=FPS)
    assert np.isnan(b["per_frame"][:, 3]).all() and b["per_sequence"][0, 3, 0] == 0 and np.isnan(b["per_sequence"][0, 3, 1:]).all() and np.isnan(b["acf"][0, 3]).all()
    assert rc.same_bits(a["per_frame"][:, :3], b["per_frame"][:, :3]) and rc.same_bits(a["acf"][0, :3], b["acf"][0, :3]) and rc.same_bits(a["per_sequence"][0, :3], b["per_sequence"][0, :3])


def test_smoothing_runs_inside_a_sequence(pipe):
    joints, trans, lengths, _ = rc.build_call()
    raw = pipe.gait_regularity(joints, lengths, trans, fps=FPS)["per_frame"]
    out = pipe.gait_regularity(joints, lengths, trans, fps=FPS, sigma=2.0)
    a = 0
    for T in lengths:
        for k in range(4):
            assert rc.same_bits(out["per_frame"][a:a + T, k], pipe.gauss_filter1d(raw[a:a + T, k], 2.0))
        a += T
    assert rc.same_bits(out["acf"], pipe.gait_autocorr(out["per_frame"], lengths, fps=FPS)["acf"])


def test_sequences_do_not_see_each_other(pipe):
    joints, trans, lengths, names = rc.build_call()
    ex = exclude_of(lengths)
    for sigma in (0.0, 2.0):
        whole = pipe.gait_regularity(joints, lengths, trans, ex, fps=FPS, sigma=sigma)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_regularity(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], fps=FPS, sigma=sigma)
            assert rc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]) and rc.same_bits(whole["acf"][q], alone["acf"][0]), names[q]
            assert rc.same_bits(whole["per_sequence"][q], alone["per_sequence"][0]), names[q]
            a += n


def test_bad_arguments_are_refused(pipe):
    joints, trans = rc.walker(30)
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(fps=0.0), "fps"),
                     (dict(fps=nan), "fps"), (dict(fps=inf), "fps"), (dict(sigma=-1.0), "sigma"), (dict(sigma=nan), "sigma"), (dict(sigma=16.5), "sigma"),
                     (dict(max_lag=7), "max_lag"), (dict(max_lag=256), "max_lag"), (dict(max_lag=60.5), "whole"), (dict(min_lag=1), "min_lag"), (dict(min_lag=59), "min_lag"),
                     (dict(min_peak=0.0), "min_peak"), (dict(min_peak=1.5), "min_peak"), (dict(min_peak=nan), "min_peak"), (dict(min_pairs=1), "min_pairs"),
                     (dict(min_pairs=2 ** 20 + 1), "min_pairs"), (dict(trans=np.zeros((29, 3))), "trans"), (dict(exclude=np.zeros(29, np.int32)), "exclude")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_regularity(joints, **kw)
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_regularity(np.zeros((3, 25, 2)))
    with pytest.raises(ValueError, match="signals"):
        pipe.gait_autocorr(np.zeros((30, 3)))
    assert pipe.REGULARITY_CHANNELS == ("sep", "lift", "sway", "bob") and len(pipe.REGULARITY_COLUMNS) == 10


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_regularity.h itself against the statement with sigma = 0: one file per sequence of the device tests' call with both tables, with and
    without trans and exclude, at max_lag 8, 60 and 255, and the hand-made signal through the hook's path.  Every bit equal."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_regularity_check.cpp")
    exe = str(tmp_path / "gait_regularity_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for J, rule, with_trans in ((25, dict(rc.RULE, fps=FPS), True), (49, dict(fps=FPS, max_lag=255, min_lag=6, min_peak=0.25, min_pairs=20), False),
                                (25, dict(fps=FPS, max_lag=8, min_lag=2, min_peak=0.1, min_pairs=2), True)):
        table = gc.KINECTV2 if J == 25 else gc.OTHER49
        joints, trans, lengths, names = rc.build_call(J, table)
        trans = trans.copy()
        trans[[5, 200]] = np.nan
        ex = exclude_of(lengths)
        a = 0
        for name, n in zip(names, lengths):
            tr = trans[a:a + n] if with_trans else None
            e = ex[a:a + n] if J == 25 else None
            host = pipe.gait_regularity(joints[a:a + n], trans=tr, exclude=e, joints=table, **rule)
            files.append(rc.write_case(str(tmp_path / f"J{J}_{rule['max_lag']}_{name}.bin"), joints[a:a + n], table, tr, None, e, rule, host))
            a += n
    x, _, _ = rc.hand_case()
    files.append(rc.write_case(str(tmp_path / "hand.bin"), None, gc.KINECTV2, None, x, None, rc.HAND_RULE, pipe.gait_autocorr(x, **rc.HAND_RULE)))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
