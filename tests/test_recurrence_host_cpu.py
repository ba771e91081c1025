"""Recurrence quantification of the gait signals on the host: pipeline.gait_recurrence and pipeline.gait_recurrence_counts, the numpy
statements, against the yardstick in plain loops over every pair of tests/helpers/recurrence_checks.py (every integer, every bit of per_sequence), on
the hand-made integer signals whose lines are worked out in the helper, at the edge shapes, on white noise against 1 - exp(-1/2) (the bar: twice the
yardstick's own miss, profiles/gait_recurrence_bounds.txt); pipeline.recurrence_rows; csrc/gait_recurrence.h, the arithmetic the kernels run, through
tests/helpers/gait_recurrence_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on files
this test writes; every refusal, in the same words from the statement and from the header.  Every figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import gait_checks as gc
from .helpers import recurrence_checks as kc
from .helpers import regularity_checks as rc


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def rows_equal(out, at, counts, hist, **kw):
    want = kc.yardstick_rows(counts, hist, **kw)
    for name in kc.ROWS:
        assert kc.same_bits(np.float64(out[name][at]), np.float64(want[name])), (name, at, out[name][at], want[name])


def equals_the_yardstick(out, signals, lengths, ex, rule, **kw):
    rows, hist, counts = kc.yardstick_call(signals, lengths, ex, **rule)
    n_seq = len(lengths)
    assert out["hist"].dtype == np.int64 and out["counts"].dtype == np.int64 and out["per_sequence"].dtype == np.float64
    assert out["per_sequence"].shape == (n_seq, 4, 5) and out["hist"].shape == (n_seq, 4, 255) and out["counts"].shape == (n_seq, 4, 6)
    assert kc.same_ints(out["counts"], counts) and kc.same_ints(out["hist"], hist) and kc.same_bits(out["per_sequence"], rows), rule
    assert kc.invariant(out["hist"], out["counts"])
    for q in range(n_seq):
        for ch in range(4):
            rows_equal(out, (q, ch), counts[q, ch].tolist(), hist[q, ch].tolist(), **kw)
    return rows, hist, counts


@pytest.mark.parametrize("J", (25, 49))
def test_statement_against_the_yardstick(pipe, J):
    joints, trans, lengths, names, ex, table = kc.noisy_call(J)
    want_frame = {True: rc.signals_of(joints, trans, table), False: rc.signals_of(joints, None, table)}
    for with_trans, with_ex in ((True, True), (True, False), (False, True), (False, False)):
        for values in (kc.RULES if with_trans and with_ex and J == 25 else kc.RULES[:2]):
            rule = kc.rule_of(*values)
            out = pipe.gait_recurrence(joints, lengths, trans if with_trans else None, ex if with_ex else None, joints=table, **rule)
            assert kc.same_bits(out["per_frame"], want_frame[with_trans])
            _, hist, counts = equals_the_yardstick(out, want_frame[with_trans], lengths, ex if with_ex else None, rule)
            if values[3] == 500:                               # a Theiler window larger than every M: no pair anywhere
                assert (counts[:, :, 1:] == 0).all() and (hist == 0).all() and counts[-1, :, 0].min() > 200
    full = pipe.gait_recurrence(joints, lengths, trans, None, joints=table)
    seq = dict(zip(names, full["counts"]))
    at = names.index("walk400_back")
    print("walk400_back: counts", seq["walk400_back"].tolist(), "rate", full["recurrence_rate"][at].tolist(), "determinism", full["determinism"][at].tolist())
    assert (seq["walk400_back"][:, 2] >= 1000).all() and (full["lines"][at] >= 100).all() and (seq["walk400_back"][:, 5] >= 5).all()
    assert np.isfinite(full["line_entropy"][at]).all() and (seq["one"] == 0).all()
    still = names.index("standing64")                          # r = 0: comparable pairs, none recurrent
    assert (seq["standing64"][:, 1] > 0).all() and (seq["standing64"][:, 2:] == 0).all() and (full["per_sequence"][still, :, 3:] == 0).all()
    enough = seq["standing64"][:, 0] >= 50
    print("standing64: counts", seq["standing64"].tolist(), "rate", full["recurrence_rate"][still].tolist())
    assert enough.sum() >= 3 and (full["recurrence_rate"][still][enough] == 0).all() and np.isnan(full["determinism"][still]).all()


def test_hand_made_signals(pipe):
    x = kc.hand_signals(kc.HAND_PERIODIC_X)
    out = pipe.gait_recurrence_counts(x, min_points=10, **kc.HAND_PERIODIC_RULE)
    print(out["per_sequence"][0, 0].tolist(), out["counts"][0, 0].tolist(), {k: out[k][0, 0] for k in kc.ROWS})
    for ch in range(4):
        assert out["counts"][0, ch].tolist() == kc.HAND_PERIODIC_COUNTS and out["hist"][0, ch].tolist() == kc.HAND_PERIODIC_HIST
    n, mu, sd, r, eps2 = out["per_sequence"][0, 0].tolist()
    assert n == 31 and mu == 18 / 31 and abs(sd - kc.HAND_SD) < 1e-15 and r == 0.5 * sd and eps2 == (r * r) * 2.0 and 1.3258 < eps2 < 1.3259
    assert out["recurrence_rate"][0, 0] == 75 / 435 and out["determinism"][0, 0] == 1.0 and out["mean_line"][0, 0] == 15.0 and out["longest"][0, 0] == 25.0
    assert out["divergence"][0, 0] == 1 / 25 and abs(out["line_entropy"][0, 0] - math.log(5.0)) < 1e-15 and out["lines"][0, 0] == 5 and out["line_points"][0, 0] == 75
    assert out["ratio"][0, 0] == 1.0 / (75 / 435)
    row, hist, counts = kc.yardstick(x[:, 0], None, **kc.HAND_PERIODIC_RULE)
    assert counts == kc.HAND_PERIODIC_COUNTS and hist == kc.HAND_PERIODIC_HIST and kc.same_bits(out["per_sequence"][0, 0], row)
    wide = pipe.gait_recurrence_counts(x, min_points=10, **kc.HAND_WIDE_RULE)
    row, hist, counts = kc.yardstick(x[:, 0], None, **kc.HAND_WIDE_RULE)
    assert counts == kc.HAND_WIDE_COUNTS and hist == kc.HAND_WIDE_HIST and 5.3032 < row[4] < 5.3033
    assert wide["counts"][0, 3].tolist() == kc.HAND_WIDE_COUNTS and wide["hist"][0, 3].tolist() == kc.HAND_WIDE_HIST
    assert (wide["lines"][0, 3], wide["line_points"][0, 3]) == kc.HAND_WIDE_LINES and wide["determinism"][0, 3] == 135 / 147
    xl = kc.hand_signals(kc.HAND_LONG_X)
    long = pipe.gait_recurrence_counts(xl, **kc.HAND_PERIODIC_RULE)
    row, hist, counts = kc.yardstick(xl[:, 0], None, **kc.HAND_PERIODIC_RULE)
    assert counts == kc.HAND_LONG_COUNTS and hist == kc.HAND_LONG_HIST and sum(hist) == 51
    assert long["counts"][0, 1].tolist() == kc.HAND_LONG_COUNTS and long["hist"][0, 1].tolist() == kc.HAND_LONG_HIST
    assert long["lines"][0, 1] == 119 and long["mean_line"][0, 1] == 35581 / 119 and long["longest"][0, 1] == 594.0
    rows_equal(long, (0, 1), counts, hist)
    xb = kc.hand_signals(kc.HAND_BROKEN_X)
    out = pipe.gait_recurrence_counts(xb, **kc.HAND_BROKEN_RULE)
    row, hist, counts = kc.yardstick(xb[:, 0], None, **kc.HAND_BROKEN_RULE)
    assert counts == kc.HAND_BROKEN_COUNTS and hist == kc.HAND_BROKEN_HIST
    assert out["counts"][0, 2].tolist() == kc.HAND_BROKEN_COUNTS and out["hist"][0, 2].tolist() == kc.HAND_BROKEN_HIST and kc.same_bits(out["per_sequence"][0, 2], row)
    assert np.isnan(out["recurrence_rate"]).all() and (out["lines"] == 6).all()      # 24 points: fewer than 50
    three = pipe.gait_recurrence_counts(np.concatenate([x, xb[:9], x]), lengths=[31, 9, 31], **kc.HAND_PERIODIC_RULE)
    assert three["counts"][0, 0].tolist() == kc.HAND_PERIODIC_COUNTS and three["counts"][2, 0].tolist() == kc.HAND_PERIODIC_COUNTS
    assert three["hist"][2, 0].tolist() == kc.HAND_PERIODIC_HIST and kc.invariant(three["hist"], three["counts"])


def test_edge_shapes(pipe):
    rng = np.random.default_rng(7)
    wide = kc.rule_of(0, 8, 16, 0, 0.8)
    for T, rule, M in ((1, kc.RULE, 0), (8, kc.RULE, 0), (9, kc.RULE, 1), (10, kc.RULE, 2), (11, kc.RULE, 3), (112, wide, 0), (113, wide, 1), (114, wide, 2), (115, wide, 3)):
        x = rng.standard_normal((T, 4))                         # one frame; span >= T; M = 1, 2 and 3: the half-offset of an even M
        rule = dict(rule, derivative=0, theiler=0, radius=10.0)      # every pair recurs
        out = pipe.gait_recurrence_counts(x, **rule)
        equals_the_yardstick(out, x, [T], None, rule)
        pairs = M * (M - 1) // 2
        want = [M, pairs, pairs, 0, 0, max(M - 1, 0)]
        print(T, M, out["counts"][0, 0].tolist())
        assert out["counts"][0, 0].tolist() == want
        assert np.isnan(out["recurrence_rate"]).all()
    x = rng.standard_normal((40, 4))
    for values in ((1, 2, 1, 3, 0.8), (0, 3, 2, 0, 1.5), (2, 2, 1, 39, 0.8), (2, 2, 1, 36, 10.0)):
        equals_the_yardstick(pipe.gait_recurrence_counts(x, min_points=5, **kc.rule_of(*values)), x, [40], None, kc.rule_of(*values), min_points=5)
    # the standing body: r = 0, every pair is comparable and none recurs, though every D2 is 0 <= eps2 = 0
    joints, trans = rc.walker(64, still=True)
    for d in (0, 1):
        still = pipe.gait_recurrence(joints, trans=trans, **dict(kc.RULE, derivative=d))
        M = 64 - d - 8
        assert np.isfinite(still["per_frame"]).all() and (still["counts"][0, :, 0] == M).all() and (still["counts"][0, :, 1] == (M - 9) * (M - 8) // 2).all()
        assert (still["counts"][0, :, 2:] == 0).all() and (still["hist"] == 0).all() and (still["per_sequence"][0, :, 3:] == 0).all()
    # an infinite distance is comparable and not recurrent
    x = np.zeros((12, 4))
    x[:, 0] = [0, 1e200, 0, 0, -1e200, 0, 0, 1e200, 0, 0, 0, 0]
    x[:, 1] = [0, 1, 0, 0, -1, 0, 0, 1, 0, 0, 0, 0]
    rule = kc.rule_of(0, 2, 1, 0, 10.0)
    out = pipe.gait_recurrence_counts(x, min_points=5, **rule)
    _, _, counts = equals_the_yardstick(out, x, [12], None, rule, min_points=5)
    assert counts[0, 0, 1] == 55 and 0 < counts[0, 0, 2] < 55 and counts[0, 1, 2] == 55 and np.isinf(out["per_sequence"][0, 0, 4])


def test_runs_at_the_word_boundary(pipe):
    """Validity runs that begin and end at frames 63, 64 and 65, by NaN and by exclude; an excluded frame in the middle of a long line."""
    x, lengths, ex = kc.boundary_call()
    for values in ((1, 5, 2, 8, 0.8), (0, 2, 1, 0, 0.2), (2, 3, 16, 5, 10.0)):
        rule = kc.rule_of(*values)
        _, hist, counts = equals_the_yardstick(pipe.gait_recurrence_counts(x, lengths, ex, **rule), x, lengths, ex, rule)
    assert (counts[:5, :, 2] > 20).all()
    out = pipe.gait_recurrence_counts(x[-300:], None, ex[-300:], **kc.rule_of(0, 2, 1, 0, 0.8))
    free = pipe.gait_recurrence_counts(x[-300:], None, None, **kc.rule_of(0, 2, 1, 0, 0.8))
    print("the long line:", free["counts"][0, 0].tolist(), "cut by an excluded frame:", out["counts"][0, 0].tolist())
    assert free["counts"][0, 0, 5] >= 270 and 100 < out["counts"][0, 0, 5] < 150 and out["counts"][0, 0, 0] == free["counts"][0, 0, 0] - 2


def test_sequences_do_not_see_each_other(pipe):
    joints, trans, lengths, names, ex, table = kc.noisy_call(25)
    for sigma in (0.0, 2.0):
        whole = pipe.gait_recurrence(joints, lengths, trans, ex, sigma=sigma)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_recurrence(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], sigma=sigma)
            assert kc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]) and kc.same_ints(whole["counts"][q], alone["counts"][0]), names[q]
            assert kc.same_ints(whole["hist"][q], alone["hist"][0]) and kc.same_bits(whole["per_sequence"][q], alone["per_sequence"][0]), names[q]
            assert kc.same_bits(whole["line_entropy"][q], alone["line_entropy"][0]), names[q]
            a += n
        reg = pipe.gait_regularity(joints, lengths, trans, ex, sigma=sigma)
        assert kc.same_bits(whole["per_frame"], reg["per_frame"])


def test_recurrence_rows(pipe):
    hist = np.zeros((1, 255), np.int64)
    hist[0, [0, 1, 2, 254]] = (40, 6, 3, 1)
    counts = np.array([[60, 1000, 40 + 12 + 9 + 255 + 300 + 700, 2, 1000, 700]], np.int64)
    assert kc.invariant(hist, counts)
    out = pipe.recurrence_rows(counts, hist)
    want = kc.yardstick_rows(counts[0].tolist(), hist[0].tolist())
    print({k: out[k][0] for k in kc.ROWS})
    assert all(kc.same_bits(np.float64(out[k][0]), np.float64(want[k])) for k in kc.ROWS) and out["lines"].dtype == np.int64
    assert out["lines"][0] == 12 and out["line_points"][0] == 12 + 9 + 255 + 1000 and out["recurrence_rate"][0] == 1316 / 1000 and out["determinism"][0] == 1276 / 1316
    assert out["mean_line"][0] == 1276 / 12 and out["longest"][0] == 700.0 and out["divergence"][0] == 1 / 700
    # the overflow class: the two long lines are ONE class beside those of 2, 3 and 255
    p = [6 / 12, 3 / 12, 1 / 12, 2 / 12]
    acc = 0.0
    for v in p:
        acc = acc + v * math.log(v)
    assert out["line_entropy"][0] == -acc
    one = pipe.recurrence_rows(counts, hist, min_line=1)
    assert one["lines"][0] == 52 and one["line_points"][0] == 1316 and one["determinism"][0] == 1.0
    top = pipe.recurrence_rows(counts, hist, min_line=255)
    assert top["lines"][0] == 3 and top["line_points"][0] == 1255 and top["mean_line"][0] == 1255 / 3
    assert all(kc.same_bits(np.float64(top[k][0]), np.float64(kc.yardstick_rows(counts[0].tolist(), hist[0].tolist(), min_line=255)[k])) for k in kc.ROWS)
    # min_points: everything but the two integers is NaN
    few = pipe.recurrence_rows(counts, hist, min_points=61)
    assert few["lines"][0] == 12 and all(np.isnan(few[k][0]) for k in kc.ROWS[2:])
    assert np.isfinite(pipe.recurrence_rows(counts, hist, min_points=60)["ratio"][0])
    # longest < min_line: longest and divergence are NaN, and with no line so are the mean line and the entropy
    short = np.zeros((1, 255), np.int64)
    short[0, 0] = 7
    lone = pipe.recurrence_rows(np.array([[60, 100, 7, 0, 0, 1]], np.int64), short)
    assert lone["lines"][0] == 0 and lone["determinism"][0] == 0.0 and lone["recurrence_rate"][0] == 0.07 and lone["ratio"][0] == 0.0
    assert all(np.isnan(lone[k][0]) for k in ("mean_line", "longest", "divergence", "line_entropy"))
    none = pipe.recurrence_rows(np.array([[60, 0, 0, 0, 0, 0]], np.int64), np.zeros((1, 255), np.int64))
    assert all(np.isnan(none[k][0]) for k in kc.ROWS[2:])
    zero = pipe.recurrence_rows(np.array([[60, 10, 0, 0, 0, 0]], np.int64), np.zeros((1, 255), np.int64))
    assert zero["recurrence_rate"][0] == 0.0 and np.isnan(zero["determinism"][0]) and np.isnan(zero["ratio"][0])
    assert pipe.recurrence_rows(np.zeros((2, 4, 6), np.int64), np.zeros((2, 4, 255), np.int64))["ratio"].shape == (2, 4)
    for bad_counts, bad_hist in ((np.zeros((1, 6)), np.zeros((1, 255), np.int64)), (np.zeros((1, 5), np.int64), np.zeros((1, 255), np.int64)),
                                 (np.zeros((1, 6), np.int64), np.zeros((1, 254), np.int64)), (np.zeros((1, 6), np.int64), np.zeros((1, 255)))):
        with pytest.raises(ValueError, match="counts"):
            pipe.recurrence_rows(bad_counts, bad_hist)
    for kw in (dict(min_line=0), dict(min_line=256), dict(min_line=1.5)):
        with pytest.raises(ValueError, match="min_line"):
            pipe.recurrence_rows(counts, hist, **kw)
    with pytest.raises(ValueError, match="min_points"):
        pipe.recurrence_rows(counts, hist, min_points=0)


def test_white_noise_against_the_closed_form(pipe):
    x = np.stack([kc.white_noise(seed) for seed in kc.WHITE_SEEDS[:4]], axis=1)
    out = pipe.gait_recurrence_counts(x, **kc.WHITE_RULE)
    bar = 2.0 * kc.WHITE_MEASURED
    miss = np.abs(out["recurrence_rate"][0] - kc.WHITE_CLOSED)
    print(f"rate {out['recurrence_rate'][0].tolist()}, closed form {kc.WHITE_CLOSED:.5f}, worst miss {miss.max():.4f} (bar {bar:.4f})")
    assert (miss <= bar).all() and (out["counts"][0, :, 1] == 998 * 997 // 2).all()
    row, hist, counts = kc.yardstick(x[:, 0], None, **kc.WHITE_RULE)
    assert out["counts"][0, 0].tolist() == counts and out["hist"][0, 0].tolist() == hist and kc.same_bits(out["per_sequence"][0, 0], row)
    record = os.path.join(ROOT, "profiles", "gait_recurrence_bounds.txt")
    with open(record) as f:
        worst = float(f.read().strip().splitlines()[-1])
    assert worst <= kc.WHITE_MEASURED < worst + 1e-4          # the constant is the record's, rounded up in the fourth place


BAD = ((dict(derivative=-1), "derivative outside [0, 2]"), (dict(derivative=3), "derivative outside [0, 2]"), (dict(dim=1), "dim outside [2, 8]"), (dict(dim=9), "dim outside [2, 8]"),
       (dict(lag=0), "lag outside [1, 16]"), (dict(lag=17), "lag outside [1, 16]"), (dict(theiler=-1), "theiler outside [0, 4096]"), (dict(theiler=4097), "theiler outside [0, 4096]"),
       (dict(radius=0.0), "radius must be finite and within (0, 10]"), (dict(radius=10.5), "radius must be finite and within (0, 10]"),
       (dict(radius=float("nan")), "radius must be finite and within (0, 10]"), (dict(radius=float("inf")), "radius must be finite and within (0, 10]"))
LONG = "sequence 0 has 32769 frames, more than 32768 (the work is quadratic in them)"


def test_bad_arguments_are_refused(pipe):
    joints, trans = rc.walker(30)
    for kw, why in BAD:
        for call in (lambda: pipe.gait_recurrence(joints, **kw), lambda: pipe.gait_recurrence_counts(np.zeros((30, 4)), **kw)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == why
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(sigma=-1.0), "sigma"),
                     (dict(sigma=float("nan")), "sigma"), (dict(sigma=16.5), "sigma"), (dict(dim=2.5), "whole"), (dict(theiler=1.5), "whole"), (dict(trans=np.zeros((29, 3))), "trans"),
                     (dict(exclude=np.zeros(29, np.int32)), "exclude"), (dict(min_line=0), "min_line"), (dict(min_points=0), "min_points")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_recurrence(joints, **kw)
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_recurrence(np.zeros((3, 25, 2)))
    with pytest.raises(ValueError, match="signals"):
        pipe.gait_recurrence_counts(np.zeros((30, 3)))
    for call in (lambda: pipe.gait_recurrence_counts(np.zeros((32769 + 5, 4)), lengths=[32769, 5]), lambda: pipe.gait_recurrence(np.zeros((32769, 25, 3), np.float32))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == LONG
    assert pipe.RECURRENCE_CHANNELS is pipe.REGULARITY_CHANNELS and pipe.RECURRENCE_COLUMNS == ("n", "mean", "sd", "r", "eps2") and pipe.RECURRENCE_BINS == 255
    assert pipe.RECURRENCE_COUNTS == ("points", "comparable", "recurrent", "long_lines", "long_points", "longest") and pipe.RECURRENCE_MAX_FRAMES == 32768
    assert pipe.RECURRENCE_ROWS == kc.ROWS


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_recurrence.h itself against the statement with sigma = 0: one file per sequence of the noisy call with both tables, with and without
    trans and exclude, over kc.RULES; the hand-made signals, the word-boundary runs and a sequence of more than two parts on signals; every refusal, in
    the statement's words.  The program deals every case's offsets to its own parts, to 1 and to 16, and walks M = 1 .. 12 against the plain triangle."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_recurrence_check.cpp")
    exe = str(tmp_path / "gait_recurrence_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for k, values in enumerate(kc.RULES):
        J, with_trans = (25, True) if k % 2 == 0 else (49, False)
        rule = kc.rule_of(*values)
        joints, trans, lengths, names, ex, table = kc.noisy_call(J)
        a = 0
        for name, n in zip(names, lengths):
            tr = trans[a:a + n] if with_trans else None
            e = ex[a:a + n] if k % 3 else None
            host = pipe.gait_recurrence(joints[a:a + n], trans=tr, exclude=e, joints=table, **rule)
            files.append(kc.write_case(str(tmp_path / f"J{J}_{k}_{name}.bin"), joints[a:a + n], table, tr, None, e, rule, host))
            a += n
    for k, (x, rule) in enumerate(kc.HAND_CASES):
        x = kc.hand_signals(x)
        files.append(kc.write_case(str(tmp_path / f"hand{k}.bin"), None, gc.KINECTV2, None, x, None, rule, pipe.gait_recurrence_counts(x, **rule)))
    x, lengths, ex = kc.boundary_call()
    a = 0
    for k, n in enumerate(lengths):
        host = pipe.gait_recurrence_counts(x[a:a + n], None, ex[a:a + n], **kc.RULE)
        files.append(kc.write_case(str(tmp_path / f"edge{k}.bin"), None, gc.KINECTV2, None, x[a:a + n], ex[a:a + n], kc.RULE, host))
        a += n
    x = np.random.default_rng(1025).standard_normal((1026 + 1, 4))      # M = 1026: 513 offsets, three parts, the half-offset among them
    rule = kc.rule_of(0, 2, 1, 1, 0.8)
    files.append(kc.write_case(str(tmp_path / "parts.bin"), None, gc.KINECTV2, None, x, None, rule, pipe.gait_recurrence_counts(x, **rule)))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
    refused = [(kc.write_case(str(tmp_path / f"bad{k}.bin"), None, gc.KINECTV2, None, np.zeros((30, 4)), None, dict(kc.RULE, **kw), None), why) for k, (kw, why) in enumerate(BAD)]
    refused.append((kc.write_case(str(tmp_path / "long.bin"), None, gc.KINECTV2, None, np.zeros((32769, 4)), None, kc.RULE, None), LONG))
    r = subprocess.run([exe] + [path for path, _ in refused], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "ok" and lines[:-1] == [f"refused {path}: {why}" for path, why in refused], r.stdout[-4000:] + r.stderr[-4000:]
