"""Sample entropy of the gait signals on the host: pipeline.gait_entropy and pipeline.gait_sampen, the numpy statements, against the
yardstick in plain loops over every pair of tests/helpers/entropy_checks.py (every integer, every bit), on the hand-made integer signal whose counts
are written out in the helper, at the edge shapes, on white noise against the closed form (the bars: twice the yardstick's own finite-sample error,
profiles/gait_entropy_bounds.txt); pipeline.entropy_rows; csrc/gait_entropy.h, the arithmetic the kernels run, through
tests/helpers/gait_entropy_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on files this
test writes; every refusal, in the same words from the statement and from the header.  Every figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import entropy_checks as ec
from .helpers import gait_checks as gc
from .helpers import regularity_checks as rc


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def rule_of(m, d, scales, fraction=0.2):
    return dict(m=m, fraction=fraction, derivative=d, scales=scales)


@pytest.mark.parametrize("J", (25, 49))
def test_statement_against_the_yardstick(pipe, J):
    joints, trans, lengths, names, ex, table = ec.noisy_call(J)
    want_frame = {True: rc.signals_of(joints, trans, table), False: rc.signals_of(joints, None, table)}
    for with_trans, with_ex in ((True, True), (True, False), (False, True), (False, False)):
        for m, d, scales in (ec.RULES if with_trans and with_ex else ec.RULES[:2]):
            rule = rule_of(m, d, scales)
            out = pipe.gait_entropy(joints, lengths, trans if with_trans else None, ex if with_ex else None, joints=table, **rule)
            assert ec.same_bits(out["per_frame"], want_frame[with_trans])
            counts, rows = ec.yardstick_call(want_frame[with_trans], lengths, ex if with_ex else None, **rule)
            assert out["counts"].dtype == np.int64 and out["counts"].shape == (7, 4, scales, 3) and out["per_sequence"].shape == (7, 4, 4)
            assert ec.same_counts(out["counts"], counts) and ec.same_bits(out["per_sequence"], rows), (J, rule, with_trans, with_ex)
            for q in range(7):
                for ch in range(4):
                    sampen, total = ec.yardstick_sampen(counts[q, ch].tolist())
                    assert ec.same_bits(out["sampen"][q, ch], sampen) and ec.same_bits(out["complexity"][q, ch], total)
    full = pipe.gait_entropy(joints, lengths, trans, None, joints=table, **ec.RULE)
    assert np.isnan(full["per_frame"][[5, 200], 3]).all() and np.isfinite(full["per_frame"][[5, 200], :3]).all()
    seq = dict(zip(names, full["counts"]))
    assert (seq["walk400_back"][:, 0, 0] == 396).all() and (seq["walk400_back"][:3, 0, 2] >= 100).all()        # 400 - 2 - 2 templates
    assert (seq["walk130"][:3, 0, 0] == 126).all() and seq["walk130"][3, 0, 0] == 121                           # bob loses five to the NaN row at frame 5
    assert np.isfinite(full["sampen"][-1]).all() and np.isfinite(full["complexity"][-1]).all()


def test_hand_made_signal(pipe):
    x = ec.hand_signals()
    for rule, n, sd, want in ec.HAND_CASES:
        out = pipe.gait_sampen(x, **rule)
        print(rule, out["counts"][0, 0].tolist(), out["per_sequence"][0, 0].tolist())
        assert (out["counts"][0] == np.array(want)).all()
        assert (out["per_sequence"][0, :, 0] == n).all() and (out["per_sequence"][0, :, 2] == sd).all()
        assert ec.same_bits(out["per_sequence"][0, :, 3], [rule["fraction"] * sd] * 4)
        counts, row = ec.yardstick(x[:, 0], None, **rule)
        assert counts == [list(w) for w in want] and row[0] == n and row[2] == sd
        two = pipe.gait_sampen(np.concatenate([x, x[:9], x]), lengths=[31, 9, 31], **rule)
        assert ec.same_counts(two["counts"][0], out["counts"][0]) and ec.same_counts(two["counts"][2], out["counts"][0])
    assert np.isnan(out["sampen"]).all()                        # 26 templates are fewer than 50
    low = pipe.gait_sampen(x, min_templates=10, **ec.HAND_CASES[0][0])
    assert ec.same_bits(low["sampen"][0, 0], [math.log(96 / 52), math.log(4 / 4)]) and low["complexity"][0, 0] == math.log(96 / 52) + 0.0


def test_edge_shapes(pipe):
    rng = np.random.default_rng(7)
    one = pipe.gait_sampen(rng.standard_normal((1, 4)), **ec.RULE)
    assert (one["counts"] == 0).all() and np.isnan(one["per_sequence"][0, :, 1:]).all() and (one["per_sequence"][0, :, 0] == 0).all()
    one = pipe.gait_sampen(rng.standard_normal((1, 4)), **rule_of(2, 0, 3))
    assert (one["counts"] == 0).all() and (one["per_sequence"][0, :, 0] == 1).all() and np.isnan(one["per_sequence"][0, :, 2:]).all()
    # N - m <= 0 at the coarse scales: 19 frames, m = 4: N = 19, 9, 6, 4, 3, 2, 2, 2
    x = rng.standard_normal((19, 4))
    out = pipe.gait_sampen(x, **rule_of(4, 0, 8, 0.5))
    assert out["counts"][0, :, :, 0].tolist() == [[15, 5, 2, 0, 0, 0, 0, 0]] * 4 and (out["counts"][0, :, 3:] == 0).all()
    counts, rows = ec.yardstick_call(x, [19], **rule_of(4, 0, 8, 0.5))
    assert ec.same_counts(out["counts"], counts) and ec.same_bits(out["per_sequence"], rows)
    # the standing body: r = 0 and nothing is counted, though every template is valid
    joints, trans = rc.walker(64, still=True)
    still = pipe.gait_entropy(joints, trans=trans, **rule_of(2, 0, 2))
    assert (still["per_sequence"][0, :, 0] == 64).all() and (still["per_sequence"][0, :, 2:] == 0).all()
    assert still["counts"][0, :, :, 0].tolist() == [[62, 30]] * 4 and (still["counts"][0, :, :, 1:] == 0).all() and np.isnan(still["sampen"]).all()
    # a coarse-graining window that straddles an excluded frame
    x = rng.standard_normal((40, 4))
    ex = ec.exclude_straddle(40)
    out = pipe.gait_sampen(x, exclude=ex, **rule_of(1, 0, 3))
    assert out["counts"][0, 0, :, 0].tolist() == [39 - 2, 19 - 2, 12 - 2] and (out["per_sequence"][0, :, 0] == 39).all()
    counts, rows = ec.yardstick_call(x, [40], ex, **rule_of(1, 0, 3))
    assert ec.same_counts(out["counts"], counts) and ec.same_bits(out["per_sequence"], rows)


def test_runs_at_the_word_boundary(pipe):
    """Validity runs that begin and end at frames 63, 64 and 65, by NaN and by exclude."""
    x, lengths, ex = ec_boundary_call()
    for m, d, scales in ((2, 2, 3), (1, 0, 2)):
        out = pipe.gait_sampen(x, lengths, ex, **rule_of(m, d, scales, 0.5))
        counts, rows = ec.yardstick_call(x, lengths, ex, **rule_of(m, d, scales, 0.5))
        assert ec.same_counts(out["counts"], counts) and ec.same_bits(out["per_sequence"], rows)
    assert out["per_sequence"][:, 0, 0].tolist() == [129, 129, 128, 126, 125, 65, 66, 66, 2]


def ec_boundary_call():
    rng = np.random.default_rng(15)
    cases = ((130, (63,), ()), (130, (64,), ()), (130, (65,), (0,)), (131, (0, 1), (63, 64, 65)), (130, (62, 63), (65, 66, 129)), (66, (), (64,)), (130, range(64, 128), ()),
             (130, (), range(0, 64)), (66, range(0, 63), (65,)))
    lengths = [T for T, _, _ in cases]
    x = rng.standard_normal((sum(lengths), 4))
    ex = np.zeros(sum(lengths), np.int32)
    a = 0
    for T, nans, excluded in cases:
        x[[a + k for k in nans], :] = np.nan
        ex[[a + k for k in excluded]] = 3
        a += T
    return x, lengths, ex


def test_sequences_do_not_see_each_other(pipe):
    joints, trans, lengths, names, ex, table = ec.noisy_call(25)
    for sigma in (0.0, 2.0):
        whole = pipe.gait_entropy(joints, lengths, trans, ex, sigma=sigma, **ec.RULE)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_entropy(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], sigma=sigma, **ec.RULE)
            assert ec.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]) and ec.same_counts(whole["counts"][q], alone["counts"][0]), names[q]
            assert ec.same_bits(whole["per_sequence"][q], alone["per_sequence"][0]) and ec.same_bits(whole["sampen"][q], alone["sampen"][0]), names[q]
            a += n
        reg = pipe.gait_regularity(joints, lengths, trans, ex, sigma=sigma)
        assert ec.same_bits(whole["per_frame"], reg["per_frame"])


def test_entropy_rows(pipe):
    counts = np.array([[[60, 40, 10], [50, 30, 30], [49, 30, 10]], [[60, 40, 0], [60, 0, 0], [60, 7, 3]], [[80, 9, 3], [70, 8, 2], [60, 7, 1]]], np.int64)
    out = pipe.entropy_rows(counts)
    want = [[math.log(40 / 10), math.log(30 / 30), math.nan], [math.nan, math.nan, math.log(7 / 3)], [math.log(9 / 3), math.log(8 / 2), math.log(7 / 1)]]
    assert ec.same_bits(out["sampen"], want) and out["sampen"][0, 1] == 0.0
    assert np.isnan(out["complexity"][:2]).all() and out["complexity"][2] == (0.0 + want[2][0] + want[2][1]) + want[2][2]
    assert ec.same_bits(pipe.entropy_rows(counts, min_templates=49)["sampen"][0, 2], math.log(30 / 10))
    assert np.isnan(pipe.entropy_rows(counts, min_templates=61)["sampen"][:2]).all()
    big = pipe.entropy_rows(np.array([[[10 ** 5, 2 ** 62 + 1, 2 ** 61 + 3]]], np.int64))      # the quotient of the integers, not of their doubles
    assert big["sampen"][0, 0] == math.log((2 ** 62 + 1) / (2 ** 61 + 3))
    for bad in (np.zeros((2, 3)), np.zeros((3,), np.int64), np.zeros((2, 4), np.int64)):
        with pytest.raises(ValueError, match="counts"):
            pipe.entropy_rows(bad)
    with pytest.raises(ValueError, match="min_templates"):
        pipe.entropy_rows(counts, min_templates=0)


def test_white_noise_against_the_closed_form(pipe):
    x = np.stack([ec.white_noise(seed) for seed in ec.WHITE_SEEDS[:4]], axis=1)
    out = pipe.gait_sampen(x, m=2, fraction=ec.WHITE_FRACTION, derivative=0, scales=2)
    for tau in (1, 2):
        bar, closed = 2.0 * ec.WHITE_MEASURED[tau], ec.white_closed(tau)
        miss = np.abs(out["sampen"][0, :, tau - 1] - closed)
        print(f"scale {tau}: SampEn {out['sampen'][0, :, tau - 1].tolist()}, closed form {closed:.5f}, worst miss {miss.max():.4f} (bar {bar:.4f})")
        assert (miss <= bar).all()
    assert abs(ec.white_closed(1) - 2.18513) < 5e-6


BAD = ((dict(m=0), "m outside [1, 4]"), (dict(m=5), "m outside [1, 4]"), (dict(fraction=0.0), "fraction must be finite and within (0, 10]"),
       (dict(fraction=-0.2), "fraction must be finite and within (0, 10]"), (dict(fraction=10.5), "fraction must be finite and within (0, 10]"),
       (dict(fraction=float("nan")), "fraction must be finite and within (0, 10]"), (dict(fraction=float("inf")), "fraction must be finite and within (0, 10]"),
       (dict(derivative=-1), "derivative outside [0, 2]"), (dict(derivative=3), "derivative outside [0, 2]"), (dict(scales=0), "scales outside [1, 8]"),
       (dict(scales=9), "scales outside [1, 8]"))
LONG = "sequence 0 has 32769 frames, more than 32768 (the work is quadratic in them)"


def test_bad_arguments_are_refused(pipe):
    joints, trans = rc.walker(30)
    for kw, why in BAD:
        for call in (lambda: pipe.gait_entropy(joints, **kw), lambda: pipe.gait_sampen(np.zeros((30, 4)), **kw)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == why
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(sigma=-1.0), "sigma"),
                     (dict(sigma=float("nan")), "sigma"), (dict(sigma=16.5), "sigma"), (dict(m=2.5), "whole"), (dict(scales=1.5), "whole"), (dict(trans=np.zeros((29, 3))), "trans"),
                     (dict(exclude=np.zeros(29, np.int32)), "exclude")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_entropy(joints, **kw)
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_entropy(np.zeros((3, 25, 2)))
    with pytest.raises(ValueError, match="signals"):
        pipe.gait_sampen(np.zeros((30, 3)))
    for call in (lambda: pipe.gait_sampen(np.zeros((32769 + 5, 4)), lengths=[32769, 5]), lambda: pipe.gait_entropy(np.zeros((32769, 25, 3), np.float32))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == LONG
    assert (pipe.gait_sampen(np.zeros((32768, 4)), scales=1)["counts"][0, :, 0] == (32764, 0, 0)).all()        # the longest is taken
    assert pipe.ENTROPY_CHANNELS == ("sep", "lift", "sway", "bob") and pipe.ENTROPY_COLUMNS == ("n", "mean", "sd", "r") and pipe.ENTROPY_COUNTS == ("templates", "B", "A")


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_entropy.h itself against the statement with sigma = 0: one file per sequence of the noisy call with both tables, with and without
    trans and exclude, over ec.RULES; the hand-made signal, the word-boundary runs and the straddled window on signals; every refusal, in the
    statement's words."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_entropy_check.cpp")
    exe = str(tmp_path / "gait_entropy_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for k, (m, d, scales) in enumerate(ec.RULES):
        J, with_trans = (25, True) if k % 2 == 0 else (49, False)
        rule = rule_of(m, d, scales)
        joints, trans, lengths, names, ex, table = ec.noisy_call(J)
        a = 0
        for name, n in zip(names, lengths):
            tr = trans[a:a + n] if with_trans else None
            e = ex[a:a + n] if k % 3 else None
            host = pipe.gait_entropy(joints[a:a + n], trans=tr, exclude=e, joints=table, **rule)
            files.append(ec.write_case(str(tmp_path / f"J{J}_{k}_{name}.bin"), joints[a:a + n], table, tr, None, e, rule, host))
            a += n
    x = ec.hand_signals()
    for k, (rule, _, _, _) in enumerate(ec.HAND_CASES):
        files.append(ec.write_case(str(tmp_path / f"hand{k}.bin"), None, gc.KINECTV2, None, x, None, rule, pipe.gait_sampen(x, **rule)))
    x, lengths, ex = ec_boundary_call()
    a = 0
    for k, n in enumerate(lengths):
        rule = rule_of(2, 2, 3, 0.5)
        files.append(ec.write_case(str(tmp_path / f"edge{k}.bin"), None, gc.KINECTV2, None, x[a:a + n], ex[a:a + n], rule, pipe.gait_sampen(x[a:a + n], None, ex[a:a + n], **rule)))
        a += n
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
    refused = [(ec.write_case(str(tmp_path / f"bad{k}.bin"), None, gc.KINECTV2, None, np.zeros((30, 4)), None, dict(ec.RULE, **kw), None), why) for k, (kw, why) in enumerate(BAD)]
    refused.append((ec.write_case(str(tmp_path / "long.bin"), None, gc.KINECTV2, None, np.zeros((32769, 4)), None, ec.RULE, None), LONG))
    r = subprocess.run([exe] + [path for path, _ in refused], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "ok" and lines[:-1] == [f"refused {path}: {why}" for path, why in refused], r.stdout[-4000:] + r.stderr[-4000:]
