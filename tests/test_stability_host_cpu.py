"""Local dynamic stability of the gait signals on the host: pipeline.gait_stability and pipeline.gait_divergence, the numpy statements,
against the yardstick in plain loops over every pair of tests/helpers/stability_checks.py (every integer, every bit), on the hand-made integer signals
whose neighbours and products are worked out in the helper, at the edge shapes, on the logistic map against ln 2 (the bar: twice the yardstick's own
miss, profiles/gait_stability_bounds.txt); pipeline.stability_rows; csrc/gait_stability.h, the arithmetic the kernels run, through
tests/helpers/gait_stability_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on files
this test writes; every refusal, in the same words from the statement and from the header.  Every figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import gait_checks as gc
from .helpers import regularity_checks as rc
from .helpers import stability_checks as sc


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def fit_of(rule):
    return dict(fit_lo=0, fit_hi=min(10, rule["horizon"]))


def equals_the_yardstick(out, signals, lengths, ex, rule):
    nn, pairs, mant = sc.yardstick_call(signals, lengths, ex, **rule)
    K = rule["horizon"]
    assert out["nn"].dtype == np.int32 and out["nn"].shape == (sum(lengths), 4) and out["pairs"].dtype == np.int64
    assert out["pairs"].shape == (len(lengths), 4, K + 1, 2) and out["mant"].shape == (len(lengths), 4, K + 1)
    assert sc.same_ints(out["nn"], nn) and sc.same_ints(out["pairs"], pairs) and sc.same_bits(out["mant"], mant), rule
    for q in range(len(lengths)):
        for ch in range(4):
            div, lam = sc.yardstick_rows(pairs[q, ch].tolist(), mant[q, ch].tolist(), **fit_of(rule))
            assert sc.same_bits(out["divergence"][q, ch], div) and sc.same_bits(out["lambda"][q, ch], lam)
    return nn, pairs, mant


@pytest.mark.parametrize("J", (25, 49))
def test_statement_against_the_yardstick(pipe, J):
    joints, trans, lengths, names, ex, table = sc.noisy_call(J)
    want_frame = {True: rc.signals_of(joints, trans, table), False: rc.signals_of(joints, None, table)}
    for with_trans, with_ex in ((True, True), (True, False), (False, True), (False, False)):
        for values in (sc.RULES if with_trans and with_ex and J == 25 else sc.RULES[:2]):
            rule = sc.rule_of(*values)
            out = pipe.gait_stability(joints, lengths, trans if with_trans else None, ex if with_ex else None, joints=table, **rule)
            assert sc.same_bits(out["per_frame"], want_frame[with_trans])
            nn, pairs, mant = equals_the_yardstick(out, want_frame[with_trans], lengths, ex if with_ex else None, rule)
            if values[3] == 500:                               # a Theiler window larger than every E: no candidate anywhere
                assert (nn == -1).all() and (pairs == 0).all() and (mant == 1.0).all()
    full = pipe.gait_stability(joints, lengths, trans, None, joints=table)
    seq = dict(zip(names, full["pairs"]))
    print("walk400_back: n", seq["walk400_back"][:, :, 0].min(axis=1).tolist(), "lambda", full["lambda"][-1].tolist())
    assert (seq["walk400_back"][:, :, 0] >= 300).all() and np.isfinite(full["lambda"][names.index("walk400_back")]).all()
    assert (seq["one"] == 0).all() and (seq["nineteen"] == 0).all() and (seq["standing64"] == 0).all()
    assert np.isnan(full["lambda"][names.index("standing64")]).all()


def test_hand_made_signals(pipe):
    x = sc.hand_signals(sc.HAND_PERIODIC_X)
    out = pipe.gait_divergence(x, fit_hi=1, min_pairs=10, **sc.HAND_PERIODIC_RULE)
    want = [sc.exact_mantissa(p) for p in sc.HAND_PERIODIC_PRODUCTS]
    print(out["nn"][:, 0].tolist(), out["pairs"][0, 0].tolist(), out["mant"][0, 0].tolist(), want)
    for ch in range(4):
        assert out["nn"][:, ch].tolist() == sc.HAND_PERIODIC_NN
        assert out["pairs"][0, ch].tolist() == [[sc.HAND_PERIODIC_N, S] for _, S in want] and out["mant"][0, ch].tolist() == [P for P, _ in want]
    half = [math.log(p) / (2 * sc.HAND_PERIODIC_N) for p in sc.HAND_PERIODIC_PRODUCTS]        # the mean logarithm of the distance itself
    assert np.abs(out["divergence"][0, 0] - half).max() < 1e-14 and abs(out["lambda"][0, 0] - (half[1] - half[0]) * 20.0) < 1e-12
    nn, pairs, mant = sc.yardstick(x[:, 0], None, **sc.HAND_PERIODIC_RULE)
    assert nn == sc.HAND_PERIODIC_NN and pairs == [[sc.HAND_PERIODIC_N, S] for _, S in want] and mant == [P for P, _ in want]
    xb = sc.hand_signals(sc.HAND_BROKEN_X)
    out = pipe.gait_divergence(xb, fit_hi=2, **sc.HAND_BROKEN_RULE)
    assert out["nn"][:, 2].tolist() == sc.HAND_BROKEN_NN and out["pairs"][0, 2].tolist() == [list(p) for p in sc.HAND_BROKEN_PAIRS]
    assert out["mant"][0, 2].tolist() == list(sc.HAND_BROKEN_MANT) and np.isnan(out["divergence"]).all() and np.isnan(out["lambda"]).all()      # fewer than 50 pairs
    nn, pairs, mant = sc.yardstick(xb[:, 0], None, **sc.HAND_BROKEN_RULE)
    assert nn == sc.HAND_BROKEN_NN and pairs == [list(p) for p in sc.HAND_BROKEN_PAIRS] and mant == list(sc.HAND_BROKEN_MANT)
    three = pipe.gait_divergence(np.concatenate([x, xb[:9], x]), lengths=[30, 9, 30], fit_hi=1, **sc.HAND_PERIODIC_RULE)
    assert three["nn"][:30, 0].tolist() == sc.HAND_PERIODIC_NN and three["nn"][39:, 0].tolist() == sc.HAND_PERIODIC_NN
    alone = pipe.gait_divergence(x, fit_hi=1, **sc.HAND_PERIODIC_RULE)
    assert sc.same_ints(three["pairs"][0], alone["pairs"][0]) and sc.same_ints(three["pairs"][2], alone["pairs"][0]) and sc.same_bits(three["mant"][2], alone["mant"][0])


def test_edge_shapes(pipe):
    rng = np.random.default_rng(7)
    for T, rule, E in ((1, sc.RULE, 0), (8, sc.RULE, 0), (9, sc.RULE, 0), (28, sc.RULE, 0), (29, sc.RULE, 1), (113, sc.rule_of(0, 8, 16, 0, 1), 0), (114, sc.rule_of(0, 8, 16, 0, 1), 1)):
        x = rng.standard_normal((T, 4))                         # one frame; span >= T; M <= K; the first E = 1, which has no other point to meet
        out = pipe.gait_divergence(x, fit_hi=1, **rule)
        assert (out["nn"] == -1).all() and (out["pairs"] == 0).all() and (out["mant"] == 1.0).all() and np.isnan(out["divergence"]).all() and np.isnan(out["lambda"]).all()
        assert max(T - (rule["dim"] - 1) * rule["lag"] - rule["horizon"], 0) == E
    x = rng.standard_normal((40, 4))
    equals_the_yardstick(pipe.gait_divergence(x, **sc.rule_of(1, 2, 1, 3, 20)), x, [40], None, sc.rule_of(1, 2, 1, 3, 20))
    # the standing body: every D2 is 0, so nothing is a neighbour
    joints, trans = rc.walker(64, still=True)
    for d in (0, 1):
        still = pipe.gait_stability(joints, trans=trans, **dict(sc.RULE, derivative=d))
        assert np.isfinite(still["per_frame"]).all() and (still["nn"] == -1).all() and (still["pairs"] == 0).all() and (still["mant"] == 1.0).all()
    # an infinite distance is a candidate and wins only where nothing finite does, and does not count in the walk
    x = np.zeros((12, 4))
    x[:, 0] = [0, 1e200, 0, 0, -1e200, 0, 0, 1e200, 0, 0, 0, 0]
    rule = sc.rule_of(0, 2, 1, 0, 1)
    equals_the_yardstick(pipe.gait_divergence(x, fit_hi=1, **rule), x, [12], None, rule)


def test_runs_at_the_word_boundary(pipe):
    """Validity runs that begin and end at frames 63, 64 and 65, by NaN and by exclude."""
    x, lengths, ex = sc.boundary_call()
    for values in ((1, 5, 2, 20, 20), (0, 2, 1, 0, 1), (2, 3, 16, 5, 20)):
        rule = sc.rule_of(*values)
        nn, pairs, _ = equals_the_yardstick(pipe.gait_divergence(x, lengths, ex, **rule), x, lengths, ex, rule)
    assert (pairs[:5, :, 0, 0] > 20).all() and (nn[:130, 0] >= 0).sum() > 20


def test_sequences_do_not_see_each_other(pipe):
    joints, trans, lengths, names, ex, table = sc.noisy_call(25)
    for sigma in (0.0, 2.0):
        whole = pipe.gait_stability(joints, lengths, trans, ex, sigma=sigma)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_stability(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], sigma=sigma)
            assert sc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]) and sc.same_ints(whole["nn"][a:a + n], alone["nn"]), names[q]
            assert sc.same_ints(whole["pairs"][q], alone["pairs"][0]) and sc.same_bits(whole["mant"][q], alone["mant"][0]), names[q]
            assert sc.same_bits(whole["lambda"][q], alone["lambda"][0]), names[q]
            a += n
        reg = pipe.gait_regularity(joints, lengths, trans, ex, sigma=sigma)
        assert sc.same_bits(whole["per_frame"], reg["per_frame"])


def test_stability_rows(pipe):
    K = 12
    n = np.full(K + 1, 60, np.int64)
    S = np.arange(K + 1, dtype=np.int64) * 120 - 600           # the logarithm grows by ln 2 a frame: (120 ln 2) / (2 60)
    pairs = np.stack([n, S], axis=-1)[None]
    mant = np.full((1, K + 1), 0.5)
    out = pipe.stability_rows(pairs, mant, fps=1.0)
    want = [(math.log(0.5) + int(s) * math.log(2.0)) / 120 for s in S]
    assert sc.same_bits(out["divergence"][0], want) and abs(out["lambda"][0] - math.log(2.0)) < 1e-14
    assert abs(pipe.stability_rows(pairs, mant)["lambda"][0] - 20.0 * math.log(2.0)) < 1e-12 and out["divergence"].shape == (1, K + 1) and out["lambda"].shape == (1,)
    div, lam = sc.yardstick_rows(pairs[0].tolist(), mant[0].tolist(), fps=1.0)
    assert sc.same_bits(out["divergence"][0], div) and sc.same_bits(out["lambda"][0], lam)
    few = pairs.copy()
    few[0, 11, 0] = 49                                          # outside the window 0 .. 10: lambda stays
    out = pipe.stability_rows(few, mant, fps=1.0)
    assert np.isnan(out["divergence"][0, 11]) and np.isfinite(out["lambda"][0])
    few[0, 4, 0] = 49                                           # inside it
    out = pipe.stability_rows(few, mant, fps=1.0)
    assert np.isnan(out["divergence"][0, [4, 11]]).all() and np.isnan(out["lambda"][0])
    assert np.isfinite(pipe.stability_rows(few, mant, fps=1.0, min_pairs=49)["lambda"][0]) and np.isfinite(pipe.stability_rows(few, mant, fit_lo=5, fit_hi=10)["lambda"][0])
    assert np.isnan(pipe.stability_rows(pairs, mant, min_pairs=61)["divergence"]).all()
    big = pipe.stability_rows(np.array([[[2 ** 40, -(2 ** 50)], [2 ** 40, 2 ** 50]]], np.int64), np.array([[0.75, 0.75]]), fit_hi=1)
    assert big["divergence"][0, 1] == (math.log(0.75) + 2 ** 50 * math.log(2.0)) / 2 ** 41
    for kw in (dict(fit_lo=-1), dict(fit_lo=3, fit_hi=3), dict(fit_lo=4, fit_hi=3), dict(fit_hi=K + 1), dict(fit_lo=0.5)):
        with pytest.raises(ValueError, match="fit window"):
            pipe.stability_rows(pairs, mant, **kw)
    pipe.stability_rows(pairs, mant, fit_lo=K - 1, fit_hi=K)
    for bad_pairs, bad_mant in ((np.zeros((1, 3, 2)), np.ones((1, 3))), (np.zeros((2,), np.int64), np.ones(())), (np.zeros((1, 3, 3), np.int64), np.ones((1, 3))),
                                (np.zeros((1, 3, 2), np.int64), np.ones((1, 4)))):
        with pytest.raises(ValueError, match="pairs"):
            pipe.stability_rows(bad_pairs, bad_mant, fit_hi=1)
    with pytest.raises(ValueError, match="min_pairs"):
        pipe.stability_rows(pairs, mant, min_pairs=0)
    with pytest.raises(ValueError, match="fps"):
        pipe.stability_rows(pairs, mant, fps=0.0)


def test_logistic_map_against_ln_2(pipe):
    x = np.stack([sc.logistic(seed) for seed in sc.LOGISTIC_SEEDS[:4]], axis=1)
    out = pipe.gait_divergence(x, **sc.LOGISTIC_RULE, **sc.LOGISTIC_FIT)
    bar = 2.0 * sc.LOGISTIC_MEASURED
    miss = np.abs(out["lambda"][0] - math.log(2.0))
    print(f"lambda {out['lambda'][0].tolist()}, ln 2 {math.log(2.0):.5f}, worst miss {miss.max():.4f} (bar {bar:.4f}), n {out['pairs'][0, :, 0, 0].tolist()}")
    assert (miss <= bar).all() and (out["pairs"][0, :, :5, 0] >= 900).all()
    nn, pairs, mant = sc.yardstick(x[:, 0], None, **sc.LOGISTIC_RULE)
    assert sc.same_ints(out["nn"][:, 0], np.array(nn, np.int32)) and sc.same_ints(out["pairs"][0, 0], np.array(pairs)) and sc.same_bits(out["mant"][0, 0], mant)


BAD = ((dict(derivative=-1), "derivative outside [0, 2]"), (dict(derivative=3), "derivative outside [0, 2]"), (dict(dim=1), "dim outside [2, 8]"), (dict(dim=9), "dim outside [2, 8]"),
       (dict(lag=0), "lag outside [1, 16]"), (dict(lag=17), "lag outside [1, 16]"), (dict(theiler=-1), "theiler outside [0, 4096]"), (dict(theiler=4097), "theiler outside [0, 4096]"),
       (dict(horizon=0), "horizon outside [1, 63]"), (dict(horizon=64), "horizon outside [1, 63]"))
LONG = "sequence 0 has 32769 frames, more than 32768 (the work is quadratic in them)"


def test_bad_arguments_are_refused(pipe):
    joints, trans = rc.walker(30)
    for kw, why in BAD:
        for call in (lambda: pipe.gait_stability(joints, **kw), lambda: pipe.gait_divergence(np.zeros((30, 4)), **kw)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == why
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(sigma=-1.0), "sigma"),
                     (dict(sigma=float("nan")), "sigma"), (dict(sigma=16.5), "sigma"), (dict(dim=2.5), "whole"), (dict(horizon=1.5), "whole"), (dict(trans=np.zeros((29, 3))), "trans"),
                     (dict(exclude=np.zeros(29, np.int32)), "exclude"), (dict(fit_hi=21), "fit window"), (dict(horizon=5, fit_hi=10), "fit window")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_stability(joints, **kw)
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_stability(np.zeros((3, 25, 2)))
    with pytest.raises(ValueError, match="signals"):
        pipe.gait_divergence(np.zeros((30, 3)))
    for call in (lambda: pipe.gait_divergence(np.zeros((32769 + 5, 4)), lengths=[32769, 5]), lambda: pipe.gait_stability(np.zeros((32769, 25, 3), np.float32))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == LONG
    assert pipe.gait_divergence(np.zeros((30, 4)), horizon=5)["lambda"].shape == (1, 4)      # the default window ends at the horizon where that is shorter
    assert pipe.STABILITY_CHANNELS == ("sep", "lift", "sway", "bob") and pipe.STABILITY_PAIRS == ("n", "exponent") and pipe.STABILITY_MAX_FRAMES == 32768


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_stability.h itself against the statement with sigma = 0: one file per sequence of the noisy call with both tables, with and without
    trans and exclude, over sc.RULES; the hand-made signals, the word-boundary runs and a sequence of more than one search tile on signals; every
    refusal, in the statement's words."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_stability_check.cpp")
    exe = str(tmp_path / "gait_stability_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for k, values in enumerate(sc.RULES):
        J, with_trans = (25, True) if k % 2 == 0 else (49, False)
        rule = sc.rule_of(*values)
        joints, trans, lengths, names, ex, table = sc.noisy_call(J)
        a = 0
        for name, n in zip(names, lengths):
            tr = trans[a:a + n] if with_trans else None
            e = ex[a:a + n] if k % 3 else None
            host = pipe.gait_stability(joints[a:a + n], trans=tr, exclude=e, joints=table, **rule)
            files.append(sc.write_case(str(tmp_path / f"J{J}_{k}_{name}.bin"), joints[a:a + n], table, tr, None, e, rule, host))
            a += n
    for k, (x, rule) in enumerate(sc.HAND_CASES):
        x = sc.hand_signals(x)
        files.append(sc.write_case(str(tmp_path / f"hand{k}.bin"), None, gc.KINECTV2, None, x, None, rule, pipe.gait_divergence(x, fit_hi=1, **rule)))
    x, lengths, ex = sc.boundary_call()
    a = 0
    for k, n in enumerate(lengths):
        host = pipe.gait_divergence(x[a:a + n], None, ex[a:a + n], **sc.RULE)
        files.append(sc.write_case(str(tmp_path / f"edge{k}.bin"), None, gc.KINECTV2, None, x[a:a + n], ex[a:a + n], sc.RULE, host))
        a += n
    x = np.random.default_rng(1025).standard_normal((1025 + 8 + 20 + 1, 4))      # E = the tile + 1 at the default rule
    files.append(sc.write_case(str(tmp_path / "tile.bin"), None, gc.KINECTV2, None, x, None, sc.RULE, pipe.gait_divergence(x, **sc.RULE)))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
    refused = [(sc.write_case(str(tmp_path / f"bad{k}.bin"), None, gc.KINECTV2, None, np.zeros((30, 4)), None, dict(sc.RULE, **kw), None), why) for k, (kw, why) in enumerate(BAD)]
    refused.append((sc.write_case(str(tmp_path / "long.bin"), None, gc.KINECTV2, None, np.zeros((32769, 4)), None, sc.RULE, None), LONG))
    r = subprocess.run([exe] + [path for path, _ in refused], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "ok" and lines[:-1] == [f"refused {path}: {why}" for path, why in refused], r.stdout[-4000:] + r.stderr[-4000:]
