"""Arm swing and inter-limb coordination on the host: pipeline.gait_coordination and pipeline.gait_cross_welch, the numpy statements,
against the yardstick by numpy.fft of tests/helpers/coordination_checks.py (the bars: 8 times what the yardstick's own renderings miss one another by
over the shape set, profiles/gait_coordination_bounds.txt -- never measured from the statement) and, where scipy imports, against scipy.signal.csd
and scipy.signal.coherence themselves; the conditions on the inputs, on the yardstick alone; the exact properties that need no measured number;
pipeline.coordination_rows; the white-noise anchor; csrc/gait_coordination.h, the arithmetic the kernels run, through
tests/helpers/gait_coordination_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on
files this test writes, whose printed bits must be the statement's; every refusal, in the same words from the statement and from the header.  Every
figure is printed before it is asserted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import coordination_checks as cc

PAIR = {name: k for k, name in enumerate(("used", "peak_bin", "peak_hz", "cross_amplitude", "coherence_peak", "phase_peak", "phase_deviation", "lag_seconds",
                                          "coherence_band", "coherence_bins"))}


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def against_yardstick(out, signals, lengths, ex, rule, noisy):
    """The worst of every barred figure of a statement's output over the sequences of one case."""
    worst = {k: 0.0 for k in cc.BARS}
    a = 0
    for q, T in enumerate(lengths):
        want = cc.yardstick(signals[a:a + T], None if ex is None else ex[a:a + T], **rule)
        assert out["limbs"][q, :, :3].tolist() == [[want["n"], want["candidates"], want["used"]]] * 4 and (out["pairs"][q, :, 0] == want["used"]).all(), q
        ra, rc = cc.ratios(out["auto"][q], out["cross"][q, :, :, 0], out["cross"][q, :, :, 1], want)
        worst["auto"], worst["cross"] = max(worst["auto"], ra), max(worst["cross"], rc)
        if noisy and want["used"]:
            fin = np.isfinite(want["peak_bin"])
            assert (out["pairs"][q, fin, PAIR["peak_bin"]] == want["peak_bin"][fin]).all() and np.isnan(out["pairs"][q, ~fin, PAIR["peak_bin"]]).all(), q
            for k in ("coherence_peak", "coherence_band", "phase_peak"):
                if fin.any():
                    worst[k] = max(worst[k], float(np.abs(out["pairs"][q, fin, PAIR[k]] - want[k][fin]).max()))
        a += T
    return worst


def test_statement_against_the_yardstick(pipe):
    worst = {k: 0.0 for k in cc.BARS}
    for name, signals, lengths, ex, rule, noisy in cc.shape_set():
        here = against_yardstick(pipe.gait_cross_welch(signals, lengths, ex, **rule), signals, lengths, ex, rule, noisy)
        print(name, {k: f"{v:.3e}" for k, v in here.items()})
        worst = {k: max(worst[k], here[k]) for k in worst}
    print("worst", {k: f"{v:.3e} of {cc.BARS[k]:.2e}" for k, v in worst.items()})
    assert all(worst[k] <= cc.BARS[k] for k in worst)
    assert all(cc.BARS[k] == 8.0 * cc.MEASURED[k] for k in cc.BARS) and cc.MEASURED["auto"] < 1e-13 and cc.MEASURED["cross"] < 1e-13 and cc.MEASURED["phase_peak"] < 1e-11


def test_scipy_where_it_imports(pipe):
    """One valid run: scipy averages the segments of ONE run, as the statement does where the signals have one."""
    x = np.random.default_rng(1973).standard_normal((400, 4))
    x[:, 1] += 0.7 * np.roll(x[:, 0], 3)
    x[:, 3] -= 0.5 * x[:, 2]
    if cc.scipy_run(x) is None:
        print("scipy does not import here: the numpy.fft yardstick stands alone")
        return
    for d, L, hop, N, m in ((0, 64, 32, 256, 4), (0, 8, 1, 8, 4), (0, 256, 32, 1024, 2), (0, 64, 64, 514, 4)):
        out = pipe.gait_cross_welch(x, **cc.rule_of(d, L, hop, N, m))
        f, csd, coh = cc.scipy_run(x, 20.0, L, hop, N)
        top = out["auto"][0].max(axis=1)
        for p, (a, b) in enumerate(cc.PAIRS):
            den = np.sqrt(top[a] * top[b])
            miss = max(np.abs(out["cross"][0, p, :, 0] - csd[p].real).max(), np.abs(out["cross"][0, p, :, 1] - csd[p].imag).max()) / den
            mine = (out["cross"][0, p, :, 0] ** 2 + out["cross"][0, p, :, 1] ** 2) / (out["auto"][0, a] * out["auto"][0, b])
            print(f"scipy: segment {L} hop {hop} nfft {N} pair {p}: csd ratio {miss:.3e}, coherence {np.abs(mine - coh[p]).max():.3e}")
            assert miss <= cc.BARS["cross"] and np.abs(mine - coh[p]).max() <= 1e-12      # the sign of Im is scipy.signal.csd(a, b)'s
        assert np.allclose(f, out["freqs"], rtol=1e-15, atol=0)


@pytest.mark.parametrize("J", (25, 49))
def test_conditions_on_the_inputs_by_the_yardstick_alone(J):
    joints, lengths, names, ex, table = cc.noisy_call(J)
    assert names[-1] == "walk400" and lengths[-1] == 400
    y = cc.yardstick(cc.angles_of(joints[-400:], table), None, **cc.RULE)
    asym = 100.0 * abs(y["amplitude"][0] - y["amplitude"][1]) / (0.5 * (y["amplitude"][0] + y["amplitude"][1]))
    print(J, y["peak_bin"], y["coherence_peak"], y["phase_deviation"], y["amplitude"], asym)
    assert y["used"] == 11 and (y["peak_bin"] == 12).all() and (y["coherence_peak"] >= 0.9).all() and (y["phase_deviation"] <= 5.0).all()
    assert abs(y["amplitude"][0] - 18.0) <= 0.5 and abs(y["amplitude"][1] - 10.8) <= 0.5 and (np.abs(y["amplitude"][2:] - 25.0) <= 0.5).all() and abs(asym - 50.0) <= 2.0


@pytest.mark.parametrize("J", (25, 49))
def test_per_frame_is_gait_kinematics_s_and_the_call_is_the_hook_on_it(pipe, J):
    joints, lengths, names, ex, table = cc.noisy_call(J)
    events = np.zeros(len(joints), np.int32)
    for sigma in (0.0, 2.0):
        kin = pipe.gait_kinematics(joints, events, lengths, sigma=sigma, joints=table)["per_frame"][:, cc.KIN_COLUMNS]
        for r in cc.RULES[:3] if sigma == 0.0 else cc.RULES[:1]:
            out = pipe.gait_coordination(joints, lengths, ex, sigma=sigma, joints=table, **cc.rule_of(*r))
            hook = pipe.gait_cross_welch(kin, lengths, ex, **cc.rule_of(*r))
            assert cc.same_bits(out["per_frame"], kin) and out["auto"].shape == (7, 4, r[3] // 2 + 1) and out["cross"].shape == (7, 6, r[3] // 2 + 1, 2)
            assert out["limbs"].shape == (7, 4, 13) and out["pairs"].shape == (7, 6, 10)
            assert all(cc.same_bits(out[k], hook[k]) for k in ("auto", "cross", "limbs", "pairs", "freqs") + pipe.COORDINATION_ROWS)
    full = pipe.gait_coordination(joints, lengths, joints=table)      # the defaults
    q = names.index("walk400")
    print(full["pairs"][q], full["amplitude"][q], full["arm_asymmetry"][q], full["leg_asymmetry"][q], full["arm_leg_ratio"][q], full["phase_deviation_mean"][q])
    assert (full["limbs"][q, :, :3] == [400, 11, 11]).all() and (full["pairs"][q, :, 1] == 12).all() and (full["pairs"][q, :, PAIR["coherence_peak"]] >= 0.9).all()
    assert (full["pairs"][q, :, PAIR["phase_deviation"]] <= 5.0).all() and abs(full["arm_asymmetry"][q] - 50.0) <= 2.0 and full["leg_asymmetry"][q] < 2.0
    assert cc.same_bits(full["limbs"][q, :, 12], 120.0 * full["limbs"][q, :, 6]) and (np.abs(full["limbs"][q, :, 6] - 20.0 / 21.7) < 0.5 * 20.0 / 256).all()
    standing = names.index("standing64")
    assert np.isnan(full["auto"][standing]).all() and np.isnan(full["cross"][standing]).all() and np.isnan(full["pairs"][standing, :, 1:]).all()
    assert (full["limbs"][standing, :, :5] == [64, 1, 0, np.nan, np.nan]).sum() == 12      # one segment of 64 is fewer than four
    still = pipe.gait_coordination(joints[sum(lengths[:standing]):][:64], joints=table, **cc.rule_of(0, 8, 4, 32))
    assert (still["auto"] == 0).all() and (still["limbs"][0, :, :5] == [64, 15, 15, 0, 0]).all() and np.isnan(still["limbs"][0, :, 5:]).all()
    assert (still["pairs"][0, :, 0] == 15).all() and np.isnan(still["pairs"][0, :, 1:]).all() and (still["amplitude"] == 0).all()
    assert np.isnan(still["arm_asymmetry"]).all() and np.isnan(still["arm_leg_ratio"]).all() and np.isnan(still["phase_deviation_mean"]).all()
    assert (full["limbs"][names.index("one"), :, :3] == [1, 0, 0]).all() and np.isnan(full["auto"][names.index("one")]).all()


def test_all_valid_signals_give_gait_welch_s_psd(pipe):
    x = np.random.default_rng(4).standard_normal((700, 4))
    lengths = [400, 65, 235]
    for d, L, hop, N, m in cc.RULES:
        rule = cc.rule_of(d, L, hop, N, m)
        out, welch = pipe.gait_cross_welch(x, lengths, **rule), pipe.gait_welch(x, lengths, **rule)
        assert cc.same_bits(out["auto"], welch["psd"]) and cc.same_bits(out["limbs"][:, :, :12], welch["per_sequence"][:, :, :12]), rule
        assert cc.same_bits(out["limbs"][:, :3, 12], welch["per_sequence"][:, :3, 12])      # gait_welch's bob counts strides, a limb always steps


def test_hand_cases(pipe):
    a = cc.hand_signals()
    rule = cc.rule_of(0, 64, 32, 64)
    same = pipe.gait_cross_welch(np.stack([a, a, a, a], axis=1), **rule)
    assert (same["cross"][0, :, :, 1] == 0).all() and not np.signbit(same["cross"][0, :, :, 1]).any()      # every Im exactly +0
    assert (same["pairs"][0, :, PAIR["coherence_peak"]] == 1.0).all() and (same["pairs"][0, :, PAIR["phase_peak"]] == 0).all() and not np.signbit(same["pairs"][0, :, PAIR["phase_peak"]]).any()
    assert (same["pairs"][0, :, PAIR["coherence_band"]] == 1.0).all() and (same["pairs"][0, :, PAIR["peak_bin"]] == 4).all()
    assert (same["pairs"][0, [2, 3], PAIR["phase_deviation"]] == 0).all() and (same["pairs"][0, [0, 1, 4, 5], PAIR["phase_deviation"]] == 180.0).all()
    anti = pipe.gait_cross_welch(np.stack([a, -a, a, -a], axis=1), **rule)
    print(anti["pairs"][0])
    assert (anti["cross"][0, :, :, 1] == 0).all() and (anti["pairs"][0, :, PAIR["coherence_peak"]] == 1.0).all()
    assert (anti["pairs"][0, [0, 1], PAIR["phase_deviation"]] < 1e-12).all() and (np.abs(anti["pairs"][0, [0, 1, 2, 3], PAIR["phase_peak"]]) > 179.9).all()      # (0,1), (2,3): antiphase, as expected
    assert (np.abs(anti["pairs"][0, [2, 3], PAIR["phase_deviation"]] - 180.0) < 1e-12).all()      # (0,3), (1,2) are expected in phase
    assert (anti["pairs"][0, [4, 5], PAIR["phase_peak"]] == 0).all() and (anti["pairs"][0, [4, 5], PAIR["phase_deviation"]] == 180.0).all()      # (0,2), (1,3): in phase, expected 180
    late = np.stack([a[2:], a[:-2], a[2:], a[:-2]], axis=1)       # b(t) = a(t - 2): b lags a by 2 frames, at bin 4 of 64 by 2 * 4 / 64 of a turn = 45 degrees
    out = pipe.gait_cross_welch(late, **rule)
    print(out["pairs"][0, 0])
    assert out["pairs"][0, 0, PAIR["peak_bin"]] == 4 and abs(out["pairs"][0, 0, PAIR["phase_peak"]] + 45.0) < 1.0      # the noise is not periodic in the segment
    pure = np.sin(2.0 * np.pi * 4.0 * np.arange(402) / 64.0)
    out = pipe.gait_cross_welch(np.stack([pure[2:], pure[:-2], pure[2:], pure[:-2]], axis=1), **rule)
    print(out["pairs"][0, 0])
    assert abs(out["pairs"][0, 0, PAIR["phase_peak"]] + 45.0) <= cc.BARS["phase_peak"] and abs(out["pairs"][0, 0, PAIR["lag_seconds"]] + 2.0 / 20.0) < 1e-12      # a negative phase: b lags a
    assert abs(out["pairs"][0, 0, PAIR["phase_deviation"]] - 135.0) < 1e-9 and abs(out["pairs"][0, 2, PAIR["phase_deviation"]] - 45.0) < 1e-9
    # a NaN stretch in ONE channel removes those segments from all pairs and all limbs
    x = np.random.default_rng(8).standard_normal((400, 4))
    hole = x.copy()
    hole[150:190, 2] = np.nan
    whole, holed = pipe.gait_cross_welch(x, **cc.RULE), pipe.gait_cross_welch(hole, **cc.RULE)
    ex = np.zeros(400, np.int32)
    ex[150:190] = 1
    masked = pipe.gait_cross_welch(x, exclude=ex, **cc.RULE)
    assert (whole["limbs"][0, :, :3] == [400, 11, 11]).all() and (holed["limbs"][0, :, :3] == [360, 3 + 5, 8]).all() and (holed["pairs"][0, :, 0] == 8).all()
    assert all(cc.same_bits(holed[k], masked[k]) for k in ("auto", "cross", "limbs", "pairs"))


def test_edge_shapes(pipe):
    rng = np.random.default_rng(3)
    one = pipe.gait_cross_welch(rng.standard_normal((1, 4)), **cc.RULE)
    assert (one["limbs"][0, :, :3] == [1, 0, 0]).all() and np.isnan(one["auto"]).all() and np.isnan(one["cross"]).all() and np.isnan(one["pairs"][0, :, 1:]).all()
    x = rng.standard_normal((159, 4))                           # 3 candidates < min_segments = 4; 160 frames hold 4
    few = pipe.gait_cross_welch(x, **cc.RULE)
    assert (few["limbs"][0, :, :3] == [159, 3, 0]).all() and np.isnan(few["auto"]).all() and (few["pairs"][0, :, 0] == 0).all() and np.isnan(few["amplitude"]).all()
    enough = pipe.gait_cross_welch(np.concatenate([x, x[:1]]), **cc.RULE)
    assert (enough["limbs"][0, :, :3] == [160, 4, 4]).all() and np.isfinite(enough["auto"]).all() and np.isfinite(enough["pairs"]).all()
    for segment, hop, nfft in ((64, 32, 256), (8, 4, 32), (64, 8, 64)):
        x, lengths, ex = cc.runs_call(segment, hop)
        for d in (0, 1, 2):
            rule = cc.rule_of(d, segment, hop, nfft, 2)
            out = pipe.gait_cross_welch(x, lengths, ex, **rule)
            worst = against_yardstick(out, x, lengths, ex, rule, False)
            assert worst["auto"] <= cc.BARS["auto"] and worst["cross"] <= cc.BARS["cross"], (rule, worst)
            if d == 0:      # a run of L - 1 frames lays no segment, one of L one, one of L + hop two; behind each lies one more run of L
                assert out["limbs"][9:, 0, 1].tolist() == [1, 0, 2, 1, 3, 2]


def test_sequences_do_not_see_each_other(pipe):
    joints, lengths, names, ex, table = cc.noisy_call(25)
    for sigma in (0.0, 2.0):
        whole = pipe.gait_coordination(joints, lengths, ex, sigma=sigma, joints=table, **cc.rule_of(1, 8, 4, 32))
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_coordination(joints[a:a + n], None, ex[a:a + n], sigma=sigma, joints=table, **cc.rule_of(1, 8, 4, 32))
            assert cc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]), names[q]
            assert all(cc.same_bits(whole[k][q], alone[k][0]) for k in ("auto", "cross", "limbs", "pairs") + pipe.COORDINATION_ROWS), names[q]
            a += n


def test_coordination_rows(pipe):
    limbs, pairs = np.full((2, 4, 13), np.nan), np.full((2, 6, 10), np.nan)
    limbs[0, :, 3] = (162.0, 58.32, 312.5, 312.5)                # amplitudes 18, 10.8, 25, 25
    pairs[0, :, 6] = (1.0, 2.0, np.nan, 3.0, np.nan, 6.0)
    limbs[1, :, 3] = (0.0, 0.0, 8.0, np.nan)
    out = pipe.coordination_rows(limbs, pairs)
    print(out)
    assert sorted(out) == sorted(pipe.COORDINATION_ROWS) and out["amplitude"].shape == (2, 4) and out["arm_asymmetry"].shape == (2,)
    assert np.allclose(out["amplitude"][0], (18.0, 10.8, 25.0, 25.0), rtol=1e-15) and abs(out["arm_asymmetry"][0] - 50.0) < 1e-12 and out["leg_asymmetry"][0] == 0.0
    assert abs(out["arm_leg_ratio"][0] - 14.4 / 25.0) < 1e-15 and out["phase_deviation_mean"][0] == 3.0
    assert out["amplitude"][1].tolist()[:3] == [0.0, 0.0, 4.0] and np.isnan(out["amplitude"][1, 3])
    assert all(np.isnan(out[k][1]) for k in ("arm_asymmetry", "leg_asymmetry", "arm_leg_ratio", "phase_deviation_mean"))      # no denominator is positive
    assert pipe.coordination_rows(limbs.reshape(1, 2, 4, 13), pairs.reshape(1, 2, 6, 10))["amplitude"].shape == (1, 2, 4)
    for bad in ((np.zeros((2, 4, 12)), np.zeros((2, 6, 10))), (np.zeros((2, 4, 13)), np.zeros((3, 6, 10))), (np.zeros((4, 13)), np.zeros((6, 9)))):
        with pytest.raises(ValueError, match="limbs"):
            pipe.coordination_rows(*bad)


def test_white_noise_anchor(pipe):
    worst = 0.0
    for seed in cc.WHITE_SEEDS[:4]:
        out = pipe.gait_cross_welch(cc.white_noise(seed), **cc.WHITE_RULE)
        assert (out["limbs"][0, :, 2] == cc.WHITE_K).all()
        mean = cc.white_mean(out["auto"][0], out["cross"][0, :, :, 0], out["cross"][0, :, :, 1])
        print(f"seed {seed}: mean coherence {mean:.5f}, 1 / K {1.0 / cc.WHITE_K:.5f}, bar {cc.WHITE_BAR}")
        worst = max(worst, abs(mean - 1.0 / cc.WHITE_K))
    assert worst <= cc.WHITE_BAR and cc.WHITE_BAR == 2.0 * cc.WHITE_MEASURED < 1.0 / cc.WHITE_K


def test_the_record_of_the_bounds_names_the_constants():
    text = open(os.path.join(ROOT, "profiles", "gait_coordination_bounds.txt")).read()
    for k, v in cc.MEASURED.items():
        assert f"{k} " in text and f"(MEASURED {v:.1e}, bar {cc.BARS[k]:.2e})" in text, k
    assert f"WHITE_MEASURED {cc.WHITE_MEASURED}, bar {cc.WHITE_BAR}" in text


BAD = ((dict(fps=0.0), "fps must be positive and finite"), (dict(fps=float("nan")), "fps must be positive and finite"), (dict(fps=float("inf")), "fps must be positive and finite"),
       (dict(derivative=-1), "derivative outside [0, 2]"), (dict(derivative=3), "derivative outside [0, 2]"), (dict(segment=6, hop=3), "segment must be even and within [8, 256]"),
       (dict(segment=63), "segment must be even and within [8, 256]"), (dict(segment=258, hop=64, nfft=512), "segment must be even and within [8, 256]"),
       (dict(hop=7), "hop outside [segment / 8, segment]"), (dict(hop=65), "hop outside [segment / 8, segment]"), (dict(nfft=62), "nfft must be even and within [segment, 1024]"),
       (dict(nfft=255), "nfft must be even and within [segment, 1024]"), (dict(nfft=1026), "nfft must be even and within [segment, 1024]"),
       (dict(f_lo=0.0), "f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2"), (dict(f_lo=3.0), "f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2"),
       (dict(f_hi=10.5), "f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2"), (dict(f_lo=float("nan")), "f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2"),
       (dict(min_segments=0), "min_segments outside [2, 2^20]"), (dict(min_segments=1), "min_segments outside [2, 2^20]"),
       (dict(min_segments=2 ** 20 + 1), "min_segments outside [2, 2^20]"), (dict(segment=63, min_segments=1), "segment must be even and within [8, 256]"))
LONG = "sequence 0 has 32769 frames, more than 32768 (the work is quadratic in them)"


def test_bad_arguments_are_refused(pipe):
    joints = cc.noisy_call(25)[0][:30]
    for kw, why in BAD:
        for call in (lambda: pipe.gait_coordination(joints, **kw), lambda: pipe.gait_cross_welch(np.zeros((30, 4)), **kw)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == why
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(sigma=-1.0), "sigma"),
                     (dict(sigma=float("nan")), "sigma"), (dict(sigma=16.5), "sigma"), (dict(segment=8.5), "whole"), (dict(nfft=256.5), "whole"), (dict(min_segments=2.5), "whole"),
                     (dict(exclude=np.zeros(29, np.int32)), "exclude")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_coordination(joints, **kw)
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_coordination(np.zeros((3, 25, 2)))
    with pytest.raises(ValueError, match="signals"):
        pipe.gait_cross_welch(np.zeros((30, 3)))
    for call in (lambda: pipe.gait_cross_welch(np.zeros((32769 + 5, 4)), lengths=[32769, 5]), lambda: pipe.gait_coordination(np.zeros((32769, 25, 3), np.float32))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == LONG
    assert (pipe.gait_cross_welch(np.zeros((32768, 4)), segment=256, hop=256, nfft=256)["limbs"][0, :, :3] == (32768, 128, 128)).all()      # the longest is taken


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_coordination.h itself against the statement: one file per sequence of every case of the shape set, the hand cases and a constant
    signal; coord_frame against kin_frame; every refusal, in the statement's words."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_coordination_check.cpp")
    exe = str(tmp_path / "gait_coordination_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    a = cc.hand_signals()
    cases = [c[:5] for c in cc.shape_set()]
    cases.append(("same", np.stack([a, a, a, a], axis=1), [400], None, cc.rule_of(0, 64, 32, 64)))
    cases.append(("anti", np.stack([a, -a, a, -a], axis=1), [400], None, cc.rule_of(0, 64, 32, 64)))
    cases.append(("late", np.stack([a[2:], a[:-2], a[2:], a[:-2]], axis=1), [398], None, cc.rule_of(0, 64, 32, 64)))
    cases.append(("flat", np.full((400, 4), 1.5), [400], None, cc.RULE))
    files, want = [], {}
    for name, x, lengths, ex, rule in cases:
        host = pipe.gait_cross_welch(x, lengths, ex, **rule)
        at = 0
        for q, T in enumerate(lengths):
            path = cc.write_case(str(tmp_path / f"{name}_{q}.bin"), x[at:at + T], None if ex is None else ex[at:at + T], rule)
            files.append(path)
            want[path] = {k: host[k][q] for k in ("auto", "cross", "limbs", "pairs")}
            at += T
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
    got = cc.parse_output(r.stdout)
    assert len(got) == 20 * len(files)
    for path, host in want.items():
        for ch in range(4):
            assert cc.same_bits(got["auto", path, ch], host["auto"][ch]) and cc.same_bits(got["limb", path, ch], host["limbs"][ch]), (path, ch)
        for p in range(6):
            assert cc.same_bits(got["cross", path, p], host["cross"][p].reshape(-1)), (path, p)
            assert cc.same_bits(got["pair", path, p], host["pairs"][p]), (path, p, got["pair", path, p], host["pairs"][p])
    refused = [(cc.write_case(str(tmp_path / f"bad{k}.bin"), np.zeros((30, 4)), None, dict(cc.RULE, **kw), True), why) for k, (kw, why) in enumerate(BAD)]
    refused.append((cc.write_case(str(tmp_path / "long.bin"), np.zeros((32769, 4)), None, cc.RULE, True), LONG))
    r = subprocess.run([exe] + [path for path, _ in refused], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "ok" and lines[:-1] == [f"refused {path}: {why}" for path, why in refused], r.stdout[-4000:] + r.stderr[-4000:]
