"""Harmonic ratios per stride on the host: pipeline.gait_harmonics and pipeline.gait_stride_dft, the numpy float64 statements, against the
yardstick in plain loops of tests/helpers/harmonic_checks.py (every bit); the twiddles against high-precision arithmetic (2^-51, every 6 <= L <= 255
and every j); every used stride's sums against numpy.fft.rfft (2^-44 of the sum of |y|); the closed form of the walker with an integer period (the
bars: twice the yardstick's own miss, profiles/gait_harmonics_bounds.txt); what a non-integer period and joint noise do to it (measured, not barred);
the edge cases of the rules; every refusal.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from .helpers import gait_checks as gc
from .helpers import harmonic_checks as hc
from .helpers import regularity_checks as rc

FPS = hc.FPS


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def call_events(pipe, joints, trans, lengths, table):
    return pipe.gait_parameters(joints, lengths, trans, fps=FPS, joints=table)["events"]


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
    trans[[5, 200]] = np.nan
    events = call_events(pipe, joints, trans, lengths, table)
    want_frame = rc.signals_of(joints, trans, table)
    for ex in (None, exclude_of(lengths)):
        for rule in (hc.RULE, dict(n_harmonics=2, derivative=0, min_stride=6, max_stride=255, max_strides=3), dict(n_harmonics=32, derivative=1, min_stride=20, max_stride=24, max_strides=512)):
            out = pipe.gait_harmonics(joints, events, lengths, trans, ex, fps=FPS, joints=table, **rule)
            assert hc.same_bits(out["per_frame"], want_frame)
            strides, spectrum, rows = hc.yardstick_call(want_frame, events, lengths, ex, fps=FPS, **rule)
            assert hc.same_bits(out["strides"], strides) and hc.same_bits(out["spectrum"], spectrum) and hc.same_bits(out["per_sequence"], rows), (J, rule)
    seq = dict(zip(names, pipe.gait_harmonics(joints, events, lengths, trans, fps=FPS, joints=table)["per_sequence"]))
    print("walk400_back:", seq["walk400_back"][0].tolist())
    assert seq["walk400_back"][0, 1] >= 20 and seq["walk400_back"][3, 1] >= 20 and seq["one"][0, 0] == 0 and np.isnan(seq["one"][0, 2:]).all()


def test_hand_placed_events_against_the_yardstick(pipe):
    x, ev, ex, lengths, names = hc.hand_events_call()
    for exclude in (None, ex):
        for rule in (dict(hc.RULE, min_stride=6, max_stride=255, max_strides=8), dict(n_harmonics=32, derivative=0, min_stride=6, max_stride=255, max_strides=128)):
            out = pipe.gait_stride_dft(x, ev, lengths, exclude, fps=FPS, **rule)
            strides, spectrum, rows = hc.yardstick_call(x, ev, lengths, exclude, fps=FPS, **rule)
            assert hc.same_bits(out["strides"], strides) and hc.same_bits(out["spectrum"], spectrum) and hc.same_bits(out["per_sequence"], rows), rule
    out = pipe.gait_stride_dft(x, ev, lengths, ex, fps=FPS, n_harmonics=32, derivative=2, min_stride=6, max_stride=255, max_strides=128)
    seq, st = dict(zip(names, out["per_sequence"])), dict(zip(names, out["strides"]))
    e = st["edges800"][0]
    print("edges800 sep:", e[:15, :4].tolist())
    L = e[:11, 1] - e[:11, 0]
    assert L.tolist() == [6, 7, 50, 1, 1, 63, 64, 65, 255, 256, 31] and e[:11, 3].tolist() == [2, 2, 24, 0, 0, 30, 30, 32, 32, 0, 14]
    assert e[10, 1] == 799 and (e[:11, 2] == 1).all() and (e[11:14, 2] == -1).all() and (e[11:14, 1] - e[11:14, 0]).tolist() == [5, 54, 200]
    assert e[11, 3] == 0 and np.isnan(e[11, 4:]).all() and np.isnan(e[14:]).all() and seq["edges800"][0, :2].tolist() == [14, 10]       # L = 5 and 256: unused
    assert seq["one"][0, 0] == 0 and seq["no_strikes"][0, 0] == 0 and np.isnan(seq["one"][:, 2:]).all() and np.isnan(st["no_strikes"]).all()
    # a NaN at t1 exactly: both left strides that touch frame 57 of sep go, and the right stride 43 .. 70 around it; bob loses those at and around frame
    # 70; the other channels keep theirs
    n = seq["nan_at_t1"]
    assert n[:, 0].tolist() == [8] * 4 and n[:, 1].tolist() == [5, 8, 8, 5] and st["nan_at_t1"][0, 5, 3] == 0 and st["nan_at_t1"][1, 5, 3] > 0 and st["nan_at_t1"][0, 1, 3] == 0 and st["nan_at_t1"][0, 2, 3] == 0 and st["nan_at_t1"][0, 0, 3] > 0
    # an excluded frame inside a stride: frame 40 lies in the left stride 30 .. 57 and the right stride 16 .. 43
    assert seq["excluded"][:, 1].tolist() == [6] * 4 and st["excluded"][0, 1, 3] == 0 and st["excluded"][0, 4, 3] == 0
    assert pipe.gait_stride_dft(x, ev, lengths, None, fps=FPS, min_stride=6, max_stride=255)["per_sequence"][names.index("excluded"), 0, 1] == 8
    # a frame with both feet striking is a strike of each
    b = st["both_feet"][0]
    assert seq["both_feet"][0, 0] == 4 and b[:4, :3].tolist() == [[0, 20, 1], [20, 40, 1], [40, 64, 1], [20, 40, -1]]
    assert seq["seven"][0, :2].tolist() == [1, 1] and seq["seven"][0, 11] == 2 and seq["seven"][0, 9] == 6 and seq["seven"][0, 10] == FPS / 6
    # more candidates than max_strides: counted and used, not stored
    few = pipe.gait_stride_dft(x, ev, lengths, ex, fps=FPS, n_harmonics=32, derivative=2, min_stride=6, max_stride=255, max_strides=3)
    assert hc.same_bits(few["per_sequence"], out["per_sequence"]) and hc.same_bits(few["spectrum"], out["spectrum"]) and hc.same_bits(few["strides"], out["strides"][:, :, :3])


def test_twiddles_against_high_precision(pipe):
    worst, where = 0.0, None
    for L in range(6, 256):
        sn, cs = pipe.harmonics_twiddles(L)
        true, miss = hc.true_twiddles(L)
        assert sn[0] == 0.0 and cs[0] == 1.0
        if L % 4 == 0:
            q = L // 4
            assert (sn[[q, 2 * q, 3 * q]] == [1.0, 0.0, -1.0]).all() and (cs[[q, 2 * q, 3 * q]] == [0.0, -1.0, 0.0]).all()
        for j in range(L):
            assert (float(sn[j]), float(cs[j])) == hc.twiddle(j, L)
            m = max(miss(float(sn[j]), true[j][0]), miss(float(cs[j]), true[j][1]))
            if m > worst:
                worst, where = m, (L, j)
    print(f"twiddles: worst miss {worst * 2 ** 53:.3f} x 2^-53 at L, j = {where}; bar 2^-51")
    assert worst <= hc.TWIDDLE_BAR


def test_sums_against_rfft(pipe):
    x, ev, ex, lengths, _ = hc.hand_events_call()
    joints, trans, wl, _ = rc.build_call()
    per_frame = pipe.gait_regularity(joints, wl, trans, fps=FPS)["per_frame"]
    worst, count = 0.0, 0
    for sig, events, ls in ((x, ev, lengths), (per_frame, call_events(pipe, joints, trans, wl, gc.KINECTV2), wl)):
        out = pipe.gait_stride_dft(sig, events, ls, fps=FPS, n_harmonics=32, min_stride=6, max_stride=255, return_sums=True)
        for q, ch, t0, t1, y, C, S in out["sums"]:
            F = np.fft.rfft(y)
            H = len(C)
            bar = 2.0 ** -44 * np.abs(y).sum()
            m = max(np.abs(C - F.real[1:H + 1]).max(), np.abs(S + F.imag[1:H + 1]).max())
            worst, count = max(worst, m / bar), count + 1
            assert m <= bar, (q, ch, t0, t1, m, bar)
    print(f"{count} used strides: C_k and S_k within {worst:.4f} of the bar 2^-44 sum |y| of numpy.fft.rfft")
    assert count > 100


@pytest.mark.parametrize("through_joints", (False, True))
def test_closed_form_with_an_integer_period(pipe, through_joints):
    bar = hc.closed_bars(through_joints)
    worst = dict(hr=0.0, ihr=0.0)
    ev = hc.periodic_events(400, hc.CLOSED_P, 5, 17)
    for B, d in hc.CLOSED_CASES:
        for theta in (hc.CLOSED_YAWS if through_joints else hc.CLOSED_YAWS[:1]):
            for phi in hc.CLOSED_PHASES:
                if through_joints:
                    joints, trans = rc.walker(400, float(hc.CLOSED_P), B, theta, phi)
                    out = pipe.gait_harmonics(joints, ev, trans=trans, fps=FPS, **dict(hc.RULE, derivative=d))
                else:
                    out = pipe.gait_stride_dft(np.repeat(hc.closed_signal(400, B, phi)[:, None], 4, axis=1), ev, fps=FPS, **dict(hc.RULE, derivative=d))
                rows, seq = out["strides"][0, 0, :31], out["per_sequence"][0, 0]
                assert seq[0] == seq[1] == 31 and seq[9] == hc.CLOSED_P and seq[11] == 10
                worst["hr"] = max(worst["hr"], np.abs(rows[:, 4] - hc.closed_hr(B, d)).max() / hc.closed_hr(B, d))
                worst["ihr"] = max(worst["ihr"], np.abs(rows[:, 5] - hc.closed_ihr(B, d)).max() / hc.closed_ihr(B, d))
                assert abs(seq[2] - hc.closed_hr(B, d)) <= bar["hr"] * hc.closed_hr(B, d) and abs(seq[7] - hc.closed_ihr(B, d)) <= bar["ihr"] * hc.closed_ihr(B, d)
    print(f"through joints {through_joints}: HR off by {worst['hr']:.3e} relative (bar {bar['hr']:.3e}), iHR by {worst['ihr']:.3e} (bar {bar['ihr']:.3e})")
    assert worst["hr"] <= bar["hr"] and worst["ihr"] <= bar["ihr"]
    assert abs(hc.closed_hr(0.3, 0) - 3.333) < 1e-3 and abs(hc.closed_ihr(0.3, 0) - 91.74) < 5e-3 and abs(hc.closed_hr(0.3, 2) - 0.8333) < 1e-4 and abs(hc.closed_ihr(0.3, 2) - 40.98) < 5e-3


def test_symmetric_walker_is_used_or_degenerate_consistently(pipe):
    """B = 0: the even sum is rounding residue and the ratio means nothing; the statement and the yardstick agree on which strides are used."""
    joints, trans = rc.walker(400, float(hc.CLOSED_P), 0.0, 0.3, 1.0)
    ev = hc.periodic_events(400, hc.CLOSED_P, 5, 17)
    out = pipe.gait_harmonics(joints, ev, trans=trans, fps=FPS)
    strides, _, rows = hc.yardstick_call(rc.signals_of(joints, trans), ev, [400], fps=FPS, **hc.RULE)
    assert hc.same_bits(out["strides"], strides) and hc.same_bits(out["per_sequence"], rows)
    zeros = np.zeros((400, 4))
    flat = pipe.gait_stride_dft(zeros, ev, fps=FPS)                # a constant signal: every stride is degenerate
    assert flat["per_sequence"][0, :, 0].tolist() == [31] * 4 and flat["per_sequence"][0, :, 1].tolist() == [0] * 4 and (flat["strides"][0, :, :31, 3] == 0).all()


def test_non_integer_period_and_noise_are_measured_not_barred(pipe):
    """Strides that alternate between two lengths do not close, and 5 mm of joint noise is amplified by k^2: what that does to HR at B = 0.3."""
    for d in (0, 2):
        for P, noise in ((21.7, 0.0), (24.0, 0.005), (21.7, 0.005)):
            joints, trans = rc.walker(400, P, 0.3, 0.3, 1.0)
            if noise:
                joints = (joints + noise * np.random.default_rng(2013).standard_normal(joints.shape)).astype(np.float32)
            events = pipe.gait_parameters(joints, trans=trans, fps=FPS)["events"]
            row = pipe.gait_harmonics(joints, events, trans=trans, fps=FPS, derivative=d)["per_sequence"][0, 0]
            print(f"d {d} P {P} noise {noise * 1000:.0f} mm: {int(row[1])} of {int(row[0])} strides used, HR {row[2]:.4f} (SD {row[3]:.4f}) for the closed {hc.closed_hr(0.3, d):.4f}, "
                  f"iHR {row[7]:.2f} for {hc.closed_ihr(0.3, d):.2f}")
            assert row[1] > 0 and np.isfinite(row[[2, 3, 7, 8]]).all()


def test_sequences_do_not_see_each_other(pipe):
    joints, trans, lengths, names = rc.build_call()
    events = call_events(pipe, joints, trans, lengths, gc.KINECTV2)
    ex = exclude_of(lengths)
    for sigma in (0.0, 2.0):
        whole = pipe.gait_harmonics(joints, events, lengths, trans, ex, fps=FPS, sigma=sigma)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_harmonics(joints[a:a + n], events[a:a + n], None, trans[a:a + n], ex[a:a + n], fps=FPS, sigma=sigma)
            for key in ("strides", "spectrum", "per_sequence"):
                assert hc.same_bits(whole[key][q], alone[key][0]), (names[q], key)
            assert hc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]), names[q]
            a += n
        assert hc.same_bits(whole["per_frame"], pipe.gait_regularity(joints, lengths, trans, fps=FPS, sigma=sigma)["per_frame"])
    assert not hc.same_bits(whole["per_sequence"], pipe.gait_harmonics(joints, events, lengths, trans, ex, fps=FPS)["per_sequence"])      # a Gaussian moves the ratio


def test_bad_arguments_are_refused(pipe):
    joints, trans = rc.walker(30)
    ev = np.zeros(30, np.int32)
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(fps=0.0), "fps"),
                     (dict(fps=nan), "fps"), (dict(fps=inf), "fps"), (dict(sigma=-1.0), "sigma"), (dict(sigma=nan), "sigma"), (dict(sigma=16.5), "sigma"),
                     (dict(n_harmonics=0), "n_harmonics"), (dict(n_harmonics=21), "n_harmonics"), (dict(n_harmonics=34), "n_harmonics"), (dict(n_harmonics=20.5), "whole"),
                     (dict(derivative=-1), "derivative"), (dict(derivative=3), "derivative"), (dict(min_stride=5), "min_stride"), (dict(min_stride=61), "min_stride"),
                     (dict(max_stride=256), "max_stride"), (dict(max_strides=0), "max_strides"), (dict(max_strides=513), "max_strides"),
                     (dict(trans=np.zeros((29, 3))), "trans"), (dict(exclude=np.zeros(29, np.int32)), "exclude")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_harmonics(joints, ev, **kw)
    with pytest.raises(ValueError, match="events"):
        pipe.gait_harmonics(joints, ev[:29])
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_harmonics(np.zeros((3, 25, 2)), ev[:3])
    with pytest.raises(ValueError, match="signals"):
        pipe.gait_stride_dft(np.zeros((30, 3)), ev)
    assert pipe.HARMONICS_CHANNELS == ("sep", "lift", "sway", "bob") and len(pipe.HARMONICS_COLUMNS) == 12 and len(pipe.HARMONICS_STRIDE_COLUMNS) == 6
