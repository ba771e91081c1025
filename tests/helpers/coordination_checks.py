"""A yardstick by numpy.fft, an articulated noisy walker, hand-made signals and the case files for arm swing and inter-limb coordination,
shared by the host and the GPU tests.  Nothing here calls the code under test: what compares it takes the statement's arrays as arguments.

THE YARDSTICK.  Rules 2 to 7 with other tools than the code under test has: the segments are laid by a plain loop over the frames of the common
mask, the window is numpy's cosine, the transform numpy.fft.rfft at nfft points, the average numpy's mean, the phase numpy.arctan2.  Where scipy
imports, scipy_run gives scipy.signal.csd and scipy.signal.coherence of ONE run of valid frames.

THE BARS are never measured from the statement or from the device.  The statement is a direct sum in a fixed order and the yardstick a fast
transform: both round, otherwise.  What each of the two KINDS of sum misses the exact value by is measured here from the yardstick's own three
renderings -- `rfft` (float64, numpy.fft), `direct` (float64, a matrix of numpy's cosines and sines times the segments: a direct sum as the statement
is one, with numpy's order) and `long` (the same matrix product in numpy.longdouble, 64 bits of mantissa, which stands for the exact value) -- and a
statement that is a correct direct sum lies within miss(rfft) + miss(direct) of the rfft yardstick.  Each bar is 8 times the worst such sum over
shape_set (measure_bounds; the record: profiles/gait_coordination_bounds.txt, written by `python -m tests.helpers.coordination_checks FILE`, which
refuses a constant below what it measures).  The margin is DESIGN 4.19's, for its reason: the set is small and the direct sum's error grows with the
segment length, and the statement's fixed order is not numpy's.  The ratios:
  auto      |difference| per bin over the row's largest bin
  cross     |difference of Re|, |difference of Im| per bin over sqrt(max P_aa max P_bb)
  coherence_peak, coherence_band (absolute) and phase_peak (degrees), ON THE NOISY CALL ONLY: a clean sinusoid's off-peak bins hold only leakage,
            and a quotient of two such numbers means nothing.
The device and the checker are held to the statement in every bit, so they inherit these bars.

THE NOISY CALL: kinematics_checks.walker with arm_right = 0.6 and 5 mm of seeded joint noise, seven sequences of 130, 1, 19, 20, 64 (standing: one
frame repeated, no noise), 65 and 400 frames, J = 25 and 49, and an exclude mask like entropy_checks.noisy_call's.  RULES names every value of
derivative, segment, hop and nfft that the tests ask for, without their whole product.  THE WHITE-NOISE ANCHOR: two independent standard-normal
signals, hop = segment = nfft = 64, K = 64 segments: the mean coherence over the bins 1 .. 31 tends to 1 / K."""
import functools

import numpy as np

from . import kinematics_checks as kc
from . import spectrum_checks as sc
from .gait_checks import same_bits  # noqa: F401  (the tests use it through this module)

FPS = 20.0
NOISE, SEED = 0.005, 11
RULE = dict(fps=FPS, derivative=0, segment=64, hop=32, nfft=256, f_lo=0.5, f_hi=3.0, min_segments=4)
# (derivative, segment, hop, nfft, min_segments): derivative 0, 1, 2; L 8, 64, 256; hop L / 8, L / 2, L; N = L, 256, 510, 512, 514 (256, 257 and 258
# bins: a block of 64 bins fewer, just full, and one more) and 1024.  Every rule lays at least min_segments segments on the 400-frame walker (the
# last two: its run of 329 first differences behind the excluded frames holds 3 segments of 256, 32 apart; its 398 second differences hold 2, 128 apart)
RULES = ((0, 64, 32, 256, 4), (1, 8, 1, 8, 4), (2, 8, 4, 256, 4), (0, 8, 8, 510, 4), (1, 64, 8, 64, 4), (2, 64, 64, 512, 2), (0, 64, 32, 514, 4), (1, 256, 32, 1024, 2),
         (2, 256, 128, 256, 2))
PAIRS = ((0, 1), (2, 3), (0, 3), (1, 2), (0, 2), (1, 3))
EXPECTED = (180.0, 180.0, 0.0, 0.0, 180.0, 180.0)
KIN_COLUMNS = (8, 9, 0, 1)
LDS_FRAMES, LDS_SEGMENTS = 1024, 128                           # csrc/kernels.h's kCoordLdsFrames and kCoordLdsSegments: more go to the call's scratch
NAMES = ("walk130", "one", "walk19", "walk20", "standing64", "walk65", "walk400")
LENGTHS = (130, 1, 19, 20, 64, 65, 400)

# measure_bounds' worst values, rounded up in the second place (profiles/gait_coordination_bounds.txt); the bars are 8 times these
MEASURED = dict(auto=2.0e-15, cross=1.4e-15, coherence_peak=2.8e-15, coherence_band=2.8e-15, phase_peak=1.1e-13)
BARS = {k: 8.0 * v for k, v in MEASURED.items()}
# the anchor: what the yardstick's own mean coherence misses 1 / K by over WHITE_SEEDS, rounded up in the fourth place; the bar is twice that
WHITE_K, WHITE_L, WHITE_SEEDS = 64, 64, tuple(range(20))
WHITE_RULE = dict(fps=FPS, derivative=0, segment=WHITE_L, hop=WHITE_L, nfft=WHITE_L, f_lo=0.5, f_hi=3.0, min_segments=4)
WHITE_MEASURED = 0.0071
WHITE_BAR = 2.0 * WHITE_MEASURED


def rule_of(derivative, segment, hop, nfft, min_segments=4, **more):
    return dict(RULE, derivative=derivative, segment=segment, hop=hop, nfft=nfft, min_segments=min_segments, **more)


@functools.lru_cache(maxsize=None)
def noisy_call(J=25):
    """(joints float32 (n,J,3), lengths, names, exclude, table) of the seven noisy sequences of one call."""
    table = kc.KINECTV2 if J == 25 else kc.OTHER49
    rng = np.random.default_rng(SEED + J)
    parts = []
    for k, (name, T) in enumerate(zip(NAMES, LENGTHS)):
        if name == "standing64":
            parts.append(np.repeat(kc.walker(1, 0.4, J=J, table=table, arm_right=0.6)[0], T, axis=0))      # the standing body stays still
            continue
        j = kc.walker(T, 0.3 * k - 0.5, 21.7, -3.02 + 0.7 * k, J, table, arm_right=0.6)[0]      # 20 / 21.7 Hz: bin 11.8 of 256
        parts.append((j.astype(np.float64) + NOISE * rng.standard_normal(j.shape)).astype(np.float32))
    ex = np.zeros(sum(LENGTHS), np.int32)
    a = 0
    for T in LENGTHS:
        ex[a + 60:a + min(T, 70)] = 2
        if T > 3:
            ex[a + 3] = 1
        a += T
    return np.concatenate(parts), list(LENGTHS), list(NAMES), ex, table


def angles_of(joints, table):
    """(T,4) float64 degrees: shoulder flexion left / right, hip flexion left / right by numpy's own arctan2 and norms, for the yardstick alone."""
    p = [np.asarray(joints, np.float64)[:, i] for i in table]
    with np.errstate(all="ignore"):
        l, u = p[2] - p[3], p[1] - p[0]
        f = np.cross(l, u)
        f = f / np.linalg.norm(f, axis=1, keepdims=True)
        n = l / np.linalg.norm(l, axis=1, keepdims=True)
        w = np.cross(f, n)
        out = np.full((len(f), 4), np.nan)
        for s in (0, 1):
            arm, d = p[12 + s] - p[10 + s], p[4 + s] - p[2 + s]
            out[:, s] = np.degrees(np.arctan2((arm * f).sum(1), -(arm * w).sum(1)))
            out[:, 2 + s] = np.degrees(np.arctan2((d * f).sum(1), -(d * w).sum(1)))
    return out


def common(x, exclude, derivative):
    """(y (T,4) with NaN on every frame that does not count, n): rule 2's one mask over the four differenced signals."""
    y = np.stack([sc.differenced(x[:, c], exclude, derivative) for c in range(4)], axis=1)
    ok = np.isfinite(y).all(axis=1)
    y[~ok] = np.nan
    return y, int(ok.sum())


def transforms(seg, nfft, mode):
    """(real, imaginary) parts (segments, nfft/2+1) of the transform of windowed segments (segments, L): numpy.fft, or a direct matrix product with
    numpy's cosines and sines at (k i) mod nfft in float64 or in longdouble."""
    if mode == "rfft":
        X = np.fft.rfft(seg, n=nfft, axis=1)
        return X.real, X.imag
    kind = np.longdouble if mode == "long" else np.float64
    turn = ((np.arange(nfft // 2 + 1)[None, :] * np.arange(seg.shape[1])[:, None]) % nfft).astype(kind)
    ang = (8 * np.arctan(kind(1))) * turn / kind(nfft)
    s = seg.astype(kind)
    return s @ np.cos(ang), -(s @ np.sin(ang))


def yardstick(x, exclude=None, fps=FPS, derivative=0, segment=64, hop=32, nfft=256, f_lo=0.5, f_hi=3.0, min_segments=4, mode="rfft"):
    """ONE sequence's signals (T,4) -> dict: auto (4,bins), re and im (6,bins) of conj(X_a) X_b, n, candidates, used, and per pair peak_bin,
    coherence_peak, phase_peak, phase_deviation, coherence_band, per limb band_power and amplitude; NaN rows where used is 0."""
    x = np.asarray(x, np.float64)
    y, n = common(x, exclude, derivative)
    starts = sc.segments_of(y[:, 0], segment, hop)
    used = len(starts) if len(starts) >= min_segments else 0
    bins = nfft // 2 + 1
    kind = np.longdouble if mode == "long" else np.float64
    out = dict(n=n, candidates=len(starts), used=used, auto=np.full((4, bins), np.nan, kind), re=np.full((6, bins), np.nan, kind), im=np.full((6, bins), np.nan, kind))
    if used:
        i = np.arange(segment, dtype=kind)
        w = 0.5 - 0.5 * np.cos((8 * np.arctan(kind(1))) * i / segment)
        scale = np.ones(bins, kind)
        scale[1:nfft // 2] = 2
        scale = scale / (kind(fps) * (w * w).sum())
        Xr, Xi = [], []
        for c in range(4):
            seg = np.stack([y[s:s + segment, c] for s in starts]).astype(kind)
            real, imag = transforms((seg - seg.mean(axis=1, keepdims=True)) * w, nfft, mode)
            Xr.append(real)
            Xi.append(imag)
            out["auto"][c] = (Xr[c] ** 2 + Xi[c] ** 2).mean(axis=0) * scale
        for p, (a, b) in enumerate(PAIRS):                     # conj(X_a) X_b, X = Xr + i Xi
            out["re"][p] = (Xr[a] * Xr[b] + Xi[a] * Xi[b]).mean(axis=0) * scale
            out["im"][p] = (Xr[a] * Xi[b] - Xi[a] * Xr[b]).mean(axis=0) * scale
    freqs = np.arange(bins) * fps / nfft
    band = np.flatnonzero((freqs >= f_lo) & (freqs <= f_hi))
    out["band"] = band
    rows = {k: np.full(6, np.nan, kind) for k in ("peak_bin", "coherence_peak", "phase_peak", "phase_deviation", "coherence_band")}
    out["band_power"] = out["auto"][:, band].sum(axis=1) * kind(fps) / nfft if used else np.full(4, np.nan)
    out["amplitude"] = np.sqrt(2 * out["band_power"])
    if used:
        with np.errstate(all="ignore"):
            for p, (a, b) in enumerate(PAIRS):
                m2 = out["re"][p] ** 2 + out["im"][p] ** 2
                coh = m2 / (out["auto"][a] * out["auto"][b])
                if not (m2[band] > 0).any():
                    continue
                k = int(band[np.argmax(m2[band])])
                phase = np.degrees(np.arctan2(out["im"][p, k], out["re"][p, k]))
                rows["peak_bin"][p], rows["coherence_peak"][p], rows["phase_peak"][p] = k, coh[k], phase
                rows["phase_deviation"][p] = abs(180 - abs(phase)) if EXPECTED[p] == 180.0 else abs(phase)
                rows["coherence_band"][p] = np.mean(coh[band][np.isfinite(coh[band])])
    out.update(rows)
    return out


def scipy_run(x, fps=FPS, segment=64, hop=32, nfft=256):
    """(freqs, csd (6,bins) complex, coherence (6,bins)) of ONE run of valid frames (T,4) by scipy.signal; None where scipy does not import."""
    try:
        from scipy import signal
    except ImportError:
        return None
    kw = dict(fs=fps, window="hann", nperseg=segment, noverlap=segment - hop, nfft=nfft, detrend="constant")
    csd = np.stack([signal.csd(x[:, a], x[:, b], scaling="density", **kw)[1] for a, b in PAIRS])
    coh = np.stack([signal.coherence(x[:, a], x[:, b], **kw)[1] for a, b in PAIRS])
    return np.arange(nfft // 2 + 1) * fps / nfft, csd, coh


def ratios(auto, re, im, want):
    """(the worst auto ratio, the worst cross ratio) of a sequence's arrays against a yardstick dict `want`; rows that are NaN must be NaN alike."""
    auto, re, im = np.asarray(auto, np.longdouble), np.asarray(re, np.longdouble), np.asarray(im, np.longdouble)
    assert (np.isnan(auto) == np.isnan(want["auto"])).all() and (np.isnan(re) == np.isnan(want["re"])).all() and (np.isnan(im) == np.isnan(want["im"])).all()
    if not want["used"]:
        return 0.0, 0.0
    top = np.asarray(want["auto"], np.longdouble).max(axis=1)
    worst_auto = worst_cross = 0.0
    for c in range(4):
        if top[c] > 0:
            worst_auto = max(worst_auto, float(np.abs(auto[c] - want["auto"][c]).max() / top[c]))
        else:
            assert (auto[c] == 0).all()
    for p, (a, b) in enumerate(PAIRS):
        den = np.sqrt(top[a] * top[b])
        if den > 0:
            worst_cross = max(worst_cross, float(max(np.abs(re[p] - want["re"][p]).max(), np.abs(im[p] - want["im"][p]).max()) / den))
        else:
            assert (re[p] == 0).all() and (im[p] == 0).all()
    return worst_auto, worst_cross


def runs_call(segment=64, hop=32):
    """spectrum_checks.runs_call: seeded noise (n,4) whose runs of validity begin and end at frames 63, 64 and 65, by NaN and by exclude, then runs
    exactly segment - 1, segment and segment + hop frames long; every NaN there is in all four channels."""
    return sc.runs_call(segment, hop)


def hand_signals(T=400, seed=5):
    """a (T,) of seeded noise on a sinusoid at bin 4 of 64, for the hand cases b = a, b = -a and b delayed."""
    rng = np.random.default_rng(seed)
    return np.sin(2.0 * np.pi * 4.0 * np.arange(T) / 64.0) + 0.1 * rng.standard_normal(T)


def white_noise(seed):
    """(WHITE_K WHITE_L, 4) independent standard-normal signals."""
    return np.random.default_rng(1000 + seed).standard_normal((WHITE_K * WHITE_L, 4))


def white_mean(auto, re, im):
    """The mean coherence of the pair (0, 1) over the bins 1 .. 31 from one sequence's auto (4,bins) and cross parts (6,bins)."""
    k = slice(1, WHITE_L // 2)
    return float(np.mean((re[0][k] ** 2 + im[0][k] ** 2) / (auto[0][k] * auto[1][k])))


def write_case(path, signals, exclude, rule, refused=False):
    """The file tests/helpers/gait_coordination_check.cpp reads: spectrum_checks.write_case's layout, ONE sequence's signals (T,4) and the scalars."""
    return sc.write_case(path, signals, exclude, rule, refused)


def parse_output(text):
    """{(what, file, index): float64 array} of the checker's lines, from their hexadecimal words."""
    out = {}
    for line in text.splitlines():
        part = line.split()
        if part and part[0] in ("auto", "cross", "limb", "pair"):
            out[part[0], part[1], int(part[2])] = np.array([int(w, 16) for w in part[3:]], np.uint64).view(np.float64)
    return out


def shape_set():
    """(name, signals (n,4), lengths, exclude, rule, noisy) of every case the bars are measured over: the noisy call's angles under RULES, every other
    case with its exclude, and the runs at segments of 64 and 8 frames."""
    joints, lengths, _, ex, table = noisy_call(25)
    signals = angles_of(joints, table)
    cases = [(f"noisy{k}", signals, lengths, ex if k % 2 else None, rule_of(*r), True) for k, r in enumerate(RULES)]
    x, run_lengths, run_ex = runs_call()
    cases.append(("runs", x, run_lengths, run_ex, rule_of(0, 64, 32, 256, 2), False))
    x8, run_lengths8, run_ex8 = runs_call(8, 4)
    cases.append(("runs8", x8, run_lengths8, run_ex8, rule_of(0, 8, 4, 32, 2), False))
    return cases


def measure_bounds():
    """({bar name: the worst miss(rfft) + miss(direct) against the longdouble rendering over shape_set}, the lines of the record)."""
    worst, lines = {k: 0.0 for k in MEASURED}, []
    for name, signals, lengths, ex, rule, noisy in shape_set():
        here = {k: 0.0 for k in MEASURED}
        a = 0
        for T in lengths:
            args = (signals[a:a + T], None if ex is None else ex[a:a + T])
            exact = yardstick(*args, **rule, mode="long")
            miss = {k: 0.0 for k in MEASURED}
            for mode in ("rfft", "direct"):
                got = yardstick(*args, **rule, mode=mode)
                assert (got["n"], got["candidates"], got["used"]) == (exact["n"], exact["candidates"], exact["used"])
                ra, rc = ratios(got["auto"], got["re"], got["im"], exact)
                miss["auto"], miss["cross"] = miss["auto"] + ra, miss["cross"] + rc
                if noisy and exact["used"]:
                    for k in ("coherence_peak", "coherence_band", "phase_peak"):
                        fin = np.isfinite(np.asarray(exact[k], np.float64))
                        assert (np.asarray(got["peak_bin"], np.float64)[fin] == np.asarray(exact["peak_bin"], np.float64)[fin]).all()
                        if fin.any():
                            miss[k] = miss[k] + float(np.abs(np.asarray(got[k], np.longdouble) - exact[k])[fin].max())
            here = {k: max(here[k], miss[k]) for k in here}
            a += T
        lines.append(f"{name}: derivative {rule['derivative']} segment {rule['segment']} hop {rule['hop']} nfft {rule['nfft']}: " +
                     ", ".join(f"{k} {v:.3e}" for k, v in here.items()))
        worst = {k: max(worst[k], here[k]) for k in worst}
    return worst, lines


def measure_white():
    """(the yardstick's worst miss of 1 / K over WHITE_SEEDS, the lines of the record)."""
    worst, lines = 0.0, []
    for seed in WHITE_SEEDS:
        y = yardstick(white_noise(seed), None, **WHITE_RULE)
        assert y["used"] == WHITE_K
        mean = white_mean(y["auto"], y["re"], y["im"])
        worst = max(worst, abs(mean - 1.0 / WHITE_K))
        lines.append(f"seed {seed:2d}: mean coherence over bins 1 .. 31 {mean:.5f}, miss {abs(mean - 1.0 / WHITE_K):.5f}")
    return worst, lines


BOUNDS_HEAD = """# Arm swing and inter-limb coordination (DESIGN 4.21): what a float64 fast transform (numpy.fft.rfft) and a float64 direct sum (a matrix of numpy's
# cosines and sines) each miss the same sums in numpy.longdouble by, added: the statement pipeline.gait_cross_welch is a direct sum in a fixed order
# (the bits of csrc/gait_coordination.h and of the kernels) and is held against the rfft yardstick of tests/helpers/coordination_checks.py, so a
# correct one lies within that sum.  Measured on the CPU FROM THE YARDSTICK ALONE by `python -m tests.helpers.coordination_checks FILE` over
# coordination_checks.shape_set: the four angles of coordination_checks.noisy_call (seven sequences of 130, 1, 19, 20, 64, 65 and 400 frames, 5 mm of
# joint noise, arm_right = 0.6) under coordination_checks.RULES, every other case with its exclude, and the hand-made runs at the word boundary.
# auto: per bin over the row's largest bin; cross: Re and Im per bin over sqrt(max P_aa max P_bb); coherence_peak and coherence_band absolute and
# phase_peak in degrees, on the noisy cases only.  The bars of the tests are 8 times the worst values below, rounded up in the second place
# (coordination_checks.MEASURED): the set is small, the direct sum's error grows with the segment length, and the statement's order is not numpy's.
"""
WHITE_HEAD = """#
# THE WHITE-NOISE ANCHOR: numpy.random.default_rng(1000 + seed).standard_normal((4096, 4)), hop = segment = nfft = 64, K = 64 segments: the mean
# coherence of the first two signals over the bins 1 .. 31 tends to 1 / K = 0.015625.  What the yardstick itself misses it by (the finite-sample error
# of the estimator, not an error of the code); the bar is twice the worst miss, rounded up in the fourth place (coordination_checks.WHITE_MEASURED).
"""


def write_bounds(path):
    """The record profiles/gait_coordination_bounds.txt, from the yardstick alone; refuses a constant below what it measures."""
    assert np.finfo(np.longdouble).nmant > 60, "numpy.longdouble is no wider than float64 here: nothing can be measured against it"
    worst, lines = measure_bounds()
    for k, v in worst.items():
        assert v <= MEASURED[k], f"{k}: measured {v:.3e}, more than MEASURED = {MEASURED[k]:.3e}"
    white, white_lines = measure_white()
    assert white <= WHITE_MEASURED, f"the yardstick misses 1 / K by {white:.5f}, more than WHITE_MEASURED = {WHITE_MEASURED}"
    with open(path, "w") as f:
        f.write(BOUNDS_HEAD + "\n".join(lines) + "\nworst: " + ", ".join(f"{k} {v:.3e} (MEASURED {MEASURED[k]:.1e}, bar {BARS[k]:.2e})" for k, v in worst.items()) + "\n")
        f.write(WHITE_HEAD + "\n".join(white_lines) + f"\nworst miss {white:.5f}: WHITE_MEASURED {WHITE_MEASURED}, bar {WHITE_BAR}\n")
    return worst, white


if __name__ == "__main__":
    import sys
    print(write_bounds(sys.argv[1]))
