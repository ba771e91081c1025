"""A yardstick by numpy.fft, hand-made signals and the case files for the movement smoothness of the gait signals, shared by the host and
the GPU tests.  Nothing here calls the code under test: what measures it takes the statement as an argument.

THE YARDSTICK.  Rules 1 to 5 and 8 with other tools than the code under test has: the segments are laid by a plain loop over the frames
(spectrum_checks.segments_of), the transform is numpy.fft.rfft(y, nfft), the magnitude numpy.abs, the peak, the band and the sums numpy's own
reductions, the logarithm math.log.  It rounds otherwise than a direct sum in a fixed order, so statement and yardstick differ in the last places.

THE CONDITION ON INPUTS.  The band is cut where the normalised magnitude crosses `amplitude`: a bin within a rounding of the threshold could fall on
either side, and the two would then differ by a whole term.  decision_margin is the smallest |m_k - amplitude| over all bins of all segments; every
input that goes through the comparison must have a margin of at least MARGIN = 1e-9, asserted.  That is a condition, not a tolerance.

THE BAR is on |statement - yardstick| relative to |yardstick|, for sparc and dj of every segment, 8 times the worst such ratio measured over
RULES on the noisy call on the CPU (measure_bound; the record: profiles/gait_smoothness_bounds.txt).  The margin is there because the set is
small and the direct sum's error grows with the segment length.  The device inherits the bar by bit-identity with the statement.

THE NOISY CALL is entropy_checks.noisy_call: seven sequences of 130, 1, 19, 20, 64, 65 and 400 frames with 5 mm of seeded noise, 35 frames excluded."""
import math

import numpy as np

from . import gait_checks as gc
from . import spectrum_checks as sc

FPS = 20.0
RULE = dict(fps=FPS, derivative=1, segment=64, hop=32, nfft=1024, f_cut=10.0, amplitude=0.05, min_segments=2)
# (derivative, segment, hop, nfft, f_cut, amplitude): the issue's rule sets.  nfft = 126, 128 and 130 give 64, 65 and 66 bins and cross a wave's width
RULES = ((1, 64, 32, 1024, 10.0, 0.05), (1, 16, 2, 16, 10.0, 0.05), (0, 16, 8, 126, 10.0, 0.05), (2, 16, 16, 128, 10.0, 0.05), (1, 32, 16, 130, 10.0, 0.2),
         (1, 8, 4, 64, 3.0, 0.05), (1, 256, 256, 4096, 10.0, 0.05))
MARGIN = 1e-9
MEASURED = 1.1e-14                                           # measure_bound's worst ratio, rounded up in the second place (profiles/gait_smoothness_bounds.txt)
BAR = 8.0 * MEASURED


def rule_of(derivative, segment, hop, nfft, f_cut=10.0, amplitude=0.05, **more):
    return dict(RULE, derivative=derivative, segment=segment, hop=hop, nfft=nfft, f_cut=f_cut, amplitude=amplitude, **more)


def slots_of(T, segment, hop):
    return (T - segment) // hop + 1 if T >= segment else 0


def yardstick(x, exclude=None, fps=FPS, derivative=1, segment=64, hop=32, nfft=1024, f_cut=10.0, amplitude=0.05, min_segments=2):
    """(rows, n, candidates, used, margin) of ONE signal of ONE sequence: rows a list of dicts start, sparc, k_first, k_last, peak_bin, dj, ldlj (None
    where the rules give NaN), margin the smallest |m_k - amplitude| over its segments' bins (inf of none)."""
    y = sc.differenced(x, exclude, derivative)
    x = np.asarray(x, np.float64)
    starts = sc.segments_of(y, segment, hop)
    used = len(starts) if len(starts) >= min_segments else 0
    bins = sum(1 for k in range(nfft // 2 + 1) if k * fps <= f_cut * nfft)      # no frequency is formed
    rows, margin = [], math.inf
    for t0 in starts:
        M = np.abs(np.fft.rfft(y[t0:t0 + segment], nfft))[:bins]
        row = dict(start=t0, sparc=None, k_first=None, k_last=None, peak_bin=None, dj=None, ldlj=None)
        rows.append(row)
        if not (M.max() > 0 and np.isfinite(M.max())):
            continue
        m = M / M.max()
        margin = min(margin, float(np.abs(m - amplitude).min()))
        inside = np.nonzero(m >= amplitude)[0]
        ka, kb = int(inside.min()), int(inside.max())
        band = m[ka:kb + 1]
        row.update(k_first=ka, k_last=kb, peak_bin=int(M.argmax()), sparc=0.0)
        if kb > ka:
            row["sparc"] = -float(np.sum(np.sqrt((1.0 / (kb - ka)) ** 2 + np.diff(band) ** 2)))
        xs = x[t0:t0 + segment]
        v = np.abs(np.diff(xs)).max()
        if v > 0:
            row["dj"] = float(np.sum(np.diff(xs, 3) ** 2) * (segment - 1) ** 3 / v ** 2)
            row["ldlj"] = -math.log(row["dj"]) if row["dj"] > 0 else None
    return rows, int(np.isfinite(y).sum()), len(starts), used, margin


def compare(out, signals, lengths, exclude, rule):
    """The statement's (or the device's) `out` against the yardstick on every sequence and channel: asserts every integer column and NaN pattern equal
    and the margin at least MARGIN; returns (the worst relative difference of sparc and dj, the smallest margin)."""
    seg, per_seq, at = np.asarray(out["per_segment"]), np.asarray(out["per_sequence"]), np.asarray(out["slot_offsets"])
    worst, margin, a = 0.0, math.inf, 0
    assert at.tolist() == np.concatenate([[0], np.cumsum([slots_of(T, rule["segment"], rule["hop"]) for T in lengths])]).tolist()
    for q, T in enumerate(lengths):
        for ch in range(4):
            rows, n, candidates, used, here = yardstick(signals[a:a + T, ch], None if exclude is None else exclude[a:a + T], **rule)
            margin = min(margin, here)
            assert here >= MARGIN, (q, ch, here)
            assert per_seq[q, ch, :3].tolist() == [n, candidates, used], (q, ch, per_seq[q, ch, :3], n, candidates, used)
            mine = seg[at[q]:at[q + 1], ch]
            assert np.isnan(mine[candidates:]).all()
            finite = [r["sparc"] for r in rows if r["sparc"] is not None]
            for got, want in zip(mine, rows):
                assert got[0] == want["start"]
                if want["sparc"] is None:
                    assert np.isnan(got[1:]).all()
                    continue
                assert got[2:5].tolist() == [want["k_first"], want["k_last"], want["peak_bin"]], (q, ch, got, want)
                assert (want["sparc"] == 0.0) == (got[1] == 0.0) and (want["dj"] is None) == bool(np.isnan(got[6]))
                if want["sparc"] != 0.0:
                    worst = max(worst, abs(got[1] - want["sparc"]) / abs(want["sparc"]))
                if want["dj"]:
                    worst = max(worst, abs(got[6] - want["dj"]) / abs(want["dj"]))
                if "ldlj" in out and want["ldlj"] is not None:
                    assert abs(out["ldlj"][at[q] + rows.index(want), ch] - want["ldlj"]) <= 1e-12 * max(1.0, abs(want["ldlj"]))
            if used:
                assert per_seq[q, ch, 3] == len(finite) and per_seq[q, ch, 9] == sum(r["dj"] is not None and np.isfinite(r["dj"]) for r in rows)
                if finite:
                    want_row = [np.mean(finite), np.std(finite), min(finite), max(finite), np.mean([r["k_last"] * rule["fps"] / rule["nfft"] for r in rows if r["sparc"] is not None])]
                    assert np.allclose(per_seq[q, ch, 4:9], want_row, rtol=1e-12, atol=1e-13), (q, ch, per_seq[q, ch], want_row)
            else:
                assert np.isnan(per_seq[q, ch, 3:]).all()
        a += T
    return worst, margin


def measure_bound(sparc, noisy):
    """(the worst ratio of the statement `sparc` against the yardstick over RULES on the noisy call, with and without exclude by turns; the smallest
    decision margin; the lines of the record)."""
    signals, lengths, ex = noisy
    worst, margin, lines = 0.0, math.inf, []
    for k, r in enumerate(RULES):
        rule, e = rule_of(*r), ex if k % 2 == 0 else None
        here, m = compare(sparc(signals, lengths, e, **rule), signals, lengths, e, rule)
        lines.append(f"derivative {r[0]} segment {r[1]} hop {r[2]} nfft {r[3]} f_cut {r[4]} amplitude {r[5]} exclude {e is not None}: worst ratio {here:.3e}, margin {m:.3e}")
        worst, margin = max(worst, here), min(margin, m)
    return worst, margin, lines


def centred_cosine(k0, L=64, T=200, amplitude=0.01):
    """signals (T,4) = a cosine with exactly k0 cycles in L frames on every channel: with nfft = L and derivative 0 it sits on bin k0 alone."""
    t = np.arange(T, dtype=np.float64)
    return np.repeat((amplitude * np.cos(2.0 * np.pi * k0 * t / L))[:, None], 4, axis=1)


def runs_signal():
    """signals (400,4) of seeded noise whose NaN frames split it into runs of 30, 64, 63, 150 and 89 frames: shorter and longer than 64."""
    x = np.random.default_rng(24).standard_normal((400, 4)) * 0.01
    x[[30, 95, 159, 310]] = np.nan
    return x


def same_bits(a, b):
    return gc.same_bits(a, b)


def write_case(path, signals, exclude, rule, refused=False):
    """The file tests/helpers/gait_smoothness_check.cpp reads: ONE sequence's signals (T,4) and the call's scalars (refused: a case that the program
    must refuse, and says why; it carries no data)."""
    T = signals.shape[0]
    with open(path, "wb") as f:
        f.write(np.array([T, exclude is not None, rule["derivative"], rule["segment"], rule["hop"], rule["nfft"], rule["min_segments"], not refused], "<i4").tobytes())
        f.write(np.array([rule["fps"], rule["f_cut"], rule["amplitude"]], "<f8").tobytes())
        if refused:
            return path
        f.write(np.ascontiguousarray(signals, "<f8").tobytes())
        if exclude is not None:
            f.write(np.ascontiguousarray(exclude, "<i4").tobytes())
    return path


def parse_output(text):
    """{(what, file, channel): float64 array} of the checker's lines, from their hexadecimal words."""
    out = {}
    for line in text.splitlines():
        part = line.split()
        if part and part[0] in ("seg", "row"):
            out[part[0], part[1], int(part[2])] = np.array([int(w, 16) for w in part[3:]], np.uint64).view(np.float64)
    return out
