"""A yardstick in plain loops over every pair of points, hand-made integer cases and white noise for the recurrence quantification of the gait
signals, shared by the host and the GPU tests.  Nothing here calls the code under test.

THE YARDSTICK.  Rules 1 (from the differencing on) to 7 as plain loops over frames and over EVERY PAIR (i, j) OF THE TRIANGLE, DIAGONAL BY DIAGONAL,
on Python floats and integers, one operation a line, with math.log: what the statement (numpy, a diagonal at a time, the runs by differences of a
padded boolean vector), the host checker and the kernels (a lane per circular offset, which walks two diagonals) must equal in every integer and bit.
Its differencing and its distance are its own, as stability_checks has its own.

THE NOISY CALL.  entropy_checks.noisy_call: sequences of 1, 19, 20, 64, 65, 130 and 400 frames with seeded noise of 5 mm.  THE CONDITION ON THE
INPUTS, no tolerance, asserted by noisy_call here on the yardstick alone: at the default rule and derivative 0, 1 and 2 the 400-frame walker has on
every channel recurrent >= 1000, at least 100 lines of 2 pairs and more, and longest >= 5.

THE HAND CASES.  x = (0, 1, 3, 1, -2) six times and one more 0, 31 frames, derivative 0, dim 2, lag 1, theiler 0.  n = 31, mu = 18 / 31, SD =
1.6283773835403774.  The points of the five phases are p0 (0,1), p1 (1,3), p2 (3,1), p3 (1,-2), p4 (-2,0), and D2 between two different phases is
at least 5 (p0-p1 and p0-p4), between points of one phase 0.  M = 30 points, 30 29 / 2 = 435 pairs.
HAND_PERIODIC, radius 0.5: eps2 = (0.5 SD)^2 2 = 1.3258.. < 5, so a pair recurs iff i = j mod 5: the diagonals 5, 10, 15, 20 and 25 are recurrent
from end to end and nothing else is -- one line each of 25, 20, 15, 10 and 5 pairs, 75 recurrent pairs.  Rows: rate 75 / 435, determinism 1, mean
line 15, longest 25, divergence 1 / 25, line entropy ln 5 (five classes of one line).  Offsets 5 and 25, and 10 and 20, are one circular offset of
M = 30: a run carried across the wrap would read 30.
HAND_WIDE, radius 1.0: eps2 = 5.3032.. >= 5, so p0-p1 and p0-p4 recur too.  The constants -- 147 recurrent pairs, 12 lines of 1, 30 of 2 and the
five long diagonals, 35 lines of 135 points at min_line 2 -- were made once by a sketch, are re-derived by the yardstick in the host test and are
stated here as constants.
HAND_LONG, the period 120 times (600 frames), radius 0.5: M = 599, the diagonals 5, 10, .., 595 with 594, 589, .., 4 pairs: 119 lines, of which the
51 of 4 .. 254 are in hist and the 68 of 259 .. 594 are long ones with 29 002 points; longest 594.
HAND_BROKEN: HAND_PERIODIC with frames 7, 13 and 22 changed and frame 17 missing at dim 3, lag 2, theiler 2, radius 0.5; its constants were MADE
ONCE BY THE YARDSTICK and are re-derived by it in the host test.

THE ANCHOR.  White noise: of standard-normal samples at dim 2 with no shared sample (lag 1, theiler 1) D2 / 2 is chi-squared with 2 degrees of
freedom, so a pair recurs with probability 1 - exp(-eps2 / 4) = 1 - exp(-radius^2 SD^2 / 2) -> 1 - e^(-1/2) = 0.39347 at radius 1."""
import functools
import math

import numpy as np

from . import entropy_checks as ec
from . import gait_checks as gc
from . import regularity_checks as rc

BINS = 255
RULE = dict(derivative=1, dim=5, lag=2, theiler=8, radius=0.8)
# (derivative, dim, lag, theiler, radius): every value of each that the tests name, without their whole product; 500 is larger than every M
RULES = ((1, 5, 2, 8, 0.8), (0, 2, 1, 0, 0.2), (2, 8, 16, 8, 10.0), (0, 5, 16, 500, 0.8), (2, 2, 2, 0, 0.8), (1, 8, 1, 1, 0.2), (0, 5, 2, 8, 0.8), (2, 5, 2, 8, 0.8))
ROWS = ("lines", "line_points", "recurrence_rate", "determinism", "mean_line", "longest", "divergence", "line_entropy", "ratio")


def rule_of(d, dim, lag, theiler, radius):
    return dict(derivative=d, dim=dim, lag=lag, theiler=theiler, radius=radius)


def differenced(x, exclude, derivative):
    nan = float("nan")
    x = [float(v) for v in x]
    T = len(x)
    y = [x[t] if math.isfinite(x[t]) and (exclude is None or int(exclude[t]) == 0) else nan for t in range(T)]
    for _ in range(derivative):
        nxt = []
        for t in range(T):
            if t + 1 < T and math.isfinite(y[t]) and math.isfinite(y[t + 1]):
                v = y[t + 1] - y[t]
                nxt.append(v if math.isfinite(v) else nan)
            else:
                nxt.append(nan)
        y = nxt
    return y


def dist2(y, a, b, dim, lag):
    t = y[a] - y[b]
    s = t * t
    for c in range(1, dim):
        t = y[a + c * lag] - y[b + c * lag]
        s = s + t * t
    return s


def yardstick(x, exclude=None, derivative=1, dim=5, lag=2, theiler=8, radius=0.8):
    """(row: [n, mu, SD, r, eps2], hist: BINS integers, counts: [points, comparable, recurrent, long_lines, long_points, longest]) of ONE signal of
    ONE sequence, as loops on Python floats."""
    nan = float("nan")
    y = differenced(x, exclude, derivative)
    T = len(y)
    n, S = 0, 0.0
    for t in range(T):
        if math.isfinite(y[t]):
            S = S + y[t]
            n += 1
    mu = S / n if n else nan
    Q = 0.0
    for t in range(T):
        if math.isfinite(y[t]):
            e = y[t] - mu
            Q = Q + e * e
    sd = math.sqrt(Q / (n - 1)) if n >= 2 else nan
    r = radius * sd
    eps2 = (r * r) * float(dim)
    M = max(T - (dim - 1) * lag, 0)
    valid = [all(math.isfinite(y[i + k * lag]) for k in range(dim)) for i in range(M)]
    hist = [0] * BINS
    comparable = recurrent = long_lines = long_points = longest = 0

    def close(run):
        nonlocal long_lines, long_points, longest
        if run == 0:
            return
        if run <= BINS:
            hist[run - 1] += 1
        else:
            long_lines += 1
            long_points += run
        longest = max(longest, run)

    for s in range(theiler + 1, M):
        run = 0
        for i in range(M - s):
            j = i + s
            hit = False
            if valid[i] and valid[j]:
                comparable += 1
                d2 = dist2(y, i, j, dim, lag)
                if r > 0 and math.isfinite(d2) and d2 <= eps2:
                    hit = True
            if hit:
                recurrent += 1
                run += 1
            else:
                close(run)
                run = 0
        close(run)
    return [float(n), mu, sd, r, eps2], hist, [sum(valid), comparable, recurrent, long_lines, long_points, longest]


def yardstick_rows(counts, hist, min_line=2, min_points=50):
    """{name: value} of one (sequence, channel) by rule 7, on Python integers and floats."""
    nan = float("nan")
    points, comparable, recurrent, long_lines, long_points, longest = counts
    lines, line_points = long_lines, long_points
    for length in range(min_line, BINS + 1):
        lines += hist[length - 1]
        line_points += length * hist[length - 1]
    row = dict.fromkeys(ROWS, nan)
    row["lines"], row["line_points"] = lines, line_points
    if points < min_points:
        return row
    if comparable > 0:
        row["recurrence_rate"] = recurrent / comparable
    if recurrent > 0:
        row["determinism"] = line_points / recurrent
    if lines > 0:
        row["mean_line"] = line_points / lines
        acc = 0.0
        for length in range(min_line, BINS + 1):
            if hist[length - 1] > 0:
                p = hist[length - 1] / lines
                acc = acc + p * math.log(p)
        if long_lines > 0:
            p = long_lines / lines
            acc = acc + p * math.log(p)
        row["line_entropy"] = -acc
    if longest >= min_line:
        row["longest"] = float(longest)
        row["divergence"] = 1.0 / longest
    if comparable > 0 and recurrent > 0:
        row["ratio"] = row["determinism"] / row["recurrence_rate"]
    return row


def yardstick_call(per_frame, lengths, exclude=None, **rule):
    """The yardstick over a call's signals (n,4): (per_sequence (n_seq,4,5), hist (n_seq,4,255) int64, counts (n_seq,4,6) int64)."""
    rows, hist, counts, a = [], [], [], 0
    for T in lengths:
        made = [yardstick(per_frame[a:a + T, ch], None if exclude is None else exclude[a:a + T], **rule) for ch in range(4)]
        rows.append([m[0] for m in made])
        hist.append([m[1] for m in made])
        counts.append([m[2] for m in made])
        a += T
    return np.array(rows), np.array(hist, np.int64), np.array(counts, np.int64)


def invariant(hist, counts):
    """Rule 6: the lines' points are the recurrent pairs, everywhere."""
    hist, counts = np.asarray(hist), np.asarray(counts)
    return bool(((hist * np.arange(1, BINS + 1)).sum(axis=-1) + counts[..., 4] == counts[..., 2]).all())


@functools.lru_cache(maxsize=None)
def noisy_call(J=25):
    """entropy_checks.noisy_call, with this call's condition on the inputs asserted on the yardstick."""
    joints, trans, lengths, names, ex, table = ec.noisy_call(J)
    a = sum(lengths[:names.index("walk400_back")])
    signals = rc.signals_of(joints[a:a + 400], trans[a:a + 400], table)
    for d in (0, 1, 2):
        for ch in range(4):
            _, hist, counts = yardstick(signals[:, ch], None, **dict(RULE, derivative=d))
            lines = sum(hist[1:]) + counts[3]
            assert counts[2] >= 1000 and lines >= 100 and counts[5] >= 5, \
                f"J {J}, derivative {d}, channel {ch}: recurrent {counts[2]}, lines {lines}, longest {counts[5]}: not a fair input"
    return joints, trans, lengths, names, ex, table


def same_bits(a, b):
    return gc.same_bits(a, b)


def same_ints(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype.kind in "iu" and b.dtype.kind in "iu" and bool((a == b).all())


def hist_of(lines):
    """BINS integers from {length: lines}."""
    out = [0] * BINS
    for length, k in lines.items():
        out[length - 1] = k
    return out


HAND_SD = 1.6283773835403774                                  # to the last place or so: the tests hold it within 1e-15
HAND_PERIODIC_X = (0, 1, 3, 1, -2) * 6 + (0,)
HAND_PERIODIC_RULE = dict(derivative=0, dim=2, lag=1, theiler=0, radius=0.5)
HAND_PERIODIC_COUNTS = [30, 435, 75, 0, 0, 25]
HAND_PERIODIC_HIST = hist_of({25: 1, 20: 1, 15: 1, 10: 1, 5: 1})
HAND_WIDE_RULE = dict(HAND_PERIODIC_RULE, radius=1.0)
HAND_WIDE_COUNTS = [30, 435, 147, 0, 0, 25]
HAND_WIDE_HIST = hist_of({1: 12, 2: 30, 25: 1, 20: 1, 15: 1, 10: 1, 5: 1})
HAND_WIDE_LINES = (35, 135)                                    # lines and their points at min_line 2
HAND_LONG_X = (0, 1, 3, 1, -2) * 120
HAND_LONG_COUNTS = [599, 179101, 35581, 68, 29002, 594]
HAND_LONG_HIST = hist_of({length: 1 for length in range(4, 255, 5)})
# frames 7, 13 and 22 changed and frame 17 missing: the points 13, 15 and 17 hold frame 17 and are not valid
HAND_BROKEN_X = tuple(None if t == 17 else v + {7: 2, 13: -1, 22: 1}.get(t, 0) for t, v in enumerate(HAND_PERIODIC_X))
HAND_BROKEN_RULE = dict(derivative=0, dim=3, lag=2, theiler=2, radius=0.5)
HAND_BROKEN_COUNTS = [24, 235, 40, 0, 0, 9]
HAND_BROKEN_HIST = hist_of({1: 14, 2: 1, 3: 2, 4: 1, 5: 1, 9: 1})
HAND_CASES = ((HAND_PERIODIC_X, HAND_PERIODIC_RULE), (HAND_PERIODIC_X, HAND_WIDE_RULE), (HAND_LONG_X, HAND_PERIODIC_RULE), (HAND_BROKEN_X, HAND_BROKEN_RULE))


def hand_signals(x):
    col = np.array([np.nan if v is None else float(v) for v in x])
    return np.repeat(col[:, None], 4, axis=1)


def boundary_call():
    """Validity runs that begin and end at frames 63, 64 and 65, by NaN and by exclude (entropy's and stability's cases); the last sequence has an
    excluded frame in the middle of what is otherwise one long line: a constant signal but for a step, whose points all recur."""
    rng = np.random.default_rng(15)
    cases = ((130, (63,), ()), (130, (64,), ()), (130, (65,), (0,)), (131, (0, 1), (63, 64, 65)), (130, (62, 63), (65, 66, 129)), (66, (), (64,)), (130, range(64, 128), ()),
             (130, (), range(0, 64)), (66, range(0, 63), (65,)), (300, (), (150,)))
    lengths = [T for T, _, _ in cases]
    x = rng.standard_normal((sum(lengths), 4))
    x[-300:] = 0.001 * x[-300:] + np.repeat(np.arange(300)[:, None] >= 280, 4, axis=1)      # a small spread against one step: every early pair recurs
    ex = np.zeros(sum(lengths), np.int32)
    a = 0
    for T, nans, excluded in cases:
        x[[a + k for k in nans], :] = np.nan
        ex[[a + k for k in excluded]] = 3
        a += T
    return x, lengths, ex


def write_case(path, joints, table, trans, signals, exclude, rule, host):
    """The file tests/helpers/gait_recurrence_check.cpp reads: ONE sequence, its inputs and the statement's result `host` with sigma = 0 (None: a
    case that the program must refuse, and says why).  joints None: a case on given signals (T,4)."""
    T = signals.shape[0] if joints is None else joints.shape[0]
    J = 0 if joints is None else joints.shape[1]
    with open(path, "wb") as f:
        f.write(np.array([T, J, trans is not None, exclude is not None, rule["derivative"], rule["dim"], rule["lag"], rule["theiler"], host is not None], "<i4").tobytes())
        f.write(np.asarray(table, "<i4").tobytes())
        f.write(np.array([rule["radius"]], "<f8").tobytes())
        if host is None:
            return path
        f.write(np.ascontiguousarray(signals, "<f8").tobytes() if joints is None else np.ascontiguousarray(joints, "<f4").tobytes())
        if trans is not None:
            f.write(np.ascontiguousarray(trans, "<f8").tobytes())
        if exclude is not None:
            f.write(np.ascontiguousarray(exclude, "<i4").tobytes())
        if joints is not None:
            f.write(np.ascontiguousarray(host["per_frame"], "<f8").tobytes())
        f.write(np.ascontiguousarray(host["per_sequence"][0], "<f8").tobytes() + np.ascontiguousarray(host["hist"][0], "<i8").tobytes() +
                np.ascontiguousarray(host["counts"][0], "<i8").tobytes())
    return path


# WHITE NOISE, the statistical anchor: 1000 standard-normal samples, derivative 0, dim 2, lag 1, theiler 1 (no pair shares a sample), radius 1.0.
# MEASURED is what the yardstick itself misses the closed form by over WHITE_SEEDS (measure_white, recorded in
# profiles/gait_recurrence_bounds.txt): the finite-sample error of the estimator, not an error of the code.  The bar is twice that.
WHITE_T, WHITE_SEEDS = 1000, tuple(range(20))
WHITE_RULE = dict(derivative=0, dim=2, lag=1, theiler=1, radius=1.0)
WHITE_CLOSED = 1.0 - math.exp(-0.5)
WHITE_MEASURED = 0.0098                                        # 0.00972, rounded up in the fourth place


def white_noise(seed):
    return np.random.default_rng(seed).standard_normal(WHITE_T)


def measure_white():
    """(the yardstick's worst miss of the closed form over WHITE_SEEDS, the lines of the record)."""
    worst, lines = 0.0, []
    for seed in WHITE_SEEDS:
        row, hist, counts = yardstick(white_noise(seed), None, **WHITE_RULE)
        rate = counts[2] / counts[1]
        worst = max(worst, abs(rate - WHITE_CLOSED))
        lines.append(f"seed {seed:2d}: SD {row[2]:.5f}, comparable {counts[1]}, recurrent {counts[2]}, rate {rate:.5f}, miss {abs(rate - WHITE_CLOSED):.5f}")
    return worst, lines


BOUNDS_HEAD = """# Recurrence quantification (DESIGN 4.20): what the estimator itself misses a known recurrence rate by, measured on the CPU with the plain loops
# over every pair of tests/helpers/recurrence_checks.py (pipeline.gait_recurrence_counts, csrc/gait_recurrence.h and the kernels equal them in every
# integer).  Written by `python -m tests.helpers.recurrence_checks profiles/gait_recurrence_bounds.txt` (a quarter of a minute).
#
# WHITE NOISE: numpy.random.default_rng(seed).standard_normal(1000); derivative 0, dim 2, lag 1, theiler 1, radius 1.0.  D2 / 2 of two points that
# share no sample is chi-squared with 2 degrees of freedom, so the recurrence rate tends to 1 - exp(-1/2) = 0.39347 as SD tends to 1.
# The bar of tests/test_recurrence_host_cpu.py and tests/test_gpu_recurrence.py is twice the worst miss below (rounded up in the fourth place,
# recurrence_checks.WHITE_MEASURED).
"""


def write_bounds(path):
    """The record profiles/gait_recurrence_bounds.txt, from the yardstick alone; refuses a constant below what it measures."""
    worst, lines = measure_white()
    assert worst <= WHITE_MEASURED, f"the yardstick misses the closed form by {worst:.5f}, more than WHITE_MEASURED = {WHITE_MEASURED}"
    with open(path, "w") as f:
        f.write(BOUNDS_HEAD + "\n".join(lines) + f"\n# worst_miss\n{worst:.5f}\n")
    return worst


if __name__ == "__main__":
    import sys
    print(f"worst miss {write_bounds(sys.argv[1]):.5f}")
