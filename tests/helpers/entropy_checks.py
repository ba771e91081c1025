"""A noisy walker, a yardstick in plain loops over every pair of templates and a hand-made case for the sample entropy of the gait signals (DESIGN
4.17), shared by the host and the GPU tests.  Nothing here calls the code under test.

THE YARDSTICK.  Rules 2 to 7 as plain loops over frames and over EVERY PAIR (i, j), i < j, on Python floats and integers, one operation a line: what
the statement (numpy, one offset at a time), the host checker and the kernels (circular offsets) must equal in every integer and bit.

THE NOISY CALL.  regularity_checks.build_call's seven sequences with seeded Gaussian noise of 5 mm on every joint coordinate: the stock walker is free
of noise, so nearly every pair of its templates matches or none does.  THE CONDITION ON THE INPUTS, no tolerance, asserted here: on the 400-frame
walker A >= 100 at scale 1 on every odd channel for derivative 0, 1 and 2 (m = 2, fraction 0.2), so that the counts the tests compare are no handful.

THE HAND CASE.  regularity_checks.HAND_X, 31 integer frames of period 7 with frame 14 missing.  Its counts are written out below and re-derived by the
yardstick in the host test."""
import functools
import math

import numpy as np

from . import gait_checks as gc
from . import regularity_checks as rc

NOISE = 0.005                                                   # metres, on every coordinate
SEED = 2011
RULE = dict(m=2, fraction=0.2, derivative=2, scales=3)
# (m, derivative, scales): every value of each that the tests name, without their whole product
RULES = ((2, 2, 3), (1, 0, 1), (4, 1, 8), (1, 2, 8), (2, 0, 3), (4, 2, 1), (2, 1, 3))


def yardstick(x, exclude=None, m=2, fraction=0.2, derivative=2, scales=3):
    """(counts: scales rows [valid templates, B, A], row: [n, mu, SD, r]) of ONE signal of ONE sequence, as loops on Python floats."""
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
    r = fraction * sd
    counts = []
    for tau in range(1, scales + 1):
        N = T // tau
        z = []
        for j in range(N):
            s = y[j * tau]
            for k in range(1, tau):
                s = s + y[j * tau + k]
            s = s / tau
            z.append(s if math.isfinite(s) else nan)
        ok = [all(math.isfinite(z[i + k]) for k in range(m + 1)) for i in range(max(N - m, 0))]
        B = A = 0
        if r > 0:
            for i in range(len(ok)):
                if not ok[i]:
                    continue
                for j in range(i + 1, len(ok)):
                    if not ok[j]:
                        continue
                    for k in range(m):
                        if not abs(z[i + k] - z[j + k]) <= r:
                            break
                    else:
                        B += 1
                        if abs(z[i + m] - z[j + m]) <= r:
                            A += 1
        counts.append([sum(ok), B, A])
    return counts, [float(n), mu, sd, r]


def yardstick_call(per_frame, lengths, exclude=None, **rule):
    """The yardstick over a call's signals (n,4): (counts (n_seq,4,scales,3) int64, per_sequence (n_seq,4,4))."""
    counts, rows, a = [], [], 0
    for T in lengths:
        made = [yardstick(per_frame[a:a + T, ch], None if exclude is None else exclude[a:a + T], **rule) for ch in range(4)]
        counts.append([m[0] for m in made])
        rows.append([m[1] for m in made])
        a += T
    return np.array(counts, np.int64), np.array(rows)


def yardstick_sampen(counts, min_templates=50):
    """ln(B / A) per row of counts, NaN by rule 8, and their sum in order."""
    out = []
    for templates, B, A in counts:
        out.append(math.log(B / A) if templates >= min_templates and A > 0 and B > 0 else float("nan"))
    total = 0.0
    for v in out:
        total = total + v
    return out, total


@functools.lru_cache(maxsize=None)
def noisy_call(J=25):
    """(joints float32, trans with two NaN rows, lengths, names, exclude, table) of the seven noisy sequences of one call; the condition on the inputs
    is asserted here."""
    table = gc.KINECTV2 if J == 25 else gc.OTHER49
    joints, trans, lengths, names = rc.build_call(J, table)
    rng = np.random.default_rng(SEED + J)
    joints = (joints.astype(np.float64) + NOISE * rng.standard_normal(joints.shape)).astype(np.float32)
    still = names.index("standing64")
    a = sum(lengths[:still])
    joints[a:a + 64] = rc.build_call(J, table)[0][a:a + 64]    # the standing body stays still: r = 0
    trans = trans.copy()
    trans[[5, 200]] = np.nan
    ex = np.zeros(sum(lengths), np.int32)
    a = 0
    for T in lengths:
        ex[a + 60:a + min(T, 70)] = 2
        if T > 3:
            ex[a + 3] = 1
        a += T
    a = sum(lengths[:names.index("walk400_back")])
    signals = rc.signals_of(joints[a:a + 400], trans[a:a + 400], table)
    for d in (0, 1, 2):
        for ch in range(3):
            counts, _ = yardstick(signals[:, ch], None, 2, 0.2, d, 1)
            assert counts[0][2] >= 100, f"J {J}: A = {counts[0][2]} at derivative {d} on channel {ch}: not a fair input"
    return joints, trans, lengths, names, ex, table


def exclude_straddle(T):
    """A mask whose excluded frame 7 lies inside the coarse-graining windows [6, 7] of scale 2 and [6, 8] of scale 3."""
    ex = np.zeros(T, np.int32)
    ex[7] = 1
    return ex


def same_bits(a, b):
    return gc.same_bits(a, b)


def same_counts(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype.kind in "iu" and b.dtype.kind in "iu" and bool((a == b).all())


# THE HAND CASE: per rule, n, SD and the (valid templates, B, A) of scales 1 and 2 on every channel.
# derivative 0, m 2: 29 templates of which 12, 13 and 14 hold frame 14; at scale 2 z(7) is missing, of 13 templates 5, 6 and 7.
# derivative 1, m 1: y(13), y(14) and y(30) are missing, so templates 12, 13, 14 and 29 of 30; at scale 2 z(6) and z(7), of 14 templates 5, 6 and 7.
HAND_CASES = ((dict(m=2, fraction=0.5, derivative=0, scales=2), 30, 2.181426297094443, ((26, 96, 52), (10, 4, 4))),
              (dict(m=1, fraction=0.2, derivative=1, scales=2), 28, 2.5142451295425774, ((26, 68, 23), (11, 12, 6))))


def hand_signals():
    x = np.array([np.nan if v is None else float(v) for v in rc.HAND_X])
    return np.repeat(x[:, None], 4, axis=1)


def write_case(path, joints, table, trans, signals, exclude, rule, host):
    """The file tests/helpers/gait_entropy_check.cpp reads: ONE sequence, its inputs and the statement's result `host` with sigma = 0 (None: a case
    that the program must refuse, and says why).  joints None: a case on given signals (T,4)."""
    T = signals.shape[0] if joints is None else joints.shape[0]
    J = 0 if joints is None else joints.shape[1]
    with open(path, "wb") as f:
        f.write(np.array([T, J, trans is not None, exclude is not None, rule["m"], rule["derivative"], rule["scales"], host is not None], "<i4").tobytes())
        f.write(np.asarray(table, "<i4").tobytes())
        f.write(np.array([rule["fraction"]], "<f8").tobytes())
        if host is None:
            return path
        f.write(np.ascontiguousarray(signals, "<f8").tobytes() if joints is None else np.ascontiguousarray(joints, "<f4").tobytes())
        if trans is not None:
            f.write(np.ascontiguousarray(trans, "<f8").tobytes())
        if exclude is not None:
            f.write(np.ascontiguousarray(exclude, "<i4").tobytes())
        if joints is not None:
            f.write(np.ascontiguousarray(host["per_frame"], "<f8").tobytes())
        f.write(np.ascontiguousarray(host["counts"][0], "<i8").tobytes() + np.ascontiguousarray(host["per_sequence"][0], "<f8").tobytes())
    return path


# WHITE NOISE, the statistical anchor: of standard-normal samples (derivative 0, m = 2) two values lie within r = fraction SD of each other with
# probability erf(fraction / 2), whatever came before, so SampEn = -ln erf(fraction / 2); at scale tau the SD has shrunk by sqrt(tau) while r stays:
# -ln erf(fraction sqrt(tau) / 2).  MEASURED is what the yardstick itself misses that by over WHITE_SEEDS (measure_white, recorded in
# profiles/gait_entropy_bounds.txt): the finite-sample error of the estimator, not an error of the code.  The bars are twice these.
WHITE_T, WHITE_FRACTION, WHITE_SEEDS = 4000, 0.2, tuple(range(20))
WHITE_MEASURED = {1: 0.0335, 2: 0.0420}                       # rounded up in the fourth place


def white_noise(seed):
    return np.random.default_rng(seed).standard_normal(WHITE_T)


def white_closed(tau):
    return -math.log(math.erf(WHITE_FRACTION * math.sqrt(tau) / 2.0))


def measure_white():
    """{tau: the yardstick's worst miss of the closed form over WHITE_SEEDS} and the lines of the record."""
    worst, lines = {1: 0.0, 2: 0.0}, []
    for seed in WHITE_SEEDS:
        counts, _ = yardstick(white_noise(seed), None, 2, WHITE_FRACTION, 0, 2)
        got, _ = yardstick_sampen(counts)
        for tau in (1, 2):
            worst[tau] = max(worst[tau], abs(got[tau - 1] - white_closed(tau)))
        lines.append(f"seed {seed:2d}: counts {counts}, SampEn {got[0]:.5f} {got[1]:.5f}")
    return worst, lines
