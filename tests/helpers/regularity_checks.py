"""A walker with a known autocorrelation, a yardstick in plain loops and the bars of gait regularity and symmetry, shared by the host
and the GPU tests.  Nothing here calls the code under test.

THE WALKER.  gait_checks.walker's skeleton with four changes: the left ankle swings A (sin p + B sin(2 p + psi)), p = 2 pi (t + phi) / P, ahead of
the pelvis -- B = 0 a symmetric walk, B = 0.3 one whose left and right steps differ; the right ankle swings -1 times the left; spine-shoulder sways
0.03 m sin(p + 0.7) to the left, period P; the pelvis bobs 0.02 m cos(2 p + 0.4), period P / 2, in `trans`.  P is no integer.

THE CLOSED FORM for sep = (lankle - rankle) . f = 2 A (sin p + B sin(2 p + psi)) over many periods: rho(m) = (cos(2 pi m / P) + B^2 cos(4 pi m / P)) /
(1 + B^2); stride regularity rho(P) = 1, step regularity -rho(P / 2) = (1 - B^2) / (1 + B^2), which is the symmetry: 0.835 at B = 0.3.

THE YARDSTICK.  Rules 4 to 7 as plain loops over frames and lags on Python floats, one operation a line: what the statement (numpy) and the kernels
must equal in every bit.

THE BARS are twice what the yardstick itself misses the closed form by on the named inputs (P of PERIODS, YAWS, PHASES, T = 400 and 130, lags up to
60), measured on the CPU and recorded in profiles/gait_regularity_bounds.txt: the finite-sample error of the estimator, not an error of the code.

THE CONDITION ON THE INPUTS, no tolerance: the integer lags found on every walker used equal round(P) or its neighbour and round(P / 2) or its
neighbour (assert_lags)."""
import math

import numpy as np

from . import gait_checks as gc

FPS = 20.0
PERIODS = (21.7, 27.3, 33.1, 19.3)
YAWS = (0.0, np.deg2rad(40.0), np.pi)
PHASES = (0.0, 0.37, 0.71)                                      # phi as a share of the period
ASYMMETRY = 0.3
RULE = dict(max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20)
# measured by measure_bounds() (profiles/gait_regularity_bounds.txt); the bars are twice these
MEASURED = {400: {0.0: dict(stride_lag=0.0619, step_lag=0.0596, rho=0.0127, symmetry=0.0047), 0.3: dict(stride_lag=0.0808, step_lag=0.1875, rho=0.0180, symmetry=0.0091)},
            130: {0.0: dict(stride_lag=0.2064, step_lag=0.1770, rho=0.0521, symmetry=0.0050), 0.3: dict(stride_lag=0.1606, step_lag=0.9214, rho=0.1000, symmetry=0.0335)}}


def bars(T, B):
    return {k: 2.0 * v for k, v in MEASURED[T][B].items()}


def walker(T, P=21.7, B=0.0, theta=0.0, phi=0.0, psi=0.9, A=0.3, J=25, table=gc.KINECTV2, degenerate=(), still=False):
    """(joints (T,J,3) float32, trans (T,3) float64).  still: a standing body whose four signals are constant and exactly representable sums (theta
    must be 0): every amplitude 0."""
    t = np.arange(T, dtype=np.float64)
    c, s = np.cos(theta), np.sin(theta)
    fwd, left, up = np.array([-s, 0.0, -c]), np.array([c, 0.0, -s]), np.array([0.0, -1.0, 0.0])
    body = np.zeros((T, J, 3))
    body[:, :, 0] = 0.01 * np.arange(J)[None, :]
    body[:, :, 1] = 0.02 * ((np.arange(J) % 5) - 2)[None, :]
    body[:, :, 2] = 0.03 * ((np.arange(J) % 7) - 3)[None, :]
    p = 2.0 * np.pi * (t + phi) / P
    amp = 0.0 if still else 1.0
    swing = amp * A * (np.sin(p) + B * np.sin(2.0 * p + psi))
    sway = amp * 0.03 * np.sin(p + 0.7)
    zero = np.zeros(T)
    for k, (a, b, h) in enumerate(((zero, zero, 0.0), (zero, sway, 0.5), (zero, zero + 0.125, 0.0), (zero, zero - 0.125, 0.0), (swing, zero + 0.125, -0.75),
                                   (-swing, zero - 0.125, -0.75), (swing, zero + 0.125, -0.875), (-swing, zero - 0.125, -0.875))):
        body[:, table[k], 0], body[:, table[k], 1], body[:, table[k], 2] = a, b, h
    for f in degenerate:
        body[f, table[2]] = body[f, table[3]]
    joints = body[:, :, 0:1] * fwd + body[:, :, 1:2] * left + body[:, :, 2:3] * up
    trans = np.array([0.25, 0.125, 6.0]) + (gc.walker_speed(A, P, 1.0) * amp * t)[:, None] * fwd
    trans[:, 1] += amp * 0.02 * np.cos(2.0 * p + 0.4)
    return joints.astype(np.float32), trans


def closed_form(m, P, B):
    m = np.asarray(m, np.float64)
    return (np.cos(2.0 * np.pi * m / P) + B * B * np.cos(4.0 * np.pi * m / P)) / (1.0 + B * B)


def closed_symmetry(B):
    return (1.0 - B * B) / (1.0 + B * B)


def pair_counts(valid, max_lag):
    """N(m) by loops over frames and the frames between them: a pair counts where no frame from t to t + m fails."""
    T = len(valid)
    N = [0] * (max_lag + 1)
    for m in range(max_lag + 1):
        for t in range(T - m):
            if all(valid[t:t + m + 1]):
                N[m] += 1
    return N


def yardstick(x, odd, exclude=None, fps=FPS, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20):
    """(acf: list of max_lag + 1 floats, row: list of 10 floats) of ONE signal of ONE sequence by rules 4 to 8, as loops on Python floats."""
    nan = float("nan")
    x = [float(v) for v in x]
    T = len(x)
    valid = [math.isfinite(x[t]) and (exclude is None or int(exclude[t]) == 0) for t in range(T)]
    run, before = [], 0
    for t in range(T):
        run.append(before)
        if not valid[t]:
            before += 1
    n, S = 0, 0.0
    for t in range(T):
        if valid[t]:
            S = S + x[t]
            n += 1
    acf, row = [nan] * (max_lag + 1), [nan] * 10
    row[0] = float(n)
    if n == 0:
        return acf, row
    mu = S / n
    d = [x[t] - mu if valid[t] else nan for t in range(T)]
    sums, N = [], []
    for m in range(max_lag + 1):
        acc, count = 0.0, 0
        for t in range(T - m):
            if valid[t] and valid[t + m] and run[t] == run[t + m]:
                prod = d[t] * d[t + m]
                acc = acc + prod
                count += 1
        sums.append(acc)
        N.append(count)
    if N[0] < min_pairs or not sums[0] / N[0] > 0.0:
        return acf, row
    A0 = sums[0] / N[0]
    row[1] = A0
    for m in range(max_lag + 1):
        if N[m] >= min_pairs:
            acf[m] = (sums[m] / N[m]) / A0

    def extremum(m, sign):
        if m < 1 or m > max_lag - 1:
            return False
        a, b, c = sign * acf[m - 1], sign * acf[m], sign * acf[m + 1]
        return b > a and b >= c                                # false where one is NaN

    def refine(m):
        a, b, c = acf[m - 1], acf[m], acf[m + 1]
        den = (a - 2.0 * b) + c
        return float(m) if den == 0.0 else m + (0.5 * (a - c)) / den

    first = -1
    for m in range(min_lag, max_lag):
        if extremum(m, 1.0) and acf[m] >= min_peak:
            first = m
            break
    d1 = d2 = -1
    if odd:
        d2 = first
        if d2 >= 0:
            for m in range(d2 - (3 * d2) // 4, d2 - d2 // 4 + 1):
                if extremum(m, -1.0) and (d1 < 0 or acf[m] < acf[d1]):
                    d1 = m
    else:
        d1 = first
        if d1 >= 0:
            for m in range(max(2 * d1 - d1 // 2, 1), min(2 * d1 + d1 // 2, max_lag - 1) + 1):
                if extremum(m, 1.0) and (d2 < 0 or acf[m] > acf[d2]):
                    d2 = m
    row[2], row[5] = float(d1), float(d2)
    if d1 >= 0:
        row[3], row[4] = refine(d1), (-acf[d1] if odd else acf[d1])
    if d2 >= 0:
        row[6], row[7] = refine(d2), acf[d2]
        row[9] = (120.0 * fps) / row[6]
        if d1 >= 0 and row[7] > 0.0:
            row[8] = row[4] / row[7]
    return acf, row


def yardstick_call(per_frame, lengths, exclude=None, **rule):
    """The yardstick over a call's signals (n,4): (acf (n_seq,4,max_lag+1), per_sequence (n_seq,4,10))."""
    acf, rows, a = [], [], 0
    for T in lengths:
        made = [yardstick(per_frame[a:a + T, ch], ch < 3, None if exclude is None else exclude[a:a + T], **rule) for ch in range(4)]
        acf.append([m[0] for m in made])
        rows.append([m[1] for m in made])
        a += T
    return np.array(acf), np.array(rows)


def signals_of(joints, trans, table=gc.KINECTV2):
    """The four signals of rule 2 frame by frame on Python floats (n,4): what every implementation's per_frame must equal with sigma = 0."""
    n = joints.shape[0]
    out = np.full((n, 4), np.nan)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    for t in range(n):
        p = [[float(v) for v in joints[t, k]] for k in table[:6]]
        if trans is not None and all(math.isfinite(v) for v in trans[t]):
            out[t, 3] = -(p[0][1] + float(trans[t, 1]))
        l = [p[2][a] - p[3][a] for a in range(3)]
        u = [p[1][a] - p[0][a] for a in range(3)]
        c = [l[1] * u[2] - l[2] * u[1], l[2] * u[0] - l[0] * u[2], l[0] * u[1] - l[1] * u[0]]
        nc, nl = math.sqrt(dot(c, c)), math.sqrt(dot(l, l))
        if not (nc > 0 and math.isfinite(nc) and nl > 0 and math.isfinite(nl)):
            continue
        nu = math.sqrt(dot(u, u))
        f, side, up = [v / nc for v in c], [v / nl for v in l], [v / nu for v in u]
        d = [p[4][a] - p[5][a] for a in range(3)]
        out[t, 0], out[t, 1], out[t, 2] = dot(d, f), dot(d, up), dot(up, side)
    return out


def assert_lags(row, P):
    """The condition on the inputs: the integer lags of a walker of period P, of an odd channel or of bob, which repeats every P / 2."""
    stride, step = P, P / 2.0
    d1, d2 = int(row[2]), int(row[5])
    assert abs(d2 - round(stride)) <= 1 and abs(d1 - round(step)) <= 1, f"P {P}: lags {d1} and {d2}: not a fair input"


def measure_bounds(T, B):
    """What the yardstick misses the closed form by on sep over PERIODS x YAWS x PHASES: {'stride_lag', 'step_lag', 'rho', 'symmetry'}."""
    worst = dict(stride_lag=0.0, step_lag=0.0, rho=0.0, symmetry=0.0)
    for P in PERIODS:
        for theta in YAWS:
            for share in PHASES:
                joints, trans = walker(T, P, B, theta, share * P)
                acf, row = yardstick(signals_of(joints, trans)[:, 0], True, **RULE)
                assert_lags(row, P)
                acf = np.array(acf)
                ok = np.isfinite(acf)
                worst["rho"] = max(worst["rho"], float(np.abs(acf[ok] - closed_form(np.arange(61)[ok], P, B)).max()))
                worst["stride_lag"] = max(worst["stride_lag"], abs(row[6] - P))
                worst["step_lag"] = max(worst["step_lag"], abs(row[3] - P / 2))
                worst["symmetry"] = max(worst["symmetry"], abs(row[8] - closed_symmetry(B)))
    return worst


def same_bits(a, b):
    return gc.same_bits(a, b)


# THE HAND-MADE SIGNAL: integers of mean 0 over the frames that count, so that d = x, every product and every sum is an integer and exact; frame 14 is
# NaN and splits two runs.  With max_lag = 8, min_lag = 2, min_pairs = 2, min_peak = 0.25: rho(m) = (HAND_SUMS[m] / HAND_N[m]) / (HAND_SUMS[0] / HAND_N[0]).
HAND_RULE = dict(fps=20.0, max_lag=8, min_lag=2, min_peak=0.25, min_pairs=2)
HAND_X = (-2, -3, 2, 2, 2, 1, -3, -2, -2, 2, 2, 2, 1, -3, None, -2, 2, 2, 2, 1, -3, -2, -2, 3, 2, 2, 1, -3, -2, -2, 2)      # 31 frames, a period of 7
HAND_SUMS = (138, 42, -22, -84, -77, 1, 38, 74, 12)            # the sum of x(t) x(t + m) over the pairs that the NaN frame does not part
HAND_N = (30, 28, 26, 24, 22, 20, 18, 16, 14)                  # 31 - m pairs less the m + 1 that hold frame 14, where m <= 14
HAND_A0 = 138 / 30
HAND_RHO = tuple((s / n) / HAND_A0 for s, n in zip(HAND_SUMS, HAND_N))
# rho(7) = 4.625 / 4.6 passes 1 and is not clipped: the first peak, at max_lag - 1.  rho(3) = rho(4) = -3.5 / 4.6, a plateau: lag 3, the earlier, is
# the minimum of [7 - 5, 7 - 1], and rule 7 puts it at 3 + 0.5 (a - b) / (a - b) = 3.5.  Lag 1 is no maximum (rho(0) is larger) and lag 6 is none.
_HAND_D2 = 7 + (0.5 * (HAND_RHO[6] - HAND_RHO[8])) / ((HAND_RHO[6] - 2.0 * HAND_RHO[7]) + HAND_RHO[8])
HAND_ROW_ODD = (30.0, HAND_A0, 3.0, 3.5, -HAND_RHO[3], 7.0, _HAND_D2, HAND_RHO[7], -HAND_RHO[3] / HAND_RHO[7], (120.0 * 20.0) / _HAND_D2)
# an even channel: the first peak is the step, and the stride's window [14 - 3, 14 + 3] lies past max_lag - 1
HAND_ROW_EVEN = (30.0, HAND_A0, 7.0, _HAND_D2, HAND_RHO[7], -1.0, float("nan"), float("nan"), float("nan"), float("nan"))


def hand_case():
    """(signals (31,4): the hand-made signal in every channel, the expected acf (4,9), the expected per_sequence (4,10))."""
    x = np.array([np.nan if v is None else float(v) for v in HAND_X])
    return np.repeat(x[:, None], 4, axis=1), np.array([HAND_RHO] * 4), np.array([HAND_ROW_ODD] * 3 + [HAND_ROW_EVEN])


def write_case(path, joints, table, trans, signals, exclude, rule, host):
    """The file tests/helpers/gait_regularity_check.cpp reads: ONE sequence, its inputs and the statement's result `host` with sigma = 0.  joints None:
    a case on given signals (T,4)."""
    T = signals.shape[0] if joints is None else joints.shape[0]
    J = 0 if joints is None else joints.shape[1]
    with open(path, "wb") as f:
        f.write(np.array([T, J, trans is not None, exclude is not None, rule["max_lag"], rule["min_lag"], rule["min_pairs"]], "<i4").tobytes())
        f.write(np.asarray(table, "<i4").tobytes())
        f.write(np.array([rule["fps"], rule["min_peak"]], "<f8").tobytes())
        f.write(np.ascontiguousarray(signals, "<f8").tobytes() if joints is None else np.ascontiguousarray(joints, "<f4").tobytes())
        if trans is not None:
            f.write(np.ascontiguousarray(trans, "<f8").tobytes())
        if exclude is not None:
            f.write(np.ascontiguousarray(exclude, "<i4").tobytes())
        if joints is not None:
            f.write(np.ascontiguousarray(host["per_frame"], "<f8").tobytes())
        f.write(np.ascontiguousarray(host["acf"][0], "<f8").tobytes() + np.ascontiguousarray(host["per_sequence"][0], "<f8").tobytes())
    return path


def build_call(J=25, table=gc.KINECTV2):
    """The seven sequences of the device tests in one call: (joints, trans, lengths, names).  Lengths 1, 19 and 20 (min_pairs = 20: the first that
    defines rho(0)), a standing body of 64 frames, 65 frames with one degenerate frame, and walks of 130 and 400 frames at other yaws and periods."""
    parts = (("walk130", dict(T=130, P=21.7, B=0.3, theta=0.7, phi=3.0)), ("one", dict(T=1, theta=0.2)), ("nineteen", dict(T=19, P=19.3, theta=0.3)),
             ("twenty", dict(T=20, P=19.3, theta=0.4)), ("standing64", dict(T=64, still=True)),
             ("degenerate65", dict(T=65, P=19.3, theta=-1.1, phi=2.2, degenerate=(30,))), ("walk400_back", dict(T=400, P=27.3, theta=np.pi - 0.4, phi=1.9)))
    made = [walker(J=J, table=table, **kw) for _, kw in parts]
    return np.concatenate([m[0] for m in made]), np.concatenate([m[1] for m in made]), [kw["T"] for _, kw in parts], [name for name, _ in parts]
