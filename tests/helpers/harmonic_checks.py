"""A yardstick in plain loops, the twiddles in high precision and the closed forms of the harmonic ratios per stride, shared by the
host and the GPU tests.  Nothing here calls the code under test.

THE WALKER is regularity_checks.walker: sep = 2 A (sin p + B sin(2 p + psi)), p = 2 pi (t + phi) / P.  With an integer period P the heel strikes of one
foot lie a whole period apart, the stride closes and the trend of rule 4 is zero, so the DFT over a stride has a_1 : a_2 = 1 : B and nothing else.

THE CLOSED FORM for sep then: HR = O / E = 1 / (B 2^d), iHR = 100 / (1 + B^2 4^d) for derivative d: 3.333 and 91.74 at B = 0.3 and d = 0, 0.8333 and
40.98 at d = 2.

THE YARDSTICK.  Rules 3 to 8 as plain loops over strides, frames and harmonics on Python floats, one operation a line: what the statement (numpy), the
host checker and the kernels must equal in every bit.

THE TWIDDLE YARDSTICK is mpmath at 40 digits where it is installed, else decimal's Taylor series at 60: the true sine and cosine of 2 pi j / L.

THE BARS of the closed form are twice what the yardstick itself misses it by on the named inputs (CLOSED_CASES), measured on the CPU and recorded in
profiles/gait_harmonics_bounds.txt: rounding of float32 joints and of the sums, not an error of the code."""
import math

import numpy as np

from . import gait_checks as gc
from . import regularity_checks as rc

FPS = 20.0
RULE = dict(n_harmonics=20, derivative=2, min_stride=8, max_stride=60, max_strides=128)
TWIDDLE_BAR = 2.0 ** -51
# the closed form's inputs: 400 frames, P = 24, B and the derivative; yaw and phase as named
CLOSED_P = 24
CLOSED_CASES = tuple((B, d) for B in (0.1, 0.3, 0.6) for d in (0, 1, 2))
CLOSED_YAWS = (0.0, np.deg2rad(40.0))
CLOSED_PHASES = (0.0, 3.7)
# measured by measure_closed() (profiles/gait_harmonics_bounds.txt): the largest relative miss of HR and of iHR of any used stride, on the float64
# signal and through the walker's float32 joints; the bars are twice these
MEASURED_CLOSED = {False: dict(hr=1.364e-12, ihr=1.297e-14), True: dict(hr=3.653e-6, ihr=3.078e-8)}


def closed_bars(through_joints):
    return {k: 2.0 * v for k, v in MEASURED_CLOSED[through_joints].items()}


def closed_hr(B, d):
    return 1.0 / (B * 2.0 ** d)


def closed_ihr(B, d):
    return 100.0 / (1.0 + B * B * 4.0 ** d)


def true_twiddles(L):
    """([(sin, cos) of 2 pi j / L for j < L] in high precision, miss(a double, one of those) -> the absolute difference as a float, taken in high
    precision so that a miss of 2^-53 shows)."""
    try:
        import mpmath
    except ImportError:
        mpmath = None
    out = []
    if mpmath is not None:
        with mpmath.workdps(40):
            for j in range(L):
                a = 2 * mpmath.pi * j / L
                out.append((mpmath.sin(a), mpmath.cos(a)))
        return out, lambda got, want: abs(float(mpmath.mpf(got) - want))
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        D = decimal.Decimal
        pi = D("3.14159265358979323846264338327950288419716939937510582097494459")
        for j in range(L):
            a = 2 * pi * j / L
            s = c = D(0)
            term = D(1)
            for n in range(90):
                if n % 2:
                    s += term if n % 4 == 1 else -term
                else:
                    c += term if n % 4 == 0 else -term
                term = term * a / (n + 1)
            out.append((s, c))

    def miss(got, want):
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            return abs(float(decimal.Decimal(got) - want))
    return out, miss


_SIN = [(-1.0) ** k / math.factorial(2 * k + 1) for k in range(9)]
_COS = [(-1.0) ** k / math.factorial(2 * k) for k in range(10)]


def twiddle(j, L):
    """Rule 5 on Python floats: (sin, cos) of 2 pi j / L."""
    r = 4 * j
    q, m = r // L, r % L
    swap = 2 * m > L
    mm = L - m if swap else m
    phi = (1.5707963267948966 * float(mm)) / float(L)
    z = phi * phi
    p = _SIN[8]
    for k in range(7, -1, -1):
        p = p * z + _SIN[k]
    s = phi * p
    c = _COS[9]
    for k in range(8, -1, -1):
        c = c * z + _COS[k]
    a, b = (c, s) if swap else (s, c)
    return ((a, b), (b, -a), (-a, -b), (-b, a))[q]


def candidates(events):
    """Rule 3's candidates of one sequence: [(t0, t1, side)], the left foot's in time order, then the right foot's."""
    out = []
    for bit, side in ((1, 1.0), (2, -1.0)):
        last = None
        for t, e in enumerate(events):
            if int(e) & bit:
                if last is not None:
                    out.append((last, t, side))
                last = t
    return out


def stride(x, t0, t1, odd, exclude=None, n_harmonics=20, derivative=2, min_stride=8, max_stride=60):
    """Rules 3 to 7 of one candidate of one channel: None where it is not used, else dict(H, HR, iHR, a, C, S, y)."""
    L = t1 - t0
    if not min_stride <= L <= max_stride:
        return None
    for t in range(t0, t1 + 1):
        if not math.isfinite(x[t]) or (exclude is not None and int(exclude[t]) != 0):
            return None
    y = []
    for i in range(L):
        slope = float(i) / float(L)
        trend = (x[t1] - x[t0]) * slope
        y.append((x[t0 + i] - x[t0]) - trend)
    tw = [twiddle(j, L) for j in range(L)]
    H = min(n_harmonics, (L - 1) // 2)
    H -= H % 2
    a, Cs, Ss = [], [], []
    for k in range(1, H + 1):
        C = S = 0.0
        j = 0
        for i in range(L):
            pc = y[i] * tw[j][1]
            ps = y[i] * tw[j][0]
            C = C + pc
            S = S + ps
            j += k
            if j >= L:
                j -= L
        cc = C * C
        ss = S * S
        a.append(math.sqrt(cc + ss) * (2.0 / float(L)))
        Cs.append(C)
        Ss.append(S)
    E = O = PE = PO = 0.0
    for k in range(1, H + 1):
        g = 1.0 if derivative == 0 else float(k) if derivative == 1 else float(k * k)
        w = a[k - 1] * g
        if k % 2:
            O = O + w
            PO = PO + w * w
        else:
            E = E + w
            PE = PE + w * w
    if not (E > 0.0 and math.isfinite(E) and O > 0.0 and math.isfinite(O)):
        return None
    HR = O / E if odd else E / O
    iHR = (100.0 * (PO if odd else PE)) / (PE + PO)
    return dict(H=H, HR=HR, iHR=iHR, a=a, C=Cs, S=Ss, y=y, L=L)


def _moments(values):
    nan = float("nan")
    if not values:
        return nan, nan
    S = 0.0
    for v in values:
        S = S + v
    m = S / len(values)
    Q = 0.0
    for v in values:
        d = v - m
        Q = Q + d * d
    return m, math.sqrt(Q / len(values))


def yardstick(x, events, odd, exclude=None, fps=FPS, n_harmonics=20, derivative=2, min_stride=8, max_stride=60, max_strides=128):
    """(strides: max_strides rows of 6, spectrum: n_harmonics rows of 2, row: 12 floats) of ONE signal of ONE sequence by rules 3 to 8."""
    nan = float("nan")
    x = [float(v) for v in x]
    cand = candidates(events)
    rows = [[nan] * 6 for _ in range(max_strides)]
    used = []
    for c, (t0, t1, side) in enumerate(cand):
        s = stride(x, t0, t1, odd, exclude, n_harmonics, derivative, min_stride, max_stride)
        if s is not None:
            used.append((side, s))
        if c < max_strides:
            rows[c] = [float(t0), float(t1), side, float(s["H"]) if s else 0.0, s["HR"] if s else nan, s["iHR"] if s else nan]
    row = [nan] * 12
    row[0], row[1] = float(len(cand)), float(len(used))
    row[2], row[3] = _moments([s["HR"] for _, s in used])
    row[4] = _moments([s["HR"] for side, s in used if side > 0])[0]
    row[5] = _moments([s["HR"] for side, s in used if side < 0])[0]
    row[6] = (100.0 * abs(row[4] - row[5])) / (0.5 * (row[4] + row[5]))
    row[7], row[8] = _moments([s["iHR"] for _, s in used])
    row[9] = _moments([float(s["L"]) for _, s in used])[0]
    row[10] = fps / row[9]
    row[11] = float(min(s["H"] for _, s in used)) if used else nan
    spectrum = [list(_moments([s["a"][k - 1] for _, s in used if s["H"] >= k])) for k in range(1, n_harmonics + 1)]
    return rows, spectrum, row


def yardstick_call(per_frame, events, lengths, exclude=None, **rule):
    """The yardstick over a call's signals (n,4): (strides (n_seq,4,max_strides,6), spectrum (n_seq,4,n_harmonics,2), per_sequence (n_seq,4,12))."""
    strides, spectra, rows, a = [], [], [], 0
    for T in lengths:
        made = [yardstick(per_frame[a:a + T, ch], events[a:a + T], ch < 3, None if exclude is None else exclude[a:a + T], **rule) for ch in range(4)]
        strides.append([m[0] for m in made])
        spectra.append([m[1] for m in made])
        rows.append([m[2] for m in made])
        a += T
    return np.array(strides), np.array(spectra), np.array(rows)


def same_bits(a, b):
    return gc.same_bits(a, b)


def periodic_events(T, P, first_left, first_right):
    """Heel strikes by hand: the left foot's every P frames from first_left, the right foot's from first_right."""
    ev = np.zeros(T, np.int32)
    ev[first_left::P] |= 1
    ev[first_right::P] |= 2
    return ev


def closed_signal(T, B, phi, psi=0.9, A=0.3):
    """sep of the walker in float64, without the rounding of its float32 joints."""
    p = 2.0 * np.pi * (np.arange(T, dtype=np.float64) + phi) / CLOSED_P
    return 2.0 * A * (np.sin(p) + B * np.sin(2.0 * p + psi))


def measure_closed(through_joints):
    """What the yardstick misses the closed form by on sep over CLOSED_CASES x CLOSED_PHASES (x CLOSED_YAWS through the walker's joints), relative:
    {'hr', 'ihr'}.  through_joints: on the walker's float32 joints, else on closed_signal."""
    worst = dict(hr=0.0, ihr=0.0)
    for B, d in CLOSED_CASES:
        for theta in (CLOSED_YAWS if through_joints else CLOSED_YAWS[:1]):
            for phi in CLOSED_PHASES:
                x = rc.signals_of(*rc.walker(400, float(CLOSED_P), B, theta, phi))[:, 0] if through_joints else closed_signal(400, B, phi)
                rows, _, row = yardstick(x, periodic_events(400, CLOSED_P, 5, 17), True, **dict(RULE, derivative=d))
                assert row[1] == row[0] == 31.0
                for r in rows[:31]:
                    worst["hr"] = max(worst["hr"], abs(r[4] - closed_hr(B, d)) / closed_hr(B, d))
                    worst["ihr"] = max(worst["ihr"], abs(r[5] - closed_ihr(B, d)) / closed_ihr(B, d))
    return worst


def write_case(path, joints, table, trans, signals, events, exclude, rule, host):
    """The file tests/helpers/gait_harmonics_check.cpp reads: ONE sequence, its inputs and the statement's result `host` with sigma = 0.  joints None:
    a case on given signals (T,4)."""
    T = signals.shape[0] if joints is None else joints.shape[0]
    J = 0 if joints is None else joints.shape[1]
    with open(path, "wb") as f:
        f.write(np.array([T, J, trans is not None, exclude is not None, rule["n_harmonics"], rule["derivative"], rule["min_stride"], rule["max_stride"],
                          rule["max_strides"]], "<i4").tobytes())
        f.write(np.asarray(table, "<i4").tobytes())
        f.write(np.array([rule["fps"]], "<f8").tobytes())
        f.write(np.ascontiguousarray(signals, "<f8").tobytes() if joints is None else np.ascontiguousarray(joints, "<f4").tobytes())
        f.write(np.ascontiguousarray(events, "<i4").tobytes())
        if trans is not None:
            f.write(np.ascontiguousarray(trans, "<f8").tobytes())
        if exclude is not None:
            f.write(np.ascontiguousarray(exclude, "<i4").tobytes())
        if joints is not None:
            f.write(np.ascontiguousarray(host["per_frame"], "<f8").tobytes())
        for key in ("strides", "spectrum", "per_sequence"):
            f.write(np.ascontiguousarray(host[key][0], "<f8").tobytes())
    return path


def hand_events_call():
    """The hook's call of the device tests on hand-placed events: (signals (n,4), events (n,), exclude (n,), lengths, names).  Strides of 6, 7, 63, 64,
    65 and 255 frames and one of 256; strikes at frames 63, 64 and 65 and at a sequence's last frame; a frame where both feet strike; a NaN at a
    stride's t1; an excluded frame inside a stride; a stride of 5; a sequence of one frame and one without strikes."""
    rng = np.random.default_rng(1971)

    def signal(T):
        t = np.arange(T, dtype=np.float64)[:, None]
        return np.sin(t * np.array([0.21, 0.17, 0.13, 0.29])) + 0.3 * np.cos(t * np.array([0.42, 0.37, 0.31, 0.58])) + 0.01 * t + 0.05 * rng.standard_normal((T, 4))
    parts, names = [], []

    def add(name, T, left=(), right=(), nan=(), ex=()):
        x, ev, e = signal(T), np.zeros(T, np.int32), np.zeros(T, np.int32)
        ev[list(left)] |= 1
        ev[list(right)] |= 2
        for t, ch in nan:
            x[t, ch] = np.nan
        e[list(ex)] = 2
        parts.append((x, ev, e))
        names.append(name)
    # left: 0 -6- 6 -7- 13 -50- 63 -1- 64 -1- 65 -63- 128 -64- 192 -65- 257 -255- 512 -256- 768 -31- 799 (the last frame); right: 5 -5- 10 -54- 64 -200- 264
    add("edges800", 800, left=(0, 6, 13, 63, 64, 65, 128, 192, 257, 512, 768, 799), right=(5, 10, 64, 264))
    add("one", 1, left=(0,))
    add("no_strikes", 70)
    add("nan_at_t1", 130, left=(3, 30, 57, 84, 111), right=(16, 43, 70, 97, 124), nan=((57, 0), (70, 3)))
    add("excluded", 130, left=(3, 30, 57, 84, 111), right=(16, 43, 70, 97, 124), ex=(40,))
    add("both_feet", 65, left=(0, 20, 40, 64), right=(20, 40))
    add("seven", 7, left=(0, 6))
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), [p[0].shape[0] for p in parts],
            names)


def device_call(J=25, table=gc.KINECTV2):
    """The seven sequences of the device tests in one call: (joints, trans, lengths, names, hand): lengths 1, 7, 8, 64, 65, 130 and 400 -- a single
    frame, the shortest that holds a stride (of 6 frames) and the next, a standing body of exactly one word of the masks, 65 frames with one
    degenerate frame, and walks of 130 and 400 frames at other yaws and periods.  hand (n,) int32: strikes put by hand at both ends of the
    sequences of 7 and 8 frames and at the last frame of the one of 65, to be or-ed into the events found."""
    parts = (("walk130", dict(T=130, P=21.7, B=0.3, theta=0.7, phi=3.0)), ("one", dict(T=1, theta=0.2)), ("seven", dict(T=7, P=6.0, B=0.3, theta=0.3)),
             ("eight", dict(T=8, P=7.0, B=0.3, theta=0.4)), ("standing64", dict(T=64, still=True)),
             ("degenerate65", dict(T=65, P=19.3, B=0.2, theta=-1.1, phi=2.2, degenerate=(30,))), ("walk400_back", dict(T=400, P=27.3, B=0.3, theta=np.pi - 0.4, phi=1.9)))
    made = [rc.walker(J=J, table=table, **kw) for _, kw in parts]
    lengths = [kw["T"] for _, kw in parts]
    hand = np.zeros(sum(lengths), np.int32)
    hand[[131, 137]] |= 1                                      # seven: frames 0 and 6
    hand[[138, 145]] |= 2                                      # eight: frames 0 and 7
    hand[[146, 209]] |= 1                                      # standing64: its first and last frame, a stride of 63 whose signal is constant
    hand[[210 + 40, 210 + 64]] |= 2                            # degenerate65: a stride that ends at the last frame
    return np.concatenate([m[0] for m in made]), np.concatenate([m[1] for m in made]), lengths, [name for name, _ in parts], hand
