"""A turning walker and the bars of the turns call, shared by the host and the GPU tests.  Nothing here calls the code under test.
u = 2^-53.

THE TURNING WALKER.  gait_checks.walker's skeleton with a yaw theta(t) per frame: theta0, minus for every turn (start, length, angle) the angle
times smoothstep((t - start) / length) -- an angle > 0 is a turn to the subject's LEFT, which lowers the walker's theta -- plus an optional pelvic
wobble a sin(2 pi t / P + psi).  Inside a turn the gait slows and shortens smoothly: with b(t) = sin^2(pi (t - start) / length) the gait's frequency
is 1 / P + (1 / turn_P - 1 / P) b and the swing A (1 - (1 - turn_A) b), so the strides inside a turn last up to turn_P = 30 frames and those outside
it P frames: they differ analytically.  The gait's phase is the running sum of the frequency.

EXPECTED TURNS.  core_window gives the frames at which the smoothstep alone turns faster than a given rate: with the edge rate plus the wobble's
largest rate a 2 pi / P fps for it, every such frame lies in the found turn, however the wobble falls.  expected_turns gives, per turn, the window [start, start + length] cut to the sequence, the direction from the sign of
(f(t) - f(t - 1)) . n of the analytic axes in the middle of the window (+1: towards the subject's left), and the angle in degrees that lies inside
the sequence.

THE MARGIN.  decision_margin is the smallest amount by which any comparison of rule 4 is decided on given [step, rate] of ONE sequence:
| |rate| - edge | over every frame with a finite rate, and over every run of either sign |max |rate| - peak| and | |sum of steps| - min_angle |.  The
run lengths are integers and decided alike on both sides.  Every input of a device test has a margin >= MIN_MARGIN = 1e-6 degrees a second (the
angle's in degrees): the two sides' rates differ by 1e-12 at most (the bars below), so they decide every comparison alike and THE PHASES, THE TURN
TABLE'S INTEGER COLUMNS AND EVERY COUNT ARE EQUAL.  It is a condition on the inputs, asserted on the CPU.

THE BARS with sigma > 0 (with sigma = 0 both sides run the same operations in the same order: every bit is equal).
  rate       b = 2 gauss_bar(raw rate of the sequence): each side's Gaussian is within (2 r + 8) u max|x| of the exact one
             (tests/helpers/track_checks.py), and both sides err.  The step is not smoothed: equal bits.
  peak       a maximum of |rate| over the same frames moves by no more than the largest change of an entry: b.
  mean peak  over n turns: every term within b, each side's sum with n - 1 roundings and one quotient: b + 2 (n + 1) u max peak.
  all else   sums of raw steps, integers, and the straight columns, which come from inputs both sides share: EQUAL BITS."""
import numpy as np

from . import gait_checks as gc
from . import track_checks as tk

U = 2.0 ** -53
MIN_MARGIN = 1e-6
DEFAULT_RULE = dict(fps=20.0, edge_rate=5.0, peak_rate=15.0, min_angle=45.0, min_frames=10, max_frames=200)
PEAK_COLUMN, MEAN_PEAK_COLUMN = 5, 9
same_bits = gc.same_bits


def smoothstep(u):
    u = np.clip(u, 0.0, 1.0)
    return u * u * (3.0 - 2.0 * u)


def yaw(T, turns=(), theta0=0.0, wobble=None, P=21.7):
    """theta(t) in radians.  turns: (start, length, degrees to the left); wobble: (amplitude in degrees, psi) at the period P."""
    t = np.arange(T, dtype=np.float64)
    theta = np.full(T, float(theta0))
    for start, length, angle in turns:
        theta -= np.deg2rad(angle) * smoothstep((t - start) / length)
    if wobble is not None:
        theta += np.deg2rad(wobble[0]) * np.sin(2.0 * np.pi * t / P + wobble[1])
    return theta


def turning_walker(T, turns=(), theta0=0.0, wobble=None, A=0.3, P=21.7, phi=-3.02, lag=2.64, J=25, table=gc.KINECTV2, degenerate=(), turn_P=30.0, turn_A=0.5):
    """(joints (T,J,3) float32, trans (T,3) float64) of the walker above."""
    t = np.arange(T, dtype=np.float64)
    theta = yaw(T, turns, theta0, wobble, P)
    bump = np.zeros(T)
    for start, length, _ in turns:
        u = (t - start) / length
        bump = np.maximum(bump, np.where((u > 0) & (u < 1), np.sin(np.pi * u) ** 2, 0.0))
    freq = 1.0 / P + (1.0 / turn_P - 1.0 / P) * bump
    cycles = np.concatenate([[0.0], np.cumsum(freq)[:-1]])      # the gait's phase in cycles: t / P on a straight walk
    amp = A * (1.0 - (1.0 - turn_A) * bump)
    swing = amp * np.sin(2.0 * np.pi * (cycles + phi / P))
    trail = amp * np.sin(2.0 * np.pi * (cycles + (phi - lag) / P))
    c, s = np.cos(theta), np.sin(theta)
    zero = np.zeros(T)
    fwd, left = np.stack([-s, zero, -c], axis=1), np.stack([c, zero, -s], axis=1)
    up = np.broadcast_to(np.array([0.0, -1.0, 0.0]), (T, 3))
    body = np.zeros((T, J, 3))
    body[:, :, 0] = 0.01 * np.arange(J)[None, :]
    body[:, :, 1] = 0.02 * ((np.arange(J) % 5) - 2)[None, :]
    body[:, :, 2] = 0.03 * ((np.arange(J) % 7) - 3)[None, :]
    for k, (a, b, h) in enumerate(((zero, 0.0, 0.0), (zero, 0.0, 0.5), (zero, 0.1, 0.0), (zero, -0.1, 0.0), (swing, 0.1, -0.8), (-swing, -0.1, -0.8),
                                   (trail, 0.1, -0.85), (-trail, -0.1, -0.85))):
        body[:, table[k], 0], body[:, table[k], 1], body[:, table[k], 2] = a, b, h
    for f in degenerate:
        body[f, table[2]] = body[f, table[3]]
    joints = body[:, :, 0:1] * fwd[:, None, :] + body[:, :, 1:2] * left[:, None, :] + body[:, :, 2:3] * up[:, None, :]
    speed = 4.0 * amp * freq
    trans = np.array([0.3, 0.1, 6.0]) + np.concatenate([np.zeros((1, 3)), np.cumsum(speed[:-1, None] * fwd[:-1], axis=0)])
    return joints.astype(np.float32), trans


def expected_turns(T, turns, theta0=0.0):
    """[(first, last, direction, degrees)] of the smoothstep windows, cut to [0, T)."""
    out = []
    for start, length, angle in turns:
        first, last = max(int(start), 0), min(int(start + length), T - 1)
        mid = (first + last) // 2
        th = yaw(mid + 1, [(start, length, angle)], theta0)
        f0, f1 = (np.array([-np.sin(v), 0.0, -np.cos(v)]) for v in th[mid - 1:mid + 1])
        n = np.array([np.cos(th[mid]), 0.0, -np.sin(th[mid])])
        direction = 1 if float(np.dot(f1 - f0, n)) > 0 else -1
        inside = abs(angle) * float(smoothstep((last - start) / length) - smoothstep((first - start) / length))
        out.append((first, last, direction, inside))
    return out


def core_window(turn, fps, floor):
    """(first, last) of the frames of a turn (start, length, degrees) at which the smoothstep alone turns faster than `floor` degrees a second, one frame
    taken off either end for the sampling: the step of frame t spans t - 1 .. t, so its rate is the derivative 6 u (1 - u) angle / length at some u in it."""
    start, length, angle = turn
    t = np.arange(int(np.floor(start)), int(np.ceil(start + length)) + 1, dtype=np.float64)
    lo, hi = np.clip((t - 1 - start) / length, 0.0, 1.0), np.clip((t - start) / length, 0.0, 1.0)
    slowest = abs(angle) / length * fps * np.minimum(6 * lo * (1 - lo), 6 * hi * (1 - hi))       # the derivative is concave: its minimum over the step is at an end
    fast = t[slowest > floor]
    return int(fast[0]) + 1, int(fast[-1]) - 1


def runs_of(mask):
    edges = np.flatnonzero(np.diff(np.concatenate([[0], np.asarray(mask, np.int8), [0]])))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def decision_margin(rows, edge_rate, peak_rate, min_angle):
    """The smallest amount by which a comparison of rule 4 is decided on rows (T,2) = [step, rate] of ONE sequence; inf where there is none."""
    rows = np.asarray(rows, np.float64)
    step, rate = rows[:, 0], rows[:, 1]
    best = np.inf
    fin = np.isfinite(rate)
    if fin.any():
        best = float(np.abs(np.abs(rate[fin]) - edge_rate).min())
    with np.errstate(invalid="ignore"):
        for mask in (rate > edge_rate, rate < -edge_rate):
            for a, b in runs_of(mask):
                best = min(best, abs(float(np.abs(rate[a:b]).max()) - peak_rate))
                angle = abs(float(np.cumsum(step[a:b])[-1]))
                if np.isfinite(angle):
                    best = min(best, abs(angle - min_angle))
    return best


def assert_margin(per_frame, lengths, edge_rate=5.0, peak_rate=15.0, min_angle=45.0):
    """The condition on the inputs: per_frame = the statement's [step, rate] rows of a call."""
    a, worst = 0, np.inf
    for T in lengths:
        worst = min(worst, decision_margin(per_frame[a:a + T], edge_rate, peak_rate, min_angle))
        a += T
    assert worst >= MIN_MARGIN, f"the input decides a comparison by {worst:.3g} < {MIN_MARGIN:g}: not a fair input"
    return worst


def rate_bar(raw_rate, sigma):
    """b for ONE sequence: raw_rate (T,) = the column that is filtered (the statement's rate with sigma = 0, the device's in every bit); NaN left out."""
    raw = np.asarray(raw_rate, np.float64)
    fin = np.isfinite(raw)
    return 2.0 * tk.gauss_bar(raw[fin], sigma) if sigma > 0 and fin.any() else 0.0


def compare(got, host, raw, lengths, sigma):
    """A result (numpy arrays) against the statement's; raw (n,): the statement's rate with sigma = 0 on the same call (None with sigma = 0).  Phases,
    the table's integer columns, the counts and everything the smoothing does not reach equal in every bit; rate, peak and mean peak within their
    bars.  Returns the worst ratio to a bar (0.0 with sigma = 0)."""
    assert np.array_equal(got["phase"], host["phase"]), "the phases differ"
    worst, a = 0.0, 0
    for q, T in enumerate(lengths):
        b = rate_bar(raw[a:a + T], sigma) if raw is not None else 0.0
        gf, hf = got["per_frame"][a:a + T], host["per_frame"][a:a + T]
        gt, ht, gs, hs = got["turns"][q], host["turns"][q], got["per_sequence"][q], host["per_sequence"][q]
        assert same_bits(gf[:, 0], hf[:, 0]), f"sequence {q}: a yaw step differs in some bit"
        assert np.array_equal(np.isnan(gf), np.isnan(hf)) and np.array_equal(np.isnan(gt), np.isnan(ht)) and np.array_equal(np.isnan(gs), np.isnan(hs)), f"sequence {q}: a NaN on one side alone"
        n = hs[0]
        b_mean = b + 2 * (n + 1) * U * (np.nanmax(ht[:, PEAK_COLUMN]) if np.isfinite(ht[:, PEAK_COLUMN]).any() else 0.0) if b > 0 else 0.0
        if b == 0:
            assert same_bits(gf[:, 1], hf[:, 1]), f"sequence {q}: a yaw rate differs in some bit"
        elif np.isfinite(hf[:, 1]).any():
            worst = max(worst, float(np.nanmax(np.abs(gf[:, 1] - hf[:, 1]))) / b)
        for c in range(7):
            if c == PEAK_COLUMN and b > 0:
                if np.isfinite(ht[:, c]).any():
                    worst = max(worst, float(np.nanmax(np.abs(gt[:, c] - ht[:, c]))) / b)
            else:
                assert same_bits(gt[:, c], ht[:, c]), f"sequence {q}: column {c} of the turn table differs: {gt[:, c]} against {ht[:, c]}"
        for c in range(24):
            if c == MEAN_PEAK_COLUMN and b > 0:
                if np.isfinite(hs[c]):
                    worst = max(worst, abs(gs[c] - hs[c]) / b_mean)
            else:
                assert same_bits(gs[c], hs[c]), f"sequence {q}: per_sequence column {c} is {gs[c]!r}, not {hs[c]!r}"
        a += T
    return worst


# ---- the hand-made case: 25 frames, rates in whole degrees a second, steps in whole degrees; edge 5, peak 15, min_angle 45, 3 .. 5 frames a turn
#        frame   0   1   2  3   4   5   6  7   8   9 10  11  12  13   14   15   16   17 18  19  20  21  22  23  24
HAND_RATE = [20, 20, 20, 2, 10, 10, 10, 0, 20, 20, 0, 20, 20, 20, -20, -20, -20, -20, 0, 20, 20, 20, 20, 20, 20]
HAND_STEP = [30, 30, 30, 0, 30, 30, 30, 0, 30, 30, 0, 2, 2, 2, -20, -20, -20, -20, 0, 10, 10, 10, 10, 10, 10]
HAND_NAN = 7                                                   # the rate of this frame becomes NaN: unknown, and a straight bout ends on either side
# runs: [0, 3) left, peak 20, 90 degrees, 3 frames: A TURN, on the first frame; [4, 7) peak 10 < 15: none; [8, 10) 2 frames < 3: none; [11, 14)
# 6 degrees < 45: none; [14, 18) right, peak 20, -80 degrees, 4 frames: A TURN; [19, 25) 6 frames > 5: none, and it ends on the last frame
HAND_RULE = dict(fps=20.0, edge_rate=5.0, peak_rate=15.0, min_angle=45.0, min_frames=3, max_frames=5)
HAND_STRIKES = {1: 1, 4: 2, 6: 1, 9: 2, 10: 8, 11: 1, 13: 2, 16: 1, 19: 2, 21: 1, 22: 8, 23: 2}      # frame: bits (1 left strike, 2 right strike, 8 right toe-off)
HAND_PHASE = [1, 1, 1, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0]
HAND_TURNS = [[0, 2, 1, 90, 3 / 20.0, 20, 1], [14, 17, -1, -80, 4 / 20.0, 20, 1]]        # one heel strike inside each: frames 1 and 16
# 2 turns, 1 left, 1 right, 7 turn frames, 1 unknown, 3 straight bouts ([3, 7), [8, 14), [18, 25)), 17 straight frames; the means over the turns
HAND_COUNTS = [2, 1, 1, 7, 1, 3, 17, (3 / 20.0 + 4 / 20.0) / 2, 85, 20, 1]
# straight steps, of the pairs (1,4) (4,6) (6,9) (9,11) (11,13) (13,16) (16,19) (19,21) (21,23) those without a busy frame (0 1 2 7 14 15 16 17) in
# [t1, t2]: (4,6) (9,11) (11,13) (19,21) (21,23): 5 steps of 2 frames, lengths 2 t at a left strike and -2 t at a right one: 12 22 -26 42 -46.
# straight strides: none of the left foot's (1,6) (6,11) (11,16) (16,21); the right foot's (9,13) and (19,23): 4 frames each; their toe-offs at 10
# and 22: stance 25 and 75 per cent.
HAND_STRAIGHT = {11: 5, 12: 0.1, 13: 0.0, 14: 600.0, 15: 0.2, 16: 0.0, 17: 0.0, 18: 0.8, 20: 0.25, 21: 0.0, 22: 50.0, 23: 8.0}      # column: value


def hand_case():
    """(rates (25,2), events (25,), gait_rows (25,7)) of the hand-made case; the gait rows hold hL = frame, hR = -frame, wd = 0.25."""
    rates = np.stack([np.asarray(HAND_STEP, np.float64), np.asarray(HAND_RATE, np.float64)], axis=1)
    rates[HAND_NAN, 1] = np.nan
    events = np.zeros(25, np.int32)
    for frame, bits in HAND_STRIKES.items():
        events[frame] = bits
    rows = np.full((25, 7), np.nan)
    t = np.arange(25, dtype=np.float64)
    rows[:, 0], rows[:, 1], rows[:, 4] = t, -t, 0.25
    return rates, events, rows
