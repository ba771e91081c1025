"""A planted-foot walker and the bars of the contacts call, shared by the host and the GPU tests.  Nothing here calls the code under
test.  u = 2^-53.

THE PLANTED-FOOT WALKER.  gait_checks' skeleton (pelvis the origin, spine-shoulder 0.5 m up, the hips 0.1 m to either side, the ankles 0.8 m down)
with feet that STAND STILL IN THE WORLD while they are on the ground.  Cycle P frames, stance share beta, speed v metres a frame.  With
u = ((t + phi) / P) mod 1 the left ankle lies, ahead of the pelvis along the facing,
    v beta P / 2 - v P u                                          for u < beta: the pelvis moves on at v, the foot does not;
    -v beta P / 2 + v beta P (w - sin(2 pi w) / (2 pi))           with w = (u - beta) / (1 - beta) otherwise: a swing that leaves and lands at rest.
In swing the ankle lifts by 0.04 (1 - cos 2 pi w) m; it sits 0.09 m to its side.  The foot joints are a fixed offset from their ankles; the right
foot does the same P / 2 later; everything is turned by a yaw.  Both feet are on the ground for (beta - 1/2) P frames twice a cycle: the
DOUBLE-SUPPORT TIME; a double support begins with a heel strike (u = 0) every P / 2 frames: the STEP TIME.  The vector from one ankle to the other
moves at 2 v over a cycle in the mean: the forward part alone covers 2 v beta P twice, the lift and nothing else comes on top.

THE MARGIN.  decision_margin is the smallest |s - thr| over the finite intervals of ONE sequence.  Every input of a device test has a margin >=
MIN_MARGIN = 1e-9 m/s on the statement's (smoothed) s and its threshold: the two sides' s and thr differ by far less (the bars below), so they decide
every comparison alike and THE PHASES, THE ATTRIBUTIONS AND EVERY COUNT ARE EQUAL.  It is a condition on the inputs, asserted on the CPU.

THE BARS with sigma > 0 (with sigma = 0 both sides run the same operations in the same order: every bit is equal).  The quotient rule used below:
where N and D > 0 are known to e_N and e_D, and |N| <= c D, N / D is known to q(c, D, e_N, e_D) = (c e_D + e_N) / (D - e_D).
  d_c        b_c = 2 gauss_bar(raw column c): each side's Gaussian is within (2 r + 8) u max|x| of the exact one (track_checks.py); both sides err.
  s          the Euclidean norm moves by no more than the sum of the changes of its components; a component d_c(k+1) - d_c(k) is known to 2 b_c and
             each side rounds it once (u |.| <= 2 u max|d_c|); squares, two additions, root and the product with fps are within 4 u relative on
             each side:  b_s = fps sum_c (2 b_c + 4 u max|d_c|) + 8 u max s.
  least s    a minimum over the same intervals: b_s.
  S / n      every term within b_s; each side's tree and chain of blocks are within (6 + blocks) u S, and one quotient: b_mean = b_s + 2 (8 + blocks)
             u mean.  thr = fraction mean: b_thr = fraction b_mean + 2 u thr; with speed > 0 the threshold is the argument: b_thr = 0.
  an edge    (k +- 1/2) + N / D with D = the statement's difference of the two speeds either side of the crossing (known to 2 b_s) and 0 <= N <= D
             the distance of one of them from thr (known to b_s + b_thr); three roundings of the quotient's parts and one of the sum on each side:
             b_e = q(1, D, b_s + b_thr, 2 b_s) + 2 u (3 + T).  B_e is the largest b_e of the sequence's closed runs.
  a time     a difference of two edges over fps: b_t = 2 B_e / fps + 4 u |time|, for the run table's duration and every term of the row's means.
  a mean     over n terms: b_t + 2 (n + 1) u max|term|.   an SD (gait_checks.py's argument): b_t + b_mean' + 2 (n + 3) u SD.
  asymmetry  100 |L - R| / (0.5 (L + R)): N = 100 |L - R| known to 100 (b_L + b_R), D known to 0.5 (b_L + b_R), N <= 200 D, five roundings a side.
  shares     100 N / stride length in frames with N <= 2 length: N known to 4 B_e, the length to 2 B_e; the mean over n strides as above.
  CV         100 SD / mean: the quotient rule with the two bars above.
  counts, leads, heel-strike frames, phases: EQUAL."""
import numpy as np

from . import gait_checks as gc
from . import track_checks as tk

U = 2.0 ** -53
MIN_MARGIN = 1e-9
FPS = 20.0
same_bits = gc.same_bits
WALKERS = ((21.7, 0.62, 1.2), (27.3, 0.66, 0.6), (33.1, 0.70, 0.4), (19.3, 0.60, 1.5))      # (P, beta, v fps)
YAWS = (0.0, np.deg2rad(40.0), np.pi)
FOOT_OFFSET = (0.12, 0.0, -0.05)                               # the foot joint from its ankle: forward, left, up


def ankle_track(t, P, beta, v, phi):
    """(ahead of the pelvis, lift) of an ankle at the times t."""
    u = np.mod((t + phi) / P, 1.0)
    w = np.clip((u - beta) / (1.0 - beta), 0.0, 1.0)
    ahead = np.where(u < beta, v * beta * P / 2 - v * P * u, -v * beta * P / 2 + v * beta * P * (w - np.sin(2 * np.pi * w) / (2 * np.pi)))
    return ahead, np.where(u < beta, 0.0, 0.04 * (1.0 - np.cos(2 * np.pi * w)))


def planted_walker(T, P=21.7, beta=0.62, speed=1.2, phi=0.0, theta=0.0, fps=FPS, J=25, table=gc.KINECTV2, nan_frames=(), still=False):
    """joints (T,J,3) float32 of the walker above; speed = v fps in metres a second.  nan_frames: frames whose left ankle is NaN.  still: both feet
    stand (a standing body: the ankles do not move at all)."""
    t = np.arange(T, dtype=np.float64)
    v = speed / fps
    c, s = np.cos(theta), np.sin(theta)
    fwd, left, up = np.array([-s, 0.0, -c]), np.array([c, 0.0, -s]), np.array([0.0, -1.0, 0.0])
    body = np.zeros((T, J, 3))
    body[:, :, 0] = 0.01 * np.arange(J)[None, :]
    body[:, :, 1] = 0.02 * ((np.arange(J) % 5) - 2)[None, :]
    body[:, :, 2] = 0.03 * ((np.arange(J) % 7) - 3)[None, :]
    zero = np.zeros(T)
    la, ll = ankle_track(t, P, beta, v, phi)
    ra, rl = ankle_track(t - P / 2, P, beta, v, phi)
    if still:
        la, ll, ra, rl = zero + 0.1, zero, zero - 0.1, zero
    rows = ((zero, 0.0, zero), (zero, 0.0, zero + 0.5), (zero, 0.1, zero), (zero, -0.1, zero), (la, 0.09, ll - 0.8), (ra, -0.09, rl - 0.8),
            (la + FOOT_OFFSET[0], 0.09 + FOOT_OFFSET[1], ll - 0.8 + FOOT_OFFSET[2]), (ra + FOOT_OFFSET[0], -0.09 + FOOT_OFFSET[1], rl - 0.8 + FOOT_OFFSET[2]))
    for k, (a, b, h) in enumerate(rows):
        body[:, table[k], 0], body[:, table[k], 1], body[:, table[k], 2] = a, b, h
    joints = body[:, :, 0:1] * fwd + body[:, :, 1:2] * left + body[:, :, 2:3] * up
    for f in nan_frames:
        joints[f, table[4]] = np.nan
    return joints.astype(np.float32)


def tree_sum(values):
    """Rule 3's sum written as loops, independent of the statement's reshapes: (S, count of finite entries)."""
    x = [float(v) for v in values]
    total, count = 0.0, 0
    for b in range(0, len(x), 64):
        block = [v if np.isfinite(v) else 0.0 for v in x[b:b + 64]]
        count += sum(1 for v in x[b:b + 64] if np.isfinite(v))
        block += [0.0] * (64 - len(block))
        while len(block) > 1:
            block = [block[i] + block[i + 1] for i in range(0, len(block), 2)]
        total = total + block[0]
    return total, count


def decision_margin(s, thr):
    """The smallest |s - thr| over the finite entries of s (the intervals of ONE sequence, its last row left out); inf where there is none."""
    s = np.asarray(s, np.float64)
    s = s[np.isfinite(s)]
    return float(np.abs(s - thr).min()) if s.size and np.isfinite(thr) else np.inf


def assert_margin(host, lengths):
    """The condition on the inputs: host = the statement's result of a call (its per_frame or, of the hook, 'speeds')."""
    s = host["per_frame"][:, 0] if "per_frame" in host else host["speeds"]
    a, worst = 0, np.inf
    for q, T in enumerate(lengths):
        worst = min(worst, decision_margin(s[a:a + T - 1], host["per_sequence"][q, 0]))
        a += T
    assert worst >= MIN_MARGIN, f"the input decides a comparison by {worst:.3g} < {MIN_MARGIN:g} m/s: not a fair input (change phi)"
    return worst


def quotient_bar(c, D, e_N, e_D):
    return (c * e_D + e_N) / (D - e_D)


def sequence_bars(host_frames, host_runs, host_row, raw, sigma, fps, fraction, speed):
    """(bars of the 4 per-frame columns, of the 6 run-table columns, of the 20 per-sequence columns) of ONE sequence from the statement's own result;
    raw (T,3): the unsmoothed vectors.  All zeros with sigma = 0."""
    frame, run, seq = np.zeros(4), np.zeros(6), np.zeros(20)
    if not sigma > 0:
        return frame, run, seq
    T = host_frames.shape[0]
    fin = np.isfinite(raw).all(axis=1)
    b_d = np.array([2.0 * tk.gauss_bar(raw[fin, c], sigma) if fin.any() else 0.0 for c in range(3)])
    big_d = np.array([np.abs(raw[fin, c]).max() if fin.any() else 0.0 for c in range(3)])
    s = host_frames[:T - 1, 0]
    big_s = np.nanmax(s) if np.isfinite(s).any() else 0.0
    b_s = fps * float(np.sum(2 * b_d + 4 * U * big_d)) + 8 * U * big_s
    frame[0], frame[1:] = b_s, b_d
    blocks = (T + 63) // 64
    thr, mean = host_row[0], host_row[1]
    b_mean = b_s + 2 * (8 + blocks) * U * mean if np.isfinite(mean) else 0.0
    b_thr = 0.0 if speed > 0 else fraction * b_mean + 2 * U * thr
    seq[0], seq[1] = (b_thr if np.isfinite(thr) else 0.0), b_mean
    B_e = 0.0
    for t0, t1 in host_runs[np.isfinite(host_runs[:, 0]), :2]:
        a, b = int(np.ceil(t0 - 0.5)), int(np.floor(t1 - 0.5))          # the run's first and last interval, from its edges
        for D in (s[a - 1] - s[a], s[b + 1] - s[b]):
            B_e = max(B_e, quotient_bar(1.0, D, b_s + b_thr, 2 * b_s) + 2 * U * (3 + T))
    run[0] = run[1] = B_e
    big_t = T / fps

    def time_bar(value=big_t):
        return 2 * B_e / fps + 4 * U * abs(value)
    run[4], run[5] = time_bar(), b_s

    def mean_bar(n, term_bar, big):
        return term_bar + 2 * (n + 1) * U * big
    n = host_row[3] + host_row[4]
    if n > 0:
        seq[6] = mean_bar(n, time_bar(), big_t)
        seq[7] = time_bar() + seq[6] + 2 * (n + 3) * U * host_row[7]
        seq[8] = seq[9] = seq[6]
        L, R = host_row[8], host_row[9]
        if np.isfinite(L) and np.isfinite(R):
            seq[10] = quotient_bar(200.0, 0.5 * (L + R), 100 * (seq[8] + seq[9]), 0.5 * (seq[8] + seq[9])) + 10 * U * host_row[10]
    n = host_row[11]
    if n > 0:
        seq[12] = mean_bar(n, time_bar(), big_t)
        seq[13] = time_bar() + seq[12] + 2 * (n + 3) * U * host_row[13]
        seq[14] = seq[15] = seq[16] = seq[12]
        shortest = 1.0                                         # frames: three runs in a row are at least two intervals apart
        share = 100 * quotient_bar(2.0, shortest, 4 * B_e, 2 * B_e) + 4 * U * 200.0
        seq[17] = seq[18] = mean_bar(n, share, 200.0)
        seq[19] = 100 * quotient_bar(1.0, host_row[12], seq[13], seq[12]) + 6 * U * max(host_row[19], 100.0) if host_row[13] <= host_row[12] else np.inf
    return frame, run, seq


def compare(got, host, raw, lengths, sigma, fps=FPS, fraction=0.25, speed=0.0):
    """A result (numpy arrays) against the statement's; raw (n,3): the statement's vectors with sigma = 0 on the same call (None with sigma = 0).
    Phases, leads, heel-strike frames and counts equal; every value whose bar is 0 equal in every bit (with sigma = 0: all of them); the others within
    their bars.  Returns the worst ratio to a bar (0.0 with sigma = 0)."""
    assert np.array_equal(got["phase"], host["phase"]), "the phases differ"
    worst, a = 0.0, 0
    for q, T in enumerate(lengths):
        gf, hf = (None, None) if "per_frame" not in host else (got["per_frame"][a:a + T], host["per_frame"][a:a + T])
        gr, hr, gs, hs = got["runs"][q], host["runs"][q], got["per_sequence"][q], host["per_sequence"][q]
        frame, run, seq = sequence_bars(hf, hr, hs, None if raw is None else raw[a:a + T], sigma, fps, fraction, speed) if sigma > 0 else (np.zeros(4), np.zeros(6), np.zeros(20))
        pairs = [(f"run table column {c}", gr[:, c], hr[:, c], run[c]) for c in range(6)] + [(f"per_sequence column {c}", gs[c:c + 1], hs[c:c + 1], seq[c]) for c in range(20)]
        if hf is not None:
            pairs += [(f"per_frame column {c}", gf[:, c], hf[:, c], frame[c]) for c in range(4)]
        for what, g, h, bar in pairs:
            assert np.array_equal(np.isnan(g), np.isnan(h)), f"sequence {q}: {what} has a NaN on one side alone"
            if bar == 0:
                assert same_bits(g, h), f"sequence {q}: {what} differs in some bit: {g} against {h}"
            elif np.isfinite(h).any():
                ratio = float(np.nanmax(np.abs(g - h))) / bar
                assert ratio <= 1.0, f"sequence {q}: {what} is off by {ratio:.3g} of its bar {bar:.3g}"
                worst = max(worst, ratio)
        a += T
    return worst


# ---- the hand-made case: 22 frames, 21 intervals, speeds in whole metres a second; thr = speed = 5, reach 1, max_frames 3, fps 20
NAN = float("nan")
#        interval  0  1  2  3    4  5  6  7  8  9 10 11 12 13 14  15 16 17 18 19 20   (frame 21 holds no interval: its entry is not read)
HAND_SPEED = [1, 1, 9, 1, NAN, 9, 3, 7, 1, 1, 1, 1, 9, 1, 3, 11, 9, 9, 1, 9, 9, -77]
HAND_RULE = dict(fps=20.0, fraction=0.25, speed=5.0, reach=1, max_frames=3)
HAND_STRIKES = {6: 1, 13: 1, 15: 2}                            # frame: bits (1 left heel strike, 2 right heel strike)
# runs: [0, 1] at the first interval: OPEN; [3] next to the NaN: OPEN; [6] one interval, closed, the left strike of frame 6 alone in frames 5 .. 8:
# LEFT-LED, from 5.5 + (9 - 5) / (9 - 3) to 6.5 + (5 - 3) / (7 - 3); [8, 11] four intervals > max_frames: closed, unattributed, from 7.5 + (7 - 5) /
# (7 - 1) to 11.5 + (5 - 1) / (9 - 1); [13, 14] with the left strike of frame 13 and the right one of frame 15 in frames 12 .. 16: struck by both,
# from 12.5 + (9 - 5) / (9 - 1) to 14.5 + (5 - 3) / (11 - 3); [18] with no strike in frames 17 .. 20: struck by neither, from 17.5 + 4 / 8 to 18.5 + 4 / 8
HAND_PHASE = [3, 3, 0, 3, 4, 0, 1, 0, 3, 3, 3, 3, 0, 3, 3, 0, 0, 0, 3, 0, 0, 4]
HAND_RUNS = [[NAN, NAN, 0, NAN, NAN, 1], [NAN, NAN, 0, NAN, NAN, 1], [5.5 + 4 / 6, 7.0, 1, 6, (7.0 - (5.5 + 4 / 6)) / 20.0, 3],
             [7.5 + 2 / 6, 12.0, 0, NAN, (12.0 - (7.5 + 2 / 6)) / 20.0, 1], [13.0, 14.75, 0, NAN, 1.75 / 20.0, 1], [18.0, 19.0, 0, NAN, 1.0 / 20.0, 1]]
# thr, the mean of the 20 finite speeds (96 / 20), 6 runs, 1 left-led, 0 right-led, 5 unattributed; the one double support's time, SD 0, the left mean;
# no right mean, no asymmetry; no stride
HAND_ROW = [5.0, 4.8, 6, 1, 0, 5, (7.0 - (5.5 + 4 / 6)) / 20.0, 0.0, (7.0 - (5.5 + 4 / 6)) / 20.0, NAN, NAN, 0] + [NAN] * 8


def hand_case():
    """(speeds (22,), events (22,)) of the hand-made case."""
    events = np.zeros(22, np.int32)
    for frame, bits in HAND_STRIKES.items():
        events[frame] = bits
    return np.asarray(HAND_SPEED, np.float64), events


def write_case(path, joints, table, speeds, events, rule, max_runs, host):
    """The file tests/helpers/gait_contacts_check.cpp reads: ONE sequence, sigma = 0.  joints None: the hook's case, on speeds."""
    T, J = (len(speeds), 0) if joints is None else joints.shape[:2]
    with open(path, "wb") as f:
        f.write(np.array([T, J, rule["reach"], rule["max_frames"], max_runs], "<i4").tobytes() + np.asarray(table, "<i4").tobytes())
        f.write(np.array([rule["fps"], rule["fraction"], rule["speed"]], "<f8").tobytes())
        f.write(np.ascontiguousarray(speeds, "<f8").tobytes() if joints is None else np.ascontiguousarray(joints, "<f4").tobytes())
        f.write(np.ascontiguousarray(events, "<i4").tobytes())
        if joints is not None:
            f.write(np.ascontiguousarray(host["per_frame"], "<f8").tobytes())
        f.write(np.ascontiguousarray(host["phase"], "<i4").tobytes() + np.ascontiguousarray(host["runs"][0], "<f8").tobytes())
        f.write(np.ascontiguousarray(host["per_sequence"][0], "<f8").tobytes())
    return path
