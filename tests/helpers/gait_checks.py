"""A synthetic walker and the bars of the gait events and parameters, shared by the host and the GPU tests.  Nothing here calls the
code under test.  u = 2^-53.

THE WALKER.  A skeleton of J joints in the camera frame of the SMPL stage (x right, y down, z away).  In the body's own frame (forward, left, up)
the pelvis is the origin, spine-shoulder 0.5 m up, the hips 0.1 m to either side, the ankles 0.8 m down and 0.1 m to either side, the feet 0.85 m
down.  The left ankle lies A sin(2 pi (t + phi) / P) ahead of the pelvis, the right one the same behind (antiphase); each foot follows its ankle
`lag` frames later.  The body is turned by the yaw theta about y (theta = 0 faces the camera: forward = -z, left = +x) and the whole of it walks
along its facing at 4 A / P metres a frame -- two steps of 2 A a period -- which goes into `trans`, as the model's joints are root-relative.  The
joints the table does not name get fixed offsets from the pelvis.  P is no integer (21.7), so the analytic extrema fall strictly between frames
and no two samples of a window tie.

EXPECTED EVENTS.  The left heel strikes where its ankle signal is largest: t = P / 4 - phi + k P; the right half a period later; the left toe
leaves where its foot signal is smallest: t = 3 P / 4 - phi + lag + k P; the right half a period earlier.  Of a sampled sinusoid the frame nearest to
the analytic extremum holds the extreme sample, so an event is expected at round(t) wherever [round(t) - w, round(t) + w] lies inside the
sequence.  expected_events REFUSES a walker one of whose extrema lies within 1.5 frames of the first or last frame that can hold an event: there
a shift of one frame, which the smoothing may cause, would make or lose an event.

THE MARGIN.  decision_margin is the smallest amount by which any comparison of the events rule is decided on given signals: |h(t)|,
|h(t) - h(t +- i)|, |excursion - min_excursion|, over every frame that has a whole window and every signal, NaN left out (a comparison with NaN is
false on both sides).  Every input of a test that goes through arithmetic must have a margin >= MIN_MARGIN = 1e-6 m: the two sides' signals differ
by 1e-15 m at most (the bars below), so they decide every comparison alike and THE EVENTS ARE EQUAL.  It is a condition on the inputs, asserted on
the CPU, not a tolerance on the output.

THE BARS with sigma > 0 (with sigma = 0 both sides run the same operations in the same order: every bit is equal).
  signals     b_k = 2 gauss_bar(raw column k of the sequence) -- the column that is filtered, which is the statement's own signal with sigma = 0 and,
              being made without a Gaussian, the device's in every bit: each side's Gaussian is within (2 r + 8) u max|x| of the exact one
              (tests/helpers/track_checks.py), and both sides err.  The width is not smoothed: equal bits.
  events, counts, steps, step and stride times, cadence, stance share, trajectory speed, step width: functions of the events, of integers and of
              unsmoothed values alone, the same operations on both sides: EQUAL BITS.
  step length at a strike: h_X - h_other, each side rounding its own difference once: b_len = b_L + b_R + 2 u max|length|.
  its mean    over n steps: every term within b_len, each side's sum with n - 1 roundings and one quotient: b_mean = b_len + 2 (n + 1) u max|length|.
  its SD      sqrt(sum(d^2) / n) with d = x - mean is 1 / sqrt(n) times a Euclidean norm, so it moves by no more than the largest change of a d,
              b_len + b_mean; each side's n squares, n - 1 additions, quotient and root are within (n + 3) u relative:
              b_sd = b_len + b_mean + 2 (n + 3) u SD.
  speed       mean length * cadence / 60 with the cadence equal: b_mean cadence / 60 + 4 u |speed|."""
import numpy as np

from . import track_checks as tk

U = 2.0 ** -53
MIN_MARGIN = 1e-6
KINECTV2 = (0, 20, 12, 16, 14, 18, 15, 19)                     # pelvis, spine-shoulder, lhip, rhip, lankle, rankle, lfoot, rfoot
OTHER49 = (39, 3, 28, 27, 30, 25, 22, 19)                      # another table, for J = 49
HEEL_L, HEEL_R, TOE_L, TOE_R = 1, 2, 4, 8
COL = {"steps": 4, "step_time": 5, "step_time_sd": 6, "cadence": 7, "stride": 8, "stride_sd": 9, "stride_cv": 10, "length": 11, "length_sd": 12, "width": 13,
       "width_sd": 14, "stance": 15, "speed": 16, "traj_speed": 17}
SMOOTHED_COLUMNS = (11, 12, 16)                                # the per-sequence columns the smoothing reaches


def walker(T, theta=0.0, A=0.3, P=21.7, phi=-3.02, lag=2.64, J=25, table=KINECTV2, degenerate=(), right=-1.0):
    """(joints (T,J,3) float32, trans (T,3) float64).  degenerate: frames whose left hip is put on the right hip.  right: the right ankle and foot
    swing `right` times the left ones' (-1: antiphase, a walk; 0.8: in phase and shorter -- a hopper, whose feet strike in the same frames)."""
    t = np.arange(T, dtype=np.float64)
    c, s = np.cos(theta), np.sin(theta)
    fwd, left, up = np.array([-s, 0.0, -c]), np.array([c, 0.0, -s]), np.array([0.0, -1.0, 0.0])       # the yaw about y of (0,0,-1) and (1,0,0)
    body = np.zeros((T, J, 3))                                 # (forward, left, up) per joint
    body[:, :, 0] = 0.01 * np.arange(J)[None, :]
    body[:, :, 1] = 0.02 * ((np.arange(J) % 5) - 2)[None, :]
    body[:, :, 2] = 0.03 * ((np.arange(J) % 7) - 3)[None, :]
    swing = A * np.sin(2.0 * np.pi * (t + phi) / P)
    trail = A * np.sin(2.0 * np.pi * (t + phi - lag) / P)
    zero = np.zeros(T)
    for k, (a, b, h) in enumerate(((zero, 0.0, 0.0), (zero, 0.0, 0.5), (zero, 0.1, 0.0), (zero, -0.1, 0.0), (swing, 0.1, -0.8), (right * swing, -0.1, -0.8),
                                   (trail, 0.1, -0.85), (right * trail, -0.1, -0.85))):
        body[:, table[k], 0], body[:, table[k], 1], body[:, table[k], 2] = a, b, h
    for f in degenerate:
        body[f, table[2]] = body[f, table[3]]
    joints = body[:, :, 0:1] * fwd + body[:, :, 1:2] * left + body[:, :, 2:3] * up
    trans = np.array([0.3, 0.1, 6.0]) + (walker_speed(A, P, 1.0) * t)[:, None] * fwd
    return joints.astype(np.float32), trans


def walker_speed(A, P, fps):
    """Metres a second: two steps of 2 A every P frames."""
    return 4.0 * A * fps / P


def expected_events(T, window, P=21.7, phi=-3.02, lag=2.64):
    """{bit: sorted frames} of the analytic extrema rounded to frames; AssertionError where one lies within 1.5 frames of the ends of the frames that
    can hold an event."""
    out = {}
    lo, hi = window, T - 1 - window                            # the first and last frame with a whole window
    for bit, first in ((HEEL_L, P / 4 - phi), (HEEL_R, 3 * P / 4 - phi), (TOE_L, 3 * P / 4 - phi + lag), (TOE_R, P / 4 - phi + lag)):
        frames = []
        k = int(np.floor(-first / P)) - 1
        while first + k * P < T + 1:
            x = first + k * P
            k += 1
            assert abs(x - (lo - 0.5)) > 1.5 and abs(x - (hi + 0.5)) > 1.5, f"an extremum at {x:.2f} is too close to frame {lo} or {hi}: choose another T or phi"
            if lo <= int(np.rint(x)) <= hi:
                frames.append(int(np.rint(x)))
        out[bit] = frames
    return out


def decision_margin(signals, window, min_excursion):
    """The smallest amount by which a comparison of the events rule is decided on signals (T,4) of ONE sequence; inf where there is none."""
    s = np.asarray(signals, np.float64)
    T, w = s.shape[0], int(window)
    best = np.inf
    if T < 2 * w + 1:
        return best
    for k in range(4):
        win = np.lib.stride_tricks.sliding_window_view(s[:, k], 2 * w + 1)
        v = win[:, w]
        exc = (v - win.min(axis=1)) if k < 2 else (win.max(axis=1) - v)
        for d in (np.abs(v), np.abs(v[:, None] - np.delete(win, w, axis=1)).ravel(), np.abs(exc - min_excursion)):
            d = d[np.isfinite(d)]
            if d.size:
                best = min(best, float(d.min()))
    return best


def assert_margin(per_frame, lengths, window, min_excursion):
    """The condition on the inputs: per_frame = the statement's rows (its smoothed signals) of a call."""
    a, worst = 0, np.inf
    for T in lengths:
        worst = min(worst, decision_margin(per_frame[a:a + T, :4], window, min_excursion))
        a += T
    assert worst >= MIN_MARGIN, f"the input decides a comparison by {worst:.3g} m < {MIN_MARGIN:g} m: not a fair input"
    return worst


def signal_bars(raw, sigma):
    """b_k, k = 0 .. 3, for ONE sequence: raw (T,4) = the columns that are filtered -- the statement's signals with sigma = 0 on the same joints, which
    are the device's in every bit.  A NaN of a degenerate frame is left out of max|x| (where it reaches, both sides hold NaN); a column without a
    finite value has the bar 0."""
    raw = np.asarray(raw, np.float64)
    return np.array([2.0 * tk.gauss_bar(raw[np.isfinite(raw[:, k]), k], sigma) if np.isfinite(raw[:, k]).any() else 0.0 for k in range(4)])


def parameter_bars(host_row, host_frames, b):
    """The bars of the per-sequence columns 11, 12 and 16 from the statement's own row and per-frame rows and the signals' bars b (4,)."""
    n = host_row[COL["steps"]]
    bars = np.zeros(18)
    if not n > 0:
        return bars
    length = host_frames[:, 5]
    big = np.nanmax(np.abs(length)) if np.isfinite(length).any() else 0.0
    b_len = b[0] + b[1] + 2 * U * big
    b_mean = b_len + 2 * (n + 1) * U * big
    bars[11] = b_mean
    bars[12] = b_len + b_mean + 2 * (n + 3) * U * host_row[12]
    bars[16] = b_mean * host_row[7] / 60.0 + 4 * U * abs(host_row[16])
    return bars


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def sequence_bars(host_frames, host_row, raw, sigma):
    """(bars of the 7 per-frame columns, bars of the 18 per-sequence columns) of ONE sequence; all zeros with sigma = 0."""
    frame, seq = np.zeros(7), np.zeros(18)
    if sigma > 0:
        b = signal_bars(raw, sigma)
        big = np.nanmax(np.abs(host_frames[:, 5])) if np.isfinite(host_frames[:, 5]).any() else 0.0
        frame[:4], frame[5] = b, b[0] + b[1] + 2 * U * big
        seq = parameter_bars(host_row, host_frames, b)
    return frame, seq


def compare(got, host, raw, lengths, sigma):
    """A result (numpy arrays) against the statement's; raw (n,4): the statement's signals with sigma = 0 on the same call (None with sigma = 0), the
    columns the bars are taken of.  The events equal; every value whose bar is 0 equal in every bit (with sigma = 0: all of
    them); the others within their bars.  Returns the worst ratio to a bar (0.0 with sigma = 0)."""
    assert np.array_equal(got["events"], host["events"]), "the events differ"
    worst, a = 0.0, 0
    for q, T in enumerate(lengths):
        gf, hf, gs, hs = got["per_frame"][a:a + T], host["per_frame"][a:a + T], got["per_sequence"][q], host["per_sequence"][q]
        frame, seq = sequence_bars(hf, hs, None if raw is None else raw[a:a + T], sigma)
        assert np.array_equal(np.isnan(gf), np.isnan(hf)) and np.array_equal(np.isnan(gs), np.isnan(hs)), f"sequence {q}: a NaN on one side alone"
        for c in range(7):
            if frame[c] == 0:
                assert same_bits(gf[:, c], hf[:, c]), f"sequence {q}: per_frame column {c} differs in some bit"
            elif np.isfinite(hf[:, c]).any():
                worst = max(worst, float(np.nanmax(np.abs(gf[:, c] - hf[:, c]))) / frame[c])
        for c in range(18):
            if seq[c] == 0:
                assert same_bits(gs[c], hs[c]), f"sequence {q}: per_sequence column {c} is {gs[c]!r}, not {hs[c]!r}"
            elif np.isfinite(hs[c]):
                worst = max(worst, abs(gs[c] - hs[c]) / seq[c])
        a += T
    return worst


def write_case(path, joints, trans, table, fps, sigma, window, min_excursion, host, weights, raw=None):
    """The file tests/helpers/gait_events_check.cpp reads: ONE sequence, its inputs, the bars and the statement's result `host`.  weights: the
    Gaussian's w[0 .. r] (None with sigma = 0); raw (T,4): the unsmoothed signals, for the bars (sigma > 0)."""
    T, J = joints.shape[:2]
    frame, seq = sequence_bars(host["per_frame"], host["per_sequence"][0], raw, sigma)
    with open(path, "wb") as f:
        f.write(np.array([T, J, window, trans is not None, -1 if weights is None else len(weights) - 1], "<i4").tobytes())
        f.write(np.asarray(table, "<i4").tobytes())
        f.write(np.array([fps, min_excursion], "<f8").tobytes() + frame.astype("<f8").tobytes() + seq.astype("<f8").tobytes())
        f.write(np.ascontiguousarray(joints, "<f4").tobytes())
        if trans is not None:
            f.write(np.ascontiguousarray(trans, "<f8").tobytes())
        if weights is not None:
            f.write(np.ascontiguousarray(weights, "<f8").tobytes())
        f.write(np.ascontiguousarray(host["per_frame"], "<f8").tobytes() + np.ascontiguousarray(host["events"], "<i4").tobytes())
        f.write(np.ascontiguousarray(host["per_sequence"][0], "<f8").tobytes())
    return path


def build_call(window, J=25, table=KINECTV2, P=21.7):
    """The seven sequences of the device tests in one call: (joints, trans, lengths, names).  Lengths 1, 2 w and 2 w + 1 -- the first that can hold
    an event, with a left heel strike put on its one frame that has a whole window -- a standing body of 64 frames (amplitude 0.02 m), 65 frames
    with one degenerate frame, and two walks of 130 frames (two words of the bitmasks and two bits) at other yaws."""
    w = int(window)
    on_frame_w = P / 4 - w - 0.03                              # phi that puts a left heel strike 0.03 frames behind frame w
    parts = (("walk130", dict(T=130, theta=0.7)), ("one", dict(T=1, theta=0.2)), ("two_w", dict(T=2 * w, theta=0.3, phi=on_frame_w)),
             ("two_w_1", dict(T=2 * w + 1, theta=0.4, phi=on_frame_w)), ("standing64", dict(T=64, theta=2.0, A=0.02)),
             ("degenerate65", dict(T=65, theta=-1.1, degenerate=(30,))), ("walk130_back", dict(T=130, theta=np.pi - 0.4, phi=1.9)))
    made = [walker(J=J, table=table, P=P, **kw) for _, kw in parts]
    return (np.concatenate([m[0] for m in made]), np.concatenate([m[1] for m in made]), [kw["T"] for _, kw in parts], [name for name, _ in parts])
