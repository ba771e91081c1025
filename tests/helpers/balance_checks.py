"""The cases, a plain-loop restatement and the bars of the balance call, shared by the host and the GPU tests.  Nothing here calls the
code under test.

THE WALKER is contact_checks.planted_walker: its feet STAND STILL IN THE WORLD while the pelvis moves on at v metres a frame along a straight line.
With the one-segment table ((0, 20, 1.0, 0.5)) the centre of mass is a fixed point of the trunk, so in exact arithmetic, for a step whose frames
t2 - window .. t2 + settle all see both feet where the rule needs them planted,
    COM speed = v fps;   MoS_ML = 0.09 (the ankles sit 0.09 m to either side of the line);   stride length = v P;   lateral excursion = 0;
    vertical excursion = 0 where the stance ankle is on the ground in every frame of the stride.

THE BARS (closed_form_bars) come from the float32 rounding of the joints alone.  Every coordinate of the walker is below 2 m, so a joint's coordinate
is off by at most E = 2^-24; float64 operations on top of it add less than SLACK = 1e-12.
  c            one segment, fraction 0.5: a mean of two joints, E.          rX = c - ankle: 2 E a component.
  v            (N / D) fps with k = -w/2 .. w/2: sum |k| 2 E / D fps a component, b_v;  sp: 2 b_v (both components).
  b            rX - rY at one frame: 4 E a component.
  direction    a and left are v / sp: turned by at most 2 b_v / sp_min, which moves a projection of a vector of length <= 1 m (b - xi) by that.
  MoS_ML       b: 4 E; xi: 2 E + b_v / w0_min, w0 = sqrt(g / l) >= 3 for l <= 0.81; the direction term.
  stride       q = b_j + b_(j-1) up to float64: 8 E a component, L: 16 E.
  lateral      a term is rX (2 E) or b + rX (6 E) along a direction p off by 16 E / L_min, times its length <= L + 0.5; max - min doubles it.
  vertical     G_y adds one b_y (4 E) a step, rX_y 2 E; max - min doubles it.  ON TOP: the events' extremum may fall on the frame BEFORE the landing
               (DESIGN 4.11), where the new stance ankle is still in the air by lift(t1), which the walker states in closed form (ankle_track): the
               bar of a stride adds the lifts of its two stance ankles at their own t1.  That is the walker's lift, not a figure of the code.
"""
import math

import numpy as np

from . import contact_checks as cc
from . import gait_checks as gc

FPS = cc.FPS
E = 2.0 ** -24
SLACK = 1e-12
same_bits = gc.same_bits
WALKERS, YAWS = cc.WALKERS, cc.YAWS
ONE_SEGMENT = ((0, 20, 1.0, 0.5),)
DEFAULTS = dict(fps=FPS, gravity=9.81, window=4, settle=1, max_step=30)
NAN = float("nan")


def walker_cases(T=400):
    """[(name, joints (T,25,3) float32, (P, beta, speed, phi, theta))]: the four walkers at the three yaws, phi = 0.3."""
    cases = []
    for P, beta, speed in WALKERS:
        for theta in YAWS:
            cases.append((f"P{P}_yaw{theta:.2f}", cc.planted_walker(T, P, beta, speed, 0.3, theta), (P, beta, speed, 0.3, theta)))
    return cases


def stance_lift(t, side, P, beta, speed, phi):
    """How far the ankle of `side` (+1 left, -1 right) is off the ground at frame t, from the walker's closed form."""
    v = speed / FPS
    return float(cc.ankle_track(np.asarray([float(t) if side > 0 else t - P / 2]), P, beta, v, phi)[1][0])


def closed_form_bars(P, beta, speed, window=4, n_steps=64):
    """{what: bar} for the closed forms above on the clean walker with ONE_SEGMENT."""
    k = [i - window / 2.0 for i in range(window + 1)]
    b_v = sum(abs(x) for x in k) * 2 * E / sum(x * x for x in k) * FPS
    sp_min, L_min = speed, speed / FPS * P
    turn = 2 * b_v / sp_min
    return {"com_speed": 2 * b_v + SLACK, "mos_ml": 4 * E + 2 * E + b_v / 3.0 + turn + SLACK, "stride_length": 16 * E + SLACK,
            "lateral": 2 * (6 * E + 16 * E / L_min * (L_min + 0.5)) + SLACK, "vertical": 2 * (2 * E + 4 * E * n_steps) + SLACK}


# ---- rules 1 to 8 as plain loops over Python floats (every operation an IEEE double operation, math.sqrt correctly rounded)
def _finite(v):
    return v - v == 0.0


def loops_rel(joints, table, segments):
    """Rule 1: rel (n,9) from joints (n,J,3) float32."""
    j = np.asarray(joints, np.float32)
    rel = np.empty((j.shape[0], 9))
    with np.errstate(all="ignore"):
        for f in range(j.shape[0]):
            den = 0.0
            for _, _, m, _ in segments:
                den = den + float(m)
            for a in range(3):
                num = 0.0
                for prox, dist, m, p in segments:
                    P, D = float(j[f, int(prox), a]), float(j[f, int(dist), a])
                    num = num + float(m) * (P + float(p) * (D - P))
                c = num / den if den != 0 else NAN
                rel[f, a], rel[f, 3 + a], rel[f, 6 + a] = c, c - float(j[f, table[4], a]), c - float(j[f, table[5], a])
    return rel


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return NAN if a == 0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else NAN


def _mean_sd(values):
    if not values:
        return NAN, NAN
    s = 0.0
    for v in values:
        s = s + v
    mean = s / len(values)
    acc = 0.0
    for v in values:
        acc = acc + (v - mean) * (v - mean)
    return mean, _sqrt(acc / len(values))


FAULTS = ("settle", "centre", "root", "swap", "restart", "stance", "same_foot", "nan_zero")


def loops_sequence(rel, events, fps, gravity, window, settle, max_step, max_steps, fault=None):
    """Rules 2 to 8 of ONE sequence: (per_frame (T,8), steps (max_steps,15), row (24,)).  fault: one of FAULTS, a mistake planted on purpose, which
    compare must catch: settle 0 for 1; the slope centred wrongly; w0 without the root; left and right swapped in MoS_ML; a footprint sum that restarts
    inside a chain; W taken from the wrong stance at t2; a chain not broken at a same-foot pair; a NaN written as 0."""
    T = len(events)
    r = [[float(v) for v in row] for row in rel]
    strikes = [(t, int(events[t]) & 3) for t in range(T) if int(events[t]) & 3]          # rule 2; a 3 is a strike of neither foot
    found = []                                                   # per pair: None or a dict
    for (t1, X), (t2, Y) in zip(strikes[:-1], strikes[1:]):
        step = None
        tb = t2 + (0 if fault == "settle" else settle)
        if X != 3 and Y != 3 and (X != Y or fault == "same_foot") and window <= t2 - t1 <= max_step and tb <= T - 1:
            cx, cy = (3 if X == 1 else 6), (3 if Y == 1 else 6)
            good = all(_finite(r[t][cx + a]) for t in range(t1, t2 + 1) for a in range(3))
            b = [r[tb][cx + a] - r[tb][cy + a] for a in range(3)]
            if good and all(_finite(v) for v in b):
                N, D = [0.0, 0.0, 0.0], 0.0
                for i in range(window + 1):
                    k = i - (window + 1 if fault == "centre" else window) / 2.0
                    for a in range(3):
                        N[a] = N[a] + k * r[t2 - window + i][cx + a]
                    D = D + k * k
                vx, vz = (N[0] / D) * fps, (N[2] / D) * fps
                sp = _sqrt(vx * vx + vz * vz)
                ell = -r[t2][cx + 1]
                if sp > 0 and _finite(sp) and ell > 0:
                    ax, az = vx / sp, vz / sp
                    lx, lz = -az, ax
                    w0 = gravity / ell if fault == "root" else _sqrt(gravity / ell)
                    xi = (r[t2][cx] + _div(vx, w0), r[t2][cx + 2] + _div(vz, w0))
                    sY = 1.0 if Y == 1 else -1.0
                    step = dict(t1=t1, t2=t2, sY=sY, cx=cx, b=b, sp=sp, ap=(b[0] - xi[0]) * ax + (b[2] - xi[1]) * az,
                                ml=(-sY if fault == "swap" else sY) * ((b[0] - xi[0]) * lx + (b[2] - xi[1]) * lz))
        found.append(step)
    chains, current = [], None                                   # rule 5
    for step in found:
        if step is None:
            current = None
            continue
        if current is None:
            current = []
            chains.append(current)
        G0 = current[-1]["G1"] if current and not (fault == "restart" and len(current) == 2) else [0.0, 0.0, 0.0]
        step["G0"], step["G1"], step["chain"], step["j"] = G0, [G0[a] + step["b"][a] for a in range(3)], len(chains) - 1, len(current)
        current.append(step)
    per_frame = [[r[t][0], r[t][1], r[t][2], NAN, NAN, NAN, 0.0, NAN] for t in range(T)]
    rows = []
    for chain in chains:
        for j, s in enumerate(chain):
            row = [float(s["t1"]), float(s["t2"]), s["sY"], float(s["chain"])] + s["G1"] + [NAN, NAN, NAN, s["sp"], s["ap"], s["ml"], NAN, NAN]
            if j >= 1:                                           # rules 6 and 8
                before = chain[j - 1]
                Gm = before["G0"]
                qx, qz = s["G1"][0] - Gm[0], s["G1"][2] - Gm[2]
                L = _sqrt(qx * qx + qz * qz)
                ys, lats = [], []
                if L > 0:
                    px, pz = qx / L, qz / L
                    row[7], row[8], row[9] = L, s["b"][0] * px + s["b"][2] * pz, abs(s["b"][0] * (-pz) + s["b"][2] * px)
                for t in range(before["t1"], s["t2"] + 1):
                    own = s if t >= s["t1"] else before
                    W = [own["G0"][a] + r[t][own["cx"] + a] for a in range(3)]
                    ys.append(W[1])
                    if L > 0:
                        lats.append((W[0] - Gm[0]) * (-pz) + (W[2] - Gm[2]) * px)
                row[13] = (max(ys) - min(ys)) + 0.0
                if L > 0:
                    row[14] = (max(lats) - min(lats)) + 0.0
            rows.append(row)
    everything = [s for chain in chains for s in chain]
    holder = {}                                                  # rule 7: the largest t1 <= t among the steps that hold t
    for s in everything:
        for t in range(s["t1"], s["t2"] + 1):
            if t not in holder or (s["t1"] > holder[t]["t1"]) != (fault == "stance"):
                holder[t] = s
    for t, s in holder.items():
        per_frame[t][3:8] = [s["G0"][a] + r[t][s["cx"] + a] for a in range(3)] + [-s["sY"], float(s["chain"])]
    steps = [[NAN] * 15 for _ in range(max_steps)]
    for i, row in enumerate(rows[:max_steps]):
        steps[i] = row
    out = [NAN] * 24
    out[0], out[1], out[2] = float(sum(1 for _, f in strikes if f != 3)), float(len(rows)), float(len(chains))
    out[3] = float(sum(1 for row in rows if row[7] == row[7]))
    for col, src in zip((4, 6, 8, 11, 14, 16, 20, 22), (7, 8, 9, 10, 11, 12, 13, 14)):
        out[col], out[col + 1] = _mean_sd([row[src] for row in rows if row[src] == row[src]])
    side = {}
    for src in (8, 12):
        for sign in (1.0, -1.0):
            side[src, sign] = _mean_sd([row[src] for row in rows if row[2] == sign and row[src] == row[src]])[0]
    if side[8, 1.0] == side[8, 1.0] and side[8, -1.0] == side[8, -1.0]:
        out[10] = (100.0 * abs(side[8, 1.0] - side[8, -1.0])) / (0.5 * (side[8, 1.0] + side[8, -1.0]))
    out[18], out[19] = side[12, 1.0], side[12, -1.0]
    if rows:
        dist = time = 0.0
        for s in everything:
            dist = dist + _sqrt(s["b"][0] * s["b"][0] + s["b"][2] * s["b"][2])
            time = time + (s["t2"] - s["t1"]) / fps
        out[13] = _div(dist, time)
    steps = np.asarray(steps, np.float64)
    return np.asarray(per_frame, np.float64), np.nan_to_num(steps, nan=0.0) if fault == "nan_zero" else steps, np.asarray(out, np.float64)


def loops_steps(rel, events, lengths=None, fps=FPS, gravity=9.81, window=4, settle=1, max_step=30, max_steps=256, fault=None):
    rel = np.asarray(rel, np.float64)
    lengths = [rel.shape[0]] if lengths is None else list(lengths)
    frames, steps, rows, a = [], [], [], 0
    with np.errstate(all="ignore"):
        for T in lengths:
            f, s, row = loops_sequence(rel[a:a + T], events[a:a + T], float(fps), float(gravity), int(window), int(settle), int(max_step), int(max_steps), fault)
            frames.append(f), steps.append(s), rows.append(row)
            a += T
    return {"per_frame": np.concatenate(frames), "steps": np.stack(steps), "per_sequence": np.stack(rows)}


def loops_balance(joints, events, lengths=None, segments=ONE_SEGMENT, table=gc.KINECTV2, **kw):
    rel = loops_rel(joints, table, segments)
    out = loops_steps(rel, events, lengths, **kw)
    out["rel"] = rel
    return out


def compare(got, want, what=""):
    """EQUAL BITS, NaN patterns included, in every output the two sides share (per_frame, steps, per_sequence, and rel where both have it)."""
    for key in ("per_frame", "steps", "per_sequence") + (("rel",) if "rel" in got and "rel" in want else ()):
        g, w = np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)
        assert g.shape == w.shape, f"{what}{key}: shape {g.shape} against {w.shape}"
        if not same_bits(g, w):
            bad = np.argwhere(~((g.view(np.int64) == w.view(np.int64)) | (np.isnan(g) & np.isnan(w))))
            first = tuple(int(v) for v in bad[0])
            raise AssertionError(f"{what}{key} differs in {len(bad)} entries, first at {first}: {g[first]!r} against {w[first]!r}")


# ---- the hand-made case of the hook: 32 frames, fps 1, gravity 4, window 2, settle 1, max_step 4.  A body whose centre of mass moves at 1 m a frame
# along +z at height 1 m over feet that land 1 m ahead of it, the left at x = -2, the right at x = +2; the centre of mass dips by 0.125 m in frame
# t1 + 2 of every step.  r_X(t) = COM(t) - the print of X's latest landing.
HAND_RULE = dict(fps=1.0, gravity=4.0, window=2, settle=1, max_step=4)
HAND_T = 32
#   0 L, 3 R, 6 L, 9 R: three steps, chain 0.   11 R: the same foot again.   12: both feet.   14 L after it: no step.   17 R: a NaN in rL(16), inside
#   the window [15, 17].   23 L: six frames after 17 > max_step.   26 R, 29 L: two steps, chain 1.
HAND_SPURIOUS = (11,)                                         # an event where no foot lands: the right foot stays on its print of frame 9
HAND_STRIKES = {0: 1, 3: 2, 6: 1, 9: 2, 11: 2, 12: 3, 14: 1, 17: 2, 23: 1, 26: 2, 29: 1}
HAND_DIPS = (2, 5, 8, 25, 28)
# every step: sp = 1 (the slope of z over three frames, (2 - 0) / 2), l = 1, w0 = sqrt(4 / 1) = 2, xi = (-x_X, 2 + 1 / 2), b = (x_Y - x_X, 0, 3) = (+-4, 0, 3),
# MoS_AP = 3 - 2.5 = 0.5, MoS_ML = |x_Y| = 2; a stride: q = (0, 6), L = 6, step length 3, step width 4; the dip: vertical excursion 0.125; lateral 0.
HAND_STEPS = [[0, 3, -1, 0, 4, 0, 3, NAN, NAN, NAN, 1, 0.5, 2, NAN, NAN],
              [3, 6, 1, 0, 0, 0, 6, 6, 3, 4, 1, 0.5, 2, 0.125, 0],
              [6, 9, -1, 0, 4, 0, 9, 6, 3, 4, 1, 0.5, 2, 0.125, 0],
              [23, 26, -1, 1, 4, 0, 3, NAN, NAN, NAN, 1, 0.5, 2, NAN, NAN],
              [26, 29, 1, 1, 0, 0, 6, 6, 3, 4, 1, 0.5, 2, 0.125, 0]]
# 10 strikes of one foot (frame 12 is none), 5 steps, 2 chains, 3 strides; stride 6, step 3, width 4, all SD 0; asymmetry 0; sp 1; ground speed
# (5 + 5 + 5 + 5 + 5) / (3 + 3 + 3 + 3 + 3); MoS_AP 0.5; MoS_ML 2, left landings 2, right landings 2; vertical 0.125; lateral 0
HAND_ROW = [10, 5, 2, 3, 6, 0, 3, 0, 4, 0, 0, 1, 0, 25.0 / 15.0, 0.5, 0, 2, 0, 2, 2, 0.125, 0, 0, 0]
HAND_SIDE = [1, 1, 1, -1, -1, -1, 1, 1, 1, 1] + [0] * 13 + [1, 1, 1, -1, -1, -1, -1, 0, 0]
HAND_CHAIN = [0] * 10 + [NAN] * 13 + [1] * 7 + [NAN] * 2


def hand_case():
    """(rel (32,9), events (32,), expected per_frame (32,8)) of the hand-made case."""
    events = np.zeros(HAND_T, np.int32)
    for frame, bits in HAND_STRIKES.items():
        events[frame] = bits
    rel = np.zeros((HAND_T, 9))
    prints = {1: (-2.0, 0.0, -2.0), 2: (2.0, 0.0, -0.5)}         # before their first landing the feet stand somewhere behind
    for t in range(HAND_T):
        bits = HAND_STRIKES.get(t, 0)
        if bits in (1, 2) and t not in HAND_SPURIOUS:
            prints[bits] = (-2.0 if bits == 1 else 2.0, 0.0, t + 1.0)
        com = (0.0, -1.125 if t in HAND_DIPS else -1.0, float(t))
        rel[t, 0:3] = com
        rel[t, 3:6] = [com[a] - prints[1][a] for a in range(3)]
        rel[t, 6:9] = [com[a] - prints[2][a] for a in range(3)]
    rel[16, 3:6] = NAN
    frame = np.full((HAND_T, 8), NAN)
    frame[:, 0:3] = rel[:, 0:3]
    frame[:, 6], frame[:, 7] = HAND_SIDE, HAND_CHAIN
    for t in range(HAND_T):                                      # W: the centre of mass from the chain's first print, (-2, 0, 1) and (-2, 0, 24)
        if t <= 9 or 23 <= t <= 29:
            frame[t, 3:6] = [2.0, rel[t, 1], t - (1.0 if t <= 9 else 24.0)]
    return rel, events, frame


def write_case(path, joints, table, segments, rel, events, rule, max_steps, host):
    """The file tests/helpers/gait_balance_check.cpp reads: ONE sequence.  joints None: the hook's case, on rel."""
    T, J = (len(events), 0) if joints is None else joints.shape[:2]
    seg = np.zeros((0, 4)) if joints is None else np.asarray(segments, np.float64)
    with open(path, "wb") as f:
        f.write(np.array([T, J, len(seg), rule["window"], rule["settle"], rule["max_step"], max_steps], "<i4").tobytes() + np.asarray(table, "<i4").tobytes())
        f.write(np.array([rule["fps"], rule["gravity"]], "<f8").tobytes())
        f.write(np.ascontiguousarray(seg[:, :2], "<i4").tobytes() + np.ascontiguousarray(seg[:, 2:], "<f8").tobytes())
        f.write(np.ascontiguousarray(rel, "<f8").tobytes() if joints is None else np.ascontiguousarray(joints, "<f4").tobytes())
        f.write(np.ascontiguousarray(events, "<i4").tobytes())
        if joints is not None:
            f.write(np.ascontiguousarray(host["rel"], "<f8").tobytes())
        f.write(np.ascontiguousarray(host["per_frame"], "<f8").tobytes() + np.ascontiguousarray(host["steps"][0], "<f8").tobytes())
        f.write(np.ascontiguousarray(host["per_sequence"][0], "<f8").tobytes())
    return path
