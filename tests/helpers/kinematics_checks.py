"""An articulated walker and the bars of the joint-angle kinematics, shared by the host and the GPU tests.  Nothing here calls the code
under test.  u = 2^-53.

THE WALKER.  A skeleton of J joints in the camera frame of the SMPL stage (x right, y down, z away), made by forward kinematics in the body's own
frame (F forward, N left, W up).  The upright body is turned by the yaw theta about y (theta = 0 faces the camera: forward = -z, left = +x); the body
frame is the upright one tipped forward by the trunk's inclination `trunk` about N, so W = cos(trunk) up + sin(trunk) forward.  Pelvis at the
origin, spine-shoulder 0.5 m along W, hips 0.1 m and shoulders 0.18 m to either side.  With w = 2 pi / P and s = t + phi:
  hip flexion      h(t) = HIP sin(w s) left, -HIP sin(w s) right (antiphase); hip abduction ABD, fixed, both sides
                   thigh = 0.42 (tan h, +-tan ABD, -1) / |.| in (F, N, W): atan2(d . F, -(d . W)) = h and atan2(+-(d . N), -(d . W)) = ABD exactly
  knee flexion     k(t) = K0 + K1 (1 - cos(w s - 0.9)), the right one half a period later; shank = 0.40 (cos k thigh^ + sin k back), back = the unit
                   vector across the thigh that points most against F: the angle between thigh and shank is k exactly
  ankle            a(t) = A0 + A1 sin(w s - 0.5), right half a period later; foot = 0.15 (cos(90 + a) shank^ + sin(90 + a) ahead), ahead = the unit
                   vector across the shank that points most along F: the angle between shank and foot is 90 + a
  shoulder flexion -+ARM sin(w s): each arm against its own leg; the right arm swings `arm_right` times the left one's amplitude
                   upper arm = 0.30 (tan, 0, -1) / |.|
  elbow flexion    e(t) = E0 + E1 (1 - cos(w s - 0.4)), right half a period later; forearm = 0.25 (cos e arm^ + sin e ahead)
  trunk            `trunk`, fixed: the angle between W and the camera's up (0, -1, 0)
The heel strikes are where the walker of gait_checks.py has them: the left foot at round(P / 4 - phi + k P) -- the hip's flexion is largest there --
the right one half a period later.  The events are GIVEN to the code under test, as an input.  The joints the table does not name get fixed offsets.

THE ANALYTIC BAR (analytic_bars; derived, not measured).  The joints are rounded to float32: each coordinate moves by at most eps = 2^-24 max|coordinate|,
a difference of two joints by at most 2 sqrt(3) eps in length, so the DIRECTION of a segment of length len by at most e(len) = 2 sqrt(3) eps / len
radians (to first order; the next term is its cube).  An angle between two segments moves by at most e(len1) + e(len2).  The axes: l = 0.2 m,
u = 0.5 m; f = l x u normalised moves by at most e(l) + e(u), n by e(l), w = f x n by 2 e(l) + e(u); an angle measured in the plane of two axes moves
by at most [e(segment) + e(axis 1) + e(axis 2)] / (the share of the segment that lies in that plane), and that share is at least cos(ABD) for
flexion (plane F, W) and cos(HIP) for abduction (plane N, W).  The trunk's inclination moves by e(u).  Float64 arithmetic adds 1e-9 degrees at most
(gait_atan2 is within 4 u pi).

THE BARS with sigma > 0 (with sigma = 0 both sides run the same operations in the same order: every bit is equal).  b = 2 gauss_bar(raw column of
the sequence) per angle column, as gait_checks.py derives it; M = max|raw column|; n = strides used.
  counts       finiteness spreads alike on both sides (every weight is positive): EQUAL BITS.
  cycle point  x0 + (x1 - x0) f, 0 <= f < 1, a convex combination of two values within b, three roundings a side of values <= 2 M: b_pt = b + 16 u M
  its mean     b_mean = b_pt + 2 (n + 1) u M;  its SD  b_pt + b_mean + 2 (n + 3) u SD   (gait_checks.py's step length, word for word)
  max, min     selections: within b; their means b + 2 (n + 1) u M
  ROM          max - min, one rounding a side: b_rom = 2 b + 4 u M; its mean b_rom + 4 (n + 1) u M; its SD b_rom + that + 2 (n + 3) u SD
  symmetry     S = 100 |L - R| / D, D = 0.5 (L + R), L and R within B_L, B_R (the ROM means' bars), s = B_L + B_R, D' = D - s / 2 > 0 (asserted):
               100 (s / D' + |L - R| (s / 2) / (D D')) + 12 u S"""
import numpy as np

from . import track_checks as tk
from .gait_checks import same_bits  # noqa: F401  (the tests use it through this module)

U = 2.0 ** -53
KINECTV2 = (0, 20, 12, 16, 13, 17, 14, 18, 15, 19, 4, 8, 5, 9, 6, 10)
OTHER49 = (39, 3, 28, 27, 30, 25, 22, 19, 44, 41, 7, 11, 33, 35, 14, 47)
HEEL_L, HEEL_R = 1, 2
THIGH, SHANK, FOOT, UPPER_ARM, FOREARM = 0.42, 0.40, 0.15, 0.30, 0.25
HIP, ABD, K0, K1, A0, A1, ARM, E0, E1, TRUNK = 25.0, 6.0, 5.0, 28.0, 2.0, 9.0, 18.0, 15.0, 12.0, 8.0      # degrees
AXIS_CHANNELS, FREE_CHANNELS = (0, 1, 2, 3, 8, 9, 12), (4, 5, 6, 7, 10, 11)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def across(v, toward):
    """The unit vector across v (rows) that points most along `toward` (rows)."""
    v = unit(v)
    return unit(toward - (toward * v).sum(axis=-1, keepdims=True) * v)


def heel_strikes(T, P=21.7, phi=-3.02):
    """(left frames, right frames): round(P / 4 - phi + k P) and half a period later, inside [0, T)."""
    out = []
    for first in (P / 4 - phi, 3 * P / 4 - phi):
        k0 = int(np.floor(-first / P)) - 1
        frames = [int(np.rint(first + k * P)) for k in range(k0, k0 + int(T / P) + 4)]
        out.append([t for t in frames if 0 <= t < T])
    return out


def walker(T, theta=0.0, P=21.7, phi=-3.02, J=25, table=KINECTV2, degenerate=(), arm_right=1.0, hip=HIP, standing=False):
    """(joints (T,J,3) float32, analytic angles (T,13) float64 in degrees, events (T,) int32).  degenerate: frames whose left hip is put on the right
    hip (the analytic angles of those frames do not hold).  standing: no events at all."""
    t = np.arange(T, dtype=np.float64)
    w = 2.0 * np.pi / P
    s = t + phi
    rad = np.deg2rad
    c, sn = np.cos(theta), np.sin(theta)
    fwd0, left, up0 = np.array([-sn, 0.0, -c]), np.array([c, 0.0, -sn]), np.array([0.0, -1.0, 0.0])
    F = np.cos(rad(TRUNK)) * fwd0 - np.sin(rad(TRUNK)) * up0
    W = np.cos(rad(TRUNK)) * up0 + np.sin(rad(TRUNK)) * fwd0
    ang = np.zeros((T, 13))
    body = np.zeros((T, J, 3))                                 # (F, N, W) coordinates per joint
    body[:, :, 0] = 0.01 * np.arange(J)[None, :]
    body[:, :, 1] = 0.02 * ((np.arange(J) % 5) - 2)[None, :]
    body[:, :, 2] = 0.03 * ((np.arange(J) % 7) - 3)[None, :]
    ahead = np.broadcast_to(np.array([1.0, 0.0, 0.0]), (T, 3))
    body[:, table[0]] = 0.0
    body[:, table[1]] = (0.0, 0.0, 0.5)
    for side in (0, 1):
        sign, half = (1.0, 0.0) if side == 0 else (-1.0, np.pi)
        h = sign * hip * np.sin(w * s)
        k = K0 + K1 * (1.0 - np.cos(w * s - 0.9 + half))
        a = A0 + A1 * np.sin(w * s - 0.5 + half)
        sh = -sign * ARM * (arm_right if side else 1.0) * np.sin(w * s)
        e = E0 + E1 * (1.0 - np.cos(w * s - 0.4 + half))
        ang[:, 0 + side], ang[:, 2 + side], ang[:, 4 + side], ang[:, 6 + side], ang[:, 8 + side], ang[:, 10 + side] = h, ABD, k, a, sh, e
        thigh = unit(np.stack([np.tan(rad(h)), np.full(T, sign * np.tan(rad(ABD))), -np.ones(T)], axis=1))
        shank = np.cos(rad(k))[:, None] * thigh + np.sin(rad(k))[:, None] * across(thigh, -ahead)
        foot = np.cos(rad(90.0 + a))[:, None] * shank + np.sin(rad(90.0 + a))[:, None] * across(shank, ahead)
        arm = unit(np.stack([np.tan(rad(sh)), np.zeros(T), -np.ones(T)], axis=1))
        fore = np.cos(rad(e))[:, None] * arm + np.sin(rad(e))[:, None] * across(arm, ahead)
        p_hip = np.array([0.0, sign * 0.1, 0.0])[None, :]
        p_sho = np.array([0.0, sign * 0.18, 0.5])[None, :]
        body[:, table[2 + side]] = p_hip
        body[:, table[4 + side]] = p_hip + THIGH * thigh
        body[:, table[6 + side]] = body[:, table[4 + side]] + SHANK * shank
        body[:, table[8 + side]] = body[:, table[6 + side]] + FOOT * foot
        body[:, table[10 + side]] = p_sho
        body[:, table[12 + side]] = p_sho + UPPER_ARM * arm
        body[:, table[14 + side]] = body[:, table[12 + side]] + FOREARM * fore
    ang[:, 12] = TRUNK
    for f in degenerate:
        body[f, table[2]] = body[f, table[3]]
    joints = body[:, :, 0:1] * F + body[:, :, 1:2] * left + body[:, :, 2:3] * W
    events = np.zeros(T, np.int32)
    if not standing:
        hl, hr = heel_strikes(T, P, phi)
        events[hl] |= HEEL_L
        events[hr] |= HEEL_R
    return joints.astype(np.float32), ang, events


def analytic_bars(joints, hip=HIP):
    """(13,) degrees: how far the float32 rounding of `joints` can move each channel (the module's text derives it)."""
    eps = 2.0 ** -24 * float(np.abs(joints).max())

    def e(length):
        return 2.0 * np.sqrt(3.0) * eps / length
    e_l, e_u = e(0.2), e(0.5)
    e_f, e_n, e_w = e_l + e_u, e_l, 2 * e_l + e_u
    bars = np.zeros(13)
    bars[0:2] = (e(THIGH) + e_f + e_w) / np.cos(np.deg2rad(ABD))
    bars[2:4] = (e(THIGH) + e_n + e_w) / np.cos(np.deg2rad(hip))
    bars[4:6] = e(THIGH) + e(SHANK)
    bars[6:8] = e(SHANK) + e(FOOT)
    bars[8:10] = e(UPPER_ARM) + e_f + e_w
    bars[10:12] = e(UPPER_ARM) + e(FOREARM)
    bars[12] = e_u
    return np.rad2deg(bars) + 1e-9


def gauss64(column, sigma):
    """The Gaussian of scipy.ndimage.gaussian_filter1d (reflect, truncate 4) on one float64 column, written out here: the helper calls nothing under test."""
    r = int(4.0 * sigma + 0.5)
    k = np.arange(-r, r + 1)
    wts = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    wts = wts / wts.sum()
    n = column.size
    idx = np.arange(-r, n + r) % (2 * n)
    ext = column[np.where(idx < n, idx, 2 * n - 1 - idx)]
    return np.array([np.dot(ext[i:i + 2 * r + 1], wts) for i in range(n)])


def column_bars(raw, sigma):
    """b (13,) and M (13,) of ONE sequence: raw (T,13) = the statement's angles with sigma = 0, the columns that are filtered (the device's in every
    bit).  NaN left out; a column without a finite value has b = M = 0."""
    b, big = np.zeros(13), np.zeros(13)
    for c in range(13):
        col = raw[np.isfinite(raw[:, c]), c]
        if col.size:
            b[c], big[c] = 2.0 * tk.gauss_bar(col, sigma), np.abs(col).max()
    return b, big


def sequence_bars(host_curves, host_rows, raw, sigma):
    """(per_frame bars (13,), curve bars (13,101,2), row bars (13,6)) of ONE sequence; all zeros with sigma = 0."""
    frame, curve, row = np.zeros(13), np.zeros((13, 101, 2)), np.zeros((13, 6))
    if not sigma > 0:
        return frame, curve, row
    b, big = column_bars(raw, sigma)
    frame[:] = b
    for c in range(13):
        n = host_rows[c, 0]
        if not n > 0:
            continue
        b_pt = b[c] + 16 * U * big[c]
        b_mean = b_pt + 2 * (n + 1) * U * big[c]
        curve[c, :, 0] = b_mean
        curve[c, :, 1] = b_pt + b_mean + 2 * (n + 3) * U * host_curves[c, :, 1]
        row[c, 1] = row[c, 2] = b[c] + 2 * (n + 1) * U * big[c]
        b_rom = 2 * b[c] + 4 * U * big[c]
        row[c, 3] = b_rom + 4 * (n + 1) * U * big[c]
        row[c, 4] = b_rom + row[c, 3] + 2 * (n + 3) * U * host_rows[c, 4]
    for c in range(0, 12, 2):
        L, R, S = host_rows[c, 3], host_rows[c + 1, 3], host_rows[c, 5]
        if np.isfinite(S):
            s = row[c, 3] + row[c + 1, 3]
            D = 0.5 * (L + R)
            assert D - 0.5 * s > 0, "the symmetry index's denominator is within its bar of zero: not a fair input"
            row[c, 5] = row[c + 1, 5] = 100.0 * (s / (D - 0.5 * s) + abs(L - R) * 0.5 * s / (D * (D - 0.5 * s))) + 12 * U * S
    return frame, curve, row


def compare(got, host, raw, lengths, sigma):
    """A result (numpy arrays) against the statement's; raw (n,13): the statement's per_frame with sigma = 0 on the same call (None with sigma = 0).
    NaN in the same places; every value whose bar is 0 equal in every bit (with sigma = 0: all of them); the others within their bars.  A result
    without 'per_frame' (the hook's) is compared without it.  Returns the worst ratio to a bar (0.0 with sigma = 0)."""
    worst, a = 0.0, 0
    for q, T in enumerate(lengths):
        frame, curve, row = sequence_bars(host["curves"][q], host["per_sequence"][q], None if raw is None else raw[a:a + T], sigma)
        pairs = [("curves", got["curves"][q], host["curves"][q], curve), ("per_sequence", got["per_sequence"][q], host["per_sequence"][q], row)]
        if "per_frame" in got:
            pairs.append(("per_frame", got["per_frame"][a:a + T], host["per_frame"][a:a + T], np.broadcast_to(frame, (T, 13))))
        for name, g, h, bar in pairs:
            assert g.shape == h.shape and np.array_equal(np.isnan(g), np.isnan(h)), f"sequence {q}: {name} has a NaN on one side alone"
            exact = bar == 0
            assert same_bits(g[exact], h[exact]), f"sequence {q}: {name} differs in some bit where nothing may differ"
            loose = ~exact & np.isfinite(h)
            if loose.any():
                worst = max(worst, float((np.abs(g[loose] - h[loose]) / bar[loose]).max()))
        a += T
    return worst


def build_call(min_stride=8, J=25, table=KINECTV2):
    """The seven sequences of the device tests in one call: (joints, events, lengths, names).  A walk of 130 frames, lengths 1, min_stride and
    min_stride + 1 (the last with heel strikes of the left foot on its first and last frame: one stride of exactly min_stride frames), a standing
    body of 64 frames without events, 65 frames with one degenerate frame inside a stride, and 130 frames whose right foot never strikes."""
    parts = (("walk130", dict(T=130, theta=0.7, arm_right=0.6)), ("one", dict(T=1, theta=0.2)), ("min", dict(T=min_stride, theta=0.3)),
             ("min_1", dict(T=min_stride + 1, theta=0.4)), ("standing64", dict(T=64, theta=2.0, standing=True)),
             ("degenerate65", dict(T=65, theta=-1.1, degenerate=(20,))), ("no_right130", dict(T=130, theta=np.pi - 0.4, phi=1.9)))
    made = {name: list(walker(J=J, table=table, **kw)) for name, kw in parts}
    ev = made["min_1"][2]
    ev[:] = 0
    ev[[0, min_stride]] = HEEL_L
    made["min"][2][:] = 0
    made["min"][2][[0, min_stride - 1]] = HEEL_L                # a stride one frame short of min_stride
    made["no_right130"][2] &= ~np.int32(HEEL_R)
    names = [name for name, _ in parts]
    return (np.concatenate([made[k][0] for k in names]), np.concatenate([made[k][2] for k in names]), [kw["T"] for _, kw in parts], names)


def hand_case():
    """(angles (80,13), events (80,), min_stride 8, max_stride 25): integers.  The left foot strikes at 0, 10, 30, 35, 65, 75: strides of 10 and 20
    frames (used), 5 (under min_stride), 30 (over max_stride) and 10 frames (used; channel 4 has a NaN at frame 70 and loses it, alone).  The right
    foot strikes at 5, 25, 45: two strides of 20 frames.  Channel 12 is the ramp x[t] = t; channel c < 12 is (t t + 3 c) mod 17 - c."""
    t = np.arange(80)
    x = np.stack([((t * t + 3 * c) % 17 - c).astype(np.float64) for c in range(12)] + [t.astype(np.float64)], axis=1)
    x[70, 4] = np.nan
    ev = np.zeros(80, np.int32)
    ev[[0, 10, 30, 35, 65, 75]] |= HEEL_L
    ev[[5, 25, 45]] |= HEEL_R
    return x, ev, 8, 25


def write_case(path, kind, min_stride, max_stride, host, joints=None, table=None, angles=None, events=None):
    """The file tests/helpers/gait_angles_check.cpp reads: ONE sequence.  kind 0: joints (T,J,3) float32 and a table, the statement's per_frame, curves
    and rows with sigma = 0; kind 2: angles (T,13) float64 instead, curves and rows."""
    with open(path, "wb") as f:
        T = len(events)
        f.write(np.array([kind, T, 0 if joints is None else joints.shape[1], min_stride, max_stride], "<i4").tobytes())
        if kind == 0:
            f.write(np.asarray(table, "<i4").tobytes() + np.ascontiguousarray(joints, "<f4").tobytes())
        else:
            f.write(np.ascontiguousarray(angles, "<f8").tobytes())
        f.write(np.ascontiguousarray(events, "<i4").tobytes())
        if kind == 0:
            f.write(np.ascontiguousarray(host["per_frame"], "<f8").tobytes())
        f.write(np.ascontiguousarray(host["curves"][0], "<f8").tobytes() + np.ascontiguousarray(host["per_sequence"][0], "<f8").tobytes())
    return path


def write_atan_case(path, y, x, want):
    """kind 1: n pairs (y, x) and what the statement's gait_atan2 made of them."""
    with open(path, "wb") as f:
        f.write(np.array([1, len(y), 0, 0, 0], "<i4").tobytes())
        f.write(np.ascontiguousarray(y, "<f8").tobytes() + np.ascontiguousarray(x, "<f8").tobytes() + np.ascontiguousarray(want, "<f8").tobytes())
    return path
