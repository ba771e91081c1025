"""The independent checker of the camera-space trajectory, for the tests of pipeline.fit_translation, of csrc/translation3.h on
the host and of grnet_fit_translation on the GPU, and for tools/make_goldens_translation.py.

The exact translation of a frame comes from fractions.Fraction on the widened float32 inputs with the REFERENCE's weights (float64 sqrt(conf))^2:
no rounding anywhere, so an error measured against it belongs to the code under test alone.  The bar on a fitted frame is derived, not tuned:
    |t - t_exact|_inf / |t_exact|_inf <= cond_2(A) 2^-52
the classical forward-error scale of a stable 3x3 solve (twice that against the golden reference values, since both sides err).  Every fitted frame
must have cond_2(A) <= 1e6, and no frame is left out.  The reprojection error is recomputed exactly (Fraction, one square root per pair) at the
translation the code returned -- t itself is held to the bar above -- and compared at 1e-10 relative plus (P + 8) 2^-53; the filled frames must
equal numpy.linspace on the code's own fitted rows bit for bit; the sequence's mean at 1e-10 + (T + 8) 2^-53 relative against math.fsum, and the
path length at (T + 8) 2^-53 relative plus 8 T 2^-53 x (largest |J_root + t|): a step is a difference of positions, each rounded once."""
import math
from fractions import Fraction

import numpy as np

FITTED, TOO_FEW, DEGENERATE, FILLED = 0, 1, 2, 3
EPS = 2.0 ** -52
MAX_COND = 1e6
# (image size, focal length, depth range in metres): the settings of the golden file (square centres: all the reference's signature allows)
GOLDEN_CAMERAS = ((224.0, 5000.0, (30.0, 60.0)), (1080.0, math.sqrt(1920.0 ** 2 + 1080.0 ** 2), (2.0, 8.0)), (1080.0, 1000.0, (2.0, 8.0)))


def widen(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def random_case(n, pairs, K3, K2, seed, f, centre, size, depth, dead=0.15):
    """float32 joints3d (n,K3,3) and joints2d (n,K2,3) of a body-sized cloud (spread 0.25 / 0.5 / 0.12 m) at a true translation `depth` metres
    away, projected through (f, centre) into a size[0] x size[1] image with 3 px noise; confidences in (0.05, 1), a share `dead` of them zeroed.
    Joints outside the pair table are NaN: nothing may read them (the root joint of the path length, index 0, stays finite).  Also t_true (n,3)."""
    g = np.random.Generator(np.random.Philox(key=[409, seed]))
    pairs = np.asarray(pairs)
    P = pairs.shape[0]
    body = g.normal(0.0, 1.0, (n, P, 3)) * np.array([0.25, 0.5, 0.12])
    t = np.empty((n, 3))
    t[:, 2] = g.uniform(depth[0], depth[1], n)
    t[:, 0] = g.uniform(-0.3, 0.3, n) * size[0] * t[:, 2] / f
    t[:, 1] = g.uniform(-0.3, 0.3, n) * size[1] * t[:, 2] / f
    cam = body + t[:, None, :]
    xy = f * cam[:, :, :2] / cam[:, :, 2:] + np.asarray(centre) + g.normal(0.0, 3.0, (n, P, 2))
    conf = g.uniform(0.05, 1.0, (n, P))
    conf[g.uniform(0, 1, (n, P)) < dead] = 0.0
    j3 = np.full((n, K3, 3), np.nan, np.float32)
    j2 = np.full((n, K2, 3), np.nan, np.float32)
    j3[:, 0] = g.normal(0.0, 0.1, (n, 3))
    j3[:, pairs[:, 0]] = body
    j2[:, pairs[:, 1], :2] = xy
    j2[:, pairs[:, 1], 2] = conf
    return j3, j2, t


def make_case(case, seed):
    """case = (P, K3, K2, n, lengths, [(f, cx, cy) per sequence], image size, depth range) -> joints3d, joints2d, pairs (a seeded choice of P
    joints of each skeleton; the 13 pairs of pipeline.BODY25_FROM_KINECTV2 at P = 13) and the keyword arguments of fit_translation."""
    P, K3, K2, n, lengths, cams, size, depth = case
    g = np.random.Generator(np.random.Philox(key=[seed, P]))
    pairs = np.stack([g.permutation(K3)[:P], g.permutation(K2)[:P]], axis=1)
    if P == 13:
        pairs = np.array([(0, 8), (4, 5), (5, 6), (6, 7), (8, 2), (9, 3), (10, 4), (12, 12), (13, 13), (14, 14), (16, 9), (17, 10), (18, 11)])
    j3, j2 = [], []
    for q, T in enumerate(lengths):
        f, cx, cy = cams[q]
        a, b, _ = random_case(T, pairs, K3, K2, seed * 10 + q, f, (cx, cy), size, depth, dead=0.0 if P == 4 else 0.15)
        j3.append(a)
        j2.append(b)
    cam = np.array(cams)
    return np.concatenate(j3), np.concatenate(j2), pairs, dict(lengths=lengths, focal_length=cam[:, 0], centre=cam[:, 1:])


def used_pairs(D, threshold):
    c = D[:, 2]
    return np.flatnonzero((c > threshold) & np.isfinite(c))


def normal_equations(S, D, used, f, cx, cy, sqrt_weights=True):
    """A (3x3) and b (3) of the frame as Fractions: S (P,3), D (P,3) the paired rows, widened.  sqrt_weights: the reference's (sqrt(conf))^2."""
    F = Fraction
    f, cx, cy = F(f), F(cx), F(cy)
    sw = swu = swv = swr = sbx = sby = sbz = F(0)
    for j in used:
        X, Y, Z = (F(float(v)) for v in S[j])
        w = F(float(np.sqrt(D[j, 2]))) ** 2 if sqrt_weights else F(float(D[j, 2]))
        u, v = F(float(D[j, 0])) - cx, F(float(D[j, 1])) - cy
        ex, ey = u * Z - f * X, v * Z - f * Y
        sw, swu, swv, swr = sw + w, swu + w * u, swv + w * v, swr + w * (u * u + v * v)
        sbx, sby, sbz = sbx + w * ex, sby + w * ey, sbz + w * (u * ex + v * ey)
    A = [[f * f * sw, F(0), -f * swu], [F(0), f * f * sw, -f * swv], [-f * swu, -f * swv, swr]]
    return A, [f * sbx, f * sby, -sbz]


def det3(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
            + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))


def exact_solve(A, b):
    """Cramer's rule in Fractions; None for a singular A."""
    d = det3(A)
    if d == 0:
        return None
    out = []
    for c in range(3):
        M = [[b[r] if k == c else A[r][k] for k in range(3)] for r in range(3)]
        out.append(det3(M) / d)
    return out


def exact_reproj(S, D, used, t, f, cx, cy):
    """The confidence-weighted mean of the pixel distances at translation t: the distances' squares exact, one square root each, math.fsum."""
    F = Fraction
    t = [F(float(v)) for v in t]
    terms, weights = [], []
    for j in used:
        X, Y, Z = (F(float(v)) for v in S[j])
        px = F(f) * (X + t[0]) / (Z + t[2]) + F(cx) - F(float(D[j, 0]))
        py = F(f) * (Y + t[1]) / (Z + t[2]) + F(cy) - F(float(D[j, 1]))
        w = float(D[j, 2])
        terms.append(w * math.sqrt(px * px + py * py))
        weights.append(w)
    return math.fsum(terms) / math.fsum(weights)


def frame_truth(S, D, f, cx, cy, threshold, min_joints):
    """(status, n_used, t_exact as floats or None, cond_2(A) or None) of one frame from the exact solution."""
    used = used_pairs(D, threshold)
    if used.size < min_joints:
        return TOO_FEW, used.size, None, None
    if not (np.isfinite(S[used]).all() and np.isfinite(D[used]).all()):
        return DEGENERATE, used.size, None, None
    A, b = normal_equations(S, D, used, f, cx, cy)
    t = exact_solve(A, b)
    if t is None or any(Fraction(float(S[j, 2])) + t[2] <= 0 for j in used):
        return DEGENERATE, used.size, None, None
    cond = float(np.linalg.cond(np.array([[float(v) for v in row] for row in A]), 2))
    return FITTED, used.size, np.array([float(v) for v in t]), cond


def compare(out, joints3d, joints2d, pairs, lengths=None, focal_length=5000.0, centre=(112.0, 112.0), conf_threshold=0.1, min_joints=4, root=0, fill=True,
            bar=1.0, other=None):
    """Every rule of DESIGN 4.9 on a result {per_frame (n,6), per_sequence (n_seq,4)} of numpy arrays -> (failures, worst ratios to the bars).
    A frame the exact solution calls singular or behind the camera must have status 2; no other frame may.
    other: a second result (the host statement beside the device's): the two must agree in n_used and status, on fitted frames within two bars
    in t -- both sides err -- and in the reprojection error within twice its tolerance plus 4 f cond 2^-52 pixels, what a two-bar change of t moves
    a projection by where |t| is at most twice the depth, as in every case here."""
    j3, j2, pairs = widen(joints3d), widen(joints2d), np.asarray(pairs)
    n = j3.shape[0]
    lengths = [n] if lengths is None else list(lengths)
    cam = np.empty((len(lengths), 3))
    cam[:, 0], cam[:, 1:] = focal_length, centre
    rows, seq = out["per_frame"], out["per_sequence"]
    fails, worst = [], {"t": 0.0, "reproj": 0.0, "mean": 0.0, "path": 0.0, "cond": 0.0}
    if other is not None:
        worst["other"] = 0.0
        if not np.array_equal(rows[:, 4:], other["per_frame"][:, 4:]) or not np.array_equal(seq[:, :2], other["per_sequence"][:, :2]):
            fails.append("the two results differ in n_used, status or the counts")
    if rows.shape != (n, 6) or seq.shape != (len(lengths), 4):
        return [f"shapes {rows.shape}, {seq.shape}"], worst
    P = pairs.shape[0]
    a = 0
    for q, T in enumerate(lengths):
        f, cx, cy = cam[q]
        r = rows[a:a + T]
        fit_status = np.empty(T, np.int64)
        for i in range(T):
            S, D = j3[a + i, pairs[:, 0]], j2[a + i, pairs[:, 1]]
            status, n_used, t, cond = frame_truth(S, D, f, cx, cy, conf_threshold, min_joints)
            fit_status[i] = status
            if r[i, 4] != n_used:
                fails.append(f"frame {a + i}: n_used {r[i, 4]}, {n_used} expected")
            if status != FITTED:
                continue
            worst["cond"] = max(worst["cond"], cond)
            if cond > MAX_COND:
                fails.append(f"frame {a + i}: cond {cond:.3e} above {MAX_COND:.0e}: the test's data, not the code")
            if r[i, 5] != FITTED:
                fails.append(f"frame {a + i}: status {r[i, 5]}, fitted expected")
                continue
            ratio = np.abs(r[i, :3] - t).max() / np.abs(t).max() / (bar * cond * EPS)
            worst["t"] = max(worst["t"], ratio)
            if not ratio <= 1.0:
                fails.append(f"frame {a + i}: t off by {ratio:.3g} bars (cond {cond:.3e})")
            want = exact_reproj(S, D, used_pairs(D, conf_threshold), r[i, :3], f, cx, cy)
            ratio = abs(r[i, 3] - want) / (want * (1e-10 + (P + 8) * 2.0 ** -53))
            worst["reproj"] = max(worst["reproj"], ratio)
            if not ratio <= 1.0:
                fails.append(f"frame {a + i}: reproj {r[i, 3]!r} against {want!r}: {ratio:.3g} bars")
            if other is not None:
                o = other["per_frame"][a + i]
                ratio = max(np.abs(r[i, :3] - o[:3]).max() / np.abs(t).max() / (2 * bar * cond * EPS),
                            abs(r[i, 3] - o[3]) / (2 * want * (1e-10 + (P + 8) * 2.0 ** -53) + 2 * cond * EPS * 2 * f))
                worst["other"] = max(worst["other"], ratio)
                if not ratio <= 1.0:
                    fails.append(f"frame {a + i}: the two results differ by {ratio:.3g} bars")
        fitted = np.flatnonzero(fit_status == FITTED)
        want_status = fit_status.copy()
        want_t = np.full((T, 3), np.nan)
        want_t[fitted] = r[fitted, :3]                         # the fill is held to the code's own fitted rows
        if fill and fitted.size:
            want_status[fit_status != FITTED] = FILLED
            want_t[:fitted[0]], want_t[fitted[-1] + 1:] = want_t[fitted[0]], want_t[fitted[-1]]
            for lo, hi in zip(fitted[:-1], fitted[1:]):
                if hi - lo > 1:
                    want_t[lo + 1:hi] = np.linspace(want_t[lo], want_t[hi], hi - lo + 1)[1:-1]
        if not np.array_equal(r[:, 5], want_status):
            fails.append(f"sequence {q}: statuses {r[:, 5].tolist()} against {want_status.tolist()}")
            a += T
            continue
        rest = want_status != FITTED
        got_t, held = r[rest, :3], ~np.isnan(want_t[rest])
        if not (np.array_equal(~np.isnan(got_t), held) and np.array_equal(got_t[held].view(np.int64), want_t[rest][held].view(np.int64))):
            fails.append(f"sequence {q}: the unfitted rows do not hold the bits of numpy.linspace / NaN")
        if not np.isnan(r[rest, 3]).all():
            fails.append(f"sequence {q}: a frame that was not fitted has a reprojection error")
        if seq[q, 0] != fitted.size or seq[q, 1] != (want_status == FILLED).sum():
            fails.append(f"sequence {q}: counts {seq[q, :2]} against {fitted.size}, {(want_status == FILLED).sum()}")
        if fitted.size:
            want = math.fsum(r[fitted, 3]) / fitted.size
            ratio = abs(seq[q, 2] - want) / (want * (1e-10 + (T + 8) * 2.0 ** -53))
            worst["mean"] = max(worst["mean"], ratio)
            if not ratio <= 1.0:
                fails.append(f"sequence {q}: mean reproj {seq[q, 2]!r} against {want!r}")
        elif not np.isnan(seq[q, 2]):
            fails.append(f"sequence {q}: mean reproj {seq[q, 2]!r} without a fitted frame")
        pos = j3[a:a + T, root] + r[:, :3]
        steps = np.sqrt((np.diff(pos, axis=0) ** 2).sum(axis=1))
        steps = steps[np.isfinite(steps)]
        want = math.fsum(steps)
        if steps.size:
            tol = (T + 8) * 2.0 ** -53 * want + 8 * T * 2.0 ** -53 * np.nanmax(np.abs(pos))
            ratio = abs(seq[q, 3] - want) / tol
            worst["path"] = max(worst["path"], ratio)
            if not ratio <= 1.0:
                fails.append(f"sequence {q}: path {seq[q, 3]!r} against {want!r}: {ratio:.3g} bars")
        elif seq[q, 3] != 0.0:
            fails.append(f"sequence {q}: path {seq[q, 3]!r} without a step")
        a += T
    return fails, worst
