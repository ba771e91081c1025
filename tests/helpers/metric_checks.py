"""The yardstick of the pose metrics: a float64 numpy statement, one frame at a time, written independently of
pipeline.pose_metrics -- it imports nothing from the package -- and a certificate for the Procrustes alignment that trusts no SVD.

expected(...)          every output of the definition for a call, plus per frame the matrix K, var1, |X2|^2, the aligned joints P, G and
                       gap = (s2 + sign s3) / s1, the conditioning of the rotation
certificate(K, R)      [] or the list of what fails: |R^T R - I|_inf <= 1e-12, det R > 0, M = R K symmetric to 1e-12 |K|, the eigenvalues
                       of M (numpy eigvalsh of the symmetrised M) l1 >= l2 >= |l3| and l2 + l3 >= -1e-12 |K|.  A proper rotation maximises
                       trace(R K) exactly when it passes.
objective_error(...)   the objective sum |s R p + t - g|^2 recomputed from a returned (s, R, t) against |X2|^2 - trace(R K)^2 / var1,
                       relative; the minimum is unique even where R is not
"""
import numpy as np

ORTH_TOL = 1e-12
SYM_TOL = 1e-12
OBJECTIVE_REL = 1e-10
GAP_MIN = 1e-3


def widen(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def align(joints, root, select):
    """(n,J,3) -> the selected joints (n,m,3) after the frame's root mean has been subtracted."""
    j = widen(joints)
    if root is not None and len(root):
        out = np.empty_like(j)
        for f in range(j.shape[0]):
            centre = np.zeros(3)
            for k in root:
                centre = centre + j[f, k]
            out[f] = j[f] - centre / len(root)
        j = out
    return j if select is None else j[:, list(select)]


def frame_procrustes(P, G):
    """One frame: (s, R, t, K, var1, |X2|^2, gap) by the textbook formula with numpy's SVD; var1 == 0: s = 0, R = I."""
    mu1, mu2 = P.mean(axis=0), G.mean(axis=0)
    X1, X2 = (P - mu1).T, (G - mu2).T
    var1 = float((X1 * X1).sum())
    K = X1 @ X2.T
    U, S, Vt = np.linalg.svd(K)
    sign = 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0
    gap = (S[1] + sign * S[2]) / S[0] if S[0] > 0 else 0.0
    if var1 == 0.0:
        return 0.0, np.eye(3), mu2.copy(), K, var1, float((X2 * X2).sum()), gap
    R = Vt.T @ np.diag([1.0, 1.0, sign]) @ U.T
    s = float(np.trace(R @ K)) / var1
    return s, R, mu2 - s * (R @ mu1), K, var1, float((X2 * X2).sum()), gap


def expected(pred, gt, lengths=None, root=None, select=None, pred_verts=None, gt_verts=None, unit=1000.0):
    P, G = align(pred, root, select), align(gt, root, select)
    n = P.shape[0]
    lengths = [n] if lengths is None else list(lengths)
    assert sum(lengths) == n
    per_frame = np.full((n, 5), np.nan)
    aux = {"K": np.zeros((n, 3, 3)), "var1": np.zeros(n), "x2": np.zeros(n), "gap": np.zeros(n), "P": P, "G": G, "transform": np.zeros((n, 13))}
    for f in range(n):
        per_frame[f, 0] = np.mean([np.sqrt(((P[f, j] - G[f, j]) ** 2).sum()) for j in range(P.shape[1])])
        s, R, t, K, var1, x2, gap = frame_procrustes(P[f], G[f])
        moved = s * (P[f] @ R.T) + t
        per_frame[f, 1] = np.mean(np.sqrt(((moved - G[f]) ** 2).sum(axis=1)))
        aux["K"][f], aux["var1"][f], aux["x2"][f], aux["gap"][f] = K, var1, x2, gap
        aux["transform"][f] = np.concatenate([[s], R.reshape(9), t])
    if pred_verts is not None:
        pv, gv = widen(pred_verts), widen(gt_verts)
        per_frame[:, 2] = np.sqrt(((pv - gv) ** 2).sum(axis=2)).mean(axis=1)
    a = 0
    for T in lengths:
        for f in range(a + 1, a + T - 1):
            acc = P[f - 1] - 2.0 * P[f] + P[f + 1]
            err = (P[f - 1] - G[f - 1]) - 2.0 * (P[f] - G[f]) + (P[f + 1] - G[f + 1])
            per_frame[f, 3] = np.sqrt((acc ** 2).sum(axis=1)).mean()
            per_frame[f, 4] = np.sqrt((err ** 2).sum(axis=1)).mean()
        a += T
    per_frame = per_frame * unit
    per_seq, sums, counts = np.full((len(lengths), 5), np.nan), np.zeros(5), np.zeros(5)
    a = 0
    for q, T in enumerate(lengths):
        for c in range(5):
            vals = [v for v in per_frame[a:a + T, c] if not np.isnan(v)]
            if vals:
                per_seq[q, c] = np.sum(vals) / len(vals)
                sums[c] += np.sum(vals)
                counts[c] += len(vals)
        a += T
    total = np.array([sums[c] / counts[c] if counts[c] else np.nan for c in range(5)])
    return per_frame, per_seq, total, aux


def structure(lengths, has_verts):
    """(n,5) bool: which entries of per_frame are defined by structure."""
    n = sum(lengths)
    d = np.zeros((n, 5), bool)
    d[:, :2] = True
    d[:, 2] = has_verts
    a = 0
    for T in lengths:
        d[a + 1:a + T - 1, 3:] = True
        a += T
    return d


def certificate(K, R):
    K, R = np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3)
    normK = float(np.sqrt((K * K).sum()))
    bad = []
    if not np.isfinite(R).all():
        return ["R is not finite"]
    orth = np.abs(R.T @ R - np.eye(3)).sum(axis=1).max()
    if not orth <= ORTH_TOL:
        bad.append(f"|R^T R - I|_inf = {orth:.3e}")
    if not np.linalg.det(R) > 0:
        bad.append(f"det R = {np.linalg.det(R):.3e}")
    M = R @ K
    asym = np.abs(M - M.T).max()
    if not asym <= SYM_TOL * normK:
        bad.append(f"R K is asymmetric by {asym:.3e} (|K| = {normK:.3e})")
    lam = np.sort(np.linalg.eigvalsh(0.5 * (M + M.T)))[::-1]
    if not (lam[1] - abs(lam[2]) >= -SYM_TOL * normK and lam[1] + lam[2] >= -SYM_TOL * normK):
        bad.append(f"eigenvalues of R K {lam} are not l1 >= l2 >= |l3| with l2 + l3 >= 0")
    return bad


def objective_error(transform, P, G, K, var1, x2):
    """Relative difference between the recomputed objective and |X2|^2 - trace(R K)^2 / var1 (var1 == 0: |X2|^2), on the scale |X2|^2."""
    s, R, t = float(transform[0]), np.asarray(transform[1:10]).reshape(3, 3), np.asarray(transform[10:13])
    got = float((((s * (P @ R.T) + t) - G) ** 2).sum())
    want = x2 - (float(np.trace(R @ K)) ** 2 / var1 if var1 > 0 else 0.0)
    return abs(got - want) / max(x2, 1e-300)


def random_case(n, J, seed, kind="noisy"):
    """Seeded joints in metres.  noisy: gt = a rotated, scaled, shifted pred plus 3 cm of noise; mirrored: gt = pred mirrored in x plus noise
    (the reflection branch); unrelated: two independent point sets."""
    g = np.random.Generator(np.random.Philox(key=[seed, n * 100 + J]))
    pred = g.normal(0.0, 0.4, (n, J, 3))
    pred += np.cumsum(g.normal(0.0, 0.02, (n, 1, 3)), axis=0)                 # a walk of the whole body
    if kind == "unrelated":
        gt = g.normal(0.0, 0.4, (n, J, 3))
    elif kind == "mirrored":
        gt = pred * np.array([-1.0, 1.0, 1.0]) + g.normal(0.0, 0.03, (n, J, 3))
    else:
        q = g.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        Q = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        gt = 1.1 * pred @ Q.T + np.array([0.3, -0.2, 2.5]) + g.normal(0.0, 0.03, (n, J, 3))
    return pred.astype(np.float32), gt.astype(np.float32)


# The bars of DESIGN 4.8, derived there, not measured: differences of widened float32 values are exact or one rounding, a correctly rounded square
# root and a sum of N non-negative terms give (N + 8) 2^-53 relative (7.7e-13 at V = 6890): 1e-11 relative for mpjpe, pve and their means.  The two
# accelerations add 1e-11 x (largest aligned coordinate) x unit absolute for the rounding of the root subtraction under the cancellation of the
# second difference.  pa_mpjpe: the rotation is conditioned like eps / gap, 1e-10 relative for gap >= 1e-3 -- and so are the means of that column,
# which cannot be better than their terms; the means of the acceleration columns keep the accelerations' bar for the same reason.
REL, PA_REL = 1e-11, 1e-10


def loose_frames(aux):
    """Frames whose pa_mpjpe is not compared by value: gap below GAP_MIN with at least three joints.  With one or two joints K has rank <= 1 and
    the gap is 0 by structure, but the aligned joints do not depend on which maximiser R is (they lie on the line R turns onto gt's), so the value
    is as well conditioned as s1's direction and IS compared."""
    return (aux["gap"] < GAP_MIN) & (aux["P"].shape[1] >= 3)


def compare(got, want, aux, unit, lengths, has_verts):
    """got, want: (per_frame, per_sequence, total).  Returns (failures, worst): failures a list of strings, worst the largest error seen per
    column in units of its bar.  Frames whose gap is below GAP_MIN are left out of the pa_mpjpe comparison (the caller certifies them) and the
    pa_mpjpe means of a call that holds one are not compared."""
    failures, worst = [], {}
    coord = max(float(np.abs(aux["P"]).max()), float(np.abs(aux["G"]).max()))
    defined = structure(lengths, has_verts)
    names = ("mpjpe", "pa_mpjpe", "pve", "accel", "accel_err")
    if not np.array_equal(np.isnan(got[0]), ~defined):
        failures.append("per_frame: the NaN pattern is not the structural one")
    loose = loose_frames(aux)
    for label, g, w in (("per_frame", got[0], want[0]), ("per_sequence", got[1], want[1]), ("total", got[2].reshape(1, 5), want[2].reshape(1, 5))):
        if g.shape != w.shape or not np.array_equal(np.isnan(g), np.isnan(w)):
            failures.append(f"{label}: shape or NaN pattern differs")
            continue
        for c, name in enumerate(names):
            rel = PA_REL if c == 1 else REL
            bar = rel * np.abs(w[:, c]) + (REL * coord * abs(unit) if c >= 3 else 0.0)
            if c == 1 and aux["P"].shape[1] <= 2:              # one or two joints: an exact similarity exists, pa_mpjpe is 0 up to rounding
                bar = bar + PA_REL * coord * abs(unit)         # the bound of the exact-similarity property, as for gt = c Q pred + d
            err = np.abs(g[:, c] - w[:, c])
            keep = ~np.isnan(w[:, c])
            if c == 1 and label == "per_frame":
                keep &= ~loose
            elif c == 1 and loose.any():
                continue
            if not keep.any():
                continue
            ratio = float((err[keep] / np.maximum(bar[keep], 1e-300)).max()) if (err[keep] > 0).any() else 0.0
            worst[f"{label}.{name}"] = ratio
            if ratio > 1.0:
                failures.append(f"{label}.{name}: {ratio:.3g} x its bar")
    return failures, worst
