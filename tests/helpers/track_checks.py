"""The bars of the per-frame boxes from 2D joints, shared by the host and the GPU tests.  The expected values are the golden file's:
what the reference's lib/utils/smooth_bbox.py returned for the stored inputs (tools/make_goldens_track.py).  u = 2^-53.

  stages 1 + 2  range and status equal; cx and cy BIT-IDENTICAL (min, max, one add, one halving; the fill is numpy.linspace's own arithmetic);
                the scale within 8 u relative: each side forms the height with at most three roundings and the quotient with one, so two correct
                implementations differ by at most 8 u; an interpolated scale is held to 8 u of the larger of its two detected neighbours.
  median        bit-identical to the golden's, given the golden's stage-2 column: a selection has no arithmetic.
  Gaussian      within (2 r + 8) u max|x| of the golden's, given the golden's median column: one rounding per term of the sum of 2 r + 1 products
                plus the weights' own roundings; max|x| over the reflected window is the column's.
  the chain     cx and cy reach the Gaussian with identical bits, so they are held to the Gaussian's bar; the scale column enters it up to 8 u of
                its largest value off (a selection passes that on unchanged, a sum of weights that add up to 1 does not enlarge it).
A device box holds 150 / scale, not the scale: one more rounding, u relative, which the functions below add where they are handed a box (the
comparison itself is exact, in Fractions)."""
import os
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
U = 2.0 ** -53
VIS_THRESH, KERNEL = 0.3, 11
CASES = ("t1", "t2", "t5", "t12", "t26gaps", "t70", "dead", "point")
FRAMES = {"t1": 1, "t2": 2, "t5": 5, "t12": 12, "t26gaps": 26, "t70": 70, "dead": 8, "point": 6}


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "track_boxes.npz"))


def detected(kp, vis_thresh=VIS_THRESH):
    """The frames kp_to_bbox_param returns a box for, by its own text: a visible joint and a norm of at least 0.5."""
    out = np.zeros(kp.shape[0], bool)
    for i, f in enumerate(kp):
        vis = f[:, 2] > vis_thresh
        out[i] = vis.any() and np.linalg.norm(f[vis, :2].max(axis=0) - f[vis, :2].min(axis=0)) >= 0.5
    return out


def expected_status(kp, start, end, scale=None):
    """0 / 1 inside [start, end) by detection, 2 outside; 3 where a smoothed scale is given and is not positive and finite."""
    st = np.full(kp.shape[0], 2, np.int32)
    if start >= 0:
        st[start:end] = np.where(detected(kp)[start:end], 0, 1)
        if scale is not None:
            st[start:end][~((scale > 0) & np.isfinite(scale))] = 3
    return st


def neighbour_scale(det, scale):
    """Per frame of [start, end): the larger scale of the detected frames on either side (its own where it is detected)."""
    idx = np.flatnonzero(det)
    out = np.empty(det.size)
    for i in range(det.size):
        lo, hi = idx[idx <= i].max(), idx[idx >= i].min()
        out[i] = max(scale[lo], scale[hi])
    return out


def worst_scale_ratio(got, want, allowed_abs, is_side):
    """max |got - want| / allowed, exactly.  is_side: got is 150 / scale (a box side), held to the same relative bar plus its quotient's u."""
    worst = 0.0
    for g, w, a in zip(got, want, allowed_abs):
        g, w = Fraction(float(g)), Fraction(float(w))
        if is_side:
            w, rel = Fraction(150) / w, Fraction(float(a)) / w + Fraction(U)
            worst = max(worst, float(abs(g - w) / (rel * w)))
        else:
            worst = max(worst, float(abs(g - w) / Fraction(float(a))) if a > 0 else (0.0 if g == w else np.inf))
    return worst


def check_unsmoothed(out, g, name, a=0):
    """out of track_boxes(kernel_size=1, sigma=0) for frames [a, a + T) of a call against get_all_bbox_params; returns the scale's worst ratio."""
    kp, params = g[name + "_kp"], g[name + "_params"]
    start, end = (int(v) for v in g[name + "_range"])
    T = kp.shape[0]
    boxes, status = np.asarray(out["boxes"])[a:a + T], np.asarray(out["status"])[a:a + T]
    assert status.tolist() == expected_status(kp, start, end).tolist(), name
    outside = status == 2
    assert (boxes[outside] == 0).all(), name
    if start < 0:
        return 0.0
    inside = boxes[start:end]
    assert np.array_equal(inside[:, :2].view(np.int64), params[:, :2].view(np.int64)), f"{name}: a centre differs in some bit"
    assert np.array_equal(inside[:, 2], inside[:, 3])
    allowed = 8 * U * neighbour_scale(detected(kp)[start:end], params[:, 2])
    if "params" in out:
        scale = np.asarray(out["params"])[a + start:a + end, 2]
        return max(worst_scale_ratio(scale, params[:, 2], allowed, False), worst_scale_ratio(inside[:, 2], params[:, 2], allowed, True))
    return worst_scale_ratio(inside[:, 2], params[:, 2], allowed, True)


def gauss_bar(column, sigma):
    return (2 * int(4.0 * sigma + 0.5) + 8) * U * np.abs(column).max()


def check_smoothed(out, g, name, a=0):
    """out of track_boxes(kernel_size=11, sigma of the case, pad zero) against smooth_bbox_params; returns the worst ratio to the chain's bar."""
    kp, params, median, smooth, sigma = g[name + "_kp"], g[name + "_params"], g[name + "_median"], g[name + "_smooth"], float(g[name + "_sigma"])
    start, end = (int(v) for v in g[name + "_range"])
    T = kp.shape[0]
    boxes, status = np.asarray(out["boxes"])[a:a + T], np.asarray(out["status"])[a:a + T]
    assert status.tolist() == expected_status(kp, start, end, smooth[:, 2]).tolist(), name
    assert (boxes[status >= 2] == 0).all(), name
    inside, ok = boxes[start:end], status[start:end] < 2
    worst = 0.0
    for c in (0, 1):
        if ok.any():
            worst = max(worst, np.abs(inside[ok, c] - smooth[ok, c]).max() / gauss_bar(median[:, c], sigma))
    allowed = np.full(int(ok.sum()), gauss_bar(median[:, 2], sigma) + 8 * U * np.abs(params[:, 2]).max())
    if ok.any():
        worst = max(worst, worst_scale_ratio(inside[ok, 2], smooth[ok, 2], allowed, True))
    return float(worst)
