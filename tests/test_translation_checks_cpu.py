"""tests/helpers/translation_checks.py, the exact-arithmetic checker of the camera-space translation, against
tests/golden/translation.npz: the translations the reference's own estimate_translation_np returned in float64 on the same widened float32 inputs
(tools/make_goldens_translation.py).  The exact solution must agree with the reference within ONE bar, cond_2(A) 2^-52 -- the checker does not
round, so the whole error is the reference's -- and the checker must refuse what is wrong: a translation ten bars off, a wrong status, a fill
that is not numpy.linspace's, a reprojection error a part in 1e8 off."""
import os

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import translation_checks as tc


@pytest.fixture(scope="module")
def golden_cases():
    g = np.load(os.path.join(ROOT, "tests", "golden", "translation.npz"))
    cases = []
    for ci in range(len(tc.GOLDEN_CAMERAS)):
        for K in (13, 25):
            name = f"c{ci}_k{K}"
            cases.append((name, g[name + "_joints3d"], g[name + "_joints2d"], g[name + "_camera"], g[name + "_t"]))
    return cases


def test_golden_file_is_what_the_tool_states(golden_cases):
    assert len(golden_cases) == 6
    for (name, j3, j2, cam, t), (size, f, depth) in zip(golden_cases, [c for c in tc.GOLDEN_CAMERAS for _ in range(2)]):
        assert j3.dtype == np.float32 and j2.dtype == np.float32 and t.dtype == np.float64, name
        assert j3.shape == j2.shape and j3.shape[0] == t.shape[0] == 20 and j3.shape[1] in (13, 25), name
        assert cam[0] == size and cam[1] == f, name
        assert depth[0] * 0.95 <= t[:, 2].min() and t[:, 2].max() <= depth[1] * 1.05, name
        conf = j2[:, :, 2]
        assert (conf == 0).any() and ((conf == 0) | ((conf > 0.05) & (conf < 1))).all(), name


def test_exact_solution_agrees_with_the_reference(golden_cases):
    worst, worst_cond, frames = 0.0, 0.0, 0
    for name, j3, j2, (size, f), t_ref in golden_cases:
        S, D = tc.widen(j3), tc.widen(j2)
        for i in range(S.shape[0]):
            status, n_used, t, cond = tc.frame_truth(S[i], D[i], f, size / 2, size / 2, 0.0, 4)
            assert status == tc.FITTED and n_used == (D[i, :, 2] > 0).sum(), (name, i)
            assert cond <= tc.MAX_COND, (name, i, cond)
            ratio = np.abs(t - t_ref[i]).max() / np.abs(t).max() / (cond * tc.EPS)
            worst, worst_cond, frames = max(worst, ratio), max(worst_cond, cond), frames + 1
    print(f"{frames} frames: the reference is within {worst:.3g} of the bar; largest cond {worst_cond:.3e}")
    assert worst <= 1.0 and frames == 120


def exact_result(j3, j2, pairs, f, centre, threshold=0.0):
    """A result made of the exact translations: what compare() must accept."""
    S, D = tc.widen(j3), tc.widen(j2)
    n = S.shape[0]
    rows = np.full((n, 6), np.nan)
    for i in range(n):
        status, n_used, t, _ = tc.frame_truth(S[i, pairs[:, 0]], D[i, pairs[:, 1]], f, centre[0], centre[1], threshold, 4)
        rows[i, 4], rows[i, 5] = n_used, status
        if status == tc.FITTED:
            rows[i, :3] = t
            rows[i, 3] = tc.exact_reproj(S[i, pairs[:, 0]], D[i, pairs[:, 1]], tc.used_pairs(D[i, pairs[:, 1]], threshold), t, f, *centre)
    return rows


def test_compare_accepts_the_exact_result_and_refuses_wrong_ones(golden_cases):
    name, j3, j2, (size, f), _ = golden_cases[3]
    j2 = j2.copy()
    j2[5:8, :, 2] = 0.0                                         # an inner run of three unfitted frames
    j2[0, :, 2] = 0.0                                           # and one at the front
    pairs = np.stack([np.arange(25)] * 2, axis=1)
    centre = (size / 2, size / 2)
    rows = exact_result(j3, j2, pairs, f, centre)
    assert rows[:, 5].tolist() == [1] + [0] * 4 + [1] * 3 + [0] * 12
    fitted = rows[:, 5] == 0
    rows[0, :3] = rows[1, :3]
    rows[5:8, :3] = np.linspace(rows[4, :3], rows[8, :3], 5)[1:-1]
    rows[~fitted, 5] = tc.FILLED
    pos = tc.widen(j3)[:, 0] + rows[:, :3]
    seq = np.array([[16, 4, rows[fitted, 3].mean(), np.sqrt((np.diff(pos, axis=0) ** 2).sum(1)).sum()]])
    kw = dict(focal_length=f, centre=centre, conf_threshold=0.0)
    fails, worst = tc.compare({"per_frame": rows, "per_sequence": seq}, j3, j2, pairs, **kw)
    print({k: float(f"{v:.3g}") for k, v in worst.items()})
    assert fails == [] and worst["t"] < 1e-3 and worst["reproj"] < 0.01

    def refused(change, word):
        r, s = rows.copy(), seq.copy()
        change(r, s)
        found, _ = tc.compare({"per_frame": r, "per_sequence": s}, j3, j2, pairs, **kw)
        assert any(word in line for line in found), (word, found)
    cond = tc.frame_truth(tc.widen(j3)[2], tc.widen(j2)[2], f, *centre, 0.0, 4)[3]
    refused(lambda r, s: r.__setitem__((2, 2), r[2, 2] * (1 + 10 * cond * tc.EPS)), "t off")
    refused(lambda r, s: r.__setitem__((2, 3), r[2, 3] * (1 + 1e-8)), "reproj")
    refused(lambda r, s: r.__setitem__((6, 5), tc.TOO_FEW), "statuses")
    refused(lambda r, s: r.__setitem__((6, 0), np.nextafter(r[6, 0], np.inf)), "numpy.linspace")
    refused(lambda r, s: r.__setitem__((0, 1), np.nextafter(r[0, 1], np.inf)), "numpy.linspace")
    refused(lambda r, s: r.__setitem__((6, 3), 1.0), "was not fitted")
    refused(lambda r, s: r.__setitem__((3, 4), 3.0), "n_used")
    refused(lambda r, s: s.__setitem__((0, 1), 3.0), "counts")
    refused(lambda r, s: s.__setitem__((0, 2), s[0, 2] * (1 + 1e-8)), "mean reproj")
    refused(lambda r, s: s.__setitem__((0, 3), s[0, 3] * (1 + 1e-9)), "path")
