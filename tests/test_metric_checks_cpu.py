"""tests/helpers/metric_checks.py, the yardstick of the pose metrics, on cases worked by hand: a unit square turned, scaled and
shifted; a parabola of three frames; the NaN structure of short sequences; means from sums and counts; what the certificate accepts and refuses."""
import numpy as np
import pytest

from .helpers import metric_checks as mc


def test_square_turned_scaled_and_shifted():
    """gt = 2 Q p + (1, 2, 3), Q a quarter turn about z: pa_mpjpe = 0, the transform is (2, Q, (1, 2, 3)), mpjpe in closed form."""
    p = np.array([[[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]], np.float32)
    Q = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    g = (2.0 * p[0] @ Q.T + np.array([1.0, 2.0, 3.0]))[None].astype(np.float32)
    assert np.array_equal(g[0], np.array([[1, 2, 3], [1, 4, 3], [-1, 4, 3], [-1, 2, 3]], np.float32))
    pf, ps, total, aux = mc.expected(p, g, unit=1.0)
    assert pf[0, 0] == pytest.approx((np.sqrt(14) + 5 + np.sqrt(22) + np.sqrt(11)) / 4, rel=1e-15)
    assert abs(pf[0, 1]) <= 1e-14
    assert np.isnan(pf[0, 2:]).all() and np.array_equal(np.isnan(ps), np.isnan(pf)) and np.array_equal(np.isnan(total), np.isnan(pf[0]))
    tf = aux["transform"][0]
    assert tf[0] == pytest.approx(2.0, rel=1e-14) and np.allclose(tf[1:10].reshape(3, 3), Q, atol=1e-14) and np.allclose(tf[10:], [1, 2, 3], atol=1e-14)
    assert mc.certificate(aux["K"][0], tf[1:10]) == []
    assert mc.objective_error(tf, aux["P"][0], aux["G"][0], aux["K"][0], aux["var1"][0], aux["x2"][0]) <= 1e-14
    assert aux["gap"][0] == pytest.approx(1.0)                 # planar square: singular values 2, 2, 0
    # the unit multiplies every metric
    assert mc.expected(p, g, unit=1000.0)[0][0, 0] == pytest.approx(1000.0 * pf[0, 0], rel=1e-15)


def test_parabola_has_a_known_acceleration():
    """P[f] = f^2 a_j + f b (root-free): the second difference is 2 a_j at the middle frame; gt moves linearly, so accel_err = accel."""
    a = np.array([[0.5, 0, 0], [0, 0.25, 0], [0, 0, 2.0]])
    pred = np.stack([f * f * a + f * np.array([1.0, 1.0, 1.0]) for f in range(3)]).astype(np.float32)
    gt = np.stack([np.full((3, 3), 0.5 * f) for f in range(3)]).astype(np.float32)
    pf, ps, total, _ = mc.expected(pred, gt, unit=1.0)
    want = (1.0 + 0.5 + 4.0) / 3
    assert pf[1, 3] == want and pf[1, 4] == want
    assert np.isnan(pf[[0, 2], 3:]).all()
    assert ps[0, 3] == want and total[4] == want
    # with a root the motion of that joint leaves every joint: joint 0 becomes still
    pf, _, _, _ = mc.expected(pred, gt, root=[0], unit=1.0)
    assert pf[1, 3] == pytest.approx((0.0 + np.linalg.norm([-1.0, 0.5, 0]) + np.linalg.norm([-1.0, 0, 4.0])) / 3, rel=1e-15)


def test_structure_of_short_sequences_and_means():
    lengths = [1, 2, 3, 5]
    pred, gt = mc.random_case(11, 14, 5)
    pf, ps, total, _ = mc.expected(pred, gt, lengths=lengths, root=[2, 3])
    assert np.array_equal(~np.isnan(pf), mc.structure(lengths, False))
    assert np.flatnonzero(~np.isnan(pf[:, 3])).tolist() == [4, 7, 8, 9]
    assert np.isnan(ps[:2, 3:]).all() and not np.isnan(ps[2:, 3:]).any() and np.isnan(ps[:, 2]).all()
    assert ps[3, 0] == pytest.approx(pf[6:, 0].mean(), rel=1e-15) and ps[3, 3] == pytest.approx(pf[7:10, 3].mean(), rel=1e-15)
    assert total[0] == pytest.approx(pf[:, 0].mean(), rel=1e-15) and total[4] == pytest.approx(pf[[4, 7, 8, 9], 4].mean(), rel=1e-15)
    assert np.isnan(total[2])
    v = np.random.Generator(np.random.Philox(key=[1, 2])).normal(size=(11, 7, 3)).astype(np.float32)
    pf, _, total, _ = mc.expected(pred, gt, lengths=lengths, pred_verts=v, gt_verts=v + np.float32(0.5), unit=1.0)
    assert np.allclose(pf[:, 2], 0.5 * np.sqrt(3), rtol=1e-6) and not np.isnan(total[2])


def test_one_joint_takes_the_stated_rule():
    pred, gt = mc.random_case(3, 1, 9)
    pf, _, _, aux = mc.expected(pred, gt)
    assert (aux["var1"] == 0).all() and (pf[:, 1] == 0).all()
    assert np.array_equal(aux["transform"][:, :10], np.tile(np.concatenate([[0.0], np.eye(3).reshape(9)]), (3, 1)))
    assert np.array_equal(aux["transform"][:, 10:], mc.widen(gt)[:, 0])


def test_certificate_accepts_maximisers_and_refuses_the_rest():
    I = np.eye(3)
    assert mc.certificate(np.diag([2.0, 1.0, -1.0]), I) == []               # s1 + s2 - s3 is the most a proper rotation reaches
    assert mc.certificate(np.diag([2.0, 1.0, 0.0]), I) == []
    assert mc.certificate(np.zeros((3, 3)), I) == []
    assert mc.certificate(np.diag([1.0, -2.0, 0.5]), I)                       # a half turn about x reaches 1 + 2 - 0.5
    assert mc.certificate(np.diag([1.0, -2.0, 0.5]), np.diag([1.0, -1.0, -1.0])) == []
    assert mc.certificate(np.diag([2.0, 1.0, -1.0]), np.diag([1.0, 1.0, -1.0]))      # a reflection: det < 0
    assert mc.certificate(np.diag([2.0, 1.0, 1.0]), 1.001 * I)                # not orthogonal
    c, s = np.cos(0.3), np.sin(0.3)
    assert mc.certificate(np.diag([2.0, 1.0, 1.0]), np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]))      # orthogonal, but R K is not symmetric
    # a random K: numpy's SVD passes, a slightly turned R does not
    K = np.random.Generator(np.random.Philox(key=[4, 4])).normal(size=(3, 3))
    U, S, Vt = np.linalg.svd(K)
    R = Vt.T @ np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))]) @ U.T
    assert mc.certificate(K, R) == []
    assert mc.certificate(K, np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ R)
