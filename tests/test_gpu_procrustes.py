"""The Procrustes rotation on the device alone (grnet_op_procrustes -> procrustes3() of csrc/procrustes3.h) on exact matrices -- zero,
rank 1, rank 2, diag(1, 1, 1), diag(2, 1, -1), repeated singular values, 1e-30 and 1e+30 scalings -- and 1000 seeded random ones: every returned R
passes the certificate of tests/helpers/metric_checks.py, which trusts no SVD; the zero matrix, for which any proper rotation would pass, also
returns R = I, the rule DESIGN 4.8 states for var1 == 0; the singular values are those of numpy to 1e-12 of the largest."""
import numpy as np
import pytest
import torch

from .helpers import metric_checks as mc

pytestmark = pytest.mark.gpu

EXACT = {
    "zero": np.zeros((3, 3)),
    "rank 1": np.outer([1.0, 2.0, 3.0], [1.0, 2.0, 3.0]),
    "rank 1, one entry": np.array([[0.0, 0, 0], [0, 0, -5.0], [0, 0, 0]]),
    "rank 2": np.diag([3.0, 2.0, 0.0]),
    "rank 2, reflection in the plane": np.array([[1.0, 1, 0], [1, -1, 0], [0, 0, 0]]),
    "diag(1,1,1)": np.eye(3),
    "diag(2,1,-1)": np.diag([2.0, 1.0, -1.0]),
    "-I": -np.eye(3),
    "repeated sigma": np.array([[0.0, 2, 0], [-2, 0, 0], [0, 0, 1]]),
    "dense": np.array([[0.3, -1.2, 0.7], [2.1, 0.4, -0.9], [-0.6, 1.5, 0.8]]),
}


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.GRNet(max_frames=1)                               # no weights: the hook needs none
    yield m
    m.close()


def check(model, Ks, names):
    R, sigma = model.op_procrustes(Ks)
    assert R.dtype == sigma.dtype == torch.float64 and tuple(R.shape) == (len(Ks), 3, 3) and tuple(sigma.shape) == (len(Ks), 3)
    R, sigma = R.cpu().numpy(), sigma.cpu().numpy()
    failures, worst = [], 0.0
    for K, r, s, name in zip(Ks, R, sigma, names):
        failures += [f"{name}: {w}" for w in mc.certificate(K, r)]
        want = np.linalg.svd(K, compute_uv=False)
        err = np.abs(s - want).max() / max(want[0], 1e-300)
        worst = max(worst, err)
        if not (s[0] >= s[1] >= s[2] >= 0 and err <= 1e-12):
            failures.append(f"{name}: singular values {s} against {want}")
    print(f"{len(Ks)} matrices, worst singular value error {worst:.2e} of the largest")
    assert not failures, failures[:10]
    return R


def test_exact_matrices(model):
    names = list(EXACT)
    Ks = [EXACT[k] for k in names]
    for k in ("rank 1", "rank 2", "diag(1,1,1)", "diag(2,1,-1)", "repeated sigma", "dense"):
        for f in (1e-30, 1e+30):
            names.append(f"{k} x {f:g}")
            Ks.append(EXACT[k] * f)
    R = check(model, np.stack(Ks), names)
    assert np.array_equal(R[0], np.eye(3))                     # K = 0: R = I
    assert np.array_equal(R[names.index("diag(2,1,-1)")], np.eye(3)) and np.array_equal(R[names.index("diag(1,1,1)")], np.eye(3))


def test_one_matrix_and_a_thousand_random_ones(model):
    check(model, EXACT["dense"][None], ["dense"])
    g = np.random.Generator(np.random.Philox(key=[41, 1000]))
    Ks = g.normal(size=(1000, 3, 3))
    Ks[::7] *= 10.0 ** g.uniform(-30, 30, (len(Ks[::7]), 1, 1))
    Ks[3::10, :, 2] = Ks[3::10, :, 0] * 0.5 - Ks[3::10, :, 1]                   # rank 2
    Ks[5::10] = np.einsum("ni,nj->nij", Ks[5::10, :, 0], Ks[5::10, 0, :])      # rank 1
    check(model, Ks, [f"random {i}" for i in range(1000)])
