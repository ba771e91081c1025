"""References of the --smooth step (tests/test_smooth_checks_cpu.py, tests/test_gpu_smooth.py).

one_euro_strict_f32 restates lib/utils/one_euro_filter.py:5-46 as lib/utils/smooth_pose.py:52-57,87-92 drives it (float32 arrays,
t_e = 1) with ONE float32 rounding per operation, in the reference's order: it equals tests/golden/one_euro.npz, which the reference
made, bit for bit.  one_euro_fma is the same recurrence with every multiply-add contracted to a fused one, as a compiler is free to
do in device code unless told otherwise; it exists only to prove that the bit-exact checks tell the two apart.
"""
import numpy as np

F = np.float32
TWO_PI = F(2 * np.pi)


def _coef(min_cutoff, beta, d_cutoff):
    r_d = F(2 * np.pi * d_cutoff)
    a_d = F(r_d / F(r_d + F(1)))
    return a_d, F(F(1) - a_d), F(min_cutoff), F(beta)


def one_euro_strict_f32(x, min_cutoff=0.004, beta=0.7, d_cutoff=1.0):
    """x (T, ...) float32 -> filtered (T, ...) float32; every +, -, *, / below is one numpy float32 operation."""
    x = np.asarray(x, F)
    a_d, na_d, mc, be = _coef(min_cutoff, beta, d_cutoff)
    out = np.empty_like(x)
    out[0] = x[0]
    x_prev, dx_prev = x[0].copy(), np.zeros_like(x[0])
    one = F(1)
    for t in range(1, x.shape[0]):
        dx = x[t] - x_prev
        dx_hat = a_d * dx + na_d * dx_prev
        cutoff = mc + be * np.abs(dx_hat)
        r = TWO_PI * cutoff
        a = r / (r + one)
        x_hat = a * x[t] + (one - a) * x_prev
        assert dx_hat.dtype == F and x_hat.dtype == F
        out[t] = x_hat
        x_prev, dx_prev = x_hat, dx_hat
    return out


def _fma(a, b, c):
    """fl32(a * b + c) with a single rounding: the product of two float32 is exact in float64, and the float64 sum is rounded once more
    to float32 (a double rounding that can differ from a true fma only in rare ties -- irrelevant for a demonstration of disagreement)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def one_euro_fma(x, min_cutoff=0.004, beta=0.7, d_cutoff=1.0):
    """The recurrence as a compiler that contracts a * b + c * d into fma(a, b, c * d) evaluates it."""
    x = np.asarray(x, F)
    a_d, na_d, mc, be = _coef(min_cutoff, beta, d_cutoff)
    out = np.empty_like(x)
    out[0] = x[0]
    x_prev, dx_prev = x[0].copy(), np.zeros_like(x[0])
    one = F(1)
    full = lambda v: np.full_like(x_prev, v)
    for t in range(1, x.shape[0]):
        dx = x[t] - x_prev
        dx_hat = _fma(full(a_d), dx, na_d * dx_prev)
        cutoff = _fma(full(be), np.abs(dx_hat), full(mc))
        r = TWO_PI * cutoff
        a = r / (r + one)
        x_hat = _fma(a, x[t], (one - a) * x_prev)
        out[t] = x_hat
        x_prev, dx_prev = x_hat, dx_hat
    return out


def rodrigues_f64(aa):
    """smplx's batch_rodrigues in float64 on the given (float32) input: angle = |aa + 1e-8|, R = I + sin K + (1 - cos) K^2."""
    aa = np.asarray(aa, np.float64).reshape(-1, 3)
    angle = np.linalg.norm(aa + 1e-8, axis=1, keepdims=True)
    d = aa / angle
    K = np.zeros((aa.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    s, c = np.sin(angle)[..., None], np.cos(angle)[..., None]
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K)


def random_walk(T, seed, ld=72, step=0.03):
    """Philox random walk (T,72) with `step`-sized steps from a start of O(1), so that no value is subnormal; with ld = 85 it is laid into
    columns 3..74 of a (T,85) array whose other 13 columns are NaN.  Returns (the (T,72) walk, the array to hand to the device)."""
    g = np.random.Generator(np.random.Philox(key=[seed, T]))
    x = (g.uniform(-1.0, 1.0, (1, 72)) + np.cumsum(g.standard_normal((T, 72)) * step, axis=0)).astype(F)
    if ld == 72:
        return x, x
    full = np.full((T, ld), np.nan, F)
    full[:, 3:75] = x
    return x, full
