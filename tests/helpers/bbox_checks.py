"""Float64 restatement of the box from 2D joints (batch_generation.py:39-93), for the tests and the golden tool: the frame rule, the cost of
a row of the 1-medoid, and the gap between the medoid and the best point that would give another centre.  Plain numpy; nothing of the package."""
import numpy as np


def prepare(kp_2d, threshold=0.1):
    """(T,K,3) float64 -> (the T K float32 points (x, y, s) the medoid is taken over, h (T,) float64): joints whose score is below the threshold take
    the frame's first joint of highest score; h = lr_y - ul_y after ul_y -= (lr_y - ul_y) * 0.10."""
    kp = np.array(kp_2d, dtype=np.float64)
    assert kp.ndim == 3 and kp.shape[2] == 3
    for t in range(kp.shape[0]):
        bad = kp[t, :, 2] < threshold
        kp[t, bad] = kp[t, int(np.argmax(kp[t, :, 2]))]
    ul_y, lr_y = kp[:, :, 1].min(axis=1), kp[:, :, 1].max(axis=1)
    ul_y = ul_y - (lr_y - ul_y) * 0.10
    return kp.reshape(-1, 3).astype(np.float32), lr_y - ul_y


def row_cost(points, i):
    """sum_j |p_i - p_j| in float64 over float32 points (n, >= 3): the first three columns count."""
    p = np.asarray(points)[:, :3].astype(np.float64)
    return float(np.sqrt(((p - p[i]) ** 2).sum(axis=1)).sum())


def row_costs(points, block=256):
    """Every row's cost, in row blocks so that no n x n array is formed."""
    cols = np.ascontiguousarray(np.asarray(points)[:, :3].astype(np.float64).T)
    out = np.empty(cols.shape[1])
    for a in range(0, cols.shape[1], block):
        d2 = sum((c[a:a + block, None] - c[None, :]) ** 2 for c in cols)
        out[a:a + block] = np.sqrt(d2).sum(axis=1)
    return out


def medoid(points, costs=None):
    """The row of least float64 cost, lowest index on ties."""
    return int(np.argmin(row_costs(points) if costs is None else costs))


def gap(points, costs=None):
    """(c2 - c1) / c1: c1 the medoid's cost, c2 the least cost among points whose (x, y) differs from the medoid's -- copies of the medoid (replaced
    joints) tie exactly, give the same centre and do not count.  inf when every point has the medoid's (x, y)."""
    p = np.asarray(points)
    costs = row_costs(p) if costs is None else np.asarray(costs)
    m = int(np.argmin(costs))
    other = (p[:, 0] != p[m, 0]) | (p[:, 1] != p[m, 1])
    if not other.any():
        return float("inf")
    return float((costs[other].min() - costs[m]) / costs[m])


def expected_box(kp_2d, threshold=0.1):
    """[cx, cy, nw, nh] float64 from the pieces above: the float32 medoid's (x, y) widened; nw = nh = median(h) * 1.1, times 1.8 below 500."""
    points, h = prepare(kp_2d, threshold)
    m = medoid(points)
    nh = np.median(h) * 1.1
    if nh < 500:
        nh = nh * 1.8
    return np.array([points[m, 0], points[m, 1], nh, nh], np.float64)
