#!/usr/bin/env python3
"""Golden vectors for the box from 2D joints, produced by RUNNING the reference's own get_bbox_from_joints2d
(batch_generation.py:39-93) through the real sklearn.  Writes tests/golden/bbox_joints2d.npz; only data, no reference source.

Two things stand between the reference and a run here:

  * batch_generation.py does not compile as shipped (`keyword argument repeated: seqlen`, line 206), but it parses.  This tool parses the file,
    takes the FunctionDef of get_bbox_from_joints2d ALONE and compiles it in a namespace that holds np, copy and the module constants
    N = 25, MIN_PIXEL = 500, BS = 1.8 -- the only names the function reads.
  * the `kmedoids` package is absent.  A stand-in module in sys.modules provides fasterpam(diss, 1, ...): the float64 argmin of the row sums of
    the matrix it is handed, lowest index on ties -- the fixed point of the real one with a single medoid (DESIGN 4.7 argues why).  Everything
    else -- the score rule, the head margin, sklearn's euclidean_distances over the three float32 columns, the medians, the aspect rule -- runs
    as the reference wrote it.

Per case: the (T,25,3) float64 input, the reference's (T,4) output, the medoid's index, the float64 cost of every point (T <= 41 only) and the
gap (c2 - c1) / c1 between the medoid and the best point with other (x, y) (tests/helpers/bbox_checks.py).  A case whose gap is below 1e-5, ten
times the bound the GPU's choice is held to, is refused: change its seed, not the bar."""
import argparse
import ast
import copy
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import bbox_checks as bc  # noqa: E402

MIN_GAP = 1e-5

# a standing body of 25 joints in units of its height: (x, y) around the pelvis, y down
BODY = np.array([[0.00, -0.45], [0.00, -0.35], [-0.10, -0.35], [-0.13, -0.18], [-0.14, -0.02], [0.10, -0.35], [0.13, -0.18], [0.14, -0.02],
                 [0.00, 0.00], [-0.06, 0.00], [-0.07, 0.24], [-0.07, 0.47], [0.06, 0.00], [0.07, 0.24], [0.07, 0.47], [-0.02, -0.47],
                 [0.02, -0.47], [-0.04, -0.46], [0.04, -0.46], [0.09, 0.50], [0.11, 0.49], [0.06, 0.49], [-0.09, 0.50], [-0.11, 0.49],
                 [-0.06, 0.49]])

# name: (T, seed, body height in pixels, a frame whose scores are all below the threshold or None)
CASES = {
    "t1": (1, 1, 620.0, None),
    "t2": (2, 2, 620.0, None),           # even T: the median is the mean of the two heights
    "t11": (11, 3, 620.0, None),         # odd T
    "t41": (41, 11, 620.0, None),
    "t400": (400, 14, 620.0, None),     # seeds 4 and 5 gave gaps of 2.2e-5 and 3.3e-6: changed, as the rule above says
    "allbelow": (12, 6, 620.0, 7),       # frame 7: every score below 0.1 -- all 25 joints become its best one
    "small": (9, 7, 300.0, None),        # median(h) * 1.1 < 500: the BS branch
}


def make_case(T, seed, height, dead_frame):
    """Gait-like joints: the body drifts across a 1920 x 1080 frame with a sway and per-joint jitter; uniform scores, about one in eight below 0.1."""
    g = np.random.Generator(np.random.Philox(key=[2025, seed]))
    t = np.arange(T, dtype=np.float64)
    cx = 400.0 + (1100.0 / max(T - 1, 1)) * t + g.uniform(-3, 3, T)
    cy = 540.0 + 12.0 * np.sin(t * 0.55) + g.uniform(-2, 2, T)
    kp = np.empty((T, 25, 3))
    kp[:, :, 0] = cx[:, None] + BODY[None, :, 0] * height + g.normal(0.0, 4.0, (T, 25))
    kp[:, :, 1] = cy[:, None] + BODY[None, :, 1] * height + g.normal(0.0, 4.0, (T, 25))
    s = g.uniform(0.1, 1.0, (T, 25))
    low = g.uniform(0.0, 1.0, (T, 25)) < 0.125
    kp[:, :, 2] = np.where(low, g.uniform(0.0, 0.1, (T, 25)), s)
    if dead_frame is not None:
        kp[dead_frame, :, 2] = g.uniform(0.0, 0.099, 25)
    return kp


def reference_function(reference):
    """get_bbox_from_joints2d compiled from the reference's own text, and the list the stand-in fasterpam appends the matrices' argmins to."""
    path = os.path.join(reference, "batch_generation.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_bbox_from_joints2d"]
    assert len(fn) == 1
    chosen = []

    def fasterpam(diss, medoids, max_iter=100, **kw):
        assert medoids == 1 and diss.ndim == 2 and diss.shape[0] == diss.shape[1]
        chosen.append(int(np.argmin(np.asarray(diss).sum(axis=1, dtype=np.float64))))
        return types.SimpleNamespace(medoids=np.array([chosen[-1]]))

    stand_in = types.ModuleType("kmedoids")
    stand_in.fasterpam = fasterpam
    sys.modules["kmedoids"] = stand_in
    ns = {"np": np, "copy": copy, "N": 25, "MIN_PIXEL": 500, "BS": 1.8}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["get_bbox_from_joints2d"], chosen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GRNET_REFERENCE", "/root/reference"), help="a checkout of the reference")
    a = ap.parse_args()
    fn, chosen = reference_function(a.reference)
    out = {}
    for name, (T, seed, height, dead) in CASES.items():
        kp = make_case(T, seed, height, dead)
        bbox = fn(kp.copy(), smooth=False)
        assert bbox.shape == (T, 4) and bbox.dtype == np.float64
        points, h = bc.prepare(kp)
        costs = bc.row_costs(points)
        m, gap = chosen[-1], bc.gap(points, costs)
        if gap < MIN_GAP:
            raise SystemExit(f"case {name}: gap {gap:.3e} < {MIN_GAP:g}: change its seed")
        exact = bc.medoid(points, costs)
        assert tuple(points[m, :2]) == tuple(points[exact, :2]) == tuple(bbox[0, :2].astype(np.float32)), name
        if dead is not None:
            assert (kp[dead, :, 2] < 0.1).all()
        small = np.median(h) * 1.1 < 500
        assert small == (name == "small"), (name, np.median(h))
        out[name + "_kp"], out[name + "_bbox"], out[name + "_medoid"], out[name + "_gap"] = kp, bbox, np.int64(m), np.float64(gap)
        if T <= 41:
            out[name + "_cost"] = costs
        print(f"{name:9s} T {T:4d}  medoid {m:5d}  gap {gap:.3e}  box {bbox[0]}  BS branch {bool(small)}")
    path = os.path.join(ROOT, "tests", "golden", "bbox_joints2d.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
