#!/usr/bin/env python3
"""Golden vectors for the per-frame boxes from 2D joints, produced by RUNNING the reference's own lib/utils/smooth_bbox.py:
get_all_bbox_params (vis_thresh = 0.3, as lib/dataset/inference.py:57 calls it) and smooth_bbox_params (kernel_size = 11, sigma per case).
Writes tests/golden/track_boxes.npz; only data, no reference source.

The reference's module is loaded from its file (it imports numpy and scipy, nothing of its package).  The joints are made as
tools/make_goldens_bbox.py makes them -- a body of 25 joints drifting across a 1920 x 1080 frame with a sway and per-joint jitter -- and a dead
frame is one whose scores are all at or below 0.3 (one of them exactly 0.3: the rule is strict).  Per case:
  <name>_kp      (T,25,3) float64 input        <name>_sigma   the Gaussian's sigma of the case
  <name>_params  (n,3) [cx, cy, scale] of get_all_bbox_params, n = end - start          <name>_range  [start, end)
  <name>_median  (n,3) scipy.signal.medfilt(column, 11) of _params, as smooth_bbox_params forms it
  <name>_smooth  (n,3) smooth_bbox_params(_params, 11, sigma)
(`dead` has no detection: the reference returns an empty array and [-1, 0), and there is nothing to smooth.)"""
import argparse
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.make_goldens_bbox import BODY  # noqa: E402

VIS_THRESH, KERNEL = 0.3, 11

# name: (T, seed, sigma, dead frames, frame whose visible joints coincide or None)
CASES = {
    "t1": (1, 1, 3.0, (), None),                                # one detected frame
    "t2": (2, 2, 3.0, (), None),                                # the shortest sequence that can be filtered
    "t5": (5, 3, 8.0, (), None),                                # radius 32 > 2n: the reflection repeats
    "t12": (12, 4, 3.0, (), None),                              # the window of 11 is just covered
    "t26gaps": (26, 5, 3.0, (0, 1, 7, 13, 14, 15, 24, 25), None),      # dead at the front, two at the back, gaps of 1 and 3 inside
    "t70": (70, 6, 8.0, "random", None),                        # about 30 % dead frames
    "dead": (8, 7, 3.0, tuple(range(8)), None),                 # no detection at all
    "point": (6, 8, 3.0, (), 3),                                # frame 3: height 0 < 0.5, so it is interpolated
}


def make_case(T, seed, dead, point):
    g = np.random.Generator(np.random.Philox(key=[2026, seed]))
    t = np.arange(T, dtype=np.float64)
    height = 620.0
    cx = 400.0 + (1100.0 / max(T - 1, 1)) * t + g.uniform(-3, 3, T)
    cy = 540.0 + 12.0 * np.sin(t * 0.55) + g.uniform(-2, 2, T)
    kp = np.empty((T, 25, 3))
    kp[:, :, 0] = cx[:, None] + BODY[None, :, 0] * height + g.normal(0.0, 4.0, (T, 25))
    kp[:, :, 1] = cy[:, None] + BODY[None, :, 1] * height + g.normal(0.0, 4.0, (T, 25))
    low = g.uniform(0.0, 1.0, (T, 25)) < 0.125
    kp[:, :, 2] = np.where(low, g.uniform(0.0, 0.3, (T, 25)), g.uniform(0.31, 1.0, (T, 25)))
    if isinstance(dead, str):
        dead = tuple(np.flatnonzero(g.uniform(0.0, 1.0, T) < 0.3))
    for k, f in enumerate(dead):
        kp[f, :, 2] = g.uniform(0.0, 0.29, 25)
        if k == 0:
            kp[f, 4, 2] = VIS_THRESH                            # exactly the threshold: not visible
    if point is not None:
        vis = kp[point, :, 2] > VIS_THRESH
        kp[point, vis, :2] = kp[point, np.flatnonzero(vis)[0], :2]
    return kp, dead


def reference_module(reference):
    spec = importlib.util.spec_from_file_location("reference_smooth_bbox", os.path.join(reference, "lib", "utils", "smooth_bbox.py"))
    module = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # scipy.ndimage.filters is a deprecated name
        spec.loader.exec_module(module)
    return module


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GRNET_REFERENCE", ""), help="a checkout of the reference")
    a = ap.parse_args()
    if not a.reference:
        sys.exit("make_goldens_track.py: name the reference checkout with --reference or GRNET_REFERENCE")
    ref = reference_module(a.reference)
    out = {}
    for name, (T, seed, sigma, dead, point) in CASES.items():
        kp, dead = make_case(T, seed, dead, point)
        params, start, end = ref.get_all_bbox_params(list(kp.copy()), vis_thresh=VIS_THRESH)
        params = np.asarray(params, np.float64)
        assert params.shape == (end - start if start >= 0 else 0, 3), (name, params.shape, start, end)
        out[name + "_kp"], out[name + "_sigma"] = kp, np.float64(sigma)
        out[name + "_params"], out[name + "_range"] = params, np.array([start, end], np.int32)
        if params.shape[0]:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                 # medfilt: kernel_size exceeds volume extent, for the short cases
                median = np.array([ref.signal.medfilt(col, KERNEL) for col in params.T]).T
                smooth = ref.smooth_bbox_params(params, KERNEL, sigma)
            assert smooth.shape == params.shape and smooth.dtype == np.float64
            out[name + "_median"], out[name + "_smooth"] = median, smooth
        print(f"{name:8s} T {T:3d}  [{start}, {end})  dead {len(dead):2d}  sigma {sigma:g}  "
              f"smoothed scale <= 0 on {int((out.get(name + '_smooth', np.ones((1, 3)))[:, 2] <= 0).sum())} frames")
    path = os.path.join(ROOT, "tests", "golden", "track_boxes.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
