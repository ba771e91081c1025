#!/usr/bin/env python3
"""Golden vectors for the camera-space translation, produced by RUNNING the reference's own estimate_translation_np
(lib/utils/geometry.py:296-337) in float64.  Writes tests/golden/translation.npz; only data, no reference source.

The reference's module is loaded from its file (it imports torch and numpy, nothing of its package).  Its signature allows one focal length and
a square image whose centre is img_size / 2, so the cases are square: img_size 224 with f = 5000 at 30-60 m, img_size 1080 with
f = sqrt(1920^2 + 1080^2) and f = 1000 at 2-8 m, each with 13 and with 25 joints, 20 frames a case (tests/helpers/translation_checks.py makes the
inputs: a body-sized cloud, 3 px noise, confidences in (0.05, 1) with some zeroed).  The function is handed the widened float32 inputs, so the
file holds exactly what the tests feed the code: per case the float32 joints3d (T,K,3) and joints2d (T,K,3), (img_size, f) and the reference's
float64 translations (T,3).  The reference weights EVERY joint by sqrt(conf): the tests call the code with conf_threshold = 0 on these cases, and
a zeroed confidence drops out of both."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import translation_checks as tc  # noqa: E402

FRAMES = 20


def reference_function(reference):
    spec = importlib.util.spec_from_file_location("reference_geometry", os.path.join(reference, "lib", "utils", "geometry.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.estimate_translation_np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GRNET_REFERENCE", ""), help="a checkout of the reference")
    a = ap.parse_args()
    if not a.reference:
        sys.exit("make_goldens_translation.py: name the reference checkout with --reference or GRNET_REFERENCE")
    fn = reference_function(a.reference)
    out, seed = {}, 0
    for ci, (size, f, depth) in enumerate(tc.GOLDEN_CAMERAS):
        for K in (13, 25):
            seed += 1
            pairs = np.stack([np.arange(K), np.arange(K)], axis=1)
            j3, j2, _ = tc.random_case(FRAMES, pairs, K, K, seed, f, (size / 2, size / 2), (size, size), depth)
            S, D = tc.widen(j3), tc.widen(j2)
            t = np.stack([fn(S[i], D[i, :, :2], D[i, :, 2], focal_length=f, img_size=size) for i in range(FRAMES)])
            assert t.dtype == np.float64 and np.isfinite(t).all()
            name = f"c{ci}_k{K}"
            out[name + "_joints3d"], out[name + "_joints2d"] = j3, j2
            out[name + "_camera"] = np.array([size, f])
            out[name + "_t"] = t
            print(f"{name}: img_size {size:.0f}, f {f:.3f}, {K} joints, depth {t[:, 2].min():.2f} .. {t[:, 2].max():.2f} m")
    path = os.path.join(ROOT, "tests", "golden", "translation.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
