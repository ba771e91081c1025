#!/usr/bin/env python3
"""Writes tests/golden/skeleton_view.npz, the pins of the 3D skeleton view, from the libraries the reference draws it with.  Runs
where matplotlib, scipy and a checkout of the reference are present (the development machine), not on the GPU machine:

  P, window      matplotlib's Axes3D.get_proj() and the part of the projected plane its axes show, for the reference's figure and settings
                 (demo.py:288-290, 311-314): a 640 x 480 figure, add_subplot(1,2,2, projection='3d'), view_init(elev=200, azim=-27), the limits
  points, proj   64 seeded points and their projected (xs, ys) by mpl_toolkits.mplot3d.proj3d.proj_transform
  bones_spin, bones_kinectv2   what the reference's get_spin_skeleton() / get_kinectv2_skeleton() RETURN (lib/data_utils/kp_utils.py, a pure
                 numpy module imported read-only from /root/reference)
  joints, ex_R   5 seeded (49,3) joint sets and the FIRST ROW of scipy.linalg.orthogonal_procrustes([[1,0,0]], cross(h, v)) for them
                 (demo.py:239-247) -- the input has rank 1, so only that row is determined

Only data is written; no reference source is copied.  lib/utils/vis.py itself (draw_3d_skeleton) cannot be imported here -- cv2, pyrender and
trimesh are absent -- so the colours and the line width are restated in pipeline.py and DESIGN 4.6 from reading vis.py:571-587."""
import os
import sys

import matplotlib
import numpy as np

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
from mpl_toolkits.mplot3d import proj3d  # noqa: E402
from scipy.linalg import orthogonal_procrustes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference/lib/data_utils")
import kp_utils  # noqa: E402

fig = plt.figure("Video")
fig.add_subplot(1, 2, 1)
ax = fig.add_subplot(1, 2, 2, projection="3d")
ax.view_init(elev=200, azim=-27)
ax.set_xlim3d([-0.6, 0.6])
ax.set_ylim3d([-1.0, 1.0])
ax.set_zlim3d([-1.0, 1.0])
fig.canvas.draw()
P = ax.get_proj()
(x0, y0), (x1, y1) = ax.transData.inverted().transform(ax.bbox.get_points())
g = np.random.Generator(np.random.Philox(key=[41, 41]))
points = g.uniform(-1.0, 1.0, (64, 3)) * (0.6, 1.0, 1.0)
xs, ys, _ = proj3d.proj_transform(points[:, 0], points[:, 1], points[:, 2], P)
joints = g.standard_normal((5, 49, 3)) * (0.2, 0.3, 0.3)
ex_R = []
for j in joints:
    h, v = j[28] - j[27], j[40] - j[39]
    h, v = h / np.linalg.norm(h), v / np.linalg.norm(v)
    R, _ = orthogonal_procrustes(np.array([[1.0, 0.0, 0.0]]), np.cross(h, v).reshape(1, 3))
    ex_R.append(R[0])
out = os.path.join(ROOT, "tests", "golden", "skeleton_view.npz")
np.savez(out, P=np.asarray(P, np.float64), window=np.array([x0, x1, y0, y1]), points=points, proj=np.stack([xs, ys], 1),
         bones_spin=np.asarray(kp_utils.get_spin_skeleton(), np.int64), bones_kinectv2=np.asarray(kp_utils.get_kinectv2_skeleton(), np.int64),
         joints=joints, ex_R=np.stack(ex_R), matplotlib_version=np.array(matplotlib.__version__))
print("wrote", out, "matplotlib", matplotlib.__version__, "window", (x0, x1, y0, y1), "P[3]", P[3])
