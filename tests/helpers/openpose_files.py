"""A folder of small OpenPose .mat files for the tests of pipeline.openpose_boxes (the rules of batch_generation.py:95-178): what each file is
for, which keys and bad names the folder must give, and for every key the scaled candidate whose box must be the one stored."""
import os

import numpy as np
import scipy.io as sio

IMG_W, IMG_H = 1920, 1080


def person(g, T, height, x0, scores):
    """(T,25,3) normalised joints of a body `height` of the image tall walking from x0: joints 0 and 1 pin the top and the bottom."""
    cx = x0 + 0.3 * np.arange(T)[:, None] / max(T - 1, 1)
    j = np.empty((T, 25, 3))
    j[:, :, 0] = cx + g.uniform(-0.04, 0.04, (T, 25))
    j[:, :, 1] = 0.5 + g.uniform(-height / 2, height / 2, (T, 25))
    j[:, 0, 1], j[:, 1, 1] = 0.5 - height / 2, 0.5 + height / 2
    j[:, :, 2] = scores
    j[:, 2, 2] = 0.8                                            # joint 2 is the one the :120 test looks at
    return j


def scaled(j):
    out = j.copy()
    out[:, :, 0] *= IMG_W
    out[:, :, 1] *= IMG_H
    return out


def write_folder(folder):
    """Writes the files; returns (keys, bad, chosen {key: scaled (T,25,3) candidate}, rejected {key: the scaled candidate that must lose})."""
    os.makedirs(folder, exist_ok=True)
    g = np.random.Generator(np.random.Philox(key=[95, 178]))
    T = 6
    s = g.uniform(0.4, 0.9, (T, 25))
    s[g.uniform(0, 1, (T, 25)) < 0.1] = 0.05                    # some joints below the 0.1 of the frame rule, all scores positive
    chosen, rejected = {}, {}

    # two persons whose mean scores differ by 0.001 (< 0.01): both are candidates, the one with the larger box wins -- the SECOND
    a, b = person(g, T, 0.55, 0.2, s), person(g, T, 0.70, 0.4, s + 0.001)
    sio.savemat(os.path.join(folder, "A001_close.mat"), {"skeleton": np.stack([a, b])})
    chosen["A001_close"], rejected["A001_close"] = scaled(b), scaled(a)

    # two persons whose mean scores differ by 0.05: only the better one is a candidate, though the other is taller
    a, b = person(g, T, 0.55, 0.3, s), person(g, T, 0.80, 0.1, s - 0.05 * (s > 0.2))
    sio.savemat(os.path.join(folder, "A002_apart.mat"), {"skeleton": np.stack([a, b])})
    chosen["A002_apart"], rejected["A002_apart"] = scaled(a), scaled(b)

    # one person, 11 frames
    a = person(g, 11, 0.6, 0.25, g.uniform(0.4, 0.9, (11, 25)))
    sio.savemat(os.path.join(folder, "A003_one.mat"), {"skeleton": a[None]})
    chosen["A003_one"] = scaled(a)

    # two persons, the second fails :120 (all three components of joint 2 <= 0.3 in frame 3) and drops out before the scores are compared
    a, b = person(g, T, 0.55, 0.2, s), person(g, T, 0.75, 0.3, s + 0.002)
    b[3, 2] = (0.2, 0.25, 0.25)
    sio.savemat(os.path.join(folder, "A004_partly.mat"), {"skeleton": np.stack([a, b])})
    chosen["A004_partly"], rejected["A004_partly"] = scaled(a), scaled(b)

    bad = []
    sio.savemat(os.path.join(folder, "A005_empty.mat"), {"skeleton": np.zeros((0, 0, 25, 3))})
    bad.append("A005_empty.mat")
    a = person(g, T, 0.6, 0.2, s)                                # the only person fails :120
    a[3, 2] = (0.2, 0.25, 0.25)
    sio.savemat(os.path.join(folder, "A006_rule120.mat"), {"skeleton": a[None]})
    bad.append("A006_rule120.mat")
    a = person(g, T, 0.6, 0.2, s)                                # frame 2 has only 3 joints of positive score: :114 wants more than 3
    a[2, 3:, 2] = 0.0
    sio.savemat(os.path.join(folder, "A007_sparse.mat"), {"skeleton": a[None]})
    bad.append("A007_sparse.mat")
    # an interaction action: skipped by its name, neither a key nor a bad file, whatever it holds
    sio.savemat(os.path.join(folder, "A045_interaction.mat"), {"skeleton": person(g, T, 0.6, 0.2, s)[None]})
    return sorted(chosen), bad, chosen, rejected
