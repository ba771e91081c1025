"""The box from 2D joints on the host: pipeline.bbox_from_joints2d against the reference's own function (tests/golden/bbox_joints2d.npz,
tools/make_goldens_bbox.py) and against sklearn's distance matrix, pipeline.openpose_boxes on .mat files written here, and the new arguments of
batch_generation.py."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from .conftest import ROOT
from .helpers import bbox_checks as bc
from .helpers import openpose_files

CASES = ("t1", "t2", "t11", "t41", "t400", "allbelow", "small")


@pytest.fixture(scope="module")
def golden_bbox():
    return np.load(os.path.join(ROOT, "tests", "golden", "bbox_joints2d.npz"))


@pytest.fixture(scope="module")
def bg():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("batch_generation")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("openpose"))
    return (d,) + openpose_files.write_folder(d)


def test_golden_file_holds_the_cases_with_their_gaps(golden_bbox):
    g = golden_bbox
    assert sorted(k[:-3] for k in g.files if k.endswith("_kp")) == sorted(CASES)
    assert [g[c + "_kp"].shape[0] for c in CASES[:5]] == [1, 2, 11, 41, 400]
    for c in CASES:
        assert float(g[c + "_gap"]) >= 1e-5, c                              # ten times the bound the GPU's choice is held to
        assert (c + "_cost" in g.files) == (g[c + "_kp"].shape[0] <= 41)
    assert (g["allbelow_kp"][7, :, 2] < 0.1).all()
    assert g["small_bbox"][0, 2] < 500 * 1.8 and g["t11_bbox"][0, 2] >= 500


@pytest.mark.parametrize("case", CASES)
def test_host_statement_equals_the_reference_bit_for_bit(pkg, golden_bbox, case):
    kp = golden_bbox[case + "_kp"]
    before = kp.copy()
    box = pkg.pipeline.bbox_from_joints2d(kp)
    assert box.dtype == np.float64 and box.shape == (kp.shape[0], 4)
    assert np.array_equal(box, golden_bbox[case + "_bbox"])
    assert np.array_equal(kp, before)
    points, _ = bc.prepare(kp)
    m = int(golden_bbox[case + "_medoid"])
    assert tuple(points[m, :2]) == tuple(box[0, :2].astype(np.float32))
    if case + "_cost" in golden_bbox.files:
        assert np.array_equal(bc.row_costs(points), golden_bbox[case + "_cost"])
        assert bc.gap(points) == float(golden_bbox[case + "_gap"])


@pytest.mark.parametrize("case", CASES)
def test_host_statement_equals_the_sklearn_path(pkg, golden_bbox, case):
    """euclidean_distances over the three float32 columns, as the reference calls it, and the float64 argmin of its row sums."""
    pairwise = pytest.importorskip("sklearn.metrics.pairwise")
    kp = golden_bbox[case + "_kp"]
    points, _ = bc.prepare(kp)
    disc = pairwise.euclidean_distances(points)
    m = int(np.argmin(disc.sum(axis=1, dtype=np.float64)))
    box = pkg.pipeline.bbox_from_joints2d(kp)
    assert tuple(box[0, :2]) == tuple(points[m, :2].astype(np.float64))


def test_host_statement_refuses_bad_input(pkg):
    f = pkg.pipeline.bbox_from_joints2d
    with pytest.raises(ValueError, match="T,K,3"):
        f(np.zeros((4, 25, 2)))
    with pytest.raises(ValueError, match="T,K,3"):
        f(np.zeros((0, 25, 3)))
    bad = np.ones((3, 25, 3))
    bad[1, 4, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        f(bad)


def test_openpose_boxes_on_the_host(pkg, folder):
    d, keys, bad, chosen, rejected = folder
    pipe = pkg.pipeline
    boxes, got_bad = pipe.openpose_boxes(d)
    assert sorted(boxes) == keys and got_bad == bad                         # the interaction file is neither
    for key, cand in chosen.items():
        want = pipe.bbox_from_joints2d(cand)
        assert boxes[key].dtype == np.float64 and np.array_equal(boxes[key], want), key
    # the candidates that lose: A001's is a candidate with the smaller box; A002's and A004's would have won by size had they been candidates
    assert pipe.bbox_from_joints2d(rejected["A001_close"])[0, 2] < boxes["A001_close"][0, 2]
    assert pipe.bbox_from_joints2d(rejected["A002_apart"])[0, 2] > boxes["A002_apart"][0, 2]
    assert pipe.bbox_from_joints2d(rejected["A004_partly"])[0, 2] > boxes["A004_partly"][0, 2]


class _HostModel:
    """Stands in for GRNet behind openpose_boxes(model=...): the same signature, the host statement per sequence; counts its calls."""

    def __init__(self, pipe):
        self.pipe, self.calls, self.closed = pipe, [], False

    def bbox_from_joints2d(self, joints2d, lengths=None, threshold=0.1):
        self.calls.append(list(lengths))
        off = np.concatenate([[0], np.cumsum(lengths)])
        return torch.from_numpy(np.stack([self.pipe.bbox_from_joints2d(joints2d[a:b], threshold)[0] for a, b in zip(off, off[1:])]))

    def close(self):
        self.closed = True


def test_openpose_boxes_hands_a_model_every_candidate_in_one_call(pkg, folder):
    d, keys, bad, chosen, _ = folder
    m = _HostModel(pkg.pipeline)
    boxes, got_bad = pkg.pipeline.openpose_boxes(d, model=m)
    assert m.calls == [[6, 6, 6, 11, 6]]                                   # A001: both persons; A002, A003, A004: one each
    host, _ = pkg.pipeline.openpose_boxes(d)
    assert sorted(boxes) == keys and got_bad == bad
    assert all(np.array_equal(boxes[k], host[k]) for k in keys)


def test_batch_generation_refuses_contradictory_box_arguments(bg, capsys):
    for argv, word in ((["--bbox_path", "a.pkl", "--openpose_folder", "d"], "give one of them"),
                       (["--bbox_out", "b.pkl"], "belong to --openpose_folder"),
                       (["--bbox_on_host", "--bbox_path", "a.pkl"], "belong to --openpose_folder"),
                       (["--openpose_folder", "d"], "--bbox_out")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv


def test_batch_generation_writes_the_box_file(pkg, bg, folder, tmp_path):
    import joblib
    d, keys, bad, chosen, _ = folder
    host, _ = pkg.pipeline.openpose_boxes(d)
    out = str(tmp_path / "coarse_bbox.json")
    bg.main(["--openpose_folder", d, "--bbox_out", out, "--bbox_on_host"])
    got = joblib.load(out)
    assert sorted(got) == keys and all(np.array_equal(got[k], host[k]) for k in keys)
    assert joblib.load(out + ".bad") == bad
    # the device path's seam: a model that is handed every candidate at once, and closed afterwards
    m = _HostModel(pkg.pipeline)
    out2 = str(tmp_path / "coarse_bbox_model.json")
    annos = bg.boxes_from_openpose(d, out2, model_factory=lambda local_rank: m)
    assert len(m.calls) == 1 and m.closed
    got2 = joblib.load(out2)
    assert all(np.array_equal(got2[k], host[k]) and np.array_equal(annos[k], host[k]) for k in keys)
