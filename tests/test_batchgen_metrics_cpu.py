"""batch_generation.py --gt_path through the model_factory / gloo seam of the CPU tests: the metrics of every video against the
independent checker, a video skipped by name and one by frame count, the JSON schema, the device method used once per window where the model has
one, the refusal of the two flags without --gt_path, and the database of a run without --gt_path unchanged."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import metric_checks as mc
from .test_host_cpu import _StandInModel, _stand_in_factory, _write_video_dir

LENGTHS = [7, 23, 3, 12, 1, 2]
KEYS = ("frames", "mpjpe", "pa_mpjpe", "accel", "accel_err")


@pytest.fixture(scope="module")
def bg():
    sys.path.insert(0, ROOT)
    return importlib.import_module("batch_generation")


@pytest.fixture(scope="module")
def plain_run(bg, tmp_path_factory):
    """One run without --gt_path: the database every other test starts from, and a ground truth made from it."""
    import joblib
    root = str(tmp_path_factory.mktemp("batchgen_metrics"))
    fv, vid_folder = _write_video_dir(root, LENGTHS)
    written = bg.prepare_data(fv, vid_folder, os.path.join(root, "plain.json"), max_frames=8, chunk=8, model_factory=_stand_in_factory, backend="gloo")
    db = joblib.load(written[0])
    g = np.random.Generator(np.random.Philox(key=[77, 1]))
    names = np.asarray(db["vid_name"])
    truth = (db["joints3D"] + g.normal(0.0, 0.05, db["joints3D"].shape)).astype(np.float32)
    order = list(dict.fromkeys(str(v) for v in names))
    assert len(order) == len(LENGTHS)
    keep = names != order[1]                                   # the ground truth lacks video 1 ...
    short = np.flatnonzero(names == order[3])[-1]
    keep[short] = False                                        # ... and has one frame less of video 3
    gt_path = os.path.join(root, "gt.pkl")
    joblib.dump({"vid_name": names[keep], "joints3D": truth[keep]}, gt_path)
    return {"root": root, "fv": fv, "vid_folder": vid_folder, "db": db, "truth": truth, "order": order, "gt_path": gt_path}


def expected_rows(run, skipped):
    db, rows = run["db"], {}
    names = np.asarray(db["vid_name"])
    for key in run["order"]:
        if key in skipped:
            continue
        at = names == key
        _, per_seq, _, _ = mc.expected(db["joints3D"][at], run["truth"][at], root=[0], unit=1000.0)
        rows[key] = (int(at.sum()), per_seq[0])
    return rows


def check_json(path, run, skipped):
    with open(path) as f:
        text = f.read()
    assert "NaN" not in text
    got = json.loads(text)
    rows = expected_rows(run, skipped)
    assert sorted(got) == sorted(list(rows) + ["total"])
    sums, counts = np.zeros(5), np.zeros(5)
    for key, (T, want) in rows.items():
        assert tuple(got[key]) == KEYS and got[key]["frames"] == T
        for c, name in ((0, "mpjpe"), (1, "pa_mpjpe"), (3, "accel"), (4, "accel_err")):
            if np.isnan(want[c]):
                assert got[key][name] is None, (key, name)
            else:
                assert got[key][name] == pytest.approx(want[c], rel=1e-9), (key, name)
                n = T if c < 2 else T - 2
                sums[c] += want[c] * n
                counts[c] += n
    assert tuple(got["total"]) == KEYS and got["total"]["frames"] == sum(T for T, _ in rows.values())
    for c, name in ((0, "mpjpe"), (1, "pa_mpjpe"), (3, "accel"), (4, "accel_err")):
        assert got["total"][name] == pytest.approx(sums[c] / counts[c], rel=1e-9)


def test_gt_path_reports_every_matched_video_and_leaves_the_database_alone(bg, plain_run, capsys):
    import joblib
    run = plain_run
    out = os.path.join(run["root"], "with_gt.json")
    written = bg.prepare_data(run["fv"], run["vid_folder"], out, max_frames=8, chunk=8, model_factory=_stand_in_factory, backend="gloo", gt_path=run["gt_path"])
    printed = capsys.readouterr().out
    skipped = (run["order"][1], run["order"][3])
    assert f"Metrics: skip video {skipped[0]}, the ground truth has no such video." in printed
    assert f"Metrics: skip video {skipped[1]}, 12 frames here and 11 in the ground truth." in printed
    assert printed.count("Metrics: skip") == 2
    db = joblib.load(written[0])
    for k in ("vid_name", "bbox", "joints3D"):
        assert np.array_equal(db[k], run["db"][k]), k
    check_json(os.path.join(run["root"], "with_gt_metrics.json"), run, skipped)      # the default path; the stand-in has no pose_metrics: host


class _StandInWithMetrics(_StandInModel):
    """The stand-in with the device method's signature (answered by the host statement): batch_generation must prefer it."""
    calls = []

    def pose_metrics(self, pred, gt, lengths=None, root=None, select=None, unit=1000.0):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).calls.append((list(lengths), list(root), list(select), unit, torch.is_tensor(pred)))
        return {k: torch.from_numpy(v) for k, v in pipe.pose_metrics(pred.numpy(), gt, lengths=lengths, root=root, select=select, unit=unit).items()}


def test_model_method_is_used_once_per_window_unless_on_host(bg, plain_run):
    run = plain_run
    skipped = (run["order"][1], run["order"][3])
    for on_host, name in ((False, "dev.json"), (True, "host.json")):
        _StandInWithMetrics.calls.clear()
        mout = os.path.join(run["root"], "m_" + name)
        bg.prepare_data(run["fv"], run["vid_folder"], os.path.join(run["root"], name), max_frames=8, chunk=8, model_factory=lambda r: _StandInWithMetrics(),
                        backend="gloo", gt_path=run["gt_path"], metrics_out=mout, metrics_on_host=on_host)
        check_json(mout, run, skipped)
        if on_host:
            assert _StandInWithMetrics.calls == []
        else:
            assert _StandInWithMetrics.calls == [([7, 3, 1, 2], [0], list(range(25)), 1000.0, True)]      # one call, one sequence per matched video


def test_metric_flags_are_refused_without_gt_path(bg):
    for argv in (["--metrics_out", "m.json"], ["--metrics_on_host"]):
        with pytest.raises(SystemExit) as e:
            bg.main(argv + ["--vid_folder", "nowhere", "--bbox_path", "none"])
        assert "--gt_path" in str(e.value)


def test_ground_truth_schema_is_checked(bg, tmp_path):
    import joblib
    path = str(tmp_path / "bad.pkl")
    joblib.dump({"vid_name": np.array(["a", "a"]), "joints3D": np.zeros((2, 24, 3), np.float32)}, path)
    with pytest.raises(ValueError, match="joints3D"):
        bg.load_ground_truth(path)
