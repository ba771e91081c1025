"""batch_generation.py --gait through the model_factory / gloo seam of the CPU tests, with --gait_on_host's path: the JSON file with
one object per video keyed by pipeline.GAIT_COLUMNS and null where a parameter is undefined, the database's gait_events column, one summary line per
video, the window's translations handed over when --trajectory is on, the device method preferred where the model has one (one call per window),
and every refusal of the new flags."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .test_host_cpu import _StandInModel, _stand_in_factory

LENGTHS = {"S001C001P001R001A001": 8, "S002C001P001R001A002": 40, "S003C001P001R001A003": 27}


@pytest.fixture(scope="module")
def bg():
    sys.path.insert(0, ROOT)
    return importlib.import_module("batch_generation")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Three videos of ready crops; the stand-in's joints are a fixed function of the pixels, so they are noise of a metre or so: the longer two have
    events, the first is shorter than one window on either side and has none."""
    root = str(tmp_path_factory.mktemp("batchgen_gait"))
    vid_folder = os.path.join(root, "videos")
    g = np.random.Generator(np.random.Philox(key=[411, 1]))
    annos, joints2d = {}, {}
    for name, n in LENGTHS.items():
        os.makedirs(os.path.join(vid_folder, name))
        for fi in range(n):
            np.save(os.path.join(vid_folder, name, f"{fi:06d}.npy"), g.standard_normal((3, 224, 224)).astype(np.float32))
        annos[name] = np.tile(np.array([[112.0, 112.0, 200.0, 200.0]], np.float32), (n, 1))
        joints2d[name] = np.concatenate([g.uniform(200, 900, (n, 25, 2)), g.uniform(0.3, 0.9, (n, 25, 1))], axis=2).astype(np.float32)
    return {"root": root, "vid_folder": vid_folder, "annos": annos, "joints2d": joints2d}


def generate(bg, world, name, **kw):
    import joblib
    written = bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], name), max_frames=16, chunk=16, model_factory=_stand_in_factory, backend="gloo",
                              annos={k: v.copy() for k, v in world["annos"].items()}, **kw)
    assert len(written) == 1
    return joblib.load(written[0])


def test_gait_on_host_writes_the_json_and_the_column(bg, pkg, world, capsys):
    pipe = pkg.pipeline
    plain = generate(bg, world, "plain.json")
    assert "gait_events" not in plain
    capsys.readouterr()
    db = generate(bg, world, "walk.json", gait={"on_host": True, "sigma": 1.0, "window": 3, "min_excursion": 0.1})
    printed = capsys.readouterr().out
    assert list(db) == ["vid_name", "bbox", "joints3D", "gait_events"] and db["gait_events"].dtype == np.uint8 and db["gait_events"].shape == (sum(LENGTHS.values()),)
    assert np.array_equal(db["joints3D"], plain["joints3D"])
    path = os.path.join(world["root"], "walk_gait.json")
    text = open(path).read()
    assert "NaN" not in text and "null" in text
    found = json.loads(text)
    names = np.asarray(db["vid_name"])
    assert sorted(found) == sorted(LENGTHS)
    for key, n in LENGTHS.items():
        want = pipe.gait_parameters(db["joints3D"][names == key], fps=20.0, sigma=1.0, window=3, min_excursion=0.1)
        assert np.array_equal(db["gait_events"][names == key], want["events"].astype(np.uint8)), key
        assert list(found[key]) == list(pipe.GAIT_COLUMNS)
        for name, v in zip(pipe.GAIT_COLUMNS, want["per_sequence"][0]):
            assert (found[key][name] is None) if np.isnan(v) else (found[key][name] == float(v)), (key, name)
        assert found[key]["trajectory_speed"] is None              # no --trajectory
    short = found["S001C001P001R001A001"]
    assert [short[c] for c in pipe.GAIT_COLUMNS[:5]] == [0.0] * 5 and all(short[c] is None for c in pipe.GAIT_COLUMNS[5:])
    assert found["S002C001P001R001A002"]["steps"] > 0 and found["S002C001P001R001A002"]["cadence"] is not None
    lines = [ln for ln in printed.splitlines() if ln.startswith("Gait:")]
    assert len(lines) == 3 and lines[0] == "Gait: video S001C001P001R001A001, 0 steps, cadence none, stride-time CV none, speed none."
    assert all(word in lines[1] for word in ("steps, cadence", "steps/min", "stride-time CV", "speed"))
    assert f"Save gait parameters of 3 videos to {path}." in printed


class _StandInWithGait(_StandInModel):
    """The stand-in with the device method's signature (answered by the host statement): every video of the window must arrive in ONE call."""
    calls = []

    def gait_parameters(self, joints3d, lengths=None, trans=None, fps=20.0, sigma=2.0, window=5, min_excursion=0.05, joints=None):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).calls.append((list(lengths), None if trans is None else (tuple(trans.shape), trans.dtype), fps, sigma, window, min_excursion, tuple(joints3d.shape)))
        out = pipe.gait_parameters(joints3d.cpu().numpy(), lengths, trans, fps, sigma, window, min_excursion)
        return {k: torch.from_numpy(v) for k, v in out.items()}


def test_model_method_gets_the_window_in_one_call_with_the_translations(bg, pkg, world, tmp_path, capsys):
    import joblib
    _StandInWithGait.calls.clear()
    out = str(tmp_path / "elsewhere.json")
    written = bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], "device.json"), max_frames=16, chunk=16, model_factory=lambda r: _StandInWithGait(),
                              backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()}, gait={"fps": 25.0, "out": out},
                              trajectory={"joints2d": dict(world["joints2d"]), "on_host": True})
    db = joblib.load(written[0])
    assert _StandInWithGait.calls == [([8, 40, 27], ((75, 3), np.float64), 25.0, 2.0, 5, 0.05, (75, 25, 3))]
    assert list(db) == ["vid_name", "bbox", "joints3D", "trans", "trans_status", "reproj", "gait_events"]
    want = pkg.pipeline.gait_parameters(db["joints3D"], lengths=[8, 40, 27], trans=db["trans"].astype(np.float64), fps=25.0)     # the translations as the database holds them
    assert np.array_equal(db["gait_events"], want["events"].astype(np.uint8))
    found = json.load(open(out))
    for key, row in zip(LENGTHS, want["per_sequence"]):
        assert [found[key][c] for c in pkg.pipeline.GAIT_COLUMNS] == [None if np.isnan(v) else float(v) for v in row]
    assert not os.path.exists(os.path.join(world["root"], "device_gait.json"))


def test_main_runs_gait_on_host(bg, world, tmp_path, monkeypatch):
    """The flags reach prepare_data: main with the seam's arguments patched in."""
    import joblib
    seen = {}
    real = bg.prepare_data

    def patched(**kw):
        seen.update(kw["gait"])
        return real(**{**kw, "fv": None, "annos": {k: v.copy() for k, v in world["annos"].items()}, "model_factory": _stand_in_factory, "backend": "gloo", "max_frames": 16})
    monkeypatch.setattr(bg, "prepare_data", patched)
    fv = str(tmp_path / "boxes.pkl")
    joblib.dump(world["annos"], fv)
    outpath = str(tmp_path / "main.json")
    bg.main(["--bbox_path", fv, "--vid_folder", world["vid_folder"], "--outpath", outpath, "--gait", "--gait_on_host", "--gait_window", "4", "--gait_fps", "30"])
    assert seen == {"fps": 30.0, "sigma": None, "window": 4, "min_excursion": None, "on_host": True, "out": None}
    assert sorted(json.load(open(str(tmp_path / "main_gait.json")))) == sorted(LENGTHS)


def test_gait_flags_are_refused_where_they_do_not_belong(bg):
    base = ["--bbox_path", "a.pkl", "--vid_folder", "v"]
    for argv, word in ((["--gait_out", "g.json"] + base, "--gait_out belongs to --gait"), (["--gait_fps", "20"] + base, "--gait_fps belongs to --gait"),
                       (["--gait_sigma", "2"] + base, "--gait_sigma belongs to --gait"), (["--gait_window", "5"] + base, "--gait_window belongs to --gait"),
                       (["--gait_min_excursion", "0.05"] + base, "--gait_min_excursion belongs to --gait"), (["--gait_on_host"] + base, "--gait_on_host belongs to --gait"),
                       (["--gait", "--bbox_path", "a.pkl"], "--gait needs --vid_folder"), (["--gait", "--openpose_folder", "d", "--bbox_out", "b.pkl"], "--gait needs --vid_folder"),
                       (["--gait", "--gait_fps", "0"] + base, "--gait_fps must be"), (["--gait", "--gait_fps", "nan"] + base, "--gait_fps must be"),
                       (["--gait", "--gait_sigma", "17"] + base, "--gait_sigma must be"), (["--gait", "--gait_sigma", "-1"] + base, "--gait_sigma must be"),
                       (["--gait", "--gait_window", "0"] + base, "--gait_window must be"), (["--gait", "--gait_window", "33"] + base, "--gait_window must be"),
                       (["--gait", "--gait_min_excursion", "-0.1"] + base, "--gait_min_excursion must be")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv
