"""batch_generation.py --gait_regularity through the model_factory / gloo seam of the CPU tests, with --regularity_on_host's path: it
needs no --gait; the JSON file with one object per video -- per channel the columns of pipeline.REGULARITY_COLUMNS, step and stride time in seconds
and the acf list, null where a value is undefined, and straight_only -- one summary line per video with the event cadence beside it where --gait ran,
the database unchanged, the device method preferred where the model has one (one call per window, with --gait_turns' phase as exclude unless
--regularity_all_frames), and every refusal of the new flags."""
import importlib
import json
import os

import numpy as np
import pytest

from .test_batchgen_gait_cpu import LENGTHS, _StandInWithGait, bg, generate, world  # noqa: F401  (fixtures)
from .test_host_cpu import _stand_in_factory

LOOSE = {"max_lag": 12, "min_lag": 2, "min_peak": 0.01, "min_pairs": 3}           # the stand-in's joints are noise: a low bar finds some peaks in it


def test_regularity_on_host_needs_no_gait_and_writes_the_json(bg, pkg, world, capsys):
    pipe = pkg.pipeline
    plain = generate(bg, world, "plain_reg.json")
    capsys.readouterr()
    db = generate(bg, world, "steady.json", regularity={"on_host": True, **LOOSE})
    printed = capsys.readouterr().out
    assert list(db) == list(plain) and all(np.array_equal(db[k], plain[k]) for k in plain)          # the database gains nothing
    path = os.path.join(world["root"], "steady_regularity.json")
    text = open(path).read()
    assert "NaN" not in text and "null" in text
    found = json.loads(text)
    names = np.asarray(db["vid_name"])
    assert sorted(found) == sorted(LENGTHS)
    peaks = 0
    for key in LENGTHS:
        want = pipe.gait_regularity(db["joints3D"][names == key], fps=20.0, **LOOSE)
        assert list(found[key]) == ["straight_only"] + list(pipe.REGULARITY_CHANNELS) and found[key]["straight_only"] is False
        for c, channel in enumerate(pipe.REGULARITY_CHANNELS):
            got = found[key][channel]
            assert list(got) == list(pipe.REGULARITY_COLUMNS) + ["step_time", "stride_time", "acf"] and len(got["acf"]) == 13
            row = want["per_sequence"][0, c]
            for name, v in zip(pipe.REGULARITY_COLUMNS, row):
                assert (got[name] is None) if np.isnan(v) else (got[name] == float(v)), (key, channel, name)
            assert got["step_time"] == (None if np.isnan(row[3]) else row[3] / 20.0) and got["stride_time"] == (None if np.isnan(row[6]) else row[6] / 20.0)
            assert got["acf"] == [None if np.isnan(v) else float(v) for v in want["acf"][0, c]]
            peaks += row[5] >= 0
        assert all(v is None for k, v in found[key]["bob"].items() if k not in ("n", "acf")) and found[key]["bob"]["n"] == 0          # no --trajectory: no bob
    print(f"{peaks} stride lags found in the noise")
    assert peaks > 0
    lines = [ln for ln in printed.splitlines() if ln.startswith("Regularity:")]
    assert len(lines) == 3 and all(word in lines[1] for word in ("from the autocorrelation, step regularity", "stride regularity", "symmetry"))
    assert lines[0].startswith("Regularity: video S001C001P001R001A001, cadence ") and all(ln.endswith(".") and "(events:" not in ln for ln in lines)
    assert f"Save gait regularity of 3 videos to {path}." in printed
    capsys.readouterr()
    generate(bg, world, "steady_walk.json", gait={"on_host": True, "sigma": 1.0, "window": 3, "min_excursion": 0.1}, regularity={"on_host": True, **LOOSE})
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Regularity:")]
    assert len(lines) == 3 and all("from the autocorrelation (events: " in ln for ln in lines)          # the event cadence beside it


class _StandInWithRegularity(_StandInWithGait):
    """The stand-in with the device methods' signatures (answered by the host statements): every video of the window must arrive in ONE call."""
    seen = []
    phases = []

    def gait_turns(self, joints3d, events, gait_rows, lengths=None, **kw):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        out = pipe.gait_turns(joints3d.cpu().numpy(), events.cpu().numpy(), gait_rows.cpu().numpy(), lengths=lengths, **kw)
        out["phase"][5:9] = 1                                  # the noise has no turn: mark one
        type(self).phases.append(out["phase"].copy())
        return {k: torch.from_numpy(v) for k, v in out.items()}

    def gait_regularity(self, joints3d, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20, joints=None):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).seen.append((None if exclude is None else np.asarray(exclude).copy(), list(lengths), trans, fps, sigma, max_lag, min_lag, min_peak, min_pairs,
                                tuple(joints3d.shape)))
        out = pipe.gait_regularity(joints3d.cpu().numpy(), lengths, trans, exclude, fps, sigma, max_lag, min_lag, min_peak, min_pairs)
        return {k: torch.from_numpy(v) for k, v in out.items()}


def test_model_method_gets_the_window_in_one_call_with_the_turns_phase(bg, pkg, world, tmp_path):
    seen, phases = _StandInWithRegularity.seen, _StandInWithRegularity.phases
    for all_frames in (False, True):
        seen.clear()
        phases.clear()
        out = str(tmp_path / f"elsewhere{int(all_frames)}.json")
        bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], f"device_regularity{int(all_frames)}.json"), max_frames=16, chunk=16,
                        model_factory=lambda r: _StandInWithRegularity(), backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()},
                        gait={"window": 3, "fps": 25.0}, turns={}, regularity={"max_lag": 12, "out": out, "all_frames": all_frames})
        assert len(seen) == 1 and len(phases) == 1
        exclude, *rest = seen[0]
        assert rest == [[8, 40, 27], None, 25.0, 0.0, 12, 4, 0.25, 20, (75, 25, 3)]                 # the gait call's fps
        found = json.load(open(out))
        assert sorted(found) == sorted(LENGTHS) and all(v["straight_only"] is (not all_frames) for v in found.values())
        if all_frames:
            assert exclude is None
        else:
            assert exclude.dtype == np.int32 and np.array_equal(exclude, phases[0]) and exclude[5:9].tolist() == [1] * 4
            assert found["S001C001P001R001A001"]["sep"]["n"] == 5                                      # frames 5 .. 7 of its 8 do not count
    seen.clear()
    bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], "device_regularity_alone.json"), max_frames=16, chunk=16,
                    model_factory=lambda r: _StandInWithRegularity(), backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()}, regularity={"fps": 30.0})
    assert len(seen) == 1 and seen[0][0] is None and seen[0][3] == 30.0 and not json.load(open(os.path.join(world["root"], "device_regularity_alone_regularity.json")))[
        "S002C001P001R001A002"]["straight_only"]


def test_main_runs_regularity_on_host(bg, world, tmp_path, monkeypatch):
    """The flags reach prepare_data: main with the seam's arguments patched in, without --gait."""
    import joblib
    seen = {}
    real = bg.prepare_data

    def patched(**kw):
        seen.update(kw["regularity"])
        assert kw["gait"] is None
        return real(**{**kw, "fv": None, "annos": {k: v.copy() for k, v in world["annos"].items()}, "model_factory": _stand_in_factory, "backend": "gloo", "max_frames": 16})
    monkeypatch.setattr(bg, "prepare_data", patched)
    fv = str(tmp_path / "boxes.pkl")
    joblib.dump(world["annos"], fv)
    outpath = str(tmp_path / "main.json")
    bg.main(["--bbox_path", fv, "--vid_folder", world["vid_folder"], "--outpath", outpath, "--gait_regularity", "--regularity_on_host", "--gait_fps", "30",
             "--regularity_sigma", "1", "--regularity_max_lag", "12", "--regularity_min_peak", "0.1", "--regularity_all_frames"])
    assert seen == {"fps": 30.0, "sigma": 1.0, "max_lag": 12, "min_lag": None, "min_peak": 0.1, "min_pairs": None, "all_frames": True, "on_host": True, "out": None}
    found = json.load(open(str(tmp_path / "main_regularity.json")))
    assert sorted(found) == sorted(LENGTHS) and not os.path.exists(str(tmp_path / "main_gait.json")) and len(found["S002C001P001R001A002"]["sep"]["acf"]) == 13


def test_regularity_flags_are_refused_where_they_do_not_belong(bg):
    base = ["--bbox_path", "a.pkl", "--vid_folder", "v"]
    on = ["--gait_regularity"] + base
    for argv, word in ((["--regularity_out", "t.json"] + base, "--regularity_out belongs to --gait_regularity"),
                       (["--regularity_sigma", "1"] + base, "--regularity_sigma belongs to --gait_regularity"),
                       (["--regularity_max_lag", "50"] + base, "--regularity_max_lag belongs to --gait_regularity"),
                       (["--regularity_min_lag", "5"] + base, "--regularity_min_lag belongs to --gait_regularity"),
                       (["--regularity_min_peak", "0.3"] + base, "--regularity_min_peak belongs to --gait_regularity"),
                       (["--regularity_min_pairs", "30"] + base, "--regularity_min_pairs belongs to --gait_regularity"),
                       (["--gait", "--regularity_all_frames"] + base, "--regularity_all_frames belongs to --gait_regularity"),
                       (["--regularity_on_host"] + base, "--regularity_on_host belongs to --gait_regularity"),
                       (["--gait_fps", "25"] + base, "--gait_fps belongs to --gait"), (["--gait_regularity", "--bbox_path", "a.pkl"], "--gait_regularity needs --vid_folder"),
                       (["--regularity_sigma", "17"] + on, "--regularity_sigma must be"), (["--regularity_sigma", "nan"] + on, "--regularity_sigma must be"),
                       (["--regularity_max_lag", "7"] + on, "--regularity_max_lag must be"), (["--regularity_max_lag", "256"] + on, "--regularity_max_lag must be"),
                       (["--regularity_min_lag", "1"] + on, "--regularity_min_lag must be"), (["--regularity_min_lag", "59"] + on, "--regularity_min_lag must be"),
                       (["--regularity_min_lag", "9", "--regularity_max_lag", "10"] + on, "--regularity_min_lag must be"),
                       (["--regularity_min_peak", "0"] + on, "--regularity_min_peak must be"), (["--regularity_min_peak", "1.5"] + on, "--regularity_min_peak must be"),
                       (["--regularity_min_peak", "nan"] + on, "--regularity_min_peak must be"), (["--regularity_min_pairs", "1"] + on, "--regularity_min_pairs must be"),
                       (["--regularity_min_pairs", "1048577"] + on, "--regularity_min_pairs must be"), (["--gait_fps", "0"] + on, "--gait_fps must be")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv
