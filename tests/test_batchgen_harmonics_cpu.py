"""batch_generation.py --gait_harmonics through the model_factory / gloo seam of the CPU tests, with --harmonics_on_host's path end to
end: it needs --gait; the JSON file with one object per video -- per channel the columns of pipeline.HARMONICS_COLUMNS, the spectrum and the stored
strides, null where a value is undefined, and straight_only -- one summary line per video, the database unchanged, the device method preferred where
the model has one (one call per window on the gait call's events, with --gait_turns' phase as exclude unless --harmonics_all_frames), and every
refusal of the new flags."""
import importlib
import json
import os

import numpy as np
import pytest

from .test_batchgen_gait_cpu import LENGTHS, _StandInWithGait, bg, generate, world  # noqa: F401  (fixtures)
from .test_host_cpu import _stand_in_factory

GAIT = {"on_host": True, "sigma": 1.0, "window": 3, "min_excursion": 0.1}
LOOSE = {"n_harmonics": 4, "min_stride": 6, "max_stride": 30}                      # the stand-in's joints are noise: its strikes lie a few frames apart


def test_harmonics_on_host_writes_the_json(bg, pkg, world, capsys):
    pipe = pkg.pipeline
    plain = generate(bg, world, "plain_har.json", gait=GAIT)
    capsys.readouterr()
    db = generate(bg, world, "smooth.json", gait=GAIT, harmonics={"on_host": True, **LOOSE})
    printed = capsys.readouterr().out
    assert list(db) == list(plain) and all(np.array_equal(db[k], plain[k]) for k in plain)          # the database gains nothing
    path = os.path.join(world["root"], "smooth_harmonics.json")
    text = open(path).read()
    assert "NaN" not in text and "null" in text
    found = json.loads(text)
    names = np.asarray(db["vid_name"])
    assert sorted(found) == sorted(LENGTHS)
    used = 0
    for key in LENGTHS:
        want = pipe.gait_harmonics(db["joints3D"][names == key], db["gait_events"][names == key], fps=20.0, **LOOSE)
        assert list(found[key]) == ["straight_only"] + list(pipe.HARMONICS_CHANNELS) and found[key]["straight_only"] is False
        for c, channel in enumerate(pipe.HARMONICS_CHANNELS):
            got = found[key][channel]
            assert list(got) == list(pipe.HARMONICS_COLUMNS) + ["spectrum", "strides"] and len(got["spectrum"]) == 4
            row = want["per_sequence"][0, c]
            for name, v in zip(pipe.HARMONICS_COLUMNS, row):
                assert (got[name] is None) if np.isnan(v) else (got[name] == float(v)), (key, channel, name)
            assert got["spectrum"] == [{"mean": None if np.isnan(m) else float(m), "sd": None if np.isnan(s) else float(s)} for m, s in want["spectrum"][0, c]]
            assert len(got["strides"]) == min(int(row[0]), 128) and all(list(s) == list(pipe.HARMONICS_STRIDE_COLUMNS) for s in got["strides"])
            for s, w in zip(got["strides"], want["strides"][0, c]):
                assert [s[k] for k in pipe.HARMONICS_STRIDE_COLUMNS] == [None if np.isnan(v) else float(v) for v in w]
            used += int(row[1])
        assert found[key]["bob"]["used"] == 0 and found[key]["bob"]["hr_mean"] is None          # no --trajectory: no bob
    print(f"{used} strides used in the noise")
    assert used > 0
    lines = [ln for ln in printed.splitlines() if ln.startswith("Harmonics:")]
    assert len(lines) == 3 and all(word in lines[1] for word in ("strides used, harmonic ratio of the ankles' separation", "left / right index"))
    assert lines[0].startswith("Harmonics: video S001C001P001R001A001, ") and all(ln.endswith(".") and "pelvis" not in ln and "straight" not in ln for ln in lines)
    assert f"Save gait harmonics of 3 videos to {path}." in printed
    with pytest.raises(ValueError, match="harmonics needs gait"):
        generate(bg, world, "no_gait.json", harmonics={"on_host": True})


class _StandInWithHarmonics(_StandInWithGait):
    """The stand-in with the device methods' signatures (answered by the host statements): every video of the window must arrive in ONE call."""
    seen = []
    phases = []
    events = []

    def gait_parameters(self, *args, **kw):
        out = super().gait_parameters(*args, **kw)
        type(self).events.append(out["events"].numpy().copy())
        return out

    def gait_turns(self, joints3d, events, gait_rows, lengths=None, **kw):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        out = pipe.gait_turns(joints3d.cpu().numpy(), events.cpu().numpy(), gait_rows.cpu().numpy(), lengths=lengths, **kw)
        out["phase"][5:9] = 1                                  # the noise has no turn: mark one
        type(self).phases.append(out["phase"].copy())
        return {k: torch.from_numpy(v) for k, v in out.items()}

    def gait_harmonics(self, joints3d, events, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, n_harmonics=20, derivative=2, min_stride=8, max_stride=60,
                       max_strides=128, joints=None):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).seen.append((None if exclude is None else np.asarray(exclude).copy(), np.asarray(events).copy(), list(lengths), None if trans is None else tuple(trans.shape),
                                fps, sigma, n_harmonics, derivative, min_stride, max_stride, max_strides, tuple(joints3d.shape)))
        out = pipe.gait_harmonics(joints3d.cpu().numpy(), np.asarray(events), lengths, trans, exclude, fps, sigma, n_harmonics, derivative, min_stride, max_stride, max_strides)
        return {k: torch.from_numpy(v) for k, v in out.items()}


def test_model_method_gets_the_window_in_one_call_with_the_events_and_the_turns_phase(bg, pkg, world, tmp_path, capsys):
    seen, phases, events = _StandInWithHarmonics.seen, _StandInWithHarmonics.phases, _StandInWithHarmonics.events
    for all_frames in (False, True):
        seen.clear()
        phases.clear()
        events.clear()
        out = str(tmp_path / f"elsewhere{int(all_frames)}.json")
        bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], f"device_harmonics{int(all_frames)}.json"), max_frames=16, chunk=16,
                        model_factory=lambda r: _StandInWithHarmonics(), backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()},
                        gait={"window": 3, "fps": 25.0}, turns={}, harmonics={"min_stride": 6, "out": out, "all_frames": all_frames})
        assert len(seen) == 1 and len(phases) == 1 and len(events) == 1
        exclude, ev, *rest = seen[0]
        assert rest == [[8, 40, 27], None, 25.0, 0.0, 20, 2, 6, 60, 128, (75, 25, 3)] and np.array_equal(ev, events[0])          # the gait call's fps and events
        found = json.load(open(out))
        assert sorted(found) == sorted(LENGTHS) and all(v["straight_only"] is (not all_frames) for v in found.values())
        if all_frames:
            assert exclude is None
        else:
            assert exclude.dtype == np.int32 and np.array_equal(exclude, phases[0]) and exclude[5:9].tolist() == [1] * 4
    capsys.readouterr()
    seen.clear()
    bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], "device_harmonics_trans.json"), max_frames=16, chunk=16,
                    model_factory=lambda r: _StandInWithHarmonics(), backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()}, gait={"window": 3},
                    trajectory={"joints2d": dict(world["joints2d"]), "on_host": True}, harmonics={"min_stride": 6})
    assert len(seen) == 1 and seen[0][0] is None and seen[0][3] == (75, 3) and seen[0][4] == 20.0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Harmonics:")]
    assert len(lines) == 3 and all("of the pelvis' height" in ln for ln in lines)


def test_main_runs_harmonics_on_host(bg, world, tmp_path, monkeypatch):
    """The flags reach prepare_data: main with the seam's arguments patched in."""
    import joblib
    seen = {}
    real = bg.prepare_data

    def patched(**kw):
        seen.update(kw["harmonics"])
        assert kw["gait"] is not None
        return real(**{**kw, "fv": None, "annos": {k: v.copy() for k, v in world["annos"].items()}, "model_factory": _stand_in_factory, "backend": "gloo", "max_frames": 16})
    monkeypatch.setattr(bg, "prepare_data", patched)
    fv = str(tmp_path / "boxes.pkl")
    joblib.dump(world["annos"], fv)
    outpath = str(tmp_path / "main.json")
    bg.main(["--bbox_path", fv, "--vid_folder", world["vid_folder"], "--outpath", outpath, "--gait", "--gait_on_host", "--gait_window", "3", "--gait_harmonics", "--harmonics_on_host",
             "--harmonics_sigma", "1", "--harmonics_count", "4", "--harmonics_derivative", "1", "--harmonics_min_stride", "6", "--harmonics_all_frames"])
    assert seen == {"sigma": 1.0, "n_harmonics": 4, "derivative": 1, "min_stride": 6, "max_stride": None, "all_frames": True, "on_host": True, "out": None}
    found = json.load(open(str(tmp_path / "main_harmonics.json")))
    assert sorted(found) == sorted(LENGTHS) and os.path.exists(str(tmp_path / "main_gait.json")) and len(found["S002C001P001R001A002"]["sep"]["spectrum"]) == 4


def test_harmonics_flags_are_refused_where_they_do_not_belong(bg):
    base = ["--bbox_path", "a.pkl", "--vid_folder", "v"]
    on = ["--gait", "--gait_harmonics"] + base
    for argv, word in ((["--harmonics_out", "t.json"] + base, "--harmonics_out belongs to --gait_harmonics"),
                       (["--harmonics_sigma", "1"] + base, "--harmonics_sigma belongs to --gait_harmonics"),
                       (["--harmonics_count", "10"] + base, "--harmonics_count belongs to --gait_harmonics"),
                       (["--harmonics_derivative", "1"] + base, "--harmonics_derivative belongs to --gait_harmonics"),
                       (["--harmonics_min_stride", "9"] + base, "--harmonics_min_stride belongs to --gait_harmonics"),
                       (["--harmonics_max_stride", "50"] + base, "--harmonics_max_stride belongs to --gait_harmonics"),
                       (["--gait", "--harmonics_all_frames"] + base, "--harmonics_all_frames belongs to --gait_harmonics"),
                       (["--harmonics_on_host"] + base, "--harmonics_on_host belongs to --gait_harmonics"),
                       (["--gait", "--gait_harmonics", "--bbox_path", "a.pkl"], "needs --vid_folder"), (["--gait_harmonics"] + base, "--gait_harmonics needs --gait"),
                       (["--harmonics_sigma", "17"] + on, "--harmonics_sigma must be"), (["--harmonics_sigma", "nan"] + on, "--harmonics_sigma must be"),
                       (["--harmonics_count", "0"] + on, "--harmonics_count must be"), (["--harmonics_count", "21"] + on, "--harmonics_count must be"),
                       (["--harmonics_count", "34"] + on, "--harmonics_count must be"), (["--harmonics_derivative", "3"] + on, "--harmonics_derivative must be"),
                       (["--harmonics_derivative", "-1"] + on, "--harmonics_derivative must be"), (["--harmonics_min_stride", "5"] + on, "--harmonics_min_stride must be"),
                       (["--harmonics_min_stride", "61"] + on, "--harmonics_min_stride must be"), (["--harmonics_max_stride", "256"] + on, "--harmonics_max_stride must be"),
                       (["--harmonics_max_stride", "7"] + on, "--harmonics_min_stride must be"),
                       (["--harmonics_min_stride", "11", "--harmonics_max_stride", "10"] + on, "--harmonics_min_stride must be")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv
