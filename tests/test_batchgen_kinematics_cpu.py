"""batch_generation.py --gait --gait_kinematics through the model_factory / gloo seam of the CPU tests, with --kinematics_on_host's
path: the JSON file with one object per video -- per channel of pipeline.KINEMATICS_CHANNELS the six columns of pipeline.KINEMATICS_COLUMNS plus
curve_mean and curve_sd, 101 numbers each, null where a value is undefined -- one summary line per video, the database unchanged, the device
method preferred where the model has one (one call per window, on the events the gait call returned), and every refusal of the new flags."""
import importlib
import json
import os

import numpy as np
import pytest

from .test_batchgen_gait_cpu import LENGTHS, _StandInWithGait, bg, generate, world  # noqa: F401  (fixtures)
from .test_host_cpu import _stand_in_factory

GAIT = {"on_host": True, "sigma": 1.0, "window": 3, "min_excursion": 0.1}


def test_kinematics_on_host_writes_the_json(bg, pkg, world, capsys):
    pipe = pkg.pipeline
    walk = generate(bg, world, "walk_only.json", gait=dict(GAIT))
    assert not os.path.exists(os.path.join(world["root"], "walk_only_kinematics.json"))
    capsys.readouterr()
    db = generate(bg, world, "angles.json", gait=dict(GAIT), kinematics={"on_host": True, "sigma": 1.0, "min_stride": 2, "max_stride": 30})
    printed = capsys.readouterr().out
    assert list(db) == list(walk) and all(np.array_equal(db[k], walk[k]) for k in db)          # the database gains nothing
    path = os.path.join(world["root"], "angles_kinematics.json")
    text = open(path).read()
    assert "NaN" not in text and "null" in text
    found = json.loads(text)
    names = np.asarray(db["vid_name"])
    assert sorted(found) == sorted(LENGTHS)
    used = {}
    for key in LENGTHS:
        want = pipe.gait_kinematics(db["joints3D"][names == key], db["gait_events"][names == key], sigma=1.0, min_stride=2, max_stride=30)
        assert list(found[key]) == list(pipe.KINEMATICS_CHANNELS)
        for c, name in enumerate(pipe.KINEMATICS_CHANNELS):
            entry = found[key][name]
            assert list(entry) == list(pipe.KINEMATICS_COLUMNS) + ["curve_mean", "curve_sd"] and len(entry["curve_mean"]) == len(entry["curve_sd"]) == 101
            got = [entry[col] for col in pipe.KINEMATICS_COLUMNS] + entry["curve_mean"] + entry["curve_sd"]
            ref = list(want["per_sequence"][0, c]) + list(want["curves"][0, c, :, 0]) + list(want["curves"][0, c, :, 1])
            assert all((g is None) if np.isnan(r) else (g == float(r)) for g, r in zip(got, ref)), (key, name)
        used[key] = [int(found[key][name]["strides"]) for name in pipe.KINEMATICS_CHANNELS]
    print(f"strides used {used}")
    short = found["S001C001P001R001A001"]                       # shorter than a window on either side: no events, nothing used
    assert all(short[name]["strides"] == 0.0 and short[name]["rom_mean"] is None and short[name]["curve_mean"] == [None] * 101 for name in short)
    assert max(used["S002C001P001R001A002"]) > 0 and found["S002C001P001R001A002"]["trunk_inclination"]["symmetry_index"] is None
    lines = [ln for ln in printed.splitlines() if ln.startswith("Kinematics:")]
    assert len(lines) == 3 and lines[0].startswith("Kinematics: video S001C001P001R001A001, knee ROM none / none, arm swing ROM none / none (symmetry index none), "
                                                   "mean trunk inclination ")
    assert all(word in lines[1] for word in ("knee ROM", "arm swing ROM", "symmetry index", "mean trunk inclination")) and lines[1].endswith(" deg.")
    assert f"Save gait kinematics of 3 videos to {path}." in printed
    with pytest.raises(ValueError, match="kinematics needs gait"):
        generate(bg, world, "alone.json", kinematics={"on_host": True})


class _StandInWithKinematics(_StandInWithGait):
    """The stand-in with both device methods' signatures (answered by the host statements): every video of the window must arrive in ONE call, with the
    very events the gait call returned."""
    seen = []
    returned = []

    def gait_parameters(self, *args, **kw):
        out = super().gait_parameters(*args, **kw)
        type(self).returned.append(out["events"])
        return out

    def gait_kinematics(self, joints3d, events, lengths=None, sigma=2.0, min_stride=8, max_stride=60, joints=None):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).seen.append((events, list(lengths), sigma, min_stride, max_stride, tuple(joints3d.shape)))
        out = pipe.gait_kinematics(joints3d.cpu().numpy(), events.cpu().numpy(), lengths, sigma, min_stride, max_stride)
        return {k: torch.from_numpy(v) for k, v in out.items()}


def test_model_method_gets_the_window_in_one_call_with_the_events(bg, pkg, world, tmp_path):
    _StandInWithKinematics.seen.clear()
    _StandInWithKinematics.returned.clear()
    out = str(tmp_path / "elsewhere.json")
    bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], "device_kin.json"), max_frames=16, chunk=16, model_factory=lambda r: _StandInWithKinematics(),
                    backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()}, gait={"window": 3}, kinematics={"min_stride": 3, "out": out})
    assert len(_StandInWithKinematics.seen) == 1 and len(_StandInWithKinematics.returned) == 1
    events, lengths, sigma, lo, hi, shape = _StandInWithKinematics.seen[0]
    assert events is _StandInWithKinematics.returned[0] and (lengths, sigma, lo, hi, shape) == ([8, 40, 27], 2.0, 3, 60, (75, 25, 3))
    assert sorted(json.load(open(out))) == sorted(LENGTHS) and not os.path.exists(os.path.join(world["root"], "device_kin_kinematics.json"))


def test_main_runs_kinematics_on_host(bg, world, tmp_path, monkeypatch):
    """The flags reach prepare_data: main with the seam's arguments patched in."""
    import joblib
    seen = {}
    real = bg.prepare_data

    def patched(**kw):
        seen.update(kw["kinematics"])
        return real(**{**kw, "fv": None, "annos": {k: v.copy() for k, v in world["annos"].items()}, "model_factory": _stand_in_factory, "backend": "gloo", "max_frames": 16})
    monkeypatch.setattr(bg, "prepare_data", patched)
    fv = str(tmp_path / "boxes.pkl")
    joblib.dump(world["annos"], fv)
    outpath = str(tmp_path / "main.json")
    bg.main(["--bbox_path", fv, "--vid_folder", world["vid_folder"], "--outpath", outpath, "--gait", "--gait_on_host", "--gait_kinematics", "--kinematics_on_host",
             "--kinematics_min_stride", "4", "--kinematics_sigma", "0"])
    assert seen == {"sigma": 0.0, "min_stride": 4, "max_stride": None, "on_host": True, "out": None}
    assert sorted(json.load(open(str(tmp_path / "main_kinematics.json")))) == sorted(LENGTHS) and os.path.isfile(str(tmp_path / "main_gait.json"))


def test_kinematics_flags_are_refused_where_they_do_not_belong(bg):
    base = ["--bbox_path", "a.pkl", "--vid_folder", "v"]
    both = ["--gait", "--gait_kinematics"] + base
    for argv, word in ((["--gait_kinematics"] + base, "--gait_kinematics belongs to --gait"), (["--gait", "--kinematics_out", "k.json"] + base, "--kinematics_out belongs to --gait_kinematics"),
                       (["--gait", "--kinematics_sigma", "2"] + base, "--kinematics_sigma belongs to --gait_kinematics"),
                       (["--gait", "--kinematics_min_stride", "8"] + base, "--kinematics_min_stride belongs to --gait_kinematics"),
                       (["--gait", "--kinematics_max_stride", "60"] + base, "--kinematics_max_stride belongs to --gait_kinematics"),
                       (["--kinematics_on_host"] + base, "--kinematics_on_host belongs to --gait_kinematics"),
                       (["--kinematics_sigma", "17"] + both, "--kinematics_sigma must be"), (["--kinematics_sigma", "-1"] + both, "--kinematics_sigma must be"),
                       (["--kinematics_sigma", "nan"] + both, "--kinematics_sigma must be"), (["--kinematics_min_stride", "0"] + both, "--kinematics_min_stride and"),
                       (["--kinematics_min_stride", "61"] + both, "--kinematics_min_stride and"), (["--kinematics_max_stride", "4097"] + both, "--kinematics_min_stride and"),
                       (["--kinematics_max_stride", "7"] + both, "--kinematics_min_stride and")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv
