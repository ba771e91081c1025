"""batch_generation.py --gait --gait_bootstrap through the model_factory / gloo seam of the CPU tests, with --bootstrap_on_host's path:
the JSON file's schema -- per video and parameter estimate, lo, median, hi, replicates and n, the step and stride tables, the cadence labelled as
derived -- null where a value is not finite, nothing new in the database, one summary line per video, the streams (0 and 1; 2 and 3 straight-only
with turns; 4 on the balance table), the device methods preferred where the model has them, and every refusal of the new flags."""
import importlib
import json
import os

import numpy as np
import pytest

from .test_batchgen_balance_cpu import LOOSE, _StandInWithBalance
from .test_batchgen_gait_cpu import LENGTHS, bg, generate, world  # noqa: F401  (fixtures)
from .test_host_cpu import _stand_in_factory

GAIT = {"on_host": True, "sigma": 1.0, "window": 3, "min_excursion": 0.1}
BOOT = {"on_host": True, "replicates": 200, "level": 90.0, "block": 2, "seed": 7}
FIELDS = ["estimate", "lo", "median", "hi", "replicates", "n"]


def test_bootstrap_on_host_writes_the_json_and_no_column(bg, pkg, world, capsys):
    pipe = pkg.pipeline
    walk = generate(bg, world, "walk_plain.json", gait=dict(GAIT))
    assert not os.path.exists(os.path.join(world["root"], "walk_plain_bootstrap.json"))
    capsys.readouterr()
    db = generate(bg, world, "bars.json", gait=dict(GAIT), bootstrap=dict(BOOT))
    printed = capsys.readouterr().out
    assert list(db) == list(walk) and all(np.array_equal(db[k], walk[k]) for k in walk)                # the database gains nothing
    path = os.path.join(world["root"], "bars_bootstrap.json")
    text = open(path).read()
    assert "NaN" not in text and "Infinity" not in text and "null" in text
    found = json.loads(text)
    names = np.asarray(db["vid_name"])
    assert sorted(found) == sorted(LENGTHS)
    some = 0
    for key in LENGTHS:
        joints = db["joints3D"][names == key]
        gait = pipe.gait_parameters(joints, fps=20.0, sigma=1.0, window=3, min_excursion=0.1)
        tables = pipe.gait_step_tables(gait["events"], gait["per_frame"], fps=20.0)
        video = found[key]
        assert list(video) == ["replicates", "level", "block", "seed", "method", "parameters", "cadence", "truncated", "step_table", "stride_table"]
        assert video["truncated"] == {}
        assert (video["replicates"], video["level"], video["block"], video["seed"], video["method"]) == (200, 90.0, 2, 7, "percentile")
        par = video["parameters"]
        assert list(par) == [f"{name}_{stat}" for name in ("step_time", "step_length", "step_width", "stride_time") for stat in ("mean", "sd", "cv")]
        assert all(list(p) == FIELDS for p in par.values())
        for c, name in ((3, "step_time"), (4, "step_length"), (5, "step_width")):
            want = pipe.bootstrap_table(tables["steps"], tables["counts"][:, 0], [c], B=200, block=2, seed=7, stream=0, quantiles=(500, 5000, 9500))["out"][0, 0]
            for s, stat in enumerate(("mean", "sd", "cv")):
                got = par[f"{name}_{stat}"]
                assert [got[f] for f in FIELDS[:4]] == [float(v) if np.isfinite(v) else None for v in want[s, [0, 2, 3, 4]]], (key, name, stat)
                assert got["replicates"] == int(want[s, 1]) and got["n"] == int(tables["counts"][0, 0])
        want = pipe.bootstrap_table(tables["strides"], tables["counts"][:, 1], [3], B=200, block=2, seed=7, stream=1, quantiles=(500, 5000, 9500))["out"][0, 0]
        assert par["stride_time_mean"]["estimate"] == (None if np.isnan(want[0, 0]) else float(want[0, 0])) and par["stride_time_cv"]["replicates"] == int(want[2, 1])
        # replicate 0 is what the gait call reports
        row = gait["per_sequence"][0]
        for name, c in (("step_time_mean", 5), ("step_time_sd", 6), ("stride_time_mean", 8), ("stride_time_sd", 9), ("stride_time_cv", 10), ("step_length_mean", 11),
                        ("step_length_sd", 12), ("step_width_mean", 13), ("step_width_sd", 14)):
            assert par[name]["estimate"] == (None if np.isnan(row[c]) else float(row[c])), (key, name)
        assert len(video["step_table"]) == int(row[4]) == tables["counts"][0, 0] and len(video["stride_table"]) == tables["counts"][0, 1]
        assert all(list(step) == list(pipe.STEP_TABLE_COLUMNS) for step in video["step_table"]) and all(list(s) == list(pipe.STRIDE_TABLE_COLUMNS) for s in video["stride_table"])
        cadence, step = video["cadence"], par["step_time_mean"]
        assert list(cadence) == ["estimate", "lo", "hi", "derived"] and "60 / step_time_mean" in cadence["derived"]
        if step["estimate"]:
            some += 1
            assert cadence["estimate"] == 60.0 / step["estimate"] == row[7] and cadence["lo"] == 60.0 / step["hi"] and cadence["hi"] == 60.0 / step["lo"]
            assert step["lo"] <= step["median"] <= step["hi"] and cadence["lo"] <= cadence["hi"]
        else:
            assert cadence["estimate"] is None and step["replicates"] == 0 and step["n"] == 0
    assert some >= 2 and found["S001C001P001R001A001"]["parameters"]["stride_time_mean"] == dict(zip(FIELDS, [None, None, None, None, 0, 0]))      # 8 frames: no event
    lines = [ln for ln in printed.splitlines() if ln.startswith("Bootstrap:")]
    assert len(lines) == 3 and all(word in lines[1] for word in ("stride time", "stride-time CV", "90 % percentile intervals of 200 replicates over"))
    assert lines[0].startswith("Bootstrap: video S001C001P001R001A001, stride time none") and all(ln.endswith(".") for ln in lines)
    assert f"Save bootstrap intervals of 3 videos to {path}." in printed
    with pytest.raises(ValueError, match="bootstrap needs gait"):
        generate(bg, world, "alone.json", bootstrap={"on_host": True})
    for bad, word in (({"replicates": 0}, "replicates"), ({"replicates": 4097}, "replicates"), ({"level": 100.0}, "level"), ({"level": 0.0}, "level")):
        with pytest.raises(ValueError, match=word):
            generate(bg, world, "bad.json", gait=dict(GAIT), bootstrap={"on_host": True, **bad})


def test_with_turns_and_balance_the_other_streams_run(bg, pkg, world):
    pipe = pkg.pipeline
    db = generate(bg, world, "all.json", gait=dict(GAIT), turns={"on_host": True}, balance={"on_host": True, **LOOSE}, bootstrap={"on_host": True, "replicates": 100})
    found = json.load(open(os.path.join(world["root"], "all_bootstrap.json")))
    names = np.asarray(db["vid_name"])
    key = "S002C001P001R001A002"
    par = found[key]["parameters"]
    base = [f"{name}_{stat}" for name in ("step_time", "step_length", "step_width", "stride_time") for stat in ("mean", "sd", "cv")]
    assert list(par) == base + ["straight_" + n for n in base] + [f"{name}_{stat}" for name in bg.WindowBootstrap.BALANCE_NAMES for stat in ("mean", "sd", "cv")]
    joints = db["joints3D"][names == key]
    gait = pipe.gait_parameters(joints, fps=20.0, sigma=1.0, window=3, min_excursion=0.1)
    turns = pipe.gait_turns(joints, gait["events"], gait["per_frame"], fps=20.0)
    straight = pipe.gait_step_tables(gait["events"], gait["per_frame"], fps=20.0, phase=turns["phase"], straight_only=True)
    want = pipe.bootstrap_table(straight["strides"], straight["counts"][:, 1], [3], B=100, stream=3, quantiles=(250, 5000, 9750))["out"][0, 0]
    got = par["straight_stride_time_mean"]
    assert [got[f] for f in FIELDS[:4]] == [float(v) if np.isfinite(v) else None for v in want[0, [0, 2, 3, 4]]] and got["replicates"] == int(want[0, 1])
    assert got["estimate"] == (None if np.isnan(turns["per_sequence"][0, 15]) else float(turns["per_sequence"][0, 15]))
    stepped = 0
    for key in LENGTHS:                                         # the balance table: the loose rule finds a step in one of the noise videos
        joints = db["joints3D"][names == key]
        events = pipe.gait_parameters(joints, fps=20.0, sigma=1.0, window=3, min_excursion=0.1)["events"]
        bal = pipe.gait_balance(joints, events, fps=20.0, **LOOSE)
        want = pipe.bootstrap_table(bal["steps"], bal["per_sequence"][:, 1].astype(np.int32), [7, 8, 9, 11, 12], B=100, stream=4, quantiles=(250, 5000, 9750))["out"][0]
        par = found[key]["parameters"]
        for i, name in enumerate(bg.WindowBootstrap.BALANCE_NAMES):
            for s, stat in enumerate(("mean", "sd", "cv")):
                got = par[f"{name}_{stat}"]
                assert [got[f] for f in FIELDS[:4]] == [float(v) if np.isfinite(v) else None for v in want[i, s, [0, 2, 3, 4]]], (key, name, stat)
                assert got["n"] == int(bal["per_sequence"][0, 1]) and got["replicates"] == int(want[i, s, 1])
        if bal["per_sequence"][0, 1] > 0:
            stepped += 1
            assert par["mos_ml_mean"]["estimate"] == float(bal["per_sequence"][0, 16]) and par["mos_ap_mean"]["estimate"] == float(bal["per_sequence"][0, 14])
    assert stepped >= 1


def test_more_rows_than_the_table_stores_are_named(bg, pkg, capsys):
    """max_rows = 4 on a walker of some 10 steps: the first four rows are resampled, n says 4, and the file and a line say how many were found."""
    from .helpers import gait_checks as gc
    pipe = pkg.pipeline
    joints = gc.walker(130, theta=0.7)[0]
    gait = pipe.gait_parameters(joints, fps=20.0)
    w = bg.WindowBootstrap(pipe, None, True, replicates=50, max_rows=4)
    w.add_window(["v"], [130], gait["events"], gait["per_frame"])
    video, steps, strides = w.videos["v"], int(gait["per_sequence"][0, 4]), int(gait["per_sequence"][0, 0] + gait["per_sequence"][0, 1]) - 2
    assert steps > 4 and video["truncated"] == {**{name: {"found": steps, "n": 4} for name in bg.WindowBootstrap.STEP_NAMES}, "stride_time": {"found": strides, "n": 4}}
    assert video["parameters"]["step_time_mean"]["n"] == 4 and len(video["step_table"]) == 4
    want = pipe.bootstrap_table(pipe.gait_step_tables(gait["events"], gait["per_frame"], max_rows=4)["steps"], [4], [3], B=1, quantiles=())["out"][0, 0, 0, 0]
    assert video["parameters"]["step_time_mean"]["estimate"] == float(want) != gait["per_sequence"][0, 5]
    printed = capsys.readouterr().out
    assert f"step_time has {steps} rows of which the first 4 are resampled" in printed and "not the whole clip's columns." in printed


class _StandInWithBootstrap(_StandInWithBalance):
    """The stand-in with the two device methods' signatures (answered by the host statements): the tables are made of the very tensors the gait call
    returned, and the balance table's count arrives as int32."""
    tables, boots = [], []

    def gait_step_tables(self, events, per_frame, lengths=None, fps=20.0, max_rows=256, phase=None, straight_only=False):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).tables.append((events, per_frame, list(lengths), fps, max_rows, phase is not None, straight_only))
        out = pipe.gait_step_tables(events.cpu().numpy(), per_frame.cpu().numpy(), lengths, fps, max_rows, None if phase is None else phase.cpu().numpy(), straight_only)
        return {k: torch.from_numpy(v) for k, v in out.items()}

    def bootstrap_table(self, table, counts, cols, B=2000, block=1, seed=0, stream=0, quantiles=(250, 5000, 9750), return_replicates=False):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).boots.append((tuple(table.shape), counts.dtype, tuple(cols), B, block, seed, stream, tuple(quantiles)))
        return {"out": torch.from_numpy(pipe.bootstrap_table(table.cpu().numpy(), counts.cpu().numpy(), cols, B, block, seed, stream, quantiles)["out"])}


def test_model_methods_get_the_gait_calls_tensors_and_the_streams(bg, pkg, world, tmp_path):
    import torch
    _StandInWithBootstrap.tables.clear(), _StandInWithBootstrap.boots.clear(), _StandInWithBootstrap.returned.clear(), _StandInWithBootstrap.seen.clear()
    out = str(tmp_path / "elsewhere.json")
    bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], "device_boot.json"), max_frames=16, chunk=16, model_factory=lambda r: _StandInWithBootstrap(),
                    backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()}, gait={"window": 3, "fps": 25.0}, balance=dict(LOOSE),
                    bootstrap={"replicates": 50, "out": out})
    assert len(_StandInWithBootstrap.tables) == 1 and len(_StandInWithBootstrap.returned) == 1
    events, rows, *rest = _StandInWithBootstrap.tables[0]
    assert events is _StandInWithBootstrap.returned[0]["events"] and rows is _StandInWithBootstrap.returned[0]["per_frame"]
    assert rest == [[8, 40, 27], 25.0, 256, False, False]      # the gait call's fps; no turns: no phase
    q = (250, 5000, 9750)
    assert _StandInWithBootstrap.boots == [((3, 256, 6), torch.int32, (3, 4, 5), 50, 1, 0, 0, q), ((3, 256, 4), torch.int32, (3,), 50, 1, 0, 1, q),
                                           ((3, 256, 15), torch.int32, (7, 8, 9, 11, 12), 50, 1, 0, 4, q)]
    assert sorted(json.load(open(out))) == sorted(LENGTHS) and not os.path.exists(os.path.join(world["root"], "device_boot_bootstrap.json"))


def test_main_runs_bootstrap_on_host(bg, world, tmp_path, monkeypatch):
    """The flags reach prepare_data: main with the seam's arguments patched in."""
    import joblib
    seen = {}
    real = bg.prepare_data

    def patched(**kw):
        seen.update(kw["bootstrap"])
        return real(**{**kw, "fv": None, "annos": {k: v.copy() for k, v in world["annos"].items()}, "model_factory": _stand_in_factory, "backend": "gloo", "max_frames": 16})
    monkeypatch.setattr(bg, "prepare_data", patched)
    fv = str(tmp_path / "boxes.pkl")
    joblib.dump(world["annos"], fv)
    outpath = str(tmp_path / "main.json")
    bg.main(["--bbox_path", fv, "--vid_folder", world["vid_folder"], "--outpath", outpath, "--gait", "--gait_on_host", "--gait_bootstrap", "--bootstrap_on_host",
             "--bootstrap_replicates", "64", "--bootstrap_level", "80", "--bootstrap_seed", "3"])
    assert seen == {"replicates": 64, "level": 80.0, "block": None, "seed": 3, "on_host": True, "out": None}
    found = json.load(open(str(tmp_path / "main_bootstrap.json")))
    assert sorted(found) == sorted(LENGTHS) and all(v["replicates"] == 64 and v["level"] == 80.0 and v["block"] == 1 for v in found.values())
    assert list(joblib.load(str(tmp_path / "main_0.json"))) == ["vid_name", "bbox", "joints3D", "gait_events"]


def test_bootstrap_flags_are_refused_where_they_do_not_belong(bg):
    base = ["--bbox_path", "a.pkl", "--vid_folder", "v"]
    both = ["--gait", "--gait_bootstrap"] + base
    for argv, word in ((["--gait_bootstrap"] + base, "--gait_bootstrap belongs to --gait"), (["--gait", "--bootstrap_out", "t.json"] + base, "--bootstrap_out belongs to --gait_bootstrap"),
                       (["--gait", "--bootstrap_replicates", "100"] + base, "--bootstrap_replicates belongs to --gait_bootstrap"),
                       (["--gait", "--bootstrap_level", "90"] + base, "--bootstrap_level belongs to --gait_bootstrap"),
                       (["--gait", "--bootstrap_block", "2"] + base, "--bootstrap_block belongs to --gait_bootstrap"),
                       (["--gait", "--bootstrap_seed", "1"] + base, "--bootstrap_seed belongs to --gait_bootstrap"),
                       (["--bootstrap_on_host"] + base, "--bootstrap_on_host belongs to --gait_bootstrap"),
                       (["--bootstrap_replicates", "0"] + both, "--bootstrap_replicates must be"), (["--bootstrap_replicates", "-5"] + both, "--bootstrap_replicates must be"),
                       (["--bootstrap_replicates", "4097"] + both, "--bootstrap_replicates must be"), (["--bootstrap_level", "0"] + both, "--bootstrap_level must"),
                       (["--bootstrap_level", "100"] + both, "--bootstrap_level must"), (["--bootstrap_level", "nan"] + both, "--bootstrap_level must"),
                       (["--bootstrap_block", "0"] + both, "--bootstrap_block must be"), (["--bootstrap_block", "1025"] + both, "--bootstrap_block must be"),
                       (["--bootstrap_seed", "-1"] + both, "--bootstrap_seed must be")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv
