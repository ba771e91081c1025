"""batch_generation.py --gait_entropy through the model_factory / gloo seam of the CPU tests: it needs no --gait; the JSON file with one
object per video -- per channel the columns of pipeline.ENTROPY_COLUMNS, per scale the counts and the sample entropy, the complexity index, null
where a value is undefined, and straight_only -- one summary line per video, the database unchanged, --entropy_on_host's path equal to the device
method's (a stand-in answered by the host statement: one call per window, with --gait_turns' phase as exclude unless --entropy_all_frames), and every
refusal of the new flags."""
import importlib
import json
import os

import numpy as np
import pytest

from .test_batchgen_gait_cpu import LENGTHS, _StandInWithGait, bg, generate, world  # noqa: F401  (fixtures)
from .test_host_cpu import _stand_in_factory

LOOSE = {"m": 1, "fraction": 0.5, "derivative": 1, "scales": 2, "min_templates": 10}      # the stand-in's videos have 8, 40 and 27 frames


def test_entropy_on_host_needs_no_gait_and_writes_the_json(bg, pkg, world, capsys):
    pipe = pkg.pipeline
    plain = generate(bg, world, "plain_ent.json")
    capsys.readouterr()
    db = generate(bg, world, "rough.json", entropy={"on_host": True, **LOOSE})
    printed = capsys.readouterr().out
    assert list(db) == list(plain) and all(np.array_equal(db[k], plain[k]) for k in plain)          # the database gains nothing
    path = os.path.join(world["root"], "rough_entropy.json")
    text = open(path).read()
    assert "NaN" not in text and "null" in text
    found = json.loads(text)
    names = np.asarray(db["vid_name"])
    assert sorted(found) == sorted(LENGTHS)
    defined = 0
    for key in LENGTHS:
        want = pipe.gait_entropy(db["joints3D"][names == key], **LOOSE)
        assert list(found[key]) == ["straight_only"] + list(pipe.ENTROPY_CHANNELS) and found[key]["straight_only"] is False
        for c, channel in enumerate(pipe.ENTROPY_CHANNELS):
            got = found[key][channel]
            assert list(got) == list(pipe.ENTROPY_COLUMNS) + ["scales", "complexity"] and len(got["scales"]) == 2
            for name, v in zip(pipe.ENTROPY_COLUMNS, want["per_sequence"][0, c]):
                assert (got[name] is None) if np.isnan(v) else (got[name] == float(v)), (key, channel, name)
            for k, scale in enumerate(got["scales"]):
                assert list(scale) == list(pipe.ENTROPY_COUNTS) + ["sampen"] and [scale[n] for n in pipe.ENTROPY_COUNTS] == want["counts"][0, c, k].tolist()
                v = want["sampen"][0, c, k]
                assert (scale["sampen"] is None) if np.isnan(v) else (scale["sampen"] == float(v))
                defined += not np.isnan(v)
            v = want["complexity"][0, c]
            assert (got["complexity"] is None) if np.isnan(v) else (got["complexity"] == float(v))
        bob = found[key]["bob"]
        assert bob["n"] == 0 and bob["sd"] is None and bob["complexity"] is None and all(s["templates"] == 0 for s in bob["scales"])      # no --trajectory: no bob
    print(f"{defined} sample entropies defined in the noise")
    assert defined > 0
    lines = [ln for ln in printed.splitlines() if ln.startswith("Entropy:")]
    assert len(lines) == 3 and all(word in lines[1] for word in ("templates, sample entropy of the ankles' separation", "complexity index over 2 scales"))
    assert lines[0].startswith("Entropy: video S001C001P001R001A001, 6 templates, sample entropy of the ankles' separation none") and all(ln.endswith(".") for ln in lines)
    assert f"Save gait entropy of 3 videos to {path}." in printed


class _StandInWithEntropy(_StandInWithGait):
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

    def gait_entropy(self, joints3d, lengths=None, trans=None, exclude=None, sigma=0.0, m=2, fraction=0.2, derivative=2, scales=3, joints=None):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).seen.append((None if exclude is None else np.asarray(exclude).copy(), list(lengths), trans, sigma, m, fraction, derivative, scales, tuple(joints3d.shape)))
        out = pipe.gait_entropy(joints3d.cpu().numpy(), lengths, trans, exclude, sigma, m, fraction, derivative, scales)
        return {k: torch.from_numpy(out[k]) for k in ("per_frame", "counts", "per_sequence")}      # the device returns no logarithm


def test_model_method_gets_the_window_in_one_call_and_equals_the_host_path(bg, pkg, world, tmp_path):
    seen, phases = _StandInWithEntropy.seen, _StandInWithEntropy.phases
    files = {}
    for all_frames in (False, True):
        for on_host in (False, True):
            seen.clear()
            phases.clear()
            out = str(tmp_path / f"elsewhere{int(all_frames)}{int(on_host)}.json")
            bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], f"device_entropy{int(all_frames)}{int(on_host)}.json"), max_frames=16, chunk=16,
                            model_factory=lambda r: _StandInWithEntropy(), backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()},
                            gait={"window": 3, "fps": 25.0}, turns={}, entropy={**LOOSE, "out": out, "all_frames": all_frames, "on_host": on_host})
            files[all_frames, on_host] = json.load(open(out))
            assert len(phases) == 1 and len(seen) == (0 if on_host else 1)
            if on_host:
                continue
            exclude, *rest = seen[0]
            assert rest == [[8, 40, 27], None, 0.0, 1, 0.5, 1, 2, (75, 25, 3)]
            found = files[all_frames, on_host]
            assert sorted(found) == sorted(LENGTHS) and all(v["straight_only"] is (not all_frames) for v in found.values())
            if all_frames:
                assert exclude is None and found["S001C001P001R001A001"]["sep"]["n"] == 7
            else:
                assert exclude.dtype == np.int32 and np.array_equal(exclude, phases[0]) and exclude[5:9].tolist() == [1] * 4
                assert found["S001C001P001R001A001"]["sep"]["n"] == 4                                  # frames 5 .. 7 of its 8 do not count: four differences
        assert files[all_frames, True] == files[all_frames, False]                                    # --entropy_on_host equals the device path
    assert files[False, False] != files[True, False]
    seen.clear()
    bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], "device_entropy_alone.json"), max_frames=16, chunk=16,
                    model_factory=lambda r: _StandInWithEntropy(), backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()}, entropy={})
    assert len(seen) == 1 and seen[0][0] is None and seen[0][3:8] == (0.0, 2, 0.2, 2, 3)
    alone = json.load(open(os.path.join(world["root"], "device_entropy_alone_entropy.json")))["S002C001P001R001A002"]
    assert not alone["straight_only"] and len(alone["sep"]["scales"]) == 3 and alone["sep"]["scales"][0]["templates"] == 36 and alone["sep"]["complexity"] is None


def test_main_runs_entropy_on_host(bg, world, tmp_path, monkeypatch):
    """The flags reach prepare_data: main with the seam's arguments patched in, without --gait."""
    import joblib
    seen = {}
    real = bg.prepare_data

    def patched(**kw):
        seen.update(kw["entropy"])
        assert kw["gait"] is None
        return real(**{**kw, "fv": None, "annos": {k: v.copy() for k, v in world["annos"].items()}, "model_factory": _stand_in_factory, "backend": "gloo", "max_frames": 16})
    monkeypatch.setattr(bg, "prepare_data", patched)
    fv = str(tmp_path / "boxes.pkl")
    joblib.dump(world["annos"], fv)
    outpath = str(tmp_path / "main.json")
    bg.main(["--bbox_path", fv, "--vid_folder", world["vid_folder"], "--outpath", outpath, "--gait_entropy", "--entropy_on_host", "--entropy_sigma", "1", "--entropy_m", "1",
             "--entropy_r", "0.5", "--entropy_scales", "2", "--entropy_min_templates", "10", "--entropy_all_frames"])
    assert seen == {"sigma": 1.0, "m": 1, "fraction": 0.5, "derivative": None, "scales": 2, "min_templates": 10, "all_frames": True, "on_host": True, "out": None}
    found = json.load(open(str(tmp_path / "main_entropy.json")))
    assert sorted(found) == sorted(LENGTHS) and not os.path.exists(str(tmp_path / "main_gait.json")) and len(found["S002C001P001R001A002"]["sep"]["scales"]) == 2


def test_entropy_flags_are_refused_where_they_do_not_belong(bg):
    base = ["--bbox_path", "a.pkl", "--vid_folder", "v"]
    on = ["--gait_entropy"] + base
    for argv, word in ((["--entropy_out", "t.json"] + base, "--entropy_out belongs to --gait_entropy"),
                       (["--entropy_sigma", "1"] + base, "--entropy_sigma belongs to --gait_entropy"),
                       (["--entropy_m", "2"] + base, "--entropy_m belongs to --gait_entropy"),
                       (["--entropy_r", "0.2"] + base, "--entropy_r belongs to --gait_entropy"),
                       (["--entropy_derivative", "1"] + base, "--entropy_derivative belongs to --gait_entropy"),
                       (["--entropy_scales", "3"] + base, "--entropy_scales belongs to --gait_entropy"),
                       (["--entropy_min_templates", "30"] + base, "--entropy_min_templates belongs to --gait_entropy"),
                       (["--gait", "--entropy_all_frames"] + base, "--entropy_all_frames belongs to --gait_entropy"),
                       (["--gait_regularity", "--entropy_on_host"] + base, "--entropy_on_host belongs to --gait_entropy"),
                       (["--gait_entropy", "--bbox_path", "a.pkl"], "--gait_entropy needs --vid_folder"),
                       (["--entropy_sigma", "17"] + on, "--entropy_sigma must be"), (["--entropy_sigma", "nan"] + on, "--entropy_sigma must be"),
                       (["--entropy_m", "0"] + on, "--entropy_m must be"), (["--entropy_m", "5"] + on, "--entropy_m must be"),
                       (["--entropy_r", "0"] + on, "--entropy_r must be"), (["--entropy_r", "10.5"] + on, "--entropy_r must be"), (["--entropy_r", "nan"] + on, "--entropy_r must be"),
                       (["--entropy_derivative", "3"] + on, "--entropy_derivative must be"), (["--entropy_derivative", "-1"] + on, "--entropy_derivative must be"),
                       (["--entropy_scales", "0"] + on, "--entropy_scales must be"), (["--entropy_scales", "9"] + on, "--entropy_scales must be"),
                       (["--entropy_min_templates", "0"] + on, "--entropy_min_templates must be")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv
