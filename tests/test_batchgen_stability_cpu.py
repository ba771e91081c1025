"""batch_generation.py --gait_stability through the model_factory / gloo seam of the CPU tests: it needs no --gait; the JSON file with one
object per video -- per channel the curve with n, exponent, mantissa and divergence per k, and lambda, null where a value is undefined, and
straight_only -- one summary line per video, the database unchanged, --stability_on_host's path equal to the device method's (a stand-in answered by
the host statement: one call per window, with --gait_turns' phase as exclude unless --stability_all_frames), and every refusal of the new flags."""
import importlib
import json
import os

import numpy as np
import pytest

from .test_batchgen_gait_cpu import LENGTHS, _StandInWithGait, bg, generate, world  # noqa: F401  (fixtures)
from .test_host_cpu import _stand_in_factory

RULE = {"derivative": 1, "dim": 2, "lag": 1, "theiler": 2, "horizon": 3}       # the stand-in's videos have 8, 40 and 27 frames: 4, 36 and 23 eligible points
LOOSE = {**RULE, "fit_lo": 0, "fit_hi": 3, "min_pairs": 5}


def prepare_with_stability(bg, world, name, **kw):
    return bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], name), max_frames=16, chunk=16, backend="gloo",
                           annos={k: v.copy() for k, v in world["annos"].items()}, **kw)


def test_stability_on_host_needs_no_gait_and_writes_the_json(bg, pkg, world, capsys):
    pipe = pkg.pipeline
    plain = generate(bg, world, "plain_stab.json")
    capsys.readouterr()
    db = generate(bg, world, "apart.json", stability={"on_host": True, **LOOSE})
    printed = capsys.readouterr().out
    assert list(db) == list(plain) and all(np.array_equal(db[k], plain[k]) for k in plain)          # the database gains nothing
    path = os.path.join(world["root"], "apart_stability.json")
    text = open(path).read()
    assert "NaN" not in text and "null" in text
    found = json.loads(text)
    names = np.asarray(db["vid_name"])
    assert sorted(found) == sorted(LENGTHS)
    defined = 0
    for key in LENGTHS:
        want = pipe.gait_stability(db["joints3D"][names == key], **LOOSE)
        assert list(found[key]) == ["straight_only"] + list(pipe.STABILITY_CHANNELS) and found[key]["straight_only"] is False
        for c, channel in enumerate(pipe.STABILITY_CHANNELS):
            got = found[key][channel]
            assert list(got) == ["curve", "lambda"] and len(got["curve"]) == 4
            for k, point in enumerate(got["curve"]):
                assert list(point) == ["n", "exponent", "mantissa", "divergence"] and [point["n"], point["exponent"]] == want["pairs"][0, c, k].tolist()
                assert point["mantissa"] == float(want["mant"][0, c, k])
                v = want["divergence"][0, c, k]
                assert (point["divergence"] is None) if np.isnan(v) else (point["divergence"] == float(v))
            v = want["lambda"][0, c]
            assert (got["lambda"] is None) if np.isnan(v) else (got["lambda"] == float(v))
            defined += not np.isnan(v)
        bob = found[key]["bob"]
        assert bob["lambda"] is None and all(p["n"] == 0 and p["mantissa"] == 1.0 for p in bob["curve"])      # no --trajectory: no bob
    print(f"{defined} exponents defined in the noise")
    assert defined > 0
    lines = [ln for ln in printed.splitlines() if ln.startswith("Stability:")]
    assert len(lines) == 3 and all(word in lines[1] for word in ("pairs of neighbours, divergence exponent of the ankles' separation", "over frames 0 to 3"))
    assert lines[0].startswith("Stability: video S001C001P001R001A001, ") and "separation none a second" in lines[0] and all(ln.endswith(".") for ln in lines)
    assert f"Save gait stability of 3 videos to {path}." in printed


class _StandInWithStability(_StandInWithGait):
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

    def gait_stability(self, joints3d, lengths=None, trans=None, exclude=None, sigma=0.0, derivative=1, dim=5, lag=2, theiler=20, horizon=20, joints=None):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).seen.append((None if exclude is None else np.asarray(exclude).copy(), list(lengths), trans, sigma, derivative, dim, lag, theiler, horizon, tuple(joints3d.shape)))
        out = pipe.gait_stability(joints3d.cpu().numpy(), lengths, trans, exclude, sigma, derivative, dim, lag, theiler, horizon)
        return {k: torch.from_numpy(out[k]) for k in ("per_frame", "nn", "pairs", "mant")}      # the device returns no logarithm


def test_model_method_gets_the_window_in_one_call_and_equals_the_host_path(bg, pkg, world, tmp_path):
    seen, phases = _StandInWithStability.seen, _StandInWithStability.phases
    files = {}
    for all_frames in (False, True):
        for on_host in (False, True):
            seen.clear()
            phases.clear()
            out = str(tmp_path / f"elsewhere{int(all_frames)}{int(on_host)}.json")
            prepare_with_stability(bg, world, f"device_stability{int(all_frames)}{int(on_host)}.json", model_factory=lambda r: _StandInWithStability(),
                                   gait={"window": 3, "fps": 25.0}, turns={}, stability={**LOOSE, "out": out, "all_frames": all_frames, "on_host": on_host})
            files[all_frames, on_host] = json.load(open(out))
            assert len(phases) == 1 and len(seen) == (0 if on_host else 1)
            if on_host:
                continue
            exclude, *rest = seen[0]
            assert rest == [[8, 40, 27], None, 0.0, 1, 2, 1, 2, 3, (75, 25, 3)]
            found = files[all_frames, on_host]
            assert sorted(found) == sorted(LENGTHS) and all(v["straight_only"] is (not all_frames) for v in found.values())
            if all_frames:
                assert exclude is None
            else:
                assert exclude.dtype == np.int32 and np.array_equal(exclude, phases[0]) and exclude[5:9].tolist() == [1] * 4
        assert files[all_frames, True] == files[all_frames, False]                                    # --stability_on_host equals the device path
    assert files[False, False] != files[True, False]
    want = pkg.pipeline.stability_rows(np.array([[p["n"], p["exponent"]] for p in files[True, False]["S002C001P001R001A002"]["sep"]["curve"]]),
                                       np.array([p["mantissa"] for p in files[True, False]["S002C001P001R001A002"]["sep"]["curve"]]), fps=25.0, fit_hi=3, min_pairs=5)
    assert files[True, False]["S002C001P001R001A002"]["sep"]["lambda"] == float(want["lambda"])            # --gait's fps reaches the slope
    seen.clear()
    prepare_with_stability(bg, world, "device_stability_alone.json", model_factory=lambda r: _StandInWithStability(), stability={})
    assert len(seen) == 1 and seen[0][0] is None and seen[0][3:9] == (0.0, 1, 5, 2, 20, 20)
    alone = json.load(open(os.path.join(world["root"], "device_stability_alone_stability.json")))["S002C001P001R001A002"]
    assert not alone["straight_only"] and len(alone["sep"]["curve"]) == 21 and alone["sep"]["lambda"] is None          # 40 frames: 11 eligible points, fewer than 50 pairs


def test_main_runs_stability_on_host(bg, world, tmp_path, monkeypatch):
    """The flags reach prepare_data: main with the seam's arguments patched in, without --gait."""
    import joblib
    seen = {}
    real = bg.prepare_data

    def patched(**kw):
        seen.update(kw["stability"])
        assert kw["gait"] is None and "entropy" not in kw
        return real(**{**kw, "fv": None, "annos": {k: v.copy() for k, v in world["annos"].items()}, "model_factory": _stand_in_factory, "backend": "gloo", "max_frames": 16})
    monkeypatch.setattr(bg, "prepare_data", patched)
    fv = str(tmp_path / "boxes.pkl")
    joblib.dump(world["annos"], fv)
    outpath = str(tmp_path / "main.json")
    bg.main(["--bbox_path", fv, "--vid_folder", world["vid_folder"], "--outpath", outpath, "--gait_stability", "--stability_on_host", "--stability_sigma", "1", "--stability_dim", "2",
             "--stability_lag", "1", "--stability_theiler", "2", "--stability_horizon", "3", "--stability_fit_hi", "3", "--stability_min_pairs", "5", "--stability_all_frames"])
    assert seen == {"sigma": 1.0, "derivative": None, "dim": 2, "lag": 1, "theiler": 2, "horizon": 3, "fit_lo": None, "fit_hi": 3, "min_pairs": 5, "all_frames": True,
                    "on_host": True, "out": None}
    found = json.load(open(str(tmp_path / "main_stability.json")))
    assert sorted(found) == sorted(LENGTHS) and not os.path.exists(str(tmp_path / "main_gait.json")) and len(found["S002C001P001R001A002"]["sep"]["curve"]) == 4


def test_fit_window_follows_a_short_horizon(bg, pkg, world):
    """Without --stability_fit_hi the window ends at 10, or at the horizon where that is shorter, as in the statements; a window outside the horizon is
    refused when the stage is made, before any inference."""
    assert bg.WindowStability(pkg.pipeline, None, True, True).rows["fit_hi"] == 10
    assert bg.WindowStability(pkg.pipeline, None, True, True, horizon=5).rows["fit_hi"] == 5 and bg.WindowStability(pkg.pipeline, None, True, True, horizon=63).rows["fit_hi"] == 10
    for kw in (dict(horizon=5, fit_hi=6), dict(fit_lo=10), dict(fit_lo=-1), dict(fit_lo=3, fit_hi=3)):
        with pytest.raises(ValueError, match="fit window"):
            bg.WindowStability(pkg.pipeline, None, True, True, **kw)
    with pytest.raises(ValueError, match="fit window"):
        prepare_with_stability(bg, world, "refused_window.json", model_factory=_stand_in_factory, stability={"horizon": 5, "fit_hi": 6, "on_host": True})
    assert not os.path.exists(os.path.join(world["root"], "refused_window.json"))
    prepare_with_stability(bg, world, "short_horizon.json", model_factory=_stand_in_factory, stability={**RULE, "horizon": 5, "min_pairs": 5, "on_host": True})
    found = json.load(open(os.path.join(world["root"], "short_horizon_stability.json")))
    assert all(len(v["sep"]["curve"]) == 6 for v in found.values()) and found["S002C001P001R001A002"]["sep"]["lambda"] is not None


def test_stability_flags_are_refused_where_they_do_not_belong(bg):
    base = ["--bbox_path", "a.pkl", "--vid_folder", "v"]
    on = ["--gait_stability"] + base
    alone = tuple(([f"--stability_{name}", value] + base, f"--stability_{name} belongs to --gait_stability") for name, value in (
        ("out", "t.json"), ("sigma", "1"), ("derivative", "1"), ("dim", "5"), ("lag", "2"), ("theiler", "20"), ("horizon", "20"), ("fit_lo", "0"), ("fit_hi", "10"), ("min_pairs", "50")))
    for argv, word in alone + ((["--gait", "--stability_all_frames"] + base, "--stability_all_frames belongs to --gait_stability"),
                               (["--gait_entropy", "--stability_on_host"] + base, "--stability_on_host belongs to --gait_stability"),
                               (["--gait_stability", "--bbox_path", "a.pkl"], "--gait_stability needs --vid_folder"),
                               (["--stability_sigma", "17"] + on, "--stability_sigma must be"), (["--stability_sigma", "nan"] + on, "--stability_sigma must be"),
                               (["--stability_derivative", "3"] + on, "--stability_derivative must be"), (["--stability_derivative", "-1"] + on, "--stability_derivative must be"),
                               (["--stability_dim", "1"] + on, "--stability_dim must be"), (["--stability_dim", "9"] + on, "--stability_dim must be"),
                               (["--stability_lag", "0"] + on, "--stability_lag must be"), (["--stability_lag", "17"] + on, "--stability_lag must be"),
                               (["--stability_theiler", "-1"] + on, "--stability_theiler must be"), (["--stability_theiler", "4097"] + on, "--stability_theiler must be"),
                               (["--stability_horizon", "0"] + on, "--stability_horizon must be"), (["--stability_horizon", "64"] + on, "--stability_horizon must be"),
                               (["--stability_fit_lo", "-1"] + on, "--stability_fit_lo must be"), (["--stability_fit_lo", "10"] + on, "--stability_fit_hi must be"),
                               (["--stability_fit_hi", "21"] + on, "--stability_fit_hi must be"), (["--stability_horizon", "5", "--stability_fit_hi", "6"] + on, "--stability_fit_hi must be"),
                               (["--stability_horizon", "5", "--stability_fit_lo", "5"] + on, "--stability_fit_hi must be"),
                               (["--stability_min_pairs", "0"] + on, "--stability_min_pairs must be")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv
