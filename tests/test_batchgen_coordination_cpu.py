"""batch_generation.py --gait_coordination through the model_factory / gloo seam of the CPU tests: it needs no --gait; the JSON file with
one object per video -- the frequency axis, per limb the columns of pipeline.COORDINATION_LIMB_COLUMNS and the amplitude, per pair by name the columns
of pipeline.COORDINATION_PAIR_COLUMNS, the asymmetries, null where a value is undefined, and straight_only -- one summary line per video, the database
unchanged, --coordination_on_host's path equal to the device method's (a stand-in answered by the host statement: one call per window, with
--gait_turns' phase as exclude unless --coordination_all_frames), and every refusal of the new flags."""
import importlib
import json
import os

import numpy as np
import pytest

from .test_batchgen_gait_cpu import LENGTHS, _StandInWithGait, bg, generate, world  # noqa: F401  (fixtures)
from .helpers import spectrum_checks as sc
from .test_host_cpu import _stand_in_factory

LOOSE = {"derivative": 1, "segment": 8, "hop": 2, "nfft": 32, "min_segments": 2}      # the stand-in's videos have 8, 40 and 27 frames
ROWS = ("arm_asymmetry", "leg_asymmetry", "arm_leg_ratio", "phase_deviation_mean")


def test_coordination_on_host_needs_no_gait_and_writes_the_json(bg, pkg, world, capsys):
    pipe = pkg.pipeline
    plain = generate(bg, world, "plain_coord.json")
    capsys.readouterr()
    db = generate(bg, world, "limbs.json", coordination={"on_host": True, **LOOSE})
    printed = capsys.readouterr().out
    assert list(db) == list(plain) and all(np.array_equal(db[k], plain[k]) for k in plain)          # the database gains nothing
    path = os.path.join(world["root"], "limbs_coordination.json")
    text = open(path).read()
    assert "NaN" not in text and "null" in text
    found = json.loads(text)
    names = np.asarray(db["vid_name"])
    assert sorted(found) == sorted(LENGTHS)
    defined = 0
    for key in LENGTHS:
        want = pipe.gait_coordination(db["joints3D"][names == key], **LOOSE)
        assert list(found[key]) == ["straight_only", "freqs"] + list(pipe.COORDINATION_CHANNELS) + list(pipe.COORDINATION_PAIR_NAMES) + list(ROWS)
        assert found[key]["straight_only"] is False and found[key]["freqs"] == want["freqs"].tolist() and len(found[key]["freqs"]) == 17
        for c, limb in enumerate(pipe.COORDINATION_CHANNELS):
            got = found[key][limb]
            assert list(got) == list(pipe.COORDINATION_LIMB_COLUMNS) + ["amplitude"] and len(got) == 14
            for name, v in zip(list(pipe.COORDINATION_LIMB_COLUMNS) + ["amplitude"], want["limbs"][0, c].tolist() + [want["amplitude"][0, c]]):
                assert (got[name] is None) if np.isnan(v) else (got[name] == float(v)), (key, limb, name)
        for p, pair in enumerate(pipe.COORDINATION_PAIR_NAMES):
            got = found[key][pair]
            assert list(got) == list(pipe.COORDINATION_PAIR_COLUMNS) and len(got) == 10
            for name, v in zip(pipe.COORDINATION_PAIR_COLUMNS, want["pairs"][0, p]):
                assert (got[name] is None) if np.isnan(v) else (got[name] == float(v)), (key, pair, name)
            defined += got["coherence_peak"] is not None
        for name in ROWS:
            assert (found[key][name] is None) if np.isnan(want[name][0]) else (found[key][name] == float(want[name][0])), (key, name)
    print(f"{defined} coherences defined in the noise")
    first = found["S001C001P001R001A001"]
    assert defined > 0 and first["arm_left"]["candidates"] == 0 and first["arm_left__arm_right"]["coherence_peak"] is None and first["arm_asymmetry"] is None      # 8 frames: 7 differences
    lines = [ln for ln in printed.splitlines() if ln.startswith("Coordination:")]
    assert len(lines) == 3 and all(word in lines[1] for word in ("segments, arm swing", "(left) and", "(right), asymmetry", "arms: coherence", "legs: coherence", "off antiphase"))
    assert lines[0].startswith("Coordination: video S001C001P001R001A001, 0 segments, arm swing none (left) and none (right), asymmetry none") and all(ln.endswith(".") for ln in lines)
    assert f"Save gait coordination of 3 videos to {path}." in printed


class _StandInWithCoordination(_StandInWithGait):
    """The stand-in with the device methods' signatures (answered by the host statements): every video of the window must arrive in ONE call."""
    seen = []
    phases = []

    def gait_turns(self, joints3d, events, gait_rows, lengths=None, **kw):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        out = pipe.gait_turns(joints3d.cpu().numpy(), events.cpu().numpy(), gait_rows.cpu().numpy(), lengths=lengths, **kw)
        out["phase"][20:24] = 1                                # the noise has no turn: mark one inside the second video (frames 12 .. 15 of its 40)
        type(self).phases.append(out["phase"].copy())
        return {k: torch.from_numpy(v) for k, v in out.items()}

    def gait_coordination(self, joints3d, lengths=None, exclude=None, fps=20.0, sigma=0.0, derivative=0, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0,
                          min_segments=4, joints=None):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).seen.append((None if exclude is None else np.asarray(exclude).copy(), list(lengths), fps, sigma, derivative, segment, hop, nfft, f_lo, f_hi,
                                min_segments, tuple(joints3d.shape)))
        out = pipe.gait_coordination(joints3d.cpu().numpy(), lengths, exclude, fps, sigma, derivative, segment, hop, nfft, f_lo, f_hi, min_segments)
        return {k: torch.from_numpy(out[k]) for k in ("per_frame", "auto", "cross", "limbs", "pairs")}      # the device returns no host rows


def test_model_method_gets_the_window_in_one_call_and_equals_the_host_path(bg, pkg, world, tmp_path, capsys):
    seen, phases = _StandInWithCoordination.seen, _StandInWithCoordination.phases
    files = {}
    for all_frames in (False, True):
        for on_host in (False, True):
            seen.clear()
            phases.clear()
            out = str(tmp_path / f"elsewhere{int(all_frames)}{int(on_host)}.json")
            bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], f"device_coordination{int(all_frames)}{int(on_host)}.json"), max_frames=16, chunk=16,
                            model_factory=lambda r: _StandInWithCoordination(), backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()},
                            gait={"window": 3, "fps": 25.0}, turns={}, coordination={**LOOSE, "out": out, "all_frames": all_frames, "on_host": on_host})
            files[all_frames, on_host] = json.load(open(out))
            assert len(phases) == 1 and len(seen) == (0 if on_host else 1)
            if on_host:
                continue
            exclude, *rest = seen[0]
            assert rest == [[8, 40, 27], 25.0, 0.0, 1, 8, 2, 32, 0.5, 3.0, 2, (75, 25, 3)]          # --gait's fps reaches the call
            found = files[all_frames, on_host]
            assert sorted(found) == sorted(LENGTHS) and all(v["straight_only"] is (not all_frames) for v in found.values())
            second = found["S002C001P001R001A002"]["arm_left"]
            if all_frames:
                assert exclude is None and second["n"] == 39 and second["candidates"] == (39 - 8) // 2 + 1
            else:
                assert exclude.dtype == np.int32 and np.array_equal(exclude, phases[0]) and exclude[20:24].tolist() == [1] * 4
                # the marked turn at its frames 12 .. 15 (and whatever the noise made a turn) splits the video into runs: no segment lies across one
                straight = exclude[8:48] == 0
                y = np.append(np.where(straight[:-1] & straight[1:], 0.0, np.nan), np.nan)
                assert second["n"] == np.isfinite(y).sum() < 35 and second["candidates"] == len(sc.segments_of(y, 8, 2)) < 16
                assert all(found["S002C001P001R001A002"][limb]["n"] == second["n"] for limb in pkg.pipeline.COORDINATION_CHANNELS)      # one mask for all limbs
        assert files[all_frames, True] == files[all_frames, False]                                    # --coordination_on_host equals the device path
    assert files[False, False] != files[True, False]
    assert "straight walking only" in capsys.readouterr().out
    seen.clear()
    bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], "device_coordination_alone.json"), max_frames=16, chunk=16,
                    model_factory=lambda r: _StandInWithCoordination(), backend="gloo", annos={k: v.copy() for k, v in world["annos"].items()}, coordination={})
    assert len(seen) == 1 and seen[0][0] is None and seen[0][2:11] == (20.0, 0.0, 0, 64, 32, 256, 0.5, 3.0, 4)
    alone = json.load(open(os.path.join(world["root"], "device_coordination_alone_coordination.json")))["S002C001P001R001A002"]
    assert not alone["straight_only"] and len(alone["freqs"]) == 129 and alone["arm_left"]["n"] == 40 and alone["arm_left"]["used"] == 0 and alone["arm_left"]["amplitude"] is None


def test_main_runs_coordination_on_host(bg, world, tmp_path, monkeypatch):
    """The flags reach prepare_data: main with the seam's arguments patched in, without --gait but with its --gait_fps."""
    import joblib
    seen = {}
    real = bg.prepare_data

    def patched(**kw):
        seen.update(kw["coordination"])
        assert kw["gait"] is None
        return real(**{**kw, "fv": None, "annos": {k: v.copy() for k, v in world["annos"].items()}, "model_factory": _stand_in_factory, "backend": "gloo", "max_frames": 16})
    monkeypatch.setattr(bg, "prepare_data", patched)
    fv = str(tmp_path / "boxes.pkl")
    joblib.dump(world["annos"], fv)
    outpath = str(tmp_path / "main.json")
    bg.main(["--bbox_path", fv, "--vid_folder", world["vid_folder"], "--outpath", outpath, "--gait_coordination", "--coordination_on_host", "--coordination_sigma", "1",
             "--coordination_segment", "8", "--coordination_hop", "2", "--coordination_nfft", "32", "--coordination_f_lo", "1", "--coordination_f_hi", "12",
             "--coordination_min_segments", "2", "--coordination_all_frames", "--gait_fps", "25"])
    assert seen == {"fps": 25.0, "sigma": 1.0, "derivative": None, "segment": 8, "hop": 2, "nfft": 32, "f_lo": 1.0, "f_hi": 12.0, "min_segments": 2, "all_frames": True,
                    "on_host": True, "out": None}
    found = json.load(open(str(tmp_path / "main_coordination.json")))
    assert sorted(found) == sorted(LENGTHS) and not os.path.exists(str(tmp_path / "main_gait.json")) and found["S002C001P001R001A002"]["freqs"][1] == 25.0 / 32
    assert found["S002C001P001R001A002"]["arm_left"]["used"] == (40 - 8) // 2 + 1


def test_coordination_flags_are_refused_where_they_do_not_belong(bg):
    base = ["--bbox_path", "a.pkl", "--vid_folder", "v"]
    on = ["--gait_coordination"] + base
    belongs = tuple(([f"--coordination_{name}", value] + base, f"--coordination_{name} belongs to --gait_coordination")
                    for name, value in (("out", "t.json"), ("sigma", "1"), ("derivative", "1"), ("segment", "64"), ("hop", "32"), ("nfft", "256"), ("f_lo", "0.5"), ("f_hi", "3"),
                                        ("min_segments", "4")))
    for argv, word in belongs + ((["--gait", "--coordination_all_frames"] + base, "--coordination_all_frames belongs to --gait_coordination"),
                                 (["--gait_spectrum", "--coordination_on_host"] + base, "--coordination_on_host belongs to --gait_coordination"),
                                 (["--gait_fps", "25"] + base, "--gait_fps belongs to --gait"),
                                 (["--gait_coordination", "--bbox_path", "a.pkl"], "--gait_coordination needs --vid_folder"),
                                 (["--gait_coordination", "--openpose_folder", "d", "--bbox_out", "b.pkl"], "--gait_coordination needs --vid_folder"),      # before any box is made
                                 (["--coordination_hop", "32", "--openpose_folder", "d", "--bbox_out", "b.pkl"], "--coordination_hop belongs to --gait_coordination"),
                                 (["--coordination_sigma", "17"] + on, "--coordination_sigma must be"), (["--coordination_sigma", "nan"] + on, "--coordination_sigma must be"),
                                 (["--coordination_derivative", "3"] + on, "--coordination_derivative must be"), (["--coordination_derivative", "-1"] + on, "--coordination_derivative must be"),
                                 (["--coordination_segment", "6"] + on, "--coordination_segment must be"), (["--coordination_segment", "63"] + on, "--coordination_segment must be"),
                                 (["--coordination_segment", "258"] + on, "--coordination_segment must be"), (["--coordination_hop", "7"] + on, "--coordination_hop must be"),
                                 (["--coordination_hop", "65"] + on, "--coordination_hop must be"), (["--coordination_nfft", "62"] + on, "--coordination_nfft must be"),
                                 (["--coordination_nfft", "255"] + on, "--coordination_nfft must be"), (["--coordination_nfft", "1026"] + on, "--coordination_nfft must be"),
                                 (["--coordination_f_lo", "0"] + on, "--coordination_f_lo and --coordination_f_hi must obey"),
                                 (["--coordination_f_lo", "3"] + on, "--coordination_f_lo and --coordination_f_hi must obey"),
                                 (["--coordination_f_hi", "10.5"] + on, "--coordination_f_lo and --coordination_f_hi must obey"),
                                 (["--coordination_f_hi", "nan"] + on, "--coordination_f_lo and --coordination_f_hi must obey"),
                                 (["--coordination_f_hi", "6", "--gait_fps", "10"] + on, "--coordination_f_lo and --coordination_f_hi must obey"),
                                 (["--coordination_min_segments", "1"] + on, "--coordination_min_segments must be"),
                                 (["--coordination_min_segments", "0"] + on, "--coordination_min_segments must be")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv
