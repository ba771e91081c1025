"""batch_generation.py --trajectory through the model_factory / gloo seam of the CPU tests, with --trajectory_on_host's path: the
three new database keys, their rows equal to pipeline.fit_translation on the database's own joints and the 2D joints of the candidate whose box
won, one line per video, a video whose frame count differs from its OpenPose length skipped with NaN rows and status 1, the device method used
once per window where the model has one, every refusal of the new flags, and the database of a run without --trajectory unchanged."""
import importlib
import os
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import openpose_files
from .test_host_cpu import _StandInModel, _stand_in_factory

SHORT = "A003_one"                                              # 11 frames of 2D joints, 9 frames of video


@pytest.fixture(scope="module")
def bg():
    sys.path.insert(0, ROOT)
    return importlib.import_module("batch_generation")


@pytest.fixture(scope="module")
def world(bg, pkg, tmp_path_factory):
    """A folder of OpenPose files, a frame folder per video (one of them two frames short), the boxes and joints, and a run without --trajectory."""
    import joblib
    root = str(tmp_path_factory.mktemp("batchgen_trajectory"))
    anno = os.path.join(root, "openpose")
    keys, bad, chosen, _ = openpose_files.write_folder(anno)
    vid_folder = os.path.join(root, "videos")
    g = np.random.Generator(np.random.Philox(key=[49, len(keys)]))
    frames = {}
    for key in keys:
        frames[key] = chosen[key].shape[0] - (2 if key == SHORT else 0)
        os.makedirs(os.path.join(vid_folder, key))
        for fi in range(frames[key]):
            np.save(os.path.join(vid_folder, key, f"{fi:06d}.npy"), g.standard_normal((3, 224, 224)).astype(np.float32))
    annos, joints2d = bg.boxes_from_openpose(anno, on_host=True, return_joints=True)
    assert sorted(joints2d) == keys and all(np.array_equal(joints2d[k], chosen[k]) for k in keys)
    plain = bg.prepare_data(None, vid_folder, os.path.join(root, "plain.json"), max_frames=8, chunk=8, model_factory=_stand_in_factory, backend="gloo",
                            annos={k: v.copy() for k, v in annos.items()})
    return {"root": root, "anno": anno, "vid_folder": vid_folder, "keys": keys, "frames": frames, "annos": annos, "joints2d": joints2d,
            "plain": joblib.load(plain[0])}


def run(bg, world, name, model_factory=_stand_in_factory, **trajectory):
    import joblib
    written = bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], name), max_frames=8, chunk=8, model_factory=model_factory, backend="gloo",
                              annos={k: v.copy() for k, v in world["annos"].items()}, trajectory={"joints2d": world["joints2d"], **trajectory})
    assert len(written) == 1
    return joblib.load(written[0])


def check_db(db, world, pipe, focal_length):
    assert list(db) == ["vid_name", "bbox", "joints3D", "trans", "trans_status", "reproj"]
    N = sum(world["frames"].values())
    assert db["trans"].shape == (N, 3) and db["trans"].dtype == np.float32
    assert db["trans_status"].shape == (N,) and db["trans_status"].dtype == np.uint8
    assert db["reproj"].shape == (N,) and db["reproj"].dtype == np.float32
    for k in ("vid_name", "bbox", "joints3D"):                 # the three keys of a run without the flag, bit for bit
        assert db[k].dtype == world["plain"][k].dtype and np.array_equal(db[k], world["plain"][k]), k
    names = np.asarray(db["vid_name"])
    lines = []
    for key in world["keys"]:
        at = names == key
        assert at.sum() == world["frames"][key]
        if key == SHORT:
            assert np.isnan(db["trans"][at]).all() and np.isnan(db["reproj"][at]).all() and (db["trans_status"][at] == 1).all()
            lines.append(f"Trajectory: skip video {key}, 9 frames here and 11 frames of 2D joints.")
            continue
        want = pipe.fit_translation(db["joints3D"][at], world["joints2d"][key], pipe.BODY25_FROM_KINECTV2, focal_length=focal_length, centre=(960.0, 540.0))
        rows, seq = want["per_frame"], want["per_sequence"][0]
        assert np.array_equal(db["trans"][at], rows[:, :3].astype(np.float32), equal_nan=True), key
        assert np.array_equal(db["trans_status"][at], rows[:, 5].astype(np.uint8)), key
        assert np.array_equal(db["reproj"][at], rows[:, 3].astype(np.float32), equal_nan=True), key
        mean = "none" if np.isnan(seq[2]) else f"{seq[2]:.2f} px"
        lines.append(f"Trajectory: video {key}, {int(seq[0])} frames fitted, {int(seq[1])} filled, mean reprojection error {mean}, path length {seq[3]:.3f} m.")
    return lines


def test_trajectory_adds_three_keys_and_one_line_per_video(bg, pkg, world, capsys):
    capsys.readouterr()
    db = run(bg, world, "traj.json", on_host=True)
    printed = capsys.readouterr().out
    lines = check_db(db, world, pkg.pipeline, float(np.hypot(1920, 1080)))        # the default focal length: the frame's diagonal
    got = [ln for ln in printed.splitlines() if ln.startswith("Trajectory:")]
    assert got[0].startswith("Trajectory: skip") and sorted(got) == sorted(lines)       # the skip is said while the window is put together
    db = run(bg, world, "traj_f.json", on_host=True, focal_length=1200.0)
    check_db(db, world, pkg.pipeline, 1200.0)


class _StandInWithFit(_StandInModel):
    """The stand-in with the device method's signature (answered by the host statement): batch_generation must prefer it."""
    calls = []

    def fit_translation(self, joints3d, joints2d, pairs, lengths=None, focal_length=5000.0, centre=(112.0, 112.0)):
        import torch
        pipe = importlib.import_module("video-based-gait-analysis-for-dementia_amd").pipeline
        type(self).calls.append((list(lengths), tuple(pairs), focal_length, tuple(centre), torch.is_tensor(joints3d), tuple(joints2d.shape), joints2d.dtype))
        out = pipe.fit_translation(joints3d.numpy(), joints2d, pairs, lengths=lengths, focal_length=focal_length, centre=centre)
        return {k: torch.from_numpy(v) for k, v in out.items()}


def test_model_method_is_used_once_per_window_unless_on_host(bg, pkg, world):
    for on_host in (False, True):
        _StandInWithFit.calls.clear()
        db = run(bg, world, f"dev_{int(on_host)}.json", model_factory=lambda r: _StandInWithFit(), on_host=on_host, focal_length=1500.0)
        check_db(db, world, pkg.pipeline, 1500.0)
        if on_host:
            assert _StandInWithFit.calls == []
        else:                                                  # one call, one sequence per video that has its 2D joints
            lengths = [world["frames"][k] for k in world["keys"] if k != SHORT]
            assert _StandInWithFit.calls == [(lengths, pkg.pipeline.BODY25_FROM_KINECTV2, 1500.0, (960.0, 540.0), True, (sum(lengths), 25, 3), np.float32)]


def test_database_without_the_flag_keeps_its_keys(world):
    assert list(world["plain"]) == ["vid_name", "bbox", "joints3D"]
    assert world["plain"]["bbox"].dtype == np.float32 and world["plain"]["joints3D"].dtype == np.float32


def test_trajectory_flags_are_refused_where_they_do_not_belong(bg):
    for argv, word in ((["--trajectory", "--vid_folder", "v"], "needs --openpose_folder"),
                       (["--trajectory", "--openpose_folder", "d", "--bbox_out", "b.pkl"], "--vid_folder"),
                       (["--trajectory", "--bbox_path", "a.pkl", "--vid_folder", "v"], "--bbox_path carries none"),
                       (["--focal_length", "1000", "--bbox_path", "a.pkl", "--vid_folder", "v"], "belong to --trajectory"),
                       (["--trajectory_on_host", "--openpose_folder", "d", "--vid_folder", "v"], "belong to --trajectory"),
                       (["--trajectory", "--focal_length", "-5", "--openpose_folder", "d", "--vid_folder", "v"], "--focal_length must be"),
                       (["--trajectory", "--focal_length", "nan", "--openpose_folder", "d", "--vid_folder", "v"], "--focal_length must be")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv


def test_help_states_the_camera_as_an_assumption(bg, capsys):
    with pytest.raises(SystemExit):
        bg.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--trajectory" in text and "ASSUMPTIONS" in text and "no calibration" in text
