"""The host path the calls over sequences lying back to back share (csrc/grnet_seq.cpp, csrc/seq_args.h), as batch_generation.py uses it: different
calls on ONE handle and one stream with no synchronise and no download between them.  What can go wrong there and in no single call: the front
of the scratch, which every table upload overwrites with other weights and other offsets; the pinned ring of four slots, which the uploads wrap
several times; and the scratch growing while earlier calls are still in flight (here: at the first gait_kinematics and again at bbox_from_joints2d).
The six gait calls run as batch_generation.py chains them: kinematics, turns, contacts and harmonics on the device tensor of the gait call's events,
turns on its rows too, regularity and harmonics with the turns' phase as exclude.

Expected: every output equals, bit for bit, the same call made alone on a second fresh handle with a synchronise after it.  That is derived, not
a tolerance: the kernels are deterministic (test_gpu_gait.py asserts equal bits for repeated calls), and nothing differs between the two runs but
the host path under test.  The bytes are compared, so a NaN must be the same NaN in the same place."""
import numpy as np
import pytest
import torch

from .helpers import gait_checks as gc
from .helpers import track_checks as tk
from .helpers import turn_checks as tc

pytestmark = pytest.mark.gpu
LENGTHS = [65, 130, 65]


def inputs():
    g = tk.golden()
    made = [tc.turning_walker(T, ((T // 4, 30, 90.0),) if T == 130 else (), theta0=0.37 * q, phi=-3.02 - 0.6137 * q) for q, T in enumerate(LENGTHS)]
    joints = np.concatenate([j for j, _ in made])
    cam = joints.astype(np.float64) + np.array([0.3, 0.1, 6.0])
    seen = np.ones_like(cam)                                    # (x, y, confidence) in pixels: the walker under a camera of f = 1000 at (960, 540)
    seen[:, :, 0] = 1000.0 * cam[:, :, 0] / cam[:, :, 2] + 960.0
    seen[:, :, 1] = 1000.0 * cam[:, :, 1] / cam[:, :, 2] + 540.0
    longer = [tc.turning_walker(4200, theta0=0.2), tc.turning_walker(65, theta0=0.9)]
    long_events = np.zeros(1100 + 65, np.int32)                 # heel strikes every 22 frames, the right foot half a stride behind
    long_events[3::22] |= gc.HEEL_L
    long_events[14::22] |= gc.HEEL_R
    return {"kp": np.concatenate([g["t26gaps_kp"], g["t70_kp"]]), "kp_lengths": [26, 70], "joints": joints, "trans": np.concatenate([t for _, t in made]),
            "shifted": joints + np.float32(0.01) * np.arange(3, dtype=np.float32), "seen": seen.astype(np.float32),
            "pairs": [(k, k) for k in range(25)], "long": np.concatenate([gc.walker(1100, theta=0.2)[0], gc.walker(65, theta=0.9)[0]]),
            "long_events": long_events, "longer": np.concatenate([j for j, _ in longer]), "longer_trans": np.concatenate([t for _, t in longer])}


def run(model, x, alone):
    """The calls in the order of the module's docstring; alone: a synchronise after each.  Returns {call: {name: tensor}}."""
    def done(out):
        if alone:
            torch.cuda.synchronize()
        return out if isinstance(out, dict) else {"out": out}
    r = {}
    # phase 1: eight table uploads through the ring of four slots; neighbours leave other weights and other offsets in the same front
    r["track"] = done(model.track_boxes(x["kp"], lengths=x["kp_lengths"], vis_thresh=tk.VIS_THRESH, kernel_size=11, sigma=3.0))
    r["gait"] = done(model.gait_parameters(x["joints"], lengths=LENGTHS, trans=x["trans"], sigma=2.0))
    r["kinematics"] = done(model.gait_kinematics(x["joints"], r["gait"]["events"], lengths=LENGTHS, sigma=2.0))
    r["turns"] = done(model.gait_turns(x["joints"], r["gait"]["events"], r["gait"]["per_frame"], lengths=LENGTHS, sigma=8.0))
    r["contacts"] = done(model.gait_contacts(x["joints"], r["gait"]["events"], lengths=LENGTHS))
    r["regularity"] = done(model.gait_regularity(x["joints"], lengths=LENGTHS, trans=x["trans"], exclude=r["turns"]["phase"]))
    r["harmonics"] = done(model.gait_harmonics(x["joints"], r["gait"]["events"], lengths=LENGTHS, trans=x["trans"], exclude=r["turns"]["phase"]))
    r["events"] = done(model.op_gait_events(r["gait"]["per_frame"][:, :4], lengths=LENGTHS))
    r["cycles"] = done(model.op_gait_cycles(r["kinematics"]["per_frame"], r["gait"]["events"], lengths=LENGTHS))
    r["median"] = done(model.op_median1d(r["track"]["boxes"][:, 0], lengths=x["kp_lengths"]))
    r["gauss"] = done(model.op_gauss1d(r["track"]["boxes"][:, 1], lengths=x["kp_lengths"], sigma=8.0))
    r["metrics"] = done(model.pose_metrics(x["joints"], x["shifted"], lengths=LENGTHS, root=[0], return_transform=True))
    box, index = model.bbox_from_joints2d(x["kp"], lengths=x["kp_lengths"], return_index=True)
    r["bbox"] = done({"box": box, "index": index})
    r["translation"] = done(model.fit_translation(x["joints"], x["seen"], x["pairs"], lengths=LENGTHS, focal_length=1000.0, centre=(960.0, 540.0)))
    r["gait0"] = done(model.gait_parameters(x["joints"], lengths=LENGTHS, trans=x["trans"], sigma=0.0))
    # phase 2: a sequence of more than 1024 frames keeps its heel-strike bitmasks in the scratch, behind the table, not in LDS
    r["long"] = done(model.gait_kinematics(x["long"], x["long_events"], lengths=[1100, 65], sigma=2.0))
    # and one of more than 4096 frames keeps the event bitmasks of gait_parameters and the strike and validity masks of gait_harmonics there
    r["longer_gait"] = done(model.gait_parameters(x["longer"], lengths=[4200, 65], trans=x["longer_trans"], sigma=2.0))
    r["longer_harmonics"] = done(model.gait_harmonics(x["longer"], r["longer_gait"]["events"], lengths=[4200, 65], trans=x["longer_trans"]))
    return r


GAUSS_LENGTHS = [1, 2, 5, 64, 65, 257, 300]     # shorter than any radius; the wave's edge and one past it; a second pass of the 256 threads; 694 in all
# call -> (its smoothed columns of per_frame, how many of them the walker moves: its ankles and feet alone swing, every other joint is rigid)
GAUSS_COLUMNS = {"gait": (range(0, 4), 4), "kinematics": (range(0, 13), 4), "contacts": (range(1, 4), 2), "regularity": (range(0, 4), 1)}


def test_the_smoothing_of_every_gait_call_is_op_gauss1d(pkg):
    """What the one Gaussian launch of gait_parameters, gait_kinematics, gait_contacts and gait_regularity (seq_gauss_columns_kernel) relies on: a
    call's smoothed column IS op_gauss1d of its unsmoothed column, inside each sequence.  Expected: equal bytes, which is derived and no tolerance --
    both run track_gauss of track_boxes.h on the same values with the same weights in the same order, in a file compiled without contraction.
    Seven sequences of one walker, so that a wrong offset, row width or first column lands in a neighbour; sigma 16 has radius 64, more than
    most of these sequences have frames.  The bytes are compared, so a NaN must be the same NaN in the same place."""
    joints, trans = gc.walker(sum(GAUSS_LENGTHS), theta=0.37)
    assert joints.shape == (694, 25, 3)

    def same(a, b):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    model = pkg.GRNet(max_frames=1)
    try:
        events = model.gait_parameters(joints, lengths=GAUSS_LENGTHS, trans=trans, sigma=0.0)["events"]
        calls = {"gait": lambda s: model.gait_parameters(joints, lengths=GAUSS_LENGTHS, trans=trans, sigma=s),
                 "kinematics": lambda s: model.gait_kinematics(joints, events, lengths=GAUSS_LENGTHS, sigma=s),
                 "contacts": lambda s: model.gait_contacts(joints, events, lengths=GAUSS_LENGTHS, sigma=s),
                 "regularity": lambda s: model.gait_regularity(joints, lengths=GAUSS_LENGTHS, trans=trans, sigma=s)}
        for name, call in calls.items():
            columns, moving = GAUSS_COLUMNS[name]
            raw = call(0.0)["per_frame"]
            assert raw.dtype == torch.float64 and raw.shape[0] == 694
            varies = [k for k in columns if float(raw[:, k].max() - raw[:, k].min()) > 1e-3]
            assert len(varies) >= moving, (name, varies)          # the columns are not constant: a Gaussian of a constant would prove little
            for sigma in (0.5, 2.0, 16.0):
                got = call(sigma)["per_frame"]
                for k in columns:
                    assert same(got[:, k], model.op_gauss1d(raw[:, k], lengths=GAUSS_LENGTHS, sigma=sigma)), (name, sigma, k)
                assert not any(same(got[:, k], raw[:, k]) for k in varies), (name, sigma)       # and the Gaussian did something
                if name == "gait":
                    assert same(got[:, 4], raw[:, 4]), sigma       # the width, which no Gaussian touches
    finally:
        model.close()


def test_calls_in_flight_together_equal_the_same_calls_alone(pkg):
    x = inputs()
    together, alone = pkg.GRNet(max_frames=1), pkg.GRNet(max_frames=1)
    try:
        torch.cuda.synchronize()
        got = run(together, x, alone=False)                     # nothing waits for the device in here
        torch.cuda.synchronize()
        got = {call: {k: v.cpu().numpy() for k, v in out.items()} for call, out in got.items()}
        want = {call: {k: v.cpu().numpy() for k, v in out.items()} for call, out in run(alone, x, alone=True).items()}
    finally:
        together.close()
        alone.close()
    assert len(got) == 18
    for call in want:
        for k, w in want[call].items():
            gk = got[call][k]
            assert gk.shape == w.shape and gk.dtype == w.dtype and w.size > 0, (call, k)
            assert np.array_equal(np.ascontiguousarray(gk).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (call, k, int((gk != w).sum()))
    # the comparison is not empty-handed: the walkers walk, the boxes are boxes
    assert (want["gait"]["events"] != 0).sum() > 20 and (want["gait0"]["events"] != 0).sum() > 20 and (want["events"]["out"] != 0).sum() > 20
    assert np.isfinite(want["kinematics"]["curves"]).any() and np.isfinite(want["cycles"]["curves"]).any() and np.isfinite(want["long"]["curves"][0]).any()
    assert (want["track"]["status"] == 0).sum() > 50 and np.isfinite(want["bbox"]["box"]).all() and np.isfinite(want["metrics"]["total"][:2]).all()
    assert (want["translation"]["per_frame"][:, 5] == 0).all()
    assert want["turns"]["per_sequence"][:, 0].tolist() == [0, 1, 0] and (want["turns"]["phase"] != 0).sum() > 10                 # a turn is found
    assert (want["contacts"]["per_sequence"][:, 3:5].sum(axis=1) > 0).all() and np.isin(want["contacts"]["phase"], (1, 2)).sum() > 10       # a double support is found
    assert want["harmonics"]["per_sequence"][1, 0, 1] > 0 and want["regularity"]["per_sequence"][1, 0, 0] < 130                 # a stride is used; the turn's frames are left out
    assert (want["longer_gait"]["events"][4096:4200] != 0).sum() > 10 and want["longer_harmonics"]["per_sequence"][0, 0, 1] > 100      # events and strides behind frame 4096
