"""Footprints, centre of mass and margin of stability on the GPU (grnet_gait_balance, csrc/gait_balance_kernels.hip) against the host
statement pipeline.gait_balance on the planted-foot walker of tests/helpers/contact_checks.py.  The arithmetic is + - * / sqrt in float64 in fixed
orders, so EVERY OUTPUT BIT IS EQUAL, NaN patterns included: there is no tolerance anywhere in this file.  The shapes: one sequence of 70 frames
(strikes on either side of the 64-frame word seam); sequences of 130, 4, 400 and 3 frames back to back (none, one and many strikes, shorter than
the window); 50 sequences of mixed lengths with yaws, NaN frames and a standing walker, one of them alone; 6 000 frames with a strike every 5 frames
(past kBalanceLdsStrikes: the list of marks lies in the call's scratch); max_steps = 4; both segment tables; the hook on the hand-made case; every
refusal; WindowBalance on a real handle after WindowGait."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

from .helpers import balance_checks as bc
from .helpers import contact_checks as cc
from .helpers import gait_checks as gc

pytestmark = pytest.mark.gpu
FPS = bc.FPS
CASE_B = (130, 4, 400, 3)


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out):
    assert sorted(out) == ["per_frame", "per_sequence", "steps"] and all(v.is_cuda and v.dtype == torch.float64 for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def case_a():
    P, beta, speed = cc.WALKERS[0]
    return cc.planted_walker(70, P, beta, speed, 1.3, 0.7), [70]             # strikes in the frames 53 and 64: the step between them spans the seam


@functools.lru_cache(maxsize=None)
def case_b():
    made = [cc.planted_walker(T, *cc.WALKERS[i % 4], 0.3 + i, 0.4 * i) for i, T in enumerate(CASE_B)]
    return np.concatenate(made), list(CASE_B)


@functools.lru_cache(maxsize=None)
def case_c():
    """50 sequences: lengths, walkers and yaws by turns, a NaN left ankle in every seventh, a standing body as sequence 20."""
    lengths = [(40, 70, 130, 64, 65, 3, 200, 1, 90, 128)[i % 10] for i in range(50)]
    made = []
    for i, T in enumerate(lengths):
        P, beta, speed = cc.WALKERS[i % 4]
        made.append(cc.planted_walker(T, P, beta, speed, 0.3 + 1.7 * i, 0.37 * i, nan_frames=(T // 2,) if i % 7 == 3 else (), still=i == 20))
    return np.concatenate(made), lengths


@functools.lru_cache(maxsize=None)
def case_d():
    """6 000 frames, P = 10: the left foot lands in the frames 0, 10, ..., the right one in 5, 15, ... (the gait call's window of 5 frames a side
    cannot tell strikes 5 frames apart, so the events are laid where the walker's feet land)."""
    joints = cc.planted_walker(6000, 10.0, 0.62, 1.2, 0.3, 0.9)
    events = np.zeros(6000, np.int32)
    events[0::10], events[5::10] = 1, 2
    return joints, events


@functools.lru_cache(maxsize=None)
def statement(pkg_name, case, segments=None, max_steps=256):
    """(events, the statement's result) of a case, computed once and shared."""
    pipe = importlib.import_module(pkg_name).pipeline
    if case == "d":
        joints, events = case_d()
        lengths = [6000]
    else:
        joints, lengths = {"a": case_a, "b": case_b, "c": case_c}[case]()
        events = pipe.gait_parameters(joints, lengths=lengths, fps=FPS)["events"]
        if case == "b":
            events[CASE_B[0] + 1] = 1                            # the gait call finds no strike in 4 frames: one is laid there, a strike without a pair
    kw = {} if segments is None else {"segments": segments}
    return events, pipe.gait_balance(joints, events, lengths=lengths, fps=FPS, max_steps=max_steps, **kw)


def test_a_strikes_on_either_side_of_the_word_seam(model, pkg):
    joints, lengths = case_a()
    events, host = statement(pkg.__name__, "a")
    strikes = np.flatnonzero(events & 3)
    assert (strikes < 64).any() and (strikes >= 64).any() and host["per_sequence"][0, 1] == len(strikes) - 1 >= 3, strikes
    bc.compare(numpy_out(model.gait_balance(joints, events, fps=FPS)), host, "A: ")


def test_b_none_one_and_many_strikes(model, pkg):
    joints, lengths = case_b()
    events, host = statement(pkg.__name__, "b")
    print("B: strikes, steps, chains, strides:", host["per_sequence"][:, :4].tolist())
    assert host["per_sequence"][1, :2].tolist() == [1, 0] and host["per_sequence"][3, :2].tolist() == [0, 0] and host["per_sequence"][2, 1] >= 20
    bc.compare(numpy_out(model.gait_balance(joints, events, lengths=lengths, fps=FPS)), host, "B: ")


def test_c_fifty_sequences_and_one_of_them_alone(model, pkg):
    joints, lengths = case_c()
    events, host = statement(pkg.__name__, "c")
    assert host["per_sequence"][20, 1] == 0 and (host["per_sequence"][:, 2] >= 2).any()          # the standing body; a NaN breaks a chain somewhere
    out = numpy_out(model.gait_balance(joints, events, lengths=lengths, fps=FPS))
    bc.compare(out, host, "C: ")
    q = 26                                                       # 200 frames, from the middle
    a = sum(lengths[:q])
    alone = numpy_out(model.gait_balance(joints[a:a + lengths[q]], events[a:a + lengths[q]], fps=FPS))
    assert host["per_sequence"][q, 1] >= 10
    assert bc.same_bits(alone["per_frame"], out["per_frame"][a:a + lengths[q]]) and bc.same_bits(alone["steps"][0], out["steps"][q])
    assert bc.same_bits(alone["per_sequence"][0], out["per_sequence"][q])


def test_d_more_strikes_than_the_lds_list(model, pkg):
    joints, events = case_d()
    _, host = statement(pkg.__name__, "d", None, 1024)
    print("D: strikes, steps, chains, strides:", host["per_sequence"][0, :4].tolist())
    assert host["per_sequence"][0, 0] == 1200 and host["per_sequence"][0, 1] >= 1190
    bc.compare(numpy_out(model.gait_balance(joints, events, fps=FPS, max_steps=1024)), host, "D: ")


def test_e_more_steps_than_the_table_stores(model, pkg):
    joints, lengths = case_b()
    events, host = statement(pkg.__name__, "b", None, 4)
    many = statement(pkg.__name__, "b")[1]
    assert bc.same_bits(host["per_sequence"], many["per_sequence"]) and bc.same_bits(host["steps"], many["steps"][:, :4]) and host["steps"].shape == (4, 4, 15)
    bc.compare(numpy_out(model.gait_balance(joints, events, lengths=lengths, fps=FPS, max_steps=4)), host, "E: ")


@pytest.mark.parametrize("segments", (None, bc.ONE_SEGMENT))
def test_f_both_segment_tables(model, pkg, segments):
    joints, lengths = case_b()
    events, host = statement(pkg.__name__, "b", segments)
    kw = {} if segments is None else {"segments": segments}
    bc.compare(numpy_out(model.gait_balance(joints, events, lengths=lengths, fps=FPS, **kw)), host, "F: ")
    if segments is None:
        assert len(pkg.pipeline.BALANCE_SEGMENTS_KINECTV2) == 14


def test_g_hook_on_the_hand_made_case(model, pkg):
    rel, events, frame = bc.hand_case()
    for max_steps in (8, 2):
        out = numpy_out(model.op_gait_balance_steps(rel, events, max_steps=max_steps, **bc.HAND_RULE))
        keep = min(max_steps, 5)
        assert bc.same_bits(out["steps"][0, :keep], bc.HAND_STEPS[:keep]) and np.isnan(out["steps"][0, keep:]).all()
        assert bc.same_bits(out["per_sequence"][0], bc.HAND_ROW) and bc.same_bits(out["per_frame"], frame)
        bc.compare(out, pkg.pipeline.gait_balance_steps(rel, events, max_steps=max_steps, **bc.HAND_RULE), "G: ")
    three = numpy_out(model.op_gait_balance_steps(np.concatenate([rel, rel[:4], rel]), np.concatenate([events, events[:4], events]), lengths=[32, 4, 32],
                                                  max_steps=8, **bc.HAND_RULE))
    assert bc.same_bits(three["steps"][[0, 2]], [bc.HAND_STEPS + [[bc.NAN] * 15] * 3] * 2)
    assert bc.same_bits(three["per_sequence"][[0, 2]], [bc.HAND_ROW] * 2) and three["per_sequence"][1, :3].tolist() == [2, 0, 0]


def test_h_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    events = torch.zeros(8, dtype=torch.int32, device="cuda")
    rel = torch.zeros(8, 9, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 8), -7.0, dtype=torch.float64, device="cuda")
    steps = torch.full((2, 4, 15), -7.0, dtype=torch.float64, device="cuda")
    per_seq = torch.full((2, 24), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")
    default = np.asarray(pkg.pipeline.BALANCE_SEGMENTS_KINECTV2)

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, seg=default, n_seg=None, fps=20.0, gravity=9.81, window=4, settle=1, hi=30, most=4, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        pairs = np.ascontiguousarray(np.asarray(seg)[:, :2], np.int32)
        weights = np.ascontiguousarray(np.asarray(seg, np.float64)[:, 2:])
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, events.data_ptr(), pairs.ctypes.data_as(C.POINTER(C.c_int32)),
                weights.ctypes.data_as(C.POINTER(C.c_double)), len(pairs) if n_seg is None else n_seg, fps, gravity, window, settle, hi, most, per_frame.data_ptr(),
                steps.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_balance(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, fps=20.0, gravity=9.81, window=4, settle=1, hi=30, most=4, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, rel.data_ptr(), events.data_ptr(), off, len(offsets) - 1 if n_seq is None else n_seq, fps, gravity, window, settle, hi, most, per_frame.data_ptr(),
                steps.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_balance_steps(*args)

    def with_row(row):
        return np.vstack([default[:3], [row], default[4:]])

    rule = ((dict(fps=0.0), b"fps"), (dict(fps=nan), b"fps"), (dict(fps=inf), b"fps"), (dict(gravity=0.0), b"gravity"), (dict(gravity=-9.81), b"gravity"),
            (dict(gravity=nan), b"gravity"), (dict(gravity=inf), b"gravity"), (dict(window=0), b"window"), (dict(window=17), b"window"), (dict(settle=-1), b"settle"),
            (dict(settle=5), b"settle"), (dict(hi=0), b"max_step"), (dict(most=0), b"max_steps"), (dict(most=1025), b"max_steps"), (dict(n_seq=0), b"n_seq 0"),
            (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 6, 7, 8, 16, 17, 18)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"), (dict(n_seq=-2), b"n_seq -2"),
            (dict(n_seg=0), b"n_seg"), (dict(n_seg=17), b"n_seg"), (dict(seg=with_row((4, 25, 0.028, 0.436))), b"segment joint"),
            (dict(seg=with_row((-1, 5, 0.028, 0.436))), b"segment joint"), (dict(seg=with_row((4, 5, 0.0, 0.436))), b"segment mass"),
            (dict(seg=with_row((4, 5, -0.1, 0.436))), b"segment mass"), (dict(seg=with_row((4, 5, nan, 0.436))), b"segment mass"),
            (dict(seg=with_row((4, 5, inf, 0.436))), b"segment mass"), (dict(seg=with_row((4, 5, 0.028, nan))), b"segment fraction"),
            (dict(seg=with_row((4, 5, 0.028, inf))), b"segment fraction")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 2, 3, 11, 12, 13)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((steps == -7.0).all()) and bool((per_seq == -7.0).all())      # nothing was written
    assert run() == 0
    torch.cuda.synchronize()
    assert bool(steps.isnan().all()) and per_seq[:, :4].tolist() == [[0, 0, 0, 0]] * 2 and bool(per_seq[:, 4:].isnan().all())       # no events: no strike
    assert bool((per_frame[:, :3] == 1.0).all()) and bool(per_frame[:, 3:6].isnan().all()) and bool((per_frame[:, 6] == 0).all())     # every joint at (1, 1, 1)
    per_seq.fill_(-7.0)
    assert hook() == 0
    torch.cuda.synchronize()
    assert per_seq[:, :4].tolist() == [[0, 0, 0, 0]] * 2 and bool((per_frame[:, :3] == 0).all())
    ok = np.ones((4, 25, 3), np.float32)
    ev = np.zeros(4, np.int32)
    for args, kw, word in (((ok[0], ev), {}, "joints3d"), ((ok, ev), {"lengths": [2, 1]}, "lengths"), ((ok, ev), {"joints": (0, 1, 2)}, "joints"), ((ok, ev[:3]), {}, "events"),
                           ((ok, ev), {"window": 1.5}, "window"), ((ok, ev), {"max_steps": 1025}, "max_steps"), ((ok, ev), {"max_steps": 0}, "max_steps"),
                           ((ok, ev), {"segments": ((0, 20, 1.0),)}, "segments"), ((ok, ev), {"segments": ((0.5, 20, 1.0, 0.5),)}, "segments")):
        with pytest.raises(ValueError, match=word):
            model.gait_balance(*args, **kw)
    for kw, word in (({"fps": 0.0}, "fps"), ({"gravity": 0.0}, "gravity"), ({"window": 17}, "window"), ({"settle": 5}, "settle"), ({"max_step": 0}, "max_step"),
                     ({"segments": ((0, 25, 1.0, 0.5),)}, "segment joint")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_balance(ok, ev, **kw)


def test_i_window_balance_on_a_real_handle(model, pkg):
    """WindowBalance after WindowGait's call, on the device and on the host: equal videos, and footprints_phase is column 6."""
    import batch_generation as bg
    joints, lengths = case_b()
    lengths = lengths[:3]
    joints = joints[:sum(lengths)]
    j3 = torch.from_numpy(joints).cuda()
    gait = model.gait_parameters(j3, lengths=lengths, fps=FPS)
    keys = [f"v{i}" for i in range(3)]
    videos = []
    for on_host in (False, True):
        w = bg.WindowBalance(pkg.pipeline, model, on_host, fps=FPS)
        assert (w.device_call is None) == on_host
        phases = w.add_window(keys, j3, lengths, gait["events"])
        assert [p.shape for p in phases] == [(T,) for T in lengths] and all(p.dtype == np.int8 for p in phases)
        videos.append((w.videos, phases))
    assert videos[0][0] == videos[1][0] and all(np.array_equal(a, b) for a, b in zip(videos[0][1], videos[1][1]))
    host = pkg.pipeline.gait_balance(joints, gait["events"].cpu().numpy(), lengths=lengths, fps=FPS)
    assert np.array_equal(np.concatenate(videos[0][1]), host["per_frame"][:, 6].astype(np.int8))
    assert videos[0][0]["v2"]["steps"] == int(host["per_sequence"][2, 1]) and len(videos[0][0]["v2"]["step_table"]) == int(host["per_sequence"][2, 1])
