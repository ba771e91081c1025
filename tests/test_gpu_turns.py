"""Turns and straight-walking gait parameters on the GPU (grnet_gait_turns, csrc/gait_turns_kernels.hip) against the host statement
pipeline.gait_turns on the turning walker of tests/helpers/turn_checks.py, at the smallest shapes that can break a stage: sequences of 1, 2, 64, 65
and 130 frames, a turn that straddles frame 64 (two words of the masks), runs on the first and on the last frame, two turns of opposite direction in
one sequence, one and seven sequences a call, a standing body, a degenerate frame, J = 25 and 49 (with another table), max_turns 1 and 8, a sequence
longer than the LDS masks, and the hand-made case through the hook.

Every input has a decision margin >= 1e-6 degrees a second, asserted on the host, so the phases, the turn table's integer columns and every count
are EQUAL; with sigma = 0 both sides run the same operations in the same order and every output bit is equal; with sigma > 0 the device's Gaussian
has its own weights and its own order of the sum, so the rate, the peak and the mean peak are held to the bars derived in turn_checks.py and
everything else stays equal in every bit.  Every worst ratio and margin is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from .helpers import gait_checks as gc
from .helpers import turn_checks as tc

pytestmark = pytest.mark.gpu
FPS = 20.0
PARTS = (("two_turns130", dict(T=130, theta0=0.7, turns=((8, 30, 90.0), (50, 30, -100.0)))),      # the second turn straddles frame 64
         ("one", dict(T=1, theta0=0.2)), ("two", dict(T=2, theta0=0.3, turns=((-1, 3, 60.0),))),
         ("standing64", dict(T=64, theta0=2.0, A=0.02)),
         ("degenerate65", dict(T=65, theta0=-1.1, turns=((4, 24, 120.0),), degenerate=(45,))),
         ("ends130", dict(T=130, theta0=0.1, turns=((-14, 40, -150.0), (104, 40, 150.0)))),       # runs on the first and on the last frame
         ("walk130_back", dict(T=130, theta0=np.pi - 0.4, phi=1.9)))
NAMES, LENGTHS = [name for name, _ in PARTS], [kw["T"] for _, kw in PARTS]


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == ([] if hook else ["per_frame"]) + ["per_sequence", "phase", "turns"]
    assert out["phase"].dtype == torch.int32 and out["turns"].dtype == torch.float64 and out["per_sequence"].dtype == torch.float64
    assert all(v.is_cuda for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def call(J):
    table = gc.KINECTV2 if J == 25 else gc.OTHER49
    made = [tc.turning_walker(J=J, table=table, **kw) for _, kw in PARTS]
    return np.concatenate([m[0] for m in made]), table


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, sigma, max_turns=8):
    """(the gait call's statement, the turns' statement) of the seven sequences, computed once and shared; the margin condition is asserted here."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, table = call(J)
    gait = pipe.gait_parameters(joints, lengths=LENGTHS, fps=FPS, sigma=2.0, joints=table)
    host = pipe.gait_turns(joints, gait["events"], gait["per_frame"], lengths=LENGTHS, fps=FPS, sigma=sigma, max_turns=max_turns, joints=table)
    margin = tc.assert_margin(host["per_frame"], LENGTHS)
    print(f"J {J} sigma {sigma:g}: decision margin {margin:.3g}; turns per sequence {dict(zip(NAMES, host['per_sequence'][:, 0].astype(int).tolist()))}")
    return gait, host


@pytest.mark.parametrize("sigma", (0.0, 2.0, 8.0))
@pytest.mark.parametrize("J,max_turns", ((25, 8), (25, 1), (49, 8)))
def test_seven_sequences_against_the_statement(model, pkg, J, max_turns, sigma):
    joints, table = call(J)
    gait, host = statement(pkg.__name__, J, sigma, max_turns)
    out = numpy_out(model.gait_turns(joints, gait["events"], gait["per_frame"], lengths=LENGTHS, fps=FPS, sigma=sigma, max_turns=max_turns, joints=table))
    raw = statement(pkg.__name__, J, 0.0, max_turns)[1]["per_frame"][:, 1] if sigma > 0 else None
    ratio = tc.compare(out, host, raw, LENGTHS, sigma)
    print(f"J {J} sigma {sigma:g} max_turns {max_turns}: worst error / bar = {ratio:.3g}")
    assert ratio <= 1.0
    seq = dict(zip(NAMES, host["per_sequence"]))
    assert out["turns"].shape == (7, max_turns, 7)
    if sigma <= 2.0:                                            # what the shapes are there for (a Gaussian of 8 frames merges the neighbours of the short clips)
        two = host["turns"][0] if max_turns == 8 else None
        assert seq["two_turns130"][0] == 2 and seq["two_turns130"][1] == 1 and seq["two_turns130"][2] == 1
        assert two is None or (two[0, 2] == 1 and two[1, 2] == -1 and two[1, 0] < 64 < two[1, 1])
        ends = host["phase"][sum(LENGTHS[:5]):sum(LENGTHS[:6])]
        assert seq["ends130"][0] == 2 and ends[0] == (2 if sigma > 0 else 0) and ends[1] == 2 and ends[-1] == 1      # the step of a first frame is +0 by rule 2
        assert seq["degenerate65"][0] == 1 and seq["degenerate65"][4] >= 2 and host["phase"][sum(LENGTHS[:4]) + 45] == 3
    assert seq["standing64"][0] == 0 and seq["standing64"][6] == 64 and seq["walk130_back"][0] == 0 and seq["one"][6] == 1
    for name in ("standing64", "walk130_back"):                # no frame of phase != 0: the straight columns ARE the gait row's
        q = NAMES.index(name)
        assert tc.same_bits(out["per_sequence"][q, 11:24], gait["per_sequence"][q, 4:17]), name


@pytest.mark.parametrize("sigma", (0.0, 8.0))
def test_one_sequence_alone_and_among_six_others(model, pkg, sigma):
    """n_seq = 1 against the statement, and the same rows in the call of seven: equal bits."""
    joints, table = call(25)
    gait, _ = statement(pkg.__name__, 25, sigma)
    whole = numpy_out(model.gait_turns(joints, gait["events"], gait["per_frame"], lengths=LENGTHS, fps=FPS, sigma=sigma))
    again = numpy_out(model.gait_turns(joints, gait["events"], gait["per_frame"], lengths=LENGTHS, fps=FPS, sigma=sigma))
    assert all(tc.same_bits(whole[k], again[k]) for k in ("per_frame", "turns", "per_sequence")) and np.array_equal(whole["phase"], again["phase"])
    a = 0
    for q, n in enumerate(LENGTHS):
        alone = numpy_out(model.gait_turns(joints[a:a + n], gait["events"][a:a + n], gait["per_frame"][a:a + n], fps=FPS, sigma=sigma))
        assert np.array_equal(alone["phase"], whole["phase"][a:a + n]), NAMES[q]
        assert tc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and tc.same_bits(alone["turns"][0], whole["turns"][q]), NAMES[q]
        assert tc.same_bits(alone["per_sequence"][0], whole["per_sequence"][q]), NAMES[q]
        if q == 0:
            host = pkg.pipeline.gait_turns(joints[:n], gait["events"][:n], gait["per_frame"][:n], fps=FPS, sigma=sigma)
            tc.assert_margin(host["per_frame"], [n])
            raw = pkg.pipeline.gait_turns(joints[:n], gait["events"][:n], gait["per_frame"][:n], fps=FPS, sigma=0.0)["per_frame"][:, 1]
            ratio = tc.compare(alone, host, raw if sigma > 0 else None, [n], sigma)
            print(f"n_seq = 1, sigma {sigma:g}: worst error / bar = {ratio:.3g}")
            assert ratio <= 1.0
        a += n


def check_hand(out, max_turns):
    assert out["phase"].tolist() == tc.HAND_PHASE
    assert out["turns"].shape == (1, max_turns, 7) and out["turns"][0, :2].tolist() == tc.HAND_TURNS[:max_turns][:2] and np.isnan(out["turns"][0, 2:]).all()
    row = out["per_sequence"][0]
    assert row[:11].tolist() == tc.HAND_COUNTS
    print(row[11:].tolist())
    assert all(abs(row[c] - v) <= 1e-12 for c, v in tc.HAND_STRAIGHT.items())


def test_hook_on_the_hand_made_case(model, pkg):
    rates, events, rows = tc.hand_case()
    for max_turns in (8, 1):
        out = numpy_out(model.op_gait_turn_runs(rates, events, rows, max_turns=max_turns, **tc.HAND_RULE), hook=True)
        check_hand(out, max_turns)
        host = pkg.pipeline.gait_turn_runs(rates, events, rows, max_turns=max_turns, **tc.HAND_RULE)
        assert np.array_equal(out["phase"], host["phase"]) and tc.same_bits(out["turns"], host["turns"]) and tc.same_bits(out["per_sequence"], host["per_sequence"])
    three = numpy_out(model.op_gait_turn_runs(np.concatenate([rates, rates[:4], rates]), np.concatenate([events, events[:4], events]),
                                              np.concatenate([rows, rows[:4], rows]), lengths=[25, 4, 25], max_turns=8, **tc.HAND_RULE), hook=True)
    assert three["phase"].tolist() == tc.HAND_PHASE + [1, 1, 1, 0] + tc.HAND_PHASE
    assert tc.same_bits(three["turns"][0], three["turns"][2]) and tc.same_bits(three["per_sequence"][0], three["per_sequence"][2]) and three["per_sequence"][1, 0] == 1


def test_two_turns_whose_first_frames_fall_to_one_thread(model, pkg):
    """A thread of the sequence kernel owns the frames t, t + 256, ...: with turns that begin at frames 10 and 266 it walks both runs in stage (b) and has
    kept the later one's peak and angle alone when it writes the rows in stage (c) -- the earlier run is walked again, to the same bits.  The third turn
    begins at another thread's frame 400."""
    T = 600
    rates = np.zeros((T, 2))
    for first, behind, rate, step in ((10, 30, 20.0, 5.25), (266, 290, -30.0, -4.125), (400, 430, 17.0, 2.0625)):
        rates[first:behind] = (step, rate)
    rates[15, 1], rates[280, 1] = 41.5, -52.25                  # the peaks
    events = np.zeros(T, np.int32)
    events[5::11], events[9::11] = 1, 2
    rows = np.zeros((T, 7))
    rows[:, 0], rows[:, 1], rows[:, 4] = np.sin(np.arange(T)), np.cos(np.arange(T)), 0.2
    host = pkg.pipeline.gait_turn_runs(rates, events, rows, max_turns=2)
    assert host["turns"][0, :, 0].tolist() == [10, 266] and host["turns"][0, :, 5].tolist() == [41.5, 52.25] and host["per_sequence"][0, :3].tolist() == [3, 2, 1]
    out = numpy_out(model.op_gait_turn_runs(rates, events, rows, max_turns=2), hook=True)      # the third turn is counted, not stored: its mean terms are walked again
    assert np.array_equal(out["phase"], host["phase"]) and tc.same_bits(out["turns"], host["turns"]) and tc.same_bits(out["per_sequence"], host["per_sequence"])
    assert out["per_sequence"][0, 9] == (41.5 + 52.25 + 17.0) / 3 and out["per_sequence"][0, 8] == (105.0 + 99.0 + 61.875) / 3


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    events = torch.zeros(8, dtype=torch.int32, device="cuda")
    rows = torch.zeros(8, 7, dtype=torch.float64, device="cuda")
    rates = torch.zeros(8, 2, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 2), -7.0, dtype=torch.float64, device="cuda")
    phase = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    turns = torch.full((2, 8, 7), -7.0, dtype=torch.float64, device="cuda")
    per_seq = torch.full((2, 24), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, fps=20.0, sigma=8.0, edge=5.0, peak=15.0, angle=45.0, lo=10, hi=200, most=8, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, events.data_ptr(), rows.data_ptr(), fps, sigma, edge, peak, angle, lo,
                hi, most, per_frame.data_ptr(), phase.data_ptr(), turns.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_turns(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, fps=20.0, edge=5.0, peak=15.0, angle=45.0, lo=10, hi=200, most=8, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, rates.data_ptr(), events.data_ptr(), rows.data_ptr(), off, len(offsets) - 1 if n_seq is None else n_seq, fps, edge, peak, angle, lo, hi, most,
                phase.data_ptr(), turns.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_turn_runs(*args)

    rule = ((dict(edge=-1.0), b"edge_rate"), (dict(edge=nan), b"edge_rate"), (dict(edge=inf), b"edge_rate"), (dict(peak=4.0), b"peak_rate"), (dict(peak=nan), b"peak_rate"),
            (dict(angle=-1.0), b"min_angle"), (dict(angle=nan), b"min_angle"), (dict(angle=inf), b"min_angle"), (dict(lo=0), b"min_frames"), (dict(hi=9), b"max_frames"),
            (dict(most=0), b"max_turns"), (dict(most=65), b"max_turns"), (dict(fps=0.0), b"fps"), (dict(fps=nan), b"fps"), (dict(n_seq=0), b"n_seq 0"),
            (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 6, 7, 16, 17, 18, 19)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"), (dict(sigma=-1.0), b"sigma"),
            (dict(sigma=nan), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(fps=inf), b"fps"), (dict(n_seq=-2), b"n_seq -2")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 2, 3, 4, 13, 14, 15)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((phase == -7).all()) and bool((turns == -7.0).all()) and bool((per_seq == -7.0).all())      # nothing was written
    assert run() == 0
    torch.cuda.synchronize()
    assert bool((phase == 3).all()) and bool(per_frame[[1, 2, 4, 5, 6, 7]].isnan().all()) and bool(turns.isnan().all())      # every joint at (1, 1, 1): no frame has axes
    assert per_seq[:, :7].tolist() == [[0, 0, 0, 0, 3, 0, 0], [0, 0, 0, 0, 5, 0, 0]]
    phase.fill_(-7)
    assert hook() == 0
    torch.cuda.synchronize()
    assert bool((phase == 0).all()) and per_seq[:, :7].tolist() == [[0, 0, 0, 0, 0, 1, 3], [0, 0, 0, 0, 0, 1, 5]]
    ok = np.ones((4, 25, 3), np.float32)
    ev, gr = np.zeros(4, np.int32), np.zeros((4, 7))
    for args, kw, word in (((ok[0], ev, gr), {}, "joints3d"), ((ok, ev, gr), {"lengths": [2, 1]}, "lengths"), ((ok, ev, gr), {"joints": (0, 1, 2)}, "joints"),
                           ((ok, ev[:3], gr), {}, "events"), ((ok, ev, gr[:, :6]), {}, "gait_rows"), ((ok, ev, gr), {"min_frames": 2.5}, "min_frames"),
                           ((ok, ev, gr), {"max_turns": 65}, "max_turns"), ((ok, ev, gr), {"max_turns": 0}, "max_turns")):
        with pytest.raises(ValueError, match=word):
            model.gait_turns(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"fps": 0.0}, "fps"), ({"peak_rate": 1.0}, "peak_rate"), ({"max_frames": 5}, "max_frames")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_turns(ok, ev, gr, **kw)


@pytest.mark.parametrize("sigma", (0.0, 8.0))
def test_a_sequence_longer_than_the_lds_masks(model, pkg, sigma):
    """4200 frames > 64 words of 64: the masks lie in the call's scratch and go through the same code; beside it a short one in LDS, first and last,
    so that the long one's words begin at another bit of the call."""
    T = 4200
    turns = tuple((300 + 400 * k, 60, 180.0 if k % 2 else -170.0) for k in range(9)) + ((4150, 45, 120.0),)
    long_j, _ = tc.turning_walker(T, turns=turns, theta0=1.3)
    short_j, _ = tc.turning_walker(65, turns=((10, 30, 90.0),), theta0=0.2)
    joints, lengths = np.concatenate([short_j, long_j, short_j]), [65, T, 65]
    gait = pkg.pipeline.gait_parameters(joints, lengths=lengths, fps=FPS, sigma=2.0)
    host = pkg.pipeline.gait_turns(joints, gait["events"], gait["per_frame"], lengths=lengths, fps=FPS, sigma=sigma, max_turns=8)
    margin = tc.assert_margin(host["per_frame"], lengths)
    out = numpy_out(model.gait_turns(joints, gait["events"], gait["per_frame"], lengths=lengths, fps=FPS, sigma=sigma, max_turns=8))
    raw = pkg.pipeline.gait_turns(joints, gait["events"], gait["per_frame"], lengths=lengths, fps=FPS, sigma=0.0)["per_frame"][:, 1] if sigma > 0 else None
    ratio = tc.compare(out, host, raw, lengths, sigma)
    print(f"T = {T}, sigma {sigma:g}: decision margin {margin:.3g}, worst error / bar = {ratio:.3g}, {int(host['per_sequence'][1, 0])} turns, "
          f"{int(host['per_sequence'][1, 11])} straight steps of {int(gait['per_sequence'][1, 4])}")
    assert ratio <= 1.0 and host["per_sequence"][1, 0] == 10 and np.isfinite(host["turns"][1]).all()      # ten turns counted, eight stored
    assert host["per_sequence"][1, 1] == 5 and host["per_sequence"][1, 2] == 5 and host["per_sequence"][[0, 2], 0].tolist() == [1, 1]
