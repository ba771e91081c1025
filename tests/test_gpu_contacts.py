"""Foot contact phases and double support on the GPU (grnet_gait_contacts, csrc/gait_contacts_kernels.hip) against the host statement
pipeline.gait_contacts on the planted-foot walker of tests/helpers/contact_checks.py, at the smallest shapes that can break a stage: sequences of 1,
2, 3, 64, 65, 66 and 130 frames, a double support that straddles interval 64 (two words of the masks), a run over the intervals 62 to 66 and runs at
the intervals 63 and 64 alone through the hook, one and seven sequences a call, a standing body, a NaN ankle frame, the hopper of DESIGN 4.11 whose
feet strike together, J = 25 and 49 (with another table), max_runs 2 and 128, a fixed speed in place of the relative threshold, a sequence longer
than the LDS masks, and the hand-made case through the hook.

Every input has a decision margin >= 1e-9 m/s, asserted on the host, so the phases, the attributions and every count are EQUAL; with sigma = 0 both
sides run the same operations in the same order and every output bit is equal; with sigma > 0 the device's Gaussian has its own weights and its own
order of the sum, so the vectors, the speeds, the edges and the row are held to the bars derived in contact_checks.py.  Every worst ratio and margin
is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from .helpers import contact_checks as cc
from .helpers import gait_checks as gc

pytestmark = pytest.mark.gpu
FPS = cc.FPS
# the planted walker's arguments; "hopper64" is gait_checks.walker(right=0.8).  walk130's left heel strikes near frame 62.6, so the double support it
# opens lies across interval 64's word boundary
PARTS = (("walk130", dict(T=130, P=21.7, beta=0.62, speed=1.2, phi=-62.6, theta=0.7)), ("one", dict(T=1, theta=0.2)), ("two", dict(T=2, theta=0.3)),
         ("three", dict(T=3, theta=0.4, phi=1.3)), ("hopper64", dict(T=64, theta=0.4, right=0.8)),
         ("nan65", dict(T=65, P=19.3, beta=0.60, speed=1.5, phi=2.2, theta=-1.1, nan_frames=(28,))),
         ("walk66_back", dict(T=66, P=27.3, beta=0.66, speed=0.6, phi=1.9, theta=np.pi - 0.4)))
NAMES, LENGTHS = [name for name, _ in PARTS], [kw["T"] for _, kw in PARTS]
STANDING = dict(T=64, theta=2.0, still=True)                   # with a fixed speed alone: nothing lies below a quarter of a mean of zero, by no margin


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == ([] if hook else ["per_frame"]) + ["per_sequence", "phase", "runs"]
    assert out["phase"].dtype == torch.int32 and out["runs"].dtype == torch.float64 and out["per_sequence"].dtype == torch.float64
    assert all(v.is_cuda for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def call(J):
    """(joints, table, lengths, names) of the seven sequences of one call."""
    table = gc.KINECTV2 if J == 25 else gc.OTHER49
    made = [gc.walker(J=J, table=table, **kw)[0] if name == "hopper64" else cc.planted_walker(J=J, table=table, **kw) for name, kw in PARTS]
    return np.concatenate(made), table, LENGTHS, NAMES


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, sigma, max_runs=128):
    """(the gait call's statement, the contacts' statement) of the sequences, computed once and shared; the margin condition is asserted here."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, table, _, _ = call(J)
    gait = pipe.gait_parameters(joints, lengths=LENGTHS, fps=FPS, sigma=0.0, joints=table)
    host = pipe.gait_contacts(joints, gait["events"], lengths=LENGTHS, fps=FPS, sigma=sigma, max_runs=max_runs, joints=table)
    margin = cc.assert_margin(host, LENGTHS)
    print(f"J {J} sigma {sigma:g}: decision margin {margin:.3g}; runs per sequence {dict(zip(NAMES, host['per_sequence'][:, 2].astype(int).tolist()))}, "
          f"attributed {(host['per_sequence'][:, 3] + host['per_sequence'][:, 4]).astype(int).tolist()}")
    return gait, host


@pytest.mark.parametrize("sigma", (0.0, 1.0, 2.0))
@pytest.mark.parametrize("J,max_runs", ((25, 128), (25, 2), (49, 128)))
def test_sequences_against_the_statement(model, pkg, J, max_runs, sigma):
    joints, table, _, _ = call(J)
    gait, host = statement(pkg.__name__, J, sigma, max_runs)
    out = numpy_out(model.gait_contacts(joints, gait["events"], lengths=LENGTHS, fps=FPS, sigma=sigma, max_runs=max_runs, joints=table))
    raw = statement(pkg.__name__, J, 0.0, max_runs)[1]["per_frame"][:, 1:] if sigma > 0 else None
    ratio = cc.compare(out, host, raw, LENGTHS, sigma)
    print(f"J {J} sigma {sigma:g} max_runs {max_runs}: worst error / bar = {ratio:.3g}")
    assert ratio <= 1.0 and out["runs"].shape == (len(LENGTHS), max_runs, 6)
    seq = dict(zip(NAMES, host["per_sequence"]))
    for name in ("one", "two", "three"):                       # three frames hold no closed run
        assert seq[name][3] == 0 and seq[name][4] == 0 and np.isnan(seq[name][6:11]).all(), name
    assert np.isnan(seq["one"][:2]).all() and seq["one"][2] == 0
    if sigma == 0:                                              # what the shapes are there for
        runs = statement(pkg.__name__, J, 0.0, 128)[1]["runs"]
        assert any(r[0] < 63.5 < r[1] and r[2] != 0 for r in runs[0]), "no double support of walk130 lies across interval 64's word boundary"
        assert seq["walk130"][3] >= 4 and seq["walk130"][4] >= 4 and seq["walk130"][11] >= 6 and seq["walk66_back"][3] + seq["walk66_back"][4] >= 3
        assert seq["hopper64"][2] >= 2 and seq["hopper64"][3] == 0 and seq["hopper64"][4] == 0          # struck by both feet: unattributed
        nan = host["phase"][sum(LENGTHS[:5]):sum(LENGTHS[:6])]
        assert np.flatnonzero(nan == 4).tolist() == [27, 28, 64] and seq["nan65"][3] + seq["nan65"][4] >= 3


@pytest.mark.parametrize("sigma", (0.0, 1.0))
def test_one_sequence_alone_and_among_six_others(model, pkg, sigma):
    """n_seq = 1 against the statement, and the same rows in the call of all: equal bytes."""
    joints, table, _, _ = call(25)
    gait, _ = statement(pkg.__name__, 25, sigma)
    whole = numpy_out(model.gait_contacts(joints, gait["events"], lengths=LENGTHS, fps=FPS, sigma=sigma))
    again = numpy_out(model.gait_contacts(joints, gait["events"], lengths=LENGTHS, fps=FPS, sigma=sigma))
    assert all(cc.same_bits(whole[k], again[k]) for k in ("per_frame", "runs", "per_sequence")) and np.array_equal(whole["phase"], again["phase"])
    a = 0
    for q, n in enumerate(LENGTHS):
        alone = numpy_out(model.gait_contacts(joints[a:a + n], gait["events"][a:a + n], fps=FPS, sigma=sigma))
        assert np.array_equal(alone["phase"], whole["phase"][a:a + n]), NAMES[q]
        assert cc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and cc.same_bits(alone["runs"][0], whole["runs"][q]), NAMES[q]
        assert cc.same_bits(alone["per_sequence"][0], whole["per_sequence"][q]), NAMES[q]
        if q == 0:
            host = pkg.pipeline.gait_contacts(joints[:n], gait["events"][:n], fps=FPS, sigma=sigma)
            cc.assert_margin(host, [n])
            raw = pkg.pipeline.gait_contacts(joints[:n], gait["events"][:n], fps=FPS, sigma=0.0)["per_frame"][:, 1:]
            ratio = cc.compare(alone, host, raw if sigma > 0 else None, [n], sigma)
            print(f"n_seq = 1, sigma {sigma:g}: worst error / bar = {ratio:.3g}")
            assert ratio <= 1.0
        a += n


@pytest.mark.parametrize("sigma", (0.0, 1.0))
def test_a_fixed_speed_in_place_of_the_fraction(model, pkg, sigma):
    """The seven sequences and a standing body of 64 frames behind them."""
    joints = np.concatenate([call(25)[0], cc.planted_walker(**STANDING)])
    lengths = LENGTHS + [STANDING["T"]]
    gait = pkg.pipeline.gait_parameters(joints, lengths=lengths, fps=FPS, sigma=0.0)
    host, raw = (pkg.pipeline.gait_contacts(joints, gait["events"], lengths=lengths, fps=FPS, sigma=s, speed=0.5) for s in (sigma, 0.0))
    margin = cc.assert_margin(host, lengths)
    out = numpy_out(model.gait_contacts(joints, gait["events"], lengths=lengths, fps=FPS, sigma=sigma, speed=0.5))
    ratio = cc.compare(out, host, raw["per_frame"][:, 1:] if sigma > 0 else None, lengths, sigma, speed=0.5)
    print(f"speed 0.5, sigma {sigma:g}: decision margin {margin:.3g}, worst error / bar = {ratio:.3g}")
    assert ratio <= 1.0 and (out["per_sequence"][:, 0] == 0.5).all()
    q = len(LENGTHS)                                           # a standing body: one open run, NaN parameters
    still = out["phase"][sum(lengths[:q]):]
    assert still.tolist() == [3] * 63 + [4] and out["per_sequence"][q, 2:6].tolist() == [1, 0, 0, 1] and np.isnan(np.delete(out["per_sequence"][q, 6:], 5)).all()
    assert out["per_sequence"][q, 11] == 0
    assert np.isnan(out["runs"][q, 0, [0, 1, 3, 4]]).all() and out["runs"][q, 0, 2] == 0 and np.isnan(out["runs"][q, 1:]).all()


def same_as_statement(out, host):
    return np.array_equal(out["phase"], host["phase"]) and cc.same_bits(out["runs"], host["runs"]) and cc.same_bits(out["per_sequence"], host["per_sequence"])


def test_hook_on_the_hand_made_case(model, pkg):
    speeds, events = cc.hand_case()
    for max_runs in (128, 2):
        out = numpy_out(model.op_gait_contact_runs(speeds, events, max_runs=max_runs, **cc.HAND_RULE), hook=True)
        keep = min(max_runs, 6)
        assert out["phase"].tolist() == cc.HAND_PHASE and cc.same_bits(out["runs"][0, :keep], cc.HAND_RUNS[:keep]) and np.isnan(out["runs"][0, keep:]).all()
        assert cc.same_bits(out["per_sequence"][0], cc.HAND_ROW)
        assert same_as_statement(out, pkg.pipeline.gait_contact_runs(speeds, events, max_runs=max_runs, **cc.HAND_RULE))
    three = numpy_out(model.op_gait_contact_runs(np.concatenate([speeds, speeds[:4], speeds]), np.concatenate([events, events[:4], events]), lengths=[22, 4, 22],
                                                 **cc.HAND_RULE), hook=True)
    assert three["phase"].tolist() == cc.HAND_PHASE + [3, 3, 0, 4] + cc.HAND_PHASE
    assert cc.same_bits(three["runs"][0], three["runs"][2]) and cc.same_bits(three["per_sequence"][0], three["per_sequence"][2]) and three["per_sequence"][1, 2] == 1


def test_runs_at_the_word_boundary_through_the_hook(model, pkg):
    """Integer speeds, thr = speed = 5: a run over the intervals 62 to 66, runs at the intervals 63 and 64 alone, a run that ends at interval 63 and one
    that begins at interval 64 with a moving interval nowhere between them but at 64 / 63 -- in sequences of 66, 130 and 131 frames of one call."""
    def signal(T, static):
        s = np.full(T, 9.0)
        s[list(static)] = [1.0 + 0.25 * (k % 3) for k in static]
        return s
    cases = ((130, range(62, 67)), (130, (63,)), (130, (64,)), (66, (62, 63)), (130, (60, 61, 62, 63, 65, 66)), (131, (0, 1, 64, 65, 128, 129)), (66, (63, 64)))
    speeds = np.concatenate([signal(T, st) for T, st in cases])
    lengths = [T for T, _ in cases]
    events = np.zeros(speeds.size, np.int32)
    a = 0
    for i, (T, st) in enumerate(cases):
        events[a + min(st) + (i % 2)] = 1 + i % 2                # a strike at the run's first or second frame, left and right by turns
        a += T
    rule = dict(fps=FPS, speed=5.0, reach=2, max_frames=20)
    host = pkg.pipeline.gait_contact_runs(speeds, events, lengths=lengths, **rule)
    assert cc.assert_margin(dict(speeds=speeds, per_sequence=host["per_sequence"]), lengths) >= 3.0
    assert host["per_sequence"][:, 2].tolist() == [1, 1, 1, 1, 2, 3, 1] and host["runs"][0, 0, :4].tolist() == [61.5 + 4 / 7.5, 66.5 + 4 / 8, 1, 62]
    assert host["per_sequence"][-1, 3:6].tolist() == [0, 0, 1]                    # the run reaches the last interval of 66 frames: open
    out = numpy_out(model.op_gait_contact_runs(speeds, events, lengths=lengths, **rule), hook=True)
    assert same_as_statement(out, host)


def test_more_runs_than_the_table_stores(model, pkg):
    """max_runs = 2 on a walker with about 36 runs: all are counted, two are stored, the row is the one of a table that holds them all."""
    P, beta, speed = cc.WALKERS[0]
    joints = cc.planted_walker(400, P, beta, speed, 0.21 * P, cc.YAWS[1])
    gait = pkg.pipeline.gait_parameters(joints, fps=FPS, sigma=0.0)
    host = pkg.pipeline.gait_contacts(joints, gait["events"], fps=FPS, max_runs=2)
    cc.assert_margin(host, [400])
    assert 34 <= host["per_sequence"][0, 2] <= 38 and np.isfinite(host["runs"][0, :, 0]).any()
    few = numpy_out(model.gait_contacts(joints, gait["events"], fps=FPS, max_runs=2))
    many = numpy_out(model.gait_contacts(joints, gait["events"], fps=FPS, max_runs=128))
    assert cc.compare(few, host, None, [400], 0.0) == 0.0
    assert cc.same_bits(few["per_sequence"], many["per_sequence"]) and cc.same_bits(few["runs"][0], many["runs"][0, :2]) and np.array_equal(few["phase"], many["phase"])
    assert np.isnan(many["runs"][0, int(host["per_sequence"][0, 2]):]).all() and np.isfinite(many["runs"][0, :int(host["per_sequence"][0, 2]), 5]).all()


def test_more_runs_than_edges_are_kept(model, pkg):
    """The sequence kernel keeps the edges of a sequence's first 512 runs in LDS for the row's walks and makes the others again from the speeds: 525
    one-interval runs, led left and right by turns, so 523 strides whose terms come from both ways to an edge.  Equal bits."""
    T = 2100
    k = np.arange(T)
    speeds = np.where(k % 4 == 1, 1.0 + 0.25 * (k % 3), 7.0 + (k % 5))
    events = np.where(k % 4 == 1, 1 + (k // 4) % 2, 0).astype(np.int32)
    rule = dict(fps=FPS, speed=5.0, reach=1, max_frames=20, max_runs=512)
    host = pkg.pipeline.gait_contact_runs(speeds, events, **rule)
    assert cc.assert_margin(dict(speeds=speeds, per_sequence=host["per_sequence"]), [T]) >= 2.0
    assert host["per_sequence"][0, 2:6].tolist() == [525, 263, 262, 0] and host["per_sequence"][0, 11] == 523 and np.isfinite(host["runs"][0]).all()
    out = numpy_out(model.op_gait_contact_runs(speeds, events, **rule), hook=True)
    assert same_as_statement(out, host)


@pytest.mark.parametrize("sigma", (0.0, 1.0))
def test_a_sequence_longer_than_the_lds_masks(model, pkg, sigma):
    """4200 frames > 64 words of 64: the masks and the block sums lie in the call's scratch and go through the same code; beside it a short one in
    LDS, first and last, so that the long one's words begin at another bit of the call."""
    T = 4200
    P, beta, speed = cc.WALKERS[2]
    long_j = cc.planted_walker(T, P, beta, speed, 4.7, 1.3)
    short_j = cc.planted_walker(65, *cc.WALKERS[3], 2.2, 0.2)
    joints, lengths = np.concatenate([short_j, long_j, short_j]), [65, T, 65]
    gait = pkg.pipeline.gait_parameters(joints, lengths=lengths, fps=FPS, sigma=0.0)
    host = pkg.pipeline.gait_contacts(joints, gait["events"], lengths=lengths, fps=FPS, sigma=sigma, max_runs=512)
    margin = cc.assert_margin(host, lengths)
    out = numpy_out(model.gait_contacts(joints, gait["events"], lengths=lengths, fps=FPS, sigma=sigma, max_runs=512))
    raw = pkg.pipeline.gait_contacts(joints, gait["events"], lengths=lengths, fps=FPS, sigma=0.0)["per_frame"][:, 1:] if sigma > 0 else None
    ratio = cc.compare(out, host, raw, lengths, sigma)
    print(f"T = {T}, sigma {sigma:g}: decision margin {margin:.3g}, worst error / bar = {ratio:.3g}, {int(host['per_sequence'][1, 2])} runs, "
          f"{int(host['per_sequence'][1, 11])} strides")
    assert ratio <= 1.0 and abs(host["per_sequence"][1, 2] - 2 * T / P) <= 2 and host["per_sequence"][1, 11] >= 2 * (T / P - 3)
    assert cc.same_bits(out["per_sequence"][0], out["per_sequence"][2])


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    events = torch.zeros(8, dtype=torch.int32, device="cuda")
    speeds = torch.zeros(8, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    phase = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    runs = torch.full((2, 4, 6), -7.0, dtype=torch.float64, device="cuda")
    per_seq = torch.full((2, 20), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, fps=20.0, sigma=1.0, fraction=0.25, speed=0.0, reach=2, hi=20, most=4, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, events.data_ptr(), fps, sigma, fraction, speed, reach, hi, most,
                per_frame.data_ptr(), phase.data_ptr(), runs.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_contacts(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, fps=20.0, fraction=0.25, speed=0.0, reach=2, hi=20, most=4, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, speeds.data_ptr(), events.data_ptr(), off, len(offsets) - 1 if n_seq is None else n_seq, fps, fraction, speed, reach, hi, most, phase.data_ptr(),
                runs.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_contact_runs(*args)

    rule = ((dict(fraction=-0.1), b"fraction"), (dict(fraction=nan), b"fraction"), (dict(fraction=inf), b"fraction"), (dict(speed=-1.0), b"speed"), (dict(speed=nan), b"speed"),
            (dict(speed=inf), b"speed"), (dict(fraction=0.0), b"both zero"), (dict(reach=-1), b"reach"), (dict(reach=9), b"reach"), (dict(hi=0), b"max_frames"),
            (dict(most=0), b"max_runs"), (dict(most=513), b"max_runs"), (dict(fps=0.0), b"fps"), (dict(fps=nan), b"fps"), (dict(fps=inf), b"fps"), (dict(n_seq=0), b"n_seq 0"),
            (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 6, 14, 15, 16, 17)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"), (dict(sigma=-1.0), b"sigma"),
            (dict(sigma=nan), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(n_seq=-2), b"n_seq -2")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 2, 3, 11, 12, 13)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((phase == -7).all()) and bool((runs == -7.0).all()) and bool((per_seq == -7.0).all())      # nothing was written
    assert run(speed=0.5) == 0
    torch.cuda.synchronize()
    assert phase.tolist() == [3, 3, 4, 3, 3, 3, 3, 4] and bool((per_frame[:, 1:] == 0).all()) and bool(runs[:, 1:].isnan().all())      # both ankles at (1, 1, 1): nothing moves
    assert per_seq[:, :6].tolist() == [[0.5, 0, 1, 0, 0, 1], [0.5, 0, 1, 0, 0, 1]] and bool(per_seq[:, 6:11].isnan().all())
    phase.fill_(-7)
    assert hook() == 0                                          # a mean of zero: nothing is below a quarter of it
    torch.cuda.synchronize()
    assert phase.tolist() == [0, 0, 4, 0, 0, 0, 0, 4] and per_seq[:, :6].tolist() == [[0, 0, 0, 0, 0, 0]] * 2 and bool(runs.isnan().all())
    ok = np.ones((4, 25, 3), np.float32)
    ev = np.zeros(4, np.int32)
    for args, kw, word in (((ok[0], ev), {}, "joints3d"), ((ok, ev), {"lengths": [2, 1]}, "lengths"), ((ok, ev), {"joints": (0, 1, 2)}, "joints"), ((ok, ev[:3]), {}, "events"),
                           ((ok, ev), {"reach": 1.5}, "reach"), ((ok, ev), {"max_runs": 513}, "max_runs"), ((ok, ev), {"max_runs": 0}, "max_runs")):
        with pytest.raises(ValueError, match=word):
            model.gait_contacts(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"fps": 0.0}, "fps"), ({"fraction": 0.0}, "both zero"), ({"reach": 9}, "reach"), ({"max_frames": 0}, "max_frames")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_contacts(ok, ev, **kw)
