"""Gait events and parameters on the GPU (grnet_gait_parameters, csrc/gait_kernels.hip) against the host statement
pipeline.gait_parameters on the synthetic walker of tests/helpers/gait_checks.py, at the smallest shapes that can break each stage: sequences of
1, 2 w, 2 w + 1 (the first length that can hold an event), 64, 65 and 130 frames -- the last three cross a word of the event bitmasks -- one
sequence and seven in a call, a standing body and a degenerate frame among them, J = 25 and 49 (with another table), windows of 1, 5 and 32.

The bars are derived in gait_checks.py and not measured.  Every input has a decision margin >= 1e-6 m, asserted on the host, so the events are
EQUAL; with sigma = 0 both sides run the same operations in the same order and every output bit is equal; with sigma > 0 the device's Gaussian has
its own weights (libm's exp, another order of their sum) and its own order of the sum, so the signals are held to twice the Gaussian's bar -- both
sides err -- and step length, its SD and the speed to that bar carried through their formulas; whatever the smoothing does not reach stays equal
in every bit.  Every worst ratio is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from .helpers import gait_checks as gc
from .test_gait_host_cpu import both_feet_events, hand_events, hand_signals

pytestmark = pytest.mark.gpu
FPS, EXC = 20.0, 0.05


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out):
    assert sorted(out) == ["events", "per_frame", "per_sequence"]
    assert out["per_frame"].dtype == torch.float64 and out["events"].dtype == torch.int32 and out["per_sequence"].dtype == torch.float64
    assert all(v.is_cuda for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def excursion(window):
    return 0.005 if window == 1 else EXC                       # three frames around a peak rise by A (1 - cos(2 pi / P)) = 0.012 m only


@functools.lru_cache(maxsize=None)
def call(window, J):
    """The seven sequences, once per (window, J); trans_nan: the translation with NaN rows, among them heel-strike frames of the first walk."""
    table = gc.KINECTV2 if J == 25 else gc.OTHER49
    joints, trans, lengths, names = gc.build_call(window, J=J, table=table)
    trans_nan = trans.copy()
    trans_nan[[8, 9, 10, 117, 200, 300]] = np.nan
    return joints, trans, trans_nan, lengths, names, table


@functools.lru_cache(maxsize=None)
def statement(pkg_name, window, J, sigma, which):
    """The host statement of a call, computed once and shared; the margin condition is asserted here."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, trans, trans_nan, lengths, _, table = call(window, J)
    tr = {"none": None, "trans": trans, "nan": trans_nan}[which]
    host = pipe.gait_parameters(joints, lengths=lengths, trans=tr, fps=FPS, sigma=sigma, window=window, min_excursion=excursion(window), joints=table)
    margin = gc.assert_margin(host["per_frame"], lengths, window, excursion(window))
    print(f"window {window} J {J} sigma {sigma:g} trans {which}: decision margin {margin:.3g} m")
    return host


@pytest.mark.parametrize("sigma", (0.0, 2.0))
@pytest.mark.parametrize("window,J", ((1, 25), (5, 25), (32, 25), (5, 49)))
def test_seven_sequences_against_the_statement(model, pkg, window, J, sigma):
    joints, trans, trans_nan, lengths, names, table = call(window, J)
    for which, tr in (("none", None), ("trans", trans), ("nan", trans_nan)):
        host = statement(pkg.__name__, window, J, sigma, which)
        out = numpy_out(model.gait_parameters(joints, lengths=lengths, trans=tr, fps=FPS, sigma=sigma, window=window, min_excursion=excursion(window), joints=table))
        raw = statement(pkg.__name__, window, J, 0.0, which)["per_frame"][:, :4] if sigma > 0 else None     # the columns that are filtered
        ratio = gc.compare(out, host, raw, lengths, sigma)
        print(f"window {window} J {J} sigma {sigma:g} trans {which}: worst error / bar = {ratio:.3g}; events per sequence "
              f"{dict(zip(names, host['per_sequence'][:, :4].sum(axis=1).astype(int).tolist()))}")
        assert ratio <= 1.0
        speed = host["per_sequence"][:, 17]
        assert np.isnan(speed).all() if which == "none" else window > 5 or np.isfinite(speed[[0, 6]]).all()
    if window == 5:
        assert host["per_sequence"][0, 4] >= 9 and host["events"][lengths[0] + 1 + 2 * window + window] & gc.HEEL_L


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_one_sequence_alone_and_among_six_others(model, pkg, sigma):
    """n_seq = 1 against the statement, and the same rows in the call of seven: equal bits."""
    joints, trans, _, lengths, names, table = call(5, 25)
    whole = numpy_out(model.gait_parameters(joints, lengths=lengths, trans=trans, fps=FPS, sigma=sigma, window=5, min_excursion=EXC))
    again = numpy_out(model.gait_parameters(joints, lengths=lengths, trans=trans, fps=FPS, sigma=sigma, window=5, min_excursion=EXC))
    assert all(gc.same_bits(whole[k], again[k]) for k in ("per_frame", "per_sequence")) and np.array_equal(whole["events"], again["events"])
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_parameters(joints[a:a + n], trans=trans[a:a + n], fps=FPS, sigma=sigma, window=5, min_excursion=EXC))
        assert np.array_equal(alone["events"], whole["events"][a:a + n]), names[q]
        assert gc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and gc.same_bits(alone["per_sequence"][0], whole["per_sequence"][q]), names[q]
        if q == 0:
            host = pkg.pipeline.gait_parameters(joints[:n], trans=trans[:n], fps=FPS, sigma=sigma, window=5, min_excursion=EXC)
            gc.assert_margin(host["per_frame"], [n], 5, EXC)
            raw = pkg.pipeline.gait_parameters(joints[:n], fps=FPS, sigma=0.0, window=5, min_excursion=EXC)["per_frame"][:, :4]
            ratio = gc.compare(alone, host, raw, [n], sigma)
            print(f"n_seq = 1, sigma {sigma:g}: worst error / bar = {ratio:.3g}")
            assert ratio <= 1.0
        a += n


def test_hook_on_the_hand_made_signal(model):
    s = hand_signals()
    ev = model.op_gait_events(s, window=2, min_excursion=1.0)
    assert ev.dtype == torch.int32 and ev.is_cuda and ev.cpu().tolist() == hand_events().tolist()
    three = model.op_gait_events(np.concatenate([s, s[:4], s]), lengths=[13, 4, 13], window=2, min_excursion=1.0).cpu().tolist()
    assert three == hand_events().tolist() + [0] * 4 + hand_events().tolist()
    assert model.op_gait_events(s, window=2, min_excursion=9.5).cpu().tolist() == [0] * 13
    both = np.stack([s[:, 0], s[:, 0], s[:, 2], s[:, 2]], axis=1)      # both feet on the one signal: both bits of a kind in the same frames
    assert model.op_gait_events(both, window=2, min_excursion=1.0).cpu().tolist() == both_feet_events().tolist()


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_both_feet_strike_in_one_frame(model, pkg, sigma):
    """The hopper of gait_checks.py: rule 5 writes the left foot's values, rule 6 counts the frame as one event of each foot, left first."""
    joints, trans = gc.walker(130, theta=0.5, right=0.8)
    host = pkg.pipeline.gait_parameters(joints, trans=trans, fps=FPS, sigma=sigma, window=5, min_excursion=EXC)
    gc.assert_margin(host["per_frame"], [130], 5, EXC)
    both = np.flatnonzero((host["events"] & 3) == 3)
    assert both.size >= 5 and not ((host["events"] & 3) == 1).any() and not ((host["events"] & 3) == 2).any()
    assert (host["per_frame"][both, 5] > 0).all() and host["per_sequence"][0, 4] == 2 * both.size - 1
    out = numpy_out(model.gait_parameters(joints, trans=trans, fps=FPS, sigma=sigma, window=5, min_excursion=EXC))
    raw = pkg.pipeline.gait_parameters(joints, fps=FPS, sigma=0.0, window=5, min_excursion=EXC)["per_frame"][:, :4]
    ratio = gc.compare(out, host, raw, [130], sigma)
    print(f"both feet, sigma {sigma:g}: {both.size} frames with both strikes, worst error / bar = {ratio:.3g}")
    assert ratio <= 1.0


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    trans = torch.zeros(8, 3, dtype=torch.float64, device="cuda")
    signals = torch.ones(8, 4, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 7), -7.0, dtype=torch.float64, device="cuda")
    events, hook_events = torch.full((8,), -7, dtype=torch.int32, device="cuda"), torch.full((8,), -7, dtype=torch.int32, device="cuda")
    per_seq = torch.full((2, 18), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, fps=20.0, sigma=2.0, window=5, exc=0.05, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, trans.data_ptr(), fps, sigma, window, exc, per_frame.data_ptr(),
                events.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_parameters(*args)

    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(null=1), b"null"), (dict(null=3), b"null"), (dict(null=5), b"null"), (dict(null=11), b"null"), (dict(null=12), b"null"), (dict(null=13), b"null"),
                     (dict(J=0), b"J 0"), (dict(J=-1), b"J -1"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"),
                     (dict(table=(25, 20, 12, 16, 14, 18, 15, 19)), b"joint index 25"), (dict(n_seq=0), b"n_seq 0"), (dict(n_seq=-2), b"n_seq -2"),
                     (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"), (dict(fps=0.0), b"fps"),
                     (dict(fps=-20.0), b"fps"), (dict(fps=nan), b"fps"), (dict(fps=inf), b"fps"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=nan), b"sigma"),
                     (dict(sigma=inf), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(window=0), b"window 0"), (dict(window=33), b"window 33"),
                     (dict(window=-1), b"window -1"), (dict(exc=-0.01), b"min_excursion"), (dict(exc=nan), b"min_excursion"), (dict(exc=inf), b"min_excursion")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    off = (C.c_int32 * 3)(0, 3, 8)
    for args, word in (([h, None, off, 2, 5, 0.05, hook_events.data_ptr(), stream], b"null"), ([h, signals.data_ptr(), None, 2, 5, 0.05, hook_events.data_ptr(), stream], b"null"),
                       ([h, signals.data_ptr(), off, 2, 5, 0.05, None, stream], b"null"), ([h, signals.data_ptr(), off, 0, 5, 0.05, hook_events.data_ptr(), stream], b"n_seq 0"),
                       ([h, signals.data_ptr(), off, 2, 0, 0.05, hook_events.data_ptr(), stream], b"window 0"),
                       ([h, signals.data_ptr(), off, 2, 33, 0.05, hook_events.data_ptr(), stream], b"window 33"),
                       ([h, signals.data_ptr(), off, 2, 5, -1.0, hook_events.data_ptr(), stream], b"min_excursion"),
                       ([h, signals.data_ptr(), (C.c_int32 * 3)(0, 8, 8), 2, 5, 0.05, hook_events.data_ptr(), stream], b"empty")):
        assert lib.grnet_op_gait_events(*args) == pkg._lib.EINVAL, word
        assert word in lib.grnet_last_error(h), (word, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((events == -7).all()) and bool((per_seq == -7.0).all()) and bool((hook_events == -7).all())      # nothing was written
    assert run() == 0 and run(null=6, sigma=0.0) == 0          # the same call without a fault goes through; trans_dev may be null
    assert lib.grnet_op_gait_events(h, signals.data_ptr(), off, 2, 1, 0.05, hook_events.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert not bool((events == -7).any()) and not bool((hook_events == -7).any()) and not bool((per_seq[:, :5] == -7.0).any())
    assert bool(per_frame.isnan().all())                        # every joint at (1, 1, 1): each frame is degenerate, NaN everywhere
    ok = np.ones((4, 25, 3), np.float32)
    for args, kw, word in (((ok[0],), {}, "joints3d"), ((ok,), {"lengths": [2, 1]}, "lengths"), ((ok,), {"joints": (0, 1, 2)}, "joints"), ((ok,), {"trans": np.zeros((3, 3))}, "trans"),
                           ((ok,), {"window": 5.7}, "window")):
        with pytest.raises(ValueError, match=word):
            model.gait_parameters(*args, **kw)
    for kw, word in (({"window": 40}, "window"), ({"sigma": 20.0}, "sigma"), ({"fps": 0.0}, "fps"), ({"joints": (0, 20, 12, 16, 14, 18, 15, 30)}, "joint index")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_parameters(ok, **kw)
    with pytest.raises(ValueError, match="window"):
        model.op_gait_events(np.ones((4, 4)), window=2.5)


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_a_sequence_longer_than_the_lds_masks(model, pkg, sigma):
    """4200 frames > 64 words of 64: the event bitmasks lie in the call's scratch and go through the same code; beside it a short one in LDS, first
    and last, so that the long one's words begin at another bit of the call."""
    T = 4200
    long_j, long_t = gc.walker(T, theta=1.3, phi=-3.02)
    short_j, short_t = gc.walker(65, theta=0.2)
    joints, trans, lengths = np.concatenate([short_j, long_j, short_j]), np.concatenate([short_t, long_t, short_t]), [65, T, 65]
    host = pkg.pipeline.gait_parameters(joints, lengths=lengths, trans=trans, fps=FPS, sigma=sigma, window=5, min_excursion=EXC)
    margin = gc.assert_margin(host["per_frame"], lengths, 5, EXC)
    out = numpy_out(model.gait_parameters(joints, lengths=lengths, trans=trans, fps=FPS, sigma=sigma, window=5, min_excursion=EXC))
    raw = pkg.pipeline.gait_parameters(joints, lengths=lengths, fps=FPS, sigma=0.0, window=5, min_excursion=EXC)["per_frame"][:, :4]
    ratio = gc.compare(out, host, raw, lengths, sigma)
    print(f"T = {T}, sigma {sigma:g}: decision margin {margin:.3g} m, worst error / bar = {ratio:.3g}, {int(host['per_sequence'][1, 4])} steps")
    assert ratio <= 1.0 and host["per_sequence"][1, 4] > 380
