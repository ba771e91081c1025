"""Joint-angle kinematics per gait cycle on the GPU (grnet_gait_kinematics, csrc/gait_kinematics_kernels.hip) against the host statement
pipeline.gait_kinematics on the articulated walker of tests/helpers/kinematics_checks.py, at the smallest shapes that can break each stage: sequences
of 1, min_stride, min_stride + 1 (the first that can hold a stride), 64, 65 and 130 frames -- the last three cross a word of the heel-strike
bitmasks -- one sequence and seven in a call, among them a standing body without events, a degenerate frame inside a stride and a walk whose right
foot never strikes; J = 25 and 49 (with another table); min_stride = max_stride; 1100 frames, past the 1024 whose bitmasks lie in LDS.

The bars are derived in kinematics_checks.py and not measured.  With sigma = 0 both sides run the same operations in the same order -- the arctangent
included, which is made of + - * / and sqrt alone -- and every output bit is equal; with sigma > 0 the device's Gaussian has its own weights and its
own order of the sum, so the angles are held to twice the Gaussian's bar and everything made of them to that bar carried through its formula; the
counts stay equal.  Every worst ratio is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from .helpers import kinematics_checks as kc
from .test_kinematics_host_cpu import check_hand_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == (["curves", "per_sequence"] if hook else ["curves", "per_frame", "per_sequence"])
    assert all(v.dtype == torch.float64 and v.is_cuda for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def call(J):
    table = kc.KINECTV2 if J == 25 else kc.OTHER49
    joints, events, lengths, names = kc.build_call(J=J, table=table)
    return joints, events, lengths, names, table


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, sigma, lo, hi):
    """The host statement of a call, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, events, lengths, _, table = call(J)
    return pipe.gait_kinematics(joints, events, lengths=lengths, sigma=sigma, min_stride=lo, max_stride=hi, joints=table)


@pytest.mark.parametrize("sigma", (0.0, 2.0))
@pytest.mark.parametrize("J,lo,hi", ((25, 8, 60), (49, 8, 60), (25, 22, 22)))
def test_seven_sequences_against_the_statement(model, pkg, J, lo, hi, sigma):
    joints, events, lengths, names, table = call(J)
    host = statement(pkg.__name__, J, sigma, lo, hi)
    out = numpy_out(model.gait_kinematics(joints, events, lengths=lengths, sigma=sigma, min_stride=lo, max_stride=hi, joints=table))
    raw = statement(pkg.__name__, J, 0.0, lo, hi)["per_frame"] if sigma > 0 else None
    ratio = kc.compare(out, host, raw, lengths, sigma)
    used = dict(zip(names, host["per_sequence"][:, :, 0].astype(int).tolist()))
    print(f"J {J} strides [{lo}, {hi}] sigma {sigma:g}: worst error / bar = {ratio:.3g}; strides used {used}")
    assert ratio <= 1.0
    assert used["one"] == used["min"] == used["standing64"] == [0] * 13 and np.isnan(host["curves"][4]).all()
    assert used["no_right130"][1::2] == [0] * 6 and used["no_right130"][0] >= 2
    if lo == 8:
        assert used["min_1"] == [1, 0] * 6 + [1] and used["walk130"] == [5] * 13
        assert all(used["degenerate65"][c] == 1 for c in kc.AXIS_CHANNELS) and all(used["degenerate65"][c] == 2 for c in kc.FREE_CHANNELS)
    else:
        assert used["walk130"] == [4] * 13 and used["min_1"] == [0] * 13       # the walk has one stride of 21 frames a foot


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_one_sequence_alone_and_among_six_others(model, pkg, sigma):
    """n_seq = 1 against the statement, and the same rows in the call of seven: equal bits."""
    joints, events, lengths, names, _ = call(25)
    whole = numpy_out(model.gait_kinematics(joints, events, lengths=lengths, sigma=sigma))
    again = numpy_out(model.gait_kinematics(joints, events, lengths=lengths, sigma=sigma))
    assert all(kc.same_bits(whole[k], again[k]) for k in whole)
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_kinematics(joints[a:a + n], events[a:a + n], sigma=sigma))
        assert kc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and kc.same_bits(alone["curves"][0], whole["curves"][q]), names[q]
        assert kc.same_bits(alone["per_sequence"][0], whole["per_sequence"][q]), names[q]
        if q == 0:
            host = pkg.pipeline.gait_kinematics(joints[:n], events[:n], sigma=sigma)
            raw = pkg.pipeline.gait_kinematics(joints[:n], events[:n], sigma=0.0)["per_frame"]
            ratio = kc.compare(alone, host, raw, [n], sigma)
            print(f"n_seq = 1, sigma {sigma:g}: worst error / bar = {ratio:.3g}")
            assert ratio <= 1.0
        a += n


def test_hook_on_the_hand_made_cycles(model, pkg):
    x, ev, lo, hi = kc.hand_case()
    out = numpy_out(model.op_gait_cycles(x, ev, min_stride=lo, max_stride=hi), hook=True)
    check_hand_case(out)
    host = pkg.pipeline.gait_cycles(x, ev, min_stride=lo, max_stride=hi)
    assert kc.compare(out, host, None, [80], 0.0) == 0.0
    three = numpy_out(model.op_gait_cycles(np.concatenate([x, x[:7], x]), np.concatenate([ev, ev[:7], ev]), lengths=[80, 7, 80], min_stride=lo, max_stride=hi), hook=True)
    assert kc.same_bits(three["curves"][0], out["curves"][0]) and kc.same_bits(three["per_sequence"][2], out["per_sequence"][0])
    assert (three["per_sequence"][1, :, 0] == 0).all() and np.isnan(three["curves"][1]).all()


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    events = torch.zeros(8, dtype=torch.int32, device="cuda")
    angles = torch.ones(8, 13, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 13), -7.0, dtype=torch.float64, device="cuda")
    curves, hook_curves = (torch.full((2, 13, 101, 2), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    per_seq, hook_seq = (torch.full((2, 13, 6), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=kc.KINECTV2, sigma=2.0, lo=8, hi=60, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 16)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, events.data_ptr(), sigma, lo, hi, per_frame.data_ptr(), curves.data_ptr(),
                per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_kinematics(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, lo=8, hi=60, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, angles.data_ptr(), events.data_ptr(), off, len(offsets) - 1 if n_seq is None else n_seq, lo, hi, hook_curves.data_ptr(), hook_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_cycles(*args)

    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(null=1), b"null"), (dict(null=3), b"null"), (dict(null=5), b"null"), (dict(null=6), b"null"), (dict(null=10), b"null"), (dict(null=11), b"null"),
                     (dict(null=12), b"null"), (dict(J=0), b"J 0"), (dict(J=-1), b"J -1"), (dict(J=19), b"joint index 20"),
                     (dict(table=kc.KINECTV2[:15] + (-1,)), b"joint index -1"), (dict(table=(25,) + kc.KINECTV2[1:]), b"joint index 25"), (dict(n_seq=0), b"n_seq 0"),
                     (dict(n_seq=-2), b"n_seq -2"), (dict(n_seq=8193), b"n_seq 8193"), (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"),
                     (dict(offsets=(0, 4, 4)), b"empty"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=nan), b"sigma"), (dict(sigma=inf), b"sigma"), (dict(sigma=16.5), b"sigma"),
                     (dict(lo=0), b"min_stride 0"), (dict(lo=-3), b"min_stride -3"), (dict(lo=9, hi=8), b"max_stride 8 < min_stride 9"), (dict(hi=4097), b"max_stride 4097")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in ((dict(null=1), b"null"), (dict(null=2), b"null"), (dict(null=3), b"null"), (dict(null=7), b"null"), (dict(null=8), b"null"), (dict(n_seq=0), b"n_seq 0"),
                     (dict(offsets=(0, 8, 8)), b"empty"), (dict(offsets=(2, 8)), b"not 0"), (dict(lo=0), b"min_stride 0"), (dict(lo=9, hi=8), b"max_stride 8"),
                     (dict(hi=4097), b"max_stride 4097")):
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (per_frame, curves, per_seq, hook_curves, hook_seq))      # nothing was written
    assert run() == 0 and run(sigma=0.0) == 0 and hook() == 0  # the same calls without a fault go through
    torch.cuda.synchronize()
    assert not any(bool((t == -7.0).any()) for t in (per_frame, curves, per_seq, hook_curves, hook_seq))
    assert bool((per_seq[:, :, 0] == 0).all()) and bool(curves.isnan().all())                  # no events: nothing used
    free, axis = list(kc.FREE_CHANNELS), list(kc.AXIS_CHANNELS)
    assert bool(per_frame[:, axis].isnan().all()) and bool(per_frame[:, free].isnan().all())   # every joint at (1, 1, 1): no axes, and every segment is zero
    ok, ev = np.ones((4, 25, 3), np.float32), np.zeros(4, np.int32)
    for args, kw, word in (((ok[0], ev), {}, "joints3d"), ((ok, ev), {"lengths": [2, 1]}, "lengths"), ((ok, ev), {"joints": (0, 1, 2)}, "joints"), ((ok, ev[:3]), {}, "events"),
                           ((ok, ev), {"min_stride": 8.5}, "whole")):
        with pytest.raises(ValueError, match=word):
            model.gait_kinematics(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"min_stride": 0}, "min_stride"), ({"max_stride": 5000}, "max_stride"), ({"joints": kc.KINECTV2[:15] + (30,)}, "joint index")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_kinematics(ok, ev, **kw)
    with pytest.raises(ValueError, match="angles"):
        model.op_gait_cycles(np.ones((4, 12)), ev)


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_a_sequence_longer_than_the_lds_masks(model, pkg, sigma):
    """1100 frames > 16 words of 64: the heel-strike bitmasks lie in the call's scratch and go through the same code; beside it a short one in LDS,
    first and last, so that the long one's words begin at another bit of the call."""
    T = 1100
    long_j, _, long_e = kc.walker(T, theta=1.3, arm_right=0.7)
    short_j, _, short_e = kc.walker(65, theta=0.2)
    joints, events, lengths = np.concatenate([short_j, long_j, short_j]), np.concatenate([short_e, long_e, short_e]), [65, T, 65]
    host = pkg.pipeline.gait_kinematics(joints, events, lengths=lengths, sigma=sigma)
    out = numpy_out(model.gait_kinematics(joints, events, lengths=lengths, sigma=sigma))
    raw = pkg.pipeline.gait_kinematics(joints, events, lengths=lengths, sigma=0.0)["per_frame"] if sigma > 0 else None
    ratio = kc.compare(out, host, raw, lengths, sigma)
    print(f"T = {T}, sigma {sigma:g}: worst error / bar = {ratio:.3g}, {host['per_sequence'][1, :, 0].astype(int).tolist()} strides used")
    assert ratio <= 1.0 and host["per_sequence"][1, :, 0].min() >= 49 and kc.same_bits(out["per_sequence"][0], out["per_sequence"][2])
