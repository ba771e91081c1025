"""Gait regularity and symmetry on the GPU (grnet_gait_regularity, csrc/gait_regularity_kernels.hip) against the host statement
pipeline.gait_regularity on the walker of tests/helpers/regularity_checks.py, at the smallest shapes that can break a stage: sequences of 1, 19, 20,
64, 65, 130 and 400 frames, one and seven sequences a call, a standing body, a degenerate frame, J = 25 and 49 (with another table), max_lag 8, 60
and 255 (one wave of lags, and all four), with and without trans and NaN rows in it, with and without exclude, runs of validity that begin and end at
the frames 63, 64 and 65 (the words of the validity mask), a sequence longer than the LDS arrays, and the hand-made signal through the hook.

With sigma = 0 both sides run the same operations in the same order and every output bit is equal.  With sigma > 0 the device's Gaussian has its own
weights and its own order of the sum: per_frame is held to twice the Gaussian's bar (gait_checks.signal_bars), and acf and per_sequence must equal in
every bit what pipeline.gait_autocorr makes of the DEVICE'S OWN per_frame -- downstream of the signals the two sides run the same operations."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from .helpers import gait_checks as gc
from .helpers import regularity_checks as rc

pytestmark = pytest.mark.gpu
FPS = rc.FPS
RULES = {8: dict(max_lag=8, min_lag=2, min_peak=0.1, min_pairs=2), 60: rc.RULE, 255: dict(max_lag=255, min_lag=6, min_peak=0.25, min_pairs=20)}


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == ["acf"] + ([] if hook else ["per_frame"]) + ["per_sequence"]
    assert all(v.is_cuda and v.dtype == torch.float64 for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def call(J):
    """(joints, trans with two NaN rows, lengths, names, exclude, table) of the seven sequences of one call."""
    table = gc.KINECTV2 if J == 25 else gc.OTHER49
    joints, trans, lengths, names = rc.build_call(J, table)
    trans = trans.copy()
    trans[[5, 200]] = np.nan
    ex = np.zeros(sum(lengths), np.int32)
    a = 0
    for T in lengths:
        ex[a + 60:a + min(T, 70)] = 2
        if T > 3:
            ex[a + 3] = 1
        a += T
    return joints, trans, lengths, names, ex, table


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, max_lag, with_trans, with_exclude):
    """The statement with sigma = 0 of the seven sequences, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, trans, lengths, _, ex, table = call(J)
    return pipe.gait_regularity(joints, lengths, trans if with_trans else None, ex if with_exclude else None, fps=FPS, joints=table, **RULES[max_lag])


def same(out, host):
    return all(rc.same_bits(out[k], host[k]) for k in ("acf", "per_sequence") + (("per_frame",) if "per_frame" in out else ()))


@pytest.mark.parametrize("with_trans,with_exclude", ((True, False), (False, True), (True, True)))
@pytest.mark.parametrize("J,max_lag", ((25, 60), (25, 8), (25, 255), (49, 60)))
def test_every_bit_of_the_statement_without_smoothing(model, pkg, J, max_lag, with_trans, with_exclude):
    joints, trans, lengths, names, ex, table = call(J)
    host = statement(pkg.__name__, J, max_lag, with_trans, with_exclude)
    out = numpy_out(model.gait_regularity(joints, lengths, trans if with_trans else None, ex if with_exclude else None, fps=FPS, joints=table, **RULES[max_lag]))
    assert out["acf"].shape == (7, 4, max_lag + 1) and out["per_sequence"].shape == (7, 4, 10) and out["per_frame"].shape == (sum(lengths), 4)
    for k in ("per_frame", "acf", "per_sequence"):
        assert rc.same_bits(out[k], host[k]), f"{k} differs in some bit"
    seq = dict(zip(names, host["per_sequence"]))
    assert np.isnan(seq["one"][:, 1:]).all() and np.isnan(seq["standing64"][:, 1:]).all()      # what the shapes are there for
    assert np.isnan(seq["nineteen"][:, 1:]).all() == (max_lag != 8)                             # min_pairs 20, or 2
    if max_lag == 60 and not with_exclude:
        assert seq["twenty"][0, 1] > 0 and seq["twenty"][0, 2] == -1 and seq["walk130"][0, 5] == 22 and seq["walk400_back"][0, 5] == 27
        assert seq["degenerate65"][0, 0] == 64 and seq["degenerate65"][3, 0] == 65 and seq["walk130"][3, 0] == 129        # the degenerate frame, the NaN trans row


@pytest.mark.parametrize("n_seq", (1, 7))
def test_smoothed_signals_within_the_gaussian_bar_and_the_rest_from_them(model, pkg, n_seq):
    joints, trans, lengths, names, ex, table = call(25)
    if n_seq == 1:
        joints, trans, lengths, ex = joints[:130], trans[:130], lengths[:1], ex[:130]
    raw = pkg.pipeline.gait_regularity(joints, lengths, trans, fps=FPS)["per_frame"]
    host = pkg.pipeline.gait_regularity(joints, lengths, trans, ex, fps=FPS, sigma=2.0)
    out = numpy_out(model.gait_regularity(joints, lengths, trans, ex, fps=FPS, sigma=2.0))
    assert np.array_equal(np.isnan(out["per_frame"]), np.isnan(host["per_frame"]))
    worst, a = 0.0, 0
    for T in lengths:
        b = gc.signal_bars(raw[a:a + T], 2.0)
        for k in range(4):
            fin = np.isfinite(host["per_frame"][a:a + T, k])
            if fin.any() and b[k] > 0:
                worst = max(worst, float(np.abs(out["per_frame"][a:a + T, k] - host["per_frame"][a:a + T, k])[fin].max()) / b[k])
            else:
                assert rc.same_bits(out["per_frame"][a:a + T, k], host["per_frame"][a:a + T, k])
        a += T
    print(f"sigma 2, {n_seq} sequence(s): worst signal error / bar = {worst:.3g}")
    assert worst <= 1.0
    again = pkg.pipeline.gait_autocorr(out["per_frame"], lengths, ex, fps=FPS)
    assert rc.same_bits(out["acf"], again["acf"]) and rc.same_bits(out["per_sequence"], again["per_sequence"])


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_one_sequence_alone_and_among_six_others(model, pkg, sigma):
    joints, trans, lengths, names, ex, _ = call(25)
    whole = numpy_out(model.gait_regularity(joints, lengths, trans, ex, fps=FPS, sigma=sigma))
    again = numpy_out(model.gait_regularity(joints, lengths, trans, ex, fps=FPS, sigma=sigma))
    assert same(whole, again)
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_regularity(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], fps=FPS, sigma=sigma))
        assert rc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and rc.same_bits(alone["acf"][0], whole["acf"][q]), names[q]
        assert rc.same_bits(alone["per_sequence"][0], whole["per_sequence"][q]), names[q]
        a += n


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_a_sequence_longer_than_the_lds_arrays(model, pkg, sigma):
    """4100 frames > 4096: the centred signal, the run numbers and the mask words lie in the call's scratch and go through the same code; beside it a
    short one in LDS, first and last, so that the long one's words begin at another bit of the call."""
    T = 4100
    long_j, long_t = rc.walker(T, 27.3, 0.3, 1.3, 4.7)
    short_j, short_t = rc.walker(65, 19.3, 0.0, 0.2, 2.2)
    joints, trans, lengths = np.concatenate([short_j, long_j, short_j]), np.concatenate([short_t, long_t, short_t]), [65, T, 65]
    ex = np.zeros(sum(lengths), np.int32)
    ex[65 + 2000:65 + 2040] = 1
    ex[65 + 4095] = 1
    out = numpy_out(model.gait_regularity(joints, lengths, trans, ex, fps=FPS, sigma=sigma))
    if sigma == 0:
        host = pkg.pipeline.gait_regularity(joints, lengths, trans, ex, fps=FPS)
        assert same(out, host) and host["per_sequence"][1, 0, 0] == T - 41 and host["per_sequence"][1, 0, 5] == 27
    else:
        host = pkg.pipeline.gait_autocorr(out["per_frame"], lengths, ex, fps=FPS)
        assert rc.same_bits(out["acf"], host["acf"]) and rc.same_bits(out["per_sequence"], host["per_sequence"])
    assert rc.same_bits(out["per_sequence"][0], out["per_sequence"][2]) and rc.same_bits(out["acf"][0], out["acf"][2])


def test_hook_on_the_hand_made_signal(model, pkg):
    x, acf, rows = rc.hand_case()
    out = numpy_out(model.op_gait_autocorr(x, **rc.HAND_RULE), hook=True)
    assert rc.same_bits(out["acf"][0], acf) and rc.same_bits(out["per_sequence"][0], rows)
    three = numpy_out(model.op_gait_autocorr(np.concatenate([x, x[:9], x]), lengths=[31, 9, 31], **rc.HAND_RULE), hook=True)
    assert rc.same_bits(three["per_sequence"][0], rows) and rc.same_bits(three["per_sequence"][2], rows) and rc.same_bits(three["acf"][2], acf)
    assert same(three, pkg.pipeline.gait_autocorr(np.concatenate([x, x[:9], x]), lengths=[31, 9, 31], **rc.HAND_RULE))


def test_runs_at_the_word_boundary_through_the_hook(model, pkg):
    """Runs of validity that begin and end at the frames 63, 64 and 65, by NaN and by exclude, in sequences of 130, 131 and 66 frames of one call."""
    rng = np.random.default_rng(15)
    cases = ((130, (63,), ()), (130, (64,), ()), (130, (65,), (0,)), (131, (0, 1), (63, 64, 65)), (130, (62, 63), (65, 66, 129)), (66, (), (64,)), (130, range(64, 128), ()),
             (130, (), range(0, 64)), (66, range(0, 63), (65,)))
    lengths = [T for T, _, _ in cases]
    t = np.arange(sum(lengths), dtype=np.float64)
    x = np.stack([np.sin(2 * np.pi * t / P) + 0.1 * rng.standard_normal(t.size) for P in (9.7, 11.3, 13.1, 6.2)], axis=1)
    ex = np.zeros(t.size, np.int32)
    a = 0
    for T, nans, excluded in cases:
        x[[a + k for k in nans], :] = np.nan
        ex[[a + k for k in excluded]] = 3
        a += T
    rule = dict(fps=FPS, max_lag=30, min_lag=3, min_peak=0.2, min_pairs=5)
    host = pkg.pipeline.gait_autocorr(x, lengths, ex, **rule)
    assert host["per_sequence"][:, 0, 0].tolist() == [129, 129, 128, 126, 125, 65, 66, 66, 2] and (host["per_sequence"][:6, 0, 5] >= 9).all()
    out = numpy_out(model.op_gait_autocorr(x, lengths, ex, **rule), hook=True)
    assert same(out, host)


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    signals = torch.zeros(8, 4, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    acf = torch.full((2, 4, 61), -7.0, dtype=torch.float64, device="cuda")
    per_seq = torch.full((2, 4, 10), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, fps=20.0, sigma=1.0, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, None, None, fps, sigma, max_lag, min_lag, min_peak, min_pairs,
                per_frame.data_ptr(), acf.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_regularity(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, fps=20.0, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, signals.data_ptr(), None, off, len(offsets) - 1 if n_seq is None else n_seq, fps, max_lag, min_lag, min_peak, min_pairs, acf.data_ptr(), per_seq.data_ptr(),
                stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_autocorr(*args)

    rule = ((dict(fps=0.0), b"fps"), (dict(fps=nan), b"fps"), (dict(fps=inf), b"fps"), (dict(max_lag=7), b"max_lag"), (dict(max_lag=256), b"max_lag"), (dict(min_lag=1), b"min_lag"),
            (dict(min_lag=59), b"min_lag"), (dict(min_peak=0.0), b"min_peak"), (dict(min_peak=1.5), b"min_peak"), (dict(min_peak=nan), b"min_peak"), (dict(min_pairs=1), b"min_pairs"),
            (dict(min_pairs=2 ** 20 + 1), b"min_pairs"), (dict(n_seq=0), b"n_seq 0"), (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"),
            (dict(offsets=(0, 4, 4)), b"empty"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 14, 15, 16)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"), (dict(sigma=-1.0), b"sigma"),
            (dict(sigma=nan), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(n_seq=-2), b"n_seq -2")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 10, 11)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((acf == -7.0).all()) and bool((per_seq == -7.0).all())      # nothing was written
    assert run(min_pairs=2) == 0                                # every joint at (1, 1, 1): no axes, and no trans
    torch.cuda.synchronize()
    assert bool(per_frame.isnan().all()) and bool(acf.isnan().all()) and bool((per_seq[:, :, 0] == 0).all()) and bool(per_seq[:, :, 1:].isnan().all())
    assert hook(min_pairs=2) == 0                               # constant signals: A(0) is not positive
    torch.cuda.synchronize()
    assert per_seq[:, :, 0].tolist() == [[3.0] * 4, [5.0] * 4] and bool(per_seq[:, :, 1:].isnan().all()) and bool(acf.isnan().all())
    ok = np.ones((4, 25, 3), np.float32)
    for args, kw, word in (((ok[0],), {}, "joints3d"), ((ok,), {"lengths": [2, 1]}, "lengths"), ((ok,), {"joints": (0, 1, 2)}, "joints"), ((ok,), {"trans": np.zeros((3, 3))}, "trans"),
                           ((ok,), {"exclude": np.zeros(3)}, "exclude"), ((ok,), {"max_lag": 60.5}, "max_lag"), ((ok,), {"max_lag": 256}, "max_lag")):
        with pytest.raises(ValueError, match=word):
            model.gait_regularity(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"fps": 0.0}, "fps"), ({"min_lag": 1}, "min_lag"), ({"min_peak": 0.0}, "min_peak"), ({"min_pairs": 1}, "min_pairs")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_regularity(ok, **kw)
