"""Harmonic ratios per stride on the GPU (grnet_gait_harmonics, csrc/gait_harmonics_kernels.hip) against the host statement
pipeline.gait_harmonics on the walker of tests/helpers/regularity_checks.py, at the smallest shapes that can break a stage: sequences of 1, 7, 8, 64,
65, 130 and 400 frames, one and seven sequences a call, a standing body, a degenerate frame, J = 25 and 49 (with another table), n_harmonics 2, 20 and
32 (one pair of lanes, and all 64), derivative 0, 1 and 2, with and without trans and NaN rows in it, with and without exclude; through the hook on
hand-placed events strides of 6, 7, 63, 64, 65, 255 and 256 frames, strikes at the frames 63, 64 and 65 (the words of the masks) and at a sequence's
last frame, and a sequence of 4100 frames longer than the LDS masks with some 340 candidates for max_strides = 8.

With sigma = 0 both sides run the same operations in the same order and every output bit is equal.  With sigma > 0 the device's Gaussian has its own
weights and its own order of the sum: per_frame is held to twice the Gaussian's bar (gait_checks.signal_bars), and the other outputs must equal in
every bit what pipeline.gait_stride_dft makes of the DEVICE'S OWN per_frame."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from .helpers import gait_checks as gc
from .helpers import harmonic_checks as hc

pytestmark = pytest.mark.gpu
FPS = hc.FPS
KEYS = ("strides", "spectrum", "per_sequence")
RULES = {20: hc.RULE, 2: dict(n_harmonics=2, derivative=0, min_stride=6, max_stride=255, max_strides=3), 32: dict(n_harmonics=32, derivative=1, min_stride=6, max_stride=70, max_strides=512)}


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == ([] if hook else ["per_frame"]) + ["per_sequence", "spectrum", "strides"]
    assert all(v.is_cuda and v.dtype == torch.float64 for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def call(pkg_name, J):
    """(joints, trans with two NaN rows, lengths, names, exclude, table, events) of the seven sequences of one call."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    table = gc.KINECTV2 if J == 25 else gc.OTHER49
    joints, trans, lengths, names, hand = hc.device_call(J, table)
    trans = trans.copy()
    trans[[5, 300]] = np.nan
    ex = np.zeros(sum(lengths), np.int32)
    ex[[50, 51, 400, 401, 402]] = 2
    events = pipe.gait_parameters(joints, lengths, trans, fps=FPS, joints=table)["events"].astype(np.int32) | hand
    return joints, trans, lengths, names, ex, table, events


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, n_harmonics, with_trans, with_exclude):
    """The statement with sigma = 0 of the seven sequences, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, trans, lengths, _, ex, table, events = call(pkg_name, J)
    return pipe.gait_harmonics(joints, events, lengths, trans if with_trans else None, ex if with_exclude else None, fps=FPS, joints=table, **RULES[n_harmonics])


def same(out, host):
    return all(hc.same_bits(out[k], host[k]) for k in KEYS + (("per_frame",) if "per_frame" in out else ()))


@pytest.mark.parametrize("with_trans,with_exclude", ((True, False), (False, True), (True, True)))
@pytest.mark.parametrize("J,n_harmonics", ((25, 20), (25, 2), (25, 32), (49, 20)))
def test_every_bit_of_the_statement_without_smoothing(model, pkg, J, n_harmonics, with_trans, with_exclude):
    joints, trans, lengths, names, ex, table, events = call(pkg.__name__, J)
    rule = RULES[n_harmonics]
    host = statement(pkg.__name__, J, n_harmonics, with_trans, with_exclude)
    out = numpy_out(model.gait_harmonics(joints, events, lengths, trans if with_trans else None, ex if with_exclude else None, fps=FPS, joints=table, **rule))
    assert out["strides"].shape == (7, 4, rule["max_strides"], 6) and out["spectrum"].shape == (7, 4, n_harmonics, 2) and out["per_sequence"].shape == (7, 4, 12)
    for k in ("per_frame",) + KEYS:
        assert hc.same_bits(out[k], host[k]), f"{k} differs in some bit"
    seq = dict(zip(names, host["per_sequence"]))
    assert seq["one"][0, 0] == 0 and np.isnan(seq["one"][:, 2:]).all() and seq["walk400_back"][0, 1] >= 20 and seq["walk130"][0, 1] >= 6      # what the shapes are there for
    assert seq["standing64"][0, 0] == 1 and seq["standing64"][0, 1] == 0                    # a constant signal: degenerate
    if n_harmonics != 20:                                          # min_stride 6
        assert seq["seven"][0, :2].tolist() == [1, 1] and seq["eight"][0, :2].tolist() == [1, 1] and seq["seven"][0, 11] == 2
        assert seq["degenerate65"][0, 1] >= 1 and host["strides"][names.index("degenerate65"), 0, int(seq["degenerate65"][0, 0]) - 1, 1] == 64


def test_one_sequence_alone_and_among_six_others(model, pkg):
    joints, trans, lengths, names, ex, _, events = call(pkg.__name__, 25)
    whole = numpy_out(model.gait_harmonics(joints, events, lengths, trans, ex, fps=FPS, derivative=0))
    again = numpy_out(model.gait_harmonics(joints, events, lengths, trans, ex, fps=FPS, derivative=0))
    assert same(whole, again) and same(whole, pkg.pipeline.gait_harmonics(joints, events, lengths, trans, ex, fps=FPS, derivative=0))
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_harmonics(joints[a:a + n], events[a:a + n], None, trans[a:a + n], ex[a:a + n], fps=FPS, derivative=0))
        assert hc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and all(hc.same_bits(alone[k][0], whole[k][q]) for k in KEYS), names[q]
        a += n
    reg = model.gait_regularity(joints, lengths, trans, ex, fps=FPS)["per_frame"].cpu().numpy()
    assert hc.same_bits(whole["per_frame"], reg)                   # the same frame kernel: gait_regularity's bits


@pytest.mark.parametrize("n_seq", (1, 7))
def test_smoothed_signals_within_the_gaussian_bar_and_the_rest_from_them(model, pkg, n_seq):
    joints, trans, lengths, names, ex, table, events = call(pkg.__name__, 25)
    if n_seq == 1:
        joints, trans, lengths, ex, events = joints[:130], trans[:130], lengths[:1], ex[:130], events[:130]
    raw = pkg.pipeline.gait_regularity(joints, lengths, trans, fps=FPS)["per_frame"]
    host = pkg.pipeline.gait_regularity(joints, lengths, trans, fps=FPS, sigma=2.0)
    out = numpy_out(model.gait_harmonics(joints, events, lengths, trans, ex, fps=FPS, sigma=2.0))
    assert np.array_equal(np.isnan(out["per_frame"]), np.isnan(host["per_frame"]))
    worst, a = 0.0, 0
    for T in lengths:
        b = gc.signal_bars(raw[a:a + T], 2.0)
        for k in range(4):
            fin = np.isfinite(host["per_frame"][a:a + T, k])
            if fin.any() and b[k] > 0:
                worst = max(worst, float(np.abs(out["per_frame"][a:a + T, k] - host["per_frame"][a:a + T, k])[fin].max()) / b[k])
            else:
                assert hc.same_bits(out["per_frame"][a:a + T, k], host["per_frame"][a:a + T, k])
        a += T
    print(f"sigma 2, {n_seq} sequence(s): worst signal error / bar = {worst:.3g}")
    assert worst <= 1.0
    again = pkg.pipeline.gait_stride_dft(out["per_frame"], events, lengths, ex, fps=FPS)
    assert all(hc.same_bits(out[k], again[k]) for k in KEYS)
    reg = model.gait_regularity(joints, lengths, trans, ex, fps=FPS, sigma=2.0)["per_frame"].cpu().numpy()
    assert hc.same_bits(out["per_frame"], reg)


@pytest.mark.parametrize("max_strides,n_harmonics,derivative", ((8, 20, 2), (128, 32, 0)))
def test_hand_placed_events_through_the_hook(model, pkg, max_strides, n_harmonics, derivative):
    x, ev, ex, lengths, names = hc.hand_events_call()
    rule = dict(fps=FPS, n_harmonics=n_harmonics, derivative=derivative, min_stride=6, max_stride=255, max_strides=max_strides)
    for exclude in (None, ex):
        host = pkg.pipeline.gait_stride_dft(x, ev, lengths, exclude, **rule)
        out = numpy_out(model.op_gait_stride_dft(x, ev, lengths, exclude, **rule), hook=True)
        for k in KEYS:
            assert hc.same_bits(out[k], host[k]), f"{k} differs in some bit"
    e = dict(zip(names, host["per_sequence"]))["edges800"]
    assert e[0, :2].tolist() == [14, 10] and e[0, 11] == 2         # strides of 6 .. 255 frames used, those of 1, 5 and 256 not
    a = sum(lengths[:3])
    alone = numpy_out(model.op_gait_stride_dft(x[a:a + 130], ev[a:a + 130], None, ex[a:a + 130], **rule), hook=True)
    assert all(hc.same_bits(alone[k][0], out[k][3]) for k in KEYS)


def test_a_sequence_longer_than_the_lds_masks(model, pkg):
    """4100 frames > 4096 with a stride every 24 frames of either foot: the masks lie in the call's scratch, some 340 candidates go to four waves and
    into 8 stored rows; beside it a short sequence in LDS, first and last, so that the long one's words and slots begin elsewhere in the call."""
    T, P = 4100, hc.CLOSED_P
    rng = np.random.default_rng(2003)
    long_x = np.stack([hc.closed_signal(T, B, phi) for B, phi in ((0.3, 0.0), (0.1, 2.0), (0.6, 5.0), (0.3, 7.0))], axis=1) + 0.01 * rng.standard_normal((T, 4))
    short_x = long_x[1000:1065].copy()
    x, lengths = np.concatenate([short_x, long_x, short_x]), [65, T, 65]
    ev = np.concatenate([hc.periodic_events(65, P, 5, 17), hc.periodic_events(T, P, 3, 15), hc.periodic_events(65, P, 5, 17)])
    ev[65 + 4099] |= 1                                             # a strike at the long sequence's last frame
    ex = np.zeros(sum(lengths), np.int32)
    ex[65 + 2000:65 + 2040] = 1
    ex[65 + 4095] = 1
    rule = dict(fps=FPS, n_harmonics=20, derivative=2, min_stride=8, max_stride=60, max_strides=8)
    host = pkg.pipeline.gait_stride_dft(x, ev, lengths, ex, **rule)
    out = numpy_out(model.op_gait_stride_dft(x, ev, lengths, ex, **rule), hook=True)
    print("4100 frames, sep:", host["per_sequence"][1, 0].tolist())
    assert host["per_sequence"][1, 0, 0] == 341 and 330 <= host["per_sequence"][1, 0, 1] < 341 and host["strides"][1, 0, 7, 3] == 10
    for k in KEYS:
        assert hc.same_bits(out[k], host[k]), f"{k} differs in some bit"
    assert all(hc.same_bits(out[k][0], out[k][2]) for k in KEYS)


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    signals = torch.zeros(8, 4, dtype=torch.float64, device="cuda")
    events = torch.zeros(8, dtype=torch.int32, device="cuda")
    per_frame = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    strides = torch.full((2, 4, 128, 6), -7.0, dtype=torch.float64, device="cuda")
    spectrum = torch.full((2, 4, 20, 2), -7.0, dtype=torch.float64, device="cuda")
    per_seq = torch.full((2, 4, 12), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, fps=20.0, sigma=1.0, n_harmonics=20, derivative=2, min_stride=8, max_stride=60, max_strides=128, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, None, events.data_ptr(), None, fps, sigma, n_harmonics, derivative, min_stride,
                max_stride, max_strides, per_frame.data_ptr(), strides.data_ptr(), spectrum.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_harmonics(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, fps=20.0, n_harmonics=20, derivative=2, min_stride=8, max_stride=60, max_strides=128, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, signals.data_ptr(), events.data_ptr(), None, off, len(offsets) - 1 if n_seq is None else n_seq, fps, n_harmonics, derivative, min_stride, max_stride,
                max_strides, strides.data_ptr(), spectrum.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_stride_dft(*args)

    rule = ((dict(fps=0.0), b"fps"), (dict(fps=nan), b"fps"), (dict(fps=inf), b"fps"), (dict(n_harmonics=0), b"n_harmonics"), (dict(n_harmonics=21), b"n_harmonics"),
            (dict(n_harmonics=34), b"n_harmonics"), (dict(derivative=-1), b"derivative"), (dict(derivative=3), b"derivative"), (dict(min_stride=5), b"min_stride"),
            (dict(min_stride=61), b"min_stride"), (dict(max_stride=256), b"max_stride"), (dict(max_strides=0), b"max_strides"), (dict(max_strides=513), b"max_strides"),
            (dict(n_seq=0), b"n_seq 0"), (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 7, 16, 17, 18, 19)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"), (dict(sigma=-1.0), b"sigma"),
            (dict(sigma=nan), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(n_seq=-2), b"n_seq -2")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 2, 4, 12, 13, 14)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (per_frame, strides, spectrum, per_seq))      # nothing was written
    assert run() == 0                                           # every joint at (1, 1, 1): no axes, no trans, no strikes
    torch.cuda.synchronize()
    assert bool(per_frame.isnan().all()) and bool(strides.isnan().all()) and bool(spectrum.isnan().all())
    assert bool((per_seq[:, :, :2] == 0).all()) and bool(per_seq[:, :, 2:].isnan().all())
    ok = np.ones((4, 25, 3), np.float32)
    ev = np.zeros(4, np.int32)
    for args, kw, word in (((ok[0], ev), {}, "joints3d"), ((ok, ev), {"lengths": [2, 1]}, "lengths"), ((ok, ev), {"joints": (0, 1, 2)}, "joints"), ((ok, ev), {"trans": np.zeros((3, 3))}, "trans"),
                           ((ok, ev), {"exclude": np.zeros(3)}, "exclude"), ((ok, ev[:3]), {}, "events"), ((ok, ev), {"n_harmonics": 21}, "n_harmonics"),
                           ((ok, ev), {"max_strides": 513}, "max_strides"), ((ok, ev), {"min_stride": 8.5}, "min_stride")):
        with pytest.raises(ValueError, match=word):
            model.gait_harmonics(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"fps": 0.0}, "fps"), ({"derivative": 3}, "derivative"), ({"min_stride": 5}, "min_stride"), ({"max_stride": 256}, "max_stride")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_harmonics(ok, ev, **kw)
