"""Movement smoothness of the gait signals on the GPU (grnet_gait_smoothness, csrc/gait_smoothness_kernels.hip) against the host statement
pipeline.gait_smoothness on the noisy walker of tests/helpers/entropy_checks.py and on hand-made signals through the hook, at the smallest shapes
that can break a stage: sequences of 1, 19, 20, 64, 65, 130 and 400 frames, one and seven a call, J = 25 and 49, with and without trans and exclude,
derivative 0, 1 and 2, segments of 8 to 256 frames, nfft = segment up to 4096, 64, 65 and 66 bins (a wave just full and one and two more), 513 and
2049 bins (rounds of the workgroup's width with one bin left over), a sequence longer than 4096 frames, runs of validity shorter and longer than a
segment, and the exact cases: a bin-centred cosine, zeros, amplitude = 1.

The kernels take no logarithm and join nothing across lanes but a maximum, a first and a last index: device and statement must agree, with
sigma = 0, in every bit of per_segment, per_sequence and per_frame, and so the device inherits the statement's bar against the numpy.fft yardstick
(tests/test_smoothness_host_cpu.py).  With sigma > 0 the device's Gaussian has its own order of the sum: per_frame is held to the Gaussian's bar
(gait_checks.signal_bars), and the rest must equal what pipeline.gait_sparc makes of the DEVICE'S OWN per_frame."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from .helpers import entropy_checks as ec
from .helpers import gait_checks as gc
from .helpers import regularity_checks as rc
from .helpers import smoothness_checks as mc

pytestmark = pytest.mark.gpu
KEYS = ("per_segment", "per_sequence")


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == ([] if hook else ["per_frame"]) + ["per_segment", "per_sequence", "slot_offsets"]
    assert all(v.is_cuda and v.dtype == torch.float64 for k, v in out.items() if k != "slot_offsets") and out["slot_offsets"].dtype == np.int64
    return {k: v if k == "slot_offsets" else v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, rule, with_trans, with_exclude):
    """The statement with sigma = 0 of the seven sequences, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, trans, lengths, _, ex, table = ec.noisy_call(J)
    return pipe.gait_smoothness(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **mc.rule_of(*rule))


def same(out, host):
    assert out["per_segment"].shape == host["per_segment"].shape and (out["slot_offsets"] == host["slot_offsets"]).all()
    return all(mc.same_bits(out[k], host[k]) for k in KEYS + (("per_frame",) if "per_frame" in out else ()))


@pytest.mark.parametrize("with_trans,with_exclude", ((True, False), (False, True), (True, True)))
@pytest.mark.parametrize("J,rule", tuple((25, r) for r in mc.RULES) + ((49, mc.RULES[0]), (49, mc.RULES[4])))
def test_every_bit_of_the_statement_without_smoothing(model, pkg, J, rule, with_trans, with_exclude):
    joints, trans, lengths, names, ex, table = ec.noisy_call(J)
    host = statement(pkg.__name__, J, rule, with_trans, with_exclude)
    out = numpy_out(model.gait_smoothness(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **mc.rule_of(*rule)))
    assert out["per_sequence"].shape == (7, 4, 10) and out["per_frame"].shape == (sum(lengths), 4) and out["per_segment"].shape == (out["slot_offsets"][-1], 4, 8)
    assert (out["slot_offsets"] == host["slot_offsets"]).all()
    for k in ("per_frame",) + KEYS:
        assert mc.same_bits(out[k], host[k]), f"{k} differs in some bit"
    seq = dict(zip(names, host["per_sequence"]))
    assert (seq["one"][:, 1:3] == 0).all() and np.isnan(seq["one"][:, 3:]).all()      # what the shapes are there for
    if rule == mc.RULES[0] and not with_exclude:
        assert (seq["walk400_back"][:3, 2] == 11).all() and np.isfinite(seq["walk400_back"][0]).all()
    if with_exclude:
        worst, margin = mc.compare(dict(out, **pkg.pipeline.smoothness_rows(out["per_segment"], out["per_sequence"], out["slot_offsets"])),
                                   host["per_frame"], lengths, ex, mc.rule_of(*rule))      # the device itself against the yardstick
        print(f"{rule}: device against the yardstick: worst ratio {worst:.3e}, margin {margin:.3e}")
        assert worst <= mc.BAR


def test_per_frame_is_gait_regularity_s(model, pkg):
    joints, trans, lengths, _, ex, _ = ec.noisy_call(25)
    for sigma in (0.0, 2.0):
        a = model.gait_smoothness(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        b = model.gait_regularity(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        assert mc.same_bits(a, b)


@pytest.mark.parametrize("n_seq", (1, 7))
def test_smoothed_signals_within_the_gaussian_bar_and_the_rest_from_them(model, pkg, n_seq):
    joints, trans, lengths, names, ex, table = ec.noisy_call(25)
    if n_seq == 1:
        joints, trans, lengths, ex = joints[:130], trans[:130], lengths[:1], ex[:130]
    raw = pkg.pipeline.gait_regularity(joints, lengths, trans)["per_frame"]
    host = pkg.pipeline.gait_regularity(joints, lengths, trans, ex, sigma=2.0)
    out = numpy_out(model.gait_smoothness(joints, lengths, trans, ex, sigma=2.0, **mc.RULE))
    assert np.array_equal(np.isnan(out["per_frame"]), np.isnan(host["per_frame"]))
    worst, a = 0.0, 0
    for T in lengths:
        b = gc.signal_bars(raw[a:a + T], 2.0)
        for k in range(4):
            fin = np.isfinite(host["per_frame"][a:a + T, k])
            if fin.any() and b[k] > 0:
                worst = max(worst, float(np.abs(out["per_frame"][a:a + T, k] - host["per_frame"][a:a + T, k])[fin].max()) / b[k])
            else:
                assert mc.same_bits(out["per_frame"][a:a + T, k], host["per_frame"][a:a + T, k])
        a += T
    print(f"sigma 2, {n_seq} sequence(s): worst signal error / bar = {worst:.3g}")
    assert worst <= 1.0
    again = pkg.pipeline.gait_sparc(out["per_frame"], lengths, ex, **mc.RULE)
    assert same({k: out[k] for k in KEYS + ("slot_offsets",)}, again)
    assert same(numpy_out(model.op_gait_sparc(out["per_frame"], lengths, ex, **mc.RULE), hook=True), again)      # the hook on the device's own signals


def test_one_sequence_alone_and_among_six_others(model, pkg):
    joints, trans, lengths, names, ex, _ = ec.noisy_call(25)
    whole = numpy_out(model.gait_smoothness(joints, lengths, trans, ex, **mc.RULE))
    again = numpy_out(model.gait_smoothness(joints, lengths, trans, ex, **mc.RULE))
    assert same(whole, again)
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_smoothness(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], **mc.RULE))
        lo, hi = whole["slot_offsets"][q:q + 2]
        assert mc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and mc.same_bits(alone["per_segment"], whole["per_segment"][lo:hi]), names[q]
        assert mc.same_bits(alone["per_sequence"][0], whole["per_sequence"][q]), names[q]
        a += n


def test_a_sequence_longer_than_4096_frames(model, pkg):
    """4097 frames with 256-frame segments a segment apart at 4096 points: 16 segments of 2049 bins, nine rounds of the workgroup's width with one bin
    in the last; beside it a short sequence, first and last, which must see nothing of it."""
    T = 4097
    rng = np.random.default_rng(4097)
    x = np.concatenate([rng.standard_normal((70, 4)), 0.01 * rng.standard_normal((T, 4)), rng.standard_normal((70, 4))])
    x[70 + T:] = x[:70]
    rule = mc.rule_of(1, 256, 256, 4096, min_segments=1)
    host = pkg.pipeline.gait_sparc(x, [70, T, 70], **rule)
    out = numpy_out(model.op_gait_sparc(x, [70, T, 70], **rule), hook=True)
    assert same(out, host) and host["slot_offsets"].tolist() == [0, 0, 16, 16] and (host["per_sequence"][1, :, :4] == [T - 1, 16, 16, 16]).all()
    rule = mc.rule_of(1, 64, 32, 1024)
    host = pkg.pipeline.gait_sparc(x, [70, T, 70], **rule)
    out = numpy_out(model.op_gait_sparc(x, [70, T, 70], **rule), hook=True)
    assert same(out, host) and mc.same_bits(out["per_segment"][:1], out["per_segment"][-1:]) and mc.same_bits(out["per_sequence"][0], out["per_sequence"][2])


def test_runs_shorter_and_longer_than_a_segment_and_a_one_frame_sequence(model, pkg):
    x = np.concatenate([mc.runs_signal(), np.ones((1, 4)), mc.runs_signal()[:100]])
    for d in (0, 1, 2):
        rule = mc.rule_of(d, 64, 32, 1024, min_segments=1)
        host = pkg.pipeline.gait_sparc(x, [400, 1, 100], **rule)
        assert same(numpy_out(model.op_gait_sparc(x, [400, 1, 100], **rule), hook=True), host), rule
        assert (host["per_sequence"][1, :, :3] == [1 if d == 0 else 0, 0, 0]).all() and host["slot_offsets"].tolist() == [0, 11, 11, 13]
    assert pkg.pipeline.gait_sparc(x, [400, 1, 100], **mc.rule_of(0, 64, 32, 1024))["per_segment"][:, 0, 0].tolist()[:5] == [31.0, 160.0, 192.0, 224.0, 311.0]
    one = numpy_out(model.op_gait_sparc(np.ones((1, 4))), hook=True)      # no slot at all: two launches, and a per_segment of no rows
    assert one["per_segment"].shape == (0, 4, 8) and (one["per_sequence"][0, :, :3] == 0).all() and np.isnan(one["per_sequence"][0, :, 3:]).all()


def test_exact_cases_through_the_hook(model, pkg):
    for k0 in (3, 11):
        x, rule = mc.centred_cosine(k0), mc.rule_of(0, 64, 32, 64)
        out = numpy_out(model.op_gait_sparc(x, **rule), hook=True)
        assert same(out, pkg.pipeline.gait_sparc(x, **rule))
        seg = out["per_segment"]
        assert (seg[..., 2] == k0).all() and (seg[..., 3] == k0).all() and (seg[..., 4] == k0).all() and (seg[..., 1] == 0.0).all() and not np.signbit(seg[..., 1]).any()
    zero = numpy_out(model.op_gait_sparc(np.zeros((200, 4)), **mc.RULE), hook=True)
    assert same(zero, pkg.pipeline.gait_sparc(np.zeros((200, 4)), **mc.RULE))
    assert (zero["per_segment"][:, :, 0] == np.arange(0, 160, 32)[:, None]).all() and np.isnan(zero["per_segment"][:, :, 1:]).all()
    assert (zero["per_sequence"][0, :, :4] == [199, 5, 5, 0]).all() and np.isnan(zero["per_sequence"][0, :, 4:9]).all()
    x = np.random.default_rng(5).standard_normal((200, 4))
    rule = mc.rule_of(1, 64, 32, 1024, amplitude=1.0)
    one = numpy_out(model.op_gait_sparc(x, **rule), hook=True)
    assert same(one, pkg.pipeline.gait_sparc(x, **rule))
    assert (one["per_segment"][..., 2] == one["per_segment"][..., 4]).all() and (one["per_segment"][..., 3] == one["per_segment"][..., 4]).all()
    assert (one["per_segment"][..., 1] == 0.0).all()
    a, b = numpy_out(model.op_gait_sparc(x, **mc.RULE), hook=True)["per_segment"], numpy_out(model.op_gait_sparc(x * 2.0 ** -7, **mc.RULE), hook=True)["per_segment"]
    assert mc.same_bits(a[..., :5], b[..., :5]) and mc.same_bits(a[..., 6], b[..., 6]) and (a[..., 2] <= a[..., 4]).all() and (a[..., 4] <= a[..., 3]).all()
    few = numpy_out(model.op_gait_sparc(x, **mc.rule_of(1, 64, 32, 1024, min_segments=6)), hook=True)
    assert mc.same_bits(few["per_segment"], a) and (few["per_sequence"][0, :, :3] == [199, 5, 0]).all() and np.isnan(few["per_sequence"][0, :, 3:]).all()


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(24, 25, 3, dtype=torch.float32, device="cuda")
    signals = torch.zeros(24, 4, dtype=torch.float64, device="cuda")
    per_frame = torch.full((24, 4), -7.0, dtype=torch.float64, device="cuda")
    per_seg = torch.full((5, 4, 8), -7.0, dtype=torch.float64, device="cuda")      # 8 and 16 frames, 8-frame segments 4 apart: 1 + 3 slots, and one to spare
    per_seq = torch.full((2, 4, 10), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")

    def run(J=25, offsets=(0, 8, 24), n_seq=None, table=gc.KINECTV2, fps=20.0, sigma=1.0, derivative=1, segment=8, hop=4, nfft=8, f_cut=10.0, amplitude=0.05, min_segments=2, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, None, None, fps, sigma, derivative, segment, hop, nfft, f_cut, amplitude,
                min_segments, per_frame.data_ptr(), per_seg.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_smoothness(*args)

    def hook(offsets=(0, 8, 24), n_seq=None, fps=20.0, derivative=1, segment=8, hop=4, nfft=8, f_cut=10.0, amplitude=0.05, min_segments=2, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, signals.data_ptr(), None, off, len(offsets) - 1 if n_seq is None else n_seq, fps, derivative, segment, hop, nfft, f_cut, amplitude, min_segments,
                per_seg.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_sparc(*args)

    rule = ((dict(fps=0.0), b"fps"), (dict(fps=nan), b"fps"), (dict(fps=inf), b"fps"), (dict(derivative=-1), b"derivative"), (dict(derivative=3), b"derivative"),
            (dict(segment=6, hop=3), b"segment must be even and within [8, 256]"), (dict(segment=9), b"segment"), (dict(segment=258, hop=129, nfft=512), b"segment"),
            (dict(segment=64, hop=7, nfft=64), b"hop outside [segment / 8, segment]"), (dict(hop=9), b"hop"), (dict(segment=16, hop=8, nfft=14), b"nfft must be even and within [segment, 4096]"),
            (dict(nfft=9), b"nfft"), (dict(nfft=4098), b"nfft"), (dict(f_cut=0.0), b"0 < f_cut <= fps / 2"), (dict(f_cut=10.5), b"f_cut"), (dict(f_cut=nan), b"f_cut"),
            (dict(amplitude=0.0), b"amplitude must be within (0, 1]"), (dict(amplitude=1.5), b"amplitude"), (dict(amplitude=nan), b"amplitude"),
            (dict(min_segments=0), b"min_segments outside [1, 2^20]"), (dict(min_segments=2 ** 20 + 1), b"min_segments"), (dict(n_seq=0), b"n_seq 0"),
            (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"),
            (dict(offsets=(0, 3, 3 + 32769)), b"sequence 1 has 32769 frames, more than 32768"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 17, 18, 19)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"), (dict(sigma=-1.0), b"sigma"),
            (dict(sigma=nan), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(n_seq=-2), b"n_seq -2")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 13, 14)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    assert lib.grnet_gait_smoothness(None, None, 25, None, 1, None, None, None, 20.0, 0.0, 1, 8, 4, 8, 10.0, 0.05, 2, None, None, None, None) == pkg._lib.EINVAL      # no handle
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((per_seg == -7.0).all()) and bool((per_seq == -7.0).all())      # nothing was written
    assert run() == 0                                           # every joint at (1, 1, 1): no axes, and no trans
    torch.cuda.synchronize()
    assert bool(per_frame.isnan().all()) and bool(per_seg[:4].isnan().all()) and bool((per_seg[4] == -7.0).all())
    assert bool((per_seq[:, :, :3] == 0).all()) and bool(per_seq[:, :, 3:].isnan().all())
    assert hook(derivative=0, min_segments=1) == 0              # zeros of 8 and 16 frames: 1 and 3 segments, none with a peak
    torch.cuda.synchronize()
    assert per_seg[:4, 0, 0].tolist() == [0.0, 0.0, 4.0, 8.0] and bool(per_seg[:4, :, 1:].isnan().all()) and bool((per_seg[4] == -7.0).all())
    assert per_seq[:, 0, :4].tolist() == [[8.0, 1.0, 1.0, 0.0], [16.0, 3.0, 3.0, 0.0]]
    slots = (C.c_int64 * 3)()
    assert lib.grnet_gait_smoothness_slots((C.c_int32 * 3)(0, 8, 24), 2, 8, 4, slots) == 0 and list(slots) == [0, 1, 4]
    ok = np.ones((4, 25, 3), np.float32)
    for args, kw, word in (((ok[0],), {}, "joints3d"), ((ok,), {"lengths": [2, 1]}, "lengths"), ((ok,), {"joints": (0, 1, 2)}, "joints"), ((ok,), {"trans": np.zeros((3, 3))}, "trans"),
                           ((ok,), {"exclude": np.zeros(3)}, "exclude"), ((ok,), {"nfft": 2.5}, "nfft"), ((ok,), {"segment": 6}, "segment"), ((ok,), {"hop": 3}, "hop")):
        with pytest.raises(ValueError, match=word):
            model.gait_smoothness(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"nfft": 4098}, "nfft"), ({"f_cut": 0.0}, "f_cut"), ({"derivative": 3}, "derivative"), ({"amplitude": 2.0}, "amplitude")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_smoothness(ok, **kw)


def test_window_smoothness_on_a_real_handle(model, pkg, tmp_path, capsys):
    """batch_generation.WindowSmoothness for one window of 3 videos: the device path writes what the host path writes, with a turn's phase as exclude."""
    import importlib
    bg = importlib.import_module("batch_generation")            # tests/conftest.py puts the repository's root on the path
    joints, trans, lengths, names, _, _ = ec.noisy_call(25)
    off = np.concatenate([[0], np.cumsum(lengths)])
    keys = ["walk130", "degenerate65", "walk400_back"]
    picked = [names.index(k) for k in keys]
    per_video = [torch.from_numpy(joints[off[q]:off[q + 1]].reshape(-1, 75)).cuda() for q in picked]
    fitted = [(trans[off[q]:off[q + 1]],) for q in picked]
    phase = [np.zeros(lengths[q], np.int32) for q in picked]
    phase[2][150:190] = 1
    files = {}
    for on_host in (False, True):
        fluent = bg.WindowSmoothness(pkg.pipeline, model, on_host, True)
        assert (fluent.device_call is None) == on_host
        fluent.add_window(keys, per_video, fitted, phase)
        files[on_host] = json.load(open(fluent.write(str(tmp_path / f"smoothness{int(on_host)}.json"))))
    assert files[False] == files[True] and sorted(files[False]) == sorted(keys)
    long = files[False]["walk400_back"]
    assert long["straight_only"] is True and long["sep"]["n"] == 400 - 1 - 41 and long["sep"]["candidates"] == 3 + 5 == len(long["sep"]["segments"])
    assert long["sep"]["sparc_mean"] < 0 and long["sep"]["ldlj_mean"] < 0 and long["sep"]["segments"][3]["start"] == 190 and 0 < long["sep"]["segments"][0]["last_hz"] <= 10
    assert files[False]["degenerate65"]["sep"]["used"] == 0 and files[False]["degenerate65"]["sep"]["sparc_mean"] is None
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Smoothness:")]
    assert len(lines) == 6 and lines[:3] == lines[3:] and all(ln.endswith(", straight walking only.") for ln in lines)
