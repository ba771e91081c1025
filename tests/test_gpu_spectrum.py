"""The Welch spectrum of the gait signals on the GPU (grnet_gait_spectrum, csrc/gait_spectrum_kernels.hip) against the host statement
pipeline.gait_spectrum on the noisy walker of tests/helpers/entropy_checks.py and on hand-made signals through the hook, at the smallest shapes that
can break a stage: sequences of 1, 19, 20, 64, 65, 130 and 400 frames, one and seven a call, a standing body, J = 25 and 49, with and without trans
and exclude, derivative 0, 1 and 2, segments of 8, 64 and 256 frames, hops of an eighth, a half and a whole segment, nfft = segment, four segments,
510, 512 and 514 (256, 257 and 258 bins: a block of 64 bins fewer, just full, and one more) and 1024, runs of validity that begin and end at the
frames 63, 64 and 65, runs exactly segment - 1, segment and segment + hop long, a sequence longer than the LDS array, and more segments than the LDS
lists hold (spectrum_checks.LDS_SEGMENTS = 512, csrc/kernels.h's kSpecLdsSegments).

The kernel takes no logarithm and adds nothing across lanes: device and statement must agree, with sigma = 0, in every bit of psd, per_sequence and
per_frame, and so the device inherits the statement's bar against the numpy.fft yardstick (tests/test_spectrum_host_cpu.py).  With sigma > 0 the
device's Gaussian has its own order of the sum: per_frame is held to the Gaussian's bar (gait_checks.signal_bars), and psd and per_sequence must
equal what pipeline.gait_welch makes of the DEVICE'S OWN per_frame."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from .helpers import entropy_checks as ec
from .helpers import gait_checks as gc
from .helpers import regularity_checks as rc
from .helpers import spectrum_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == ([] if hook else ["per_frame"]) + ["per_sequence", "psd"]
    assert all(v.is_cuda and v.dtype == torch.float64 for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, rule, with_trans, with_exclude):
    """The statement with sigma = 0 of the seven sequences, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, trans, lengths, _, ex, table = ec.noisy_call(J)
    return pipe.gait_spectrum(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **sc.rule_of(*rule))


def same(out, host):
    return all(sc.same_bits(out[k], host[k]) for k in ("psd", "per_sequence") + (("per_frame",) if "per_frame" in out else ()))


@pytest.mark.parametrize("with_trans,with_exclude", ((True, False), (False, True), (True, True)))
@pytest.mark.parametrize("J,rule", tuple((25, r) for r in sc.RULES) + ((49, sc.RULES[0]), (49, sc.RULES[6])))
def test_every_bit_of_the_statement_without_smoothing(model, pkg, J, rule, with_trans, with_exclude):
    joints, trans, lengths, names, ex, table = ec.noisy_call(J)
    host = statement(pkg.__name__, J, rule, with_trans, with_exclude)
    out = numpy_out(model.gait_spectrum(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **sc.rule_of(*rule)))
    assert out["psd"].shape == (7, 4, rule[3] // 2 + 1) and out["per_sequence"].shape == (7, 4, 13) and out["per_frame"].shape == (sum(lengths), 4)
    for k in ("per_frame", "psd", "per_sequence"):
        assert sc.same_bits(out[k], host[k]), f"{k} differs in some bit"
    seq = dict(zip(names, host["per_sequence"]))
    assert (seq["one"][:, 1:3] == 0).all() and np.isnan(seq["one"][:, 3:]).all()      # what the shapes are there for
    if rule == sc.RULES[0] and not with_exclude:
        assert (seq["walk400_back"][:3, 2] == 11).all() and np.isfinite(seq["walk400_back"][:3, :8]).all()      # 398 values of y: (398 - 64) // 32 + 1; a width may lack a crossing
    if rule[1] == 8:
        assert (seq["standing64"][:3, 2] > 0).all()


def test_per_frame_is_gait_regularity_s(model, pkg):
    joints, trans, lengths, _, ex, _ = ec.noisy_call(25)
    for sigma in (0.0, 2.0):
        a = model.gait_spectrum(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        b = model.gait_regularity(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        assert sc.same_bits(a, b)


@pytest.mark.parametrize("n_seq", (1, 7))
def test_smoothed_signals_within_the_gaussian_bar_and_the_rest_from_them(model, pkg, n_seq):
    joints, trans, lengths, names, ex, table = ec.noisy_call(25)
    if n_seq == 1:
        joints, trans, lengths, ex = joints[:130], trans[:130], lengths[:1], ex[:130]
    raw = pkg.pipeline.gait_regularity(joints, lengths, trans)["per_frame"]
    host = pkg.pipeline.gait_regularity(joints, lengths, trans, ex, sigma=2.0)
    out = numpy_out(model.gait_spectrum(joints, lengths, trans, ex, sigma=2.0, **sc.RULE))
    assert np.array_equal(np.isnan(out["per_frame"]), np.isnan(host["per_frame"]))
    worst, a = 0.0, 0
    for T in lengths:
        b = gc.signal_bars(raw[a:a + T], 2.0)
        for k in range(4):
            fin = np.isfinite(host["per_frame"][a:a + T, k])
            if fin.any() and b[k] > 0:
                worst = max(worst, float(np.abs(out["per_frame"][a:a + T, k] - host["per_frame"][a:a + T, k])[fin].max()) / b[k])
            else:
                assert sc.same_bits(out["per_frame"][a:a + T, k], host["per_frame"][a:a + T, k])
        a += T
    print(f"sigma 2, {n_seq} sequence(s): worst signal error / bar = {worst:.3g}")
    assert worst <= 1.0
    again = pkg.pipeline.gait_welch(out["per_frame"], lengths, ex, **sc.RULE)
    assert sc.same_bits(out["psd"], again["psd"]) and sc.same_bits(out["per_sequence"], again["per_sequence"])


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_one_sequence_alone_and_among_six_others(model, pkg, sigma):
    joints, trans, lengths, names, ex, _ = ec.noisy_call(25)
    whole = numpy_out(model.gait_spectrum(joints, lengths, trans, ex, sigma=sigma, **sc.RULE))
    again = numpy_out(model.gait_spectrum(joints, lengths, trans, ex, sigma=sigma, **sc.RULE))
    assert same(whole, again)
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_spectrum(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], sigma=sigma, **sc.RULE))
        assert sc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and sc.same_bits(alone["psd"][0], whole["psd"][q]), names[q]
        assert sc.same_bits(alone["per_sequence"][0], whole["per_sequence"][q]), names[q]
        a += n


def test_a_sequence_longer_than_the_lds_array(model, pkg):
    """4200 frames > 4096: the differenced signal lies in the workgroup's span of the call's scratch and goes through the same code; beside it a short
    one, first and last.  With 8-frame segments one frame apart the long sequence also holds more segments than the LDS lists (512), the short ones
    do not: all four forms of the kernel's stages run."""
    T = 4200
    rng = np.random.default_rng(42)
    long_j, long_t = rc.walker(T, 27.3, 0.3, 1.3, 4.7)
    short_j, short_t = rc.walker(65, 19.3, 0.0, 0.2, 2.2)
    long_j = (long_j + ec.NOISE * rng.standard_normal(long_j.shape)).astype(np.float32)
    short_j = (short_j + ec.NOISE * rng.standard_normal(short_j.shape)).astype(np.float32)
    joints, trans, lengths = np.concatenate([short_j, long_j, short_j]), np.concatenate([short_t, long_t, short_t]), [65, T, 65]
    ex = np.zeros(sum(lengths), np.int32)
    ex[65 + 2000:65 + 2040] = 1
    ex[65 + 4095] = 1
    for rule in (sc.RULE, sc.rule_of(1, 8, 1, 32), sc.rule_of(2, 256, 32, 1024)):
        out = numpy_out(model.gait_spectrum(joints, lengths, trans, ex, **rule))
        host = pkg.pipeline.gait_spectrum(joints, lengths, trans, ex, **rule)
        assert same(out, host) and np.isfinite(host["psd"][1, :3]).all(), rule
        assert sc.same_bits(out["psd"][0], out["psd"][2]) and sc.same_bits(out["per_sequence"][0], out["per_sequence"][2])
    assert host["per_sequence"][1, 0, 0] == T - 2 - 42 - 3
    many = pkg.pipeline.gait_spectrum(joints, lengths, trans, ex, **sc.rule_of(1, 8, 1, 32))["per_sequence"]
    assert many[1, 0, 2] > sc.LDS_SEGMENTS > many[0, 0, 2] > 0


def test_more_segments_than_the_lds_lists_hold_through_the_hook(model, pkg):
    """600 frames in LDS with 8-frame segments one frame apart: 593 segments > spectrum_checks.LDS_SEGMENTS = 512, so starts and means lie in the
    call's scratch while the signal stays in LDS; 519 frames hold exactly 512, 520 one more."""
    rng = np.random.default_rng(512)
    lengths = [600, 519, 520, 40]
    x = rng.standard_normal((sum(lengths), 4))
    rule = sc.rule_of(0, 8, 1, 8)
    host = pkg.pipeline.gait_welch(x, lengths, **rule)
    assert host["per_sequence"][:, 0, 2].tolist() == [593, sc.LDS_SEGMENTS, sc.LDS_SEGMENTS + 1, 33]
    assert same(numpy_out(model.op_gait_welch(x, lengths, **rule), hook=True), host)
    x[300, :] = np.nan
    for rule in (sc.rule_of(0, 8, 1, 8), sc.rule_of(1, 8, 1, 514), sc.rule_of(2, 8, 2, 64)):
        assert same(numpy_out(model.op_gait_welch(x, lengths, **rule), hook=True), pkg.pipeline.gait_welch(x, lengths, **rule)), rule


def test_runs_at_the_word_boundary_and_of_a_segment_s_length_through_the_hook(model, pkg):
    for segment, hop, nfft in ((64, 32, 256), (8, 4, 32), (64, 8, 64)):
        x, lengths, ex = sc.runs_call(segment, hop)
        for d in (0, 1, 2):
            rule = sc.rule_of(d, segment, hop, nfft, min_segments=1)
            host = pkg.pipeline.gait_welch(x, lengths, ex, **rule)
            assert same(numpy_out(model.op_gait_welch(x, lengths, ex, **rule), hook=True), host), rule
            if d == 0:      # a run of L - 1 frames lays no segment, one of L one, one of L + hop two; behind each lies one more run of L
                assert host["per_sequence"][9:, 0, 1].tolist() == [1, 0, 2, 1, 3, 2]


def test_exact_bin_sinusoid_and_constant_through_the_hook(model, pkg):
    for k0 in (8, 13, 30):
        x = sc.sinusoid(k0)
        out = numpy_out(model.op_gait_welch(x, **sc.rule_of(0, 64, 32, 256)), hook=True)
        assert same(out, pkg.pipeline.gait_welch(x, **sc.rule_of(0, 64, 32, 256)))
        row = out["per_sequence"][0]
        assert (row[:, 5] == k0).all() and (np.abs(row[:, 6] - k0 * 20.0 / 256) <= 0.5 * 20.0 / 256).all()
        assert sc.same_bits(row[:3, 12], 120.0 * row[:3, 6]) and row[3, 12] == 60.0 * row[3, 6] and (row[:, 4] >= row[:, 3]).all()
    flat = numpy_out(model.op_gait_welch(np.full((400, 4), 1.5), **sc.rule_of(0, 64, 32, 256)), hook=True)
    assert (flat["psd"] == 0).all() and (flat["per_sequence"][0, :, :5] == [400, 11, 11, 0, 0]).all() and np.isnan(flat["per_sequence"][0, :, 5:]).all()
    short = numpy_out(model.op_gait_welch(np.random.default_rng(3).standard_normal((95, 4)), **sc.rule_of(0, 64, 32, 256)), hook=True)
    assert np.isnan(short["psd"]).all() and (short["per_sequence"][0, :, :3] == [95, 1, 0]).all() and np.isnan(short["per_sequence"][0, :, 3:]).all()


def test_the_longest_sequence_through_the_hook(model, pkg):
    """32 768 frames, the most a call takes, at the widest transform and with eight-frame segments a frame apart (32 761 of them, in the scratch at
    the largest offsets the call reaches); a short sequence lies behind it and must not be touched.  The statement is held on the short rule alone
    and on the long one by a sample of bins, so that the test stays quick: the bins a lane owns do not depend on one another."""
    T = 32768
    rng = np.random.default_rng(32768)
    x = np.concatenate([0.01 * rng.standard_normal((T, 4)), rng.standard_normal((70, 4))])
    x[T - 9, :] = np.nan
    rule = sc.rule_of(2, 256, 256, 1024)
    assert same(numpy_out(model.op_gait_welch(x, [T, 70], **rule), hook=True), pkg.pipeline.gait_welch(x, [T, 70], **rule))
    rule = sc.rule_of(0, 8, 1, 8)
    out = numpy_out(model.op_gait_welch(x, [T, 70], **rule), hook=True)
    assert same(out, pkg.pipeline.gait_welch(x, [T, 70], **rule)) and out["per_sequence"][0, 0, 2] == T - 9 - 7 + 1 and out["per_sequence"][1, 0, 2] == 63


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    signals = torch.zeros(8, 4, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    psd = torch.full((2, 4, 5), -7.0, dtype=torch.float64, device="cuda")
    per_seq = torch.full((2, 4, 13), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, fps=20.0, sigma=1.0, derivative=2, segment=8, hop=4, nfft=8, f_lo=0.5, f_hi=3.0, min_segments=2, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, None, None, fps, sigma, derivative, segment, hop, nfft, f_lo, f_hi,
                min_segments, per_frame.data_ptr(), psd.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_spectrum(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, fps=20.0, derivative=2, segment=8, hop=4, nfft=8, f_lo=0.5, f_hi=3.0, min_segments=2, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, signals.data_ptr(), None, off, len(offsets) - 1 if n_seq is None else n_seq, fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments,
                psd.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_welch(*args)

    rule = ((dict(fps=0.0), b"fps"), (dict(fps=nan), b"fps"), (dict(fps=inf), b"fps"), (dict(derivative=-1), b"derivative"), (dict(derivative=3), b"derivative"),
            (dict(segment=6, hop=3), b"segment must be even and within [8, 256]"), (dict(segment=9), b"segment"), (dict(segment=258, hop=129, nfft=512), b"segment"),
            (dict(segment=64, hop=7, nfft=64), b"hop outside [segment / 8, segment]"), (dict(hop=9), b"hop"), (dict(segment=16, hop=8, nfft=14), b"nfft must be even and within [segment, 1024]"),
            (dict(nfft=9), b"nfft"), (dict(nfft=1026), b"nfft"), (dict(f_lo=0.0), b"0 < f_lo < f_hi <= fps / 2"), (dict(f_lo=3.0), b"f_lo"), (dict(f_hi=10.5), b"f_lo"),
            (dict(f_lo=nan), b"f_lo"), (dict(min_segments=0), b"min_segments outside [1, 2^20]"), (dict(min_segments=2 ** 20 + 1), b"min_segments"), (dict(n_seq=0), b"n_seq 0"),
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
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((psd == -7.0).all()) and bool((per_seq == -7.0).all())      # nothing was written
    assert run() == 0                                           # every joint at (1, 1, 1): no axes, and no trans
    torch.cuda.synchronize()
    assert bool(per_frame.isnan().all()) and bool(psd.isnan().all()) and bool((per_seq[:, :, :3] == 0).all()) and bool(per_seq[:, :, 3:].isnan().all())
    psd.fill_(-7.0)
    assert hook(offsets=(0, 3, 8), derivative=0, min_segments=1) == 0      # constant signals of 3 and 5 frames: no segment of 8
    torch.cuda.synchronize()
    assert per_seq[:, :, 0].tolist() == [[3.0] * 4, [5.0] * 4] and bool((per_seq[:, :, 1:3] == 0).all()) and bool(psd.isnan().all())
    ok = np.ones((4, 25, 3), np.float32)
    for args, kw, word in (((ok[0],), {}, "joints3d"), ((ok,), {"lengths": [2, 1]}, "lengths"), ((ok,), {"joints": (0, 1, 2)}, "joints"), ((ok,), {"trans": np.zeros((3, 3))}, "trans"),
                           ((ok,), {"exclude": np.zeros(3)}, "exclude"), ((ok,), {"nfft": 2.5}, "nfft"), ((ok,), {"nfft": 1026}, "nfft")):
        with pytest.raises(ValueError, match=word):
            model.gait_spectrum(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"segment": 6}, "segment"), ({"f_lo": 0.0}, "f_lo"), ({"derivative": 3}, "derivative"), ({"hop": 3}, "hop")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_spectrum(ok, **kw)


def test_window_spectrum_on_a_real_handle(model, pkg, tmp_path, capsys):
    """batch_generation.WindowSpectrum for one window of 3 videos: the device path writes what the host path writes, with a turn's phase as exclude."""
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
        bands = bg.WindowSpectrum(pkg.pipeline, model, on_host, True)
        assert (bands.device_call is None) == on_host
        bands.add_window(keys, per_video, fitted, phase)
        files[on_host] = json.load(open(bands.write(str(tmp_path / f"spectrum{int(on_host)}.json"))))
    assert files[False] == files[True] and sorted(files[False]) == sorted(keys)
    long = files[False]["walk400_back"]
    assert long["straight_only"] is True and long["sep"]["n"] == 400 - 2 - 42 and long["sep"]["candidates"] == 3 + 5 and len(long["sep"]["psd"]) == 129 == len(long["freqs"])
    assert abs(long["sep"]["peak_hz"] - 20.0 / 27.3) < 20.0 / 256 and long["bob"]["used"] > 0 and 0 < long["sep"]["spectral_entropy"] < 1
    assert files[False]["degenerate65"]["sep"]["used"] == 0 and files[False]["degenerate65"]["sep"]["peak_hz"] is None
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Spectrum:")]
    assert len(lines) == 6 and lines[:3] == lines[3:] and all(ln.endswith(", straight walking only.") for ln in lines)
