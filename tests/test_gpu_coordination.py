"""Arm swing and inter-limb coordination on the GPU (grnet_gait_coordination, csrc/gait_coordination_kernels.hip) against the host
statement pipeline.gait_coordination on the articulated noisy walker of tests/helpers/coordination_checks.py and on hand-made signals through the
hook, at the smallest shapes that can break a stage: sequences of 1, 19, 20, 64, 65, 130 and 400 frames, one and seven a call, a standing body,
J = 25 and 49, with and without exclude, derivative 0, 1 and 2, segments of 8, 64 and 256 frames, hops of an eighth, a half and a whole segment,
nfft = segment, 256, 510, 512 and 514 (256, 257 and 258 bins: a block of 64 bins fewer, just full, and one more) and 1024, runs of validity that
begin and end at the frames 63, 64 and 65, runs exactly segment - 1, segment and segment + hop long, a sequence one frame longer than the LDS array
(coordination_checks.LDS_FRAMES = 1024, csrc/kernels.h's kCoordLdsFrames), more segments than the LDS lists hold (LDS_SEGMENTS = 128), and the
longest sequence a call takes.

The kernel adds nothing across lanes and its arctangent is gait_atan2: device and statement must agree, with sigma = 0, in every bit of per_frame,
auto, cross, limbs and pairs, and so the device inherits the statement's bars against the numpy.fft yardstick (tests/test_coordination_host_cpu.py).
With sigma > 0 the device's Gaussian has its own order of the sum: per_frame is held to the Gaussian's bar (kinematics_checks.column_bars), and the
rest must equal what pipeline.gait_cross_welch makes of the DEVICE'S OWN per_frame."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from .helpers import coordination_checks as cc
from .helpers import kinematics_checks as kc

pytestmark = pytest.mark.gpu
KEYS = ("auto", "cross", "limbs", "pairs")


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == sorted(KEYS + (() if hook else ("per_frame",)))
    assert all(v.is_cuda and v.dtype == torch.float64 for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, rule, with_exclude):
    """The statement with sigma = 0 of the seven sequences, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, lengths, _, ex, table = cc.noisy_call(J)
    return pipe.gait_coordination(joints, lengths, ex if with_exclude else None, joints=table, **cc.rule_of(*rule))


def same(out, host):
    return all(cc.same_bits(out[k], host[k]) for k in KEYS + (("per_frame",) if "per_frame" in out else ()))


@pytest.mark.parametrize("with_exclude", (False, True))
@pytest.mark.parametrize("J,rule", tuple((25, r) for r in cc.RULES) + ((49, cc.RULES[0]), (49, cc.RULES[6])))
def test_every_bit_of_the_statement_without_smoothing(model, pkg, J, rule, with_exclude):
    joints, lengths, names, ex, table = cc.noisy_call(J)
    host = statement(pkg.__name__, J, rule, with_exclude)
    out = numpy_out(model.gait_coordination(joints, lengths, ex if with_exclude else None, joints=table, **cc.rule_of(*rule)))
    bins = rule[3] // 2 + 1
    assert out["auto"].shape == (7, 4, bins) and out["cross"].shape == (7, 6, bins, 2) and out["limbs"].shape == (7, 4, 13) and out["pairs"].shape == (7, 6, 10)
    assert out["per_frame"].shape == (sum(lengths), 4)
    for k in ("per_frame",) + KEYS:
        assert cc.same_bits(out[k], host[k]), f"{k} differs in some bit"
    seq = dict(zip(names, host["limbs"]))
    assert (seq["one"][:, 1:3] == 0).all() and np.isnan(seq["one"][:, 3:]).all()      # what the shapes are there for
    if not with_exclude:                                        # behind the excluded frames the 400-frame walker holds one segment of 256, 128 apart
        assert (seq["walk400"][:, 2] >= rule[4]).all() and np.isfinite(host["pairs"][names.index("walk400")]).all()
    if rule == cc.RULES[0] and not with_exclude:
        assert (seq["walk400"][:, 2] == 11).all() and (host["pairs"][names.index("walk400"), :, 1] == 12).all()


def test_per_frame_is_gait_kinematics_s(model, pkg):
    joints, lengths, _, ex, table = cc.noisy_call(25)
    events = np.zeros(len(joints), np.int32)
    for sigma in (0.0, 2.0):
        a = model.gait_coordination(joints, lengths, ex, sigma=sigma, joints=table)["per_frame"].cpu().numpy()
        b = model.gait_kinematics(joints, events, lengths, sigma=sigma, joints=table)["per_frame"].cpu().numpy()
        assert cc.same_bits(a, b[:, cc.KIN_COLUMNS]), sigma


@pytest.mark.parametrize("n_seq", (1, 7))
def test_smoothed_signals_within_the_gaussian_bar_and_the_rest_from_them(model, pkg, n_seq):
    joints, lengths, names, ex, table = cc.noisy_call(25)
    if n_seq == 1:
        joints, lengths, ex = joints[:130], lengths[:1], ex[:130]
    raw = pkg.pipeline.gait_coordination(joints, lengths, joints=table)["per_frame"]
    host = pkg.pipeline.gait_coordination(joints, lengths, ex, sigma=2.0, joints=table)
    out = numpy_out(model.gait_coordination(joints, lengths, ex, sigma=2.0, joints=table, **cc.RULE))
    assert np.array_equal(np.isnan(out["per_frame"]), np.isnan(host["per_frame"]))
    worst, a = 0.0, 0
    for T in lengths:
        raw13 = np.full((T, 13), np.nan)
        raw13[:, cc.KIN_COLUMNS] = raw[a:a + T]
        b = kc.column_bars(raw13, 2.0)[0][list(cc.KIN_COLUMNS)]
        for k in range(4):
            fin = np.isfinite(host["per_frame"][a:a + T, k])
            if fin.any() and b[k] > 0:
                worst = max(worst, float(np.abs(out["per_frame"][a:a + T, k] - host["per_frame"][a:a + T, k])[fin].max()) / b[k])
            else:
                assert cc.same_bits(out["per_frame"][a:a + T, k], host["per_frame"][a:a + T, k])
        a += T
    print(f"sigma 2, {n_seq} sequence(s): worst signal error / bar = {worst:.3g}")
    assert worst <= 1.0
    again = pkg.pipeline.gait_cross_welch(out["per_frame"], lengths, ex, **cc.RULE)
    assert all(cc.same_bits(out[k], again[k]) for k in KEYS)


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_one_sequence_alone_among_six_others_and_twice(model, pkg, sigma):
    joints, lengths, names, ex, table = cc.noisy_call(25)
    rule = cc.rule_of(1, 8, 4, 32)
    whole = numpy_out(model.gait_coordination(joints, lengths, ex, sigma=sigma, joints=table, **rule))
    again = numpy_out(model.gait_coordination(joints, lengths, ex, sigma=sigma, joints=table, **rule))
    assert same(whole, again)
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_coordination(joints[a:a + n], None, ex[a:a + n], sigma=sigma, joints=table, **rule))
        assert cc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]), names[q]
        assert all(cc.same_bits(alone[k][0], whole[k][q]) for k in KEYS), names[q]
        a += n


def test_auto_is_op_gait_welch_s_psd_on_all_valid_signals(model, pkg):
    x = np.random.default_rng(4).standard_normal((700, 4))
    lengths = [400, 65, 235]
    for d, L, hop, N, m in (cc.RULES[0], cc.RULES[2], cc.RULES[6], cc.RULES[7]):
        rule = cc.rule_of(d, L, hop, N, m)
        out = numpy_out(model.op_gait_cross_welch(x, lengths, **rule), hook=True)
        welch = model.op_gait_welch(x, lengths, **rule)
        assert cc.same_bits(out["auto"], welch["psd"].cpu().numpy()), rule
        assert cc.same_bits(out["limbs"][:, :, :12], welch["per_sequence"].cpu().numpy()[:, :, :12]), rule


def test_hand_cases_through_the_hook(model, pkg):
    a = cc.hand_signals()
    rule = cc.rule_of(0, 64, 32, 64)
    pure = np.sin(2.0 * np.pi * 4.0 * np.arange(402) / 64.0)
    hole = np.random.default_rng(8).standard_normal((400, 4))
    hole[150:190, 2] = np.nan
    for x, r in ((np.stack([a, a, a, a], axis=1), rule), (np.stack([a, -a, a, -a], axis=1), rule), (np.stack([pure[2:], pure[:-2], pure[2:], pure[:-2]], axis=1), rule),
                 (hole, cc.RULE), (np.full((400, 4), 1.5), cc.RULE)):
        out = numpy_out(model.op_gait_cross_welch(x, **r), hook=True)
        assert same(out, pkg.pipeline.gait_cross_welch(x, **r))
    same_out = numpy_out(model.op_gait_cross_welch(np.stack([a, a, a, a], axis=1), **rule), hook=True)
    assert (same_out["pairs"][0, :, 4] == 1.0).all() and (same_out["cross"][0, :, :, 1] == 0).all() and not np.signbit(same_out["cross"][0, :, :, 1]).any()
    late = numpy_out(model.op_gait_cross_welch(np.stack([pure[2:], pure[:-2], pure[2:], pure[:-2]], axis=1), **rule), hook=True)
    assert late["pairs"][0, 0, 1] == 4 and abs(late["pairs"][0, 0, 5] + 45.0) <= cc.BARS["phase_peak"]      # b lags a: a negative phase
    assert (out["auto"] == 0).all() and (out["cross"] == 0).all() and (out["limbs"][0, :, :5] == [400, 11, 11, 0, 0]).all() and np.isnan(out["pairs"][0, :, 1:]).all()


def test_edge_shapes_through_the_hook(model, pkg):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((160, 4))
    for signals in (x[:1], x[:159], x):                         # one frame; 3 candidates < min_segments = 4; 4 candidates
        out = numpy_out(model.op_gait_cross_welch(signals, **cc.RULE), hook=True)
        assert same(out, pkg.pipeline.gait_cross_welch(signals, **cc.RULE))
    assert (out["limbs"][0, :, :3] == [160, 4, 4]).all()
    for segment, hop, nfft in ((64, 32, 256), (8, 4, 32), (64, 8, 64)):
        x, lengths, ex = cc.runs_call(segment, hop)
        for d in (0, 1, 2):
            rule = cc.rule_of(d, segment, hop, nfft, 2)
            host = pkg.pipeline.gait_cross_welch(x, lengths, ex, **rule)
            assert same(numpy_out(model.op_gait_cross_welch(x, lengths, ex, **rule), hook=True), host), rule
            if d == 0:
                assert host["limbs"][9:, 0, 1].tolist() == [1, 0, 2, 1, 3, 2]
    joints, lengths, names, ex, table = cc.noisy_call(25)
    standing = names.index("standing64")
    still = joints[sum(lengths[:standing]):][:64]
    out = numpy_out(model.gait_coordination(still, joints=table, **cc.rule_of(0, 8, 4, 32)))
    assert same(out, pkg.pipeline.gait_coordination(still, joints=table, **cc.rule_of(0, 8, 4, 32)))
    assert (out["auto"] == 0).all() and (out["limbs"][0, :, 2] == 15).all() and np.isnan(out["pairs"][0, :, 1:]).all()      # no peak, nothing divided by 0


def test_a_sequence_one_frame_longer_than_the_lds_array_through_the_hook(model, pkg):
    """1025 frames > 1024: the four differenced columns lie in the workgroup's span of the call's scratch and go through the same code; beside it a
    short one, first and last.  With 8-frame segments one frame apart the long sequence also holds more segments than the LDS lists (128), the
    short ones do not: every form of the kernel's stages runs."""
    T = cc.LDS_FRAMES + 1
    rng = np.random.default_rng(1025)
    short = rng.standard_normal((65, 4))
    x = np.concatenate([short, rng.standard_normal((T, 4)), short])
    lengths = [65, T, 65]
    ex = np.zeros(sum(lengths), np.int32)
    ex[65 + 500:65 + 540] = 1
    ex[65 + 1023] = 1
    x[65 + 700, 1] = np.nan
    for rule in (cc.RULE, cc.rule_of(1, 8, 1, 32), cc.rule_of(2, 256, 32, 1024, 2), cc.rule_of(0, 64, 32, 514)):
        out = numpy_out(model.op_gait_cross_welch(x, lengths, ex, **rule), hook=True)
        host = pkg.pipeline.gait_cross_welch(x, lengths, ex, **rule)
        assert same(out, host) and np.isfinite(host["auto"][1]).all(), rule
        assert all(cc.same_bits(out[k][0], out[k][2]) for k in KEYS)
    many = pkg.pipeline.gait_cross_welch(x, lengths, ex, **cc.rule_of(1, 8, 1, 32))["limbs"]
    assert many[1, 0, 2] > cc.LDS_SEGMENTS > many[0, 0, 2] > 0
    exact = numpy_out(model.op_gait_cross_welch(x[65:65 + cc.LDS_FRAMES], **cc.RULE), hook=True)      # exactly the LDS array
    assert same(exact, pkg.pipeline.gait_cross_welch(x[65:65 + cc.LDS_FRAMES], **cc.RULE))


def test_more_segments_than_the_lds_lists_hold_through_the_hook(model, pkg):
    """300 frames in LDS with 8-frame segments one frame apart: 293 segments > coordination_checks.LDS_SEGMENTS = 128, so starts and means lie in the
    call's scratch while the signals stay in LDS; 135 frames hold exactly 128, 136 one more."""
    rng = np.random.default_rng(128)
    lengths = [300, 135, 136, 40]
    x = rng.standard_normal((sum(lengths), 4))
    rule = cc.rule_of(0, 8, 1, 8)
    host = pkg.pipeline.gait_cross_welch(x, lengths, **rule)
    assert host["limbs"][:, 0, 2].tolist() == [293, cc.LDS_SEGMENTS, cc.LDS_SEGMENTS + 1, 33]
    assert same(numpy_out(model.op_gait_cross_welch(x, lengths, **rule), hook=True), host)
    x[150, 3] = np.nan
    for rule in (cc.rule_of(0, 8, 1, 8), cc.rule_of(1, 8, 1, 514), cc.rule_of(2, 8, 2, 64), cc.rule_of(0, 8, 1, 510), cc.rule_of(0, 8, 1, 512)):
        assert same(numpy_out(model.op_gait_cross_welch(x, lengths, **rule), hook=True), pkg.pipeline.gait_cross_welch(x, lengths, **rule)), rule


def test_the_longest_sequence_through_the_hook(model, pkg):
    """32 768 standard-normal frames, the most a call takes, at the defaults (1023 segments in the scratch at the largest offsets the call reaches); a
    short sequence lies behind it and must not be touched."""
    T = 32768
    rng = np.random.default_rng(32768)
    x = np.concatenate([rng.standard_normal((T, 4)), rng.standard_normal((200, 4))])
    out = numpy_out(model.op_gait_cross_welch(x, [T, 200], **cc.RULE), hook=True)
    host = pkg.pipeline.gait_cross_welch(x, [T, 200], **cc.RULE)
    assert same(out, host) and (out["limbs"][:, 0, 2] == [1023, 5]).all()
    print("coherence of unrelated signals over 1023 segments:", out["pairs"][0, :, 8])
    assert (out["pairs"][0, :, 8] < 0.01).all()                 # about 1 / K


def test_white_noise_anchor(model, pkg):
    worst = 0.0
    for seed in cc.WHITE_SEEDS[:4]:
        out = numpy_out(model.op_gait_cross_welch(cc.white_noise(seed), **cc.WHITE_RULE), hook=True)
        assert (out["limbs"][0, :, 2] == cc.WHITE_K).all()
        mean = cc.white_mean(out["auto"][0], out["cross"][0, :, :, 0], out["cross"][0, :, :, 1])
        print(f"seed {seed}: mean coherence {mean:.5f}, 1 / K {1.0 / cc.WHITE_K:.5f}, bar {cc.WHITE_BAR}")
        worst = max(worst, abs(mean - 1.0 / cc.WHITE_K))
    assert worst <= cc.WHITE_BAR


def test_window_coordination_on_a_real_handle(model, pkg, tmp_path, capsys):
    """batch_generation.WindowCoordination for one window of 3 videos: the device path writes what the host path writes, with a turn's phase as exclude."""
    import importlib
    import json
    bg = importlib.import_module("batch_generation")            # tests/conftest.py puts the repository's root on the path
    joints, lengths, names, _, _ = cc.noisy_call(25)
    off = np.concatenate([[0], np.cumsum(lengths)])
    keys = ["walk130", "standing64", "walk400"]
    picked = [names.index(k) for k in keys]
    per_video = [torch.from_numpy(joints[off[q]:off[q + 1]].reshape(-1, 75)).cuda() for q in picked]
    phase = [np.zeros(lengths[q], np.int32) for q in picked]
    phase[2][150:190] = 1
    files = {}
    for on_host in (False, True):
        limbs = bg.WindowCoordination(pkg.pipeline, model, on_host, True)
        assert (limbs.device_call is None) == on_host
        limbs.add_window(keys, per_video, phase)
        files[on_host] = json.load(open(limbs.write(str(tmp_path / f"coordination{int(on_host)}.json"))))
    assert files[False] == files[True] and sorted(files[False]) == sorted(keys)
    long = files[False]["walk400"]
    assert long["straight_only"] is True and long["arm_left"]["n"] == 360 and long["arm_left"]["candidates"] == 3 + 5 and len(long["freqs"]) == 129
    assert long["arm_left__arm_right"]["peak_bin"] == 12 and long["arm_left__arm_right"]["coherence_peak"] > 0.9 and abs(long["arm_asymmetry"] - 50.0) < 5.0
    assert files[False]["standing64"]["arm_left"]["used"] == 0 and files[False]["standing64"]["arm_left__arm_right"]["phase_peak"] is None
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Coordination:")]
    assert len(lines) == 6 and lines[:3] == lines[3:] and all(ln.endswith(", straight walking only.") for ln in lines)


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    signals = torch.zeros(8, 4, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    au = torch.full((2, 4, 5), -7.0, dtype=torch.float64, device="cuda")
    cr = torch.full((2, 6, 5, 2), -7.0, dtype=torch.float64, device="cuda")
    limbs = torch.full((2, 4, 13), -7.0, dtype=torch.float64, device="cuda")
    pairs = torch.full((2, 6, 10), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=kc.KINECTV2, fps=20.0, sigma=1.0, derivative=2, segment=8, hop=4, nfft=8, f_lo=0.5, f_hi=3.0, min_segments=2, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 16)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, None, fps, sigma, derivative, segment, hop, nfft, f_lo, f_hi,
                min_segments, per_frame.data_ptr(), au.data_ptr(), cr.data_ptr(), limbs.data_ptr(), pairs.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_coordination(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, fps=20.0, derivative=2, segment=8, hop=4, nfft=8, f_lo=0.5, f_hi=3.0, min_segments=2, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, signals.data_ptr(), None, off, len(offsets) - 1 if n_seq is None else n_seq, fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments,
                au.data_ptr(), cr.data_ptr(), limbs.data_ptr(), pairs.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_cross_welch(*args)

    rule = ((dict(fps=0.0), b"fps"), (dict(fps=nan), b"fps"), (dict(fps=inf), b"fps"), (dict(derivative=-1), b"derivative"), (dict(derivative=3), b"derivative"),
            (dict(segment=6, hop=3), b"segment must be even and within [8, 256]"), (dict(segment=9), b"segment"), (dict(segment=258, hop=129, nfft=512), b"segment"),
            (dict(segment=64, hop=7, nfft=64), b"hop outside [segment / 8, segment]"), (dict(hop=9), b"hop"), (dict(segment=16, hop=8, nfft=14), b"nfft must be even and within [segment, 1024]"),
            (dict(nfft=9), b"nfft"), (dict(nfft=1026), b"nfft"), (dict(f_lo=0.0), b"0 < f_lo < f_hi <= fps / 2"), (dict(f_lo=3.0), b"f_lo"), (dict(f_hi=10.5), b"f_lo"),
            (dict(f_lo=nan), b"f_lo"), (dict(min_segments=0), b"min_segments outside [2, 2^20]"), (dict(min_segments=1), b"min_segments outside [2, 2^20]"),
            (dict(min_segments=2 ** 20 + 1), b"min_segments"), (dict(n_seq=0), b"n_seq 0"),
            (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"),
            (dict(offsets=(0, 3, 3 + 32769)), b"sequence 1 has 32769 frames, more than 32768"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 16, 17, 18, 19, 20)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 13, 17, 14, 18, 15, 19, 4, 8, 5, 9, -1, 10)), b"joint index -1"),
            (dict(sigma=-1.0), b"sigma"), (dict(sigma=nan), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(n_seq=-2), b"n_seq -2")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 13, 14, 15, 16)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (per_frame, au, cr, limbs, pairs))      # nothing was written
    assert run() == 0                                           # every joint at (1, 1, 1): no axes
    torch.cuda.synchronize()
    assert bool(per_frame.isnan().all()) and bool(au.isnan().all()) and bool(cr.isnan().all()) and bool((limbs[:, :, :3] == 0).all()) and bool(limbs[:, :, 3:].isnan().all())
    assert bool((pairs[:, :, 0] == 0).all()) and bool(pairs[:, :, 1:].isnan().all())
    au.fill_(-7.0)
    assert hook(offsets=(0, 3, 8), derivative=0) == 0           # constant signals of 3 and 5 frames: no segment of 8
    torch.cuda.synchronize()
    assert limbs[:, :, 0].tolist() == [[3.0] * 4, [5.0] * 4] and bool((limbs[:, :, 1:3] == 0).all()) and bool(au.isnan().all())
    ok = np.ones((4, 25, 3), np.float32)
    for args, kw, word in (((ok[0],), {}, "joints3d"), ((ok,), {"lengths": [2, 1]}, "lengths"), ((ok,), {"joints": (0, 1, 2)}, "joints"),
                           ((ok,), {"exclude": np.zeros(3)}, "exclude"), ((ok,), {"nfft": 2.5}, "nfft"), ((ok,), {"nfft": 1026}, "nfft")):
        with pytest.raises(ValueError, match=word):
            model.gait_coordination(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"segment": 6}, "segment"), ({"f_lo": 0.0}, "f_lo"), ({"derivative": 3}, "derivative"), ({"hop": 3}, "hop"),
                     ({"min_segments": 1}, "min_segments")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_coordination(ok, **kw)
