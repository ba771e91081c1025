"""Recurrence quantification of the gait signals on the GPU (grnet_gait_recurrence, csrc/gait_recurrence_kernels.hip) against the host
statement pipeline.gait_recurrence on the noisy walker of tests/helpers/entropy_checks.py, at the smallest shapes that can break a stage: sequences
of 1, 19, 20, 64, 65, 130 and 400 frames, one and seven sequences a call, a standing body, J = 25 and 49 (with another table), derivative 0, 1 and 2,
dim 2, 5 and 8, lag 1, 2 and 16, theiler 0, 1, 8 and larger than every M, radius 0.2, 0.8 and 10, with and without trans and exclude; through the
hook M = 511 .. 516 and 1023 .. 1028 (offsets around one and two blocks of 256 lanes), the hand-made signals with their lines of more than 255 pairs,
lines of exactly 255 and 256 pairs, runs of validity that begin and end at the frames 63, 64 and 65, a sequence longer than the LDS array between two
short ones, a sequence with more offsets than 16 parts of 256 lanes take in one round, the longest sequence a call takes, and white noise against
1 - exp(-1/2).

counts and hist are integers: device and statement must agree in every one of them, in every bit of per_sequence and, with sigma = 0, of per_frame.
With sigma > 0 the device's Gaussian has its own order of the sum: per_frame is held to the Gaussian's bar (gait_checks.signal_bars), and the rest
must equal what pipeline.gait_recurrence_counts makes of the DEVICE'S OWN per_frame.  Rule 6's invariant is asserted on every output."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from .helpers import gait_checks as gc
from .helpers import recurrence_checks as kc
from .helpers import regularity_checks as rc

pytestmark = pytest.mark.gpu
KINDS = {"per_sequence": torch.float64, "hist": torch.int64, "counts": torch.int64, "per_frame": torch.float64}


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == ["counts", "hist"] + ([] if hook else ["per_frame"]) + ["per_sequence"]
    assert all(v.is_cuda and v.dtype == KINDS[k] for k, v in out.items())
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert kc.invariant(got["hist"], got["counts"]), "the lines' points are not the recurrent pairs"
    return got


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, rule, with_trans, with_exclude):
    """The statement with sigma = 0 of the seven sequences, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, trans, lengths, _, ex, table = kc.noisy_call(J)
    return pipe.gait_recurrence(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **kc.rule_of(*rule))


def same(out, host):
    return (kc.same_ints(out["counts"], host["counts"]) and kc.same_ints(out["hist"], host["hist"]) and kc.same_bits(out["per_sequence"], host["per_sequence"])
            and ("per_frame" not in out or kc.same_bits(out["per_frame"], host["per_frame"])))


@pytest.mark.parametrize("with_trans,with_exclude", ((True, False), (False, True), (True, True)))
@pytest.mark.parametrize("J,rule", tuple((25, r) for r in kc.RULES) + ((49, kc.RULES[0]), (49, kc.RULES[2])))
def test_every_integer_and_bit_of_the_statement_without_smoothing(model, pkg, J, rule, with_trans, with_exclude):
    joints, trans, lengths, names, ex, table = kc.noisy_call(J)
    host = statement(pkg.__name__, J, rule, with_trans, with_exclude)
    out = numpy_out(model.gait_recurrence(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **kc.rule_of(*rule)))
    assert out["counts"].shape == (7, 4, 6) and out["hist"].shape == (7, 4, 255) and out["per_sequence"].shape == (7, 4, 5) and out["per_frame"].shape == (sum(lengths), 4)
    assert kc.same_ints(out["counts"], host["counts"]), "counts differ"
    assert kc.same_ints(out["hist"], host["hist"]), "hist differs"
    for k in ("per_sequence", "per_frame"):
        assert kc.same_bits(out[k], host[k]), f"{k} differs in some bit"
    seq = dict(zip(names, host["counts"]))
    assert (seq["one"] == 0).all() and (seq["standing64"][:, 2:] == 0).all()                                # what the shapes are there for
    if rule[3] == 500:
        assert (host["counts"][:, :, 1:] == 0).all() and (host["hist"] == 0).all()
    elif rule == kc.RULES[0]:
        assert (seq["walk400_back"][:3, 2] >= 1000).all() and (seq["walk400_back"][:3, 5] >= 5).all()      # without trans there is no bob


def test_per_frame_is_gait_regularity_s(model, pkg):
    joints, trans, lengths, _, ex, _ = kc.noisy_call(25)
    for sigma in (0.0, 2.0):
        a = model.gait_recurrence(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        b = model.gait_regularity(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        assert kc.same_bits(a, b)


@pytest.mark.parametrize("n_seq", (1, 7))
def test_smoothed_signals_within_the_gaussian_bar_and_the_rest_from_them(model, pkg, n_seq):
    joints, trans, lengths, names, ex, table = kc.noisy_call(25)
    if n_seq == 1:
        joints, trans, lengths, ex = joints[:130], trans[:130], lengths[:1], ex[:130]
    raw = pkg.pipeline.gait_regularity(joints, lengths, trans)["per_frame"]
    host = pkg.pipeline.gait_regularity(joints, lengths, trans, ex, sigma=2.0)
    out = numpy_out(model.gait_recurrence(joints, lengths, trans, ex, sigma=2.0, **kc.RULE))
    assert np.array_equal(np.isnan(out["per_frame"]), np.isnan(host["per_frame"]))
    worst, a = 0.0, 0
    for T in lengths:
        b = gc.signal_bars(raw[a:a + T], 2.0)
        for k in range(4):
            fin = np.isfinite(host["per_frame"][a:a + T, k])
            if fin.any() and b[k] > 0:
                worst = max(worst, float(np.abs(out["per_frame"][a:a + T, k] - host["per_frame"][a:a + T, k])[fin].max()) / b[k])
            else:
                assert kc.same_bits(out["per_frame"][a:a + T, k], host["per_frame"][a:a + T, k])
        a += T
    print(f"sigma 2, {n_seq} sequence(s): worst signal error / bar = {worst:.3g}")
    assert worst <= 1.0
    again = pkg.pipeline.gait_recurrence_counts(out["per_frame"], lengths, ex, **kc.RULE)
    assert kc.same_ints(out["counts"], again["counts"]) and kc.same_ints(out["hist"], again["hist"]) and kc.same_bits(out["per_sequence"], again["per_sequence"])


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_one_sequence_alone_and_among_six_others(model, pkg, sigma):
    joints, trans, lengths, names, ex, _ = kc.noisy_call(25)
    whole = numpy_out(model.gait_recurrence(joints, lengths, trans, ex, sigma=sigma, **kc.RULE))
    again = numpy_out(model.gait_recurrence(joints, lengths, trans, ex, sigma=sigma, **kc.RULE))
    assert same(whole, again)
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_recurrence(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], sigma=sigma, **kc.RULE))
        assert kc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and kc.same_ints(alone["counts"][0], whole["counts"][q]), names[q]
        assert kc.same_ints(alone["hist"][0], whole["hist"][q]) and kc.same_bits(alone["per_sequence"][0], whole["per_sequence"][q]), names[q]
        a += n


def hook_equals_the_statement(model, pkg, x, lengths, ex, rule):
    host = pkg.pipeline.gait_recurrence_counts(x, lengths, ex, **rule)
    out = numpy_out(model.op_gait_recurrence_counts(x, lengths, ex, **rule), hook=True)
    assert kc.same_ints(out["counts"], host["counts"]), ("counts", rule, out["counts"].tolist(), host["counts"].tolist())
    assert kc.same_ints(out["hist"], host["hist"]) and kc.same_bits(out["per_sequence"], host["per_sequence"]), ("hist and per_sequence", rule)
    return host


def test_blocks_of_offsets_through_the_hook(model, pkg):
    """M = 511 .. 516 and 1023 .. 1028 at dim 2, lag 1 (M = T - 1): 255 .. 258 and 511 .. 514 offsets, one fewer than, as many as and more than the
    lanes of one and of two workgroups, odd and even M; then at the default rule with runs of validity that begin and end at the frames 63, 64, 65."""
    rng = np.random.default_rng(256)
    lengths = [1 + M for M in (511, 512, 513, 514, 515, 516, 1023, 1024, 1025, 1026, 1027, 1028)]
    x = rng.standard_normal((sum(lengths), 4))
    ex = np.zeros(sum(lengths), np.int32)
    host = hook_equals_the_statement(model, pkg, x, lengths, ex, kc.rule_of(0, 2, 1, 1, 0.8))
    assert host["counts"][:, 0, 0].tolist() == [T - 1 for T in lengths] and (host["counts"][:, :, 2] > 10000).all()
    a = 0
    for k, T in enumerate(lengths):
        x[a + (63, 64, 65)[k % 3], :] = np.nan
        ex[a + (65, 63, 64)[k % 3] + 64] = 1
        a += T
    for values in ((1, 5, 2, 8, 0.8), (2, 8, 16, 8, 10.0)):
        hook_equals_the_statement(model, pkg, x, lengths, ex, kc.rule_of(*values))


def test_a_sequence_longer_than_the_lds_array(model, pkg):
    """4100 frames > 4096: the pairs kernel reads y from the call's scratch, through the same code; beside it a short sequence, first and last."""
    T = 4100
    rng = np.random.default_rng(41)
    short = rng.standard_normal((65, 4))
    x = np.concatenate([short, rng.standard_normal((T, 4)), short])
    lengths = [65, T, 65]
    ex = np.zeros(sum(lengths), np.int32)
    ex[65 + 2000:65 + 2040] = 1
    ex[65 + 4095] = 1
    x[65 + 1023, :] = np.nan
    host = hook_equals_the_statement(model, pkg, x, lengths, ex, kc.rule_of(0, 2, 1, 1, 0.8))
    assert (host["counts"][1, :, 0] >= 4000).all() and kc.same_ints(host["counts"][0], host["counts"][2]) and (host["counts"][1, :, 2] > 10 ** 6).all()


def test_more_offsets_than_one_round_of_sixteen_parts(model, pkg):
    """8300 standard-normal frames: 4149 offsets, more than 16 parts of 256 lanes take in one round, 3.4e7 pairs; a short sequence behind."""
    rng = np.random.default_rng(8300)
    x = rng.standard_normal((8300 + 40, 4))
    host = hook_equals_the_statement(model, pkg, x, [8300, 40], None, kc.rule_of(0, 2, 1, 1, 0.8))
    assert (host["counts"][0, :, 1] == 8297 * 8298 // 2).all() and (host["counts"][0, :, 2] > 5 * 10 ** 6).all()


def test_runs_at_the_word_boundary_through_the_hook(model, pkg):
    x, lengths, ex = kc.boundary_call()
    for values in ((1, 5, 2, 8, 0.8), (0, 2, 1, 0, 0.2), (2, 3, 16, 5, 10.0)):
        host = hook_equals_the_statement(model, pkg, x, lengths, ex, kc.rule_of(*values))
    assert (host["counts"][:5, :, 2] > 20).all()


def test_hook_on_the_hand_made_signals(model, pkg):
    x = kc.hand_signals(kc.HAND_PERIODIC_X)
    out = numpy_out(model.op_gait_recurrence_counts(x, **kc.HAND_PERIODIC_RULE), hook=True)
    for ch in range(4):
        assert out["counts"][0, ch].tolist() == kc.HAND_PERIODIC_COUNTS and out["hist"][0, ch].tolist() == kc.HAND_PERIODIC_HIST      # a run carried across the wrap would read 30
    out = numpy_out(model.op_gait_recurrence_counts(x, **kc.HAND_WIDE_RULE), hook=True)
    assert out["counts"][0, 3].tolist() == kc.HAND_WIDE_COUNTS and out["hist"][0, 3].tolist() == kc.HAND_WIDE_HIST
    rows = pkg.pipeline.recurrence_rows(out["counts"], out["hist"], min_points=10)
    assert (rows["lines"][0, 3], rows["line_points"][0, 3]) == kc.HAND_WIDE_LINES
    xl = kc.hand_signals(kc.HAND_LONG_X)
    out = numpy_out(model.op_gait_recurrence_counts(xl, **kc.HAND_PERIODIC_RULE), hook=True)
    assert out["counts"][0, 1].tolist() == kc.HAND_LONG_COUNTS and out["hist"][0, 1].tolist() == kc.HAND_LONG_HIST                    # 68 lines past the last bin
    xb = kc.hand_signals(kc.HAND_BROKEN_X)
    out = numpy_out(model.op_gait_recurrence_counts(xb, **kc.HAND_BROKEN_RULE), hook=True)
    assert out["counts"][0, 2].tolist() == kc.HAND_BROKEN_COUNTS and out["hist"][0, 2].tolist() == kc.HAND_BROKEN_HIST
    three = np.concatenate([x, xb[:9], xl, x])
    host = hook_equals_the_statement(model, pkg, three, [31, 9, 600, 31], None, kc.HAND_PERIODIC_RULE)
    assert host["counts"][3, 0].tolist() == kc.HAND_PERIODIC_COUNTS and host["counts"][2, 0].tolist() == kc.HAND_LONG_COUNTS


def test_lines_of_the_last_bin_and_the_first_long_one(model, pkg):
    """M = 257 points that all recur (radius 10): diagonal 1 is ONE line of 256 pairs, the first long one, diagonal 2 one of 255, the last bin."""
    x = np.random.default_rng(255).standard_normal((258, 4))
    host = hook_equals_the_statement(model, pkg, x, None, None, kc.rule_of(0, 2, 1, 0, 10.0))
    assert host["counts"][0, 0].tolist() == [257, 257 * 256 // 2, 257 * 256 // 2, 1, 256, 256] and host["hist"][0, 0].tolist() == [1] * 255


def test_standing_body_recurs_nowhere(model, pkg):
    joints, trans = rc.walker(64, still=True)
    out = numpy_out(model.gait_recurrence(joints, trans=trans, **kc.RULE))
    assert np.isfinite(out["per_frame"]).all() and (out["counts"][0, :, 0] == 55).all() and (out["counts"][0, :, 1] == 46 * 47 // 2).all()
    assert (out["counts"][0, :, 2:] == 0).all() and (out["hist"] == 0).all() and (out["per_sequence"][0, :, 3:] == 0).all()


def test_white_noise_against_the_closed_form(model, pkg):
    x = np.stack([kc.white_noise(seed) for seed in kc.WHITE_SEEDS[:4]], axis=1)
    out = numpy_out(model.op_gait_recurrence_counts(x, **kc.WHITE_RULE), hook=True)
    rows = pkg.pipeline.recurrence_rows(out["counts"], out["hist"])
    bar = 2.0 * kc.WHITE_MEASURED
    miss = np.abs(rows["recurrence_rate"][0] - kc.WHITE_CLOSED)
    print(f"rate {rows['recurrence_rate'][0].tolist()}, closed form {kc.WHITE_CLOSED:.5f}, worst miss {miss.max():.4f} (bar {bar:.4f})")
    assert (miss <= bar).all() and (out["counts"][0, :, 1] == 998 * 997 // 2).all()


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    signals = torch.zeros(8, 4, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    per_seq = torch.full((2, 4, 5), -7.0, dtype=torch.float64, device="cuda")
    hist = torch.full((2, 4, 255), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((2, 4, 6), -7, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = float("nan")

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, sigma=1.0, derivative=1, dim=2, lag=1, theiler=0, radius=0.8, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, None, None, sigma, derivative, dim, lag, theiler, radius,
                per_frame.data_ptr(), per_seq.data_ptr(), hist.data_ptr(), counts.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_recurrence(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, derivative=1, dim=2, lag=1, theiler=0, radius=0.8, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, signals.data_ptr(), None, off, len(offsets) - 1 if n_seq is None else n_seq, derivative, dim, lag, theiler, radius, per_seq.data_ptr(), hist.data_ptr(),
                counts.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_recurrence_counts(*args)

    radius = b"radius must be finite and within (0, 10]"
    rule = ((dict(derivative=-1), b"derivative outside [0, 2]"), (dict(derivative=3), b"derivative outside [0, 2]"), (dict(dim=1), b"dim outside [2, 8]"), (dict(dim=9), b"dim outside [2, 8]"),
            (dict(lag=0), b"lag outside [1, 16]"), (dict(lag=17), b"lag outside [1, 16]"), (dict(theiler=-1), b"theiler outside [0, 4096]"),
            (dict(theiler=4097), b"theiler outside [0, 4096]"), (dict(radius=0.0), radius), (dict(radius=-0.5), radius), (dict(radius=10.5), radius), (dict(radius=nan), radius),
            (dict(radius=float("inf")), radius), (dict(n_seq=0), b"n_seq 0"), (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"),
            (dict(offsets=(0, 3, 3 + 32769)), b"sequence 1 has 32769 frames, more than 32768 (the work is quadratic in them)"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 14, 15, 16, 17)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"), (dict(sigma=-1.0), b"sigma"),
            (dict(sigma=nan), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(n_seq=-2), b"n_seq -2")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 10, 11, 12)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((per_seq == -7.0).all()) and bool((hist == -7).all()) and bool((counts == -7).all())      # nothing was written
    assert run() == 0                                           # every joint at (1, 1, 1): no axes, and no trans
    torch.cuda.synchronize()
    assert bool(per_frame.isnan().all()) and bool((hist == 0).all()) and bool((counts == 0).all()) and bool((per_seq[:, :, 0] == 0).all()) and bool(per_seq[:, :, 1:].isnan().all())
    counts.fill_(-7)
    assert hook(derivative=0) == 0                              # constant signals: r = 0, every pair comparable, none recurrent
    torch.cuda.synchronize()
    assert counts[:, 0].tolist() == [[2, 1, 0, 0, 0, 0], [4, 6, 0, 0, 0, 0]] and bool((hist == 0).all()) and bool((per_seq[:, :, 2:] == 0).all())
    ok = np.ones((4, 25, 3), np.float32)
    for args, kw, word in (((ok[0],), {}, "joints3d"), ((ok,), {"lengths": [2, 1]}, "lengths"), ((ok,), {"joints": (0, 1, 2)}, "joints"), ((ok,), {"trans": np.zeros((3, 3))}, "trans"),
                           ((ok,), {"exclude": np.zeros(3)}, "exclude"), ((ok,), {"dim": 2.5}, "dim")):
        with pytest.raises(ValueError, match=word):
            model.gait_recurrence(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"dim": 1}, "dim outside"), ({"lag": 17}, "lag outside"), ({"theiler": -1}, "theiler outside"), ({"derivative": 3}, "derivative"),
                     ({"radius": 0.0}, "radius must be finite"), ({"radius": 11.0}, "radius must be finite")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_recurrence(ok, **kw)


def test_the_longest_sequence_through_the_hook(model, pkg):
    """32 768 frames, the most a call takes, at dim 8, lag 16 and theiler 4096: the largest offsets the call reaches, 16 parts of four rounds.  The
    signal is constant, so r = 0 and nothing recurs, and every point but the last is valid: comparable is the closed form sum over s > w of (V - s)
    over the V valid points, 4.1e8 (5.3e8 at theiler 8), which needs no statement.  A short noisy sequence lies behind it, whose workgroups past its
    one part return at once, and must equal the statement of it alone."""
    T, w = 32768, 4096
    rng = np.random.default_rng(32768)
    short = rng.standard_normal((300, 4))
    x = np.concatenate([np.full((T, 4), 0.5), short])
    rule = kc.rule_of(1, 8, 16, w, 0.8)
    out = numpy_out(model.op_gait_recurrence_counts(x, [T, 300], **rule), hook=True)
    M = T - 7 * 16 - 1                                          # the last point holds the last frame's difference, which is none
    want = (M - w - 1) * (M - w) // 2
    print("comparable", out["counts"][0, :, 1].tolist(), "closed form", want)
    assert want > 4 * 10 ** 8 and (out["counts"][0, :, 0] == M).all() and (out["counts"][0, :, 1] == want).all()
    assert (out["counts"][0, :, 2:] == 0).all() and (out["hist"][0] == 0).all() and (out["per_sequence"][0, :, 2:] == 0).all()
    host = pkg.pipeline.gait_recurrence_counts(short, **dict(rule, theiler=8))
    out = numpy_out(model.op_gait_recurrence_counts(x, [T, 300], **dict(rule, theiler=8)), hook=True)
    assert (out["counts"][0, :, 1] == (M - 9) * (M - 8) // 2).all() and (out["counts"][0, :, 2:] == 0).all()
    assert kc.same_ints(out["counts"][1], host["counts"][0]) and kc.same_ints(out["hist"][1], host["hist"][0]) and kc.same_bits(out["per_sequence"][1], host["per_sequence"][0])
    assert (host["counts"][0, :, 2] > 50).all()
