"""Sample entropy of the gait signals on the GPU (grnet_gait_entropy, csrc/gait_entropy_kernels.hip) against the host statement
pipeline.gait_entropy on the noisy walker of tests/helpers/entropy_checks.py, at the smallest shapes that can break a stage: sequences of 1, 19, 20,
64, 65, 130 and 400 frames, one and seven sequences a call, a standing body, a degenerate frame, J = 25 and 49 (with another table), m 1, 2 and 4,
derivative 0, 1 and 2, scales 1, 3 and 8 (several leave no template of the short sequences), with and without trans and exclude, 255 .. 258 and 511 .. 514 frames
(one template fewer than, as many as and one more than the workgroup's lanes, and than twice as many, at scales 1 and 2), runs of validity that begin and end at the frames 63, 64
and 65, a sequence longer than the LDS array, and the hand-made signal through the hook.

The counts are integers: device and statement must agree in every one, and, with sigma = 0, in every bit of per_frame and per_sequence.  With sigma
> 0 the device's Gaussian has its own order of the sum: per_frame is held to the Gaussian's bar (gait_checks.signal_bars), and counts and per_sequence
must equal what pipeline.gait_sampen makes of the DEVICE'S OWN per_frame."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from .helpers import entropy_checks as ec
from .helpers import gait_checks as gc
from .helpers import regularity_checks as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == ["counts"] + ([] if hook else ["per_frame"]) + ["per_sequence"]
    assert all(v.is_cuda and v.dtype == (torch.int64 if k == "counts" else torch.float64) for k, v in out.items())
    return {k: v.cpu().numpy() for k, v in out.items()}


def rule_of(m, d, scales, fraction=0.2):
    return dict(m=m, fraction=fraction, derivative=d, scales=scales)


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, rule, with_trans, with_exclude):
    """The statement with sigma = 0 of the seven sequences, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, trans, lengths, _, ex, table = ec.noisy_call(J)
    return pipe.gait_entropy(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **rule_of(*rule))


def same(out, host):
    return ec.same_counts(out["counts"], host["counts"]) and all(ec.same_bits(out[k], host[k]) for k in ("per_sequence",) + (("per_frame",) if "per_frame" in out else ()))


@pytest.mark.parametrize("with_trans,with_exclude", ((True, False), (False, True), (True, True)))
@pytest.mark.parametrize("J,rule", tuple((25, r) for r in ec.RULES) + ((49, ec.RULES[0]), (49, ec.RULES[2])))
def test_every_integer_and_bit_of_the_statement_without_smoothing(model, pkg, J, rule, with_trans, with_exclude):
    joints, trans, lengths, names, ex, table = ec.noisy_call(J)
    host = statement(pkg.__name__, J, rule, with_trans, with_exclude)
    out = numpy_out(model.gait_entropy(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **rule_of(*rule)))
    assert out["counts"].shape == (7, 4, rule[2], 3) and out["per_sequence"].shape == (7, 4, 4) and out["per_frame"].shape == (sum(lengths), 4)
    assert ec.same_counts(out["counts"], host["counts"]), "counts differ"
    for k in ("per_frame", "per_sequence"):
        assert ec.same_bits(out[k], host[k]), f"{k} differs in some bit"
    seq = dict(zip(names, host["counts"]))
    assert (seq["one"] == 0).all() and (seq["standing64"][:, :, 1:] == 0).all() and (seq["standing64"][:3, 0, 0] > 0).all()      # what the shapes are there for
    if rule == ec.RULES[0] and not with_exclude:
        assert (seq["walk400_back"][:3, 0, 2] >= 100).all() and (seq["walk400_back"][:3, 0, 0] == 396).all()
    if rule == ec.RULES[2]:
        assert (seq["nineteen"][:, 3:] == 0).all()              # m = 4: N - m <= 0 from scale 4 on


def test_per_frame_is_gait_regularity_s(model, pkg):
    joints, trans, lengths, _, ex, _ = ec.noisy_call(25)
    for sigma in (0.0, 2.0):
        a = model.gait_entropy(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        b = model.gait_regularity(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        assert ec.same_bits(a, b)


@pytest.mark.parametrize("n_seq", (1, 7))
def test_smoothed_signals_within_the_gaussian_bar_and_the_rest_from_them(model, pkg, n_seq):
    joints, trans, lengths, names, ex, table = ec.noisy_call(25)
    if n_seq == 1:
        joints, trans, lengths, ex = joints[:130], trans[:130], lengths[:1], ex[:130]
    raw = pkg.pipeline.gait_regularity(joints, lengths, trans)["per_frame"]
    host = pkg.pipeline.gait_regularity(joints, lengths, trans, ex, sigma=2.0)
    out = numpy_out(model.gait_entropy(joints, lengths, trans, ex, sigma=2.0, **ec.RULE))
    assert np.array_equal(np.isnan(out["per_frame"]), np.isnan(host["per_frame"]))
    worst, a = 0.0, 0
    for T in lengths:
        b = gc.signal_bars(raw[a:a + T], 2.0)
        for k in range(4):
            fin = np.isfinite(host["per_frame"][a:a + T, k])
            if fin.any() and b[k] > 0:
                worst = max(worst, float(np.abs(out["per_frame"][a:a + T, k] - host["per_frame"][a:a + T, k])[fin].max()) / b[k])
            else:
                assert ec.same_bits(out["per_frame"][a:a + T, k], host["per_frame"][a:a + T, k])
        a += T
    print(f"sigma 2, {n_seq} sequence(s): worst signal error / bar = {worst:.3g}")
    assert worst <= 1.0
    again = pkg.pipeline.gait_sampen(out["per_frame"], lengths, ex, **ec.RULE)
    assert ec.same_counts(out["counts"], again["counts"]) and ec.same_bits(out["per_sequence"], again["per_sequence"])


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_one_sequence_alone_and_among_six_others(model, pkg, sigma):
    joints, trans, lengths, names, ex, _ = ec.noisy_call(25)
    whole = numpy_out(model.gait_entropy(joints, lengths, trans, ex, sigma=sigma, **ec.RULE))
    again = numpy_out(model.gait_entropy(joints, lengths, trans, ex, sigma=sigma, **ec.RULE))
    assert same(whole, again)
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_entropy(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], sigma=sigma, **ec.RULE))
        assert ec.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and ec.same_counts(alone["counts"][0], whole["counts"][q]), names[q]
        assert ec.same_bits(alone["per_sequence"][0], whole["per_sequence"][q]), names[q]
        a += n


def test_a_sequence_longer_than_the_lds_array(model, pkg):
    """4100 frames > 4096: at scale 1 the coarse-grained signal lies in the call's scratch and goes through the same code, at scales 2 and 3 in LDS;
    beside it a short one, first and last."""
    T = 4100
    rng = np.random.default_rng(41)
    long_j, long_t = rc.walker(T, 27.3, 0.3, 1.3, 4.7)
    short_j, short_t = rc.walker(65, 19.3, 0.0, 0.2, 2.2)
    long_j = (long_j + ec.NOISE * rng.standard_normal(long_j.shape)).astype(np.float32)
    short_j = (short_j + ec.NOISE * rng.standard_normal(short_j.shape)).astype(np.float32)
    joints, trans, lengths = np.concatenate([short_j, long_j, short_j]), np.concatenate([short_t, long_t, short_t]), [65, T, 65]
    ex = np.zeros(sum(lengths), np.int32)
    ex[65 + 2000:65 + 2040] = 1
    ex[65 + 4095] = 1
    out = numpy_out(model.gait_entropy(joints, lengths, trans, ex, **ec.RULE))
    host = pkg.pipeline.gait_entropy(joints, lengths, trans, ex, **ec.RULE)
    assert same(out, host) and host["per_sequence"][1, 0, 0] == T - 2 - 42 - 3 and (host["counts"][1, :, :, 2] >= 100).all()
    assert ec.same_counts(out["counts"][0], out["counts"][2]) and ec.same_bits(out["per_sequence"][0], out["per_sequence"][2])


def test_as_many_templates_as_lanes_through_the_hook(model, pkg):
    """255 .. 514 frames with m = 1 and derivative 0: 254 .. 257 and 510 .. 513 templates at scale 1 and 254 .. 256 at scale 2, around the 256 lanes of
    the workgroup and twice as many; then with runs of validity that begin and end at the frames 63, 64 and 65."""
    rng = np.random.default_rng(256)
    lengths = [255, 256, 257, 258, 511, 512, 513, 514]
    x = rng.standard_normal((sum(lengths), 4))
    ex = np.zeros(sum(lengths), np.int32)
    host = pkg.pipeline.gait_sampen(x, lengths, ex, **rule_of(1, 0, 2))
    assert host["counts"][:, 0, :, 0].tolist() == [[254, 126], [255, 127], [256, 127], [257, 128], [510, 254], [511, 255], [512, 255], [513, 256]]
    assert same(numpy_out(model.op_gait_sampen(x, lengths, ex, **rule_of(1, 0, 2)), hook=True), host)
    a = 0
    for k, T in enumerate(lengths):
        x[a + (63, 64, 65)[k % 3], :] = np.nan
        ex[a + (65, 63, 64)[k % 3] + 64] = 1
        a += T
    for rule in (rule_of(1, 0, 2), rule_of(2, 2, 3), rule_of(4, 1, 2, 0.5)):
        assert same(numpy_out(model.op_gait_sampen(x, lengths, ex, **rule), hook=True), pkg.pipeline.gait_sampen(x, lengths, ex, **rule)), rule


def test_runs_at_the_word_boundary_through_the_hook(model, pkg):
    rng = np.random.default_rng(15)
    cases = ((130, (63,), ()), (130, (64,), ()), (130, (65,), (0,)), (131, (0, 1), (63, 64, 65)), (130, (62, 63), (65, 66, 129)), (66, (), (64,)), (130, range(64, 128), ()),
             (130, (), range(0, 64)), (66, range(0, 63), (65,)))
    lengths = [T for T, _, _ in cases]
    x = rng.standard_normal((sum(lengths), 4))
    ex = np.zeros(sum(lengths), np.int32)
    a = 0
    for T, nans, excluded in cases:
        x[[a + k for k in nans], :] = np.nan
        ex[[a + k for k in excluded]] = 3
        a += T
    for rule in (rule_of(1, 0, 2, 0.5), rule_of(2, 2, 3, 0.5)):
        host = pkg.pipeline.gait_sampen(x, lengths, ex, **rule)
        assert same(numpy_out(model.op_gait_sampen(x, lengths, ex, **rule), hook=True), host)
    assert host["per_sequence"][:, 0, 0].tolist() == [125, 125, 124, 122, 120, 62, 62, 64, 0]


def test_hook_on_the_hand_made_signal(model, pkg):
    x = ec.hand_signals()
    for rule, n, sd, want in ec.HAND_CASES:
        out = numpy_out(model.op_gait_sampen(x, **rule), hook=True)
        assert (out["counts"][0] == np.array(want)).all() and (out["per_sequence"][0, :, 0] == n).all() and (out["per_sequence"][0, :, 2] == sd).all()
        three = numpy_out(model.op_gait_sampen(np.concatenate([x, x[:9], x]), lengths=[31, 9, 31], **rule), hook=True)
        assert same(three, pkg.pipeline.gait_sampen(np.concatenate([x, x[:9], x]), lengths=[31, 9, 31], **rule))
        assert ec.same_counts(three["counts"][0], out["counts"][0]) and ec.same_counts(three["counts"][2], out["counts"][0])


def test_standing_body_counts_nothing(model, pkg):
    joints, trans = rc.walker(64, still=True)
    out = numpy_out(model.gait_entropy(joints, trans=trans, **rule_of(2, 0, 2)))
    assert (out["per_sequence"][0, :, 0] == 64).all() and (out["per_sequence"][0, :, 2:] == 0).all()
    assert out["counts"][0, :, :, 0].tolist() == [[62, 30]] * 4 and (out["counts"][0, :, :, 1:] == 0).all()


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    signals = torch.zeros(8, 4, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((2, 4, 3, 3), -7, dtype=torch.int64, device="cuda")
    per_seq = torch.full((2, 4, 4), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, sigma=1.0, m=2, fraction=0.2, derivative=2, scales=3, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, None, None, sigma, m, fraction, derivative, scales,
                per_frame.data_ptr(), counts.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_entropy(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, m=2, fraction=0.2, derivative=2, scales=3, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, signals.data_ptr(), None, off, len(offsets) - 1 if n_seq is None else n_seq, m, fraction, derivative, scales, counts.data_ptr(), per_seq.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_sampen(*args)

    rule = ((dict(m=0), b"m outside"), (dict(m=5), b"m outside"), (dict(fraction=0.0), b"fraction"), (dict(fraction=-1.0), b"fraction"), (dict(fraction=10.5), b"fraction"),
            (dict(fraction=nan), b"fraction"), (dict(fraction=inf), b"fraction"), (dict(derivative=-1), b"derivative"), (dict(derivative=3), b"derivative"),
            (dict(scales=0), b"scales"), (dict(scales=9), b"scales"), (dict(n_seq=0), b"n_seq 0"), (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"),
            (dict(offsets=(0, 4, 4)), b"empty"), (dict(offsets=(0, 3, 3 + 32769)), b"sequence 1 has 32769 frames, more than 32768"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 13, 14, 15)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"), (dict(sigma=-1.0), b"sigma"),
            (dict(sigma=nan), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(n_seq=-2), b"n_seq -2")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 9, 10)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((counts == -7).all()) and bool((per_seq == -7.0).all())      # nothing was written
    assert run() == 0                                           # every joint at (1, 1, 1): no axes, and no trans
    torch.cuda.synchronize()
    assert bool(per_frame.isnan().all()) and bool((counts == 0).all()) and bool((per_seq[:, :, 0] == 0).all()) and bool(per_seq[:, :, 1:].isnan().all())
    assert hook(derivative=0) == 0                              # constant signals: r = 0
    torch.cuda.synchronize()
    assert per_seq[:, :, 0].tolist() == [[3.0] * 4, [5.0] * 4] and bool((per_seq[:, :, 1:] == 0).all())
    assert counts[:, 0, :, 0].tolist() == [[1, 0, 0], [3, 0, 0]] and bool((counts[:, :, :, 1:] == 0).all())
    ok = np.ones((4, 25, 3), np.float32)
    for args, kw, word in (((ok[0],), {}, "joints3d"), ((ok,), {"lengths": [2, 1]}, "lengths"), ((ok,), {"joints": (0, 1, 2)}, "joints"), ((ok,), {"trans": np.zeros((3, 3))}, "trans"),
                           ((ok,), {"exclude": np.zeros(3)}, "exclude"), ((ok,), {"scales": 2.5}, "scales"), ((ok,), {"scales": 9}, "scales")):
        with pytest.raises(ValueError, match=word):
            model.gait_entropy(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"m": 0}, "m outside"), ({"fraction": 0.0}, "fraction"), ({"derivative": 3}, "derivative")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_entropy(ok, **kw)


def test_the_longest_sequence_through_the_hook(model, pkg):
    """32 768 frames, the most a call takes, at 8 scales: every scale up to 7 builds its coarse-grained signal in the call's scratch, at the largest
    offsets the call reaches.  The signal is constant but for a NaN, so r = 0 and both sides only count the valid templates; a short noisy sequence
    lies behind it and must not be touched."""
    T = 32768
    rng = np.random.default_rng(32768)
    x = np.concatenate([np.full((T, 4), 0.5), rng.standard_normal((70, 4))])
    x[T - 9, :] = np.nan
    rule = rule_of(2, 1, 8, 0.5)
    host = pkg.pipeline.gait_sampen(x, [T, 70], **rule)
    assert host["counts"][0, 0, :, 0].tolist() == [T - 7, 16378, 10917, 8187, 6549, 5457, 4677, 4092] and (host["counts"][0, :, :, 1:] == 0).all() and (host["counts"][1, :, 0, 2] > 0).all()
    assert same(numpy_out(model.op_gait_sampen(x, [T, 70], **rule), hook=True), host)
