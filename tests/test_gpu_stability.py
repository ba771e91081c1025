"""Local dynamic stability of the gait signals on the GPU (grnet_gait_stability, csrc/gait_stability_kernels.hip) against the host
statement pipeline.gait_stability on the noisy walker of tests/helpers/entropy_checks.py, at the smallest shapes that can break a stage: sequences of
1, 19, 20, 64, 65, 130 and 400 frames, one and seven sequences a call, a standing body, J = 25 and 49 (with another table), derivative 0, 1 and 2, dim
2, 5 and 8, lag 1, 2 and 16, theiler 0, 20 and larger than every E, horizon 1, 20 and 63, with and without trans and exclude; through the hook 255 ..
258 and 511 .. 514 eligible points (around one and two blocks of reference points), sequences and eligible points of the search tile - 1, the tile and
the tile + 1, a sequence longer than the curve kernel's LDS arrays between two short ones, runs of validity that begin and end at the frames 63, 64
and 65, the hand-made signals, the longest sequence a call takes, and the logistic map against ln 2.

nn and pairs are integers and mant is carried in a fixed order: device and statement must agree in every integer and bit, and, with sigma = 0, in
every bit of per_frame.  With sigma > 0 the device's Gaussian has its own order of the sum: per_frame is held to the Gaussian's bar
(gait_checks.signal_bars), and the rest must equal what pipeline.gait_divergence makes of the DEVICE'S OWN per_frame."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from .helpers import gait_checks as gc
from .helpers import regularity_checks as rc
from .helpers import stability_checks as sc

pytestmark = pytest.mark.gpu
TILE = 1024                                                     # csrc/gait_stability.h's kStabTile
KINDS = {"nn": torch.int32, "pairs": torch.int64, "mant": torch.float64, "per_frame": torch.float64}


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out, hook=False):
    assert sorted(out) == ["mant", "nn", "pairs"] + ([] if hook else ["per_frame"])
    assert all(v.is_cuda and v.dtype == KINDS[k] for k, v in out.items())
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def statement(pkg_name, J, rule, with_trans, with_exclude):
    """The statement with sigma = 0 of the seven sequences, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    joints, trans, lengths, _, ex, table = sc.noisy_call(J)
    return pipe.gait_stability(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **sc.rule_of(*rule))


def same(out, host):
    return (sc.same_ints(out["nn"], host["nn"]) and sc.same_ints(out["pairs"], host["pairs"]) and sc.same_bits(out["mant"], host["mant"])
            and ("per_frame" not in out or sc.same_bits(out["per_frame"], host["per_frame"])))


@pytest.mark.parametrize("with_trans,with_exclude", ((True, False), (False, True), (True, True)))
@pytest.mark.parametrize("J,rule", tuple((25, r) for r in sc.RULES) + ((49, sc.RULES[0]), (49, sc.RULES[2])))
def test_every_integer_and_bit_of_the_statement_without_smoothing(model, pkg, J, rule, with_trans, with_exclude):
    joints, trans, lengths, names, ex, table = sc.noisy_call(J)
    host = statement(pkg.__name__, J, rule, with_trans, with_exclude)
    out = numpy_out(model.gait_stability(joints, lengths, trans if with_trans else None, ex if with_exclude else None, joints=table, **sc.rule_of(*rule)))
    K = rule[4]
    assert out["nn"].shape == (sum(lengths), 4) and out["pairs"].shape == (7, 4, K + 1, 2) and out["mant"].shape == (7, 4, K + 1) and out["per_frame"].shape == (sum(lengths), 4)
    assert sc.same_ints(out["nn"], host["nn"]), "nn differs"
    assert sc.same_ints(out["pairs"], host["pairs"]), "pairs differ"
    for k in ("mant", "per_frame"):
        assert sc.same_bits(out[k], host[k]), f"{k} differs in some bit"
    seq = dict(zip(names, host["pairs"]))
    assert (seq["one"] == 0).all() and (seq["standing64"] == 0).all()                                     # what the shapes are there for
    if rule[3] == 500:
        assert (host["nn"] == -1).all() and (host["pairs"] == 0).all() and (host["mant"] == 1.0).all()
    elif rule[1] * rule[2] < 100:
        assert (seq["walk400_back"][:3, 0, 0] >= 100).all()
    if rule == sc.RULES[0] and not with_exclude:
        assert (seq["walk400_back"][:3, :, 0] >= 300).all()


def test_per_frame_is_gait_regularity_s(model, pkg):
    joints, trans, lengths, _, ex, _ = sc.noisy_call(25)
    for sigma in (0.0, 2.0):
        a = model.gait_stability(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        b = model.gait_regularity(joints, lengths, trans, ex, sigma=sigma)["per_frame"].cpu().numpy()
        assert sc.same_bits(a, b)


@pytest.mark.parametrize("n_seq", (1, 7))
def test_smoothed_signals_within_the_gaussian_bar_and_the_rest_from_them(model, pkg, n_seq):
    joints, trans, lengths, names, ex, table = sc.noisy_call(25)
    if n_seq == 1:
        joints, trans, lengths, ex = joints[:130], trans[:130], lengths[:1], ex[:130]
    raw = pkg.pipeline.gait_regularity(joints, lengths, trans)["per_frame"]
    host = pkg.pipeline.gait_regularity(joints, lengths, trans, ex, sigma=2.0)
    out = numpy_out(model.gait_stability(joints, lengths, trans, ex, sigma=2.0, **sc.RULE))
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
    again = pkg.pipeline.gait_divergence(out["per_frame"], lengths, ex, **sc.RULE)
    assert sc.same_ints(out["nn"], again["nn"]) and sc.same_ints(out["pairs"], again["pairs"]) and sc.same_bits(out["mant"], again["mant"])


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_one_sequence_alone_and_among_six_others(model, pkg, sigma):
    joints, trans, lengths, names, ex, _ = sc.noisy_call(25)
    whole = numpy_out(model.gait_stability(joints, lengths, trans, ex, sigma=sigma, **sc.RULE))
    again = numpy_out(model.gait_stability(joints, lengths, trans, ex, sigma=sigma, **sc.RULE))
    assert same(whole, again)
    a = 0
    for q, n in enumerate(lengths):
        alone = numpy_out(model.gait_stability(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], sigma=sigma, **sc.RULE))
        assert sc.same_bits(alone["per_frame"], whole["per_frame"][a:a + n]) and sc.same_ints(alone["nn"], whole["nn"][a:a + n]), names[q]
        assert sc.same_ints(alone["pairs"][0], whole["pairs"][q]) and sc.same_bits(alone["mant"][0], whole["mant"][q]), names[q]
        a += n


def hook_equals_the_statement(model, pkg, x, lengths, ex, rule):
    host = pkg.pipeline.gait_divergence(x, lengths, ex, **rule)
    out = numpy_out(model.op_gait_divergence(x, lengths, ex, **rule), hook=True)
    assert sc.same_ints(out["nn"], host["nn"]), ("nn", rule)
    assert sc.same_ints(out["pairs"], host["pairs"]) and sc.same_bits(out["mant"], host["mant"]), ("the curve", rule)
    return host


def test_a_sequence_longer_than_the_lds_arrays(model, pkg):
    """4100 frames > 4096: the curve kernel keeps y in the call's scratch and reads nn from the output, through the same code; beside it a short
    sequence, first and last; five search tiles, the last of 4 points."""
    T = 4100
    rng = np.random.default_rng(41)
    short = rng.standard_normal((65, 4))
    x = np.concatenate([short, rng.standard_normal((T, 4)), short])
    lengths = [65, T, 65]
    ex = np.zeros(sum(lengths), np.int32)
    ex[65 + 2000:65 + 2040] = 1
    ex[65 + 4095] = 1
    x[65 + 1023, :] = np.nan
    host = hook_equals_the_statement(model, pkg, x, lengths, ex, sc.RULE)
    assert (host["pairs"][1, :, :, 0] >= 3900).all() and sc.same_ints(host["pairs"][0], host["pairs"][2]) and (host["nn"][65:65 + T] >= 4096 - 28).any()


def test_blocks_of_reference_points_through_the_hook(model, pkg):
    """E = 255 .. 258 and 511 .. 514 at the default rule (E = T - 28): one reference point fewer than, as many as and more than the lanes of one and
    of two workgroups; then with runs of validity that begin and end at the frames 63, 64 and 65."""
    rng = np.random.default_rng(256)
    lengths = [28 + E for E in (255, 256, 257, 258, 511, 512, 513, 514)]
    x = rng.standard_normal((sum(lengths), 4))
    ex = np.zeros(sum(lengths), np.int32)
    host = hook_equals_the_statement(model, pkg, x, lengths, ex, sc.RULE)
    assert host["pairs"][:, 0, 0, 0].tolist() == [255, 256, 257, 258, 511, 512, 513, 514]
    a = 0
    for k, T in enumerate(lengths):
        x[a + (63, 64, 65)[k % 3], :] = np.nan
        ex[a + (65, 63, 64)[k % 3] + 64] = 1
        a += T
    for values in ((1, 5, 2, 20, 20), (0, 2, 1, 0, 1), (2, 8, 16, 20, 63)):
        hook_equals_the_statement(model, pkg, x, lengths, ex, sc.rule_of(*values))


def test_the_search_tile_through_the_hook(model, pkg):
    """Sequences of the search tile - 1, the tile and the tile + 1 frames, and as many eligible points (dim 2, lag 1, horizon 1: E = T - 2)."""
    rng = np.random.default_rng(TILE)
    lengths = [TILE - 1, TILE, TILE + 1, TILE + 2, TILE + 3]
    x = rng.standard_normal((sum(lengths), 4))
    host = hook_equals_the_statement(model, pkg, x, lengths, None, sc.rule_of(0, 2, 1, 0, 1))
    assert host["pairs"][:, 0, 0, 0].tolist() == [T - 2 for T in lengths]
    hook_equals_the_statement(model, pkg, x, lengths, None, sc.rule_of(1, 8, 16, 20, 20))
    # the only close neighbour of a point of the first tile lies in the second, and the other way round
    x = rng.standard_normal((TILE + 200, 4))
    x[TILE + 50:TILE + 60] = x[100:110] + 1e-6
    host = hook_equals_the_statement(model, pkg, x, None, None, sc.RULE)
    assert host["nn"][100, 0] == TILE + 50 and host["nn"][TILE + 50, 0] == 100


def test_runs_at_the_word_boundary_through_the_hook(model, pkg):
    x, lengths, ex = sc.boundary_call()
    for values in ((1, 5, 2, 20, 20), (0, 2, 1, 0, 1), (2, 3, 16, 5, 20)):
        hook_equals_the_statement(model, pkg, x, lengths, ex, sc.rule_of(*values))


def test_hook_on_the_hand_made_signals(model, pkg):
    x = sc.hand_signals(sc.HAND_PERIODIC_X)
    out = numpy_out(model.op_gait_divergence(x, **sc.HAND_PERIODIC_RULE), hook=True)
    want = [sc.exact_mantissa(p) for p in sc.HAND_PERIODIC_PRODUCTS]
    for ch in range(4):
        assert out["nn"][:, ch].tolist() == sc.HAND_PERIODIC_NN
        assert out["pairs"][0, ch].tolist() == [[sc.HAND_PERIODIC_N, S] for _, S in want] and out["mant"][0, ch].tolist() == [P for P, _ in want]
    xb = sc.hand_signals(sc.HAND_BROKEN_X)
    out = numpy_out(model.op_gait_divergence(xb, **sc.HAND_BROKEN_RULE), hook=True)
    assert out["nn"][:, 1].tolist() == sc.HAND_BROKEN_NN and out["pairs"][0, 1].tolist() == [list(p) for p in sc.HAND_BROKEN_PAIRS] and out["mant"][0, 1].tolist() == list(sc.HAND_BROKEN_MANT)
    three = np.concatenate([x, xb[:9], x])
    host = hook_equals_the_statement(model, pkg, three, [30, 9, 30], None, sc.HAND_PERIODIC_RULE)
    assert host["nn"][39:, 0].tolist() == sc.HAND_PERIODIC_NN


def test_standing_body_has_no_neighbour(model, pkg):
    joints, trans = rc.walker(64, still=True)
    out = numpy_out(model.gait_stability(joints, trans=trans, **sc.RULE))
    assert np.isfinite(out["per_frame"]).all() and (out["nn"] == -1).all() and (out["pairs"] == 0).all() and (out["mant"] == 1.0).all()


def test_logistic_map_against_ln_2(model, pkg):
    x = np.stack([sc.logistic(seed) for seed in sc.LOGISTIC_SEEDS[:4]], axis=1)
    out = numpy_out(model.op_gait_divergence(x, **sc.LOGISTIC_RULE), hook=True)
    rows = pkg.pipeline.stability_rows(out["pairs"], out["mant"], **sc.LOGISTIC_FIT)
    bar = 2.0 * sc.LOGISTIC_MEASURED
    miss = np.abs(rows["lambda"][0] - math.log(2.0))
    print(f"lambda {rows['lambda'][0].tolist()}, ln 2 {math.log(2.0):.5f}, worst miss {miss.max():.4f} (bar {bar:.4f})")
    assert (miss <= bar).all() and (out["pairs"][0, :, :5, 0] >= 900).all()


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    signals = torch.zeros(8, 4, dtype=torch.float64, device="cuda")
    per_frame = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    nn = torch.full((8, 4), -7, dtype=torch.int32, device="cuda")
    pairs = torch.full((2, 4, 3, 2), -7, dtype=torch.int64, device="cuda")
    mant = torch.full((2, 4, 3), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = float("nan")

    def run(J=25, offsets=(0, 3, 8), n_seq=None, table=gc.KINECTV2, sigma=1.0, derivative=1, dim=2, lag=1, theiler=0, horizon=2, null=None):
        off, tab = (C.c_int32 * len(offsets))(*offsets), (C.c_int32 * 8)(*table)
        args = [h, joints.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq, tab, None, None, sigma, derivative, dim, lag, theiler, horizon,
                per_frame.data_ptr(), nn.data_ptr(), pairs.data_ptr(), mant.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_stability(*args)

    def hook(offsets=(0, 3, 8), n_seq=None, derivative=1, dim=2, lag=1, theiler=0, horizon=2, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, signals.data_ptr(), None, off, len(offsets) - 1 if n_seq is None else n_seq, derivative, dim, lag, theiler, horizon, nn.data_ptr(), pairs.data_ptr(),
                mant.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_op_gait_divergence(*args)

    rule = ((dict(derivative=-1), b"derivative outside [0, 2]"), (dict(derivative=3), b"derivative outside [0, 2]"), (dict(dim=1), b"dim outside [2, 8]"), (dict(dim=9), b"dim outside [2, 8]"),
            (dict(lag=0), b"lag outside [1, 16]"), (dict(lag=17), b"lag outside [1, 16]"), (dict(theiler=-1), b"theiler outside [0, 4096]"),
            (dict(theiler=4097), b"theiler outside [0, 4096]"), (dict(horizon=0), b"horizon outside [1, 63]"), (dict(horizon=64), b"horizon outside [1, 63]"),
            (dict(n_seq=0), b"n_seq 0"), (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"),
            (dict(offsets=(0, 3, 3 + 32769)), b"sequence 1 has 32769 frames, more than 32768"))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 5, 14, 15, 16, 17)) + rule + (
            (dict(J=0), b"J 0"), (dict(J=19), b"joint index 20"), (dict(table=(0, 20, 12, 16, 14, 18, -1, 19)), b"joint index -1"), (dict(sigma=-1.0), b"sigma"),
            (dict(sigma=nan), b"sigma"), (dict(sigma=16.5), b"sigma"), (dict(n_seq=-2), b"n_seq -2")):
        assert run(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 3, 10, 11, 12)) + rule:
        assert hook(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((per_frame == -7.0).all()) and bool((nn == -7).all()) and bool((pairs == -7).all()) and bool((mant == -7.0).all())      # nothing was written
    assert run() == 0                                           # every joint at (1, 1, 1): no axes, and no trans
    torch.cuda.synchronize()
    assert bool(per_frame.isnan().all()) and bool((nn == -1).all()) and bool((pairs == 0).all()) and bool((mant == 1.0).all())
    nn.fill_(-7)
    assert hook(derivative=0) == 0                              # constant signals: every D2 is 0
    torch.cuda.synchronize()
    assert bool((nn == -1).all()) and bool((pairs == 0).all()) and bool((mant == 1.0).all())
    ok = np.ones((4, 25, 3), np.float32)
    for args, kw, word in (((ok[0],), {}, "joints3d"), ((ok,), {"lengths": [2, 1]}, "lengths"), ((ok,), {"joints": (0, 1, 2)}, "joints"), ((ok,), {"trans": np.zeros((3, 3))}, "trans"),
                           ((ok,), {"exclude": np.zeros(3)}, "exclude"), ((ok,), {"horizon": 2.5}, "horizon"), ((ok,), {"horizon": 64}, "horizon")):
        with pytest.raises(ValueError, match=word):
            model.gait_stability(*args, **kw)
    for kw, word in (({"sigma": 20.0}, "sigma"), ({"dim": 1}, "dim outside"), ({"lag": 17}, "lag outside"), ({"theiler": -1}, "theiler outside"), ({"derivative": 3}, "derivative")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.gait_stability(ok, **kw)


def test_the_longest_sequence_through_the_hook(model, pkg):
    """32 768 frames, the most a call takes, at dim 8, lag 16 and horizon 63: the largest offsets the call reaches, 128 blocks of reference points and
    32 search tiles.  The signal is constant, so every D2 is 0: every nn is -1 and every n is 0.  A short noisy sequence lies behind it, whose
    workgroups past its frames return at once, and must equal the statement of it alone."""
    T = 32768
    rng = np.random.default_rng(32768)
    short = rng.standard_normal((300, 4))
    x = np.concatenate([np.full((T, 4), 0.5), short])
    rule = sc.rule_of(1, 8, 16, 20, 63)
    out = numpy_out(model.op_gait_divergence(x, [T, 300], **rule), hook=True)
    assert (out["nn"][:T] == -1).all() and (out["pairs"][0] == 0).all() and (out["mant"][0] == 1.0).all()
    host = pkg.pipeline.gait_divergence(short, **rule)
    assert sc.same_ints(out["nn"][T:], host["nn"]) and sc.same_ints(out["pairs"][1], host["pairs"][0]) and sc.same_bits(out["mant"][1], host["mant"][0])
    assert (host["pairs"][0, :, :, 0] > 50).all()
