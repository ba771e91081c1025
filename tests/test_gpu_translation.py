"""The camera-space trajectory on the GPU (grnet_fit_translation, csrc/translation_kernels.hip) against the exact checker
tests/helpers/translation_checks.py and the host statement pipeline.fit_translation, at the smallest shapes that can break each stage.

The bars are derived in DESIGN 4.9 and stated in the checker, not measured: a fitted translation within cond_2(A) 2^-52 of the exact solution
(relative, infinity norm), every fitted frame with cond_2(A) <= 1e6 and none left out; the reprojection error at 1e-10 relative plus
(P + 8) 2^-53; filled rows equal to numpy.linspace on the device's own fitted rows bit for bit; device and host within two bars of each other.
The fit kernel runs one lane per frame in tiles of 64, the sequence kernel 256 threads with ceil(T / 256) consecutive frames each, so the sizes
sit around 64 and beyond 256.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from .helpers import translation_checks as tc

pytestmark = pytest.mark.gpu

HD = (1920, 1080)
CAM = (float(np.hypot(*HD)), 960.0, 540.0)


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out):
    assert sorted(out) == ["per_frame", "per_sequence"]
    for k, v in out.items():
        assert v.dtype == torch.float64 and v.is_cuda, k
    return {k: v.cpu().numpy() for k, v in out.items()}


def run(model, pkg, j3, j2, pairs, **kw):
    out = numpy_out(model.fit_translation(j3, j2, pairs, **kw))
    host = pkg.pipeline.fit_translation(j3, j2, pairs, **kw)
    fails, worst = tc.compare(out, j3, j2, pairs, other=host, **kw)
    print(f"errors in units of their bars: { {k: float(f'{v:.3g}') for k, v in worst.items()} }")
    assert worst["cond"] <= tc.MAX_COND
    assert not fails, fails
    return out


def case(P, lengths, cams=None, K3=None, K2=None, seed=1, depth=(2.0, 8.0)):
    cams = cams or [CAM] * len(lengths)
    return tc.make_case((P, K3 or max(P + 3, 25), K2 or max(P + 1, 25), sum(lengths), lengths, cams, HD, depth), seed)


def unfit(j2, frames):
    j2 = j2.copy()
    j2[list(frames), :, 2] = 0.0
    return j2


@pytest.mark.parametrize("P", (2, 3, 4, 13, 25, 63, 64))
def test_pair_counts(model, pkg, P):
    """2 pairs: four equations for three unknowns, min_joints at its floor; 64: the whole table."""
    j3, j2, pairs, kw = case(P, [6], seed=11)
    if P < 13:
        j2[:, pairs[:, 1], 2] = np.float32(0.3) + np.float32(0.1) * np.arange(P, dtype=np.float32)      # every pair of a small table lives
    out = run(model, pkg, j3, j2, pairs, min_joints=min(P, 4), **kw)
    assert (out["per_frame"][:, 5] == 0).all()


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257))
def test_call_sizes(model, pkg, n):
    j3, j2, pairs, kw = case(13, [n], seed=12)
    out = run(model, pkg, j3, j2, pairs, **kw)
    assert (out["per_frame"][:, 5] == 0).sum() >= n - 2


@pytest.mark.parametrize("lengths", ([1], [2], [1, 1, 3], [5, 64, 1, 130]), ids=str)
def test_sequences_with_their_own_intrinsics(model, pkg, lengths):
    cams = [(1000.0 + 300.0 * q, 960.0 - 40.0 * q, 540.0 + 25.0 * q) for q in range(len(lengths))]
    j3, j2, pairs, kw = case(13, lengths, cams=cams, seed=13)
    j2 = unfit(j2, [sum(lengths) - 1])                         # the last frame of the last sequence: filled from its neighbour, if it has one
    out = run(model, pkg, j3, j2, pairs, **kw)
    assert out["per_frame"][-1, 5] == (3 if lengths[-1] > 1 else 1)


def test_unfitted_runs_are_filled(model, pkg):
    """Runs at the front and the end, inner runs of 1, 2 and 70 frames, in a sequence of 90 frames (one frame a thread) and of 600 (three a thread:
    the long run crosses 23 threads' blocks and four waves); a wholly unfitted sequence between two good ones keeps its rows."""
    dead = [0, 1, 5, 9, 10] + list(range(14, 84)) + [88, 89]
    for T in (90, 600):
        j3, j2, pairs, kw = case(13, [T], seed=14)
        j2 = unfit(j2, dead + ([T - 1] if T > 90 else []))
        out = run(model, pkg, j3, j2, pairs, **kw)
        rows = out["per_frame"]
        assert (rows[dead, 5] == 3).all() and np.isnan(rows[dead, 3]).all()
        assert np.array_equal(rows[14:84, :3], np.linspace(rows[13, :3], rows[84, :3], 72)[1:-1])
        assert np.array_equal(rows[0, :3], rows[2, :3]) and np.array_equal(rows[T - 1, :3], rows[T - 2 if T > 90 else 87, :3])
        plain = run(model, pkg, j3, j2, pairs, fill=False, **kw)
        assert (plain["per_frame"][dead, 5] == 1).all() and np.isnan(plain["per_frame"][dead, :4]).all() and plain["per_sequence"][0, 1] == 0
    j3, j2, pairs, kw = case(13, [30, 300, 30], seed=15)
    j2 = unfit(j2, list(range(30, 330)) + [3, 340])
    out = run(model, pkg, j3, j2, pairs, **kw)
    assert (out["per_frame"][30:330, 5] == 1).all() and np.isnan(out["per_frame"][30:330, :4]).all()
    assert out["per_sequence"][1, :2].tolist() == [0, 0] and np.isnan(out["per_sequence"][1, 2]) and out["per_sequence"][1, 3] == 0
    assert out["per_frame"][[3, 340], 5].tolist() == [3, 3]


def test_min_joints_and_threshold_at_their_edges(model, pkg):
    j3, j2, pairs, kw = case(13, [8], cams=[(1000.0, 960.0, 540.0)], seed=16)
    j2[:, pairs[:, 1], 2] = 0.5
    thr = float(np.float32(0.25))
    j2[0, pairs[4:, 1], 2] = 0.0                                # exactly min_joints = 4 used pairs: fitted
    j2[1, pairs[3:, 1], 2] = 0.0                                # three: too few
    j2[2, pairs[:4, 1], 2] = thr                                # a confidence EQUAL to the threshold is not used ...
    j2[3, pairs[:4, 1], 2] = np.nextafter(np.float32(thr), np.float32(1))   # ... the next float32 above it is
    j2[4, pairs[0, 1], 2] = np.inf                              # a non-finite confidence drops the pair
    j2[4, pairs[1, 1], 2] = np.nan
    j3[5, pairs[:, 0], :2] *= -1.0                              # the mirror image through the centre: a body behind the camera, Z + tz < 0
    j2[6, pairs[:, 1], :2] = (960.0, 540.0)                     # every detection at the centre: the third pivot is exactly zero
    j3[7, pairs[2, 0], 1] = np.nan                              # a NaN coordinate of a used joint: a non-finite result
    kw = dict(kw, conf_threshold=thr, fill=False)
    rows = run(model, pkg, j3, j2, pairs, **kw)["per_frame"]
    assert rows[:, 5].tolist() == [0, 1, 0, 0, 0, 2, 2, 2]
    assert rows[:, 4].tolist() == [4, 3, 9, 13, 11, 13, 13, 13]
    assert np.isnan(rows[[1, 5, 6, 7], :4]).all() and np.isfinite(rows[[0, 2, 3, 4], :4]).all()
    assert run(model, pkg, j3, j2, pairs, **dict(kw, min_joints=5))["per_frame"][0, 5] == 1


def bits(t):
    return t.contiguous().view(torch.int64)


def test_one_call_and_three_calls_give_the_same_bytes(model):
    lengths = [70, 1, 130]
    j3, j2, pairs, kw = case(25, lengths, cams=[(1000.0, 960.0, 540.0), (1500.0, 900.0, 500.0), (2200.0, 1000.0, 560.0)], seed=17)
    j2 = unfit(j2, [4, 100])
    whole = model.fit_translation(j3, j2, pairs, fill=False, **kw)
    again = model.fit_translation(j3, j2, pairs, fill=False, **kw)
    assert torch.equal(bits(whole["per_frame"]), bits(again["per_frame"])) and torch.equal(bits(whole["per_sequence"]), bits(again["per_sequence"]))
    filled = model.fit_translation(j3, j2, pairs, **kw)
    a = 0
    for q, T in enumerate(lengths):
        one_kw = dict(focal_length=kw["focal_length"][q], centre=kw["centre"][q])
        one = model.fit_translation(j3[a:a + T], j2[a:a + T], pairs, fill=False, **one_kw)
        assert torch.equal(bits(one["per_frame"]), bits(whole["per_frame"][a:a + T])), q
        assert torch.equal(bits(one["per_sequence"][0]), bits(whole["per_sequence"][q])), q
        one = model.fit_translation(j3[a:a + T], j2[a:a + T], pairs, **one_kw)
        assert torch.equal(bits(one["per_frame"]), bits(filled["per_frame"][a:a + T])), q
        assert torch.equal(bits(one["per_sequence"][0]), bits(filled["per_sequence"][q])), q
        a += T
    # a frame's fit does not depend on where the call is cut: the same frames as sequences of other lengths, and one frame alone
    cut = model.fit_translation(j3[:70], j2[:70], pairs, lengths=[3, 64, 3], fill=False, focal_length=1000.0, centre=(960.0, 540.0))
    assert torch.equal(bits(cut["per_frame"]), bits(whole["per_frame"][:70]))
    alone = model.fit_translation(j3[66:67], j2[66:67], pairs, focal_length=1000.0, centre=(960.0, 540.0))
    assert torch.equal(bits(alone["per_frame"][0]), bits(whole["per_frame"][66]))


def test_more_sequences_than_one_launch_holds(model, pkg):
    """150 short sequences: three launch batches of 64; each sequence keeps its own intrinsics and its own row of the summary."""
    g = np.random.Generator(np.random.Philox(key=[3, 150]))
    lengths = [int(v) for v in g.integers(1, 4, 150)]
    cams = [(1000.0 + 5.0 * q, 960.0 - q, 540.0 + q) for q in range(150)]
    j3, j2, pairs, kw = case(13, lengths, cams=cams, seed=18)
    out = run(model, pkg, j3, j2, pairs, **kw)
    a = sum(lengths[:140])
    one = numpy_out(model.fit_translation(j3[a:a + lengths[140]], j2[a:a + lengths[140]], pairs, focal_length=cams[140][0], centre=cams[140][1:]))
    assert np.array_equal(one["per_frame"], out["per_frame"][a:a + lengths[140]], equal_nan=True)
    assert np.array_equal(one["per_sequence"][0], out["per_sequence"][140], equal_nan=True)


def test_golden_cases_on_the_device(model, pkg):
    """The reference's own translations (tests/golden/translation.npz): twice the bar, since both sides err."""
    import os
    from .conftest import ROOT
    g = np.load(os.path.join(ROOT, "tests", "golden", "translation.npz"))
    worst = 0.0
    for ci in range(3):
        for K in (13, 25):
            name = f"c{ci}_k{K}"
            j3, j2, (size, f), t_ref = g[name + "_joints3d"], g[name + "_joints2d"], g[name + "_camera"], g[name + "_t"]
            pairs = np.stack([np.arange(K)] * 2, axis=1)
            kw = dict(focal_length=f, centre=(size / 2, size / 2), conf_threshold=0.0)
            out = run(model, pkg, j3, j2, pairs, **kw)
            assert (out["per_frame"][:, 5] == 0).all()
            for i in range(j3.shape[0]):
                cond = tc.frame_truth(tc.widen(j3)[i], tc.widen(j2)[i], f, size / 2, size / 2, 0.0, 4)[3]
                worst = max(worst, np.abs(out["per_frame"][i, :3] - t_ref[i]).max() / np.abs(t_ref[i]).max() / (2 * cond * tc.EPS))
    print(f"worst ratio to the golden bar: {worst:.3g}")
    assert worst <= 1.0


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    j3 = torch.zeros(8, 25, 3, dtype=torch.float32, device="cuda")
    j2 = torch.ones(8, 25, 3, dtype=torch.float32, device="cuda")
    outs = [torch.full(shape, -7.0, dtype=torch.float64, device="cuda") for shape in ((8, 6), (2, 4))]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = [v for pair in pkg.pipeline.BODY25_FROM_KINECTV2 for v in pair]

    def call(K3=25, K2=25, frames=8, offsets=(0, 3, 8), n_seq=None, pairs=table, n_pairs=None, cam=(1000.0, 960.0, 540.0, 1200.0, 900.0, 500.0), thr=0.1,
             min_joints=4, root=0, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        pr = (C.c_int32 * len(pairs))(*pairs)
        cm = (C.c_double * len(cam))(*cam)
        args = [h, j3.data_ptr(), K3, j2.data_ptr(), K2, frames, off, len(offsets) - 1 if n_seq is None else n_seq, pr, len(pairs) // 2 if n_pairs is None else n_pairs,
                cm, thr, min_joints, root, 1, outs[0].data_ptr(), outs[1].data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_fit_translation(*args)

    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(n_pairs=0), b"n_pairs 0"), (dict(pairs=[0, 0] * 65), b"n_pairs 65"), (dict(pairs=[25, 0]), b"pairs[0][0] = 25"),
                     (dict(pairs=[0, 0, 3, 25]), b"pairs[1][1] = 25"), (dict(pairs=[-1, 0]), b"pairs[0][0] = -1"), (dict(K3=18), b"outside [0, K3 = 18)"),
                     (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty"), (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 3, 7)), b"end at 7"),
                     (dict(frames=9), b"end at 8"), (dict(n_seq=0), b"n_seq 0"), (dict(cam=(0.0, 1.0, 1.0, 1.0, 1.0, 1.0)), b"focal length of sequence 0"),
                     (dict(cam=(1.0, 1.0, 1.0, -2.0, 1.0, 1.0)), b"focal length of sequence 1"), (dict(cam=(nan, 1.0, 1.0, 1.0, 1.0, 1.0)), b"focal length"),
                     (dict(cam=(inf, 1.0, 1.0, 1.0, 1.0, 1.0)), b"focal length"), (dict(cam=(1.0, nan, 1.0, 1.0, 1.0, 1.0)), b"centre of sequence 0"),
                     (dict(thr=nan), b"conf_threshold"), (dict(thr=-0.5), b"conf_threshold"), (dict(min_joints=1), b"min_joints 1"), (dict(root=25), b"root 25"),
                     (dict(root=-1), b"root -1"), (dict(K2=0), b"K2 0"), (dict(null=1), b"null"), (dict(null=3), b"null"), (dict(null=6), b"null"), (dict(null=8), b"null"),
                     (dict(null=10), b"null"), (dict(null=15), b"null"), (dict(null=16), b"null")):
        assert call(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)          # nothing was written
    assert call() == 0                                         # the same call without a fault goes through, with every output
    torch.cuda.synchronize()
    assert all(not bool((o == -7.0).any()) for o in outs)
    ok3, ok2 = np.zeros((4, 25, 3), np.float32), np.ones((4, 25, 3), np.float32)
    pairs = pkg.pipeline.BODY25_FROM_KINECTV2
    for args, kw, word in (((ok3[0], ok2, pairs), {}, "joints3d"), ((ok3, ok2[:3], pairs), {}, "frames"), ((ok3, ok2, pairs), {"lengths": [2, 1]}, "lengths"),
                           ((ok3, ok2, [0, 1]), {}, "pairs"), ((ok3, ok2, pairs), {"focal_length": [1.0, 2.0]}, "focal_length")):
        with pytest.raises(ValueError, match=word):
            model.fit_translation(*args, **kw)
    for kw, word in (({"root": 25}, "root"), ({"min_joints": 1}, "min_joints"), ({"focal_length": 0.0}, "focal length"), ({"conf_threshold": -1.0}, "conf_threshold")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.fit_translation(ok3, ok2, pairs, **kw)
    with pytest.raises(pkg._lib.GrnetError, match="pairs"):
        model.fit_translation(ok3, ok2, [(0, 25)])


def test_a_handle_without_weights(pkg):
    m = pkg.GRNet(max_frames=1)
    try:
        j3, j2, pairs, kw = case(13, [4, 5], seed=19)
        run(m, pkg, j3, j2, pairs, **kw)
    finally:
        m.close()
