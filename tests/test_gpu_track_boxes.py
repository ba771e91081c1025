"""The per-frame boxes from 2D joints on the GPU (grnet_track_boxes, csrc/track_kernels.hip) against the golden values the reference's
lib/utils/smooth_bbox.py gave (tests/golden/track_boxes.npz) and the host statement pipeline.track_boxes, at the smallest shapes that can break
each stage: 1 to 70 frames a sequence, a gap over a 64-frame word of the validity bitmask, K = 1, 25 and 64.

The bars are those of the host test, derived in tests/helpers/track_checks.py and not measured: range and status equal, the centres of stages 1
and 2 bit-identical, the scale within 8 u, the median bit-identical, the Gaussian within (2 r + 8) u max|x|.  Where the expected values come from
the numpy statement the device runs the same operations in the same order on the centres and in the selection -- equal bits -- and its own
Gaussian weights (libm's exp, another order of their sum) and summation order, so filtered values are held to twice the Gaussian's bar: both
sides err.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from .helpers import track_checks as tk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


@pytest.fixture(scope="module")
def g():
    return tk.golden()


def numpy_out(out):
    assert sorted(out) == ["boxes", "range", "status"]
    assert out["boxes"].dtype == torch.float64 and out["status"].dtype == torch.int32 and out["range"].dtype == torch.int32
    assert all(v.is_cuda for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def against_statement(out, host, median_cols=None, sigma=0.0):
    """Device against the numpy statement: status and range equal; without a Gaussian every bit equal; with one, twice its bar."""
    assert out["status"].tolist() == host["status"].tolist() and out["range"].tolist() == host["range"].tolist()
    if sigma == 0:
        assert np.array_equal(bits(out["boxes"]), bits(host["boxes"]))
        return 0.0
    worst = 0.0
    ok = host["status"] < 2
    for c in (0, 1):
        worst = max(worst, np.abs(out["boxes"][ok, c] - host["boxes"][ok, c]).max() / (2 * tk.gauss_bar(median_cols[:, c], sigma)))
    rel = 2 * tk.gauss_bar(median_cols[:, 2], sigma) / host["params"][ok, 2] + 2 * tk.U       # a side is 150 / scale: the same relative error, and a quotient each
    worst = max(worst, (np.abs(out["boxes"][ok, 2] - host["boxes"][ok, 2]) / (rel * host["boxes"][ok, 2])).max())
    return float(worst)


@pytest.mark.parametrize("name", tk.CASES)
def test_golden_cases(model, g, name):
    """K = 25.  Stages 1 and 2 alone, then the whole chain with the reference's kernel of 11 and the case's sigma, zero padding."""
    kp = g[name + "_kp"]
    out = numpy_out(model.track_boxes(kp, vis_thresh=tk.VIS_THRESH))
    assert out["range"].tolist() == [g[name + "_range"].tolist()]
    ratio = tk.check_unsmoothed(out, g, name)
    print(f"{name}: worst scale error / (8 u) = {ratio:.3g}")
    assert ratio <= 1.0
    if name == "dead":
        return
    out = numpy_out(model.track_boxes(kp, vis_thresh=tk.VIS_THRESH, kernel_size=tk.KERNEL, sigma=float(g[name + "_sigma"])))
    assert out["range"].tolist() == [g[name + "_range"].tolist()]
    ratio = tk.check_smoothed(out, g, name)
    print(f"{name}: worst smoothed error / the chain's bar = {ratio:.3g}")
    assert ratio <= 1.0
    if name == "t5":                                             # more than half of every window is padding: the reference's own zeros
        assert (out["status"] == 3).all() and (out["boxes"] == 0).all()


def test_median_and_gaussian_alone(model, g):
    """The two hooks on the goldens' own stage inputs, every column of every case in ONE call each."""
    names = [n for n in tk.CASES if n != "dead"]
    lengths = [g[n + "_params"].shape[0] for n in names for _ in range(3)]
    stage2 = np.concatenate([g[n + "_params"][:, c] for n in names for c in range(3)])
    median = np.concatenate([g[n + "_median"][:, c] for n in names for c in range(3)])
    got = model.op_median1d(stage2, lengths=lengths, kernel_size=tk.KERNEL, pad="zero").cpu().numpy()
    assert np.array_equal(bits(got), bits(median))
    for sigma in (3.0, 8.0):
        cases = [n for n in names if float(g[n + "_sigma"]) == sigma]
        lengths = [g[n + "_median"].shape[0] for n in cases for _ in range(3)]
        got = model.op_gauss1d(np.concatenate([g[n + "_median"][:, c] for n in cases for c in range(3)]), lengths=lengths, sigma=sigma).cpu().numpy()
        a = 0
        for n in cases:
            for c in range(3):
                col, want = g[n + "_median"][:, c], g[n + "_smooth"][:, c]
                err, bar = np.abs(got[a:a + col.size] - want).max(), tk.gauss_bar(col, sigma)
                print(f"{n} column {c} sigma {sigma:g}: Gaussian error / ((2 r + 8) u max|x|) = {err / bar if bar else err:.3g}")
                assert err <= bar
                a += col.size


def test_one_call_equals_each_case_alone_and_itself(model, g):
    """All cases in one call, `dead` in the middle: no window, fill or reflection crosses a sequence.  The same call twice: equal bits."""
    order = ("t26gaps", "t5", "t1", "t70", "dead", "t12", "point", "t2")
    kp = np.concatenate([g[n + "_kp"] for n in order])
    lengths = [tk.FRAMES[n] for n in order]
    for kw in (dict(), dict(kernel_size=tk.KERNEL, sigma=8.0), dict(kernel_size=5, sigma=3.0, pad="edge")):
        whole = numpy_out(model.track_boxes(kp, lengths=lengths, vis_thresh=tk.VIS_THRESH, **kw))
        again = numpy_out(model.track_boxes(kp, lengths=lengths, vis_thresh=tk.VIS_THRESH, **kw))
        assert all(np.array_equal(whole[k], again[k]) for k in whole) and np.array_equal(bits(whole["boxes"]), bits(again["boxes"]))
        a = 0
        for q, n in enumerate(order):
            alone = numpy_out(model.track_boxes(g[n + "_kp"], vis_thresh=tk.VIS_THRESH, **kw))
            T = tk.FRAMES[n]
            assert np.array_equal(bits(whole["boxes"][a:a + T]), bits(alone["boxes"])), (n, kw)
            assert np.array_equal(whole["status"][a:a + T], alone["status"]) and whole["range"][q].tolist() == alone["range"][0].tolist()
            a += T
        if not kw:
            a = 0
            for n in order:
                assert tk.check_unsmoothed(whole, g, n, a) <= 1.0
                a += tk.FRAMES[n]


def test_joint_counts_1_and_64(model, pkg, g):
    kp = g["t26gaps_kp"]
    one = numpy_out(model.track_boxes(kp[:, 3:4], vis_thresh=0.0))                              # one joint: every height is 0
    assert one["range"].tolist() == [[-1, 0]] and (one["status"] == 2).all() and (one["boxes"] == 0).all()
    wide = np.concatenate([kp, kp[:, ::-1] + np.array([7.0, -3.0, 0.0]), kp[:, :14] * np.array([1.01, 0.99, 1.0])], axis=1)
    assert wide.shape[1] == 64
    for kw in (dict(), dict(kernel_size=tk.KERNEL, sigma=3.0, pad="edge")):
        host = pkg.pipeline.track_boxes(wide, vis_thresh=tk.VIS_THRESH, return_params=True, **kw)
        out = numpy_out(model.track_boxes(wide, vis_thresh=tk.VIS_THRESH, **kw))
        med = pkg.pipeline.track_boxes(wide, vis_thresh=tk.VIS_THRESH, kernel_size=kw.get("kernel_size", 1), pad=kw.get("pad", "zero"), return_params=True)
        start, end = host["range"][0]
        ratio = against_statement(out, host, med["params"][start:end], kw.get("sigma", 0.0))
        print(f"K = 64 {kw}: worst error / twice the Gaussian's bar = {ratio:.3g}")
        assert ratio <= 1.0 and host["range"].tolist() == [[2, 24]]


@pytest.mark.parametrize("name", ("t12", "t26gaps"))
def test_pad_edge_against_the_statement(model, pkg, g, name):
    kp = g[name + "_kp"]
    kw = dict(vis_thresh=tk.VIS_THRESH, kernel_size=tk.KERNEL, pad="edge")
    host_median = pkg.pipeline.track_boxes(kp, return_params=True, **kw)
    out = numpy_out(model.track_boxes(kp, **kw))
    against_statement(out, host_median)                         # the median alone: every bit
    host = pkg.pipeline.track_boxes(kp, sigma=3.0, return_params=True, **kw)
    out = numpy_out(model.track_boxes(kp, sigma=3.0, **kw))
    start, end = host["range"][0]
    ratio = against_statement(out, host, host_median["params"][start:end], 3.0)
    print(f"{name} pad = edge: worst error / twice the Gaussian's bar = {ratio:.3g}")
    assert ratio <= 1.0
    assert not (out["status"] == 3).any() and (out["boxes"][start:end, 2] > 0).all()


def test_nan_joint_makes_its_frame_interpolated(model, g):
    kp = g["t12_kp"].copy()
    clean = numpy_out(model.track_boxes(kp, vis_thresh=tk.VIS_THRESH))
    j = int(np.flatnonzero(kp[5, :, 2] > tk.VIS_THRESH)[0])
    kp[5, j, 1] = np.nan
    out = numpy_out(model.track_boxes(kp, vis_thresh=tk.VIS_THRESH))
    assert out["status"].tolist() == [0] * 5 + [1] + [0] * 6 and out["range"].tolist() == [[0, 12]] and np.isfinite(out["boxes"]).all()
    rest = np.arange(12) != 5
    assert np.array_equal(bits(out["boxes"][rest]), bits(clean["boxes"][rest]))                # nothing else changes
    for c in (0, 1):
        assert out["boxes"][5, c] == np.linspace(clean["boxes"][4, c], clean["boxes"][6, c], 3)[1]
    kp[5, j] = (np.nan, np.inf, np.nan)                          # a NaN score hides the joint, and what lies beside it is not looked at
    assert numpy_out(model.track_boxes(kp, vis_thresh=tk.VIS_THRESH))["status"][5] == 0


def test_gap_across_a_64_frame_boundary(model, pkg, g):
    """T = 130 with frames 60 to 70 dead, alone and behind a sequence of 5 frames (so the gap sits at other bits of the call's words), and with
    dead frames over a whole word (50 to 129 of 200)."""
    base = np.tile(g["t70_kp"][:1], (200, 1, 1))
    base[:, :, 0] += 3.0 * np.arange(200)[:, None] + np.sin(np.arange(200))[:, None]
    base[:, :, 1] += np.cos(0.3 * np.arange(200))[:, None]
    kp = base[:130].copy()
    kp[60:71, :, 2] = 0.0
    host = pkg.pipeline.track_boxes(kp, vis_thresh=tk.VIS_THRESH)
    assert host["status"].tolist() == [0] * 60 + [1] * 11 + [0] * 59
    against_statement(numpy_out(model.track_boxes(kp, vis_thresh=tk.VIS_THRESH)), host)
    both = numpy_out(model.track_boxes(np.concatenate([g["t5_kp"], kp]), lengths=[5, 130], vis_thresh=tk.VIS_THRESH))
    assert np.array_equal(bits(both["boxes"][5:]), bits(host["boxes"])) and both["status"][5:].tolist() == host["status"].tolist()
    long = base.copy()
    long[50:130, :, 2] = 0.0
    long[:3, :, 2] = 0.0
    long[190:, :, 2] = 0.0
    host = pkg.pipeline.track_boxes(long, vis_thresh=tk.VIS_THRESH)
    assert host["range"].tolist() == [[3, 190]]
    against_statement(numpy_out(model.track_boxes(long, vis_thresh=tk.VIS_THRESH)), host)


def test_a_track_longer_than_the_lds_buffers(model, pkg, g):
    """1100 frames > 1024: the median and the Gaussian run in the call's scratch through the same code; beside it a short one in LDS."""
    T = 1100
    kp = np.tile(g["t70_kp"][:1], (T, 1, 1))
    kp[:, :, 0] += np.arange(T)[:, None] + 5.0 * np.sin(0.7 * np.arange(T))[:, None]
    kp[:, :, 1] *= 1.0 + 0.05 * np.cos(0.11 * np.arange(T))[:, None]
    kp[np.arange(T) % 7 == 3, :, 2] = 0.1
    kp = np.concatenate([kp, g["t26gaps_kp"]])
    kw = dict(lengths=[T, 26], vis_thresh=tk.VIS_THRESH, kernel_size=5, pad="edge")
    host_median = pkg.pipeline.track_boxes(kp, return_params=True, **kw)
    against_statement(numpy_out(model.track_boxes(kp, **kw)), host_median)
    host = pkg.pipeline.track_boxes(kp, sigma=1.0, return_params=True, **kw)
    out = numpy_out(model.track_boxes(kp, sigma=1.0, **kw))
    ratio = against_statement({k: v[:T] if k != "range" else v[:1] for k, v in out.items()}, {k: v[:T] if k != "range" else v[:1] for k, v in host.items()},
                              host_median["params"][:T], 1.0)
    print(f"T = {T}: worst error / twice the Gaussian's bar = {ratio:.3g}")
    assert ratio <= 1.0


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    joints = torch.ones(8, 25, 3, dtype=torch.float64, device="cuda")
    x = torch.ones(8, dtype=torch.float64, device="cuda")
    boxes = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    status, rng = torch.full((8,), -7, dtype=torch.int32, device="cuda"), torch.full((2, 2), -7, dtype=torch.int32, device="cuda")
    filtered = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(K=25, offsets=(0, 3, 8), n_seq=None, thr=0.3, kernel=11, sigma=3.0, pad=0, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, joints.data_ptr(), K, off, len(offsets) - 1 if n_seq is None else n_seq, thr, kernel, sigma, pad, boxes.data_ptr(), status.data_ptr(),
                rng.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_track_boxes(*args)

    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(K=0), b"K 0"), (dict(K=65), b"K 65"), (dict(n_seq=0), b"n_seq 0"), (dict(null=1), b"null"), (dict(null=3), b"null"), (dict(null=9), b"null"),
                     (dict(null=10), b"null"), (dict(null=11), b"null"), (dict(offsets=(1, 8)), b"not 0"), (dict(offsets=(0, 5, 3)), b"increase"),
                     (dict(offsets=(0, 4, 4)), b"empty"), (dict(kernel=10), b"kernel_size 10"), (dict(kernel=33), b"kernel_size 33"), (dict(kernel=0), b"kernel_size 0"),
                     (dict(kernel=-3), b"kernel_size -3"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=nan), b"sigma"), (dict(sigma=inf), b"sigma"),
                     (dict(sigma=16.5), b"sigma"), (dict(thr=nan), b"vis_thresh"), (dict(thr=inf), b"vis_thresh"), (dict(pad=2), b"unknown pad 2"),
                     (dict(pad=-1), b"unknown pad -1")):
        assert call(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    off = (C.c_int32 * 3)(0, 3, 8)
    for fn, args, word in ((lib.grnet_op_median1d, [h, x.data_ptr(), off, 2, 10, 0, filtered.data_ptr(), stream], b"kernel_size 10"),
                           (lib.grnet_op_median1d, [h, x.data_ptr(), off, 2, 11, 3, filtered.data_ptr(), stream], b"unknown pad"),
                           (lib.grnet_op_median1d, [h, None, off, 2, 11, 0, filtered.data_ptr(), stream], b"null"),
                           (lib.grnet_op_median1d, [h, x.data_ptr(), off, 2, 11, 0, x.data_ptr(), stream], b"must not be x_dev"),
                           (lib.grnet_op_gauss1d, [h, x.data_ptr(), off, 2, 0.0, filtered.data_ptr(), stream], b"sigma"),
                           (lib.grnet_op_gauss1d, [h, x.data_ptr(), off, 2, 17.0, filtered.data_ptr(), stream], b"sigma"),
                           (lib.grnet_op_gauss1d, [h, x.data_ptr(), off, 0, 3.0, filtered.data_ptr(), stream], b"n_seq 0"),
                           (lib.grnet_op_gauss1d, [h, x.data_ptr(), (C.c_int32 * 3)(0, 8, 8), 2, 3.0, filtered.data_ptr(), stream], b"empty")):
        assert fn(*args) == pkg._lib.EINVAL, word
        assert word in lib.grnet_last_error(h), (word, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((boxes == -7.0).all()) and bool((status == -7).all()) and bool((rng == -7).all()) and bool((filtered == -7.0).all())      # nothing was written
    assert call() == 0                                         # the same call without a fault goes through, with every output
    torch.cuda.synchronize()
    assert not bool((boxes == -7.0).any()) and not bool((status == -7).any()) and not bool((rng == -7).any())
    ok = np.ones((4, 25, 3))
    for args, kw, word in (((ok[0],), {}, "joints2d"), ((ok,), {"lengths": [2, 1]}, "lengths"), ((ok,), {"pad": "wrap"}, "pad")):
        with pytest.raises(ValueError, match=word):
            model.track_boxes(*args, **kw)
    for kw, word in (({"kernel_size": 4}, "kernel_size"), ({"sigma": 20.0}, "sigma"), ({"vis_thresh": nan}, "vis_thresh")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.track_boxes(ok, **kw)
