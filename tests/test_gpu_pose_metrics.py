"""The pose metrics on the GPU (grnet_pose_metrics, csrc/metric_kernels.hip) against the independent float64 checker
tests/helpers/metric_checks.py, at the smallest shapes that can break each stage.

The bars are derived in DESIGN 4.8 and stated in the checker, not measured: 1e-11 relative for mpjpe, pve and the means (differences of widened
float32 values are exact or one rounding; a correctly rounded square root and a sum of N non-negative terms give (N + 8) 2^-53, 7.7e-13 at
V = 6890); the same plus 1e-11 x (largest aligned coordinate) x unit absolute for the two accelerations; 1e-10 relative for pa_mpjpe where
gap = (s2 + sign s3) / s1 >= 1e-3.  Every frame's returned (s, R, t) must pass the certificate that trusts no SVD and reproduce the unique
objective to 1e-10; a frame whose gap is below 1e-3 is checked by those two alone, and at most 5 % of a test's frames may be such (with these
seeds none is).  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from .helpers import metric_checks as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def numpy_out(out):
    for k, v in out.items():
        assert v.dtype == torch.float64 and v.is_cuda, k
    return {k: v.cpu().numpy() for k, v in out.items()}


def run(model, pred, gt, **kw):
    out = numpy_out(model.pose_metrics(pred, gt, return_transform=True, **kw))
    want = mc.expected(pred, gt, **kw)
    aux = want[3]
    n = pred.shape[0]
    lengths = kw.get("lengths") or [n]
    assert out["per_frame"].shape == (n, 5) and out["per_sequence"].shape == (len(lengths), 5) and out["total"].shape == (5,) and out["transform"].shape == (n, 13)
    failures, worst = mc.compare((out["per_frame"], out["per_sequence"], out["total"]), want[:3], aux, kw.get("unit", 1000.0), lengths,
                                 kw.get("pred_verts") is not None)
    worst_objective = 0.0
    for f in range(n):
        tf = out["transform"][f]
        failures += [f"frame {f}: {w}" for w in mc.certificate(aux["K"][f], tf[1:10])]
        err = mc.objective_error(tf, aux["P"][f], aux["G"][f], aux["K"][f], aux["var1"][f], aux["x2"][f])
        worst_objective = max(worst_objective, err)
        if err > mc.OBJECTIVE_REL:
            failures.append(f"frame {f}: objective off by {err:.3e}")
    loose = mc.loose_frames(aux)
    print(f"errors in units of their bars: { {k: float(f'{v:.3g}') for k, v in worst.items()} }; objective {worst_objective:.2e}; smallest gap "
          f"{aux['gap'].min():.2e}; frames below gap 1e-3: {int(loose.sum())} of {n}")
    assert loose.mean() <= 0.05
    assert not failures, failures
    return out


@pytest.mark.parametrize("J", (1, 2, 3, 14, 17, 25, 49, 63, 64))
@pytest.mark.parametrize("kind", ("noisy", "mirrored", "unrelated"))
def test_joint_counts(model, J, kind):
    """1 joint: the var1 == 0 rule; 2: K of rank 1; 3: planar, rank 2; a full wave at 64.  mirrored takes the reflection branch."""
    pred, gt = mc.random_case(5, J, 11, kind)
    out = run(model, pred, gt, root=[0])
    if J == 1:
        assert np.array_equal(out["transform"][:, :10], np.tile(np.concatenate([[0.0], np.eye(3).reshape(9)]), (5, 1)))
        assert (out["per_frame"][:, :2] == 0).all()            # the root is the only joint


@pytest.mark.parametrize("n", (1, 2, 3, 64, 65, 257))
def test_call_sizes(model, n):
    pred, gt = mc.random_case(n, 25, 12)
    run(model, pred, gt, root=[0])


@pytest.mark.parametrize("root,select", ((None, None), ([0], [7]), ([2, 3], list(range(0, 25, 2))), ([0], None), ([24, 0], [24, 3, 3, 0])))
def test_root_and_select(model, root, select):
    """A select of 1 and of 13 out of 25 joints, a root of none, 1 and 2; the last case: indices out of order and repeated."""
    pred, gt = mc.random_case(6, 25, 13)
    out = run(model, pred, gt, root=root, select=select, unit=1.0)
    if select == [7]:
        assert (out["per_frame"][:, 1] == 0).all()             # one selected joint: var1 == 0, s = 0, R = I, t = that joint of gt


def test_lengths_put_nan_exactly_at_the_ends(model):
    lengths = [1, 2, 3, 5]
    pred, gt = mc.random_case(11, 14, 14)
    out = run(model, pred, gt, lengths=lengths, root=[2, 3])
    assert np.flatnonzero(~np.isnan(out["per_frame"][:, 3])).tolist() == np.flatnonzero(~np.isnan(out["per_frame"][:, 4])).tolist() == [4, 7, 8, 9]
    assert np.isnan(out["per_sequence"][:2, 3:]).all() and not np.isnan(out["per_sequence"][2:, 3:]).any()
    assert np.isnan(out["per_frame"][:, 2]).all() and np.isnan(out["per_sequence"][:, 2]).all() and np.isnan(out["total"][2])
    assert "transform" not in model.pose_metrics(pred, gt)


def verts_case(n, V, seed):
    g = np.random.Generator(np.random.Philox(key=[seed, V]))
    pv = g.normal(0.0, 0.5, (n, V, 3)).astype(np.float32)
    return pv, (pv + g.normal(0.0, 0.02, pv.shape)).astype(np.float32)


@pytest.mark.parametrize("V", (1, 255, 256, 257, 6890))
def test_vertices(model, V):
    """Fewer vertices than threads, one pass of pairs and its two neighbours, the SMPL mesh; odd V: frames that start 4-byte aligned."""
    pred, gt = mc.random_case(3, 25, 15)
    pv, gv = verts_case(3, V, 16)
    out = run(model, pred, gt, lengths=[1, 2], root=[0], pred_verts=pv, gt_verts=gv)
    assert not np.isnan(out["per_frame"][:, 2]).any() and not np.isnan(out["total"][2])


def test_vertices_have_the_same_bits_through_either_load_form(model):
    """V = 6890: frames start 8-byte aligned and go through 8-byte loads; the same floats 4 bytes further go through 4-byte loads."""
    pred, gt = mc.random_case(2, 25, 17)
    pv, gv = verts_case(2, 6890, 18)
    a = model.pose_metrics(pred, gt, pred_verts=pv, gt_verts=gv)["per_frame"]
    shifted = []
    for v in (pv, gv):
        flat = torch.zeros(v.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = torch.from_numpy(v).cuda().reshape(-1)
        shifted.append(flat[1:].reshape(v.shape))
        assert shifted[-1].data_ptr() % 8 == 4 and shifted[-1].is_contiguous()
    b = model.pose_metrics(pred, gt, pred_verts=shifted[0], gt_verts=shifted[1])["per_frame"]
    assert torch.equal(a[:, 2], b[:, 2])


# proper rotations with entries 0, +-1: with dyadic coordinates, scales and shifts, gt = c Q pred + d holds EXACTLY in float32, so the property is
# about the kernel alone and not about the rounding of the test's data
QUARTER_TURNS = {0.5: [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], 1.0: [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],
                 3.0: [[-1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]}


@pytest.mark.parametrize("c", (0.5, 1.0, 3.0))
def test_an_exact_similarity_is_removed(model, c):
    """gt = c Q pred + d gives pa_mpjpe <= 1e-10 x (largest coordinate of gt) x unit while mpjpe is large."""
    g = np.random.Generator(np.random.Philox(key=[20, int(c * 10)]))
    pred = (g.integers(-2000, 2000, (4, 25, 3)) / 1024.0).astype(np.float32)
    Q = np.array(QUARTER_TURNS[c])
    assert np.linalg.det(Q) == 1.0
    gt64 = c * pred.astype(np.float64) @ Q.T + np.array([0.25, -0.5, 2.5])
    gt = gt64.astype(np.float32)
    assert np.array_equal(gt.astype(np.float64), gt64)         # of the test's data: nothing was rounded
    out = numpy_out(model.pose_metrics(pred, gt, return_transform=True))
    want = mc.expected(pred, gt)
    bound = 1e-10 * float(np.abs(gt).max()) * 1000.0
    print(f"c {c}: pa_mpjpe {out['per_frame'][:, 1]} against {bound:.3e}; mpjpe {out['per_frame'][:, 0]}")
    assert (out["per_frame"][:, 1] <= bound).all() and (out["per_frame"][:, 0] > 100.0).all()
    assert np.allclose(out["transform"][:, 0], c, rtol=1e-12) and np.allclose(out["transform"][:, 1:10].reshape(-1, 3, 3), Q, atol=1e-12)
    assert np.allclose(out["transform"][:, 10:], [0.25, -0.5, 2.5], atol=1e-12)
    for f in range(4):
        assert mc.certificate(want[3]["K"][f], out["transform"][f, 1:10]) == []


def test_a_mirror_image_takes_the_reflection_branch(model):
    pred, _ = mc.random_case(4, 25, 21)
    gt = pred * np.float32([-1.0, 1.0, 1.0])
    out = run(model, pred, gt)
    want = mc.expected(pred, gt)
    for f in range(4):
        K = want[3]["K"][f]
        assert np.linalg.det(K) < 0                            # of the test's data: the unconstrained optimum is a reflection
    assert (np.linalg.det(out["transform"][:, 1:10].reshape(-1, 3, 3)) > 0).all() and (out["per_frame"][:, 1] > 1.0).all()


def test_equal_inputs_give_zero(model):
    """pred == gt: all five values are at most 1e-10 x (largest coordinate) x unit.  The acceleration of pred == gt is the motion of pred itself, so
    all five are asserted on a body in uniform motion (dyadic positions and velocity: every second difference is exactly zero), and the four that
    measure an error on a randomly moving body as well."""
    g = np.random.Generator(np.random.Philox(key=[22, 1]))
    body = g.integers(-2000, 2000, (1, 25, 3)) / 1024.0
    pred = (body + np.arange(7)[:, None, None] * np.array([0.125, -0.0625, 0.03125])).astype(np.float32)
    pv, _ = verts_case(7, 257, 23)
    defined = mc.structure([3, 4], True)
    for root in (None, [0], [2, 3]):
        out = numpy_out(model.pose_metrics(pred, pred, lengths=[3, 4], root=root, pred_verts=pv, gt_verts=pv))
        bound = 1e-10 * float(np.abs(pred).max()) * 1000.0
        print(f"root {root}: largest value {np.nanmax(out['per_frame']):.3e} against {bound:.3e}")
        assert np.array_equal(~np.isnan(out["per_frame"]), defined)
        assert (out["per_frame"][defined] <= bound).all() and (out["per_sequence"] <= bound).all() and (out["total"] <= bound).all()
    moving, _ = mc.random_case(7, 25, 22)
    out = numpy_out(model.pose_metrics(moving, moving, lengths=[3, 4], root=[0], pred_verts=pv, gt_verts=pv))
    bound = 1e-10 * float(np.abs(moving).max()) * 1000.0
    assert (out["per_frame"][:, [0, 1, 2]] <= bound).all() and (out["per_frame"][defined[:, 4], 4] <= bound).all()
    assert (out["per_frame"][defined[:, 3], 3] > 1.0).all()  # the motion of pred, not an error


def bits(t):
    return t.contiguous().view(torch.int64)


def test_seven_sequences_in_one_call_equal_seven_calls_bit_for_bit(model):
    lengths = [1, 2, 11, 41, 400, 3, 64]
    pred, gt = mc.random_case(sum(lengths), 25, 24)
    pv, gv = verts_case(sum(lengths), 31, 25)
    kw = dict(root=[0], select=list(range(1, 25)), pred_verts=pv, gt_verts=gv, return_transform=True)
    first = model.pose_metrics(pred, gt, lengths=lengths, **kw)
    again = model.pose_metrics(pred, gt, lengths=lengths, **kw)
    for k in first:
        assert torch.equal(bits(first[k]), bits(again[k])), k
    a = 0
    for q, T in enumerate(lengths):
        for _ in range(2):
            one = model.pose_metrics(pred[a:a + T], gt[a:a + T], **{**kw, "pred_verts": pv[a:a + T], "gt_verts": gv[a:a + T]})
            assert torch.equal(bits(one["per_frame"]), bits(first["per_frame"][a:a + T])), q
            assert torch.equal(bits(one["transform"]), bits(first["transform"][a:a + T])), q
            assert torch.equal(bits(one["per_sequence"][0]), bits(first["per_sequence"][q])), q
            assert torch.equal(bits(one["total"]), bits(one["per_sequence"][0])), q
        a += T


def test_a_frame_has_the_same_row_wherever_it_sits(model):
    pred, gt = mc.random_case(257, 25, 26)
    pv, gv = verts_case(257, 63, 27)
    whole = model.pose_metrics(pred, gt, lengths=[200, 1, 56], root=[2, 3], pred_verts=pv, gt_verts=gv, return_transform=True)
    one = model.pose_metrics(pred[200:201], gt[200:201], root=[2, 3], pred_verts=pv[200:201], gt_verts=gv[200:201], return_transform=True)
    assert torch.equal(bits(one["per_frame"][0]), bits(whole["per_frame"][200])) and torch.equal(bits(one["transform"][0]), bits(whole["transform"][200]))
    # inside one long sequence the frame's own three values are the same again, and its accelerations those of the three-frame call around it
    long = model.pose_metrics(pred, gt, root=[2, 3], pred_verts=pv, gt_verts=gv)
    three = model.pose_metrics(pred[199:202], gt[199:202], root=[2, 3], pred_verts=pv[199:202], gt_verts=gv[199:202])
    assert torch.equal(bits(long["per_frame"][200, :3]), bits(one["per_frame"][0, :3]))
    assert torch.equal(bits(long["per_frame"][200]), bits(three["per_frame"][1]))


def test_more_sequences_than_one_launch_holds(model):
    """200 short sequences: two launch batches of the acceleration and the means; the total comes from all of them."""
    g = np.random.Generator(np.random.Philox(key=[3, 200]))
    lengths = [int(v) for v in g.integers(1, 6, 200)]
    pred, gt = mc.random_case(sum(lengths), 17, 28)
    out = run(model, pred, gt, lengths=lengths, root=[0])
    a = sum(lengths[:150])
    one = numpy_out(model.pose_metrics(pred[a:a + lengths[150]], gt[a:a + lengths[150]], root=[0]))
    assert np.array_equal(one["per_sequence"][0], out["per_sequence"][150], equal_nan=True)


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    i32p = C.POINTER(C.c_int32)
    pred = torch.zeros(8, 25, 3, dtype=torch.float32, device="cuda")
    verts = torch.zeros(8, 5, 3, dtype=torch.float32, device="cuda")
    outs = [torch.full(shape, -7.0, dtype=torch.float64, device="cuda") for shape in ((8, 5), (2, 5), (5,), (8, 13))]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(J=25, offsets=(0, 3, 8), n_seq=None, select=None, n_select=None, root=None, n_root=None, pv=None, gv=None, V=5, unit=1000.0, pred_ptr=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        sel = (C.c_int32 * len(select))(*select) if select is not None else None
        rt = (C.c_int32 * len(root))(*root) if root is not None else None
        return lib.grnet_pose_metrics(h, pred.data_ptr() if pred_ptr is None else pred_ptr, pred.data_ptr(), J, off, len(offsets) - 1 if n_seq is None else n_seq,
                                      C.cast(sel, i32p) if sel is not None else None, (len(select) if select is not None else 0) if n_select is None else n_select,
                                      C.cast(rt, i32p) if rt is not None else None, (len(root) if root is not None else 0) if n_root is None else n_root,
                                      pv, gv, V, unit, *[o.data_ptr() for o in outs], stream)

    v = verts.data_ptr()
    for kw, word in ((dict(J=0), b"J 0"), (dict(J=65), b"J 65"), (dict(n_seq=0), b"n_seq"), (dict(pred_ptr=0), b"null"), (dict(offsets=(1, 8)), b"not 0"),
                     (dict(offsets=(0, 4, 4)), b"empty"), (dict(offsets=(0, 5, 3)), b"increase"), (dict(select=[0] * 65), b"n_select 65"),
                     (dict(select=[0], n_select=0), b"n_select 0"), (dict(n_select=3), b"without select_host"), (dict(select=[25]), b"select[0] = 25"),
                     (dict(select=[3, -1]), b"select[1] = -1"), (dict(root=[0] * 65), b"n_root 65"), (dict(n_root=2), b"without root_host"),
                     (dict(root=[0, 25]), b"root[1] = 25"), (dict(pv=v), b"go together"), (dict(gv=v), b"go together"), (dict(pv=v, gv=v, V=0), b"V 0"),
                     (dict(unit=float("nan")), b"unit"), (dict(unit=float("inf")), b"unit")):
        assert call(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    K = torch.zeros(2, 9, dtype=torch.float64, device="cuda")
    R = torch.full((2, 9), -7.0, dtype=torch.float64, device="cuda")
    assert lib.grnet_op_procrustes(h, K.data_ptr(), 0, R.data_ptr(), R.data_ptr(), stream) == pkg._lib.EINVAL and b"k 0" in lib.grnet_last_error(h)
    assert lib.grnet_op_procrustes(h, K.data_ptr(), 2, None, R.data_ptr(), stream) == pkg._lib.EINVAL and b"null" in lib.grnet_last_error(h)
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs) and bool((R == -7.0).all())       # nothing was written
    assert call() == 0                                         # the same call without a fault goes through, with every output
    torch.cuda.synchronize()
    assert all(not bool((o == -7.0).any()) for o in outs)
    ok, other = mc.random_case(4, 25, 29)
    bad = ok.copy()
    bad[2, 3, 1] = np.inf
    for args, kw, word in (((bad, other), {}, "non-finite"), ((ok, bad), {}, "non-finite"), ((ok, other[:3]), {}, "shape"), ((ok, other), {"lengths": [2, 1]}, "lengths"),
                           ((ok, other), {"pred_verts": np.zeros((4, 5, 3))}, "together"), ((ok, other), {"pred_verts": np.zeros((4, 5, 3)), "gt_verts": np.zeros((4, 6, 3))}, "verts"),
                           ((ok, other), {"pred_verts": np.full((4, 5, 3), np.nan), "gt_verts": np.zeros((4, 5, 3))}, "non-finite")):
        with pytest.raises(ValueError, match=word):
            model.pose_metrics(*args, **kw)
    with pytest.raises(pkg._lib.GrnetError, match="root"):
        model.pose_metrics(ok, other, root=[25])
    with pytest.raises(pkg._lib.GrnetError, match="J 65"):
        model.pose_metrics(np.zeros((2, 65, 3)), np.zeros((2, 65, 3)))


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_a_handle_without_weights(pkg, dtype):
    m = pkg.GRNet(max_frames=1, dtype=dtype)
    try:
        pred, gt = mc.random_case(9, 25, 30)
        pv, gv = verts_case(9, 257, 31)
        run(m, pred, gt, lengths=[4, 5], root=[0], pred_verts=pv, gt_verts=gv)
    finally:
        m.close()


def test_only_the_outputs_asked_for_are_written(model, pkg):
    """Any output pointer may be NULL: the total alone equals the total of a full call bit for bit."""
    lib, h = pkg._lib.load(), model._h
    pred, gt = mc.random_case(20, 25, 32)
    full = model.pose_metrics(pred, gt, lengths=[9, 11], root=[0])
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    total = torch.empty(5, dtype=torch.float64, device="cuda")
    root = (C.c_int32 * 1)(0)
    rc = lib.grnet_pose_metrics(h, p.data_ptr(), g.data_ptr(), 25, (C.c_int32 * 3)(0, 9, 20), 2, None, 0, root, 1, None, None, 0, 1000.0, None, None, total.data_ptr(), None,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.grnet_last_error(h)
    assert torch.equal(bits(total), bits(full["total"]))
