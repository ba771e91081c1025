"""The box from 2D joints on the GPU (grnet_bbox_from_joints2d / grnet_op_medoid, csrc/bbox_kernels.hip): the reference's boxes bit for
bit on the golden cases, the 1-medoid's cost bound at the sizes where a row tile, a column tile or a tail can go wrong, forced column splits,
batched against single calls, ties, the frame rule, the medians and the small-box branch, refusals, a handle without weights, openpose_boxes.

The bound: distances are formed in float32 (three differences, squares, sum, one square root of <= 1 ulp: within 3 * 2^-24 = 1.8e-7 of the exact
distance between the float32 points) and summed in float64, so the float64 cost of the row the GPU picks is <= (1 + 1e-6) times the minimum and the
cost it reports is within 1e-6 of that row's float64 cost.  The golden cases have gaps >= 1e-5 between the medoid and the next centre."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from .conftest import ROOT
from .helpers import bbox_checks as bc
from .helpers import openpose_files

pytestmark = pytest.mark.gpu
CASES = ("t1", "t2", "t11", "t41", "t400", "allbelow", "small")
REL = 1e-6


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


@pytest.fixture(scope="module")
def golden_bbox():
    return np.load(os.path.join(ROOT, "tests", "golden", "bbox_joints2d.npz"))


def random_points(n, seed=7):
    g = np.random.Generator(np.random.Philox(key=[seed, n]))
    return np.stack([g.uniform(0, 1920, n), g.uniform(0, 1080, n), g.uniform(0, 1, n)], 1).astype(np.float32)


def random_joints(T, K, seed, height=600.0):
    g = np.random.Generator(np.random.Philox(key=[seed, T * 100 + K]))
    kp = np.empty((T, K, 3))
    kp[:, :, 0] = 300.0 + 40.0 * np.arange(T)[:, None] + g.uniform(-60, 60, (T, K))
    kp[:, :, 1] = 540.0 + g.uniform(-height / 2, height / 2, (T, K))
    kp[:, :, 2] = g.uniform(0.0, 1.0, (T, K))
    return kp


@pytest.mark.parametrize("case", CASES)
def test_golden_boxes_bit_for_bit(model, golden_bbox, case):
    kp, want = golden_bbox[case + "_kp"], golden_bbox[case + "_bbox"]
    box, index = model.bbox_from_joints2d(kp, return_index=True)
    assert box.dtype == torch.float64 and tuple(box.shape) == (1, 4) and index.dtype == torch.int32
    box, index = box.cpu().numpy(), int(index.cpu()[0])
    points, _ = bc.prepare(kp)
    print(f"{case}: box {box[0]} index {index} (golden medoid {int(golden_bbox[case + '_medoid'])}, gap {float(golden_bbox[case + '_gap']):.2e})")
    assert np.array_equal(box[0], want[0])
    assert 0 <= index < points.shape[0] and tuple(points[index, :2].astype(np.float64)) == tuple(want[0, :2])
    if case + "_cost" in golden_bbox.files:
        costs = golden_bbox[case + "_cost"]
        assert costs[index] <= (1 + REL) * costs.min()


@pytest.mark.parametrize("n", (1, 25, 255, 256, 257, 1023, 1025, 10000))
def test_medoid_cost_bound(model, n):
    p = random_points(n)
    index, cost = model.op_medoid(p)
    assert index.dtype == torch.int32 and cost.dtype == torch.float64 and tuple(index.shape) == tuple(cost.shape) == (1,)
    i, c = int(index.cpu()[0]), float(cost.cpu()[0])
    costs = bc.row_costs(p)
    print(f"n {n}: row {i} (float64 argmin {int(np.argmin(costs))}), cost {c!r} against {costs[i]!r}: rel {abs(c - costs[i]) / max(costs[i], 1e-300):.2e}, "
          f"over the minimum by {costs[i] / max(costs.min(), 1e-300) - 1:.2e}")
    assert 0 <= i < n
    assert abs(c - costs[i]) <= REL * costs[i]
    assert costs[i] <= (1 + REL) * costs.min()
    assert bc.row_cost(p, i) == pytest.approx(costs[i], rel=1e-12)


def test_forced_splits_agree(model):
    p = random_points(1025)
    want, c0 = model.op_medoid(p)
    for splits in (1, 2, 3, 7):
        index, cost = model.op_medoid(p, splits=splits)
        assert int(index.cpu()[0]) == int(want.cpu()[0]), splits
        assert float(cost.cpu()[0]) == pytest.approx(float(c0.cpu()[0]), rel=REL)


def test_batched_call_equals_single_calls_and_repeats(model, golden_bbox):
    g = golden_bbox
    seqs = [g["t1_kp"], g["t2_kp"], g["t11_kp"], g["t41_kp"], g["t400_kp"], g["t41_kp"][5:8], g["t400_kp"][100:164]]
    lengths = [s.shape[0] for s in seqs]
    assert lengths == [1, 2, 11, 41, 400, 3, 64]
    cat = np.concatenate(seqs, 0)
    box, index = model.bbox_from_joints2d(cat, lengths=lengths, return_index=True)
    box2, index2 = model.bbox_from_joints2d(cat, lengths=lengths, return_index=True)
    assert tuple(box.shape) == (7, 4) and torch.equal(box, box2) and torch.equal(index, index2)
    for q, s in enumerate(seqs):
        b1, i1 = model.bbox_from_joints2d(s, return_index=True)
        assert torch.equal(b1[0], box[q]) and int(i1[0]) == int(index[q]), q


def test_more_sequences_than_one_launch_holds(model):
    """200 short sequences: two launch batches; every box equals the float64 statement's."""
    g = np.random.Generator(np.random.Philox(key=[3, 200]))
    lengths = [int(v) for v in g.integers(1, 6, 200)]
    seqs = [random_joints(T, 25, 1000 + q) for q, T in enumerate(lengths)]
    box = model.bbox_from_joints2d(np.concatenate(seqs, 0), lengths=lengths).cpu().numpy()
    for q, s in enumerate(seqs):
        assert bc.gap(bc.prepare(s)[0]) >= 1e-5, q                             # of the test's data: the centre is decided
        assert np.array_equal(box[q], bc.expected_box(s)), q


def test_ties_take_the_lowest_index(model):
    p = np.tile(np.float32([[812.5, 377.25, 0.5]]), (300, 1))
    index, cost = model.op_medoid(p)
    assert int(index.cpu()[0]) == 0 and float(cost.cpu()[0]) == 0.0
    # a copy of the medoid behind the other points, then in front of them: the first of the two equal rows
    q = random_points(600, seed=9)
    m = bc.medoid(q)
    index, _ = model.op_medoid(np.concatenate([q, q[m:m + 1]], 0))
    assert int(index.cpu()[0]) == m
    index, _ = model.op_medoid(np.concatenate([q[m:m + 1], q], 0))
    assert int(index.cpu()[0]) == 0


@pytest.mark.parametrize("T,K,height", ((4, 7, 900.0), (5, 7, 900.0), (6, 64, 300.0), (7, 1, 900.0)))
def test_frame_rule_medians_and_small_boxes(model, T, K, height):
    """Even and odd T, K other than 25 (a full wave at 64, one joint at 1), a frame whose scores are all below the threshold, and boxes
    below 500 pixels, which take the 1.8 branch (a body 300 pixels tall; one joint: height 0)."""
    kp = random_joints(T, K, 21, height)
    kp[1, :, 2] = np.linspace(0.01, 0.09, K)                                # every score of frame 1 below 0.1: all joints become its last
    want = bc.expected_box(kp)
    assert bc.gap(bc.prepare(kp)[0]) >= 1e-5 and bc.gap(bc.prepare(kp, 0.5)[0]) >= 1e-5      # of the test's data: the centres are decided
    assert (np.median(bc.prepare(kp)[1]) * 1.1 < 500) == (height == 300.0 or K == 1)                # of the test's data: which cases take the 1.8 branch
    box, index = model.bbox_from_joints2d(kp, return_index=True)
    print(T, K, box.cpu().numpy()[0], want)
    assert np.array_equal(box.cpu().numpy()[0], want)
    assert tuple(bc.prepare(kp)[0][int(index.cpu()[0]), :2]) == tuple(want[:2].astype(np.float32))
    other = model.bbox_from_joints2d(kp, threshold=0.5).cpu().numpy()[0]
    assert np.array_equal(other, bc.expected_box(kp, 0.5))


def test_refusals_launch_nothing(model, pkg):
    lib, h = pkg._lib.load(), model._h
    box = torch.full((2, 4), -7.0, dtype=torch.float64, device="cuda")
    joints = torch.zeros(4100, 25, 3, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(K, offsets, n_seq=None, threshold=0.1, joints_ptr=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        return lib.grnet_bbox_from_joints2d(h, joints.data_ptr() if joints_ptr is None else joints_ptr, K, off, len(offsets) - 1 if n_seq is None else n_seq,
                                            threshold, box.data_ptr(), None, stream)

    for args, word in (((25, [0, 4097]), b"4096"), ((0, [0, 4]), b"K 0"), ((65, [0, 4]), b"K 65"), ((25, [0, 4, 4]), b"empty"),
                       ((25, [0, 5, 3]), b"increase"), ((25, [1, 5]), b"not 0"), ((25, [0, 4], 0), b"n_seq"),
                       ((25, [0, 4], None, float("nan")), b"threshold"), ((25, [0, 4], None, 0.1, 0), b"null")):
        assert call(*args) == pkg._lib.EINVAL, args
        assert word in lib.grnet_last_error(h), (args, lib.grnet_last_error(h))
    index = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    cost = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    pts = torch.zeros(8, 4, dtype=torch.float32, device="cuda")
    for off, splits, word in (([0, 0], 0, b"empty"), ([0, 8], 65, b"splits"), ([0, 8], -1, b"splits"), ([0, 4096 * 64 + 1], 0, b"more than")):
        rc = lib.grnet_op_medoid(h, pts.data_ptr(), (C.c_int32 * 2)(*off), 1, splits, index.data_ptr(), cost.data_ptr(), stream)
        assert rc == pkg._lib.EINVAL and word in lib.grnet_last_error(h), (off, splits, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert bool((box == -7.0).all()) and int(index[0]) == -7 and float(cost[0]) == -7.0       # nothing was written
    with pytest.raises(ValueError, match="non-finite"):
        model.bbox_from_joints2d(np.full((2, 25, 3), np.inf))
    with pytest.raises(ValueError, match="lengths"):
        model.bbox_from_joints2d(np.zeros((5, 25, 3)), lengths=[2, 2])
    with pytest.raises(pkg._lib.GrnetError, match="4096"):
        model.bbox_from_joints2d(np.ones((4097, 25, 3)))


def test_a_handle_without_weights(pkg, golden_bbox):
    m = pkg.GRNet(max_frames=1)
    try:
        box = m.bbox_from_joints2d(torch.from_numpy(golden_bbox["t11_kp"])).cpu().numpy()
        assert np.array_equal(box[0], golden_bbox["t11_bbox"][0])
        p = random_points(257)
        index, _ = m.op_medoid(torch.from_numpy(p).cuda())
        costs = bc.row_costs(p)
        assert costs[int(index.cpu()[0])] <= (1 + REL) * costs.min()
    finally:
        m.close()


def test_openpose_boxes_on_the_device_equal_the_host(model, pkg, tmp_path):
    d = str(tmp_path / "openpose")
    keys, bad, chosen, _ = openpose_files.write_folder(d)
    host, host_bad = pkg.pipeline.openpose_boxes(d)
    dev, dev_bad = pkg.pipeline.openpose_boxes(d, model=model)
    assert sorted(dev) == keys and dev_bad == host_bad == bad
    for k in keys:
        assert dev[k].dtype == np.float64 and np.array_equal(dev[k], host[k]), k
