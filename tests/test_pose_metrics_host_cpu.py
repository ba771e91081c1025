"""pipeline.pose_metrics, the host statement of the pose metrics, against the independent checker tests/helpers/metric_checks.py at the
bars derived there, on the shapes of the GPU test: 1, 2 and 3 joints (the var1 == 0 rule, rank 1, planar), full skeletons up to 64 joints, a
select of 1 and of 13 joints, a root of 0, 1 and 2 joints, calls of 1 .. 257 frames, lengths [1, 2, 3, 5], vertices; the refusals."""
import numpy as np
import pytest

from .helpers import metric_checks as mc


def run(pkg, pred, gt, **kw):
    out = pkg.pipeline.pose_metrics(pred, gt, return_transform=True, **kw)
    want = mc.expected(pred, gt, **kw)
    lengths = kw.get("lengths") or [pred.shape[0]]
    failures, worst = mc.compare((out["per_frame"], out["per_sequence"], out["total"]), want[:3], want[3], kw.get("unit", 1000.0), lengths,
                                 kw.get("pred_verts") is not None)
    aux = want[3]
    for f in range(pred.shape[0]):
        tf = out["transform"][f]
        failures += [f"frame {f}: {w}" for w in mc.certificate(aux["K"][f], tf[1:10])]
        err = mc.objective_error(tf, aux["P"][f], aux["G"][f], aux["K"][f], aux["var1"][f], aux["x2"][f])
        if err > mc.OBJECTIVE_REL:
            failures.append(f"frame {f}: objective off by {err:.3e}")
    print(worst, "loose frames:", int(mc.loose_frames(aux).sum()))
    assert mc.loose_frames(aux).mean() <= 0.05
    assert not failures, failures
    return out


@pytest.mark.parametrize("J", (1, 2, 3, 14, 17, 25, 49, 63, 64))
@pytest.mark.parametrize("kind", ("noisy", "mirrored", "unrelated"))
def test_joint_counts(pkg, J, kind):
    pred, gt = mc.random_case(5, J, 11, kind)
    run(pkg, pred, gt, root=[0])


@pytest.mark.parametrize("n", (1, 2, 3, 64, 65, 257))
def test_call_sizes(pkg, n):
    pred, gt = mc.random_case(n, 25, 12)
    run(pkg, pred, gt, root=[0])


@pytest.mark.parametrize("root,select", ((None, None), ([0], [7]), ([2, 3], list(range(0, 25, 2))), ([0], None)))
def test_root_and_select(pkg, root, select):
    pred, gt = mc.random_case(6, 25, 13)
    out = run(pkg, pred, gt, root=root, select=select, unit=1.0)
    if select == [7]:
        assert (out["per_frame"][:, 1] == 0).all()             # one selected joint: var1 == 0, s = 0, R = I, t = that joint of gt


def test_lengths_and_vertices(pkg):
    lengths = [1, 2, 3, 5]
    pred, gt = mc.random_case(11, 14, 14)
    g = np.random.Generator(np.random.Philox(key=[14, 257]))
    pv = g.normal(0, 0.5, (11, 257, 3)).astype(np.float32)
    gv = (pv + g.normal(0, 0.02, pv.shape)).astype(np.float32)
    out = run(pkg, pred, gt, lengths=lengths, root=[2, 3], pred_verts=pv, gt_verts=gv)
    assert np.flatnonzero(~np.isnan(out["per_frame"][:, 3])).tolist() == [4, 7, 8, 9]
    assert np.isnan(out["per_sequence"][:2, 3:]).all() and not np.isnan(out["per_sequence"][:, 2]).any()
    assert "transform" not in pkg.pipeline.pose_metrics(pred, gt)


def test_refusals(pkg):
    f = pkg.pipeline.pose_metrics
    pred, gt = mc.random_case(4, 25, 15)
    bad = pred.copy()
    bad[1, 2, 0] = np.nan
    for args, kw, word in (((bad, gt), {}, "non-finite"), ((pred, gt[:3]), {}, "shape"), ((pred, gt), {"lengths": [2, 1]}, "lengths"),
                           ((pred, gt), {"lengths": [4, 0]}, "lengths"), ((pred, gt), {"root": [25]}, "root"), ((pred, gt), {"select": [-1]}, "select"),
                           ((pred, gt), {"select": []}, "select"), ((pred, gt), {"pred_verts": np.zeros((4, 5, 3))}, "together"),
                           ((pred, gt), {"pred_verts": np.zeros((4, 5, 3)), "gt_verts": np.zeros((3, 5, 3))}, "verts"),
                           ((np.zeros((2, 65, 3)), np.zeros((2, 65, 3))), {}, "64"), ((pred, gt), {"unit": float("inf")}, "unit")):
        with pytest.raises(ValueError, match=word):
            f(*args, **kw)
