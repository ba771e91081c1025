"""tests/helpers/pool_checks.py, the float64 yardstick of the attention pooling ("attention pooling, per element"), checked without a GPU:

- the reference is the oracle's keypoint_attention under oracle.float64(), and the data makers give what their recipes state;
- the two independent fp32 evaluations per kernel (the reference's order; the kernel's stated arithmetic with the merge of head_tail_kernel<true>)
  stay inside the accepted ratio on every data kind, and the yardsticks themselves stay below the ceilings the arithmetic explains: the bar of
  tests/test_gpu_pool_elements.py cannot go blind through its own yardstick;
- thirteen planted faults, each on the emulation of the kernel it belongs to: every one PASSES the bar the operation had before
  (rel_err < 1e-4 of the tensor's maximum) on the data kinds of FAULT_KINDS and FAILS the per-element rule there."""
import numpy as np
import pytest

from .helpers import pool_checks as pc

YARD_CEILING = pc.YARD_CEILING

_CASES = {}


def _case(kernel, name):
    key = (kernel, name)
    if key not in _CASES:
        _CASES[key] = pc.make_case(name, bf16=kernel == "bf16")                     # the cases of tests/test_gpu_pool_elements.py themselves
    return _CASES[key]


def test_reference_is_the_oracles_pooling_in_float64(oracle):
    case = _case("f32", "x8_signed")
    with oracle.float64():
        got = {k: np.asarray(oracle.keypoint_attention(case[f], case["heat"][:, 1:])).reshape(case["ref"][k].shape)
               for k, f in (("point_local_feat", "fa"), ("cam_shape_feats", "fb"))}
    assert all(v.dtype == np.float64 for v in got.values())
    r = pc.ratios(got, case["ref"], case["mag"])
    assert all(v < 1e-6 for v, _ in r.values()), r


def test_data_kinds_are_what_the_recipes_state():
    fa, fb = pc.make_features(3, pc.CASE_SEED)
    F = np.concatenate([fa.reshape(3, 128, -1), fb.reshape(3, 64, -1)], 1).astype(np.float64)
    assert not F[:, list(pc.DEAD)].any() and set(pc.DEAD) == {0, 5, 127, 191}
    assert (F >= 0).all() and 0.4 < (F == 0).mean() < 0.6                                     # behind a ReLU
    loud = np.abs(F).mean((0, 2))
    live = np.delete(loud, list(pc.DEAD) + list(pc.QUIET))
    assert live.max() / live.min() > 1e3                                                       # channel scales over decades
    assert all(1e-6 < loud[c] / loud.max() < 1e-4 for c in pc.QUIET) and [c % 16 for c in pc.QUIET] == [0, 15, 0, 15]
    assert len({F[i].tobytes() for i in range(3)}) == 3
    inner = np.delete(np.abs(F), np.r_[pc.QUIET_CORNER], 2)
    assert 0.0005 < (inner > 20 * loud[None, :, None] + 1e-30).mean() < 0.005                # the x 50 outliers
    sa, sb = pc.make_features(3, pc.CASE_SEED, signed=True)
    assert (sa < 0).any() and (sb < 0).any()
    top = lambda h: h.reshape(len(h), 25, -1)[:, 1:].astype(np.float64)
    h = top(pc.make_heat(3, pc.CASE_SEED, "equal"))
    assert (h == h[0, 0, 0]).all()
    h = top(pc.make_heat(3, pc.CASE_SEED, "seam"))
    assert set(h.argmax(-1).ravel().tolist()) <= {447, 448} and (np.sort(h, -1)[..., -1] - np.sort(h, -1)[..., -3] > 50).all()
    assert (h[:, 2::3, 447] == h[:, 2::3, 448]).all()
    h = top(pc.make_heat(3, pc.CASE_SEED, "ends"))
    assert (h.argmax(-1)[:, 0::2] == 0).all() and (h.argmax(-1)[:, 1::2] == pc.P - 1).all()
    h = top(pc.make_heat(3, pc.CASE_SEED, "two_maxima"))
    first, second = np.argsort(h, -1)[..., -1], np.argsort(h, -1)[..., -2]
    assert (np.take_along_axis(h, first[..., None], -1) == np.take_along_axis(h, second[..., None], -1)).all() and (first // pc.CHUNK != second // pc.CHUNK).all()
    h = top(pc.make_heat(3, pc.CASE_SEED, "underflow"))
    gap = np.sort(h.reshape(3, 24, 7, 448).max(-1), -1)
    below = (gap[..., -1:] - gap[..., :-1]).astype(np.float32)
    w = np.exp(-below)                                                                         # the merge weights in fp32
    assert below.min() > 88 and below.max() < 118 and (w == 0).any() and ((w > 0) & (w < 1.2e-38)).any()
    h = top(pc.make_heat(3, pc.CASE_SEED, "offset"))
    assert h.min() > 2.9e4
    h = top(pc.make_heat(3, pc.CASE_SEED, "graded"))
    share = np.exp(h - h.max(-1, keepdims=True))
    share /= share.sum(-1, keepdims=True)
    assert np.allclose(share[..., pc.LIGHT_POSITION], pc.LIGHT_SHARE, rtol=1e-3)
    per_range = np.sort(share.reshape(3, 24, 7, 448).sum(-1), -1)
    assert (per_range[..., :6] < 1e-4).all() and (per_range[..., :6] > 1e-6).all()
    h = top(pc.make_heat(3, pc.CASE_SEED, "quiet_joints"))
    am = h.argmax(-1)[:, 16:]
    assert (am >= pc.QUIET_CORNER.start).all() and (am < pc.QUIET_CORNER.stop).all()
    for kind in pc.HEAT_KINDS:
        bg = pc.make_heat(1, pc.CASE_SEED, kind)[:, 0]
        assert np.isfinite(bg).all() and bg.std() > 0                                          # the background is never a copy of a joint's channel


@pytest.mark.parametrize("kernel", ["f32", "bf16"])
def test_clean_emulations_sit_inside_the_accepted_ratio_on_every_data_kind(kernel):
    for name in pc.CASES:
        case = _case(kernel, name)
        yard = pc.yardsticks(kernel, case)
        accepted = pc.bars(yard)
        for which, out in case["yard_" + kernel].items():
            r = pc.ratios(out, case["ref"], case["mag"])
            print(f"{kernel} {name:13s} {which:15s} " + " ".join(f"{k}={v:.2f}@{at}" for k, (v, at) in r.items()) +
                  f"  rel_err {pc.old_bar_error(out, case['ref']):.1e}")
            assert all(r[k][0] <= accepted[k] for k in r), (kernel, name, which, r, accepted)
            assert all(r[k][0] <= YARD_CEILING[kernel] for k in r), (kernel, name, which, r)
            assert all(not np.asarray(out[k])[:, [c if k == "point_local_feat" else c - pc.CA for c in pc.DEAD if (c < pc.CA) == (k == "point_local_feat")]].any()
                       for k in pc.OUTPUTS)
        assert all(4.0 <= accepted[k] <= 4 * YARD_CEILING[kernel] for k in accepted)


# fault -> the (kernel, data kind) pairs on which it passes rel_err < 1e-4 and fails the rule; asserted pair by pair
FAULT_KINDS = {
    pc.FAULTS[0]: [("bf16", "two_maxima"), ("bf16", "seam")],
    pc.FAULTS[1]: [("bf16", "two_maxima"), ("bf16", "ends")],
    pc.FAULTS[2]: [("f32", "nearly_equal"), ("bf16", "nearly_equal")],
    pc.FAULTS[3]: [("f32", "quiet_joints")],
    pc.FAULTS[4]: [("f32", "graded"), ("bf16", "graded")],
    pc.FAULTS[5]: [("f32", "graded"), ("bf16", "graded")],
    pc.FAULTS[6]: [("f32", "graded"), ("bf16", "graded")],
    pc.FAULTS[7]: [("f32", "graded"), ("bf16", "graded")],
    pc.FAULTS[8]: [("f32", "nearly_equal"), ("bf16", "nearly_equal")],
    pc.FAULTS[9]: [("f32", "x1"), ("bf16", "x8")],
    pc.FAULTS[10]: [("f32", "x60"), ("bf16", "equal")],
    pc.FAULTS[11]: [("f32", "x8"), ("bf16", "equal")],
    pc.FAULTS[12]: [("f32", "graded"), ("bf16", "graded")],
}


@pytest.mark.parametrize("fault", pc.FAULTS)
def test_planted_fault_passes_the_bar_of_before_and_fails_the_rule(fault):
    assert set(FAULT_KINDS) == set(pc.FAULTS)
    for kernel, name in FAULT_KINDS[fault]:
        case = _case(kernel, name)
        accepted = pc.bars(pc.yardsticks(kernel, case))
        got = pc.emulate(kernel, case["heat"], case["fa"], case["fb"], fault)
        r = pc.ratios(got, case["ref"], case["mag"])
        new = max(r[k][0] / accepted[k] for k in r)
        old = pc.old_bar_error(got, case["ref"])
        worst = max(r, key=lambda k: r[k][0] / accepted[k])
        print(f"{fault:55s} {kernel:4s} {name:13s} rel_err {old:8.2g} (bar {pc.OLD_BAR:g})   per element {new:10.3g} x accepted at "
              f"{pc.where(worst, r[worst][1], case['top'])}")
        assert old < pc.OLD_BAR, (fault, kernel, name, old)
        assert new > 1.0, (fault, kernel, name, new)


def test_faults_of_one_kernel_only():
    case = _case("bf16", "quiet_joints")
    with pytest.raises(AssertionError):
        pc.emulate("bf16", case["heat"], case["fa"], case["fb"], pc.FAULTS[3])
    case = _case("f32", "x1")
    with pytest.raises(AssertionError):
        pc.emulate("f32", case["heat"], case["fa"], case["fb"], pc.FAULTS[0])


def test_ratio_excludes_nothing_and_names_the_place():
    ref = np.array([[[1.0, 0.0], [-2.0, 3.0]]])
    mag = np.array([[[1.0, 0.0], [8.0, 3.0]]])
    assert pc.ratio(ref, ref, mag) == (0.0, (0, 0, 0))
    got = ref.copy()
    got[0, 1, 0] += 8 * pc.EPS * 2.5
    assert pc.ratio(got, ref, mag) == (2.5, (0, 1, 0))
    got[0, 0, 1] = 1e-30                                                   # magnitude 0: every term is 0, the element must be exactly 0
    assert pc.ratio(got, ref, mag) == (np.inf, (0, 0, 1))
    got[0, 0, 1], got[0, 1, 1] = 0.0, np.nan
    assert pc.ratio(got, ref, mag) == (np.inf, (0, 1, 1))
    assert pc.bars({"a": (0.9, "x"), "b": (1.3, "y"), "c": 0.0}) == {"a": 4.0, "b": 5.2, "c": 4.0}
    top = np.full((2, 24), 3)
    assert pc.where("cam_shape_feats", (1, 63, 17), top) == "frame1/joint17/B.ch63(row15of16)/max_in_range3"
    assert pc.where("point_local_feat", (0, 16, 0), top) == "frame0/joint0/A.ch16(row0of16)/max_in_range3"
    line = pc.bounds_line("bf16", "seam", 3, "point_local_feat", (1.5, (0, 1, 2)), (2.0, "kernel order"), 8.0, "here")
    assert line == "pool_bounds kernel=bf16 data=seam n=3 output=point_local_feat gpu=1.500 at=(0, 1, 2) where=here yardstick=kernel_order:2.000 accepted=8.000"
    x = np.array([1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0, np.inf, np.nan], np.float32)      # ties go to the even mantissa; inf and NaN pass through
    y = pc.round_bf16(x)
    assert np.array_equal(y[:5], np.array([1.0, 1.0, 1 + 2.0 ** -6, -0.0, np.inf], np.float32)) and np.isnan(y[5])
