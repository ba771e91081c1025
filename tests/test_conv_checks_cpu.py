"""tests/helpers/conv_checks.py, the float64 yardstick of the fp32 convolution kernels, checked without a GPU:

- on even, uneven and spiky data the three fp32 evaluations (torch's convolution, the strictly sequential chain, the F(4x4,3x3) emulation) stay
  inside their own accepted ratios, the direct ones inside the worst case of a chain of Cin x 9 terms, and a dead channel is exactly 0 in all;
- the float64 Winograd identity holds on whole maps to 1e-9 of a rounding of fp32: 56x56, 28x28 and the zero-padded 14 -> 16 and 7 -> 8 maps;
- seven planted faults, each applied to the F(4x4,3x3) emulation's own output: every one stays below rel_err < 1e-4, the bar the kernels had, and
  every one is at least 2 x outside the accepted ratio (the one in the dead channel infinitely);
- the inputs are what the recipes state; where() names borders, seams and channels; the bilinear pair and the folded BatchNorm."""
import numpy as np
import pytest
import torch

from .helpers import conv_checks as cc

N, CIN, COUT, HW = 2, 40, 32, 28
KEY = (120, 2040032)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for data in cc.DATA:
        d = cc.make_inputs(data, KEY, N, CIN, COUT, 3, HW)
        out[data] = (d, cc.Case("direct", d["x"], d["w"], d["bias"], d["residual"]), cc.Case("wino4", d["x"], d["w"], d["bias"], d["residual"]))
    return out


def test_inputs_are_what_the_recipes_state(cases):
    d = cases["uneven"][0]
    sp = cc.special_channels(COUT)
    assert sp == {"quiet": (16, 31), "mid": 9, "dead": 0}
    assert cc.special_channels(25)["quiet"] == (16, 24) and cc.special_channels(96)["quiet"] == (80, 95) and cc.special_channels(256)["quiet"] == (240, 255)
    assert not d["w"][0].any() and d["bias"][0] == 0 and not d["residual"][:, 0].any()
    scale = np.abs(d["w"]).max((1, 2, 3))
    loud = np.delete(scale, [0, 9, 16, 31])
    assert 0.1 < loud.min() and np.allclose(scale[[16, 31]] / np.median(loud), 1e-5, rtol=1.0) and np.allclose(scale[9] / np.median(loud), 1e-3, rtol=1.0)
    assert (d["x"] >= 0).all() and not d["x"][:, CIN - 1].any() and 0 < d["x"][:, 1].max() < 1e-3
    ch = d["x"].max((0, 2, 3))[:CIN - 1]
    assert np.delete(ch, 1).max() / np.delete(ch, 1).min() > 20                                # lognormal channel scales: decades apart
    s = cases["spiky"][0]["x"]
    share = (s != d["x"]).mean()
    assert 0.0005 < share < 0.002 and np.allclose(s[s != d["x"]], 50 * d["x"][s != d["x"]])    # 0.2 % of the pixels, half of them 0 after the ReLU
    e = cases["even"][0]
    assert (e["x"] < 0).any() and (e["s_out"] == 1).all()
    stem = cc.make_inputs("uneven", (121, 1), 1, 3, 64, 3, 64, 2, signed=True)
    assert (stem["x"] < 0).any() and stem["residual"].shape == (1, 64, 32, 32)
    assert cc.make_inputs("uneven", KEY, N, CIN, COUT, 3, HW)["x"].tobytes() == d["x"].tobytes()


@pytest.mark.parametrize("data", cc.DATA)
def test_fp32_evaluations_stay_inside_their_accepted_ratios(cases, data):
    d, direct, wino = cases[data]
    terms = CIN * 9 + 2                                              # a chain of that many sums cannot lose more roundings of the magnitude
    for form in cc.Case.FORMS:
        bar_d, bar_w = cc.accepted(direct.yardstick_ratio(form)), cc.accepted(wino.yardstick_ratio(form))
        got = {**direct.fp32_ratios(form), **wino.fp32_ratios(form)}
        print(f"conv_bounds cpu data={data} form={form} " + " ".join(f"{k}={v:.2f}" for k, v in got.items()) + f" accepted direct={bar_d:.2f} winograd={bar_w:.2f}"
              f" rel_err winograd={cc.rel_err(wino.fp32['winograd'][0], direct.lin):.2g}")
        assert set(got) == {"torch", "sequential", "winograd"}
        assert got["torch"] <= bar_d and got["sequential"] <= bar_d and got["winograd"] <= bar_w
        assert got["torch"] <= terms and got["sequential"] <= terms
        assert bar_d >= cc.FACTOR and bar_w >= cc.FACTOR
    if data != "even":                                               # the dead channel: exactly 0 in every evaluation, magnitude 0
        assert not direct.lin_mag[:, 0].any()
        assert all(not lin[:, 0].any() for lin, _ in {**direct.fp32, **wino.fp32}.values())
    assert cc.rel_err(wino.fp32["winograd"][0], direct.lin) < 1e-5      # what the bar of before sees of the emulation: nothing


@pytest.mark.parametrize("shape", [(1, 8, 24, 56), (2, 40, 32, 28), (3, 16, 20, 14), (5, 16, 20, 7)], ids=lambda s: "x".join(map(str, s)))
def test_winograd_identity_in_float64_on_whole_maps(shape):
    """Border tiles read the zero padding; 14 and 7 are no multiple of 4: the map is padded to 16 / 8 and the outputs beyond it are dropped."""
    n, cin, cout, h = shape
    for data in ("even", "spiky"):
        d = cc.make_inputs(data, (122, h), n, cin, cout, 3, h)
        ref, mag = cc.conv_reference(d["x"], d["w"]), cc.conv_magnitude(d["x"], d["w"])
        got = cc.winograd_f43(d["x"], d["w"], np.float64)
        assert got.shape == ref.shape and got.dtype == np.float64
        assert (np.abs(got - ref) <= 1e-9 * mag).all(), cc.ratio(got, ref, mag)          # 1e-9 of each element's own magnitude


def test_planted_faults(cases):
    """Each fault on the linear result of the F(4x4,3x3) emulation on uneven data.  Fixed, not measured: below the bar of before, and at least
    2 x outside the accepted ratio."""
    d, _, wino = cases["uneven"]
    ref, mag = wino.reference("linear")
    out = wino.fp32["winograd"][0]
    clean = cc.ratio(out, ref, mag)[0]
    bar = cc.accepted(clean)
    assert clean <= bar and cc.rel_err(out, ref) < cc.OLD_BAR
    worst = {}
    for name in cc.PLANTED_FAULTS:
        bad = cc.plant(name, out, d["x"], d["w"], ref, mag)
        assert not np.array_equal(bad, out)
        old, (new, at) = cc.rel_err(bad, ref), cc.ratio(bad, ref, mag)
        worst[name] = new / bar
        print(f"{name:70s} rel_err {old:8.2g} PASSES the bar of before   per-element {new:10.3g} = {new / bar:9.3g} x accepted ({bar:.1f})  FLAGGED at {at} "
              f"{cc.where(at, 'wino4', {}, HW, d['s_out'])}")
        assert old < cc.OLD_BAR, (name, old)
        assert new >= 2 * bar, (name, new, bar)
    assert worst["6 1e-12 written into the dead channel"] == np.inf


def test_where_names_the_place():
    s_out = cc.output_scales(32)
    assert cc.where((0, 0, 5, 5), "wino4", {}, 28, s_out) == "dead channel"
    assert cc.where((0, 31, 0, 5), "wino4", {}, 28, s_out) == "quiet channel+border"
    assert cc.where((0, 3, 5, 4), "wino4", {}, 28, s_out) == "seam" and cc.where((0, 3, 5, 3), "wino4", {}, 28, s_out) == "seam"
    assert cc.where((0, 3, 5, 5), "wino4", {}, 28, s_out) == "interior"
    assert cc.where((0, 3, 13, 5), "wino4s", {}, 14) == "border+seam" and cc.where((0, 3, 12, 5), "wino4s", {}, 14) == "seam"
    assert cc.where((0, 3, 8, 5), "direct", {"rows": 8}, 56) == "seam" and cc.where((0, 3, 9, 5), "direct", {"rows": 8}, 56) == "interior"
    assert cc.where((0, 3, 9, 55), "pw", {}, 56) == "border"


def test_bilinear_pair_and_folded_batchnorm():
    x = cc.make_map("spiky", (123, 1), (2, 16, 7, 7))
    ref, mag = cc.bilinear2x_reference(x), cc.bilinear2x_magnitude(x)
    t64 = torch.nn.functional.interpolate(torch.from_numpy(x).double(), scale_factor=2, mode="bilinear", align_corners=True).numpy()
    assert ref.shape == (2, 16, 14, 14) and cc.ratio(t64, ref, mag)[0] < 1e-6
    assert np.array_equal(ref[:, :, 0, 0], x[:, :, 0, 0].astype(np.float64))                   # the first corner is the input's
    for shape in ((2, 16, 7, 7), (1, 8, 28, 28)):
        xs = cc.make_map("spiky", (123, 1), shape)
        rs, ms = cc.bilinear2x_reference(xs), cc.bilinear2x_magnitude(xs)
        fp32 = {k: cc.ratio(f(xs), rs, ms)[0] for k, f in (("two-tap", cc.bilinear2x_fp32), ("torch", cc.bilinear2x_torch_fp32))}
        bare = cc.ratio(cc.bilinear2x_torch_fp32(xs), rs, cc._bilinear(np.abs(cc.widen(xs)), np.float64))[0]
        print(f"bilinear2x {shape} fp32 evaluations, in roundings of the magnitude: {fp32}; torch's without the coordinates' term: {bare:.1f}")
        # 1 - lx, the product, the sum, and the same three vertically: six roundings of the values' magnitude; the coordinates' within their term
        assert max(fp32.values()) <= 6.0
    assert bare > 100                                     # what the coordinates' term is for: 28 -> 56, a weight of 0.02 on an outlier
    assert not ref[:, 15].any() and (mag >= np.abs(ref)).all()
    r, at, y, name, bar = cc.bilinear_check(cc.bilinear2x_fp32(x), x)
    assert r <= y and bar == max(cc.FACTOR, cc.FACTOR * y)
    bad = cc.bilinear2x_fp32(x)
    bad[0, 15, 3, 3] = 1e-20                                                                   # the channel of zeros must stay exactly 0
    assert cc.bilinear_check(bad, x)[0] == np.inf
    g = np.random.default_rng(5)
    w, gamma, beta, mean, var = (g.standard_normal(s).astype(np.float32) for s in ((8, 4, 3, 3), 8, 8, 8, 8))
    var = np.abs(var) + np.float32(0.1)
    xx = g.standard_normal((1, 4, 6, 6)).astype(np.float32)
    wf, shift = cc.fold_bn(w, gamma, beta, mean, var)
    bn = torch.nn.functional.batch_norm(torch.from_numpy(cc.conv_reference(xx, w)), *(torch.from_numpy(a).double() for a in (mean, var, gamma, beta)), training=False, eps=1e-5)
    assert np.abs(cc.conv_reference(xx, wf.astype(np.float64), shift) - bn.numpy()).max() < 1e-12
