"""Every fp32 convolution kernel against float64, element by element, in roundings of each element's own magnitude (tests/helpers/conv_checks.py; DESIGN 5,
"The bound of the convolutions, per element"; the numbers of one run: profiles/conv_element_bounds.txt).

The kernels run through the single-op hooks (op_conv2d with the hints of tests/test_gpu_conv_f32.py and tests/test_gpu_parity.py, op_bilinear2x) on the
data a trained checkpoint gives them and the other tests do not: channel scales decades apart, sparse post-ReLU maps, a dead output channel, quiet
channels on the first channel of a block and on the last valid channel before the padding, and (spiky) a few very large pixels.  Per case and hint:
the plain linear form and the bias + ReLU (+ residual, where the kernel takes one) form; a first call on other data of the same shape, then the checked
call; one line `conv_bounds ...` per check (pytest -s); gpu <= accepted = FACTOR x the yardstick's ratio on the same inputs (at least FACTOR), no
element left out, and the dead channel exactly 0.  The yardstick is the F(4x4,3x3) emulation for the Winograd kernels, the larger of torch's fp32
convolution and the strictly sequential fp32 chain for the others (torch's alone where the chain would take more than a second or two: the line
says which).

Where a Winograd case has a shape of test_conv_kernel (CONV_CASES), the whole-K direct kernel runs on the same inputs and one line
`conv_amplification ...` gives the Winograd kernel's ratio over the direct kernel's on the linear form: measured and written down, not asserted."""
import numpy as np
import pytest
import torch

from .helpers import conv_checks as cc
from .test_gpu_parity import CONV_CASES

pytestmark = pytest.mark.gpu

DATA = ("uneven", "spiky")
WINO_DATA = ("even",) + DATA                      # even data as well: the Winograd kernels' amplification next to the direct kernel on all three
DIRECT_HINT = 7                                   # the whole-K direct kernel the amplification is measured against
ALL_HINTS = (14, 7, 1071, 1072, 1041, 1042, 1171, 1141)
WINO4 = [(1, 64, 64, 56), (3, 40, 96, 56), (5, 32, 256, 56), (1, 32, 32, 28), (3, 40, 96, 28), (2, 64, 64, 28)]
WINO4W = [(1, 128, 128, 56), (2, 48, 128, 56), (2, 64, 384, 56), (1, 480, 256, 56)]
WINO4S = [(1, 128, 14), (3, 256, 14), (5, 256, 7), (3, 256, 7)]
STEM = [(1, 224), (2, 64)]
PW = [(1, 64, 256), (3, 128, 25), (2, 64, 64)]
SMALLEST_S1, SMALLEST_S2 = (32, 32, 3, 1, 56), (32, 32, 3, 2, 56)
BILINEAR = [(2, 64, 28, 28), (3, 128, 14, 14), (2, 256, 7, 7), (1, 128, 28, 28)]
ids = lambda c: "x".join(map(str, c))


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=16, with_gru=False)
    yield m
    m.close()


def _wino_family(hint, cin, cout, h):
    """launch_conv_wino4's choice (conv_wino4_wide): eight waves on 56x56 maps with 128 output channels per workgroup and 16-channel chunks, unless
    hint 2003 asks for the 4-wave kernel"""
    return "wino4w" if hint == 2001 and h == 56 and cout % 128 == 0 and cin % 16 == 0 else "wino4"


def _check_conv(model, name, family, data, n, cin, cout, k, h, stride, hints, forms, key, signed=False, amplification=False):
    """family: a name, or hint -> name.  Every (hint, form) is measured and printed before anything is asserted."""
    d = cc.make_inputs(data, key, n, cin, cout, k, h, stride, signed)
    o = cc.make_inputs(data, (key[0] + 50, key[1]), n, cin, cout, k, h, stride, signed)
    fam = family if callable(family) else (lambda hint: family)
    case = cc.Case(fam(hints[0]), d["x"], d["w"], d["bias"], d["residual"], stride)
    assert len({cc.YARDSTICK[fam(hint)] for hint in hints}) == 1
    dev = lambda a: torch.from_numpy(a).cuda()
    xd, rd, xo, ro = dev(d["x"]), dev(d["residual"]), dev(o["x"]), dev(o["residual"])
    dead = cc.special_channels(cout)["dead"] if data != "even" else None
    ho = case.lin.shape[2]
    failures, linear = [], {}
    if amplification and (cin, cout, k, stride, h) in CONV_CASES:
        hints = tuple(hints) + (DIRECT_HINT,)
    for hint in hints:
        if hint == DIRECT_HINT and amplification:               # the direct kernel on the same inputs, checked by its own yardstick in test_direct_kernels
            ref, mag = case.reference("linear")
            direct = cc.ratio(model.op_conv2d(xd, d["w"], None, stride=stride, relu=False, tile_hint=hint).cpu().numpy(), ref, mag)[0]
            for (fm, hn), r in linear.items():
                print(f"conv_amplification family={fm} case={name} hint={hn} data={data} form=linear winograd={r:.3f} direct={direct:.3f} amplification={r / direct:.1f}")
            continue
        for form in forms:
            b, r, relu = cc.Case.FORMS[form]
            model.op_conv2d(xo, o["w"], o["bias"] if b else None, stride=stride, relu=relu, add=ro if r else None, tile_hint=hint)   # other data first
            got = model.op_conv2d(xd, d["w"], d["bias"] if b else None, stride=stride, relu=relu, add=rd if r else None, tile_hint=hint).cpu().numpy()
            ratio, at, y, yname, bar = case.check(got, form)
            print(f"conv_bounds family={fam(hint)} case={name} hint={hint} data={data} form={form} gpu={ratio:.3f} at={at} "
                  f"where={cc.where(at, fam(hint), {}, ho, d['s_out'])} yardstick={yname}:{y:.3f} accepted={bar:.3f}")
            if form == "linear":
                linear[fam(hint), hint] = ratio
            if not ratio <= bar:
                failures.append((hint, form, ratio, at, bar))
            if dead is not None and got[:, dead].any():
                failures.append((hint, form, "dead channel", float(np.abs(got[:, dead]).max())))
    assert not failures, (name, data, failures)


@pytest.mark.parametrize("data", WINO_DATA)
@pytest.mark.parametrize("case", WINO4, ids=ids)
def test_winograd_kernel_four_waves(model, case, data):
    """conv_wino4_f32 under hint 2001 and, where 2001 takes the eight-wave kernel (5 x 32 -> 256), under 2003: 56x56 with one block of 64 channels, 40
    input channels (five chunks) into 96 (blocks of 32), a half-full last round of workgroups; 28x28, where the last group's lower half stores nothing."""
    n, cin, cout, h = case
    _check_conv(model, ids(case), lambda hint: _wino_family(hint, cin, cout, h), data, n, cin, cout, 3, h, 1, (2001, 2003), ("linear", "bias_relu_res"),
                (130, n * 100000 + cin * 1000 + cout + h), amplification=True)


@pytest.mark.parametrize("data", WINO_DATA)
@pytest.mark.parametrize("case", WINO4W, ids=ids)
def test_winograd_kernel_eight_waves(model, case, data):
    """conv_wino4w_f32: 128 -> 128, an odd chunk count (48), three channel blocks (384), the PARE shape 480 -> 256."""
    n, cin, cout, h = case
    assert _wino_family(2001, cin, cout, h) == "wino4w"
    _check_conv(model, ids(case), "wino4w", data, n, cin, cout, 3, h, 1, (2001,), ("linear", "bias_relu_res"), (131, n * 100000 + cin * 1000 + cout + h),
                amplification=True)


@pytest.mark.parametrize("data", WINO_DATA)
@pytest.mark.parametrize("case", WINO4S, ids=ids)
def test_winograd_kernel_small_maps(model, case, data):
    """conv_wino4s_f32 on 14x14 (padded to 16) and 7x7 (padded to 8, four images per row tile: 5 and 3 images leave a partial one), with the default,
    2 and 4 waves splitting the input channels."""
    n, c, h = case
    _check_conv(model, ids(case), "wino4s", data, n, c, c, 3, h, 1, (2020, 2022, 2024), ("linear", "bias_relu_res"), (132, n * 100000 + c * 100 + h),
                amplification=True)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", STEM, ids=ids)
def test_stem_kernel(model, case, data):
    """conv_stem_f32 on signed frames with a scale per colour channel; the kernel takes no residual."""
    n, h = case
    _check_conv(model, ids(case), "stem", data, n, 3, 64, 3, h, 2, (3001,), ("linear", "bias_relu"), (133, n * 1000 + h), signed=True)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", PW, ids=ids)
def test_pointwise_kernel(model, case, data):
    """conv_pw_f32: 64 -> 256, 128 -> 25 (24 of 25 is the last valid channel of a partial block), 64 -> 64."""
    n, cin, cout = case
    _check_conv(model, ids(case), "pw", data, n, cin, cout, 1, 56, 1, (3002,), ("linear", "bias_relu_res"), (134, n * 100000 + cin * 10 + cout))


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", CONV_CASES, ids=ids)
def test_direct_kernels(model, case, data):
    """conv_direct_f32 on every shape of test_conv_kernel at one whole-K hint (7) and one 8-wave split-K hint (1171)."""
    cin, cout, k, stride, h = case
    n = 3 if h <= 28 else 2
    _check_conv(model, ids(case), "direct", data, n, cin, cout, k, h, stride, (7, 1171), ("linear", "bias_relu_res"),
                (135, (cin * 1000 + cout) * 1000 + k * 100 + stride * 10 + h % 10), signed=cin == 3)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", [SMALLEST_S1, SMALLEST_S2], ids=ids)
def test_direct_kernels_every_hint(model, case, data):
    """All eight tuner candidates on the smallest 3x3 stride-1 and the smallest stride-2 shape (output rows of 56 and 28 pixels: every tile holds them)."""
    cin, cout, k, stride, h = case
    _check_conv(model, ids(case), "direct", data, 2, cin, cout, k, h, stride, ALL_HINTS, ("linear", "bias_relu_res"), (136, stride))


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape", BILINEAR, ids=ids)
def test_bilinear2x_kernel(model, shape, data):
    x, other = cc.make_map(data, (137, shape[1] + shape[2]), shape), cc.make_map(data, (187, shape[1] + shape[2]), shape)
    model.op_bilinear2x(torch.from_numpy(other).cuda())
    got = model.op_bilinear2x(torch.from_numpy(x).cuda()).cpu().numpy()
    ratio, at, y, yname, bar = cc.bilinear_check(got, x)
    print(f"conv_bounds family=bilinear case={ids(shape)} hint=0 data={data} form=linear gpu={ratio:.3f} at={at} where={cc.where(at, 'bilinear', {}, 2 * shape[2])} "
          f"yardstick={yname}:{y:.3f} accepted={bar:.3f}")
    assert ratio <= bar, (shape, data, ratio, at, bar)
    assert not got[:, shape[1] - 1].any()                                      # the channel of zeros
