"""The yardstick of the fp32 convolution kernels ("The bound of the convolutions, per element"): numpy and torch-CPU float64, written from
the definition of the operations -- it imports nothing from the package and nothing from the oracle.  The rule is the one of the SMPL stage
(tests/helpers/smpl_checks.py: ratio, bars, EPS, FACTOR are taken from there, not copied).

Every operation exists twice: as the computation in float64 on the fp32 inputs widened, and as its MAGNITUDE, the same computation on |x|, |w|,
|bias|, |residual|.  The magnitude of an element is the sum of the absolute values of all the terms that make it up, so 2^-24 x magnitude is one
fp32 rounding of the largest partial sum any summation order can meet.  With a ReLU the ReLU'd values are compared against the pre-activation
magnitude: |relu a - relu b| <= |a - b|.

conv_reference / conv_magnitude            nn.Conv2d with padding k // 2, + bias, + residual, ReLU
bilinear2x_reference / _magnitude          nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True); the magnitude carries the coordinates' rounding
fold_bn                                    BatchNorm2d (eval) folded into the weights and a shift, float64
torch_fp32 / sequential_fp32               the two direct fp32 evaluations: torch's convolution, and one strictly sequential chain of fp32 products
                                           and sums over (input channel, tap) -- the longest chain any direct kernel can form
winograd_f43 / winograd_f43_fp32           F(4x4,3x3) on the whole map (zero-padded to whole tiles: 14 -> 16, 7 -> 8): filter transform in float64 then
                                           stored in the working type; input transform, channel sum (one sequential chain) and output transform in the
                                           working type.  In float64 it reproduces conv_reference to 1e-9 of a rounding of fp32.
bilinear2x_fp32 / bilinear2x_torch_fp32    the two fp32 evaluations of the upsampling: the two-tap formula with fp32 coordinates, and torch's kernel
epilogue                                   + bias, + residual, ReLU in fp32 on a linear fp32 result; `residual` is one addend or a list of them (added in the
                                           listed order), `relu` a bool or a mask per output channel (a merged launch, linear below relu_from) -- here and
                                           in conv_reference / conv_magnitude / forward_check; tests/helpers/fuse_checks.py holds the fuse layers with them
accepted(yardstick ratio)                  FACTOR x the yardstick's ratio on the same inputs, never below FACTOR.  The yardstick is the larger of the
                                           direct evaluations for the direct, stem, 1x1 and fuse kernels (YARDSTICK), the Winograd emulation for wino4,
                                           wino4w and wino4s.  No element is left out; an element of magnitude 0 must equal the reference exactly.
make_inputs                                seeded inputs (Philox, keyed like the kernel tests): even, uneven, spiky; the stem's signed variant
where                                      names the place of an element: dead / quiet channel, image border, tile or workgroup seam, interior
planted faults                             PLANTED_FAULTS and plant(): the seven faults of tests/test_conv_checks_cpu.py
"""
import numpy as np
import torch
import torch.nn.functional as F

from .smpl_checks import EPS, FACTOR, bars, ratio, widen                      # one rule, not a second copy

# The transform matrices the Winograd kernels are built on (tests/test_winograd_algebra_cpu.py checks the identity tile by tile).
F23 = dict(
    BT=np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64),
    G=np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64),
    AT=np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64), m=2)
F43 = dict(
    BT=np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                 [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64),
    G=np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
                [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64),
    AT=np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64), m=4)

OLD_BAR = 1e-4                                   # rel_err = max |a - b| / max |b| over the tensor: the Winograd kernels' bar before
YARDSTICK = {"direct": "direct", "stem": "direct", "pw": "direct", "fuse": "direct", "bilinear": "bilinear",
             "wino4": "winograd", "wino4w": "winograd", "wino4s": "winograd"}
SEQUENTIAL_MAX_TERMS = 4e8                       # Cin x taps x outputs up to which the sequential chain takes a second or two
SEQUENTIAL_MIN_CHANNELS = 8


def _as64(a):
    """fp32 values widened; what is float64 already (folded weights) is taken as it is"""
    a = np.asarray(a)
    return np.ascontiguousarray(a) if a.dtype == np.float64 else widen(a)


def _t64(a, mag=False):
    a = torch.from_numpy(_as64(a))
    return a.abs() if mag else a


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ----------------------------------------------------------------------------------------------------------------- reference, magnitude
def addends(residual):
    """`residual` as the list of a launch's addends, in the order the launch adds them: None, one array, or a list of arrays"""
    return [] if residual is None else list(residual) if isinstance(residual, (list, tuple)) else [residual]


def apply_relu(y, relu):
    """relu: a bool, or a mask per output channel -- a merged launch is linear below ConvLayer::relu_from and ReLU'd from there on"""
    if isinstance(relu, (bool, np.bool_)):
        return np.maximum(y, y.dtype.type(0)) if relu else y
    mask = np.asarray(relu, bool)
    assert mask.shape == (y.shape[1],), (mask.shape, y.shape)
    return np.where(mask[None, :, None, None], np.maximum(y, y.dtype.type(0)), y)


def _conv64(x, w, bias, stride, residual, mag):
    w = _t64(w, mag)
    y = F.conv2d(_t64(x, mag), w, None if bias is None else _t64(bias, mag), stride=stride, padding=w.shape[-1] // 2)
    for r in addends(residual):                                              # float64: the order does not matter; the magnitude adds |r|
        y = y + _t64(r, mag)
    return y.numpy()


def conv_reference(x, w, bias=None, stride=1, residual=None, relu=False):
    return apply_relu(_conv64(x, w, bias, stride, residual, False), relu)


def conv_magnitude(x, w, bias=None, stride=1, residual=None):
    """The pre-activation magnitude, with or without a ReLU behind it."""
    return _conv64(x, w, bias, stride, residual, True)


def fold_bn(w, gamma, beta, mean, var, eps=1e-5):
    """BatchNorm2d in eval mode behind a convolution without bias, float64: (w x scale[o], shift[o]) with scale = gamma / sqrt(var + eps)."""
    scale = widen(gamma) / np.sqrt(widen(var) + eps)
    return widen(w) * scale[:, None, None, None], widen(beta) - widen(mean) * scale


def _taps(n_in, dtype):
    """align_corners=True, factor 2: src = dst (n_in - 1) / (2 n_in - 1); the taps floor(src), min(floor + 1, n_in - 1), the weight of the second,
    and src itself -- all in `dtype`, as an implementation in that type computes them."""
    n_out = 2 * n_in
    scale = dtype(n_in - 1) / dtype(n_out - 1)
    src = (scale * np.arange(n_out).astype(dtype)).astype(dtype)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), (src - i0.astype(dtype)).astype(dtype), src


def _bilinear(x, dtype, coordinates=False):
    y0, y1, ly, sy = _taps(x.shape[2], dtype)
    x0, x1, lx, sx = _taps(x.shape[3], dtype)
    one = dtype(1)
    a, b, c, d = x[:, :, y0][..., x0], x[:, :, y0][..., x1], x[:, :, y1][..., x0], x[:, :, y1][..., x1]
    top = (a * (one - lx) + b * lx).astype(dtype)
    bot = (c * (one - lx) + d * lx).astype(dtype)
    out = (top * (one - ly)[:, None] + bot * ly[:, None]).astype(dtype)
    if not coordinates:
        return out
    dx = (a + b) * (one - ly)[:, None] + (c + d) * ly[:, None]               # |d out / d lx| and |d out / d ly| on |x|
    dy = (a + c) * (one - lx) + (b + d) * lx
    return out + COORDINATE_ROUNDINGS * (sx * dx + sy[:, None] * dy)


COORDINATE_ROUNDINGS = 2.0     # an fp32 coordinate src = fl(fl((n - 1) / (2 n - 1)) dst) is off by up to 2 x 2^-24 src: the quotient's rounding, the product's


def bilinear2x_reference(x):
    return _bilinear(widen(x), np.float64)


def bilinear2x_magnitude(x):
    """The magnitude of the value, (1 - ly) ((1 - lx) |a| + lx |b|) + ly ((1 - lx) |c| + lx |d|), plus what the coordinates contribute: an fp32
    implementation computes lx, ly from coordinates that carry up to COORDINATE_ROUNDINGS x 2^-24 src of error, and the output moves by
    |d out / d lx| <= (1 - ly) (|a| + |b|) + ly (|c| + |d|) per unit of lx (the magnitude propagated through the weights, as smpl_checks.project
    does through the quotient).  Without that term an element whose heavy tap is 0 and whose light tap (weight 0.02) is an outlier is measured in
    roundings of 0.02 of the outlier while every fp32 implementation, torch's included, moves it by 2^-24 x 27 of it: 1 700 "roundings" on spiky
    28x28 maps.  Row and column 0 have src = 0 and get no such term; a map of zeros has magnitude 0."""
    return _bilinear(np.abs(widen(x)), np.float64, coordinates=True)


def bilinear2x_fp32(x):
    return _bilinear(np.asarray(x, np.float32), np.float32)


def bilinear2x_torch_fp32(x):
    return F.interpolate(torch.from_numpy(np.asarray(x, np.float32)), scale_factor=2, mode="bilinear", align_corners=True).numpy()


# ----------------------------------------------------------------------------------------------------------------- fp32 evaluations
def torch_fp32(x, w, stride=1):
    w = torch.from_numpy(np.asarray(w, np.float32))
    return F.conv2d(torch.from_numpy(np.asarray(x, np.float32)), w, stride=stride, padding=w.shape[-1] // 2).numpy()


def sequential_terms(x, w, stride=1):
    return x.shape[1] * w.shape[2] * w.shape[3] * x.shape[0] * w.shape[0] * (x.shape[2] // stride) * (x.shape[3] // stride)


def sequential_channels(x, w, stride=1, special=True):
    """The output channels the sequential chain is run on: all of them where that stays below SEQUENTIAL_MAX_TERMS, else as many as fit (at least
    SEQUENTIAL_MIN_CHANNELS: the four special channels and others evenly spaced), else None -- torch's result alone is the yardstick then."""
    cout = w.shape[0]
    fit = int(SEQUENTIAL_MAX_TERMS // (sequential_terms(x, w, stride) // cout))
    if fit >= cout:
        return np.arange(cout)
    if fit < SEQUENTIAL_MIN_CHANNELS:
        return None
    sp = special_channels(cout) if special else {"quiet": ()}
    fixed = sorted({*sp["quiet"], *(sp[k] for k in ("mid", "dead") if k in sp)})
    spaced = [c for c in np.linspace(1, cout - 2, fit).astype(int).tolist() if c not in fixed]
    return np.array(sorted(fixed + spaced[:fit - len(fixed)]))


def sequential_fp32(x, w, stride=1, channels=None):
    """acc = fl(acc + fl(x w)), input channel by input channel and tap by tap, every element one chain of Cin x taps fp32 roundings: the order of a
    whole-K direct kernel, which walks (channel chunk, tap) with one accumulator.  channels: the output channels to compute (all)."""
    x, w = torch.from_numpy(np.asarray(x, np.float32)), torch.from_numpy(np.asarray(w, np.float32))
    if channels is not None:
        w = w[torch.from_numpy(np.asarray(channels))]
    n, cin, h, wd = x.shape
    cout, _, k, _ = w.shape
    p = k // 2
    ho, wo = (h + 2 * p - k) // stride + 1, (wd + 2 * p - k) // stride + 1
    xp = F.pad(x, (p, p, p, p))
    acc = torch.zeros(n, cout, ho, wo, dtype=torch.float32)
    for c in range(cin):
        for ky in range(k):
            for kx in range(k):
                patch = xp[:, c, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
                acc.add_(patch.unsqueeze(1) * w[None, :, c, ky, kx, None, None])
    return acc.numpy()


def winograd_f43(x, w, dtype=np.float32):
    """A^T [ sum_c (G g G^T) . (B^T d B) ] A on every 4x4 output tile of the map (the map zero-padded to whole tiles, as the kernels do it; the
    padding's outputs are dropped).  (n,cin,h,w), (cout,cin,3,3) -> (n,cout,h,w) in `dtype`."""
    td = torch.float32 if dtype == np.float32 else torch.float64
    x = np.asarray(x, np.float32).astype(dtype)
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    th, tw = -(-h // 4), -(-wd // 4)
    xp = np.zeros((n, cin, 4 * th + 2, 4 * tw + 2), dtype)
    xp[:, :, 1:h + 1, 1:wd + 1] = x
    d = np.lib.stride_tricks.sliding_window_view(xp, (6, 6), axis=(2, 3))[:, :, ::4, ::4]          # (n,cin,th,tw,6,6)
    BT, AT = torch.from_numpy(F43["BT"].astype(dtype)), torch.from_numpy(F43["AT"].astype(dtype))
    V = torch.matmul(torch.matmul(BT, torch.from_numpy(np.ascontiguousarray(d))), BT.T)           # two passes, each rounded to dtype
    V = V.reshape(n, cin, th * tw, 36)
    U = torch.from_numpy(np.einsum("ia,ocab,jb->ocij", F43["G"], _as64(w), F43["G"]).astype(dtype)).reshape(cout, cin, 36)
    M = torch.zeros(n, cout, th * tw, 36, dtype=td)
    for c in range(cin):                                                                          # one chain over the input channels
        M.add_(U[None, :, c, None, :] * V[:, None, c])
    Y = torch.matmul(torch.matmul(AT, M.reshape(n, cout, th, tw, 6, 6)), AT.T)                    # (n,cout,th,tw,4,4)
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(n, cout, 4 * th, 4 * tw)[:, :, :h, :wd].contiguous().numpy()


def winograd_f43_fp32(x, w):
    return winograd_f43(x, w, np.float32)


def epilogue(lin, bias=None, residual=None, relu=False):
    """fl(fl(lin + bias) + residual), ReLU: what follows the sum in fp32.  Several addends are added in the listed order; relu may be a mask per
    output channel (apply_relu)."""
    y = np.asarray(lin, np.float32)
    if bias is not None:
        y = y + np.asarray(bias, np.float32)[None, :, None, None]
    for r in addends(residual):
        y = y + np.asarray(r, np.float32)
    return apply_relu(y, relu)


def accepted(yardstick_ratio):
    return bars({"r": yardstick_ratio})["r"]


class Case:
    """One set of inputs with everything the forms of a check share, computed once: the linear float64 result and magnitude, and the linear results
    of the yardstick's fp32 evaluations.  check(got, form) -> (ratio, index, yardstick ratio, yardstick's name, accepted ratio)."""
    FORMS = {"linear": (False, False, False), "bias_relu": (True, False, True), "bias_relu_res": (True, True, True)}

    def __init__(self, family, x, w, bias=None, residual=None, stride=1):
        self.family, self.x, self.w, self.bias, self.residual, self.stride = family, x, w, bias, residual, stride
        self.lin = _conv64(x, w, None, stride, None, False)
        self.lin_mag = _conv64(x, w, None, stride, None, True)
        every = np.arange(w.shape[0])
        if YARDSTICK[family] == "winograd":
            self.fp32, self.yardstick = {"winograd": (winograd_f43_fp32(x, w), every)}, "winograd"
        else:
            self.fp32, self.yardstick = {"torch": (torch_fp32(x, w, stride), every)}, "torch"
            ch = sequential_channels(x, w, stride)
            if ch is not None:
                self.fp32["sequential"] = (sequential_fp32(x, w, stride, ch), ch)
                self.yardstick += "+sequential" + ("" if len(ch) == len(every) else f"[{len(ch)}/{len(every)}ch]")

    def reference(self, form):
        b, r, relu = self.FORMS[form]
        ref = self.lin.copy()
        mag = self.lin_mag.copy()
        if b:
            ref += widen(self.bias)[None, :, None, None]
            mag += np.abs(widen(self.bias))[None, :, None, None]
        if r:
            ref += widen(self.residual)
            mag += np.abs(widen(self.residual))
        return (np.maximum(ref, 0.0) if relu else ref), mag

    def fp32_ratios(self, form, ref=None, mag=None):
        """name -> the ratio of that fp32 evaluation under the form's epilogue, on the output channels it was computed on"""
        b, r, relu = self.FORMS[form]
        if ref is None:
            ref, mag = self.reference(form)
        return {k: ratio(epilogue(lin, self.bias[ch] if b else None, self.residual[:, ch] if r else None, relu), ref[:, ch], mag[:, ch])[0]
                for k, (lin, ch) in self.fp32.items()}

    def yardstick_ratio(self, form, ref=None, mag=None):
        return max(self.fp32_ratios(form, ref, mag).values())

    def check(self, got, form):
        ref, mag = self.reference(form)
        y = self.yardstick_ratio(form, ref, mag)
        r, at = ratio(got, ref, mag)
        return r, at, y, self.yardstick, accepted(y)


def forward_check(family, got, x, w64, shift64, stride=1, residual=None, relu=False):
    """One launch of the forward on its own tapped input x (and residual): w64, shift64 are the BatchNorm-folded weights and shift in float64
    (fold_bn), which is what the reference and the magnitude are computed from; the yardstick's fp32 evaluation takes them rounded to fp32, the
    Winograd emulation transforms the float64 filter as the weight packers do.  residual: one addend or a list of them (the reference adds them in
    float64, the magnitude their absolute values, the fp32 yardstick adds them in the listed order); relu: a bool or a mask per output channel (a
    merged launch: w64, shift64 are the segments' concatenated).  Returns what Case.check returns."""
    ref, mag = conv_reference(x, w64, shift64, stride, residual, relu), conv_magnitude(x, w64, shift64, stride, residual)
    if not isinstance(relu, (bool, np.bool_)):
        relu = np.asarray(relu, bool)
    w32, b32 = w64.astype(np.float32), shift64.astype(np.float32)
    if YARDSTICK[family] == "winograd":
        fp32, name = {"winograd": (winograd_f43(x, w64, np.float32), np.arange(len(w64)))}, "winograd"
    else:
        fp32, name = {"torch": (torch_fp32(x, w32, stride), np.arange(len(w64)))}, "torch"
        ch = sequential_channels(x, w32, stride, special=False)
        if ch is not None:
            fp32["sequential"] = (sequential_fp32(x, w32, stride, ch), ch)
            name += "+sequential" + ("" if len(ch) == len(w64) else f"[{len(ch)}/{len(w64)}ch]")
    on = lambda ch: relu if isinstance(relu, (bool, np.bool_)) else relu[ch]
    y = max(ratio(epilogue(lin, b32[ch], [r[:, ch] for r in addends(residual)], on(ch)), ref[:, ch], mag[:, ch])[0] for lin, ch in fp32.values())
    r, at = ratio(got, ref, mag)
    return r, at, y, name, accepted(y)


def bilinear_check(got, x):
    ref, mag = bilinear2x_reference(x), bilinear2x_magnitude(x)
    y = max(ratio(bilinear2x_fp32(x), ref, mag)[0], ratio(bilinear2x_torch_fp32(x), ref, mag)[0])
    r, at = ratio(got, ref, mag)
    return r, at, y, "two-tap+torch", accepted(y)


# ----------------------------------------------------------------------------------------------------------------- inputs
DATA = ("even", "uneven", "spiky")
SPIKE_SHARE, SPIKE_GAIN = 0.002, 50.0


def special_channels(cout):
    """Where the uneven weights put their four special output channels: s_out = 1e-5 on the first channel of the last 16-channel block and on the
    last valid channel before the padding (24 of 25, 95 of 96, 39 of 40), 1e-3 on an interior channel, exactly 0 (dead) on channel 0, the first of
    a block."""
    assert cout >= 20
    first, last = 16 * ((cout - 1) // 16), cout - 1
    if first == last:
        first -= 16
    return {"quiet": (first, last), "mid": cout // 4 + 1, "dead": 0}


def output_scales(cout):
    sp = special_channels(cout)
    s = np.ones(cout)
    s[list(sp["quiet"])], s[sp["mid"]], s[sp["dead"]] = 1e-5, 1e-3, 0.0
    return s


def input_scales(g, cin):
    """lognormal (sigma 1) per input channel; the last valid channel exactly 0, channel 1 at 1e-4"""
    s = np.exp(g.standard_normal(cin))
    if cin >= 8:
        s[cin - 1], s[1] = 0.0, 1e-4
    return s


def make_inputs(data, key, n, cin, cout, k=3, h=56, stride=1, signed=False):
    """dict(x (n,cin,h,h), w (cout,cin,k,k), bias (cout), residual (n,cout,ho,ho), s_out (cout)), fp32, from Philox(key).
    even: x ~ N(0,1), He-scaled weights, bias 0.1 N(0,1), residual N(0,1) -- the data of the kernel tests.
    uneven: x = relu(N(0,1)) s_in[c] (signed: N(0,1) s_in[c], the stem's frames); w = He-scaled x s_out[o]; bias and residual x s_out[o], so that a
    quiet channel stays quiet.  spiky: uneven with SPIKE_SHARE of the input pixels x SPIKE_GAIN."""
    assert data in DATA
    g = np.random.Generator(np.random.Philox(key=list(key)))
    ho = (h + 2 * (k // 2) - k) // stride + 1
    x = g.standard_normal((n, cin, h, h))
    w = g.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))
    b = g.standard_normal(cout) * 0.1
    r = g.standard_normal((n, cout, ho, ho))
    s_out = np.ones(cout)
    if data != "even":
        s_in, s_out = input_scales(g, cin), output_scales(cout)
        x = (x if signed else np.maximum(x, 0.0)) * s_in[None, :, None, None]
        w, b, r = w * s_out[:, None, None, None], b * s_out, r * s_out[None, :, None, None]
        if data == "spiky":
            x = np.where(g.random(x.shape) < SPIKE_SHARE, x * SPIKE_GAIN, x)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return {"x": f(x), "w": f(w), "bias": f(b), "residual": f(r), "s_out": s_out}


def make_map(data, key, shape):
    """The input of an upsampling: even N(0,1); uneven relu(N(0,1)) x lognormal channel scale, one channel 0, one at 1e-4; spiky as above."""
    g = np.random.Generator(np.random.Philox(key=list(key)))
    x = g.standard_normal(shape)
    if data != "even":
        x = np.maximum(x, 0.0) * input_scales(g, shape[1])[None, :, None, None]
        if data == "spiky":
            x = np.where(g.random(x.shape) < SPIKE_SHARE, x * SPIKE_GAIN, x)
    return np.ascontiguousarray(x, np.float32)


# ----------------------------------------------------------------------------------------------------------------- where
def where(index, family, form, h, s_out=None):
    """Names the place of element (n, c, y, x) of an h x h output: dead / quiet channel (from s_out), image border, either side of a tile or
    workgroup seam of the kernel family (the slices of tests/test_gpu_f32_stages.py's _seams), else interior."""
    from ..test_gpu_f32_stages import _seams                                   # imported here: that module imports this one
    _, c, y, x = index
    tags = []
    if s_out is not None and s_out[c] == 0:
        tags.append("dead channel")
    elif s_out is not None and s_out[c] < 1:
        tags.append("quiet channel")
    border = seam = False
    for k, sl in enumerate(_seams(family, form or {}, h)):
        m = np.zeros((1, 1, h, h), bool)
        m[sl] = True
        if m[0, 0, y, x]:
            border, seam = border or k < 4, seam or k >= 4
    tags += ["border"] * border + ["seam"] * seam
    return "+".join(tags) if tags else "interior"


# ----------------------------------------------------------------------------------------------------------------- planted faults
PLANTED_FAULTS = (
    "1 a quiet output channel written as zeros",
    "2 tap (2,2) dropped at the image corner of a quiet channel",
    "3 1e-6 of a loud channel leaking into a quiet one",
    "4 one 4x4 tile of a quiet channel taken from the other image",
    "5 a 1e-3 relative error on the whole last column of the 1e-3 channel",
    "6 1e-12 written into the dead channel",
    "7 a 2e-4 relative error at one pixel of a loud channel",
)


def plant(name, out, x, w, ref, mag):
    """A copy of the linear result `out` (n >= 2 images) with fault `name` planted; x, w are the inputs, ref / mag the float64 pair (used only to
    pick the loud pixel of fault 7: the one of its channel where the least cancels, below 0.4 of the tensor's maximum)."""
    sp = special_channels(out.shape[1])
    q, q2, mid, dead = sp["quiet"][1], sp["quiet"][0], sp["mid"], sp["dead"]
    loud = next(c for c in range(out.shape[1] // 2, out.shape[1]) if c not in (q, q2, mid, dead))
    bad = np.array(out, np.float32)
    k = PLANTED_FAULTS.index(name) + 1
    if k == 1:
        bad[:, q] = 0.0
    elif k == 2:                                                # output (0,0) reads input (1,1) through tap (2,2); the far corner reads the padding
        bad[:, q, 0, 0] -= (w[q, :, 2, 2][None] * x[:, :, 1, 1]).sum(1)
    elif k == 3:
        bad[:, q2] += np.float32(1e-6) * bad[:, loud]
    elif k == 4:
        bad[0, q, 8:12, 8:12] = out[1, q, 8:12, 8:12]
    elif k == 5:
        bad[:, mid, :, -1] *= np.float32(1 + 1e-3)
    elif k == 6:
        bad[0, dead, 5, 5] = 1e-12
    else:
        score = np.where(np.abs(ref[0, loud]) < 0.4 * np.abs(ref).max(), np.abs(ref[0, loud]) / mag[0, loud], 0.0)
        y, xx = np.unravel_index(int(np.argmax(score)), score.shape)
        bad[0, loud, y, xx] *= np.float32(1 + 2e-4)
    return bad
