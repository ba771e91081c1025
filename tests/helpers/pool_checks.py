"""The yardstick of the attention pooling ("attention pooling, per element"): KeypointAttention.forward -- the softmax of every joint's
heat map over the 3136 positions, then the matmul with the features -- on the two feature maps of the PARE head, as attn_pool_kernel (fp32) or
attn_pool_bf16x_kernel<12> (bf16) and the merge at the front of head_tail_kernel<true> compute it.  Plain numpy; it imports nothing from the package
and nothing from the oracle.

reference(heat, fa, fb)            float64 on exactly the fp32 values the GPU was given: ref[c,j] = sum_p w[j,p] f[c,p] with w the softmax of heat
                                   channel 1 + j, and the MAGNITUDE mag[c,j] = sum_p w[j,p] |f[c,p]| (1 + |h[j,p] - M_j|): 2^-24 mag is one fp32 rounding
                                   of the largest partial sum any order can meet, times the conditioning of exp on a rounded argument
fp32_reference_order               yardstick (a): fp32 softmax over the whole row, then an fp32 matmul -- the reference's own order
emulate(kernel, ...)               yardstick (b): the kernel's stated arithmetic.  "f32": seven ranges, exp(h - range max), the 16x16x4 steps of
                                   four positions (p, p + 4, p + 8, p + 12), one fp32 rounding per step.  "bf16": fp32 (h - m) 1.442695..., exp2, the
                                   hi = bf16(e), lo = bf16(e - hi) split, exact products, fp32 accumulation in steps of 32 positions, hi before lo.
                                   Both: the merge as head_tail_kernel<true> writes it.  `fault` plants one of FAULTS (tests/test_pool_checks_cpu.py)
ratio / ratios / bars              max |got - ref| / (2^-24 mag) and where, per output; an element of magnitude 0 must be exactly 0; accepted =
                                   max(4, 4 x yardstick), the yardstick never taken from the code under test
yardsticks(kernel, case)           the larger of (a) and (b) per output, with its name
check / tapped_case                what a test prints and asserts for one call; the case of maps tapped from a forward
where / bounds_line                joint, channel, tensor (A or B) and the range that holds the row's maximum; the pool_bounds line
make_features / make_heat / make_case / CASES   the seeded data kinds
"""
import hashlib

import numpy as np

EPS = 2.0 ** -24
FACTOR = 4.0
P, SPLIT, CHUNK = 3136, 7, 448
CA, CB, C, J = 128, 64, 192, 24
OUTPUTS = ("point_local_feat", "cam_shape_feats")
OLD_BAR = 1e-4                                   # rel_err of the tensor's maximum: the bar the operation had before
LOG2E = np.float32(1.442695040888963)
# What an independent evaluation may reach, in roundings of the element's magnitude; a yardstick above it means the data left fp32's range (elements made
# of underflowed terms alone read 1e5) and the bar holds nothing: the tests refuse such a bar.  fp32: a sum of 3136 rounded terms walks sqrt(3136) = 56
# roundings of the magnitude at the worst (the evaluations read 0.3 .. 15).  bf16: the hi + lo split leaves 2^-17 = 128 roundings on a weight, and where
# one or two positions carry the whole mass nothing averages it: twice that, and the fp32 sums' share (the evaluations read 0.5 .. 50).
YARD_CEILING = {"f32": 56.0, "bf16": 312.0}

DEAD = (0, 5, 127, 191)                          # channels at 0: channel 0, one inside a tile, and the last channel of each tensor (127, and 191 = B's 63)
QUIET = (16, 31, 128, 159)                       # 1e-5 of the loudest channel: the first and the last row of a 16-row tile, in A and in B (128: B's first, next to A's dead last)
QUIET_CORNER = slice(3080, 3120)                 # positions whose features are 1e-6 of the others (heat kind "quiet_joints" puts joints 16 .. 23 there)
LIGHT_POSITION = 447                             # heat kind "graded": the last position of range 0 carries LIGHT_SHARE of every row's mass
LIGHT_SHARE = 2e-5


def widen(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def round_bf16(x):
    """fp32 -> nearest-even bf16 -> fp32 (NaN and inf pass through)."""
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32).reshape(x.shape)
    return np.where(np.isfinite(x), r, x)


def split(x):
    return {"point_local_feat": x[:, :CA], "cam_shape_feats": x[:, CA:]}


def _maps(heat, fa, fb, dtype, heat_channel=1):
    n = len(heat)
    h = np.asarray(heat, np.float32).reshape(n, 25, P)[:, heat_channel:heat_channel + J]
    F = np.concatenate([np.asarray(fa, np.float32).reshape(n, CA, P), np.asarray(fb, np.float32).reshape(n, CB, P)], 1)
    return h.astype(dtype), F.astype(dtype)


# ----------------------------------------------------------------------------------------------------------------- reference
def reference(heat, fa, fb):
    """(ref, mag, top): dicts of (n,128,24) / (n,64,24) float64, and top (n,24): the range that holds each row's maximum."""
    h, F = _maps(heat, fa, fb, np.float64)
    M = h.max(-1, keepdims=True)
    e = np.exp(h - M)
    w = e / e.sum(-1, keepdims=True)
    ref = F @ w.transpose(0, 2, 1)
    mag = np.abs(F) @ (w * (1.0 + np.abs(h - M))).transpose(0, 2, 1)
    return split(ref), split(mag), h.argmax(-1) // CHUNK


def fp32_reference_order(heat, fa, fb):
    """Yardstick (a): F.softmax over the whole row and torch.matmul, in fp32 (numpy's pairwise sums, the BLAS's order)."""
    h, F = _maps(heat, fa, fb, np.float32)
    e = np.exp(h - h.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True, dtype=np.float32)
    out = np.matmul(F, np.ascontiguousarray(w.transpose(0, 2, 1)))
    assert out.dtype == np.float32
    return split(out)


# ----------------------------------------------------------------------------------------------------------------- emulations
FAULTS = (
    "lo dropped",                                         # bf16
    "lo with its mantissa cut",                           # bf16
    "joint j read from heat channel j",                   # instead of j + 1
    "joints 16..23 taken from lanes 8..15",               # of the second accumulator: the fp32 kernel's zero columns
    "the last position of a range dropped",
    "the lightest range's maximum off in the merge",      # by 0.5: its weight by e^0.5
    "the heaviest range's maximum off in the merge",
    "one partial left out of the fixed-order sum",        # the lightest range's
    "the division by S using the unweighted sums",
    "a quiet channel zeroed",
    "1e-12 in the dead channel",
    "channel 127 and 128 swapped between the two tensors",
    "frame 1's features on a light position of frame 0",
)
BF16_ONLY = FAULTS[:2]
F32_ONLY = FAULTS[3:4]                                   # the bf16 kernel's lanes 8 .. 15 hold copies of joints 16 .. 23: the same fault changes nothing there


def _wave_sum(e):
    """(..., 448) fp32 -> (...): a lane adds its seven values (lane + 64 i) one after another, then the butterfly over the 64 lanes."""
    x = e.reshape(e.shape[:-1] + (CHUNK // 64, 64))
    acc = np.zeros(x.shape[:-2] + (64,), np.float32)
    for i in range(CHUNK // 64):
        acc = acc + x[..., i, :]
    w = 32
    while w:
        acc = acc[..., :w] + acc[..., w:2 * w]
        w //= 2
    return acc[..., 0]


def _steps_f32():
    """The positions of every 16x16x4 step of a range, in the kernel's order: round p0 (64), group g (16), k-step s: p0 + 16 g + s + 4 lq."""
    return [[p0 + 16 * g + s + 4 * lq for lq in range(4)] for p0 in range(0, CHUNK, 64) for g in range(4) for s in range(4)]


def _accumulate(F64, e64, steps):
    """acc[n,z,c,j] over the steps (lists of positions of a range): exact products, their sum and the addition to acc rounded to fp32 ONCE per step."""
    n = F64.shape[0]
    Fz = F64.reshape(n, C, SPLIT, CHUNK).transpose(0, 2, 1, 3)                 # (n,7,192,448)
    acc = np.zeros((n, SPLIT, C, e64.shape[2]), np.float32)
    for pos in steps:
        acc = (acc.astype(np.float64) + Fz[..., pos] @ e64[..., pos].transpose(0, 1, 3, 2)).astype(np.float32)
    return acc


def _merge(m, sm, part, fault, share):
    """head_tail_kernel<true>'s front: m, sm (n,7,24) fp32 range maxima and sums, part (n,7,192,24) fp32 -> (n,192,24) fp32.
    share (n,7,24): each range's true share of the row's mass (which range is the lightest / the heaviest)."""
    n = len(m)
    M = m.max(1, keepdims=True)
    wz = np.exp(m - M).astype(np.float32)
    pick = None
    if fault in (FAULTS[5], FAULTS[7]):
        pick = share.argmin(1)
    elif fault == FAULTS[6]:
        pick = share.argmax(1)
    sel = np.zeros(m.shape, bool) if pick is None else (np.arange(SPLIT)[None, :, None] == pick[:, None, :])
    if fault in (FAULTS[5], FAULTS[6]):
        wz = np.where(sel, np.exp((m + np.float32(0.5)) - M).astype(np.float32), wz)
    S = np.zeros((n, J), np.float32)
    acc = np.zeros((n, C, J), np.float32)
    for z in range(SPLIT):
        S = S + sm[:, z] * (np.float32(1.0) if fault == FAULTS[8] else wz[:, z])
        term = part[:, z] * wz[:, z][:, None, :]
        if fault == FAULTS[7]:
            term = np.where(sel[:, z][:, None, :], np.float32(0.0), term)
        acc = acc + term
    out = acc * (np.float32(1.0) / S)[:, None, :]
    assert out.dtype == np.float32
    return out


def emulate(kernel, heat, fa, fb, fault=None):
    """The stated arithmetic of the fp32 ("f32") or the bf16 ("bf16") pooling kernel and of the merge, on the maps the GPU is given (a bf16 handle's:
    already rounded to bf16).  Returns the dict of the two outputs, fp32."""
    assert kernel in ("f32", "bf16") and (fault is None or fault in FAULTS)
    assert (kernel == "bf16" or fault not in BF16_ONLY) and (kernel == "f32" or fault not in F32_ONLY)
    h, F = _maps(heat, fa, fb, np.float32, heat_channel=0 if fault == FAULTS[2] else 1)
    n = len(h)
    if fault == FAULTS[11]:
        F = F.copy()
        F[:, [127, 128]] = F[:, [128, 127]]
    if fault == FAULTS[12]:
        assert n >= 2
        F = F.copy()
        F[0, :, LIGHT_POSITION] = F[1, :, LIGHT_POSITION]
    hz = h.reshape(n, J, SPLIT, CHUNK).transpose(0, 2, 1, 3)                   # (n,7,24,448)
    m = hz.max(-1)
    if kernel == "f32":
        e = np.exp(hz - m[..., None])
    else:
        e = np.exp2((hz - m[..., None]) * LOG2E)
    assert e.dtype == np.float32
    sm = _wave_sum(e)
    h64 = h.astype(np.float64)
    ex = np.exp(h64 - h64.max(-1, keepdims=True)).reshape(n, J, SPLIT, CHUNK).sum(-1)
    share = (ex / ex.sum(-1, keepdims=True)).transpose(0, 2, 1)
    F64 = F.astype(np.float64)

    def rows(x):                                                               # the 32 joint columns of the two accumulators
        x = x.astype(np.float64)
        if fault == FAULTS[4]:
            x = x.copy()
            x[:, 0, :, CHUNK - 1] = 0.0
        return np.concatenate([x, np.zeros((n, SPLIT, 8, CHUNK))], 2)          # the fp32 kernel's rows 24 .. 31 are zero

    if kernel == "f32":
        part = _accumulate(F64, rows(e), _steps_f32())
    else:
        hi = round_bf16(e)
        lo = round_bf16(e - hi)
        if fault == FAULTS[0]:
            lo = np.zeros_like(lo)
        elif fault == FAULTS[1]:
            lo = (lo.view(np.uint32) & np.uint32(0xFF800000)).view(np.float32)
        steps = [list(range(p, p + 32)) for p in range(0, CHUNK, 32)]
        hi64, lo64 = rows(hi), rows(lo)
        Fz = F64.reshape(n, C, SPLIT, CHUNK).transpose(0, 2, 1, 3)
        part = np.zeros((n, SPLIT, C, 32), np.float32)
        for pos in steps:
            for x in (hi64, lo64):
                part = (part.astype(np.float64) + Fz[..., pos] @ x[..., pos].transpose(0, 1, 3, 2)).astype(np.float32)
    if fault == FAULTS[3]:
        part = np.concatenate([part[..., :16], part[..., 24:32]], -1)          # columns 8 .. 15 of the second accumulator
    else:
        part = part[..., :J]
    out = _merge(m, sm, np.ascontiguousarray(part), fault, share)
    if fault == FAULTS[9]:
        out[:, QUIET[1]] = 0.0
    if fault == FAULTS[10]:
        out[:, DEAD[0]] = np.float32(1e-12)
    return split(out)


# ----------------------------------------------------------------------------------------------------------------- the check
def ratio(got, ref, mag):
    """(max |got - ref| / (2^-24 mag), index of the worst element).  No element is excluded: where the magnitude is 0 every term of the element
    is 0, and anything but exactly 0 counts as infinitely wrong."""
    got, ref, mag = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(mag > 0, d / (EPS * mag), np.where(d == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    i = int(np.argmax(q))
    return float(q.flat[i]), tuple(int(k) for k in np.unravel_index(i, q.shape))


def ratios(got, ref, mag, frames=slice(None)):
    """output -> (ratio, index); `frames` selects the frames of ref / mag that the call was given."""
    return {k: ratio(np.asarray(got[k]).reshape(ref[k][frames].shape), ref[k][frames], mag[k][frames]) for k in OUTPUTS}


def bars(yard):
    """output -> accepted ratio: FACTOR x the yardstick's, never below FACTOR."""
    return {k: max(FACTOR, FACTOR * (r[0] if isinstance(r, tuple) else r)) for k, r in yard.items()}


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def old_bar_error(got, ref, frames=slice(None)):
    """The worst of the two tensors' rel_err: what the stage tests held below OLD_BAR."""
    return max(rel_err(np.asarray(got[k]).reshape(ref[k][frames].shape), ref[k][frames]) for k in OUTPUTS)


def yardsticks(kernel, case, frames=slice(None)):
    """output -> (ratio, name): the larger of the two independent fp32 evaluations on the frames of the case, each computed once per case."""
    key = "yard_" + kernel
    if key not in case:
        args = (case["heat"], case["fa"], case["fb"])
        case[key] = {"reference order": fp32_reference_order(*args), "kernel order": emulate(kernel, *args)}
    out = {}
    for k in OUTPUTS:
        best = max(((ratio(v[k][frames], case["ref"][k][frames], case["mag"][k][frames])[0], name) for name, v in case[key].items()))
        out[k] = best
    return out


def check(kernel, case, got, frames=slice(None)):
    """[(output, (ratio, at), (yardstick, its name), accepted, where)] of a call that was given `frames` of the case; nothing is asserted here."""
    r, yard = ratios(got, case["ref"], case["mag"], frames), yardsticks(kernel, case, frames)
    accepted = bars(yard)
    return [(k, r[k], yard[k], accepted[k], where(k, r[k][1], case["top"][frames])) for k in OUTPUTS]


_TAPPED = {}


def tapped_case(heat, fa, fb):
    """The case of maps tapped from a forward (the values the pooling launch read), reference and yardsticks computed once per distinct content."""
    heat, fa, fb = (np.ascontiguousarray(a, np.float32) for a in (heat, fa, fb))
    key = hashlib.sha256(heat.tobytes() + fa.tobytes() + fb.tobytes()).hexdigest()
    if key not in _TAPPED:
        ref, mag, top = reference(heat, fa, fb)
        _TAPPED[key] = {"name": "forward", "n": len(heat), "heat": heat, "fa": fa, "fb": fb, "ref": ref, "mag": mag, "top": top}
    return _TAPPED[key]


def where(output, at, top):
    """`at` = (frame, channel, joint) in `output`; top: the (n,24) ranges of the call's rows."""
    f, c, j = at
    tensor = "A" if output == "point_local_feat" else "B"
    return f"frame{f}/joint{j}/{tensor}.ch{c}(row{(c if tensor == 'A' else CA + c) % 16}of16)/max_in_range{int(top[f, j])}"


def bounds_line(kernel, data, n, output, res, yard, accepted, place):
    r, at = res
    return (f"pool_bounds kernel={kernel} data={data} n={n} output={output} gpu={r:.3f} at={at} where={place} "
            f"yardstick={yard[1].replace(' ', '_')}:{yard[0]:.3f} accepted={accepted:.3f}")


# ----------------------------------------------------------------------------------------------------------------- data
def _rng(seed, name):
    return np.random.default_rng([seed, *name.encode()])


def make_features(n, seed, signed=False):
    """(n,128,56,56), (n,64,56,56) fp32.  Channel scales log-uniform over four decades; N(0,1) behind a ReLU (or signed); 0.2 % of the entries x 50;
    the channels DEAD at 0; the channels QUIET at 1e-5 of the loudest; the positions QUIET_CORNER at 1e-6 of the others.  Every frame its own."""
    g = _rng(seed, f"features{n}{signed}")
    scale = 10.0 ** g.uniform(-2.0, 2.0, C)
    scale[list(QUIET)] = 1e-5 * scale.max()
    x = g.standard_normal((n, C, P))
    if not signed:
        x = np.maximum(x, 0.0)
    x = x * np.where(g.random((n, C, P)) < 0.002, 50.0, 1.0) * scale[None, :, None]
    x[:, :, QUIET_CORNER] *= 1e-6
    x[:, list(DEAD)] = 0.0
    x = x.astype(np.float32)
    return x[:, :CA].reshape(n, CA, 56, 56).copy(), x[:, CA:].reshape(n, CB, 56, 56).copy()


HEAT_KINDS = ("equal", "x1", "x8", "x60", "seam", "ends", "two_maxima", "underflow", "offset", "graded", "nearly_equal", "quiet_joints")


def make_heat(n, seed, kind):
    """(n,25,56,56) fp32; channel 0 (the background, never part of a result) is N(0,1) x 30
    (nearly_equal: like the joints' channels).
    equal: every position 0.37.  x1 / x8 / x60: N(0,1) times that.  seam: the whole mass (+60: the other positions keep e^-60 of it, which fp32 still holds) on position 447 (joints 0 mod 3), 448 (1 mod 3), both
    (2 mod 3): the seam of ranges 0 and 1.  ends: on position 0 (even joints) and 3135 (odd).  two_maxima: 4 N(0,1) with two equal maxima (+30) in two
    different ranges.  underflow: one range N(0,1), the six others 95 .. 110 below it (the merge weights pass through the denormals to 0).  offset:
    8 N(0,1) + 3e4.  graded: one range N(0,1), the six others 10.5 below, and position LIGHT_POSITION carrying LIGHT_SHARE of the row's mass.
    nearly_equal: 5e-5 N(0,1), the background too.  quiet_joints: N(0,1), joints 16 .. 23 with the whole mass inside QUIET_CORNER."""
    g = _rng(seed, f"heat{n}{kind}")
    z = g.standard_normal((n, J, P))
    j = np.arange(J)
    if kind == "equal":
        h = np.full((n, J, P), 0.37)
    elif kind in ("x1", "x8", "x60"):
        h = z * float(kind[1:])
    elif kind == "seam":
        h = z.copy()
        h[:, j % 3 != 1, 447] += 60.0
        h[:, j % 3 != 0, 448] += 60.0
        h[:, j % 3 == 2, 447] = h[:, j % 3 == 2, 448]
    elif kind == "ends":
        h = z.copy()
        h[:, 0::2, 0] += 60.0
        h[:, 1::2, P - 1] += 60.0
    elif kind == "two_maxima":
        h = 4.0 * z
        top = h.max(-1) + 30.0
        for f in range(n):
            for jj in range(J):
                ra, rb = g.choice(SPLIT, 2, replace=False)
                h[f, jj, ra * CHUNK + g.integers(CHUNK)] = h[f, jj, rb * CHUNK + g.integers(CHUNK)] = top[f, jj]
    elif kind in ("underflow", "graded"):
        h = z.reshape(n, J, SPLIT, CHUNK).copy()
        heavy = g.integers(0, SPLIT, (n, J))
        drop = g.uniform(95.0, 110.0, (n, J, SPLIT)) if kind == "underflow" else np.full((n, J, SPLIT), 10.5)
        drop[np.arange(SPLIT)[None, None, :] == heavy[..., None]] = 0.0
        h = (h - drop[..., None]).reshape(n, J, P)
        if kind == "graded":
            h[..., LIGHT_POSITION] = -np.inf
            M = h.max(-1)
            h[..., LIGHT_POSITION] = M + np.log(LIGHT_SHARE * np.exp(h - M[..., None]).sum(-1))
    elif kind == "offset":
        h = 8.0 * z + 3e4
    elif kind == "nearly_equal":
        h = 5e-5 * z
    elif kind == "quiet_joints":
        h = z.copy()
        h[:, j[16:], QUIET_CORNER.start + 4 * (j[16:] - 16)] += 60.0
    else:
        raise ValueError(kind)
    out = np.concatenate([(5e-5 if kind == "nearly_equal" else 30.0) * g.standard_normal((n, 1, P)), h], 1).astype(np.float32)
    return out.reshape(n, 25, 56, 56)


# name -> (heat kind, signed features)
CASES = {k: (k, False) for k in HEAT_KINDS}
CASES.update({"x1_signed": ("x1", True), "x8_signed": ("x8", True)})
# x 60 with signed features only.  Behind a ReLU half the features are 0, and an element whose features are 0 at every position that keeps a weight above
# fp32's range (exp(-87)) is made of underflowed terms alone: float64 gives 1e-50, any fp32 evaluation gives 0, and the rule reads 2^24 / (1 + |h - M|) =
# 1.6e5 for both yardsticks and for the kernels alike -- a bar of 6e5 roundings on the whole tensor holds nothing.
CASES["x60"] = ("x60", True)
CASE_FRAMES, CASE_SEED, OTHER_SEED = 3, 11, 12


def make_case(name, n=CASE_FRAMES, seed=CASE_SEED, bf16=False):
    """The maps of n frames (rounded to bf16 first for a bf16 handle: the values that kernel is given), with reference and magnitudes, computed once."""
    kind, signed = CASES[name]
    fa, fb = make_features(n, seed, signed)
    heat = make_heat(n, seed, kind)
    if bf16:
        heat, fa, fb = round_bf16(heat), round_bf16(fa), round_bf16(fb)
    ref, mag, top = reference(heat, fa, fb)
    return {"name": name, "n": n, "heat": heat, "fa": fa, "fb": fb, "ref": ref, "mag": mag, "top": top}
