"""The yardstick of the fp32 fuse layers ("The fuse layers, per element"), built on tests/helpers/conv_checks.py: the rule (ratio, bars,
EPS, FACTOR), the float64 convolution, the two direct fp32 evaluations and the folded BatchNorm are taken from there, not copied.  Numpy and
torch-CPU float64 from the definition of the layer (hrnet.py:189-244 as used by :258-265); nothing is imported from the package or the oracle.

Output i of a module with nb branches is relu(sum_j term_ij): term_ii = x_i; j > i: nearest_up_{2^(j-i)}(BN(conv1x1(x_j))); j < i: a chain of i - j
stride-2 3x3 convolutions with BatchNorm, ReLU between them and none behind the last.  The fp32 plan (csrc/grnet_plan.cpp hr_fuse_grouped) runs it as

  down     the stride-2 convolutions of the chains, each its own launch -- except the first links of all chains that start at one branch, which
           are ONE launch: the segments' output channels side by side, linear below ConvLayer::relu_from (the whole chain of output j + 1),
           ReLU'd from there on.  Taps "<stage>.<m>.d<i>.<j>.<level>", one per slice of a merged launch.
  up       ONE hr_fuse_up_f32 launch for outputs 0 .. nb-2: x_i + the finished chains D_ij + the summed shifts + the 1x1 terms, ReLU.
  finish   ONE stride-2 convolution from branch nb-2 for output nb-1, with x_{nb-1} and the finished chains as addends, ReLU.

fuse_launches(nb)            those launches in plan order, by tap names relative to the module ("x1", "d2.0.0", "y0")
FuseWeights(sd, prefix)      the BatchNorm-folded float64 weights and shifts of a module's fuse terms
check_launch(...)            one launch on its own tapped inputs: conv_checks.forward_check for down / finish, fuse_up_check for every output of up
fuse_up_check(...)           reference, magnitude (sum_j |shift_j|, not |sum shift|) and the larger of two fp32 compositions as the yardstick
where(...)                   channel class (dead-term, quiet, mid, loud), image border, band seam, source-pixel seam of the coarsest source
uneven_fuse_state_dict       the LAST BatchNorm of every fuse term scaled per output channel: conv_checks.output_scales x 10^-u, u from Philox
silent_branch_state_dict     every x_b exactly 0 on its first quiet channel and its 1e-3 channel: there an element of y_i IS its small terms
PLANTED_FAULTS, plant()      the ten faults of tests/test_fuse_checks_cpu.py
"""
import numpy as np

from . import conv_checks as cc
from .conv_checks import EPS, FACTOR, accepted, bars, ratio, rel_err, widen      # noqa: F401  (one rule: re-exported for the tests)

BR = (32, 64, 128, 256)                            # channels of branch b; its maps are (56 >> b) x (56 >> b)
OLD_BAR = 2e-5                                     # rel_err of oracle.hr_fuse against the tapped y_i: the only bar the fuse layers had
STAGES = (("stage2", 1, 2), ("stage3", 4, 3), ("stage4", 3, 4))
DECADES = (0, 0, 0, 1, 2, 3)                       # u: the last BatchNorm of a term is scaled by output_scales(C_i) x 10^-u[c]
BN_FIELDS = (".weight", ".bias", ".running_mean", ".running_var")


def modules():
    return [(stage, m, nb) for stage, n_mod, nb in STAGES for m in range(n_mod)]


# ----------------------------------------------------------------------------------------------------------------- the launches
def chain_last(i, j):
    return i - j - 1


def fuse_launches(nb):
    """The launches of one fuse layer in plan order.  down: dict(kind, x, segs [(i, j, level)], taps); up: dict(kind, outputs [dict(i, base, extras,
    sources [(tap, j)], tap)]); finish: dict(kind, x, seg, residual [taps], tap).  Segment (i, j, level) has the weights fuse_layers.i.j.level.0 / .1,
    BR[i] output channels and no ReLU if it is the chain's last (level == i - j - 1), else BR[j] channels and a ReLU."""
    out = []
    for j in range(nb - 1):
        for level in range(nb - 1 - j):
            members = [i for i in range(j + 1, nb) if level < i - j and not (i == nb - 1 and j == nb - 2)]
            if level == 0 and len(members) >= 2:
                out.append(dict(kind="down", x=f"x{j}", segs=[(i, j, 0) for i in members], taps=[f"d{i}.{j}.0" for i in members]))
                continue
            for i in members:
                out.append(dict(kind="down", x=f"x{j}" if level == 0 else f"d{i}.{j}.{level - 1}", segs=[(i, j, level)], taps=[f"d{i}.{j}.{level}"]))
    out.append(dict(kind="up", outputs=[dict(i=i, base=f"x{i}", extras=[f"d{i}.{j}.{chain_last(i, j)}" for j in range(i)],
                                             sources=[(f"x{j}", j) for j in range(i + 1, nb)], tap=f"y{i}") for i in range(nb - 1)]))
    i = nb - 1
    out.append(dict(kind="finish", x=f"x{i - 1}", seg=(i, i - 1, 0), residual=[f"x{i}"] + [f"d{i}.{j}.{chain_last(i, j)}" for j in range(i - 1)], tap=f"y{i}"))
    return out


def down_taps(nb):
    return [t for L in fuse_launches(nb) if L["kind"] == "down" for t in L["taps"]]


def seg_shape(seg):
    """(output channels, ReLU) of segment (i, j, level)"""
    i, j, level = seg
    last = level == chain_last(i, j)
    return (BR[i] if last else BR[j]), not last


def relu_mask(segs):
    return np.concatenate([np.full(seg_shape(s)[0], seg_shape(s)[1]) for s in segs])


def last_batchnorms(p="backbone."):
    """The 62 BatchNorms uneven_fuse_state_dict edits, as (key prefix, output branch i): fuse_layers.i.j.1 for j > i, fuse_layers.i.j.<i-j-1>.1 for j < i."""
    out = []
    for stage, m, nb in modules():
        for i in range(nb):
            for j in range(nb):
                if j != i:
                    out.append((f"{p}{stage}.{m}.fuse_layers.{i}.{j}." + ("1" if j > i else f"{chain_last(i, j)}.1"), i))
    return out


def term_scales(key):
    """BatchNorm prefix -> the scale of each of its output channels (float64): output_scales(C_i) x 10^-u[c], u drawn from DECADES with Philox(key),
    in the order of last_batchnorms()."""
    g = np.random.Generator(np.random.Philox(key=list(key)))
    return {bn: cc.output_scales(BR[i]) * 10.0 ** -g.choice(DECADES, BR[i]).astype(np.float64) for bn, i in last_batchnorms()}


def uneven_fuse_state_dict(sd, key):
    """A copy of `sd` in which the last BatchNorm of every fuse term has weight and bias multiplied per output channel by term_scales(key): never
    above 1, so no activation grows; channel 0 of every term -- the shift included -- is exactly 0; the quiet channels (1e-5 and below) are the first
    of the last 16-channel block and the last one, which in a merged launch is the channel right below relu_from."""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    for bn, s in term_scales(key).items():
        for f in (".weight", ".bias"):
            out[bn + f] = (widen(sd[bn + f]) * s).astype(np.float32)
    return out


SILENCE = -1e4                                     # added to a BatchNorm's bias: far below any activation of the forward (features peak near 25)


def silenced_channels(c):
    """The channels of a C-channel branch output that silent_branch_state_dict turns off: the first quiet channel and the 1e-3 one."""
    sp = cc.special_channels(c)
    return sp["quiet"][0], sp["mid"]


def last_block_batchnorms(p="backbone."):
    """(bn2 of the last BasicBlock of branch b, b) for every branch of every module: the launch that writes x_b"""
    return [(f"{p}{stage}.{m}.branches.{b}.3.bn2", b) for stage, m, nb in modules() for b in range(nb)]


def silent_branch_state_dict(sd):
    """A copy of `sd` in which x_b is exactly 0 on silenced_channels(C_b), for every branch of every module (the bias of the BatchNorm in front of
    the ReLU that writes x_b lowered by 1e4: nothing can grow).  The forward's own branch outputs are positive almost everywhere -- a residual
    chain of ReLUs -- so with uneven_fuse_state_dict alone an element of a quiet channel is still x_i plus something 1e5 x smaller, and a fault
    in the small terms stays below a rounding of x_i.  On a silenced channel every element of y_i IS its small terms.  The second quiet channel
    and the dead one keep the forward's own x_i."""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    for bn, b in last_block_batchnorms():
        out[bn + ".bias"][list(silenced_channels(BR[b]))] += np.float32(SILENCE)
    return out


class FuseWeights:
    """The folded float64 weights of the fuse layer under key prefix p ("backbone.stage4.0."): down((i, j, level)) -> (w (cout,cin,3,3), shift),
    up(i, j) -> (w (C_i, C_j), shift)."""

    def __init__(self, sd, p):
        self.sd, self.p = sd, p

    def _fold(self, q):
        return cc.fold_bn(self.sd[q + "0.weight"], *(self.sd[q + "1" + f] for f in BN_FIELDS))

    def down(self, seg):
        return self._fold(f"{self.p}fuse_layers.{seg[0]}.{seg[1]}.{seg[2]}.")

    def down_key(self, seg):
        return f"{self.p}fuse_layers.{seg[0]}.{seg[1]}.{seg[2]}.0.weight"

    def up(self, i, j):
        w, shift = self._fold(f"{self.p}fuse_layers.{i}.{j}.")
        return w[:, :, 0, 0], shift


# ----------------------------------------------------------------------------------------------------------------- the up launch
def nearest_up(t, s):
    return t if s == 1 else np.repeat(np.repeat(t, s, 2), s, 3)


def _pw64(x, w, shift, mag):
    x, w, shift = (np.abs(a) if mag else a for a in (widen(x), np.asarray(w, np.float64), np.asarray(shift, np.float64)))
    return np.einsum("oc,nchw->nohw", w, x) + shift[None, :, None, None]


def fuse_up_reference(base, extras, sources, relu=True, mag=False):
    """relu(base + sum extras + sum_j nearest_up(conv1x1(x_j; w64) + shift64)) in float64; mag: the same on absolute values, before the ReLU."""
    f = (lambda a: np.abs(widen(a))) if mag else widen
    y = f(base).copy()
    for e in extras:
        y += f(e)
    for x, w64, shift64, s in sources:
        y += nearest_up(_pw64(x, w64, shift64, mag), s)
    return y if mag or not relu else np.maximum(y, 0.0)


def fuse_up_fp32(base, extras, sources, relu=True):
    """name -> the two fp32 compositions.  "torch": the reference's order j = 0 .. nb-1 -- the chains, x_i, then each up term as torch's fp32 1x1
    convolution + its own shift.  "sequential": ((base + extras) + fl32(sum of the shifts)) + T_0 + T_1 + T_2, each T_j one strictly sequential
    fp32 chain over the input channels -- the order of hr_fuse_up_f32, whose biases are summed at load."""
    f32 = lambda a: np.asarray(a, np.float32)
    pw = lambda x, w64: f32(w64)[:, :, None, None]
    y = None
    for e in extras:
        y = f32(e) if y is None else y + f32(e)
    y = f32(base) if y is None else y + f32(base)
    for x, w64, shift64, s in sources:
        y = y + nearest_up(cc.torch_fp32(x, pw(x, w64)) + f32(shift64)[None, :, None, None], s)
    z = f32(base)
    for e in extras:
        z = z + f32(e)
    z = z + f32(sum(np.asarray(sh, np.float64) for _, _, sh, _ in sources))[None, :, None, None]
    for x, w64, _, s in sources:
        z = z + nearest_up(cc.sequential_fp32(x, pw(x, w64)), s)
    return {"torch": cc.apply_relu(y, bool(relu)), "sequential": cc.apply_relu(z, bool(relu))}


def fuse_up_check(got, base, extras, sources, relu=True):
    """One output of the grouped launch on its own tapped inputs; sources = [(x_j, w64_ij (C_i, C_j), shift64_ij, 2 ** (j - i)), ...].  An element
    of magnitude 0 must be exact (ratio()).  Returns (ratio, index, yardstick ratio, yardstick's name, accepted ratio) like forward_check."""
    ref, mag = fuse_up_reference(base, extras, sources, relu), fuse_up_reference(base, extras, sources, mag=True)
    y = max(ratio(v, ref, mag)[0] for v in fuse_up_fp32(base, extras, sources, relu).values())
    r, at = ratio(got, ref, mag)
    return r, at, y, "torch+sequential", accepted(y)


def where(index, i, nb, s_out=None):
    """Names the place of element (n, c, y, x) of output i of a module with nb branches: the channel's class (from s_out, the output_scales pattern of
    the uneven weights), the image border, a band seam of hr_fuse_up_f32 (the first row of a band of 8 >> i rows), a seam between two pixels of the
    coarsest source (2^(nb-1-i) output pixels each, rows or columns)."""
    _, c, y, x = index
    h, band, src = 56 >> i, max(8 >> i, 1), 1 << (nb - 1 - i)
    tags = []
    if y in (0, h - 1) or x in (0, h - 1):
        tags.append("border")
    if i < nb - 1 and band > 1 and y > 0 and y % band == 0:
        tags.append("band seam")
    if src > 1 and ((y > 0 and y % src == 0) or (x > 0 and x % src == 0)):
        tags.append("source seam")
    tags = tags or ["interior"]
    if s_out is not None:
        tags.insert(0, "dead-term channel" if s_out[c] == 0 else "quiet channel" if s_out[c] <= 1e-5 else "mid channel" if s_out[c] < 1 else "loud channel")
    return "+".join(tags)


# ----------------------------------------------------------------------------------------------------------------- a launch on its own taps
def check_launch(launch, weights, taps, frames=slice(None), family="direct"):
    """taps: name relative to the module -> (n,C,H,W) fp32.  Returns a list of (name, family, form text, got, result of the check, output branch)
    -- one entry, or one per output of the up launch."""
    T = lambda name: np.asarray(taps[name])[frames]
    if launch["kind"] == "up":
        out = []
        for o in launch["outputs"]:
            i = o["i"]
            sources = [(T(t), *weights.up(i, j), 1 << (j - i)) for t, j in o["sources"]]
            res = fuse_up_check(T(o["tap"]), T(o["base"]), [T(e) for e in o["extras"]], sources)
            out.append((o["tap"], "fuse", f"up{len(sources)}_add{len(o['extras'])}_relu", T(o["tap"]), res, i))
        return out
    if launch["kind"] == "down":
        segs, got = launch["segs"], np.concatenate([T(t) for t in launch["taps"]], 1)
        ws, shifts = zip(*(weights.down(s) for s in segs))
        mask = relu_mask(segs)
        relu = bool(mask[0]) if mask.all() or not mask.any() else mask
        res = cc.forward_check(family, got, T(launch["x"]), np.concatenate(ws), np.concatenate(shifts), 2, None, relu)
        form = "bias" + ("_relu" if relu is True else "" if relu is False else f"_relu_from{int(np.argmax(mask))}")
        return [("+".join(launch["taps"]), family, form, got, res, segs[0][0])]
    w64, shift = weights.down(launch["seg"])
    res = cc.forward_check(family, T(launch["tap"]), T(launch["x"]), w64, shift, 2, [T(r) for r in launch["residual"]], True)
    return [(launch["tap"], family, f"bias_relu_res{len(launch['residual'])}", T(launch["tap"]), res, launch["seg"][0])]


def fp32_taps(nb, weights, xs, up="torch"):
    """The whole layer as a plain fp32 composition on the branch outputs xs: every tap of fuse_launches(nb), name -> (n,C,H,W) fp32.  The
    convolutions are torch's, the epilogue conv_checks.epilogue, the up launch fuse_up_fp32[up]."""
    taps = {f"x{b}": np.asarray(x, np.float32) for b, x in enumerate(xs)}
    for L in fuse_launches(nb):
        if L["kind"] == "down":
            ws, shifts = zip(*(weights.down(s) for s in L["segs"]))
            lin = cc.torch_fp32(taps[L["x"]], np.concatenate(ws).astype(np.float32), 2)
            y, off = cc.epilogue(lin, np.concatenate(shifts).astype(np.float32), None, relu_mask(L["segs"])), 0
            for t, s in zip(L["taps"], L["segs"]):
                taps[t] = np.ascontiguousarray(y[:, off:off + seg_shape(s)[0]])
                off += seg_shape(s)[0]
        elif L["kind"] == "up":
            for o in L["outputs"]:
                sources = [(taps[t], *weights.up(o["i"], j), 1 << (j - o["i"])) for t, j in o["sources"]]
                taps[o["tap"]] = fuse_up_fp32(taps[o["base"]], [taps[e] for e in o["extras"]], sources)[up]
        else:
            w64, shift = weights.down(L["seg"])
            taps[L["tap"]] = cc.epilogue(cc.torch_fp32(taps[L["x"]], w64.astype(np.float32), 2), shift.astype(np.float32), [taps[r] for r in L["residual"]], True)
    return taps


def bounds_line(case, name, fam, form, res, place):
    r, at, y, yname, bar = res
    return (f"conv_bounds family={fam} case={case}:{name} data=forward form={form} gpu={r:.3f} at={at} where={place} "
            f"yardstick={yname}:{y:.3f} accepted={bar:.3f}")


# ----------------------------------------------------------------------------------------------------------------- planted faults
PLANTED_FAULTS = (
    "1 the 7x7 source's term of a quiet channel read one source row off, on the first row of a band (y = 8)",
    "2 the 28x28 source's whole term dropped on a quiet channel",
    "3 the 14x14 source's whole term dropped on a quiet channel",
    "4 the 7x7 source's whole term dropped on a quiet channel",
    "5 the 14x14 term of the other frame on a quiet channel",
    "6 1e-9 added in the channel whose every term is dead",
    "7 the channel just below relu_from ReLU'd",
    "8 the first channel at relu_from left linear",
    "9 one addend of the finishing convolution taken from the other frame, on a quiet channel",
    "10 a 1e-3 relative error of the up terms on the last column of the 1e-3 channel",
)
UP_FAULTS, MERGED_FAULTS, FINISH_FAULTS = PLANTED_FAULTS[:6] + PLANTED_FAULTS[9:], PLANTED_FAULTS[6:8], PLANTED_FAULTS[8:9]


def plant(name, out, **ctx):
    """A copy of the fp32 result `out` (n >= 2 frames) with fault `name` planted.  UP_FAULTS: out is output 0 of a 4-branch layer BEFORE its ReLU
    (the caller applies it) and ctx holds terms = the fp32 up terms at their own resolution, [(n,32,28,28), (n,32,14,14), (n,32,7,7)], shift
    included, and base = x_0 (fault 6 goes where it is 0: there the element has no term at all).  MERGED_FAULTS: out is the merged launch's
    result and ctx holds lin, the same without any ReLU, and relu_from.  FINISH_FAULTS: out is the finishing convolution before its ReLU and ctx
    holds addend, one of its addends."""
    k = int(name.split()[0])
    bad = np.array(out, np.float32)
    c_out = out.shape[1] if k not in (7, 8) else ctx["relu_from"]
    sp = cc.special_channels(c_out)
    q, mid, dead = ctx.get("quiet", sp["quiet"][1]), sp["mid"], sp["dead"]            # quiet=: the other quiet channel (silenced_channels)
    if k == 1:                                                 # rows 8 .. 15 read source row 1; the first of them takes row 0
        t = ctx["terms"][2]
        bad[:, q, 8] += np.repeat(t[:, q, 0] - t[:, q, 1], 8, -1)
    elif k in (2, 3, 4):
        bad[:, q] -= nearest_up(ctx["terms"][k - 2], 2 << (k - 2))[:, q]
    elif k == 5:
        t = nearest_up(ctx["terms"][1], 4)
        bad[0, q] += t[1, q] - t[0, q]
    elif k == 6:
        y, x = np.argwhere(np.asarray(ctx["base"])[0, dead] == 0)[0]
        bad[0, dead, y, x] += np.float32(1e-9)
    elif k == 7:
        bad[:, q] = np.maximum(bad[:, q], 0)
    elif k == 8:
        bad[:, c_out] = ctx["lin"][:, c_out]
    elif k == 9:
        bad[0, q] += ctx["addend"][1, q] - ctx["addend"][0, q]
    else:                                                       # on what the launch computes there, the up terms: x_0 itself is only passed through
        t = sum(nearest_up(t, 2 << s) for s, t in enumerate(ctx["terms"]))
        bad[:, mid, :, -1] += np.float32(1e-3) * t[:, mid, :, -1]
    return bad
