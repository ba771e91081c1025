"""Every launch of the fp32 forward on its OWN input, at the call sizes of the production jobs: 16 frames (the headline), 400 (batch_generation's
calls) and 50 (the remainder of a 1 250-frame shard) -- the method of tests/test_gpu_bf16_stages.py on the fp32 path, one launch deep.

Teacher forcing: each launch's reference is the float64 oracle (oracle.float64()) on the GPU's tapped fp32 input (and residual) of that launch
(grnet_debug_tensor), never on the oracle's previous stage, so the bar is the one of the per-kernel test of the family that runs it.  The call is 8
distinct frames tiled (frame k is frame k % 8): every copy of a frame must give the same bits in every tap and every output, and the references run
on the 8 distinct frames.  Before the checked forward the handle runs a forward of the same size on other frames, so a consumer that reads a buffer
before its producer has written it reads different numbers and fails.  Which kernel and launch form each size takes is asserted first
(grnet_conv_kernel_info, grnet_conv_launch_form), so that a plan change cannot quietly move a check onto another kernel.  At 16 frames every convolution launch is also held, element by element,
to the rule of tests/test_gpu_conv_elements.py on its own tapped input (Checker.conv; tests/helpers/conv_checks.py forward_check) -- the 42 launches
of the eight fuse layers included (Checker.fuse; tests/helpers/fuse_checks.py: the down chains are tapped as "<stage>.<m>.d<i>.<j>.<level>") -- and the
six bilinear launches likewise (Checker.bilinear); the attention pooling with the merge that finishes it is held on all 8 distinct frames to the rule of
tests/test_gpu_pool_elements.py on its tapped heat and feature maps (Checker.pool; tests/helpers/pool_checks.py)."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from .conftest import rel_err
from .helpers import conv_checks as cc
from .helpers import fuse_checks as fc
from .helpers import pool_checks as pc
from .helpers import smpl_checks as sc

pytestmark = pytest.mark.gpu

SIZES = [16, 50, 400]
BR = [32, 64, 128, 256]
MODULES = [("stage2", 0, 2)] + [("stage3", m, 3) for m in range(4)] + [("stage4", m, 4) for m in range(3)]
HEADS = [(2, 1, 1), (3, 2, 2), (4, 3, 3)]                        # upsample_stage_{idx}: layers, source branch (hrnet.py:440-453)
B = "backbone."
# the bars of the per-kernel tests of each family (rel_err: max |a - b| / max |b|)
BARS = {"direct": 1e-5, "stem": 1e-5, "pw": 1e-5, "bilinear": 1e-5,                 # test_conv_kernel, test_stem_..., test_pointwise_..., test_bilinear2x
        "wino4": 1e-4, "wino4w": 1e-4, "wino4s": 1e-4,                              # test_winograd_*, test_small_map_winograd_kernel
        "fuse": 2e-5,                                                               # test_fuse_layer_of_every_hr_module_matches_oracle
        "attn_pool": 1e-4,                                                          # test_gpu_bf16_stages.py
        "rotmat": 1e-5, "theta": 1e-4, "smpl": 1e-4}                                # test_head_pass_single_op_matches_reference_golden
TOL = 1e-4                                                                          # test_forward_matches_oracle_full
HINTS = [14, 7, 1071, 1072, 1041, 1042, 1171, 1141]                                 # grnet_tune's candidates besides the cost model (0)
OUTS = (("point_local_feat", (128, 24)), ("cam_shape_feats", (64, 24)), ("theta", (85,)), ("rotmat", (24, 3, 3)), ("verts", (6890, 3)),
        ("kp_3d", (29, 3)), ("kp_2d", (29, 2)))


def _module_inputs(stage, m, nb):
    first = {"stage2.0": ["transition1.0", "transition1.1"], "stage3.0": ["stage2.0.y0", "stage2.0.y1", "transition2.2"],
             "stage4.0": ["stage3.3.y0", "stage3.3.y1", "stage3.3.y2", "transition3.3"]}
    return first.get(f"{stage}.{m}") or [f"{stage}.{m - 1}.y{b}" for b in range(nb)]


def _block_io(stage, m, b, k, nb):
    """(input tap, conv1 tap, output tap) of BasicBlock k of branch b of an HR module; block 3's output is the module's x{b}."""
    tag = f"{stage}.{m}."
    x_in = _module_inputs(stage, m, nb)[b] if k == 0 else f"{tag}b{b}.{k - 1}"
    return x_in, f"{tag}b{b}.{k}.conv1", f"{tag}x{b}" if k == 3 else f"{tag}b{b}.{k}"


def _tap_names(direct_only=False):
    names = ["stem_conv1", "stem_conv2", "layer1.0.downsample"] + [f"layer1.{k}{s}" for k in range(4) for s in (".conv1", ".conv2", "")]
    names += ["transition1.0", "transition1.1", "transition2.2", "transition3.3"]
    for stage, m, nb in MODULES:
        for b in range(nb):
            if not direct_only:
                names += [f"{stage}.{m}.b{b}.{k}.conv1" for k in range(4)] + [f"{stage}.{m}.b{b}.{k}" for k in range(3)]
            names.append(f"{stage}.{m}.x{b}")
        names += [f"{stage}.{m}.{t}" for t in fc.down_taps(nb)]          # the down chains of the fuse layer: direct launches, a tap per slice
        names += [f"{stage}.{m}.y{i}" for i in range(nb)]
    if direct_only:
        return names + ["head.smpl_feats", "head.cam_shape"]
    for idx, layers, _ in HEADS:
        names += [f"up{idx}.{l}.{k}" for l in range(layers) for k in ("bilinear", "conv")]
    return names + ["cat", "head.first", "head.part_feats", "head.heat", "head.smpl_feats", "head.cam_shape"]


def _forward_taps(m, n, base, other, names):
    """One forward on `other` (stale numbers in every buffer), then the checked forward on `base` tiled to n frames.  Returns the taps and outputs of
    the 8 distinct frames (host, fp32) and the taps / outputs in which some copy of a frame does not have the first copy's bits (name -> rel. diff)."""
    idx = torch.arange(n, device="cuda") % 8
    tile = lambda a: torch.from_numpy(a).cuda()[idx].contiguous()
    extras = ("point_local_feat", "cam_shape_feats")
    m(tile(other), extras=extras)
    out = m(tile(base), extras=extras)[-1]
    torch.cuda.synchronize()
    return _collect(m, n, names, out)


def _collect(m, n, names, out):
    idx = torch.arange(n, device="cuda") % 8
    got, differ = {}, {}
    for name in names:
        t = m.debug_tensor(name, n)
        if not torch.equal(t, t[:8][idx]):                                    # a frame's result does not depend on its place in the call
            differ[name] = float((t - t[:8][idx]).abs().max() / t[:8].abs().max())
        got[name] = t[:8].cpu().numpy()
        del t
    for k, shape in OUTS:
        t = out[k].reshape(n, *shape)
        if not torch.equal(t, t[:8][idx]):
            differ[k] = float((t - t[:8][idx]).abs().max() / t[:8].abs().max())
        got[k] = t[:8].cpu().numpy()
    return got, differ


def _frames(pkg):
    return pkg.synth.make_frames(8), pkg.synth.make_frames(8, start=8)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _np(t):
    return t.numpy() if torch.is_tensor(t) else np.asarray(t)


def _forms_by_key(forms):
    """weight key of a launch's first segment -> (kernel name, launch form, tuning index)"""
    return {key: (name, form, ti) for (key, name), (_, form, ti) in zip(forms["kernels"], forms["forms"])}


def _seams(fam, form, h):
    """The image borders, and the rows / columns on both sides of every tile seam of the kernel that runs the layer: F(4x4,3x3)'s 4x4 tiles (+ the
    8-row workgroups of the 4- / 8-wave kernels on 28x28 maps), the small-map kernel's padded edge tiles (14 -> 16, 7 -> 8), the direct kernel's row
    tiles (rows per tile from the launch form)."""
    sl = [np.s_[:, :, 0], np.s_[:, :, -1], np.s_[:, :, :, 0], np.s_[:, :, :, -1]]
    pairs = lambda step: sorted({r for k in range(step, h, step) for r in (k - 1, k)})
    steps = []
    if fam in ("wino4", "wino4w", "wino4s"):
        steps.append(4)
        if h == 28:
            steps.append(8)
        if fam == "wino4s":
            edge = list(range(h // 4 * 4, h))                                    # the last tile row / column: partly outside the map
            sl += [np.s_[:, :, edge], np.s_[:, :, :, edge]]
    elif fam == "direct" and 0 < form.get("rows", 0) < h:
        steps.append(form["rows"])
    for st in steps:
        rows = pairs(st)
        if rows:
            sl += [np.s_[:, :, rows], np.s_[:, :, :, rows]]
    return sl


class Checker:
    """elements > 0 (with the state dict): conv() also takes the per-element ratio of the launch on the first `elements` distinct frames of its own
    tapped input (tests/helpers/conv_checks.py forward_check), given `own` = dict(x, bn | bias, stride, relu, residual, keys, bns)."""

    def __init__(self, by_key, sd=None, elements=0):
        self.by_key, self.worst, self.sd, self.elements = by_key, {}, sd, elements

    def __call__(self, fam, name, g, r, form=None):
        r = _np(r)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        bar = BARS[fam]
        e = rel_err(g, r)
        self.worst[fam] = max(self.worst.get(fam, 0.0), e / bar)
        assert e <= bar, (name, fam, e, bar)
        if g.ndim == 4:
            for sl in _seams(fam, form or {}, g.shape[2]):
                es = rel_err(g[sl], r[sl])
                self.worst[fam] = max(self.worst[fam], es / bar)
                assert es <= bar, (name, fam, "border / seam", sl, es, bar)

    def conv(self, key, name, g, r, own=None):
        _, form, _ = self.by_key[key]
        self(form["family"], name, g, r, form)
        if self.elements and own is not None:
            self._elements(key, name, g, form, **own)

    def _elements(self, key, name, g, form, x, bn=None, bias=None, stride=1, relu=False, residual=None, keys=None, bns=None):
        """|got - float64| per element in roundings of the element's magnitude, from |x|, |BatchNorm-folded weights|, |shift|, |residual|; the bar
        is the family's yardstick on the same tapped input (FACTOR x its ratio, at least FACTOR).  keys / bns: the layers one launch computes."""
        sd, f, fam = self.sd, slice(0, self.elements), form["family"]
        ws, shifts = [], []
        for k, b in zip(keys or [key], bns or [bn]):
            if b is not None:
                w64, sh = cc.fold_bn(sd[k], *(sd[b + s] for s in (".weight", ".bias", ".running_mean", ".running_var")))
            else:
                w64, sh = cc.widen(sd[k]), cc.widen(sd[bias]) if bias else np.zeros(len(sd[k]))
            ws.append(w64)
            shifts.append(sh)
        res = None if residual is None else _np(residual)[f]
        ratio, at, y, yname, bar = cc.forward_check(fam, g[f], _np(x)[f], np.concatenate(ws), np.concatenate(shifts), stride, res, relu)
        print(f"conv_bounds family={fam} case=forward16:{name} data=forward form={'bias' + '_relu' * relu + '_res' * (res is not None)} gpu={ratio:.3f} "
              f"at={at} where={cc.where(at, fam, form, g.shape[2])} yardstick={yname}:{y:.3f} accepted={bar:.3f}")
        k = fam + " elements"
        self.worst[k] = max(self.worst.get(k, 0.0), ratio / bar)
        assert ratio <= bar, (name, fam, ratio, at, bar)

    def bilinear(self, name, g, r, x):
        self("bilinear", name, g, r)
        if self.elements:
            f = slice(0, self.elements)
            res = cc.bilinear_check(g[f], _np(x)[f])
            print(fc.bounds_line("forward16", name, "bilinear", "linear", res, cc.where(res[1], "bilinear", {}, g.shape[2])))
            self._hold("bilinear", name, res)

    def fuse(self, tag, nb, got):
        """Every launch of the fuse layer of module `tag` on its own tapped inputs, per element: the down chains' stride-2 convolutions (a merged
        first link as ONE convolution with a ReLU per segment), every output of the grouped launch (fuse_checks.fuse_up_check), and the finishing
        convolution with its addends.  Measured and printed first, asserted at the end."""
        w, f = fc.FuseWeights(self.sd, f"{B}{tag}."), slice(0, self.elements)
        taps = {t: got[f"{tag}.{t}"] for t in [f"x{b}" for b in range(nb)] + [f"y{b}" for b in range(nb)] + fc.down_taps(nb)}
        held = []
        for L in fc.fuse_launches(nb):
            form = {} if L["kind"] == "up" else self.by_key[w.down_key(L["segs"][0] if L["kind"] == "down" else L["seg"])][1]
            for name, fam, text, g, res, i in fc.check_launch(L, w, taps, f, form.get("family", "fuse")):
                place = fc.where(res[1], i, nb) if L["kind"] == "up" else cc.where(res[1], fam, form, g.shape[2])
                print(fc.bounds_line("forward16", f"{tag}.{name}", fam, text, res, place))
                held.append((fam if L["kind"] != "finish" else fam + " finish", f"{tag}.{name}", res))
        for fam, name, res in held:
            self._hold(fam, name, res)

    def pool(self, got):
        """head.heat / head.smpl_feats / head.cam_shape -> point_local_feat / cam_shape_feats on the 8 distinct frames, per element: within
        max(4, 4 x yardstick) roundings of the element's magnitude of the float64 pooling of the tapped maps.  Printed first, asserted at the end."""
        case = pc.tapped_case(got["head.heat"], got["head.smpl_feats"], got["head.cam_shape"])
        res = pc.check("f32", case, {k: got[k] for k in pc.OUTPUTS})
        for output, r, yard, accepted, place in res:
            print(pc.bounds_line("f32", "forward16", case["n"], output, r, yard, accepted, place))
        for output, (ratio, at), yard, accepted, _ in res:
            self.worst["attn_pool elements"] = max(self.worst.get("attn_pool elements", 0.0), ratio / accepted)
            assert accepted <= pc.FACTOR * pc.YARD_CEILING["f32"] and ratio <= accepted, (output, ratio, at, yard, accepted)

    def _hold(self, fam, name, res):
        ratio, at, _, _, bar = res
        k = fam + " elements"
        self.worst[k] = max(self.worst.get(k, 0.0), ratio / bar)
        assert ratio <= bar, (name, fam, ratio, at, bar)


def _check_direct_stages(ck, oracle, sd, got, base):
    """The stages that hold a direct-kernel launch: stem_conv2, layer1's convolutions, the transitions, the fuse layers and head.cam_shape."""
    T = lambda name: _t(got[name])
    with oracle.float64():
        ck.conv(B + "conv2.weight", "stem_conv2", got["stem_conv2"], oracle.conv_bn(T("stem_conv1"), sd, B + "conv2.weight", B + "bn2", stride=2, relu=True),
                own=dict(x=got["stem_conv1"], bn=B + "bn2", stride=2, relu=True))
        q = B + "layer1.0."
        ck.conv(q + "downsample.0.weight", "layer1.0.downsample", got["layer1.0.downsample"],
                oracle.conv_bn(T("stem_conv2"), sd, q + "downsample.0.weight", q + "downsample.1"), own=dict(x=got["stem_conv2"], bn=q + "downsample.1"))
        for k in range(4):
            q, x_in = f"{B}layer1.{k}.", "stem_conv2" if k == 0 else f"layer1.{k - 1}"
            res = T("layer1.0.downsample") if k == 0 else T(x_in)
            ck.conv(q + "conv1.weight", f"layer1.{k}.conv1", got[f"layer1.{k}.conv1"], oracle.conv_bn(T(x_in), sd, q + "conv1.weight", q + "bn1", relu=True),
                    own=dict(x=got[x_in], bn=q + "bn1", relu=True))
            ck.conv(q + "conv2.weight", f"layer1.{k}.conv2", got[f"layer1.{k}.conv2"],
                    oracle.conv_bn(T(f"layer1.{k}.conv1"), sd, q + "conv2.weight", q + "bn2", relu=True), own=dict(x=got[f"layer1.{k}.conv1"], bn=q + "bn2", relu=True))
            ck.conv(q + "conv3.weight", f"layer1.{k}", got[f"layer1.{k}"],
                    oracle.conv_bn(T(f"layer1.{k}.conv2"), sd, q + "conv3.weight", q + "bn3", relu=True, residual=res),
                    own=dict(x=got[f"layer1.{k}.conv2"], bn=q + "bn3", relu=True, residual=res))
        for name, src, stride in (("transition1.0", "layer1.3", 1), ("transition1.1", "layer1.3", 2), ("transition2.2", "stage2.0.y1", 2),
                                  ("transition3.3", "stage3.3.y2", 2)):
            w = B + name + (".0.weight" if name == "transition1.0" else ".0.0.weight")
            ck.conv(w, name, got[name], oracle.conv_bn(T(src), sd, w, w[:-len("0.weight")] + "1", stride=stride, relu=True),
                    own=dict(x=got[src], bn=w[:-len("0.weight")] + "1", stride=stride, relu=True))
        for stage, mi, nb in MODULES:
            tag = f"{stage}.{mi}"
            ys = oracle.hr_fuse([T(f"{tag}.x{b}") for b in range(nb)], sd, f"{B}{tag}.")
            for i in range(nb):
                ck("fuse", f"{tag}.y{i}", got[f"{tag}.y{i}"], ys[i])
            if ck.elements:
                ck.fuse(tag, nb, got)
        hd = "head."
        ck.conv(hd + "smpl_final_layer.weight", "head.cam_shape", got["head.cam_shape"],
                oracle.conv2d(T("head.smpl_feats"), sd[hd + "smpl_final_layer.weight"], bias=sd[hd + "smpl_final_layer.bias"]),
                own=dict(x=got["head.smpl_feats"], bias=hd + "smpl_final_layer.bias"))


def _check_all_stages(ck, oracle, sd, smpl, got, base):
    T = lambda name: _t(got[name])
    _check_direct_stages(ck, oracle, sd, got, base)
    with oracle.float64():
        ck.conv(B + "conv1.weight", "stem_conv1", got["stem_conv1"], oracle.conv_bn(_t(base), sd, B + "conv1.weight", B + "bn1", stride=2, relu=True),
                own=dict(x=base, bn=B + "bn1", stride=2, relu=True))
        # the four BasicBlocks of every branch: each convolution from its own tapped input (and the block's tapped input as the residual)
        for stage, mi, nb in MODULES:
            for b in range(nb):
                for k in range(4):
                    x_in, c1, out = _block_io(stage, mi, b, k, nb)
                    q = f"{B}{stage}.{mi}.branches.{b}.{k}."
                    ck.conv(q + "conv1.weight", c1, got[c1], oracle.conv_bn(T(x_in), sd, q + "conv1.weight", q + "bn1", relu=True),
                            own=dict(x=got[x_in], bn=q + "bn1", relu=True))
                    ck.conv(q + "conv2.weight", out, got[out], oracle.conv_bn(T(c1), sd, q + "conv2.weight", q + "bn2", relu=True, residual=T(x_in)),
                            own=dict(x=got[c1], bn=q + "bn2", relu=True, residual=got[x_in]))
        # upsample heads: bilinear x2 from the previous tap, the 3x3 from the bilinear tap
        for idx, layers, br in HEADS:
            prev = f"stage4.2.y{br}"
            for l in range(layers):
                nm, q = f"up{idx}.{l}", f"{B}upsample_stage_{idx}."
                ck.bilinear(nm + ".bilinear", got[nm + ".bilinear"], oracle.upsample_bilinear2x(T(prev)), got[prev])
                ck.conv(q + f"{4 * l + 1}.weight", nm + ".conv", got[nm + ".conv"],
                        oracle.conv_bn(T(nm + ".bilinear"), sd, q + f"{4 * l + 1}.weight", q + f"{4 * l + 2}", relu=True),
                        own=dict(x=got[nm + ".bilinear"], bn=q + f"{4 * l + 2}", relu=True))
                prev = nm + ".conv"
        # cat: the four slices ARE the taps (stage4.2's y0 is written into it, the heads' last convolutions too)
        parts = ["stage4.2.y0", "up2.0.conv", "up3.1.conv", "up4.2.conv"]
        assert np.array_equal(got["cat"], np.concatenate([got[p] for p in parts], 1))
        # PARE head (pare.py:305-336): the two 480 -> 128 first convolutions as one launch, the second ones from its halves, the 1x1 heat map
        hd = "head."
        ref_first = np.concatenate([_np(oracle.conv_bn(T("cat"), sd, hd + f"{b}.0.weight", hd + f"{b}.1", relu=True))
                                    for b in ("keypoint_deconv_layers", "smpl_deconv_layers")], 1)
        ck.conv(hd + "keypoint_deconv_layers.0.weight", "head.first", got["head.first"], ref_first,
                own=dict(x=got["cat"], relu=True, keys=[hd + f"{b}.0.weight" for b in ("keypoint_deconv_layers", "smpl_deconv_layers")],
                         bns=[hd + f"{b}.1" for b in ("keypoint_deconv_layers", "smpl_deconv_layers")]))
        ck.conv(hd + "keypoint_deconv_layers.3.weight", "head.part_feats", got["head.part_feats"],
                oracle.conv_bn(_t(got["head.first"][:, :128]), sd, hd + "keypoint_deconv_layers.3.weight", hd + "keypoint_deconv_layers.4", relu=True),
                own=dict(x=got["head.first"][:, :128], bn=hd + "keypoint_deconv_layers.4", relu=True))
        ck.conv(hd + "smpl_deconv_layers.3.weight", "head.smpl_feats", got["head.smpl_feats"],
                oracle.conv_bn(_t(got["head.first"][:, 128:]), sd, hd + "smpl_deconv_layers.3.weight", hd + "smpl_deconv_layers.4", relu=True),
                own=dict(x=got["head.first"][:, 128:], bn=hd + "smpl_deconv_layers.4", relu=True))
        ck.conv(hd + "keypoint_final_layer.weight", "head.heat", got["head.heat"],
                oracle.conv2d(T("head.part_feats"), sd[hd + "keypoint_final_layer.weight"], bias=sd[hd + "keypoint_final_layer.bias"]),
                own=dict(x=got["head.part_feats"], bias=hd + "keypoint_final_layer.bias"))
        # attention pooling from the tapped heat / feature maps
        attn = got["head.heat"][:, 1:]
        for k, feat in (("point_local_feat", "head.smpl_feats"), ("cam_shape_feats", "head.cam_shape")):
            ck("attn_pool", k, got[k], oracle.keypoint_attention(got[feat], attn).reshape(got[k].shape))
        if ck.elements:
            ck.pool(got)
        # the tail from the GPU's pooled features
        rot6d, shape, cam = oracle.head_tail(got["point_local_feat"], got["cam_shape_feats"], sd)
    rotmat = oracle.rot6d_to_rotmat(rot6d).reshape(-1, 24, 3, 3)
    aa = oracle.rotmat_to_aa(rotmat.reshape(-1, 3, 3)).reshape(-1, 72)
    ck("rotmat", "rotmat", got["rotmat"], rotmat)
    ck("theta", "theta", got["theta"], np.concatenate([cam, aa, shape], 1))
    # SMPL and the projection from the GPU's own theta / rotmat, in float64
    betas, cam = got["theta"][:, 75:], got["theta"][:, :3]
    with oracle.float64():
        verts, j24 = oracle.smpl_lbs(betas, got["rotmat"], smpl)
        kp3d = oracle.smpl_joints29(verts, j24, smpl)
        kp2d = oracle.project(kp3d, cam)
    assert verts.dtype == kp3d.dtype == kp2d.dtype == np.float64
    ck("smpl", "verts", got["verts"], verts)
    ck("smpl", "kp_3d", got["kp_3d"], kp3d)
    ck("smpl", "kp_2d", got["kp_2d"], kp2d)
    # ... and element by element, in roundings of each element's magnitude (tests/helpers/smpl_checks.py; the rule of tests/test_gpu_smpl.py:
    # up to 4 x what the fp32 oracle reaches on the same inputs, never below 4)
    case = {"betas": betas, "rotmat": got["rotmat"], "cam": cam}
    ref = sc.smpl_reference(betas, got["rotmat"], cam, smpl)
    assert sc.min_abs_depth(ref, cam) >= 1.0
    mag = sc.smpl_magnitude(betas, got["rotmat"], cam, smpl, ref)
    mine = {k: got[k] for k in ("verts", "kp_3d", "kp_2d")}
    orc = sc.ratios({k: v for k, v in sc.fp32_oracle(oracle, case, smpl).items() if k in mine}, ref, mag)
    r, bar = sc.ratios(mine, ref, mag), sc.bars(orc)
    for k in mine:
        print(f"smpl_bounds forward frames={len(betas)} (distinct) output={k} gpu={r[k][0]:.3f} at={r[k][1]} oracle={orc[k][0]:.3f} accepted={bar[k]:.3f}")
        ck.worst["smpl elements"] = max(ck.worst.get("smpl elements", 0.0), r[k][0] / bar[k])
        assert r[k][0] <= bar[k], (k, r[k], bar[k])


_REF = {}


def _end_to_end(oracle, sd, smpl, got, base):
    if "ref" not in _REF:
        _REF["ref"] = oracle.grnet_forward(base, sd, smpl)
    for k in ("theta", "rotmat", "verts", "kp_3d", "kp_2d"):
        r = np.asarray(_REF["ref"][k]).reshape(got[k].shape)
        assert rel_err(got[k], r) < TOL, (k, rel_err(got[k], r))


def _run(pkg, n, names, table=None):
    m = pkg.build_synthetic_model(max_frames=n, with_gru=False)
    try:
        if table is not None:
            table(m)
        forms = {"kernels": m.conv_kernels(n), "forms": m.conv_launch_forms(n)}
        base, other = _frames(pkg)
        got, differ = _forward_taps(m, n, base, other, names)
    finally:
        m.close()
    return forms, got, differ, base


# The launch forms each size was chosen for, as grnet_conv_launch_form reports them on the MI355X (256 CUs; the split last round depends on it):
XCD_64_56 = {16: 1, 50: 0, 400: 1}              # XCD-aware order on layer1's 64 -> 64 @56 (224 / 700 / 5 600 tiles)
PARTIAL_7 = {16: 0, 50: 1, 400: 0}              # a partial last row tile (4 images) on every conv_wino4s_f32<7,256> launch
SPLIT = {16: set(), 50: {B + "upsample_stage_4.5.weight"}, 400: {B + "upsample_stage_3.1.weight"}}   # 800 = 3 x 256 + 32, 3 200 = 12 x 256 + 128 workgroups


def _assert_forms(n, by_key):
    """The kernels and launch forms each size was chosen for (grnet_conv_kernel_info names, grnet_conv_launch_form fields)."""
    name = lambda key: by_key[key][0]
    form = lambda key: by_key[key][1]
    for stage, mi, nb in MODULES:                                   # the fuse layers: direct stride-2 convolutions and one grouped launch each
        w = fc.FuseWeights(None, f"{B}{stage}.{mi}.")
        for L in fc.fuse_launches(nb):
            if L["kind"] == "up":
                assert form(f"{B}{stage}.{mi}.fuse_layers(up)")["family"] == "fuse_up", (stage, mi)
                continue
            key = w.down_key(L["segs"][0] if L["kind"] == "down" else L["seg"])
            assert name(key) == "conv_direct_f32 3x3 s2" and form(key)["family"] == "direct", (key, name(key), form(key))
    for stage, mi, nb in MODULES:
        for b in range(nb):
            c, w = BR[b], 56 >> b
            for k in range(4):
                for j in (1, 2):
                    nm = name(f"{B}{stage}.{mi}.branches.{b}.{k}.conv{j}.weight")
                    if w >= 28:
                        assert nm.startswith("conv_wino4_f32<"), (stage, mi, b, k, nm)
                    else:
                        assert nm == f"conv_wino4s_f32<{w},{c}>", (stage, mi, b, k, nm)
                        ipw = form(f"{B}{stage}.{mi}.branches.{b}.{k}.conv{j}.weight")
                        assert ipw["images_per_tile"] == (4 if w == 7 else 1) and ipw["partial"] == (PARTIAL_7[n] if w == 7 else 0), ipw
    assert name(B + "conv1.weight") == "conv_stem_f32"
    assert name(B + "conv2.weight") == "conv_direct_f32 3x3 s2"
    assert name(B + "layer1.0.conv3.weight") == name(B + "layer1.0.downsample.0.weight") == "conv_pw_f32<64>"
    for k in range(4):
        f2 = form(f"{B}layer1.{k}.conv2.weight")
        assert f2["family"] == "wino4" and f2["xcd"] == XCD_64_56[n], f2
        assert name(f"{B}layer1.{k}.conv1.weight") == "conv_direct_f32 1x1 s1"
    assert name(B + "transition1.1.0.0.weight") == name(B + "transition2.2.0.0.weight") == name(B + "transition3.3.0.0.weight") == "conv_direct_f32 3x3 s2"
    assert name("head.smpl_final_layer.weight") == "conv_direct_f32 1x1 s1" and name("head.keypoint_final_layer.weight") == "conv_pw_f32<128>"
    assert form("head.keypoint_deconv_layers.0.weight")["family"] == "wino4w"
    split = {key for key, (_, f, _) in by_key.items() if f.get("split")}
    assert split == SPLIT[n], (split, "CUs:", torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("n", SIZES)
def test_every_fp32_launch_matches_float64_oracle_on_its_own_input(pkg, oracle, synth_weights, synth_smpl, n):
    """(a) the kernel families and launch forms of the size; (b) every convolution launch outside the fuse layers, every fuse layer, the bilinear
    upsamplings and `cat` on their own tapped inputs -- at 16 frames also every launch INSIDE the fuse layers (down chains, grouped launch, finishing
    convolution: Checker.fuse) and the bilinear launches per element; (c) attention pooling, the tail and SMPL from the GPU's own inputs; (d) the 8 distinct frames'
    outputs against oracle.grnet_forward.  Borders and tile seams separately, each slice at the bar of its family."""
    forms, got, differ, base = _run(pkg, n, _tap_names())
    assert not differ, f"copies of a frame differ at {n} frames: {differ}"
    by_key = _forms_by_key(forms)
    _assert_forms(n, by_key)
    ck = Checker(by_key, synth_weights, elements=2 if n == 16 else 0)       # the first two of the eight distinct frames, every convolution launch
    _check_all_stages(ck, oracle, synth_weights, synth_smpl, got, base)
    _end_to_end(oracle, synth_weights, synth_smpl, got, base)
    print(f"n={n} worst err / bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ck.worst.items())))


def _hint_table(pkg, m, n, h):
    """A measured table (mode 5: table, eager launches) that puts hint h on every direct launch the launch-form report accepts it for, 0 elsewhere."""
    direct = [ti for _, form, ti in m.conv_launch_forms(n) if form["family"] == "direct"]
    text = lambda idxs: ("mode 5\n" + "".join(f"{i} {h}\n" for i in idxs)).encode()
    assert m._lib.grnet_set_tuning(m._h, n, text(direct)) == 0
    ok = []
    for pos in range(len(m.describe_convs())):
        try:
            form, ti = m.conv_launch_form(pos, n)
        except pkg._lib.GrnetError as e:
            assert "code -22" in str(e), e
            continue
        if form["family"] == "direct":
            ok.append(ti)
    assert m._lib.grnet_set_tuning(m._h, n, ("mode 5\n" + "".join(f"{i} {h if i in ok else 0}\n" for i in direct)).encode()) == 0


def _hint_config(h):
    """the configuration a tile hint names (csrc/conv_kernels.hip conv_choose): (split-K, pixel tile, channel tile, waves)"""
    if h in (7, 14):
        return 0, 16 * h, None, None
    code = h - 1000
    return 1, 16 * ((code % 100) // 10), 16 * (code % 10), 8 if code >= 100 else 4


@pytest.mark.parametrize("n", [400, 16])
def test_every_tuner_candidate_on_the_direct_launches(pkg, oracle, synth_weights, synth_smpl, n):
    """grnet_tune may put any valid candidate on any direct layer.  For each hint: a table with it on every direct launch it is valid for, then the
    stale and the checked forward, and every stage that holds a direct launch re-checked on its own inputs, plus the end-to-end outputs."""
    worst = {}
    for h in HINTS:
        forms, got, differ, base = _run(pkg, n, _tap_names(direct_only=True), table=lambda m: _hint_table(pkg, m, n, h))
        assert not differ, (h, differ)
        split_k, pt, ct, waves = _hint_config(h)
        ran = [f for _, f, _ in forms["forms"] if f["family"] == "direct" and f["hint"] == h]
        assert ran, f"hint {h} ran on no layer at {n} frames"
        # the report names h's configuration there (hint 14 falls back to the 7-tile where a 224-pixel tile does not fit: not on every layer)
        named = [f for f in ran if f["split_k"] == split_k and f["pixel_tile"] == pt and ct in (None, f["channel_tile"]) and waves in (None, f["waves"])]
        assert named, (h, ran)
        ck = Checker(_forms_by_key(forms))
        _check_direct_stages(ck, oracle, synth_weights, got, base)
        _end_to_end(oracle, synth_weights, synth_smpl, got, base)
        for k, v in ck.worst.items():
            worst[k] = max(worst.get(k, 0.0), v)
        print(f"n={n} hint {h}: on {len(ran)} launches ({len(named)} in its own configuration)")
    print(f"n={n} tuner candidates, worst err / bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_graph_replay_equals_eager_tap_for_tap(pkg):
    """The 16-frame forward replayed from a captured hipGraph (GRNET_OPT_USE_GRAPH) equals the eager lane streams in every tap and output, bit for
    bit (only digests of the eager run are kept).  A graph is keyed by the call's frame and output pointers and captured the second time its key
    is seen (grnet_run.cpp forward), so the graph calls go through grnet_forward with ONE frames buffer and ONE set of output buffers: other frames
    (first sight: eager), the checked frames (captured, then replayed), other frames (replay), the checked frames again -- a replay."""
    n = 16
    digest = lambda got: {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in got.items()}
    _, eager, differ, _ = _run(pkg, n, _tap_names())
    assert not differ
    eager = digest(eager)
    m = pkg.build_synthetic_model(max_frames=n, with_gru=False)
    try:
        m.set_option(pkg._lib.OPT_USE_GRAPH, 1)
        base, other = _frames(pkg)
        idx = torch.arange(n, device="cuda") % 8
        x = torch.empty(n, 3, 224, 224, device="cuda")
        out = {k: torch.empty(n, *shape, device="cuda") for k, shape in OUTS}
        o = pkg._lib.Outputs()
        for k, t in out.items():
            setattr(o, k, t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for frames in (other, base, other, base):
            x.copy_(torch.from_numpy(frames).cuda()[idx])
            pkg._lib.check(m._lib, m._h, m._lib.grnet_forward(m._h, C.c_void_p(x.data_ptr()), n, C.byref(o), stream), "grnet_forward")
        torch.cuda.synchronize()
        replay, differ = _collect(m, n, _tap_names(), out)
    finally:
        m.close()
    assert not differ
    assert digest(replay) == eager


def test_debug_tensor_on_fp32_handles_refuses_frames_it_does_not_hold(pkg):
    """grnet_debug_tensor on an fp32 handle reads only what the last forward wrote: n_frames outside [1, last call's frames] is refused before any
    copy, as on bf16 handles; the per-convolution taps exist and follow the last call.  grnet_conv_launch_form reports fp32 handles only, and the
    bf16 chain launches still refuse the taps they keep on chip."""
    m = pkg.build_synthetic_model(max_frames=16, with_gru=False)
    try:
        frames = torch.from_numpy(np.tile(pkg.synth.make_frames(8), (2, 1, 1, 1))).cuda()
        m(frames[:8])
        torch.cuda.synchronize()
        assert m.debug_tensor("stage4.2.b3.0.conv1", 8).shape == (8, 256, 7, 7)
        assert m.debug_tensor("layer1.0.downsample", 8).shape == (8, 256, 56, 56)
        # the down chains of the fuse layers, a merged first link slice by slice
        assert m.debug_tensor("stage4.0.d3.0.2", 8).shape == (8, 256, 7, 7) and m.debug_tensor("stage3.1.d1.0.0", 8).shape == (8, 64, 28, 28)
        assert m.debug_tensor("stage4.1.d3.1.0", 8).shape == (8, 64, 14, 14)
        with pytest.raises(pkg._lib.GrnetError, match="code -22.*unknown debug tensor"):
            m.debug_tensor("stage2.0.d1.0.0", 8)                                 # output 1 of a 2-branch layer is the finishing convolution alone
        for bad in (0, 9):
            with pytest.raises(pkg._lib.GrnetError, match="code -22"):
                m.debug_tensor("layer1.2.conv2", bad)
        m(frames)
        torch.cuda.synchronize()
        whole = m.debug_tensor("stage3.1.b2.1", 16)
        assert torch.equal(whole[8:], whole[:8]) and torch.equal(m.debug_tensor("stage3.1.b2.1", 8), whole[:8])
        with pytest.raises(pkg._lib.GrnetError, match="code -22"):
            m.debug_tensor("stem_conv1", 17)
    finally:
        m.close()
    m = pkg.build_synthetic_model(max_frames=64, with_gru=False, dtype="bf16")
    try:
        with pytest.raises(pkg._lib.GrnetError, match="code -1:"):
            m.conv_launch_form(0, 64)
        m(torch.from_numpy(np.tile(pkg.synth.make_frames(8), (8, 1, 1, 1))).cuda())
        torch.cuda.synchronize()
        for name in ("stage3.0.b1.0.conv1", "stage3.0.b1.2", "layer1.1.conv1"):
            with pytest.raises(pkg._lib.GrnetError, match="code -1:.*not written"):
                m.debug_tensor(name, 64)
        assert m.debug_tensor("stage3.0.x1", 64).shape == (64, 64, 28, 28)
        for name in ("stage4.0.d3.0.2", "stage3.1.d1.0.0"):                      # taps of the fp32 plan only: unknown names here
            with pytest.raises(pkg._lib.GrnetError, match="code -22.*unknown debug tensor"):
                m.debug_tensor(name, 64)
    finally:
        m.close()
