"""Every stage of the bf16 forward after layer1, on its OWN input, at the call sizes that select the production kernels (64 / 65 / 256 frames: BasicBlock
chains incl. the 7x7 frame pairs and the 56x56 pipeline, stride-2 row walks and bands, the wide / ring kernels writing into the 480-channel `cat` buffer,
the 1x1 stream kernel, the bf16 attention pooling) -- the method of tests/test_gpu_bf16_roll.py extended past layer1.

Teacher forcing: each stage's reference is the fp32 oracle under oracle.bf16_storage() evaluated on the GPU's tapped input of that stage (grnet_debug_tensor),
never on the oracle's previous stage, so the bar is the one of a single launch: rounding ties (the two helpers below, shared with the per-launch tests).
The call is 8 distinct frames tiled (frame k is frame k % 8, the odd call's tail included): every copy must give the same bits in every tap, and the oracle
runs on the 8 distinct frames.  Before the checked forward the handle runs a forward of the same size on other frames, so a consumer that reads a buffer
before its producer has written it reads different numbers and fails."""
import numpy as np
import pytest
import torch

from .conftest import rel_err
from .helpers import pool_checks as pc
from .test_gpu_bf16_roll import _close_up_to_ties, _rb
from .test_gpu_conv_bf16 import _close_up_to_rounding_ties

pytestmark = pytest.mark.gpu

SIZES = [64, 65, 256]
BR = [32, 64, 128, 256]
MODULES = [("stage2", 0, 2)] + [("stage3", m, 3) for m in range(4)] + [("stage4", m, 4) for m in range(3)]
HEADS = [(2, 1, 1), (3, 2, 2), (4, 3, 3)]                        # upsample_stage_{idx}: layers, source branch (hrnet.py:440-453)
B = "backbone."


def _tap_names():
    names = ["layer1", "transition1.0", "transition1.1", "transition2.2", "transition3.3"]
    for stage, m, nb in MODULES:
        names += [f"{stage}.{m}.x{b}" for b in range(nb)] + [f"{stage}.{m}.y{i}" for i in range(nb)]
    for idx, layers, _ in HEADS:
        names += [f"up{idx}.{l}.{k}" for l in range(layers) for k in ("bilinear", "conv")]
    return names + ["cat", "head.first", "head.part_feats", "head.heat", "head.smpl_feats", "head.cam_shape"]


def _forward_taps(m, n, base, other):
    """One forward on `other` (stale numbers in every buffer), then the checked forward on `base` tiled to n frames.  Returns the taps and outputs of the
    8 distinct frames, after checking that every copy of a frame has the same bits."""
    idx = torch.arange(n, device="cuda") % 8
    tile = lambda a: torch.from_numpy(a).cuda()[idx].contiguous()
    extras = ("point_local_feat", "cam_shape_feats")
    m(tile(other), extras=extras)
    out = m(tile(base), extras=extras)[-1]
    torch.cuda.synchronize()
    got = {}
    for name in _tap_names():
        t = m.debug_tensor(name, n)
        assert torch.equal(t, t[:8][idx]), name                                   # a frame's result does not depend on its place in the call
        got[name] = t[:8].cpu().numpy()
        assert np.array_equal(got[name], _rb(got[name])), name                    # stored as bf16
    for k, shape in (("point_local_feat", (128, 24)), ("cam_shape_feats", (64, 24)), ("theta", (85,)), ("rotmat", (24, 3, 3))):
        t = out[k].reshape(n, *shape)
        assert torch.equal(t, t[:8][idx]), k
        got[k] = t[:8].cpu().numpy()
    return got


_RUNS = {}


def _run(pkg, n, graph=False):
    key = (n, graph)
    if key not in _RUNS:
        m = pkg.build_synthetic_model(max_frames=n, with_gru=False, dtype="bf16")
        try:
            if graph:
                m.set_option(pkg._lib.OPT_USE_GRAPH, 1)
            base = pkg.synth.make_frames(8)
            other = pkg.synth.make_frames(8, start=8)
            if graph:                                                             # capture both, then replay each once: the checked call is a replay
                _forward_taps(m, n, base, other)
            _RUNS[key] = _forward_taps(m, n, base, other)
            _RUNS[key]["_kernels"] = m.conv_kernels(n)
        finally:
            m.close()
    return _RUNS[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _fuse(oracle, xs, sd, p):
    """The bf16 plan's fuse layer (csrc/grnet_plan.cpp hr_fuse_separate) on the branch outputs xs, rounding where it stores: every 1x1 up term W_ij x_j (+ BN) is
    stored in bf16 at the source resolution and nearest-upsampled where it is consumed; every link of a down chain D_ij (j < i-1) is stored in bf16; output 0
    is an elementwise fp32 sum of x_0 and the up terms, rounded once (fuse_sum_bf16); output i >= 1 is the stride-2 convolution from branch i-1 with x_i,
    the D_ij and the up terms added in its fp32 epilogue -- that link is NOT rounded before the sum -- then ReLU and one rounding.  (oracle.hr_fuse
    rounds every term instead; the sum is taken in the same order j = 0 .. nb-1 up to fp32 re-association.)"""
    nb = len(xs)
    up = lambda i, j: oracle.upsample_nearest(oracle.conv_bn(xs[j], sd, f"{p}fuse_layers.{i}.{j}.0.weight", f"{p}fuse_layers.{i}.{j}.1"), 2 ** (j - i))
    outs = [oracle._q(torch.relu(sum([xs[0]] + [up(0, j) for j in range(1, nb)])))]
    for i in range(1, nb):
        add = xs[i].clone()
        for j in range(i - 1):
            d = xs[j]
            for k in range(i - j):
                d = oracle.conv_bn(d, sd, f"{p}fuse_layers.{i}.{j}.{k}.0.weight", f"{p}fuse_layers.{i}.{j}.{k}.1", stride=2, relu=k != i - j - 1)
            add = add + d
        for j in range(i + 1, nb):
            add = add + up(i, j)
        q = f"{p}fuse_layers.{i}.{i - 1}.0."
        outs.append(oracle.conv_bn(xs[i - 1], sd, q + "0.weight", q + "1", stride=2, relu=True, residual=add))
    return outs


def _ratio(got, ref, floor):
    """max err / bound of _close_up_to_ties / _close_up_to_rounding_ties (same bound form): the margin, printed."""
    rms = float(np.sqrt(np.mean(ref * ref)))
    return float((np.abs(got - ref) / (np.abs(ref) * 2.0 ** -7 + floor * rms)).max())


def _slices(h, segs=()):
    """The image borders, and the rows on both sides of every band seam / segment boundary a kernel of this map size has: the wide / ring kernels' bands of
    4, 7, 8 and 14 rows, the row walks' segments (`segs`: rows per segment)."""
    sl = [np.s_[:, :, 0], np.s_[:, :, -1], np.s_[:, :, :, 0], np.s_[:, :, :, -1]]
    for step in sorted({4, 7, 8, 14} | set(segs)):
        rows = sorted({r for k in range(step, h, step) for r in (k - 1, k)})
        if rows and h > 7:
            sl.append(np.s_[:, :, rows])
    return sl


def _s2_rows_per_segment(n, wo):
    """conv_bf16_s2_rows' rows per workgroup at n frames (csrc/conv_bf16_s2.hip launch_s2_rows, from the device's CU count)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    segs = 1 if n >= 4 * cus else 4 if wo == 28 and 2 * n < 4 * cus else 2
    return -(-wo // segs), segs


@pytest.mark.parametrize("n", SIZES)
def test_stages_run_on_the_production_kernels(pkg, n):
    """grnet_conv_kernel_info at n frames: the stages checked below really are the LDS-resident kernels (a plan change that moves one back to the generic
    kernel would otherwise leave this file checking the generic kernel).  Names are families (grnet_run.cpp kernel_name); within a family the launcher picks by
    shape: conv_bf16_chain<256,7> is the frame-pair kernel (a grid of (N+1)/2), <32,56> the 8-convolution pipeline; conv_bf16_s2<28> on 32 -> 64 / 32 -> 32
    and conv_bf16_s2<14> on 64 -> 64 are the row walks conv_bf16_s2_rows, the other stride-2 shapes the band kernel; conv_bf16_wide<128,56> on 480 -> 256 is
    conv_bf16_wide_ring<256,56,4,true>."""
    ks = _run(pkg, n)["_kernels"]
    by_key = {}
    for key, name in ks:
        by_key.setdefault(key, []).append(name)
    one = lambda key: by_key[key][0] if len(by_key[key]) == 1 else by_key[key]
    for stage, m, nb in MODULES:
        for b in range(nb):
            c, w = BR[b], 56 >> b
            names = [one(f"{B}{stage}.{m}.branches.{b}.{k}.conv{j}.weight") for k in range(4) for j in (1, 2)]
            assert names == [f"conv_bf16_chain<{c},{w}>"] + [f"conv_bf16_chain<{c},{w}>+"] * 7, (stage, m, b, names)
    assert one(f"{B}transition1.0.0.weight") == "conv_bf16_wide<128,56>"
    assert one(f"{B}transition2.2.0.0.weight") == "conv_bf16_s2<14>"
    assert one("head.keypoint_deconv_layers.0.weight") == "conv_bf16_wide<128,56>"            # the 480 -> 256 ring launch (both first convolutions)
    assert one("head.keypoint_deconv_layers.3.weight") == one("head.smpl_deconv_layers.3.weight") == "conv_bf16_wide<128,56>"
    assert one("head.keypoint_final_layer.weight") == one("head.smpl_final_layer.weight") == "conv_bf16"                   # conv_bf16_pw_stream (>= 42 frames)
    assert one(f"{B}upsample_stage_2.1.weight") == "conv_bf16_wide<64,56>"
    assert by_key[f"{B}upsample_stage_4.9.weight"] == ["conv_bf16_wide<128,56>"] and by_key[f"{B}upsample_stage_3.5.weight"] == ["conv_bf16_wide<128,56>"]
    # the fuse layers' stride-2 links: the row walks (32 -> 64 / 32 -> 32 @56 -> 28, 64 -> 64 @28 -> 14) and the band kernel, incl. every finishing link
    for stage, m, nb in MODULES:
        p = f"{B}{stage}.{m}.fuse_layers."
        assert one(p + "1.0.0.0.weight") == "conv_bf16_s2<28>"                                   # 32 -> 64 finishing output 1, addends x_1 and the up terms
        if nb > 2:
            assert one(p + "2.1.0.0.weight") == "conv_bf16_s2<14>"                               # 64 -> 128 (band), finishing output 2
            assert one(p + "2.0.0.0.weight") == "conv_bf16_s2<28>"                               # 32 -> 32 first link (with (3,0)'s as 32 -> 64 in stage 4)
        if nb > 3:
            assert one(p + "3.1.0.0.weight") == "conv_bf16_s2<14>"                               # 64 -> 64 row walk
    assert one(f"{B}conv1.weight") == "conv_bf16_stem_pair" and one(f"{B}conv2.weight") == "conv_bf16_stem_pair+"


@pytest.mark.parametrize("n", SIZES)
def test_stages_equal_oracle_on_their_own_inputs(pkg, oracle, synth_weights, n):
    """Transitions, the four BasicBlocks of every branch, every fuse layer, the upsample heads, `cat`, the PARE head's convolutions, the attention pooling and
    the fp32 tail -- each on the GPU's own input.  Bars: one convolution or one fuse layer: _close_up_to_ties at depth 1 / 2 (a fuse output is one rounding
    behind stored terms that the GPU and the emulation round at the same places; 2 = the rounding of the term plus that of the output); a branch (8
    convolutions, 8 rounding points): _close_up_to_rounding_ties with blocks=4, as tests/test_gpu_conv_bf16.py holds the 8-convolution chain.  Borders and seams
    (fewer elements: the fraction / mean parts of the bar see fewer samples) at twice the depth, as test_gpu_bf16_roll.py does."""
    got = _run(pkg, n)
    sd = synth_weights
    worst = {}

    def check(fam, name, g, r, depth, segs=()):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        _close_up_to_ties(g, r, name, depth=depth)
        for sl in _slices(g.shape[2], segs):
            _close_up_to_ties(g[sl], r[sl], f"{name} border/seam", depth=2 * depth)
        worst[fam] = max(worst.get(fam, 0.0), _ratio(g, r, 2.0 ** -6))

    s2r = lambda wo: (_s2_rows_per_segment(n, wo)[0],)
    T = lambda name: _t(got[name])
    with oracle.bf16_storage():
        # transitions (hrnet.py:348-387)
        check("transition", "transition1.0", got["transition1.0"], oracle.conv_bn(T("layer1"), sd, B + "transition1.0.0.weight", B + "transition1.0.1", relu=True).numpy(), 1)
        check("transition", "transition1.1", got["transition1.1"],
              oracle.conv_bn(T("layer1"), sd, B + "transition1.1.0.0.weight", B + "transition1.1.0.1", stride=2, relu=True).numpy(), 1)
        check("transition", "transition2.2", got["transition2.2"],
              oracle.conv_bn(T("stage2.0.y1"), sd, B + "transition2.2.0.0.weight", B + "transition2.2.0.1", stride=2, relu=True).numpy(), 1)
        check("transition", "transition3.3", got["transition3.3"],
              oracle.conv_bn(T("stage3.3.y2"), sd, B + "transition3.3.0.0.weight", B + "transition3.3.0.1", stride=2, relu=True).numpy(), 1)
        # HR modules: the branches from the module's tapped inputs, the fuse layer from the tapped branch outputs
        inputs = {"stage2.0": ["transition1.0", "transition1.1"], "stage3.0": ["stage2.0.y0", "stage2.0.y1", "transition2.2"],
                  "stage4.0": ["stage3.3.y0", "stage3.3.y1", "stage3.3.y2", "transition3.3"]}
        for stage, mi, nb in MODULES:
            tag = f"{stage}.{mi}"
            ins = inputs.get(tag) or [f"{stage}.{mi - 1}.y{b}" for b in range(nb)]
            for b in range(nb):
                x = T(ins[b])
                for k in range(4):
                    x = oracle.basic_block(x, sd, f"{B}{tag}.branches.{b}.{k}.")
                g, r = got[f"{tag}.x{b}"], x.numpy()
                frac = _close_up_to_rounding_ties(g, r, 0.03 * 8, blocks=4)
                for sl in _slices(g.shape[2]):
                    _close_up_to_rounding_ties(g[sl], r[sl], 0.06 * 8, blocks=4)
                worst["branch"] = max(worst.get("branch", 0.0), _ratio(g, r, 2.0 ** -6))
            ys = _fuse(oracle, [T(f"{tag}.x{b}") for b in range(nb)], sd, f"{B}{tag}.")
            for i in range(nb):
                check("fuse", f"{tag}.y{i}", got[f"{tag}.y{i}"], ys[i].numpy(), 2, s2r(28) if i == 1 else s2r(14) if i == 2 else ())
        # upsample heads: bilinear x2 from the previous tap, the 3x3 from the bilinear tap
        for idx, layers, br in HEADS:
            prev = f"stage4.2.y{br}"
            for l in range(layers):
                nm = f"up{idx}.{l}"
                check("bilinear", nm + ".bilinear", got[nm + ".bilinear"], oracle.upsample_bilinear2x(T(prev)).numpy(), 1)
                q = f"{B}upsample_stage_{idx}."
                check("up_conv", nm + ".conv", got[nm + ".conv"], oracle.conv_bn(T(nm + ".bilinear"), sd, q + f"{4 * l + 1}.weight", q + f"{4 * l + 2}", relu=True).numpy(), 1)
                prev = nm + ".conv"
        # cat: the four slices ARE the taps (stage4.2's y0 is written into it, the heads' last convolutions too)
        parts = ["stage4.2.y0", "up2.0.conv", "up3.1.conv", "up4.2.conv"]
        assert np.array_equal(got["cat"], np.concatenate([got[p] for p in parts], 1))
        ys = _fuse(oracle, [T(f"stage4.2.x{b}") for b in range(4)], sd, f"{B}stage4.2.")
        ref_cat = np.concatenate([ys[0].numpy()] + [oracle.conv_bn(T(f"up{idx}.{layers - 1}.bilinear"), sd, f"{B}upsample_stage_{idx}.{4 * layers - 3}.weight",
                                                                   f"{B}upsample_stage_{idx}.{4 * layers - 2}", relu=True).numpy() for idx, layers, _ in HEADS], 1)
        check("cat", "cat", got["cat"], ref_cat, 2)
        # PARE head (pare.py:305-336): the 480 -> 256 first convolutions, the two second ones from the halves, heat / cam-shape maps
        hd = "head."
        ref_first = np.concatenate([oracle.conv_bn(T("cat"), sd, hd + f"{b}.0.weight", hd + f"{b}.1", relu=True).numpy()
                                    for b in ("keypoint_deconv_layers", "smpl_deconv_layers")], 1)
        check("head_conv", "head.first", got["head.first"], ref_first, 1)
        check("head_conv", "head.part_feats", got["head.part_feats"],
              oracle.conv_bn(_t(got["head.first"][:, :128]), sd, hd + "keypoint_deconv_layers.3.weight", hd + "keypoint_deconv_layers.4", relu=True).numpy(), 1)
        check("head_conv", "head.smpl_feats", got["head.smpl_feats"],
              oracle.conv_bn(_t(got["head.first"][:, 128:]), sd, hd + "smpl_deconv_layers.3.weight", hd + "smpl_deconv_layers.4", relu=True).numpy(), 1)
        lin = lambda x, k: oracle._q(oracle.conv2d(x, oracle._q(_t(sd[hd + k + ".weight"])), bias=sd[hd + k + ".bias"])).numpy()
        check("head_1x1", "head.heat", got["head.heat"], lin(T("head.part_feats"), "keypoint_final_layer"), 1)
        check("head_1x1", "head.cam_shape", got["head.cam_shape"], lin(T("head.smpl_feats"), "smpl_final_layer"), 1)
    # attention pooling (fp32 softmax / sums over bf16 maps): 1e-4 of the tensor's scale -- fp32 re-association over 3136 positions is ~1e-6
    attn = got["head.heat"][:, 1:]
    for k, feat in (("point_local_feat", "head.smpl_feats"), ("cam_shape_feats", "head.cam_shape")):
        e = rel_err(got[k], oracle.keypoint_attention(got[feat], attn))
        worst["attn_pool"] = max(worst.get("attn_pool", 0.0), e / 1e-4)
        assert e <= 1e-4, (k, e)
    # ... and element by element on the 8 distinct frames: the one bf16-path launch whose output is fp32, so the float64 pooling of the tapped bf16 maps
    # has no rounding tie to allow for -- the rule of tests/test_gpu_pool_elements.py (tests/helpers/pool_checks.py), printed first, then asserted
    case = pc.tapped_case(got["head.heat"], got["head.smpl_feats"], got["head.cam_shape"])
    held = pc.check("bf16", case, {k: got[k] for k in pc.OUTPUTS})
    for output, r, yard, accepted, place in held:
        print(pc.bounds_line("bf16", f"forward{n}", case["n"], output, r, yard, accepted, place))
    for output, (ratio, at), yard, accepted, _ in held:
        worst["attn_pool elements"] = max(worst.get("attn_pool elements", 0.0), ratio / accepted)
        assert accepted <= pc.FACTOR * pc.YARD_CEILING["bf16"] and ratio <= accepted, (output, ratio, at, yard, accepted)
    # the fp32 tail from the GPU's pooled features: the fp32 path's parity bar (tests/test_gpu_parity.py, 1e-3 of the tensor's scale)
    for k, e in _tail_errors(oracle, sd, got).items():
        worst["tail"] = max(worst.get("tail", 0.0), e / 1e-3)
        assert e < 1e-3, (k, e)
    print(f"n={n} worst err / bound per stage family: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _tail_errors(oracle, sd, got):
    rot6d, shape, cam = oracle.head_tail(got["point_local_feat"], got["cam_shape_feats"], sd)
    rotmat = oracle.rot6d_to_rotmat(rot6d).reshape(-1, 24, 3, 3)
    aa = oracle.rotmat_to_aa(rotmat.reshape(-1, 3, 3)).reshape(-1, 72)
    theta = np.concatenate([cam, aa, shape], 1)
    return {"theta": rel_err(got["theta"], theta), "rotmat": rel_err(got["rotmat"], rotmat)}


def test_graph_replay_equals_eager_tap_for_tap(pkg):
    """The 64-frame forward replayed from a captured hipGraph (GRNET_OPT_USE_GRAPH; the lanes become graph branches, the events behind empty chain-member ops
    become edges) equals the eager lane streams in every tap, bit for bit."""
    eager, graph = _run(pkg, 64), _run(pkg, 64, graph=True)
    for k in eager:
        if k != "_kernels":
            assert np.array_equal(eager[k], graph[k]), k


def test_debug_tensor_refuses_frames_it_does_not_hold_and_taps_not_written(pkg):
    """grnet_debug_tensor reads only what the last forward wrote: n_frames outside [1, last call's frames] is refused before any copy, and from 64 frames
    on stem_conv1 (computed inside conv_bf16_stem_pair, never stored) is refused instead of returning an earlier forward's values."""
    m = pkg.build_synthetic_model(max_frames=64, with_gru=False, dtype="bf16")
    try:
        frames = torch.from_numpy(np.tile(pkg.synth.make_frames(8), (8, 1, 1, 1))).cuda()
        m(frames[:16])
        torch.cuda.synchronize()
        small = m.debug_tensor("stem_conv1", 16)
        assert small.shape == (16, 64, 112, 112)
        for bad in (0, 17):
            with pytest.raises(pkg._lib.GrnetError, match="code -22"):
                m.debug_tensor("layer1", bad)
        m(frames)
        torch.cuda.synchronize()
        with pytest.raises(pkg._lib.GrnetError, match="code -1.*not written"):
            m.debug_tensor("stem_conv1", 64)
        assert torch.equal(m.debug_tensor("stem_conv2", 64)[:16], m.debug_tensor("stem_conv2", 16))
        with pytest.raises(pkg._lib.GrnetError, match="code -22"):
            m.debug_tensor("stem_conv2", 65)
    finally:
        m.close()


@pytest.mark.parametrize("scale", [0.0, 1.0, 60.0], ids=["uniform", "as_is", "peaked"])
def test_bf16_attention_pooling_under_extreme_heat_maps(pkg, oracle, synth_smpl, scale):
    """attn_pool_bf16x (csrc/head_kernels.hip) on a bf16 handle: per range of positions exp(h - max) and the partial sums, finished over the ranges by
    head_tail_kernel -- with the heat maps scaled to all-equal, as given, and x 60 (most ranges underflow to zero).  Teacher-forced on the tapped bf16 heat and
    feature maps (64 frames: the production kernels), pooled features at 1e-4 of their scale, the fp32 tail at the parity bar."""
    sd = {k: v.copy() for k, v in pkg.synth.make_state_dict().items()}
    for k in [k for k in sd if "keypoint_final_layer" in k]:
        sd[k] = (sd[k] * np.float32(scale)).astype(np.float32)
    m = pkg.GRNet(max_frames=64, dtype="bf16")
    try:
        m.load_state_dict(sd, strict=True)
        m.load_smpl(synth_smpl)
        m.finalize()
        idx = torch.arange(64) % 8
        frames = torch.from_numpy(pkg.synth.make_frames(8))[idx].contiguous().cuda()
        out = m(frames, extras=("point_local_feat", "cam_shape_feats"))[-1]
        torch.cuda.synchronize()
        got = {k: m.debug_tensor(k, 8).cpu().numpy() for k in ("head.heat", "head.smpl_feats", "head.cam_shape")}
        got["point_local_feat"] = out["point_local_feat"][:8].cpu().numpy()
        got["cam_shape_feats"] = out["cam_shape_feats"][:8].cpu().numpy()
        got["theta"] = out["theta"].reshape(64, 85)[:8].cpu().numpy()
        got["rotmat"] = out["rotmat"].reshape(64, 24, 3, 3)[:8].cpu().numpy()
        if scale == 0.0:
            assert not got["head.heat"].any()
        attn = got["head.heat"][:, 1:]
        for k, feat in (("point_local_feat", "head.smpl_feats"), ("cam_shape_feats", "head.cam_shape")):
            e = rel_err(got[k], oracle.keypoint_attention(got[feat], attn))
            print(f"scale {scale}: {k} {e:.2e}")
            assert e <= 1e-4, (k, e)
        for k, e in _tail_errors(oracle, sd, got).items():
            assert e < 1e-3, (k, e)
    finally:
        m.close()
