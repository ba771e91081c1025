"""bf16 convolution kernels of csrc/conv_bf16_chain.hip, conv_bf16_wide.hip, conv_bf16_s2.hip and csrc/conv_bf16.hip (round 5): BasicBlock chains with the frame resident in LDS (hrnet.py:30-59,
141-187), wide-band / ring kernels, stride-2 band kernel, layer1's 1x1 pairs and stream kernel, the bf16 fuse layer, bilinear x2 on NHWC bf16.
Bar (bf16 has no reference mode; stated as in test_gpu_bf16.py): every intermediate is rounded to bf16 exactly where the launch-per-convolution path stores it, so a
fused launch must equal (i) the fp32 oracle on bf16-rounded operands with the intermediates rounded to bf16 and (ii) the launch-per-convolution kernels, both up
to fp32 summation order: single elements differ by ONE bf16 ulp on rounding ties.  (The row-walking launches of round 6: tests/test_gpu_bf16_roll.py.)
Regrouped by component in round 6; the tests themselves are unchanged."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from .conftest import CALL_SIZE_NOISE, ROOT, elem_ratio, rel_err

pytestmark = pytest.mark.gpu

def _rb(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()

@pytest.fixture(scope="module")
def bmodel(pkg):
    m = pkg.build_synthetic_model(max_frames=64, with_gru=False, dtype="bf16")
    yield m
    m.close()

def _chain_weights(g, c, nconv):
    ws = [_rb(g.standard_normal((c, c, 3, 3)) * np.sqrt(2.0 / (c * 9))) for _ in range(nconv)]
    bs = [(g.standard_normal((c,)) * 0.1).astype(np.float32) for _ in range(nconv)]
    return ws, bs

def _oracle_chain(oracle, x, ws, bs):
    """BasicBlock by BasicBlock on the CPU: t = rb(relu(conv1(x) + b1)); x = rb(relu(conv2(t) + b2 + x))."""
    x = torch.from_numpy(x)
    for k in range(0, len(ws), 2):
        t = torch.from_numpy(_rb(torch.relu(oracle.conv2d(x.numpy(), ws[k], bias=bs[k])).numpy()))
        x = torch.from_numpy(_rb(torch.relu(oracle.conv2d(t.numpy(), ws[k + 1], bias=bs[k + 1]) + x).numpy()))
    return x.numpy()

def _close_up_to_rounding_ties(got, ref, max_mismatch, blocks=1):
    """One BasicBlock: an element is off by at most ONE bf16 ulp of itself (plus a floor for sums that cancel).  Behind several blocks an
    element y = conv(t) + x that nearly cancels inherits a whole ulp of its SUMMANDS (x is then ~the tensor's scale, and x itself may sit on
    the other side of a tie): the bar is one ulp of the tensor's scale there, and the mean error says that this is noise, not a wrong term."""
    err = np.abs(got - ref)
    rms = float(np.sqrt(np.mean(ref * ref)))
    floor = (2e-3 if blocks == 1 else 2.0 ** -6) * rms
    assert np.all(err <= np.abs(ref) * 2.0 ** -7 + floor), float((err / (np.abs(ref) * 2.0 ** -7 + floor)).max())
    frac = float(np.mean(err > np.abs(ref) * 2.0 ** -12 + 1e-6))
    assert frac <= max_mismatch, frac                                                                                # only on a few elements
    assert float(err.mean()) <= 2e-3 * rms * blocks ** 0.5, float(err.mean() / rms)
    return frac

@pytest.mark.parametrize("shape", [(64, 28), (128, 14), (256, 7), (32, 56)], ids=lambda s: f"{s[0]}ch{s[1]}")
@pytest.mark.parametrize("nconv", [2, 8])
def test_bf16_chain_equals_oracle_blocks(bmodel, oracle, shape, nconv):
    c, w = shape
    g = np.random.Generator(np.random.Philox(key=[85, c * 10 + nconv]))
    n = 3
    x = _rb(g.standard_normal((n, c, w, w)))
    ws, bs = _chain_weights(g, c, nconv)
    got = bmodel.op_conv_chain(torch.from_numpy(x).cuda(), ws, bs).cpu().numpy()
    assert got.shape == x.shape and np.array_equal(got, _rb(got))
    ref = _oracle_chain(oracle, x, ws, bs)
    frac = _close_up_to_rounding_ties(got, ref, 0.03 * nconv, blocks=nconv // 2)
    print(f"chain {c}ch @{w} x{nconv}: {frac:.4f} of the elements off by a rounding tie")
    # the borders are where the zero halo of the LDS image is read: looked at separately
    for sl in (np.s_[:, :, 0], np.s_[:, :, -1], np.s_[:, :, :, 0], np.s_[:, :, :, -1]):
        _close_up_to_rounding_ties(got[sl], ref[sl], 0.06 * nconv, blocks=nconv // 2)

@pytest.mark.parametrize("shape", [(64, 28), (128, 14), (256, 7), (32, 56)], ids=lambda s: f"{s[0]}ch{s[1]}")
def test_bf16_chain_equals_launch_per_convolution(bmodel, shape):
    """One BasicBlock: the chain launch against two launches of the per-convolution kernels on the same handle."""
    c, w = shape
    g = np.random.Generator(np.random.Philox(key=[86, c]))
    x = _rb(g.standard_normal((2, c, w, w)))
    ws, bs = _chain_weights(g, c, 2)
    xd = torch.from_numpy(x).cuda()
    t = bmodel.op_conv2d(xd, ws[0], bs[0], relu=True)
    ref = bmodel.op_conv2d(t, ws[1], bs[1], relu=True, add=xd).cpu().numpy()
    got = bmodel.op_conv_chain(xd, ws, bs).cpu().numpy()
    _close_up_to_rounding_ties(got, ref, 0.04)
    again = bmodel.op_conv_chain(xd, ws, bs).cpu().numpy()
    assert np.array_equal(got, again)                                    # deterministic

def test_bf16_pipeline_chain_equals_the_block_kernels_bit_for_bit(bmodel):
    """The 56x56 branch's 8-convolution chain is ONE launch (conv_bf16_chain_pipe: a pipeline of rows, a wave per convolution, rings of 4-6 rows in LDS); the same
    chain as two 4-convolution calls runs conv_bf16_block_frame (one launch per BasicBlock, the frame walked in bands).  Same seeds, tap order and rounding points:
    the bits must agree -- on 5 frames whose rows differ (a ring row read one step early or late would show), and again on a second call of the same handle."""
    c, w = 32, 56
    g = np.random.Generator(np.random.Philox(key=[89, 1]))
    x = torch.from_numpy(_rb(g.standard_normal((5, c, w, w)))).cuda()
    ws, bs = _chain_weights(g, c, 8)
    for _ in range(2):
        whole = bmodel.op_conv_chain(x, ws, bs)
        halves = bmodel.op_conv_chain(bmodel.op_conv_chain(x, ws[:4], bs[:4]), ws[4:], bs[4:])
        assert torch.equal(whole, halves)

def test_bf16_chain_frames_are_independent(bmodel):
    """A workgroup is a frame: the same frame gives the same bits wherever it sits in the call, and a 70-frame call (more workgroups than a
    test usually launches) equals its frames one by one."""
    c, w = 128, 14
    g = np.random.Generator(np.random.Philox(key=[87, 1]))
    base = _rb(g.standard_normal((5, c, w, w)))
    ws, bs = _chain_weights(g, c, 4)
    x = torch.from_numpy(np.tile(base, (14, 1, 1, 1))).cuda()            # 70 frames
    out = bmodel.op_conv_chain(x, ws, bs)
    one = bmodel.op_conv_chain(x[:5].contiguous(), ws, bs)
    for k in range(14):
        assert torch.equal(out[5 * k:5 * k + 5], one)

def test_bf16_forward_with_chains_equals_forward_without(bmodel, pkg):
    """The whole bf16 forward at 64 frames (the chain launches are taken from 64 frames per call on) against the same forward with one
    launch per convolution (GRNET_OPT_BF16_CHAIN = 0): same network, same roundings, different summation order in 120 of its launches."""
    frames = torch.from_numpy(np.tile(pkg.synth.make_frames(8), (8, 1, 1, 1))).cuda()
    keys = ("features", "point_local_feat")
    with_chain = bmodel(frames, extras=keys)[-1]
    n_with = bmodel.num_kernel_launches()
    bmodel.set_option(pkg._lib.OPT_BF16_CHAIN, 0)
    try:
        without = bmodel(frames, extras=keys)[-1]
        n_without = bmodel.num_kernel_launches()
    finally:
        bmodel.set_option(pkg._lib.OPT_BF16_CHAIN, -1)
    torch.cuda.synchronize()
    assert n_without - n_with == 7 * (8 + 7 + 3) + 7 * 8 + 8 + 1, (n_with, n_without)    # 26 chains of 8 convolutions became 26 launches (round 6: the 56x56 branch's too -- conv_bf16_chain_pipe); layer1's 12 convolutions 4 Bottleneck launches, the stem's two one
    # (the wide-band and stride-2 band kernels -- bits 4, 5 of the mask -- replace launches one for one: 45 stride-2 layers with up to three shifted addends run here)
    for k in keys + ("theta", "kp_3d", "verts"):
        a, b = with_chain[k].float().cpu().numpy(), without[k].float().cpu().numpy()
        rel = float(np.abs(a - b).max() / np.abs(b).max())
        mean_rel = float(np.abs(a - b).mean() / np.abs(b).mean())
        print(k, rel, mean_rel)
        # two bf16 evaluations of one network that differ in summation order: each is ~1.7e-2 from the fp32 oracle on the features (test_gpu_bf16.py), so
        # up to ~sqrt(2) x that from each other (measured 2.2e-2).  The pose outputs have single ill-conditioned entries (frames whose two 6-D vectors
        # are nearly collinear move by several 1e-2 under ANY bf16 noise: tools/bf16_outliers.py), so they are held on the mean
        if k in keys:
            assert rel < 4e-2, (k, rel)
        assert mean_rel < 2.5e-2, (k, mean_rel)
    d = (with_chain["kp_3d"] - without["kp_3d"]).reshape(-1, 29, 3).float()
    assert float(d.norm(dim=-1).mean()) < 5e-3                          # mean joint distance between the two evaluations: millimetres
    th = with_chain["theta"].reshape(8, 8, 85)
    assert torch.equal(th[0], th[5])                                     # the 8 distinct frames repeat exactly

@pytest.mark.parametrize("shape", [(64, 28), (128, 14), (256, 7), (32, 56)], ids=lambda s: f"{s[0]}ch{s[1]}")
def test_bf16_chain_time_at_256_frames(pkg, shape):
    """Not a parity test: prints the duration of the 8-convolution chain launch at 256 frames (one frame per CU) next to eight launches of the
    per-convolution kernel (tools/bf16_micro.py measures those: 31.3 / 30.5 / 31.2 us each in round 4)."""
    c, w = shape
    m = pkg.build_synthetic_model(max_frames=4, with_gru=False, dtype="bf16")
    g = np.random.Generator(np.random.Philox(key=[88, c]))
    x = torch.from_numpy(_rb(g.standard_normal((256, c, w, w)))).cuda()
    ws, bs = _chain_weights(g, c, 8)
    out, us = m.op_conv_chain(x, ws, bs, reps=20)
    flops = 2.0 * 256 * w * w * c * c * 9 * 8
    print(f"\nconv_bf16_chain<{c},{w}> x8 at 256 frames: {us:.1f} us per chain = {us / 8:.2f} us per convolution, {flops / us / 1e6:.0f} TFLOP/s")
    assert torch.isfinite(out).all() and us > 0
    m.close()

WIDE = [(128, 128, 56), (256, 256, 56), (480, 256, 56), (64, 64, 56), (256, 256, 28), (128, 128, 28), (160, 128, 56), (256, 32, 56)]

@pytest.mark.parametrize("case", WIDE, ids=lambda c: "x".join(map(str, c)))
def test_bf16_wide_band_kernel(bmodel, oracle, case):
    """conv_bf16_wide_band (one wide 3x3 stride-1 convolution, a band of the input resident in LDS, 128 / 64 input channels per pass): equal to the
    fp32 oracle on the same bf16-rounded operands up to the one rounding of its bf16 output -- the bar of every bf16 launch (test_gpu_bf16.py) --
    with and without ReLU; 480 and 160 input channels take a last pass of 96 / 32 channels; three frames = 24 / 12 / 6 bands; 256 -> 32: transition1's layer on the ring kernel with one 32-channel block."""
    cin, cout, h = case
    g = np.random.Generator(np.random.Philox(key=[89, cin * 1000 + cout + h]))
    n = 3 if h == 28 else 2
    x = _rb(g.standard_normal((n, cin, h, h)))
    w = _rb(g.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (cin * 9)))
    b = (g.standard_normal((cout,)) * 0.1).astype(np.float32)
    for relu in (True, False):
        ref = oracle.conv2d(x, w, bias=b)
        ref = (torch.relu(ref) if relu else ref).numpy()
        got = bmodel.op_conv2d(torch.from_numpy(x).cuda(), w, b, relu=relu, tile_hint=3003).cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got, _rb(got))
        assert np.all(np.abs(got - ref) <= np.abs(ref) * 2.0 ** -8 + 1e-5), float(np.abs(got - ref).max())
        for sl in (np.s_[:, :, 0], np.s_[:, :, -1], np.s_[:, :, :, 0], np.s_[:, :, :, -1], np.s_[:, :, 6:8], np.s_[:, :, 13:15]):      # borders, band seams
            assert np.all(np.abs(got[sl] - ref[sl]) <= np.abs(ref[sl]) * 2.0 ** -8 + 1e-5)

def test_bf16_wide_band_refuses_other_shapes(bmodel, pkg):
    x = torch.zeros(1, 128, 14, 14).cuda()
    with pytest.raises(pkg._lib.GrnetError, match="not eligible"):
        bmodel.op_conv2d(x, np.zeros((128, 128, 3, 3), np.float32), None, tile_hint=3003)
    with pytest.raises(pkg._lib.GrnetError, match="not eligible"):
        bmodel.op_conv2d(torch.zeros(1, 256, 56, 56).cuda(), np.zeros((96, 256, 3, 3), np.float32), None, tile_hint=3003)

@pytest.mark.parametrize("with_add", [True, False])
def test_bf16_pointwise_256_channel_tile(bmodel, oracle, with_add):
    """layer1's 64 -> 256 1x1 convolutions (hrnet.py:80-100) at 20 frames: the residual is requested beside the patch DMA (round 5) instead of in
    the epilogue.  Same bar as every bf16 launch."""
    g = np.random.Generator(np.random.Philox(key=[90, int(with_add)]))
    n = 20
    x = _rb(g.standard_normal((n, 64, 56, 56)))
    w = _rb(g.standard_normal((256, 64, 1, 1)) * np.sqrt(2.0 / 64))
    b = (g.standard_normal((256,)) * 0.1).astype(np.float32)
    add = _rb(g.standard_normal((n, 256, 56, 56))) if with_add else None
    ref = oracle.conv2d(x, w, bias=b)
    ref = torch.relu(ref + torch.from_numpy(add) if with_add else ref).numpy()
    got = bmodel.op_conv2d(torch.from_numpy(x).cuda(), w, b, relu=True, add=torch.from_numpy(add).cuda() if with_add else None).cpu().numpy()
    assert np.array_equal(got, _rb(got))
    assert np.all(np.abs(got - ref) <= np.abs(ref) * 2.0 ** -8 + 1e-5), float(np.abs(got - ref).max())

S2 = [(64, 64, 112), (64, 128, 28), (32, 128, 28), (32, 32, 28), (32, 64, 56), (32, 32, 56), (64, 64, 28)]

@pytest.mark.parametrize("case", S2, ids=lambda c: "x".join(map(str, c)))
def test_bf16_stride2_band_kernel(bmodel, oracle, case):
    """conv_bf16_s2_band (one 3x3 stride-2 convolution; the input band de-interleaved by row and column parity into four LDS sub-planes so that every tap
    is a constant offset) and, round 6, conv_bf16_s2_rows (32 -> 64 / 32 -> 32 @56 -> 28, 64 -> 64 @28 -> 14: a walk over output rows, two new input rows per step
    by LDS-DMA de-interleaved by column parity, a wave per (tile, channel block) with its weights in registers; 2 or 5 frames run as 2 or 4 row segments each):
    every shape they are used for, with and without a fused addend and ReLU, against the fp32 oracle on the same bf16-rounded operands up to the one rounding
    of the bf16 output.  Frames of 56 / 28 / 14 / 7 output rows: first, middle and last (partial) bands."""
    cin, cout, h = case
    g = np.random.Generator(np.random.Philox(key=[91, cin * 1000 + cout + h]))
    n = 2 if h >= 56 else 5
    x = _rb(g.standard_normal((n, cin, h, h)))
    w = _rb(g.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (cin * 9)))
    b = (g.standard_normal((cout,)) * 0.1).astype(np.float32)
    add = _rb(g.standard_normal((n, cout, h // 2, h // 2)))
    lin = oracle.conv2d(x, w, stride=2, bias=b)
    for relu, with_add in ((True, True), (False, False)):
        ref = lin + torch.from_numpy(add) if with_add else lin
        ref = (torch.relu(ref) if relu else ref).numpy()
        got = bmodel.op_conv2d(torch.from_numpy(x).cuda(), w, b, stride=2, relu=relu, add=torch.from_numpy(add).cuda() if with_add else None, tile_hint=3004).cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got, _rb(got))
        assert np.all(np.abs(got - ref) <= np.abs(ref) * 2.0 ** -8 + 1e-5), float(np.abs(got - ref).max())
        for sl in (np.s_[:, :, 0], np.s_[:, :, -1], np.s_[:, :, :, 0], np.s_[:, :, :, -1]):
            assert np.all(np.abs(got[sl] - ref[sl]) <= np.abs(ref[sl]) * 2.0 ** -8 + 1e-5)

S2_ROWS = [(32, 64, 56), (32, 32, 56), (64, 64, 28)]

def _s2_rows_call_sizes(wo):
    """Call sizes that give conv_bf16_s2_rows 4 / 2 / 1 row segments per frame (launch_s2_rows, from the device's CU count: 4 below 2 x CUs frames -- only
    on 28-row outputs --, 2 below 4 x CUs, 1 from there on)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return ({4: 5, 2: 2 * cus, 1: 4 * cus} if wo == 28 else {2: 5, 1: 4 * cus}), cus

@pytest.mark.parametrize("case", S2_ROWS, ids=lambda c: "x".join(map(str, c)))
def test_bf16_stride2_row_walk_at_every_segment_count(bmodel, oracle, pkg, case):
    """conv_bf16_s2_rows at the call sizes that split a frame into 4, 2 and 1 row segments (the forward reaches 4 and 2 only; 1 from 4 x CUs frames), plainly
    and in the fuse layers' finishing-link form: ReLU over three addends read through channel-offset views, the last one a nearest-upsampled (shift 1) term.
    5 distinct frames tiled: every copy gives the same bits, and the oracle runs on the distinct ones (fp32 on the same bf16 operands, one output rounding)."""
    cin, cout, h = case
    ho = h // 2
    g = np.random.Generator(np.random.Philox(key=[93, cin * 1000 + cout + h]))
    x = _rb(g.standard_normal((5, cin, h, h)))
    w = _rb(g.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (cin * 9)))
    b = (g.standard_normal((cout,)) * 0.1).astype(np.float32)
    adds = [(_rb(g.standard_normal((5, cout, ho, ho))), 0, 0), (_rb(g.standard_normal((5, cout + 32, ho, ho))), 32, 0),
            (_rb(g.standard_normal((5, cout + 64, ho // 2, ho // 2))), 64, 1)]
    lin = oracle.conv2d(x, w, stride=2, bias=b).numpy()
    three = lin + adds[0][0] + adds[1][0][:, 32:] + oracle.upsample_nearest(torch.from_numpy(adds[2][0][:, 64:]), 2).numpy()
    sizes, cus = _s2_rows_call_sizes(ho)
    assert sizes[1] == 4 * cus and 2 * cus <= 1024
    for segs, n in sizes.items():
        idx = torch.arange(n) % 5
        tile = lambda a: torch.from_numpy(a)[idx].contiguous().cuda()
        for relu, with_adds in ((False, False), (True, True)):
            got = bmodel.op_conv2d_adds(tile(x), w, b, stride=2, relu=relu, adds=[(tile(a), off, sh) for a, off, sh in adds] if with_adds else (), tile_hint=3004)
            assert torch.equal(got, got[:5][idx.cuda()]), (segs, n)                                     # every copy of a frame: the same bits
            got = got[:5].cpu().numpy()
            ref = np.maximum(three, 0) if with_adds else lin
            assert got.shape == ref.shape and np.array_equal(got, _rb(got))
            rows = -(-ho // segs)
            for sl in (np.s_[:], np.s_[:, :, 0], np.s_[:, :, -1], np.s_[:, :, :, 0], np.s_[:, :, :, -1],
                       np.s_[:, :, sorted({r for k in range(rows, ho, rows) for r in (k - 1, k)})] if segs > 1 else np.s_[:, :, :1]):
                assert np.all(np.abs(got[sl] - ref[sl]) <= np.abs(ref[sl]) * 2.0 ** -8 + 1e-5), (segs, n, relu, float(np.abs(got[sl] - ref[sl]).max()))
        del got
    with pytest.raises(pkg._lib.GrnetError, match="bad addend"):                                        # a view past the addend's channels is refused
        bmodel.op_conv2d_adds(torch.zeros(1, cin, h, h).cuda(), w, b, stride=2, adds=[(torch.zeros(1, cout, ho, ho).cuda(), 8, 0)], tile_hint=3004)

def test_bf16_stride2_kernels_refuse_other_shapes(bmodel, pkg):
    """Forced onto the stride-2 kernels (tile_hint 3004), a shape none of them is built for is refused, not run on something else: a 128-channel input (four
    passes of the band kernel lose to the generic one, the row walk holds 32 / 64 input channels), a stride-1 layer, an odd map."""
    for x, w, stride in ((torch.zeros(1, 128, 28, 28), np.zeros((256, 128, 3, 3), np.float32), 2),
                         (torch.zeros(1, 32, 56, 56), np.zeros((64, 32, 3, 3), np.float32), 1),
                         (torch.zeros(1, 32, 30, 30), np.zeros((64, 32, 3, 3), np.float32), 2)):
        with pytest.raises(pkg._lib.GrnetError, match="not eligible"):
            bmodel.op_conv2d(x.cuda(), w, None, stride=stride, tile_hint=3004)

def test_bf16_layer1_pairs_are_bit_identical(bmodel, pkg):
    """layer1's 64 -> 256 expansion + the next Bottleneck's 256 -> 64 reduction as one launch (bit 6 of the mask): the reduction reads the very bf16 tile
    the stand-alone launch would read from HBM, in the same k order -- the whole forward must not change by a bit (compared with the 256-channel tile
    of the expansion forced either way, so that the only difference is where the reduction runs)."""
    frames = torch.from_numpy(np.tile(pkg.synth.make_frames(8), (8, 1, 1, 1))).cuda()
    base = 1023 - 256 - 512                                       # (round 6: the Bottleneck launches, bits 8 / 9, replace the pairs at this call size: off here)
    try:
        bmodel.set_option(pkg._lib.OPT_BF16_CHAIN, base)
        a = bmodel(frames, extras=("features",))[-1]
        n_a = bmodel.num_kernel_launches()
        bmodel.set_option(pkg._lib.OPT_BF16_CHAIN, base - 64)
        b = bmodel(frames, extras=("features",))[-1]
        n_b = bmodel.num_kernel_launches()
    finally:
        bmodel.set_option(pkg._lib.OPT_BF16_CHAIN, -1)
    torch.cuda.synchronize()
    assert n_b - n_a == 3
    for k in ("features", "theta", "verts"):
        assert torch.equal(a[k], b[k]), k

# ----------------------------------------------------------------------------- the grouped fuse launch on the bf16 path (csrc/hr_fuse.hip: hr_fuse_up_bf16)
FUSE_MODULES = [("stage2", 0, 2)] + [("stage3", m, 3) for m in range(4)] + [("stage4", m, 4) for m in range(3)]

@pytest.fixture(scope="module")
def fmodel(pkg):
    """The bf16 plan's fuse layer (hr_fuse_separate: one merged 1x1 launch per source branch, every output finished by its stride-2 convolution's epilogue, output 0
    by an elementwise sum).  Round 5 also measured two layouts around the grouped launch hr_fuse_up_bf16 (output 0 only / the fp32 path's layout); both lost and are
    A/B variants of diagnostic builds only (GRNET_AB(BF16_FUSE_UP) in csrc/grnet_plan.cpp) -- this fixture used to build them through an environment variable."""
    m = pkg.build_synthetic_model(max_frames=16, with_gru=False, dtype="bf16")
    yield m
    m.close()

@pytest.mark.parametrize("n", [1, 3, 16])
def test_bf16_fuse_layer_of_every_hr_module_matches_oracle(fmodel, pkg, oracle, synth_weights, n):
    """As tests/test_gpu_round4.py does for fp32: the module's branch outputs x_b and outputs y_i are read back from the bf16 forward, the fp32 oracle's
    fuse layer (hrnet.py:189-244, 258-265) runs on those x_b, and every y_i must agree to bf16 accuracy: weights and the stored 1x1 terms / chain
    links are rounded to bf16 (2^-9 relative each), so max |diff| <= 1.5e-2 of the tensor's scale and the mean error <= 2e-3 of its rms; outputs >= 0."""
    frames = pkg.synth.make_frames(n)
    fmodel(torch.from_numpy(frames).cuda().unsqueeze(0))
    torch.cuda.synchronize()
    for stage, m, nb in FUSE_MODULES:
        tag = f"{stage}.{m}."
        xs = [fmodel.debug_tensor(tag + f"x{b}", n).cpu() for b in range(nb)]
        ref = oracle.hr_fuse(xs, synth_weights, f"backbone.{tag}")
        for i in range(nb):
            got = fmodel.debug_tensor(tag + f"y{i}", n).cpu().numpy()
            r = ref[i].numpy()
            assert got.shape == r.shape and got.min() >= 0.0
            err = np.abs(got - r)
            assert err.max() <= 1.5e-2 * np.abs(r).max(), (tag, i, float(err.max() / np.abs(r).max()))
            assert err.mean() <= 2e-3 * np.sqrt(np.mean(r * r)), (tag, i, float(err.mean() / np.sqrt(np.mean(r * r))))

def test_bf16_fuse_layer_launch_count_and_macs(fmodel):
    """The default bf16 layout has no grouped launch; the 31 1x1 up terms are 18 launches (the terms of ONE source branch merged, output channels side by side);
    the MACs still add up to SURVEY 8(d)'s 15 441 563 648 per frame."""
    convs = fmodel.describe_convs()
    assert len([c for c in convs if c["cin"] == 0]) == 0
    assert sum(c["macs"] for c in convs) == 15441563648
    left = [c for c in convs if c["ks"] == 1 and "fuse_layers" in c["name"] and c["cin"]]
    assert len(left) == 18, len(left)

# ---- layer1's 64 -> 256 1x1 layers as a stream (csrc/conv_bf16.hip: conv_bf16_pw_stream) -------------------------------------------------
def _forward_digest(m, frames):
    import hashlib
    out = m(frames, extras=("features",))[-1]
    torch.cuda.synchronize()
    return [m.num_kernel_launches()] + [hashlib.sha256(out[k].cpu().numpy().tobytes()).hexdigest() for k in ("features", "theta", "verts")]

@pytest.mark.parametrize("n", [8, 64])
def test_bf16_layer1_stream_kernel_is_bit_identical_to_the_generic_one(pkg, bmodel, n):
    """conv_bf16_pw_stream (persistent workgroups, register prefetch; all three forms: [t ; x] two-input + pair, residual + pair, residual alone) against
    conv_bf16_nhwc on the same layers: same operands, same k order, same (acc + residual) + bias -> ReLU -> bf16 -- the whole forward may not change by a
    bit.  GRNET_OPT_BF16_CHAIN bit 7 switches the stream kernel; bits 8 / 9 -- the Bottleneck and stem-pair launches that replace these layers in large calls -- are off here.  8 frames: forced
    on with GRNET_OPT_BF16_MIN_FRAMES = 1 (fewer tiles than workgroups, the clamped re-request of the last tile); 64 frames: the size it is picked at."""
    lib = pkg._lib
    frames = torch.from_numpy(np.tile(pkg.synth.make_frames(8), (n // 8, 1, 1, 1))).cuda()
    try:
        base = 1023 - 256 - 512                                   # the Bottleneck / stem-pair launches off: layer1's 1x1 layers run as launches of their own
        bmodel.set_option(lib.OPT_BF16_MIN_FRAMES, 1)
        bmodel.set_option(lib.OPT_BF16_CHAIN, base - 128)
        ref = _forward_digest(bmodel, frames)
        bmodel.set_option(lib.OPT_BF16_CHAIN, base)
        got = _forward_digest(bmodel, frames)
        assert ref == got                                         # same number of launches, same bits
        bmodel.set_option(lib.OPT_BF16_CHAIN, base - 64)
        unpaired = _forward_digest(bmodel, frames)
        assert unpaired[1:] == ref[1:]
    finally:
        bmodel.set_option(lib.OPT_BF16_CHAIN, -1)
        bmodel.set_option(lib.OPT_BF16_MIN_FRAMES, 0)

@pytest.mark.parametrize("shape", [(2, 64, 28, 28), (3, 128, 14, 14), (2, 256, 7, 7), (1, 128, 28, 28), (2, 256, 28, 28), (16, 256, 14, 14)])
def test_bf16_bilinear2x_rows_kernel(bmodel, oracle, shape):
    """bilinear2x_bf16_rows_kernel (an input row pair per workgroup, staged in LDS; fp contraction off) through the op entry of a bf16 handle: the fp32 two-tap
    formula of nn.Upsample(scale_factor=2, bilinear, align_corners=True) (hrnet.py:443) on the bf16-rounded input, rounded once to bf16 -- every element within
    one bf16 rounding of torch's CPU kernel, every output row written (the last one's source coordinate rounds to just below H - 1), results bf16 values."""
    g = np.random.Generator(np.random.Philox(key=[97, shape[1] * 100 + shape[2]]))
    x = _rb(g.standard_normal(shape))
    ref = oracle.upsample_bilinear2x(x).numpy()
    got = bmodel.op_bilinear2x(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got, _rb(got))
    assert np.all(np.abs(got - ref) <= np.abs(ref) * 2.0 ** -8 + 1e-5), float(np.abs(got - ref).max())
    assert np.all(np.abs(got[:, :, -1] - ref[:, :, -1]) <= np.abs(ref[:, :, -1]) * 2.0 ** -8 + 1e-5) and np.all(np.abs(got[:, :, 0] - ref[:, :, 0]) <= np.abs(ref[:, :, 0]) * 2.0 ** -8 + 1e-5)
