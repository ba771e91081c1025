"""oracle.float64(): the float64 mode the fp32 stage tests (tests/test_gpu_f32_stages.py) take their references from."""
import numpy as np
import torch

from .conftest import rel_err


def test_float64_oracle_agrees_with_fp32_oracle_on_golden_frames(pkg, oracle, synth_weights, synth_smpl):
    """A forward on the 4 golden frames under float64() agrees with the fp32 oracle on `features` and `point_local_feat` to 1e-5 of their scale (the
    fp32 oracle's own rounding), its backbone and head tensors are float64, and leaving the context restores float32."""
    frames = pkg.synth.make_frames(4)
    ref = oracle.grnet_forward(frames, synth_weights, synth_smpl, return_intermediates=True)
    with oracle.float64():
        d = oracle.grnet_forward(frames, synth_weights, synth_smpl, return_intermediates=True)
        assert oracle.conv_bn(torch.zeros(1, 64, 8, 8), synth_weights, "backbone.conv2.weight", "backbone.bn2").dtype == torch.float64
    for k in ("features", "point_local_feat"):
        assert d[k].dtype == np.float64, k
        e = rel_err(ref[k], d[k])
        assert 0 < e <= 1e-5, (k, e)
    assert oracle.conv_bn(torch.zeros(1, 64, 8, 8), synth_weights, "backbone.conv2.weight", "backbone.bn2").dtype == torch.float32


def test_float64_temporal_modules_agree_with_fp32_oracle_and_goldens(pkg, oracle):
    """ts_attn_block / multi_attention, gru_forward and feat_corrector under float64() -- there the composition of the per-launch stage functions -- against the
    fp32 oracle and the reference's own outputs (tests/golden/{tsattn,gru,featcorr}.npz) within the bars tests/test_oracle_golden.py holds the fp32 oracle to;
    results are float64 inside the context and float32 again outside it."""
    import os
    from .conftest import ROOT
    gold = lambda name: np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    g, sd = gold("tsattn"), pkg.synth.make_tsattn_state_dict()
    for (b, t) in ((2, 8), (1, 16)):
        x, xs = pkg.synth.make_tsattn_inputs(b, t)
        with oracle.float64():
            a, y = oracle.multi_attention(x, xs, sd, "mulattn."), oracle.ts_attn_block(x, xs, sd)
        assert a.dtype == np.float64 and y.dtype == np.float64 and y.shape == (b, t, 3072)
        assert rel_err(a[:, :, ::8], g[f"attn_{b}_{t}"]) < 2e-5 and rel_err(y, g[f"y_{b}_{t}"]) < 2e-5
        y32 = oracle.ts_attn_block(x, xs, sd)
        assert y32.dtype == np.float32 and 0 < rel_err(y32, y) < 2e-5
    g, sd = gold("gru"), pkg.synth.make_gru_state_dict()
    for (b, t) in ((2, 6), (1, 16)):
        x, cp = pkg.synth.make_gru_inputs(b, t)
        with oracle.float64():
            y, ph, xc = oracle.gru_forward(x, cp, sd)
        assert y.dtype == ph.dtype == xc.dtype == np.float64
        for got, key in ((y, "y"), (ph, "phase"), (xc, "xc")):
            assert rel_err(got, g[f"{key}_{b}_{t}"]) < 1e-5, key
        y32, ph32, _ = oracle.gru_forward(x, cp, sd)
        assert y32.dtype == np.float32 and rel_err(y32, y) < 1e-5 and rel_err(ph32, ph) < 1e-5
    g, sd = gold("featcorr"), pkg.synth.make_featcorr_state_dict()
    for (b, n) in ((2, 8), (1, 16)):
        x, cp = pkg.synth.make_featcorr_inputs(b, n)
        with oracle.float64():
            y, avg, ph = oracle.feat_corrector(x, cp, sd)
            cparams = oracle.gait_cparams(cp.reshape(-1, 3), *pkg.synth.make_gait_boxes(b, n))
        assert y.dtype == np.float64 and y.shape == (b * n, 128, 24) and cparams.dtype == np.float64
        assert rel_err(y, g[f"y_{b}_{n}"]) < 2e-5 and rel_err(avg, g[f"avg_{b}_{n}"]) < 1e-5 and rel_err(ph, g[f"phase_{b}_{n}"]) < 1e-5
        y32, avg32, ph32 = oracle.feat_corrector(x, cp, sd)
        assert y32.dtype == np.float32 and rel_err(y32, y) < 2e-5 and rel_err(avg32, avg) < 1e-5 and rel_err(ph32, ph) < 1e-5
        assert rel_err(oracle.gait_cparams(cp.reshape(-1, 3), *pkg.synth.make_gait_boxes(b, n)), cparams) < 1e-6


def test_stage_chains_restate_the_module_functions(pkg, oracle):
    """Outside float64() the stage chains (ts_stages, gru_stages, fc_stages: one function per GPU launch) are a second fp32 restatement of the modules: they
    agree with the module functions within the fp32 rounding of either."""
    sd = pkg.synth.make_tsattn_state_dict()
    x, xs = pkg.synth.make_tsattn_inputs(2, 8)
    st = oracle.ts_stages(x, xs, sd)
    assert st["out"].dtype == np.float32 and rel_err(st["out"], oracle.ts_attn_block(x, xs, sd)) < 5e-6
    assert rel_err(st["y_t"] + st["y_s"], oracle.multi_attention(x, xs, sd, "mulattn.")) < 5e-6
    sd = pkg.synth.make_featcorr_state_dict()
    x, cp = pkg.synth.make_featcorr_inputs(2, 8)
    st = oracle.fc_stages(x, cp, sd)
    y, avg, ph = oracle.feat_corrector(x, cp, sd)
    assert rel_err(st["out"].reshape(y.shape), y) < 5e-6 and rel_err(st["avg"], avg) < 5e-6 and rel_err(st["phase"], ph) < 5e-6


def test_chunked_and_sampled_temporal_attention_equal_the_unchunked_one(pkg, oracle):
    """ts_stage_temporal_attention at 500 frames: chunks of 64 queries, a list of query rows, and key ranges merged by hand all give the one-piece result (to
    float64 rounding); the key-part ranges are the blocked kernel's (whole 32-key blocks, block floor(nblk p / parts))."""
    sd = pkg.synth.make_tsattn_state_dict()
    x, _ = pkg.synth.make_tsattn_inputs(1, 500)
    qkv = np.asarray(oracle.linear(x.reshape(1, 500, -1), sd["mulattn.qkv_t.weight"], sd["mulattn.qkv_t.bias"]), np.float32)
    rows = np.array([0, 1, 15, 127, 128, 255, 256, 383, 384, 498, 499])
    with oracle.float64():
        whole = oracle.ts_stage_temporal_attention(qkv, chunk=500)
        assert whole.dtype == np.float64
        assert np.abs(oracle.ts_stage_temporal_attention(qkv, chunk=64) - whole).max() < 1e-13
        assert np.abs(oracle.ts_stage_temporal_attention(qkv, rows, chunk=4) - whole[:, rows]).max() < 1e-13
        ranges = oracle.ts_key_part_ranges(500, 3)
        assert ranges == [(0, 160), (160, 320), (320, 500)]
        parts = [oracle.ts_stage_temporal_attention(qkv, rows, key_range=kr, partial=True) for kr in ranges]
        lse = np.stack([p[1] for p in parts])                                         # (parts, 1, rows, heads), base 2
        w = np.exp2(lse - lse.max(0))
        w = np.repeat(w / w.sum(0), 250, -1)
        merged = sum(wp * p[0] for wp, p in zip(w, parts))
        assert np.abs(merged - whole[:, rows]).max() < 1e-13
    assert oracle.ts_stage_temporal_attention(qkv, rows).dtype == np.float32
    assert oracle.ts_key_part_ranges(10000, 4) == [(0, 2496), (2496, 4992), (4992, 7488), (7488, 10000)]          # 78 / 78 / 78 / 79 blocks
