"""The stage checks of tests/test_gpu_temporal_stages.py can fail: no GPU here, the checks of tests/helpers/temporal_checks.py are fed

  * the plain fp32 restatement of every stage (the oracle's stage functions outside float64(), each on the previous stage's fp32 output) -- must pass;
  * mutated references rounded to fp32 -- subtly wrong GEMMs, attention kernels, gates, LayerNorms, recurrences -- each must fail its stage's check with an
    error of at least twice the bar.  Where a mutant passed a per-tensor check, the CHECK was changed (per-row metric for the attention stages, the
    low-variance input for the LayerNorms), not the mutant.

Every mutant is an independent float64 computation of the faulty arithmetic on the stage's own fp32 input.
"""
import numpy as np
import pytest

from .helpers import temporal_checks as tc

LOG2E = 1.4426950408889634


def _walk(walk, cls_of, label):
    log = []
    for stage, got, ref in walk:
        tc.check_stage(stage, cls_of(stage), got, ref, log, label)
    tc.report(log)


def _must_fail(name, stage, cls, mutant, ref):
    """The mutant, rounded to fp32, misses the stage's bar by a factor of two or more in at least one metric of the check."""
    got = np.asarray(mutant, np.float32).reshape(ref.shape)
    ratios = {m: (e, tc.bar(stage, cls, m)) for m, e in tc.stage_errors(stage, got, ref).items()}
    tc.report([f"mutant {name:58s} {stage:14s} class {cls:2s} " + "  ".join(f"[{m}] error {e:.2e} bar {b:.2e}" for m, (e, b) in ratios.items())])
    assert max(e / max(b, 1e-30) for e, b in ratios.values()) >= 2.0, (name, ratios)
    with pytest.raises(AssertionError):
        tc.check_stage(stage, cls, got, ref)


def test_fp32_restatement_passes_every_stage_check(pkg, oracle):
    """An honest fp32 implementation passes: the attention block at 4 x 64 and 1 x 385 (3 key parts), the low-variance LayerNorm case, the GRU at 4 x 64 and
    3 x 257, the corrector at 1 x 16."""
    sd = pkg.synth.make_tsattn_state_dict()
    for b, n, parts in ((4, 64, 1), (1, 385, 3)):
        x, xs = pkg.synth.make_tsattn_inputs(b, n)
        cls = tc.size_class("ts", n)
        _walk(tc.ts_walk(oracle, sd, tc.HostSource(x=x.reshape(b, n, -1), xs=xs.reshape(b, n, -1)), b, n, parts), lambda s: cls, f"f32 ts {b}x{n}")
    lsd, x, xs = tc.low_variance_case(pkg)
    _walk(tc.ts_walk(oracle, lsd, tc.HostSource(x=x.reshape(1, 16, -1), xs=xs.reshape(1, 16, -1)), 1, 16, 1), lambda s: "LN", "f32 ts LN")
    gsd = pkg.synth.make_gru_state_dict()
    for b, t in ((4, 64), (3, 257)):
        x, cp = pkg.synth.make_gru_inputs(b, t)
        cls = tc.size_class("gru", t)
        _walk(tc.gru_walk(oracle, gsd, tc.HostSource(x=x, cparams=cp), b, t), lambda s: cls, f"f32 gru {b}x{t}")
    fsd = pkg.synth.make_featcorr_state_dict()
    x, _ = pkg.synth.make_featcorr_inputs(1, 16)
    cam, bbox, cimg = tc.make_gait_inputs(pkg, 1, 16)
    _walk(tc.fc_walk(oracle, fsd, tc.HostSource(x=x, cam=cam, bbox=bbox, cimg=cimg), 1, 16, 1), lambda s: "S", "f32 fc 1x16")


# ------------------------------------------------------------------------------------------------- attention block
@pytest.fixture(scope="module")
def ts385(pkg, oracle):
    """The fp32 restatement's tensors of one 385-frame clip (3 key parts on 256 CUs): every stage's input."""
    sd = pkg.synth.make_tsattn_state_dict()
    x, xs = pkg.synth.make_tsattn_inputs(1, 385)
    src = tc.HostSource(x=x.reshape(1, 385, -1), xs=xs.reshape(1, 385, -1))
    refs = {stage: ref for stage, _, ref in tc.ts_walk(oracle, sd, src, 1, 385, 3)}
    return sd, src.t, refs


def _f64(a):
    return np.asarray(a, np.float64)


def _gemm(a, w, bias):
    return _f64(a) @ _f64(w).T + _f64(bias)


def test_gemm_mutants_fail(pkg, oracle, ts385):
    sd, t, refs = ts385
    W = lambda k: sd["mulattn." + k]
    # one k-step of 4 omitted in one 64 x 64 tile (qkv_t: 385 x 3000 x 3072)
    a, w = t["x"][0], W("qkv_t.weight")
    m = _gemm(a, w, W("qkv_t.bias"))
    m[64:128, 128:192] -= _f64(a[64:128, 1024:1028]) @ _f64(w[128:192, 1024:1028]).T
    _must_fail("GEMM: one k-step of 4 omitted in one 64x64 tile", "ts.qkv_t", "M", m, refs["ts.qkv_t"][0])
    # bias missing in the last, partial N tile (3000 = 46 x 64 + 56)
    m = _gemm(a, w, W("qkv_t.bias"))
    m[:, 2944:] -= _f64(W("qkv_t.bias"))[2944:]
    _must_fail("GEMM: bias missing in the last partial N tile (N 3000)", "ts.qkv_t", "M", m, refs["ts.qkv_t"][0])
    # the K tail beyond the last full 32 dropped, K = 1000 (fc_t: 992 + 8)
    a, w = t["ts.x_t_gated"][0], W("fc_t.weight")
    _must_fail("GEMM: K tail beyond the last full 32 dropped (K 1000)", "ts.y_t", "M", _gemm(a[:, :992], w[:, :992], W("fc_t.bias")), refs["ts.y_t"][0])
    # one split-K slice added twice (gate logits: 1 x 2000 x 2000 in 13 slices of 160)
    a, w = t["ts.mean"], W("ts_attn.weight")
    m = _gemm(a, w, W("ts_attn.bias")) + _f64(a[:, 160:320]) @ _f64(w[:, 160:320]).T
    _must_fail("GEMM: one split-K slice added twice (K 2000)", "ts.logits", "M", m, refs["ts.logits"])
    # K = 600 (phase head's hidden layer: 576 + 24) and its partial N tile (100 = 64 + 36), on the GRU's layer-1 output
    gsd = pkg.synth.make_gru_state_dict()
    x, cp = pkg.synth.make_gru_inputs(4, 64)
    src = tc.HostSource(x=x, cparams=cp)
    grefs = {stage: ref for stage, _, ref in tc.gru_walk(oracle, gsd, src, 4, 64)}
    a, w, bias = src.t["gru.l1"].reshape(-1, 600), gsd["phase_mlp.0.weight"], gsd["phase_mlp.0.bias"]
    _must_fail("GEMM: K tail beyond the last full 32 dropped (K 600)", "gru.hid_phase", "S", _gemm(a[:, :576], w[:, :576], bias), grefs["gru.hid_phase"])
    m = _gemm(a, w, bias)
    m[:, 64:] -= _f64(bias)[64:]
    _must_fail("GEMM: bias missing in the last partial N tile (N 100)", "gru.hid_phase", "S", m, grefs["gru.hid_phase"])


def _flash(qkv, rows, key_range, scale=None, skip_rescale_block=None, dup_key=None, heads=4):
    """The blocked kernel's arithmetic for one key range in float64: 32-key blocks, running maximum m (base 2), l and O; optional faults.
    -> O (rows, E) unnormalised, m (rows, H), l (rows, H)."""
    qkv = _f64(qkv)
    E = qkv.shape[-1] // 3
    dh = E // heads
    scale = LOG2E / np.sqrt(dh) if scale is None else scale
    keys = list(range(*key_range))
    if dup_key is not None:
        keys.append(dup_key)
    O, M, L = np.zeros((len(rows), E)), np.zeros((len(rows), heads)), np.zeros((len(rows), heads))
    for h in range(heads):
        q = qkv[rows, h * dh:(h + 1) * dh] * scale
        m, l, o = np.full(len(rows), -np.inf), np.zeros(len(rows)), np.zeros((len(rows), dh))
        for j, k0 in enumerate(range(0, len(keys), 32)):
            kk = keys[k0:k0 + 32]
            s = q @ qkv[kk, E + h * dh:E + (h + 1) * dh].T
            m_new = np.maximum(m, s.max(-1))
            alpha = np.exp2(m - m_new)
            p = np.exp2(s - m_new[:, None])
            l = l * alpha + p.sum(-1)
            o = o * (1.0 if j == skip_rescale_block else alpha[:, None]) + p @ qkv[kk, 2 * E + h * dh:2 * E + (h + 1) * dh]
            m = m_new
        O[:, h * dh:(h + 1) * dh], M[:, h], L[:, h] = o, m, l
    return O, M, L


def _norm(O, L):
    return O / np.repeat(L, O.shape[-1] // L.shape[-1], -1)


def test_temporal_attention_mutants_fail(pkg, oracle, ts385):
    sd, t, refs = ts385
    qkv, rows, ref = t["ts.qkv_t"][0], np.arange(385), refs["ts.x_t"][0]
    O, M, L = _flash(qkv, rows, (0, 385))
    assert tc.rel_err(_norm(O, L), ref) < 1e-12                  # the blocked arithmetic itself is the reference's
    _must_fail("temporal attention: the clip's last key unread (n 385)", "ts.x_t", "M", _norm(*_flash(qkv, rows, (0, 384))[::2]), ref)
    _must_fail("temporal attention: one key counted twice", "ts.x_t", "M", _norm(*_flash(qkv, rows, (0, 385), dup_key=200)[::2]), ref)
    _must_fail("temporal attention: one block's accumulator not rescaled", "ts.x_t", "M", _norm(*_flash(qkv, rows, (0, 385), skip_rescale_block=3)[::2]), ref)
    _must_fail("temporal attention: scale 1/sqrt(256)", "ts.x_t", "M", _norm(*_flash(qkv, rows, (0, 385), scale=LOG2E / 16.0)[::2]), ref)
    # parts merged with exp() where the stored maxima are base 2
    parts = [_flash(qkv, rows, kr) for kr in oracle.ts_key_part_ranges(385, 3)]
    top = np.max([p[1] for p in parts], 0)
    for name, f, fails in (("exp2", np.exp2, False), ("exp", np.exp, True)):
        w = [f(p[1] - top) for p in parts]
        merged = _norm(sum(p[0] * np.repeat(wp, 250, -1) for p, wp in zip(parts, w)), sum(p[2] * wp for p, wp in zip(parts, w)))
        if fails:
            _must_fail("temporal attention: parts merged with exp, maxima base 2", "ts.x_t", "M", merged, ref)
        else:
            assert tc.rel_err(merged, ref) < 1e-12
    # the same faults seen in ONE part's (O, m, l): the last part without the clip's last key
    kr = oracle.ts_key_part_ranges(385, 3)
    po = np.stack([_norm(*_flash(qkv, rows, (k0, k1 - (p == 2)))[::2]) for p, (k0, k1) in enumerate(kr)])[:, None]
    _must_fail("temporal attention: last key unread, in the last part's O / l", "ts.part_o", "M", po, refs["ts.part_o"])
    lse = np.stack([(lambda r: r[1] + np.log2(r[2]))(_flash(qkv, rows, (k0, k1 - (p == 2)))) for p, (k0, k1) in enumerate(kr)])[:, None]
    _must_fail("temporal attention: last key unread, in the last part's m + log2 l", "ts.part_lse", "M", lse, refs["ts.part_lse"])


def test_temporal_attention_last_key_unread_at_10000_frames_fails(pkg, oracle):
    """One key of 10 000: the production size (on the 1 024 sampled rows; the GPU test checks every row, of which these are a part)."""
    sd = pkg.synth.make_tsattn_state_dict()
    x, _ = pkg.synth.make_tsattn_inputs(1, 10000)
    qkv = np.asarray(oracle.linear(x.reshape(1, 10000, -1), sd["mulattn.qkv_t.weight"], sd["mulattn.qkv_t.bias"]), np.float32)
    rows = tc.sample_rows(10000)
    with oracle.float64():
        ref = oracle.ts_stage_temporal_attention(qkv, rows)
        mutant = oracle.ts_stage_temporal_attention(qkv, rows, key_range=(0, 9999))
    tc.check_stage("ts.x_t", "L", np.asarray(oracle.ts_stage_temporal_attention(qkv, rows), np.float32), ref)
    _must_fail("temporal attention: the clip's last key unread (n 10000)", "ts.x_t", "L", mutant, ref)


def test_spatial_attention_and_gate_mutants_fail(pkg, oracle, ts385):
    sd, t, refs = ts385
    z = _f64(t["ts.qkv_s"][0]).reshape(385, 3, 4, 10, 25)
    q, k, v = z[:, 0], z[:, 1], z[:, 2]

    def spatial(scale=1.0, transpose=False):
        s = np.einsum("rhct,rhcu->rhtu", q, k) * scale
        e = np.exp(s - s.max(-1, keepdims=True))
        o = np.einsum("rhtu,rhcu->rhct", e / e.sum(-1, keepdims=True), v)
        return (o.transpose(0, 1, 3, 2) if transpose else o).reshape(385, 1000)

    assert tc.rel_err(spatial(), refs["ts.x_s"][0]) < 1e-12
    _must_fail("spatial attention: scores scaled by 1/sqrt(10)", "ts.x_s", "M", spatial(scale=1 / np.sqrt(10.0)), refs["ts.x_s"][0])
    _must_fail("spatial attention: output index t*10+c instead of c*25+t", "ts.x_s", "M", spatial(transpose=True), refs["ts.x_s"][0])
    both = np.concatenate([_f64(t["ts.x_t"]), _f64(t["ts.x_s"])], -1)
    assert tc.rel_err(both.sum(1) / 385, refs["ts.mean"]) < 1e-12
    _must_fail("gate: mean divided by n rounded up to 128", "ts.mean", "M", both.sum(1) / 512, refs["ts.mean"])
    _must_fail("gate: last partial 128-row block dropped", "ts.mean", "M", both[:, :384].sum(1) / 385, refs["ts.mean"])
    lg = _f64(t["ts.logits"])
    a0, a1 = lg[:, :1000], lg[:, 1000:]                          # pairs (e, e + 1000) instead of (2e, 2e + 1)
    w0 = 1.0 / (1.0 + np.exp(a1 - a0))
    _must_fail("gate: pairs (e, e+1000) instead of (2e, 2e+1), x_t", "ts.x_t_gated", "M", _f64(t["ts.x_t"]) * w0[:, None], refs["ts.x_t_gated"])
    _must_fail("gate: pairs (e, e+1000) instead of (2e, 2e+1), x_s", "ts.x_s_gated", "M", _f64(t["ts.x_s"]) * (1 - w0)[:, None], refs["ts.x_s_gated"])


def _ln(z, g, b, ddof=1, eps_under_root=False):
    z = _f64(z)
    mean, var = z.mean(-1, keepdims=True), z.var(-1, keepdims=True, ddof=ddof)
    den = np.sqrt(var + 1e-6) if eps_under_root else np.sqrt(var) + 1e-6
    return _f64(g) * ((z - mean) / den) + _f64(b)


def test_layer_norm_and_jwff_mutants_fail(pkg, oracle, ts385):
    sd, t, refs = ts385
    z = _f64(t["x"]) + (_f64(t["ts.y_t"]) + _f64(t["ts.y_s"]))
    assert tc.rel_err(_ln(z, sd["norm1.gamma"], sd["norm1.beta"]), refs["ts.x1"]) < 1e-12
    _must_fail("LayerNorm: biased std", "ts.x1", "M", _ln(z, sd["norm1.gamma"], sd["norm1.beta"], ddof=0), refs["ts.x1"])
    # eps under the root: invisible on unit-variance rows (5e-7), so the LayerNorm checks also run on the low-variance case
    unit = _ln(z, sd["norm1.gamma"], sd["norm1.beta"], eps_under_root=True)
    assert tc.rel_err(unit, refs["ts.x1"]) < tc.bar("ts.x1", "M")
    lsd, x, xs = tc.low_variance_case(pkg)
    src = tc.HostSource(x=x.reshape(1, 16, -1), xs=xs.reshape(1, 16, -1))
    lrefs = {stage: ref for stage, _, ref in tc.ts_walk(oracle, lsd, src, 1, 16, 1)}
    _must_fail("LayerNorm 1: eps under the root (low-variance rows)", "ts.x1", "LN", _ln(src.t["x"], lsd["norm1.gamma"], lsd["norm1.beta"], eps_under_root=True),
               lrefs["ts.x1"])
    _must_fail("LayerNorm 2: eps under the root (low-variance rows)", "ts.out", "LN", _ln(src.t["ts.x1"], lsd["norm2.gamma"], lsd["norm2.beta"], eps_under_root=True),
               lrefs["ts.out"])
    _must_fail("LayerNorm 2: biased std (low-variance rows)", "ts.out", "LN", _ln(src.t["ts.x1"], lsd["norm2.gamma"], lsd["norm2.beta"], ddof=0), lrefs["ts.out"])
    # JWFF with the tanh form of GELU
    x1 = _f64(t["ts.x1"][0])
    w1, w2 = _f64(sd["ffn.jwff_layer1.weight"])[0, :, :, :, 0, 0], _f64(sd["ffn.jwff_layer2.weight"])[0, :, :, :, 0, 0]
    from scipy.special import erf
    for name, gelu, fails in (("erf", lambda u: 0.5 * u * (1 + erf(u / np.sqrt(2.0))), False),
                              ("tanh", lambda u: 0.5 * u * (1 + np.tanh(np.sqrt(2 / np.pi) * (u + 0.044715 * u ** 3))), True)):
        hdn = gelu(np.einsum("rcj,ocj->roj", x1.reshape(385, 128, 24), w1))
        out = _ln(np.einsum("roj,poj->rpj", hdn, w2).reshape(385, -1) + x1, sd["norm2.gamma"], sd["norm2.beta"])
        if fails:
            _must_fail("JWFF: tanh-form GELU", "ts.out", "M", out, refs["ts.out"][0])
        else:
            assert tc.rel_err(out, refs["ts.out"][0]) < 1e-12


# ------------------------------------------------------------------------------------------------- GRU
def _gru_dir(gi, w_hh, b_hh, reverse, fault=None):
    """One GRU direction in float64 with an optional fault: "bhn_outside" (b_hn added outside r * (...)), "swap_zr", "stale" (at one step the units 8 .. 15 of
    the hidden state that the matrix product reads are those of the step before: a missed hand-off of one 8-unit slice)."""
    gi, w, bh = _f64(gi), _f64(w_hh).T, _f64(b_hh)
    b, T, _ = gi.shape
    H = w.shape[0]
    h, prev, out = np.zeros((b, H)), np.zeros((b, H)), np.empty((b, T, H))
    sig = lambda u: 1 / (1 + np.exp(-u))
    for i, tt in enumerate(range(T - 1, -1, -1) if reverse else range(T)):
        hin = h.copy()
        if fault == "stale" and i == T // 2:
            hin[:, 8:16] = prev[:, 8:16]
        g, gh = gi[:, tt], hin @ w
        r, z = sig(g[:, :H] + gh[:, :H] + bh[:H]), sig(g[:, H:2 * H] + gh[:, H:2 * H] + bh[H:2 * H])
        if fault == "swap_zr":
            r, z = z, r
        n = np.tanh(g[:, 2 * H:] + r * gh[:, 2 * H:] + bh[2 * H:]) if fault == "bhn_outside" else np.tanh(g[:, 2 * H:] + r * (gh[:, 2 * H:] + bh[2 * H:]))
        prev, h = h, (1 - z) * n + z * h
        out[:, tt] = h
    return out


def test_gru_recurrence_mutants_fail(pkg, oracle):
    sd = pkg.synth.make_gru_state_dict()
    x, cp = pkg.synth.make_gru_inputs(3, 257)
    src = tc.HostSource(x=x, cparams=cp)
    refs = {stage: ref for stage, _, ref in tc.gru_walk(oracle, sd, src, 3, 257)}

    def layer0(fault):
        return np.concatenate([_gru_dir(src.t[f"gru.gi0{d}"], sd[f"rnn.weight_hh_l0{suf}"], sd[f"rnn.bias_hh_l0{suf}"], bool(d), fault if d == 0 else None)
                               for d, suf in enumerate(("", "_reverse"))], -1)

    assert tc.rel_err(layer0(None), refs["gru.l0"]) < 1e-12
    _must_fail("GRU: b_hn outside r*(...)", "gru.l0", "M", layer0("bhn_outside"), refs["gru.l0"])
    _must_fail("GRU: z and r swapped", "gru.l0", "M", layer0("swap_zr"), refs["gru.l0"])
    _must_fail("GRU: one step's hand-off stale for one 8-unit slice", "gru.l0", "M", layer0("stale"), refs["gru.l0"])


# ------------------------------------------------------------------------------------------------- corrector
def test_corrector_mutants_fail(pkg, oracle):
    p = "pfeat_corrector."
    sd = pkg.synth.make_featcorr_state_dict()
    x, _ = pkg.synth.make_featcorr_inputs(1, 16)
    cam, bbox, cimg = tc.make_gait_inputs(pkg, 1, 16)
    src = tc.HostSource(x=x, cam=cam, bbox=bbox, cimg=cimg)
    refs = {stage: ref for stage, _, ref in tc.fc_walk(oracle, sd, src, 1, 16, 1)}
    avg, ph = _f64(src.t["gru.avg"]), _f64(src.t["gru.phase"])
    W = lambda k: _f64(sd[p + k])

    def hidden(swap_norms=False, slope=0.05):
        n1, n2 = np.linalg.norm(ph[..., :2], axis=-1, keepdims=True), np.linalg.norm(ph[..., 2:], axis=-1, keepdims=True)
        if swap_norms:
            n1, n2 = n2, n1
        raw = np.concatenate([np.broadcast_to(avg[:, None], (1, 16, 3)), ph[..., :2] / n1, ph[..., 2:] / n2], -1).reshape(16, 7)
        lrelu = lambda u: np.where(u > 0, u, slope * u)
        hs = lrelu(raw @ W("gfeat_mpl_s.0.weight").T + W("gfeat_mpl_s.0.bias"))
        return lrelu(raw @ W("gfeat_mpl_t.0.weight").T + W("gfeat_mpl_t.0.bias")), hs @ W("gfeat_mpl_s.3.weight").T + W("gfeat_mpl_s.3.bias")

    assert tc.rel_err(hidden()[0], refs["fc.hid_t"]) < 1e-12 and tc.rel_err(hidden()[1], refs["fc.g_s"]) < 1e-12
    _must_fail("corrector: phase pair normalised by the other pair's norm, hid_t", "fc.hid_t", "S", hidden(swap_norms=True)[0], refs["fc.hid_t"])
    _must_fail("corrector: phase pair normalised by the other pair's norm, g_s", "fc.g_s", "S", hidden(swap_norms=True)[1], refs["fc.g_s"])
    _must_fail("corrector: LeakyReLU slope 0.01, hid_t", "fc.hid_t", "S", hidden(slope=0.01)[0], refs["fc.hid_t"])
    _must_fail("corrector: LeakyReLU slope 0.01, g_s", "fc.g_s", "S", hidden(slope=0.01)[1], refs["fc.g_s"])
    z = _f64(src.t["x"]).reshape(16, -1) + _f64(src.t["fc.g_t"]).reshape(16, -1)
    bn = lambda eps: (z - W("bn_in.running_mean")) / np.sqrt(W("bn_in.running_var") + eps) * W("bn_in.weight") + W("bn_in.bias")
    assert tc.rel_err(bn(1e-5), refs["fc.y"]) < 1e-12
    _must_fail("corrector: BatchNorm eps 1e-3", "fc.y", "S", bn(1e-3), refs["fc.y"])
    # gait_cparams with the box taken as 224 wide (the case the module-level test is confined to)
    c, bb, ci = _f64(cam).reshape(-1, 3), _f64(bbox).reshape(-1, 4), _f64(cimg).reshape(-1, 2)
    assert tc.rel_err(np.concatenate([bb[:, 2:3] / 224 * c[:, :1], (bb[:, :2] - ci) / (bb[:, 2:3] / 224 * c[:, :1]) / 112 + c[:, 1:]], -1), refs["fc.cparams"]) < 1e-12
    _must_fail("corrector: cparams with the box width taken as 224", "fc.cparams", "S",
               np.concatenate([c[:, :1], (bb[:, :2] - ci) / c[:, :1] / 112 + c[:, 1:]], -1), refs["fc.cparams"])
