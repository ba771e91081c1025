"""Every launch of the temporal branch (csrc/gru_kernels.hip, tsattn_kernels.hip, featcorr_kernels.hip) against a float64 reference of that launch on the
launch's OWN input -- the method of tests/test_gpu_f32_stages.py for the per-frame path.

The inputs and outputs of the launches are the taps of ONE production call (grnet_temporal_taps: device-to-device copies enqueued between the production
launches; the scratch itself cannot be read afterwards -- x_t is gated in place, the key-part partials share memory with y_t | y_s | x1, the GRU's gi becomes
the heads' hidden buffer).  For every checked call: a call of the same size on OTHER data runs first (stale scratch holds different numbers), the armed
call's outputs are compared bit for bit with the unarmed call's, the plan (grnet_tsattn_plan: which attention kernel, how many key parts) is asserted
BEFORE the checks so that a plan change cannot move a check onto another kernel, and each stage is compared with oracle/grnet_oracle.py's float64 stage
function on the tapped fp32 input (tests/helpers/temporal_checks.py: walkers, metrics, bars).

Bars: 8 x the rounding floor of the plain fp32 restatement of the stage (measured on a CPU, table FLOORS in tests/helpers/temporal_checks.py, tool
tools/temporal_stage_floors.py), never above the module bars 5e-5 / 1e-4 / 3e-5.  Floors, bars and the errors measured on an MI355X per stage and size:
profiles/temporal_stage_errors.md.  tests/test_temporal_stage_checks_cpu.py shows that each check fails on a subtly wrong stage.

Clips of 17 000 and 32 768 frames are checked on 1 024 query rows (first / last 16, both sides of 32 random query-tile seams, random rows; selected on the
device); the clip mean always over every frame; every query at 10 000 frames.
"""
import re

import numpy as np
import pytest
import torch

from .helpers import temporal_checks as tc

pytestmark = pytest.mark.gpu

OTHER_SEED = 4242                                                # the data of the call that runs before each checked call


_report = tc.report


def _tapped(m, pkg, call, call_other, same):
    """other data -> unarmed call -> other data -> armed call.  The armed call is first given a one-float buffer: refused up front with the size needed.
    `same(a, b)` compares two results bit for bit.  -> (result, taps {name: tensor}, gemms [(M, N, K, slices)])."""
    call_other()
    plain = call()
    call_other()
    tiny = torch.empty(1, dtype=torch.float32, device="cuda")
    m.arm_temporal_taps(tiny)
    with pytest.raises(pkg._lib.GrnetError, match=r"copies \d+ floats: nothing was enqueued") as refusal:
        call()
    need = int(re.search(r"copies (\d+) floats", str(refusal.value)).group(1))
    buf = torch.empty(need, dtype=torch.float32, device="cuda")
    m.arm_temporal_taps(buf)
    armed = call()
    torch.cuda.synchronize()
    taps = m.temporal_taps(buf)
    _, gemms = m.temporal_tap_layout()
    assert sum(int(np.prod(t.shape)) for t in taps.values()) == need, "the size the refusal names is the size the armed call copies"
    same(armed, plain)
    again = call()                                               # the arming held for ONE call: this one copies nothing and equals both
    torch.cuda.synchronize()
    same(again, plain)
    return armed, taps, gemms


def _run_checks(walk, cls_of, label):
    """Walk the stages, print every figure, then assert: all failing stages are named at once."""
    log, bad, seen = [], [], []
    for stage, got, ref in walk:
        seen.append(stage)
        try:
            tc.check_stage(stage, cls_of(stage), got, ref, log, label)
        except AssertionError as e:
            bad.append(str(e))
    _report(log)
    assert not bad, "\n".join(bad)
    return seen


def _expect_plan(m, n):
    """The plan of a clip of n frames, asserted against what the launcher's rules give on THIS device (its CU count), not against 256 CUs."""
    plan = m.tsattn_plan(n)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if n < 384:
        assert plan == {"kernel": "per_query", "parts": 1, "key_blocks": 0, "lds_bytes": (512 + n) * 4}, (n, plan)
    else:
        assert plan == {"kernel": "blocked", "parts": tc.flash_key_parts(n, cus), "key_blocks": (n + 31) // 32, "lds_bytes": 2 * 32 * (258 + 260) * 4}, (n, plan)
        assert 1 <= plan["parts"] <= 8
    return plan


def _single_part_clip(m):
    """The shortest clip from 7 169 frames up that the blocked kernel takes in ONE key part on this device (it then normalises and stores itself)."""
    for n in range(7169, 32769):
        if m.tsattn_plan(n)["parts"] == 1:
            return n
    raise AssertionError("no clip of 7 169 .. 32 768 frames runs the blocked kernel in one key part on this device")


@pytest.fixture(scope="module")
def ts_model(pkg):
    m = pkg.build_synthetic_model(max_frames=2, with_gru=True, with_tsattn=True, use_gait_feat=False)
    yield m
    m.close()


TS_CASES = [(4, 64), (1, 16), (1, 1), (1, 383), (1, 384), (2, 1100), (1, 10000), (1, "single_part"), (1, 17000), (1, 32768)]


def _ts_case(m, pkg, oracle, sd, b, n, x, xs, cls, label):
    plan = _expect_plan(m, n)
    g = np.random.Generator(np.random.Philox(key=[OTHER_SEED, n]))
    xd, xsd = torch.from_numpy(x).cuda(), torch.from_numpy(xs).cuda()
    od = torch.from_numpy(g.standard_normal((b, n, 128, 24), dtype=np.float32)).cuda()
    osd = torch.cat([od, torch.from_numpy(g.standard_normal((b, n, 128, 1), dtype=np.float32)).cuda()], -1)
    y, taps, gemms = _tapped(m, pkg, lambda: m.tsattn_forward(xd, xsd), lambda: m.tsattn_forward(od, osd), lambda a, c: _assert_same(a, c))
    del od, osd
    assert ("ts.part_o" in taps) == (plan["parts"] > 1), "per-part (O, m, l) are tapped exactly when the keys were split"
    t = {k[3:]: v for k, v in taps.items()}
    src = {"ts." + k: v.reshape(b, n, -1) for k, v in t.items() if k not in ("mean", "logits", "part_o", "part_ml")}
    src.update({"ts.mean": t["mean"], "ts.logits": t["logits"], "x": xd.reshape(b, n, -1), "xs": xsd.reshape(b, n, -1)})
    if plan["parts"] > 1:
        src["ts.part_o"] = t["part_o"].reshape(plan["parts"], b, n, -1)
        src["ts.part_ml"] = t["part_ml"].reshape(plan["parts"], b, n, 4, 2)
    assert torch.equal(src["ts.out"], y), "the last tap is the call's output"
    rows = tc.sample_rows(n) if n > 10000 else None
    seen = _run_checks(tc.ts_walk(oracle, sd, tc.TapSource(src), b, n, plan["parts"], rows), lambda s: cls, label)
    want = ["qkv_t", "qkv_s"] + (["part_o", "part_lse"] if plan["parts"] > 1 else []) + ["x_t", "x_s", "mean", "logits", "x_t_gated", "x_s_gated", "y_t", "y_s",
                                                                                          "x1", "out"]
    assert seen == ["ts." + k for k in want]
    return plan, gemms


def _assert_same(a, b):
    if isinstance(a, dict):
        for k in a:
            assert torch.equal(a[k], b[k]), f"{k}: the armed call's output differs from the unarmed call's"
    elif isinstance(a, (tuple, list)):
        for u, v in zip(a, b):
            assert torch.equal(u, v), "the armed call's output differs from the unarmed call's"
    else:
        assert torch.equal(a, b), "the armed call's output differs from the unarmed call's"


@pytest.mark.parametrize("b,n", TS_CASES, ids=[f"{b}x{n}" for b, n in TS_CASES])
def test_attention_block_every_launch_against_float64(pkg, oracle, ts_model, b, n):
    """tsattn_forward launch by launch: both qkv GEMMs, the temporal attention (per-query kernel below 384 frames, the blocked kernel from there on; for split
    clips each part's (O, m, l) against the float64 partial softmax over that part's key range, which isolates the blocked kernel from the combine kernel, then
    the merged x_t), the spatial attention, the clip mean, the gate logits, the gated x_t / x_s, both output GEMMs, LN1 and JWFF + LN2.
    4 x 64: the 4-tracks job; 1 x 16: split-K GEMMs (47 row blocks); 1 x 1; 383 / 384: the two sides of the kernel switch; 2 x 1 100: a ragged query tile of 76
    rows, a last key block of 12, two clips; 1 x 10 000: production (4 parts of 78/78/78/79 blocks on 256 CUs, last key block and last query tile of 16), every
    query checked; single_part: the shortest clip from 7 169 frames on whose plan has one part (the blocked kernel's own normalise-and-store way out);
    17 000 (non-periodic input) and 32 768 (the advertised limit; parts of at most 4 096 keys: in ONE part its x_t was off by 7.5e-6 against a bar of 3.2e-6,
    NOTES_rejected.md section 13): 1 024 sampled query rows."""
    m = ts_model
    if n == "single_part":
        n = _single_part_clip(m)
    sd = pkg.synth.make_tsattn_state_dict()
    x, xs = pkg.synth.make_tsattn_inputs(b, n)
    plan, _ = _ts_case(m, pkg, oracle, sd, b, n, x, xs, tc.size_class("ts", n), f"ts {b}x{n}")
    if n == 17000:
        assert plan["key_blocks"] == 532


def test_attention_sizes_cover_both_kernels_and_one_intermediate_and_eight_key_parts(ts_model):
    """The sizes of the test above, by the plan query on this device: the per-query kernel and the blocked one; among the blocked clips one key part, an
    intermediate count and eight."""
    m = ts_model
    sizes = [n if n != "single_part" else _single_part_clip(m) for _, n in TS_CASES]
    plans = {n: _expect_plan(m, n) for n in sizes}
    _report([f"plan {n:6d}: {plans[n]}" for n in sizes])
    assert {p["kernel"] for p in plans.values()} == {"per_query", "blocked"}
    assert plans[383]["kernel"] == "per_query" and plans[384]["kernel"] == "blocked"
    parts = {p["parts"] for p in plans.values() if p["kernel"] == "blocked"}
    assert 1 in parts and 8 in parts and any(1 < p < 8 for p in parts), parts


def test_layer_norms_on_low_variance_rows(pkg, oracle):
    """LN1 and LN2 on rows of standard deviation 1e-3, where the reference's (std + eps) and nn.LayerNorm's sqrt(var + eps) differ by 40 % -- on the unit-variance
    rows of every other case they differ by 5e-7, which no fp32 check can see.  An attention block with zero fc_t / fc_s / JWFF weights, so that LN1 normalises
    x itself and LN2 x1 (tests/helpers/temporal_checks.py: low_variance_case)."""
    sd, x, xs = tc.low_variance_case(pkg)
    m = pkg.GRNet(max_frames=2, device_id=0, dtype="f32", use_gait_feat=False)
    try:
        full = pkg.synth.make_state_dict()
        full.update({"tsattn." + k: v for k, v in sd.items()})
        m.load_state_dict(full, strict=True)
        m.load_smpl(pkg.synth.make_smpl_tables())
        m.finalize()
        _ts_case(m, pkg, oracle, sd, 1, 16, x, xs, "LN", "ts LN 1x16")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------- GRU
@pytest.fixture(scope="module")
def gru_model(pkg):
    m = pkg.build_synthetic_model(max_frames=2, with_gru=True)
    yield m
    m.close()


GRU_CASES = [(1, 16, 3), (4, 64, 3), (16, 9, 3), (3, 257, 3), (3, 257, 0), (1, 2000, 3), (1, 10000, 3)]


def _gru_src(taps, b, T, x, cp):
    src = {k: (v.reshape(b, T, -1) if v.shape[0] == b * T and k not in ("gru.hfin", "gru.hid_speed", "gru.hid_step", "gru.avg") else v)
           for k, v in taps.items() if k.startswith("gru.")}
    src.update({"x": x, "cparams": cp})
    return src


@pytest.mark.parametrize("b,T,mode", GRU_CASES, ids=[f"{b}x{T}_mode{mode}" for b, T, mode in GRU_CASES])
def test_gru_every_launch_against_float64(pkg, oracle, gru_model, b, T, mode):
    """gru_forward launch by launch: xc / xin, each of the four gi GEMMs, each layer's recurrence on the GPU's own gi of that layer (both directions), the final
    hidden states, each head's hidden GEMM and mlp_out.  Default recurrence (GRNET_OPT_GRU_MODE 3: eight workgroups per (sequence, direction), v_exp / v_rcp
    gates) and, once at 3 x 257, mode 0 (one workgroup per (sequence, direction), libm gates)."""
    m = gru_model
    m.set_option(pkg._lib.OPT_GRU_MODE, mode)
    try:
        sd = pkg.synth.make_gru_state_dict()
        x, cp = pkg.synth.make_gru_inputs(b, T)
        ox, ocp = pkg.synth.make_gru_inputs(b, T, seed=OTHER_SEED)
        xd, cpd, oxd, ocpd = (torch.from_numpy(a).cuda() for a in (x, cp, ox, ocp))
        (y, ph, xc), taps, _ = _tapped(m, pkg, lambda: m.gru_forward(xd, cpd), lambda: m.gru_forward(oxd, ocpd), _assert_same)
        assert torch.equal(taps["gru.avg"], y) and torch.equal(taps["gru.phase"].reshape(ph.shape), ph) and torch.equal(taps["gru.xc"].reshape(xc.shape), xc)
        cls = tc.size_class("gru", T)
        seen = _run_checks(tc.gru_walk(oracle, sd, tc.TapSource(_gru_src(taps, b, T, xd, cpd)), b, T), lambda s: cls, f"gru {b}x{T} m{mode}")
        assert seen == ["gru." + k for k in ("xc", "xin", "gi00", "gi01", "l0", "gi10", "gi11", "l1", "hfin", "hid_speed", "hid_step", "hid_phase", "avg", "phase")]
    finally:
        m.set_option(pkg._lib.OPT_GRU_MODE, 3)


# ------------------------------------------------------------------------------------------------- corrector
@pytest.fixture(scope="module")
def fc_model(pkg):
    m = pkg.build_synthetic_model(max_frames=64, use_gait_feat=True)
    yield m
    m.close()


FC_CASES = [(1, 16), (4, 64), (1, 10000)]


def _fc_call(m, b, n, x, cam, bbox, cimg):
    csf = torch.zeros(b * n, 64, 24, device="cuda")
    keep = ("point_local_feat", "pred_avg", "pred_phase", "pred_cparam", "theta")
    return lambda: {k: v for k, v in m.gait_correct(x.reshape(b * n, 128, 24), csf, cam.reshape(b * n, 3), bbox, cimg, b, n).items() if k in keep}


def _fc_tapped(m, pkg, b, n):
    x, _ = pkg.synth.make_featcorr_inputs(b, n)
    cam, bbox, cimg = tc.make_gait_inputs(pkg, b, n)
    assert not np.any(bbox[..., 2] == 224.0) and not np.any(bbox[..., :2] == cimg), "boxes that are not 224 wide and not centred"
    ox, ocam = pkg.synth.make_featcorr_inputs(b, n, seed=OTHER_SEED)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xd, camd, bbd, cid = d(x), d(cam), d(bbox), d(cimg)
    out, taps, gemms = _tapped(m, pkg, _fc_call(m, b, n, xd, camd, bbd, cid), _fc_call(m, b, n, d(ox), d(ocam), bbd, cid), _assert_same)
    return out, taps, gemms, dict(x=xd, cam=camd, bbox=bbd, cimg=cid)


@pytest.mark.parametrize("b,n", FC_CASES, ids=[f"{b}x{n}" for b, n in FC_CASES])
def test_corrector_every_launch_against_float64(pkg, oracle, fc_model, b, n):
    """gait_correct launch by launch: gait_cparams_kernel on boxes that are neither 224 wide nor centred, the GRU on (x, cparams), gfeat_hidden_kernel (hid_t,
    g_s), the 1536 -> 3072 GEMM (g_t), featcorr_bn_kernel (y, y_s), the attention block on (y, y_s) and the final residual.  At 1 x 10 000 the attention block's
    row-wise stages and the residual are checked on 1 024 sampled rows (every query of a 10 000-frame clip is checked by the attention block's own test)."""
    m = fc_model
    plan = _expect_plan(m, n)
    out, taps, _, inp = _fc_tapped(m, pkg, b, n)
    sd = pkg.synth.make_featcorr_state_dict()
    assert torch.equal(taps["fc.out"].reshape(out["point_local_feat"].shape), out["point_local_feat"]) and torch.equal(taps["fc.att"], taps["ts.out"])
    assert torch.equal(taps["fc.cparams"], out["pred_cparam"]) and torch.equal(taps["gru.avg"], out["pred_avg"])
    src = _gru_src(taps, b, n, inp["x"], None)
    for k, v in taps.items():
        if k.startswith("fc.") or (k.startswith("ts.") and k not in ("ts.mean", "ts.logits", "ts.part_o", "ts.part_ml")):
            src[k] = v.reshape(b, n, -1)
    src.update({"ts.mean": taps["ts.mean"], "ts.logits": taps["ts.logits"], **inp})
    if plan["parts"] > 1:
        src["ts.part_o"] = taps["ts.part_o"].reshape(plan["parts"], b, n, -1)
        src["ts.part_ml"] = taps["ts.part_ml"].reshape(plan["parts"], b, n, 4, 2)
    rows = tc.sample_rows(n) if n > 2000 else None
    seen = _run_checks(tc.fc_walk(oracle, sd, tc.TapSource(src), b, n, plan["parts"], rows), lambda s: tc.size_class(s.split(".")[0], n), f"fc {b}x{n}")
    for k in ("fc.cparams", "gru.l1", "gru.phase", "fc.hid_t", "fc.g_s", "fc.g_t", "fc.y", "fc.y_s", "ts.x_t", "ts.out", "fc.out"):
        assert k in seen, k


# ------------------------------------------------------------------------------------------------- GEMM census
GEMM_SHAPES = {(3000, 3072): "qkv_t", (3000, 3200): "qkv_s", (2000, 2000): "gate logits", (3072, 1000): "fc_t / fc_s", (900, 3072): "gi, layer 0",
               (900, 600): "gi, layer 1", (100, 1200): "speed / step hidden", (100, 600): "phase hidden", (3072, 1536): "g_t"}
# shapes whose row counts in the branch reach both sides of launch_gemm_nt_bias's split rule (fewer than 128 tiles of 64 x 64 and K >= 512: split-K);
# the gate logits and the speed / step heads have one row per clip and always split
BOTH_WAYS = [(3000, 3072), (3000, 3200), (3072, 1000), (900, 3072), (900, 600), (100, 600), (3072, 1536)]


def test_gemm_census_every_shape_split_and_unsplit(pkg, ts_model, gru_model, fc_model):
    """From the tap layouts of armed calls at sizes the tests above check: launch_gemm_nt_bias ran every (N, K) shape of the branch -- K tails 1000, 1200, 600,
    2000 (8, 16, 24, 16 of a 32-chunk), partial N tiles 100, 900, 3000 -- and each shape both with and without split-K where the branch's call sizes reach both."""
    runs = set()

    def layout(m, call):
        call()                                                   # (sizes the handle has not seen allocate scratch: not in the armed call)
        buf = torch.empty(1, dtype=torch.float32, device="cuda")
        m.arm_temporal_taps(buf)
        with pytest.raises(pkg._lib.GrnetError) as r:
            call()
        buf = torch.empty(int(re.search(r"copies (\d+) floats", str(r.value)).group(1)), dtype=torch.float32, device="cuda")
        m.arm_temporal_taps(buf)
        call()
        torch.cuda.synchronize()
        for (M, N, K, slices) in m.temporal_tap_layout()[1]:
            runs.add((N, K, slices > 1))

    for b, n in ((1, 16), (4, 64)):
        assert (b, n) in TS_CASES and (b, n) in FC_CASES
        x, xs = pkg.synth.make_tsattn_inputs(b, n)
        xd, xsd = torch.from_numpy(x).cuda(), torch.from_numpy(xs).cuda()
        layout(ts_model, lambda: ts_model.tsattn_forward(xd, xsd))
        cam, bbox, cimg = tc.make_gait_inputs(pkg, b, n)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        layout(fc_model, _fc_call(fc_model, b, n, d(pkg.synth.make_featcorr_inputs(b, n)[0]), d(cam), d(bbox), d(cimg)))
    for b, T in ((1, 16), (1, 2000), (1, 10000)):
        assert (b, T, 3) in GRU_CASES
        x, cp = pkg.synth.make_gru_inputs(b, T)
        xd, cpd = torch.from_numpy(x).cuda(), torch.from_numpy(cp).cuda()
        layout(gru_model, lambda: gru_model.gru_forward(xd, cpd))
    _report([f"gemm N {N:5d} K {K:5d} {'split-K' if sp else 'one slice'}" for N, K, sp in sorted(runs)])
    assert {(N, K) for N, K, _ in runs} == set(GEMM_SHAPES), {(N, K) for N, K, _ in runs} ^ set(GEMM_SHAPES)
    for shape in GEMM_SHAPES:
        assert (shape + (True,)) in runs, f"{GEMM_SHAPES[shape]} never ran split-K"
    for shape in BOTH_WAYS:
        assert (shape + (False,)) in runs, f"{GEMM_SHAPES[shape]} never ran in one slice"
