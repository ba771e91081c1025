"""tests/helpers/fuse_checks.py, the float64 yardstick of the fp32 fuse layers, checked without a GPU:

- the launch list is the plan's: 42 launches per forward -- 26 stride-2 convolutions of the down chains (10 of them merged first links), 8 grouped
  up launches, 8 finishing convolutions -- and 39 down-chain taps;
- a plain fp32 composition of every launch of a 2-, 3- and 4-branch layer passes the rule on its own tapped inputs, on the synthetic weights as
  they are and with uneven_fuse_state_dict; a channel whose every term is dead equals x_i bit for bit;
- the planted faults, each on the fp32 composition's own result on uneven weights: every one fails the rule where where() says, and every one but
  one passes rel_err < 2e-5, the only bar the fuse layers had (a whole loud channel left linear is the one that bar does see);
- the per-channel-ReLU and list-of-addends forms of forward_check / epilogue equal the old forms where both apply;
- uneven_fuse_state_dict edits the weight and bias of exactly 62 BatchNorms and nothing else."""
import numpy as np
import pytest

from .helpers import conv_checks as cc
from .helpers import fuse_checks as fc

KEY = (130, 4)
N = 2
PREFIX = {2: "backbone.stage2.0.", 3: "backbone.stage3.1.", 4: "backbone.stage4.0."}


def _branches(nb, key=(131, 1)):
    """post-ReLU N(0,1) branch outputs, as BasicBlocks leave them"""
    g = np.random.Generator(np.random.Philox(key=list(key)))
    return [np.maximum(g.standard_normal((N, fc.BR[b], 56 >> b, 56 >> b)), 0.0).astype(np.float32) for b in range(nb)]


@pytest.fixture(scope="module")
def state_dicts(synth_weights):
    return {"even": synth_weights, "uneven": fc.uneven_fuse_state_dict(synth_weights, KEY)}


def test_launch_list_is_the_plans():
    kinds = [L for _, _, nb in fc.modules() for L in fc.fuse_launches(nb)]
    down = [L for L in kinds if L["kind"] == "down"]
    assert len(kinds) == 42 and len(down) == 26 and sum(len(L["segs"]) > 1 for L in down) == 10
    assert sum(L["kind"] == "up" for L in kinds) == 8 and sum(L["kind"] == "finish" for L in kinds) == 8
    assert sum(len(fc.down_taps(nb)) for _, _, nb in fc.modules()) == 39 and fc.down_taps(2) == []
    first = fc.fuse_launches(4)[0]
    assert first["segs"] == [(1, 0, 0), (2, 0, 0), (3, 0, 0)] and first["taps"] == ["d1.0.0", "d2.0.0", "d3.0.0"] and first["x"] == "x0"
    mask = fc.relu_mask(first["segs"])
    assert mask.shape == (128,) and not mask[:64].any() and mask[64:].all()              # relu_from = 64
    fin = fc.fuse_launches(4)[-1]
    assert fin["residual"] == ["x3", "d3.0.2", "d3.1.1"] and fin["x"] == "x2" and fin["tap"] == "y3"
    up = fc.fuse_launches(4)[-2]["outputs"]
    assert [o["extras"] for o in up] == [[], ["d1.0.0"], ["d2.0.1", "d2.1.0"]] and [len(o["sources"]) for o in up] == [3, 2, 1]


@pytest.mark.parametrize("nb", [2, 3, 4])
@pytest.mark.parametrize("weights", ["even", "uneven"])
def test_fp32_compositions_pass_the_rule(state_dicts, weights, nb):
    w = fc.FuseWeights(state_dicts[weights], PREFIX[nb])
    xs = _branches(nb)
    for up in ("torch", "sequential"):
        taps = fc.fp32_taps(nb, w, xs, up)
        for L in fc.fuse_launches(nb):
            for name, fam, form, got, res, i in fc.check_launch(L, w, taps):
                print(fc.bounds_line(f"cpu {weights} nb={nb} up={up}", name, fam, form, res, fc.where(res[1], i, nb)))
                assert res[0] <= res[2] and res[4] == max(fc.FACTOR, fc.FACTOR * res[2]), (name, res)   # it is one of the yardstick's own evaluations
                assert res[0] <= res[4], (name, res)
        if weights == "uneven":
            for i in range(nb):                                        # every term of channel 0 is exactly 0, the shift included
                assert np.array_equal(taps[f"y{i}"][:, 0], taps[f"x{i}"][:, 0])


@pytest.fixture(scope="module")
def stage4(state_dicts):
    w = fc.FuseWeights(state_dicts["uneven"], PREFIX[4])
    xs = _branches(4)
    return w, xs, fc.fp32_taps(4, w, xs)


def _flagged(name, old, res, bar, place):
    print(f"{name:105s} rel_err {old:8.2g}   per-element {res[0]:10.3g} = {res[0] / bar:9.3g} x accepted ({bar:.1f})  FLAGGED at {res[1]} {place}")


def test_planted_faults_in_the_up_launch(stage4):
    """Output 0 of the stage-4 layer: three sources, bands of 8 rows, one band = one row of the 7x7 source."""
    w, xs, _ = stage4
    f32 = lambda a: np.asarray(a, np.float32)
    sources = [(xs[j], *w.up(0, j), 1 << j) for j in (1, 2, 3)]
    terms = [cc.torch_fp32(x, f32(w64)[:, :, None, None]) + f32(sh)[None, :, None, None] for x, w64, sh, _ in sources]
    pre = fc.fuse_up_fp32(xs[0], [], sources, relu=False)["torch"]
    ref, mag = fc.fuse_up_reference(xs[0], [], sources), fc.fuse_up_reference(xs[0], [], sources, mag=True)
    clean, _, y, _, bar = fc.fuse_up_check(np.maximum(pre, 0), xs[0], [], sources)
    assert clean <= bar and cc.rel_err(np.maximum(pre, 0), ref) < fc.OLD_BAR
    s_out = cc.output_scales(32)
    for name in fc.UP_FAULTS:
        bad = np.maximum(fc.plant(name, pre, terms=terms, base=xs[0]), 0)
        assert not np.array_equal(bad, np.maximum(pre, 0)), name
        old, res = cc.rel_err(bad, ref), fc.ratio(bad, ref, mag)
        place = fc.where(res[1], 0, 4, s_out)
        _flagged(name, old, res, bar, place)
        assert old < fc.OLD_BAR, (name, old)
        assert res[0] >= 2 * bar, (name, res, bar)
        k = int(name.split()[0])
        assert place.startswith("dead-term channel" if k == 6 else "mid channel+border" if k == 10 else "quiet channel"), (name, place)
        if k == 1:
            assert res[1][2] == 8 and "band seam" in place and "source seam" in place, (res, place)
        if k == 5:
            assert res[1][0] == 0, res
        if k == 6:
            assert res[0] == np.inf


def test_planted_faults_in_the_merged_and_finishing_launches(stage4):
    w, xs, taps = stage4
    first, fin = fc.fuse_launches(4)[0], fc.fuse_launches(4)[-1]
    # the merged first links from branch 0: 64 linear channels (the whole chain of output 1), then 2 x 32 ReLU'd
    ws, shifts = zip(*(w.down(s) for s in first["segs"]))
    w64, sh64, mask = np.concatenate(ws), np.concatenate(shifts), fc.relu_mask(first["segs"])
    relu_from = int(np.argmax(mask))
    assert relu_from == 64
    lin = cc.epilogue(cc.torch_fp32(xs[0], w64.astype(np.float32), 2), sh64.astype(np.float32))
    out = cc.apply_relu(lin, mask)
    assert np.array_equal(out, np.concatenate([taps[t] for t in first["taps"]], 1))
    ref, mag = cc.conv_reference(xs[0], w64, sh64, 2, None, mask), cc.conv_magnitude(xs[0], w64, sh64, 2)
    clean, _, y, _, bar = cc.forward_check("direct", out, xs[0], w64, sh64, 2, None, mask)
    assert clean <= bar
    s_out = np.concatenate([cc.output_scales(64), np.ones(64)])
    for name in fc.MERGED_FAULTS:
        bad = fc.plant(name, out, lin=lin, relu_from=relu_from)
        old, res = cc.rel_err(bad, ref), fc.ratio(bad, ref, mag)
        place = cc.where(res[1], "direct", {}, 28, s_out)
        _flagged(name, old, res, bar, place)
        assert res[0] >= 2 * bar, (name, res, bar)
        if name.startswith("7"):
            assert old < fc.OLD_BAR and res[1][1] == relu_from - 1 and place.startswith("quiet channel"), (name, old, res, place)
        else:                      # a whole loud channel without its ReLU is wrong by the size of the tensor: the one fault rel_err sees as well
            assert old >= fc.OLD_BAR and res[1][1] == relu_from, (name, old, res)
    # the finishing convolution of output 3: three addends
    w64, sh64 = w.down(fin["seg"])
    adds = [taps[r] for r in fin["residual"]]
    pre = cc.epilogue(cc.torch_fp32(xs[2], w64.astype(np.float32), 2), sh64.astype(np.float32), adds)
    assert np.array_equal(np.maximum(pre, 0), taps["y3"])
    ref, mag = cc.conv_reference(xs[2], w64, sh64, 2, adds, True), cc.conv_magnitude(xs[2], w64, sh64, 2, adds)
    clean, _, y, _, bar = cc.forward_check("direct", taps["y3"], xs[2], w64, sh64, 2, adds, True)
    assert clean <= bar
    for name in fc.FINISH_FAULTS:
        bad = np.maximum(fc.plant(name, pre, addend=adds[1]), 0)
        old, res = cc.rel_err(bad, ref), fc.ratio(bad, ref, mag)
        place = cc.where(res[1], "direct", {}, 7, cc.output_scales(256))
        _flagged(name, old, res, bar, place)
        assert old < fc.OLD_BAR and res[0] >= 2 * bar and place.startswith("quiet channel") and res[1][0] == 0, (name, old, res, bar, place)


def test_new_forms_of_forward_check_equal_the_old_ones():
    d = cc.make_inputs("uneven", (132, 1), 2, 24, 32, 3, 14, 2)
    x, w64, b64, r = d["x"], cc.widen(d["w"]), cc.widen(d["bias"]), d["residual"]
    lin = cc.torch_fp32(x, d["w"], 2)
    for relu in (False, True):
        mask = np.full(32, relu)
        assert cc.forward_check("direct", lin, x, w64, b64, 2, r, relu) == cc.forward_check("direct", lin, x, w64, b64, 2, [r], mask)
        assert cc.forward_check("direct", lin, x, w64, b64, 2, None, relu) == cc.forward_check("direct", lin, x, w64, b64, 2, [], mask)
        assert np.array_equal(cc.epilogue(lin, d["bias"], r, relu), cc.epilogue(lin, d["bias"], [r], mask))
        assert np.array_equal(cc.conv_reference(x, w64, b64, 2, r, relu), cc.conv_reference(x, w64, b64, 2, [r], mask))
    assert np.array_equal(cc.conv_magnitude(x, w64, b64, 2, r), cc.conv_magnitude(x, w64, b64, 2, [r]))
    # a mask is ReLU on its channels only; addends are added in the listed order in fp32, their absolute values in the magnitude
    mask = np.arange(32) >= 16
    y = cc.epilogue(lin, d["bias"], None, mask)
    assert np.array_equal(y[:, :16], cc.epilogue(lin, d["bias"])[:, :16]) and np.array_equal(y[:, 16:], cc.epilogue(lin, d["bias"], None, True)[:, 16:])
    assert (y[:, :16] < 0).any()
    big, r2 = np.full_like(r, 1e8), np.full_like(r, -1e8)
    assert np.array_equal(cc.epilogue(lin, None, [big, r2]), (lin + big) + r2) and not np.array_equal(cc.epilogue(lin, None, [big, r2]), lin)
    assert np.allclose(cc.conv_magnitude(x, w64, None, 2, [big, r2]), cc.conv_magnitude(x, w64, None, 2) + 2e8)
    assert np.allclose(cc.conv_reference(x, w64, None, 2, [big, r2]), cc.conv_reference(x, w64, None, 2))


def test_uneven_state_dict_edits_exactly_the_last_batchnorms(synth_weights, state_dicts):
    sd, un = synth_weights, state_dicts["uneven"]
    bns = fc.last_batchnorms()
    assert len(bns) == len({b for b, _ in bns}) == 62
    edited = {b + f for b, _ in bns for f in (".weight", ".bias")}
    assert set(un) == set(sd) and edited <= set(sd)
    changed = {k for k in sd if np.asarray(un[k]).tobytes() != np.asarray(sd[k]).tobytes()}
    assert changed == edited, (sorted(changed - edited)[:3], sorted(edited - changed)[:3])
    assert all(np.asarray(un[k]).dtype == np.asarray(sd[k]).dtype and np.shape(un[k]) == np.shape(sd[k]) for k in sd)
    scales = fc.term_scales(KEY)
    assert "backbone.stage4.1.fuse_layers.3.0.2.1" in scales and "backbone.stage3.0.fuse_layers.0.2.1" in scales
    seen = set()
    for (bn, i), s in zip(bns, scales.values()):
        sp = cc.special_channels(fc.BR[i])
        assert s.shape == (fc.BR[i],) and s.max() <= 1 and s[0] == 0 and (s[1:] > 0).all()
        assert (s[list(sp["quiet"])] <= 1e-5).all() and s[sp["mid"]] <= 1e-3
        seen |= set(np.round(-np.log10(np.delete(s, [0, sp["mid"], *sp["quiet"]]))).astype(int).tolist())
        assert not un[bn + ".weight"][0] and not un[bn + ".bias"][0]
        w64, shift = cc.fold_bn(un[bn[:-1] + "0.weight"], *(un[bn + f] for f in fc.BN_FIELDS))
        assert not w64[0].any() and shift[0] == 0                                    # the dead channel: the folded shift too
    assert seen == {0, 1, 2, 3}
    assert fc.uneven_fuse_state_dict(sd, KEY)[bns[5][0] + ".weight"].tobytes() == un[bns[5][0] + ".weight"].tobytes()
    assert fc.uneven_fuse_state_dict(sd, (130, 5))[bns[5][0] + ".weight"].tobytes() != un[bns[5][0] + ".weight"].tobytes()


def test_where_names_the_place():
    s = cc.output_scales(32)
    assert fc.where((0, 0, 5, 5), 0, 4, s) == "dead-term channel+interior"
    assert fc.where((0, 31, 8, 5), 0, 4, s) == "quiet channel+band seam+source seam"
    assert fc.where((0, 9, 3, 55), 0, 4, s) == "mid channel+border"
    assert fc.where((0, 3, 5, 16), 0, 4, s) == "loud channel+source seam" and fc.where((0, 3, 5, 17), 0, 4) == "interior"
    assert fc.where((0, 3, 4, 5), 1, 4) == "band seam+source seam" and fc.where((0, 3, 2, 5), 1, 3) == "source seam"
    assert fc.where((0, 3, 2, 3), 2, 4) == "band seam+source seam" and fc.where((0, 3, 3, 3), 3, 4) == "interior"


def test_silent_state_dict_lowers_the_bias_in_front_of_every_branch_output(synth_weights):
    sd, si = synth_weights, fc.silent_branch_state_dict(synth_weights)
    bns = fc.last_block_batchnorms()
    assert len(bns) == 2 + 4 * 3 + 3 * 4 and fc.silenced_channels(32) == (16, 9) and fc.silenced_channels(256) == (240, 65)
    changed = {k for k in sd if np.asarray(si[k]).tobytes() != np.asarray(sd[k]).tobytes()}
    assert changed == {bn + ".bias" for bn, _ in bns}
    for bn, b in bns:
        d = si[bn + ".bias"].astype(np.float64) - sd[bn + ".bias"]
        on = list(fc.silenced_channels(fc.BR[b]))
        assert np.allclose(d[on], fc.SILENCE, atol=1e-2) and not np.delete(d, on).any()
        # the ReLU behind it (BasicBlock: relu(bn2(conv2) + x)) then writes 0 whatever the forward feeds it, up to activations of 1e3
        _, shift = cc.fold_bn(si[bn[:-3] + "conv2.weight"], *(si[bn + f] for f in fc.BN_FIELDS))
        assert (shift[on] < -9e3).all()
