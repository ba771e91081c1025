"""Every launch of the eight fp32 fuse layers, element by element, on weights that make a fault visible ("The fuse layers, per element").

On the synthetic weights all terms of a fuse output have one scale and x_i dominates, so a zeroed term, a row read one off or a tile of another frame
moves the output by 1e-6 of its maximum.  Here the handle is loaded with tests/helpers/fuse_checks.py uneven_fuse_state_dict: the last BatchNorm of
every fuse term is scaled per output channel (1 ... 1e-8, channel 0 exactly 0), so that at the pixels where post-ReLU x_i is 0 an output IS its small
terms -- and, because the forward's own x_i are positive almost everywhere, with silent_branch_state_dict, which makes every x_b exactly 0 on its first
quiet channel and on its 1e-3 channel (the second quiet channel and the dead one keep the forward's own x_b).  The call sizes are 1 and 3 distinct
frames (the network fixes the map sizes; 1 frame is the smallest grid, with 3 a tile of another frame shows), the checked forward follows a forward on other frames, and at 3 frames the launches are repeated under the tile hints 7 and 1171, which
grnet_tune may put on any direct launch.  Per module and launch, on the launch's own tapped inputs (grnet_debug_tensor; the down chains are tapped as
"<stage>.<m>.d<i>.<j>.<level>"): |got - float64| <= accepted x 2^-24 x magnitude with no element left out -- conv_checks.forward_check for the
stride-2 convolutions (a merged first link as ONE convolution, linear below relu_from; the finishing convolution with its list of addends),
fuse_checks.fuse_up_check for every output of hr_fuse_up_f32.  Everything is measured and printed before anything is asserted."""
import numpy as np
import pytest
import torch

from .helpers import conv_checks as cc
from .helpers import fuse_checks as fc
from .test_gpu_f32_stages import _forms_by_key, _hint_table

pytestmark = pytest.mark.gpu

KEY = (140, 1)
B = "backbone."
CASES = [(1, 0), (3, 0), (3, 7), (3, 1171)]


@pytest.fixture(scope="module")
def uneven(synth_weights):
    """uneven fuse terms, and branch outputs that are exactly 0 on two of the special channels (see silent_branch_state_dict for why)"""
    return fc.silent_branch_state_dict(fc.uneven_fuse_state_dict(synth_weights, KEY))


def _tap_names():
    return [f"{stage}.{m}.{t}" for stage, m, nb in fc.modules()
            for t in [f"x{b}" for b in range(nb)] + fc.down_taps(nb) + [f"y{b}" for b in range(nb)]]


def _taps(m, n):
    return {name: m.debug_tensor(name, n).cpu().numpy() for name in _tap_names()}


def _s_out(L):
    """the output_scales pattern of a launch's output channels: the chain's last BatchNorm is the scaled one"""
    if L["kind"] == "finish":
        return cc.output_scales(fc.BR[L["seg"][0]])
    return np.concatenate([cc.output_scales(fc.seg_shape(s)[0]) if not fc.seg_shape(s)[1] else np.ones(fc.seg_shape(s)[0]) for s in L["segs"]])


_RUNS = {}


def _run(pkg, synth_smpl, uneven, n, hint):
    """(launch forms by weight key, the fuse taps of the checked forward, the same taps of a second checked forward), once per case"""
    if (n, hint) in _RUNS:
        return _RUNS[n, hint]
    m = pkg.GRNet(max_frames=n)
    try:
        m.load_state_dict(uneven, strict=True)
        m.load_smpl(synth_smpl)
        m.finalize()
        if hint:
            _hint_table(pkg, m, n, hint)
        by_key = _forms_by_key({"kernels": m.conv_kernels(n), "forms": m.conv_launch_forms(n)})
        frames = pkg.synth.make_frames(2 * n)
        base, other = torch.from_numpy(frames[:n]).cuda(), torch.from_numpy(frames[n:]).cuda()
        m(other)                                                      # stale numbers in every buffer
        m(base)
        torch.cuda.synchronize()
        taps = _taps(m, n)
        m(base)
        torch.cuda.synchronize()
        again = _taps(m, n)
    finally:
        m.close()
    _RUNS[n, hint] = by_key, taps, again
    return _RUNS[n, hint]


@pytest.mark.parametrize("n,hint", CASES, ids=lambda v: str(v))
def test_every_fuse_launch_per_element_on_uneven_weights(pkg, synth_smpl, uneven, n, hint):
    by_key, taps, again = _run(pkg, synth_smpl, uneven, n, hint)
    held, under_hint = [], 0
    for stage, mi, nb in fc.modules():
        tag = f"{stage}.{mi}"
        w = fc.FuseWeights(uneven, f"{B}{tag}.")
        local = {t: taps[f"{tag}.{t}"] for t in [f"x{b}" for b in range(nb)] + [f"y{b}" for b in range(nb)] + fc.down_taps(nb)}
        for L in fc.fuse_launches(nb):
            if L["kind"] == "up":
                assert by_key[f"{B}{tag}.fuse_layers(up)"][1]["family"] == "fuse_up"
                form = {}
            else:
                name, form, _ = by_key[w.down_key(L["segs"][0] if L["kind"] == "down" else L["seg"])]
                assert name == "conv_direct_f32 3x3 s2" and form["family"] == "direct", (tag, L, name, form)
                under_hint += bool(hint) and form["hint"] == hint
            for name, fam, text, g, res, i in fc.check_launch(L, w, local, slice(None), form.get("family", "fuse")):
                place = fc.where(res[1], i, nb, cc.output_scales(fc.BR[i])) if L["kind"] == "up" else cc.where(res[1], fam, form, g.shape[2], _s_out(L))
                print(fc.bounds_line(f"uneven{n}" + f"h{hint}" * bool(hint), f"{tag}.{name}", fam, text, res, place))
                held.append((f"{tag}.{name}", res, place))
    dead = {f"{s}.{mi}.y{i}": (taps[f"{s}.{mi}.y{i}"][:, 0].view(np.int32) != taps[f"{s}.{mi}.x{i}"][:, 0].view(np.int32)).sum()
            for s, mi, nb in fc.modules() for i in range(nb)}
    differ = [k for k in taps if taps[k].tobytes() != again[k].tobytes()]
    alive = {k: float((taps[k] > 0).mean()) for k in ("stage4.2.y0", "stage4.2.y3")}
    worst = max(held, key=lambda h: h[1][0] / h[1][4])
    print(f"uneven fuse n={n} hint={hint}: {len(held)} checks, {under_hint} fuse convolutions under the hint, worst gpu / accepted "
          f"{worst[1][0] / worst[1][4]:.3f} at {worst[0]} {worst[1][1]} {worst[2]}; non-zero share {alive}")
    assert len(held) == 8 + 26 + sum(nb - 1 for _, _, nb in fc.modules())
    assert all(np.isfinite(v).all() for v in taps.values()) and min(alive.values()) > 0.1          # the forward stays finite and alive
    assert not hint or under_hint, f"hint {hint} ran on no fuse convolution at {n} frames"
    bad = [(name, res[0], res[1], res[4], place) for name, res, place in held if not res[0] <= res[4]]
    assert not bad, bad
    assert not any(dead.values()), {k: int(v) for k, v in dead.items() if v}    # channel 0: every term is dead, y_i = x_i bit for bit
    assert not differ, differ                                                   # a second forward: the same bits in every fuse tap


def test_the_forwards_own_data_exposes_the_planted_faults(pkg, synth_smpl, uneven):
    """What the edited weights are for: on the branch outputs the GPU itself produced (3 frames), output 0 of a stage-4 layer has two channels
    whose every element IS its small terms (x_0 exactly 0 there).  Each fault of the up launch (tests/test_fuse_checks_cpu.py) is planted into a
    plain fp32 composition on those tapped inputs, in each of the three stage-4 modules: every planted result passes rel_err < 2e-5, and every
    fault is at least 2 x outside the bar the kernel is held to in at least one module -- not in each: a silenced channel whose summed shift is
    negative is 0 behind the ReLU with or without the fault (the share of positive outputs is printed), and which channels those are is the
    weights' choice.  The kernel's own output on the same inputs is inside the bar in all three."""
    _, taps, _ = _run(pkg, synth_smpl, uneven, 3, 0)
    f32 = lambda a: np.asarray(a, np.float32)
    q, mid = fc.silenced_channels(32)
    best = {}
    for tag in ("stage4.0", "stage4.1", "stage4.2"):
        w = fc.FuseWeights(uneven, f"{B}{tag}.")
        xs = [taps[f"{tag}.x{b}"] for b in range(4)]
        sources = [(xs[j], *w.up(0, j), 1 << j) for j in (1, 2, 3)]
        terms = [cc.torch_fp32(x, f32(w64)[:, :, None, None]) + f32(sh)[None, :, None, None] for x, w64, sh, _ in sources]
        pre = fc.fuse_up_fp32(xs[0], [], sources, relu=False)["sequential"]
        ref, mag = fc.fuse_up_reference(xs[0], [], sources), fc.fuse_up_reference(xs[0], [], sources, mag=True)
        gpu, _, _, _, bar = fc.fuse_up_check(taps[f"{tag}.y0"], xs[0], [], sources)
        silent = all(not xs[b][:, list(fc.silenced_channels(fc.BR[b]))].any() for b in range(4))
        alive = {c: round(float((ref[:, c] > 0).mean()), 3) for c in (q, mid)}
        print(f"{tag}.y0: gpu {gpu:.3f} accepted {bar:.3f}; x_b silent on its two channels: {silent}; share of positive outputs there: {alive}; "
              f"pixels of the dead channel with x_0 = 0: {int((xs[0][:, 0] == 0).sum())}")
        assert gpu <= bar and silent, (tag, gpu, bar, silent)
        for name in fc.UP_FAULTS:
            if name.startswith("6") and (xs[0][0, 0] != 0).all():  # no element of the dead channel without a term: the rule can only see what a
                continue                                           # rounding of x_0 leaves; the bit-for-bit comparison of channel 0 sees all
            bad = np.maximum(fc.plant(name, pre, terms=terms, base=xs[0], quiet=q), 0)
            old, (new, at) = cc.rel_err(bad, ref), fc.ratio(bad, ref, mag)
            print(f"{name:105s} rel_err {old:8.2g}   per-element {new:10.3g} = {new / bar:9.3g} x accepted  at {at} {fc.where(at, 0, 4, cc.output_scales(32))}")
            assert old < fc.OLD_BAR, (tag, name, old)
            best[name] = max(best.get(name, 0.0), new / bar)
    assert set(best) == set(fc.UP_FAULTS) and min(best.values()) >= 2, best
