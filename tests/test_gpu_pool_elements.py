"""The attention pooling and the range-softmax merge that finishes it, element by element against float64 ("attention pooling, per element"):
attn_pool_kernel on an fp32 handle, attn_pool_bf16x_kernel<12> on a bf16 handle, then the front of head_tail_kernel<true>, through the single-op hook
grnet_op_attention_pool on maps the test supplies -- the forward's own launches on a workspace of the call.

The rule (tests/helpers/pool_checks.py): every element of point_local_feat (n,128,24) and cam_shape_feats (n,64,24), none left out, within
accepted x 2^-24 x mag of the float64 pooling of exactly the fp32 values the kernel was given (a bf16 handle: values rounded to bf16 first, so the
conversion in front of the kernel changes nothing); mag = sum_p w |f| (1 + |h - max|); an element of magnitude 0 exactly 0.  accepted = max(4, 4 x
yardstick), the yardstick the larger of two independent fp32 evaluations on the same maps (the reference's order; the kernel's stated arithmetic),
never the GPU's own result.  tests/test_pool_checks_cpu.py plants thirteen faults that the bar of before (1e-4 of the tensor's maximum) lets through.

Per data kind and handle: a call on other data first (the workspace holds stale partials and range statistics), the checked call of 3 frames, frame 0
alone (its rows of the call of 3, bit for bit), the call again (every bit), and the background channel filled with NaN and with +inf (no bit changes).
Every pool_bounds line is printed before anything is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from .helpers import pool_checks as pc

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(kernel, name, seed=pc.CASE_SEED):
    key = (kernel, name, seed)
    if key not in _CASES:
        _CASES[key] = pc.make_case(name, seed=seed, bf16=kernel == "bf16")
    return _CASES[key]


@pytest.fixture(scope="module", params=["f32", "bf16"])
def handle(request, pkg):
    m = pkg.build_synthetic_model(max_frames=2, with_gru=False, dtype=request.param)
    yield request.param, m
    m.close()


def _pool(m, heat, fa, fb):
    plf, csf = m.op_attention_pool(*(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (heat, fa, fb)))
    return {"point_local_feat": plf.cpu().numpy(), "cam_shape_feats": csf.cpu().numpy()}


def _same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in pc.OUTPUTS)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_attention_pooling_per_element(handle, name):
    kernel, m = handle
    case, other = _case(kernel, name), _case(kernel, "x8_signed" if name != "x8_signed" else "x1", seed=pc.OTHER_SEED)
    heat, fa, fb = case["heat"], case["fa"], case["fb"]
    _pool(m, other["heat"], other["fa"], other["fb"])                       # stale partials, maxima and sums in the workspace of the next call
    got3 = _pool(m, heat, fa, fb)
    got1 = _pool(m, heat[:1], fa[:1], fb[:1])
    again = _pool(m, heat, fa, fb)
    held = []
    for n, got, frames in ((3, got3, slice(None)), (1, got1, slice(0, 1))):
        for output, res, yard, accepted, place in pc.check(kernel, case, got, frames):
            print(pc.bounds_line(kernel, name, n, output, res, yard, accepted, place))
            held.append((n, output, res, accepted))
    background = {}
    for fill in (np.nan, np.inf):
        h = heat.copy()
        h[:, 0] = fill
        background[str(fill)] = _same_bits(_pool(m, h, fa, fb), got3)
    for n, output, (ratio, at), accepted in held:
        assert accepted <= pc.FACTOR * pc.YARD_CEILING[kernel], (kernel, name, n, output, accepted, "the yardstick left fp32's range: this bar holds nothing")
        assert ratio <= accepted, (kernel, name, n, output, ratio, at, accepted)
    assert _same_bits({k: v[:1] for k, v in got3.items()}, got1), "frame 0 alone differs from its rows in the call of 3"
    assert _same_bits(again, got3), "a second run does not repeat every bit"
    assert all(background.values()), f"the background channel reaches a result: {background}"


def test_hook_refuses_bad_arguments_and_writes_nothing(handle, pkg):
    kernel, m = handle
    case = _case(kernel, "x1")
    heat, fa, fb = (torch.from_numpy(case[k][:1]).cuda() for k in ("heat", "fa", "fb"))
    plf, csf = torch.full((1, 128, 24), 7.0, device="cuda"), torch.full((1, 64, 24), 7.0, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    good = [m._h, ptr(heat), ptr(fa), ptr(fb), 1, ptr(plf), ptr(csf), stream]
    for i in (0, 1, 2, 3, 5, 6):
        args = list(good)
        args[i] = None
        assert m._lib.grnet_op_attention_pool(*args) == -22, i
    for n in (0, -3):
        args = list(good)
        args[4] = n
        assert m._lib.grnet_op_attention_pool(*args) == -22, n
    torch.cuda.synchronize()
    assert bool((plf == 7.0).all()) and bool((csf == 7.0).all())
    assert m._lib.grnet_op_attention_pool(*good) == 0
    torch.cuda.synchronize()
    assert not bool((plf == 7.0).any())
    raw = pkg.GRNet(max_frames=1, dtype=kernel)                             # no weights: the tail behind the merge has nothing to read
    try:
        with pytest.raises(pkg._lib.GrnetError, match="before grnet_finalize_weights"):
            raw.op_attention_pool(heat, fa, fb)
    finally:
        raw.close()
