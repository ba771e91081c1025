"""The cross-lane hand-offs of the four-lane forward with the reduced wait set (csrc/lane_deps.h).  The reduction may not change a bit: a missing
edge shows as a differing bit in some forward, not as a fault.  Per call size
(fp32: 1, 5 -- a partial 4-image row tile on the 7x7 layers -- and 16 frames; bf16: 16 and 64 frames, below and on the frame-resident kernel groups)
the reference is the SAME handle with GRNET_OPT_MULTI_LANE = 0, all launches one after another on one stream."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("theta", "verts", "kp_3d", "kp_2d", "rotmat", "point_local_feat", "cam_shape_feats", "features")
SHAPES = {"theta": (85,), "verts": (6890, 3), "kp_3d": (29, 3), "kp_2d": (29, 2), "rotmat": (24, 3, 3), "point_local_feat": (128, 24),
          "cam_shape_feats": (64, 24), "features": (480, 56, 56)}
CASES = [("f32", 1), ("f32", 5), ("f32", 16), ("bf16", 16), ("bf16", 64)]
BACK_TO_BACK = 20


@pytest.fixture(scope="module")
def handles(pkg):
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = pkg.build_synthetic_model(max_frames=16 if dtype == "f32" else 64, with_gru=False, dtype=dtype)
        return made[dtype]

    yield get
    for m in made.values():
        m.close()


def _new_outputs(n):
    return {k: torch.empty((n,) + SHAPES[k], dtype=torch.float32, device="cuda") for k in KEYS}


def _forward_into(pkg, m, x, outs):
    """grnet_forward on the current stream into caller-owned buffers: no allocation, no host synchronisation"""
    o = pkg._lib.Outputs()
    for k, t in outs.items():
        setattr(o, k, t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = m._lib.grnet_forward(m._h, C.c_void_p(x.data_ptr()), x.shape[0], C.byref(o), stream)
    pkg._lib.check(m._lib, m._h, rc, "grnet_forward")


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in KEYS)


def _differing(a, b):
    return [k for k in KEYS if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]


@pytest.fixture(scope="module")
def references(pkg, handles):
    """Per case, computed once and left unchanged: the frames and the outputs of the one-stream forward"""
    made = {}

    def get(dtype, n):
        if (dtype, n) not in made:
            m = handles(dtype)
            x = torch.from_numpy(np.ascontiguousarray(pkg.synth.make_frames(n))).cuda()
            m.set_option(pkg._lib.OPT_USE_GRAPH, 0)
            m.set_option(pkg._lib.OPT_MULTI_LANE, 0)
            ref = _new_outputs(n)
            _forward_into(pkg, m, x, ref)
            torch.cuda.synchronize()
            m.set_option(pkg._lib.OPT_MULTI_LANE, 1)
            assert all(bool(torch.isfinite(ref[k]).all()) for k in KEYS) and float(ref["verts"].abs().max()) > 0
            made[(dtype, n)] = (x, ref)
        return made[(dtype, n)]

    return get


@pytest.mark.parametrize("dtype,n", CASES)
def test_eager_lanes_match_one_stream_back_to_back(pkg, handles, references, dtype, n):
    """20 eager four-lane forwards enqueued with no host synchronisation in between, each into its own buffers: every one of them equals the
    one-stream forward bit for bit (forward k+1's side lanes start behind forward k's end through the fork alone where a join was dropped)."""
    m = handles(dtype)
    x, ref = references(dtype, n)
    m.set_option(pkg._lib.OPT_USE_GRAPH, 0)
    m.set_option(pkg._lib.OPT_MULTI_LANE, 1)
    outs = [_new_outputs(n) for _ in range(BACK_TO_BACK)]
    for o in outs:
        for t in o.values():
            t.fill_(float("nan"))
    torch.cuda.synchronize()
    for o in outs:
        _forward_into(pkg, m, x, o)
    torch.cuda.synchronize()
    bad = {i: _differing(o, ref) for i, o in enumerate(outs) if not _same_bits(o, ref)}
    assert not bad, f"{dtype} n={n}: forwards that differ from the one-stream forward: {bad}"


@pytest.mark.parametrize("dtype,n", CASES)
def test_graph_replay_matches_one_stream(pkg, handles, references, dtype, n):
    """The captured forward takes its edges from the same reduced Op::waits: first sight of the key runs eager, the second captures and replays,
    the third replays into buffers wiped in between."""
    m = handles(dtype)
    x, ref = references(dtype, n)
    m.set_option(pkg._lib.OPT_MULTI_LANE, 1)
    m.set_option(pkg._lib.OPT_USE_GRAPH, 1)
    try:
        out = _new_outputs(n)
        for rep in range(3):
            for t in out.values():
                t.fill_(float("nan"))
            _forward_into(pkg, m, x, out)
            torch.cuda.synchronize()
            assert _same_bits(out, ref), f"{dtype} n={n}: pass {rep} (0 eager, 1 capture + replay, 2 replay) differs in {_differing(out, ref)}"
    finally:
        m.set_option(pkg._lib.OPT_USE_GRAPH, 0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_plan_keeps_fewer_waits_than_edges(handles, dtype):
    c = handles(dtype).plan_counts()
    print(dtype, c)
    # the invariant: the reduction drops waits, never adds one, and an event is recorded only for a kept wait
    assert c["ops"] > 100 and 1 <= c["lanes_all"] <= 3, c
    assert 0 < c["waits"] < c["waits_all"], c
    assert 0 < c["records"] <= c["waits"] and c["records"] <= c["records_all"], c
    assert c["lanes_joined"] <= c["lanes_all"], c
    # the figures DESIGN.md section 4.2 quotes for these two plans (max_frames 16 / 64).  They follow the plan and the lane scheduler: a change to
    # either moves them although the reduction is right -- update them here and in DESIGN.md together
    quoted = {"f32": dict(ops=289, waits_all=79, records_all=66, waits=54, records=52, lanes_all=3, lanes_joined=0),
              "bf16": dict(ops=316, waits_all=79, records_all=57, waits=67, records=52, lanes_all=3, lanes_joined=0)}[dtype]
    assert c == quoted, f"DESIGN.md section 4.2 quotes {quoted}, the plan now gives {c}: update both"
