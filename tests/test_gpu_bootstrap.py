"""Step tables and bootstrap intervals on the GPU (grnet_gait_step_tables, grnet_bootstrap_table, csrc/gait_bootstrap_kernels.hip)
against the host statements pipeline.gait_step_tables and pipeline.bootstrap_table.  The generator is integers and the statistics are + - * / sqrt in
float64 in a fixed order, and the selection names one replicate, so EVERY OUTPUT BIT IS EQUAL, NaN patterns included: there is no tolerance anywhere
in this file.  The bootstrap's shapes (tests/helpers/bootstrap_checks.py's cases): one sequence of 0, 1, 2, 3 rows with B = 1, 63, 64, 65; four
sequences of 0, 1, 17 and 65 rows in a table of 80 with blocks of 1, 2, 17 and 100; 50 sequences of mixed counts, one of them alone; the caps (1 024
rows, 4 096 replicates, eight columns); NaN rows, an all-NaN column, equal values, equal negative values, a mean that crosses zero, samples of -0; a count above
max_rows.  The tables run on test_gpu_gait.py's calls (imported), on sequences of 1 to 4 frames, on a sequence past the LDS words, with max_rows = 4
and with a phase of gait_turns; the identities on the device's own gait, turn and balance outputs; every refusal; WindowBootstrap on a real handle."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

from .helpers import bootstrap_checks as bk
from .helpers import contact_checks as cc
from .helpers import gait_checks as gc
from . import test_gpu_gait as gg

pytestmark = pytest.mark.gpu
FPS = 20.0
CASES = ("one_n0_B1", "one_n0_B63", "one_n0_B64", "one_n0_B65", "one_n1_B1", "one_n1_B63", "one_n1_B64", "one_n1_B65", "one_n2_B1", "one_n2_B63", "one_n2_B64",
         "one_n2_B65", "one_n3_B1", "one_n3_B63", "one_n3_B64", "one_n3_B65", "four_block1", "four_block2", "four_block17", "four_block100", "fifty", "cap", "patterns",
         "patterns_block2", "negative_zeros", "count_above_max_rows")
TABLE_CASES = ("seven_w5", "seven_w1", "short", "long", "max_rows4", "turn")


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=1)
    yield m
    m.close()


def table_cases(pkg_name):
    """tests/helpers/bootstrap_checks.py's table cases; its seven sequences ARE test_gpu_gait.py's calls, which is asserted here."""
    for window in (5, 1):
        joints, _, _, lengths, _, table = gg.call(window, 25)
        mine, _, my_lengths, _ = gc.build_call(window, J=25, table=gc.KINECTV2)
        assert table == gc.KINECTV2 and lengths == my_lengths and np.array_equal(joints, mine) and gg.excursion(window) == bk.excursion(window)
    return bk.table_cases(pkg_name)


tables_statement = bk.tables_statement


def numpy_out(out, keys):
    assert sorted(out) == sorted(keys) and all(v.is_cuda for v in out.values())
    assert all(v.dtype == (torch.int32 if k == "counts" else torch.float64) for k, v in out.items())
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", CASES)
def test_bootstrap_equals_the_statement(model, pkg, name):
    assert CASES == tuple(c[0] for c in bk.cases())
    _, table, counts, kw = next(c for c in bk.cases() if c[0] == name)
    host = bk.statement(pkg.__name__, name)
    with_reps = numpy_out(model.bootstrap_table(table, counts, return_replicates=True, **kw), ("out", "replicates"))
    bk.compare(with_reps, host, name + ": ")
    without = numpy_out(model.bootstrap_table(table, counts, **kw), ("out",))
    bk.compare(without, host, name + " without replicates: ")
    print(f"{name}: f = {sorted(set(host['out'][..., 1].ravel().tolist()))[:6]}: equal bits")
    if name == "fifty":                                         # one of the fifty alone: the same bits
        q = 23                                                  # 40 rows, from the middle
        assert counts[q] == 40
        alone = numpy_out(model.bootstrap_table(table[q:q + 1], counts[q:q + 1], return_replicates=True, **kw), ("out", "replicates"))
        assert bk.same_bits(alone["out"][0], with_reps["out"][q]) and bk.same_bits(alone["replicates"][0], with_reps["replicates"][q])
        same = [i for i, n in enumerate(counts) if n == 40]
        assert len(same) >= 5                                   # equal n, equal indices: stated, and visible where the rows are equal too
        twice = np.concatenate([table[q:q + 1]] * 2)
        both = numpy_out(model.bootstrap_table(twice, [40, 40], **kw), ("out",))
        assert bk.same_bits(both["out"][0], both["out"][1])


@pytest.mark.parametrize("name", TABLE_CASES)
def test_step_tables_equal_the_statement(model, pkg, name):
    assert TABLE_CASES == tuple(c[0] for c in table_cases(pkg.__name__))
    _, events, rows, lengths, phase, max_rows, _ = next(c for c in table_cases(pkg.__name__) if c[0] == name)
    host = tables_statement(pkg.__name__, name)
    out = numpy_out(model.gait_step_tables(events, rows, lengths=lengths, fps=FPS, max_rows=max_rows, phase=phase, straight_only=phase is not None),
                    ("steps", "strides", "counts"))
    bk.compare_tables(out, host, name + ": ")
    print(f"{name}: steps and strides {host['counts'].tolist()}")
    if name == "max_rows4":
        assert (host["counts"][[0, 6]] > 4).all() and np.isfinite(host["steps"][0]).all()
    if name == "long":
        assert host["counts"][1, 0] > 380
    if name == "short":
        assert host["counts"].tolist() == [[0, 0], [1, 0], [2, 1], [2, 3]]
    if name == "turn":                                          # the phase alone, without straight_only, changes nothing
        plain = numpy_out(model.gait_step_tables(events, rows, lengths=lengths, fps=FPS, max_rows=max_rows, phase=phase), ("steps", "strides", "counts"))
        none = numpy_out(model.gait_step_tables(events, rows, lengths=lengths, fps=FPS, max_rows=max_rows), ("steps", "strides", "counts"))
        bk.compare_tables(plain, none)
        assert (plain["counts"][0] > out["counts"][0]).all() and plain["counts"][1].tolist() == out["counts"][1].tolist()


def test_identity_on_the_devices_own_outputs(model, pkg):
    """Replicate 0 of the device's tables IS the device's gait row, its turn row's straight columns and its balance row."""
    joints, lengths = bk.turning_case()
    j3 = torch.from_numpy(joints).cuda()
    gait = model.gait_parameters(j3, lengths=lengths, fps=FPS)
    turns = model.gait_turns(j3, gait["events"], gait["per_frame"], lengths=lengths, fps=FPS)
    at = list(bk.GAIT_ROW_AT)
    for phase, row in ((None, gait["per_sequence"].cpu().numpy()[:, at]), (turns["phase"], turns["per_sequence"].cpu().numpy()[:, [c + 7 for c in at]])):
        t = model.gait_step_tables(gait["events"], gait["per_frame"], lengths=lengths, fps=FPS, phase=phase, straight_only=phase is not None)
        a = model.bootstrap_table(t["steps"], t["counts"][:, 0], [3, 4, 5], B=1, quantiles=())["out"].cpu().numpy()[..., 0]
        b = model.bootstrap_table(t["strides"], t["counts"][:, 1], [3], B=1, quantiles=())["out"].cpu().numpy()[..., 0]
        got = np.concatenate([a[:, :, :2].reshape(2, 6), b[:, 0, :]], axis=1)
        assert np.isfinite(row).all() and bk.same_bits(got, row), (got.tolist(), row.tolist())
    made = [cc.planted_walker(T, *cc.WALKERS[i % 4], 0.3 + i, 0.4 * i) for i, T in enumerate((130, 400, 200))]
    lengths = [130, 400, 200]
    j3 = torch.from_numpy(np.concatenate(made)).cuda()
    events = model.gait_parameters(j3, lengths=lengths, fps=FPS)["events"]
    bal = model.gait_balance(j3, events, lengths=lengths, fps=FPS)
    counts = bal["per_sequence"][:, 1].to(torch.int32)
    out = model.bootstrap_table(bal["steps"], counts, [7, 8, 9, 11, 12], B=1, quantiles=())["out"].cpu().numpy()[..., 0]
    row = bal["per_sequence"].cpu().numpy()
    for q in range(3):
        assert row[q, 1] >= 5 and bk.same_bits(out[q, :, :2].ravel(), row[q, [4, 5, 6, 7, 8, 9, 14, 15, 16, 17]]), q


def test_refusals_leave_the_outputs_untouched(model, pkg):
    lib, h = pkg._lib.load(), model._h
    table = torch.ones(2, 8, 4, dtype=torch.float64, device="cuda")
    counts = torch.tensor([3, 8], dtype=torch.int32, device="cuda")
    out = torch.full((2, 2, 3, 5), -7.0, dtype=torch.float64, device="cuda")
    reps = torch.full((2, 2, 3, 10), -7.0, dtype=torch.float64, device="cuda")
    events = torch.zeros(8, dtype=torch.int32, device="cuda")
    rows = torch.zeros(8, 7, dtype=torch.float64, device="cuda")
    steps = torch.full((2, 4, 6), -7.0, dtype=torch.float64, device="cuda")
    strides = torch.full((2, 4, 4), -7.0, dtype=torch.float64, device="cuda")
    found = torch.full((2, 2), -7, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def boot(n_seq=2, max_rows=8, width=4, cols=(1, 3), n_cols=None, B=10, block=1, seed=0, draw=0, q=(250, 5000, 9750), n_q=None, null=None):
        args = [h, table.data_ptr(), counts.data_ptr(), n_seq, max_rows, width, (C.c_int32 * max(len(cols), 1))(*cols), len(cols) if n_cols is None else n_cols, B, block,
                seed, draw, (C.c_int32 * max(len(q), 1))(*q), len(q) if n_q is None else n_q, out.data_ptr(), reps.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_bootstrap_table(*args)

    def tables(offsets=(0, 3, 8), n_seq=None, fps=20.0, max_rows=4, phase=None, straight=0, null=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        args = [h, events.data_ptr(), rows.data_ptr(), off, len(offsets) - 1 if n_seq is None else n_seq, fps, max_rows, phase, straight, steps.data_ptr(),
                strides.data_ptr(), found.data_ptr(), stream]
        if null is not None:
            args[null] = None
        return lib.grnet_gait_step_tables(*args)

    nan, inf = float("nan"), float("inf")
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 2, 6, 12, 14)) + (
            (dict(n_seq=0), b"n_seq 0"), (dict(n_seq=8193), b"n_seq 8193"), (dict(n_seq=-1), b"n_seq -1"), (dict(max_rows=0), b"max_rows"), (dict(max_rows=1025), b"max_rows"),
            (dict(width=0), b"C outside"), (dict(width=17), b"C outside"), (dict(width=3), b"column"), (dict(cols=(1, -1)), b"column"), (dict(n_cols=0), b"n_cols"),
            (dict(cols=(0,) * 9), b"n_cols"), (dict(B=0), b"B outside"), (dict(B=4097), b"B outside"), (dict(block=0), b"block"), (dict(block=1025), b"block"),
            (dict(draw=-1), b"stream"), (dict(draw=65536), b"stream"), (dict(n_q=-1), b"n_q"), (dict(q=(0,) * 6), b"n_q"), (dict(q=(250, -1, 9750)), b"quantile"),
            (dict(q=(250, 10001, 9750)), b"quantile")):
        assert boot(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    for kw, word in tuple((dict(null=i), b"null") for i in (1, 2, 3, 9, 10, 11)) + (
            (dict(fps=0.0), b"fps"), (dict(fps=nan), b"fps"), (dict(fps=inf), b"fps"), (dict(max_rows=0), b"max_rows 0"), (dict(max_rows=1025), b"max_rows 1025"),
            (dict(straight=1), b"straight_only"), (dict(n_seq=0), b"n_seq 0"), (dict(n_seq=-2), b"n_seq -2"), (dict(offsets=(1, 8)), b"not 0"),
            (dict(offsets=(0, 5, 3)), b"increase"), (dict(offsets=(0, 4, 4)), b"empty")):
        assert tables(**kw) == pkg._lib.EINVAL, kw
        assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in (out, reps, steps, strides, found))                      # nothing was written
    assert boot() == 0 and tables() == 0                       # the same calls without a fault go through
    torch.cuda.synchronize()
    assert bool((out[:, :, 0, [0, 2, 3, 4]] == 1.0).all()) and bool((out[:, :, 1:, [0, 2, 3, 4]] == 0).all()) and bool((out[:, :, :, 1] == 10).all())      # a table of ones
    assert bool((reps[:, :, 0] == 1.0).all()) and found.tolist() == [[0, 0]] * 2 and bool(steps.isnan().all()) and bool(strides.isnan().all())
    assert boot(null=15) == 0 and boot(q=(), null=12) == 0     # replicates_dev may be null, and quantiles_host where n_q is 0
    torch.cuda.synchronize()
    t = np.ones((2, 8, 4))
    for kw, word in ((dict(table=np.ones((2, 8))), "table"), (dict(counts=[3]), "counts"), (dict(cols=[]), "cols"), (dict(cols=[0] * 9), "cols"), (dict(B=0), "B"),
                     (dict(B=4097), "B"), (dict(B=2.5), "whole"), (dict(quantiles=(1,) * 6), "quantiles"), (dict(seed=-1), "seed")):
        with pytest.raises(ValueError, match=word):
            model.bootstrap_table(**{**dict(table=t, counts=[3, 8], cols=[1], B=10), **kw})
    for kw, word in ((dict(cols=[4]), "column"), (dict(block=0), "block"), (dict(stream=65536), "stream"), (dict(quantiles=(10001,)), "quantile"),
                     (dict(table=np.ones((2, 1025, 4))), "max_rows"), (dict(table=np.ones((2, 8, 17))), "C outside")):
        with pytest.raises(pkg._lib.GrnetError, match=word):
            model.bootstrap_table(**{**dict(table=t, counts=[3, 8], cols=[1], B=10), **kw})
    ev, fr = np.zeros(8, np.int32), np.zeros((8, 7))
    for args, kw, word in (((ev, fr[:, :6]), {}, "per_frame"), ((ev[:7], fr), {}, "events"), ((ev, fr), dict(lengths=[3, 4]), "lengths"), ((ev, fr), dict(max_rows=0), "max_rows"),
                           ((ev, fr), dict(max_rows=1025), "max_rows"), ((ev, fr), dict(phase=ev[:7]), "phase"), ((ev, fr), dict(straight_only=True), "straight_only")):
        with pytest.raises(ValueError, match=word):
            model.gait_step_tables(*args, **kw)
    with pytest.raises(pkg._lib.GrnetError, match="fps"):
        model.gait_step_tables(ev, fr, fps=0.0)


def test_window_bootstrap_on_a_real_handle(model, pkg):
    """WindowBootstrap after WindowGait's, WindowTurns' and WindowBalance's calls, on the device and on the host: equal videos."""
    import batch_generation as bg
    joints, lengths = bk.turning_case()
    j3 = torch.from_numpy(joints).cuda()
    keys = ["v0", "v1"]
    gait = model.gait_parameters(j3, lengths=lengths, fps=FPS)
    turns = model.gait_turns(j3, gait["events"], gait["per_frame"], lengths=lengths, fps=FPS)
    bal = model.gait_balance(j3, gait["events"], lengths=lengths, fps=FPS)
    videos = []
    for on_host in (False, True):
        w = bg.WindowBootstrap(pkg.pipeline, model, on_host, fps=FPS, replicates=300, level=90.0, block=2, seed=5)
        assert (w.device_call is None) == on_host
        w.add_window(keys, lengths, gait["events"], gait["per_frame"], turns["phase"], (bal["steps"], bal["per_sequence"]))
        videos.append(w.videos)
    assert videos[0] == videos[1] and sorted(videos[0]) == keys
    v = videos[0]["v0"]
    host = pkg.pipeline.gait_parameters(joints, lengths=lengths, fps=FPS)
    assert v["parameters"]["stride_time_mean"]["estimate"] == host["per_sequence"][0, 8] and v["parameters"]["stride_time_mean"]["replicates"] == 300
    assert v["parameters"]["stride_time_mean"]["lo"] <= v["parameters"]["stride_time_mean"]["median"] <= v["parameters"]["stride_time_mean"]["hi"]
    assert len(v["step_table"]) == int(host["per_sequence"][0, 4]) and "straight_stride_time_cv" in v["parameters"] and "mos_ml_mean" in v["parameters"]
