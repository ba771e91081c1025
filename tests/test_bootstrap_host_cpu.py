"""Step tables and bootstrap intervals on the host: pipeline.gait_step_tables and pipeline.bootstrap_table, the numpy statements,
against the plain-loop restatement of tests/helpers/bootstrap_checks.py and against csrc/gait_bootstrap.h, the arithmetic the kernels run, through
tests/helpers/gait_bootstrap_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on files
this test writes.  All three agree IN EVERY BIT on every case the GPU tests use.  Then the generator's known answers, the identity (replicate 0 IS the
column the gait, turn and balance calls report), the faults compare must catch, the uniformity of the indices, the width and the coverage of the
interval of a mean, and every refusal.  Every figure is printed before it is asserted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import bootstrap_checks as bk
from .helpers import contact_checks as cc
from .helpers import gait_checks as gc
from .helpers import turn_checks as tc

FPS = 20.0


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def gait_cases(pipe):
    """[(name, events, per_frame, lengths, phase, max_rows, gait rows (n_seq,9))] of the GPU tests' table calls (tests/helpers/bootstrap_checks.py): the
    gait call's seven sequences (strikes on either side of a word seam, sequences of 1 frame up), a sequence past the LDS words, max_rows = 4, and a
    walker with a turn."""
    return bk.table_cases(PKG_NAME)


def test_known_answers(pipe):
    for args, u, i7, i1024 in bk.KNOWN_U:
        got = int(pipe.bootstrap_u(*args))
        print(args, hex(got), int(pipe.bootstrap_index(got, 7)), int(pipe.bootstrap_index(got, 1024)))
        assert got == u == bk.u_of(*args) and int(pipe.bootstrap_index(got, 7)) == i7 == bk.index_of(u, 7)
        assert int(pipe.bootstrap_index(got, 1024)) == i1024 == bk.index_of(u, 1024)
    for (block, r), idx in bk.KNOWN_IDX:
        assert pipe.bootstrap_indices(10, r, block)[r].tolist() == idx == bk.loops_indices(10, r, block)
    assert pipe.bootstrap_indices(10, 3, 1)[0].tolist() == list(range(10)) and pipe.bootstrap_indices(0, 3).shape == (4, 0)
    # a block above n: one draw, then the rows in circular order
    assert pipe.bootstrap_indices(7, 1, 100)[1].tolist() == [(1 + p) % 7 for p in range(7)]
    # equal n, equal indices, wherever the sequence lies in the call
    t = np.random.default_rng(1).normal(size=(3, 9, 2))
    out = pipe.bootstrap_table(np.concatenate([t, t[:1]]), [9, 5, 9, 9], [0, 1], B=50, seed=8)["out"]
    assert bk.same_bits(out[0], out[3])


def test_statement_equals_the_loops(pipe):
    for name, table, counts, kw in bk.cases():
        host = bk.statement(PKG_NAME, name)
        if name == "cap":                                       # 4 097 replicates of 1 024 rows in 8 columns: every 97th replicate, and the selection by a sort
            only = list(range(1, 4097, 97)) + [4096]
            loops = bk.loops_bootstrap(table, counts, only=only, **kw)
            at = [r - 1 for r in only]
            assert bk.same_bits(loops["replicates"][..., at], host["replicates"][..., at]) and bk.same_bits(loops["out"][..., 0], host["out"][..., 0])
            for k in range(len(kw["cols"])):
                for s in range(3):
                    assert bk.same_bits(bk.sorted_select(host["replicates"][0, k, s].tolist(), kw["quantiles"]), host["out"][0, k, s, 1:]), (k, s)
        else:
            loops = bk.loops_bootstrap(table, counts, **kw)
            bk.compare(host, loops, name + ": ")
            for q in range(len(counts)):
                for k in range(len(kw["cols"])):
                    for s in range(3):
                        assert bk.same_bits(bk.sorted_select(host["replicates"][q, k, s].tolist(), kw["quantiles"]), host["out"][q, k, s, 1:]), (name, q, k, s)
        print(f"{name}: f = {sorted(set(host['out'][..., 1].ravel().tolist()))}: equal bits")


def test_the_value_patterns_are_there(pipe):
    """What the `patterns` case is for, asserted on the statement so that the GPU test's comparison means what its docstring says."""
    out, reps = (bk.statement(PKG_NAME, "patterns")[k] for k in ("out", "replicates"))
    B = 200
    assert np.isnan(out[:, 1]).sum() == out[:, 1].size - 2 * 3 and (out[:, 1, :, 1] == 0).all()         # all NaN: f = 0, everything else NaN
    assert out[1, 0, 0, 1] < B and np.isnan(reps[1, 0, 0]).any() and np.isfinite(out[:, 0, 0, 0]).all()  # NaN rows: three of four in the second, so a replicate draws NaN alone
    assert (out[:, 2, 1, 0] == 0).all() and (out[:, 2, 1, 2:] == 0).all() and (out[:, 2, :, 1] == B).all()   # equal values: SD = 0, every replicate ties
    assert np.signbit(out[:, 3, 2, 0]).all() and (out[:, 3, 2, :1] == 0).all() and np.signbit(out[:, 3, 2, 2:]).all()      # equal negative values: CV = -0
    cv = reps[:, 4, 2]
    print(f"mean crossing zero: {np.isinf(cv).sum()} infinite CVs, {np.isnan(cv).sum()} of 0 / 0, {(np.signbit(cv) & (cv == 0)).sum()} of -0, f = {out[:, 4, 2, 1].tolist()}")
    assert np.isinf(cv).all(axis=1).tolist() == [False, False] and np.isinf(cv).any(axis=1).all() and np.isnan(cv[0]).any() and out[0, 4, 2, 1] < B
    assert (out[:, 4, 0, 1] == B).all() and np.isinf(out[:, 4, 2, -1]).all()                           # the infinite CVs are kept, 0 / 0 is left out
    assert ((cv[1] == 0) & np.signbit(cv[1])).any() and ((cv[1] == 0) & ~np.signbit(cv[1])).any()       # -0 among +0: the order by replicate number decides the bits
    assert out[1, 4, 2, 3] == 0                                 # ... and a quantile falls among them
    zeros = bk.statement(PKG_NAME, "negative_zeros")            # samples of -0.0: every sum begins at +0.0, so no mean is -0.0
    assert not np.signbit(zeros["out"][:, :2, 0, 0]).any() and (zeros["out"][:, :2, 0, 0] == 0).all() and not np.signbit(zeros["replicates"][:, :2, 0]).any()
    # a count above max_rows is read as max_rows
    name, table, counts, kw = next(c for c in bk.cases() if c[0] == "count_above_max_rows")
    assert bk.same_bits(bk.statement(PKG_NAME, name)["out"], pipe.bootstrap_table(table, [12, 12], **kw)["out"])


@pytest.mark.parametrize("fault", bk.FAULTS)
def test_compare_catches_a_planted_fault(pipe, fault):
    caught = []
    for name in ("four_block17", "patterns", "patterns_block2"):
        _, table, counts, kw = next(c for c in bk.cases() if c[0] == name)
        host = bk.statement(PKG_NAME, name)
        bk.compare(bk.loops_bootstrap(table, counts, **kw), host)                # without the fault: equal
        try:
            bk.compare(bk.loops_bootstrap(table, counts, fault=fault, **kw), host)
        except AssertionError as e:
            caught.append(name)
            print(f"{fault} on {name}: {e}")
    want = {"rank": "four_block17", "tie": "patterns", "nan_f": "patterns", "no_wrap": "four_block17", "stream": "four_block17"}[fault]
    assert want in caught, f"{fault}: caught on {caught}"


def chi2(cells):
    cells = np.asarray(cells, np.float64).ravel()
    e = cells.sum() / cells.size
    return float(((cells - e) ** 2 / e).sum())


def test_the_indices_are_uniform(pipe):
    """10 000 replicates of n = 7.  The bars are the 99.9 % points of chi-square at 6 and at 48 degrees of freedom."""
    for seed in (0, 1, 12345):
        p = np.arange(7)
        r = np.arange(1, 10001)[:, None]                        # B is at most 4 096 in a call; the generator itself takes any r
        idx = pipe.bootstrap_index(pipe.bootstrap_u(seed, 0, r, p[None, :]), 7).astype(np.int64)
        assert np.array_equal(idx[:4096], pipe.bootstrap_indices(7, 4096, 1, seed, 0)[1:])
        other = pipe.bootstrap_index(pipe.bootstrap_u(seed, 1, r, p[None, :]), 7).astype(np.int64)
        one = chi2(np.bincount(idx.ravel(), minlength=7))
        positions = chi2(np.bincount((idx[:, :-1] * 7 + idx[:, 1:]).ravel(), minlength=49))
        replicates = chi2(np.bincount((idx[:-1] * 7 + idx[1:]).ravel(), minlength=49))
        streams = chi2(np.bincount((idx * 7 + other).ravel(), minlength=49))
        print(f"seed {seed}: chi2 of the 7 cells {one:.2f} (bar 22.46); of the 49 cells of neighbouring positions {positions:.1f}, of neighbouring replicates "
              f"{replicates:.1f}, of streams 0 against 1 {streams:.1f} (bar 84.0)")
        assert one < 22.46 and max(positions, replicates, streams) < 84.0


def test_width_of_the_interval_of_the_mean(pipe):
    x = np.random.default_rng(7).normal(1.1, 0.04, 20)
    normal = 2 * 1.959964 * x.std() / np.sqrt(20)
    for block in (1, 2):
        for B in (500, 2000):
            est, f, lo, hi = pipe.bootstrap_table(x[None, :, None], [20], [0], B=B, block=block, seed=0, stream=0, quantiles=(250, 9750))["out"][0, 0, 0]
            print(f"block {block}, B = {B}: [{lo:.5f}, {hi:.5f}] around {est:.5f}, {(hi - lo) / normal:.3f} of the normal interval's width")
            assert f == B and 0.85 <= (hi - lo) / normal <= 1.15 and lo <= est <= hi


def test_coverage_of_the_percentile_interval(pipe):
    """400 samples of 20 from N(1.1, 0.04), B = 500: the share of 95 % intervals that hold 1.1.  The binomial SD is 0.014; the shortfall against 0.95
    is the percentile method's at n = 20 (DESIGN 4.23 states it)."""
    rng = np.random.default_rng(11)
    hold = 0
    for i in range(400):
        x = rng.normal(1.1, 0.04, 20)
        _, _, lo, hi = pipe.bootstrap_table(x[None, :, None], [20], [0], B=500, seed=i, quantiles=(250, 9750))["out"][0, 0, 0]
        hold += lo <= 1.1 <= hi
    print(f"coverage of the 95 % percentile interval of the mean at n = 20: {hold / 400:.4f}")
    assert 0.87 <= hold / 400 <= 0.96


def test_tables_equal_the_loops_and_sequences_do_not_see_each_other(pipe):
    for name, events, rows, lengths, phase, max_rows, _ in gait_cases(pipe):
        host = pipe.gait_step_tables(events, rows, lengths, FPS, max_rows, phase, phase is not None)
        bk.compare_tables(host, bk.loops_step_tables(events, rows, lengths, FPS, max_rows, phase, phase is not None), name + ": ")
        print(f"{name}: steps and strides {host['counts'].tolist()}")
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_step_tables(events[a:a + n], rows[a:a + n], None, FPS, max_rows, None if phase is None else phase[a:a + n], phase is not None)
            assert bk.same_bits(alone["steps"][0], host["steps"][q]) and bk.same_bits(alone["strides"][0], host["strides"][q]), (name, q)
            assert alone["counts"][0].tolist() == host["counts"][q].tolist()
            a += n
        if phase is not None:                                   # a phase without straight_only changes nothing
            assert bk.same_bits(pipe.gait_step_tables(events, rows, lengths, FPS, max_rows, phase, False)["steps"],
                                pipe.gait_step_tables(events, rows, lengths, FPS, max_rows)["steps"])


def identity_of(pipe, tables, counts, row, at):
    """Replicate 0 of the tables' columns against the columns `at` of a call's row, for the sequences whose columns hold no NaN and whose counts are
    within max_rows; returns how many sequences were compared."""
    steps = pipe.bootstrap_table(tables["steps"], counts[:, 0], [3, 4, 5], B=1, quantiles=())["out"][..., 0]
    strides = pipe.bootstrap_table(tables["strides"], counts[:, 1], [3], B=1, quantiles=())["out"][..., 0]
    done = 0
    for q in range(len(counts)):
        got = [steps[q, 0, 0], steps[q, 0, 1], steps[q, 1, 0], steps[q, 1, 1], steps[q, 2, 0], steps[q, 2, 1], strides[q, 0, 0], strides[q, 0, 1], strides[q, 0, 2]]
        want = row[q, list(at)]
        if counts[q].max() > tables["steps"].shape[1] or counts[q].min() < 1 or np.isnan(want).any():
            continue
        assert bk.same_bits(got, want), (q, got, want.tolist())
        done += 1
    return done


def test_identity_with_the_gait_turn_and_balance_columns(pipe):
    """Replicate 0 of the step and stride columns IS columns 5, 6, 11 .. 14 and 8 .. 10 of gait_parameters' row, straight-only of gait_turns' straight
    columns (kTurnGaitAt = 7 further), and on gait_balance's table per_sequence[4 .. 9, 14 .. 17], bit for bit."""
    walkers = [gc.walker(T, theta=theta, phi=phi)[0] for T, theta, phi in ((130, 0.7, -3.02), (400, 0.2, 1.9), (65, -1.1, -3.02), (200, 2.0, 0.4))]
    joints, lengths = np.concatenate(walkers), [len(w) for w in walkers]
    for sigma in (0.0, 2.0):
        gait = pipe.gait_parameters(joints, lengths=lengths, fps=FPS, sigma=sigma)
        tables = pipe.gait_step_tables(gait["events"], gait["per_frame"], lengths, FPS)
        done = identity_of(pipe, tables, tables["counts"], gait["per_sequence"], bk.GAIT_ROW_AT)
        print(f"sigma {sigma:g}: {done} walkers, steps and strides {tables['counts'].tolist()}")
        assert done == 4 and tables["counts"][:, 0].tolist() == gait["per_sequence"][:, 4].astype(int).tolist()
    joints, lengths = bk.turning_case()
    gait = pipe.gait_parameters(joints, lengths=lengths, fps=FPS)
    turns = pipe.gait_turns(joints, gait["events"], gait["per_frame"], lengths=lengths, fps=FPS)
    tables = pipe.gait_step_tables(gait["events"], gait["per_frame"], lengths, FPS, phase=turns["phase"], straight_only=True)
    assert turns["per_sequence"][0, 0] == 1 and tables["counts"][0, 0] == turns["per_sequence"][0, 11] < gait["per_sequence"][0, 4]
    assert identity_of(pipe, tables, tables["counts"], turns["per_sequence"], [c + 7 for c in bk.GAIT_ROW_AT]) == 2
    made = [cc.planted_walker(T, *cc.WALKERS[i % 4], 0.3 + i, 0.4 * i) for i, T in enumerate((130, 400, 200))]
    joints, lengths = np.concatenate(made), [130, 400, 200]
    events = pipe.gait_parameters(joints, lengths=lengths, fps=FPS)["events"]
    bal = pipe.gait_balance(joints, events, lengths=lengths, fps=FPS)
    out = pipe.bootstrap_table(bal["steps"], bal["per_sequence"][:, 1].astype(np.int32), [7, 8, 9, 11, 12], B=1, quantiles=())["out"][..., 0]
    for q in range(3):
        got = out[q, :, :2].ravel()                             # mean and SD of stride length, step length, step width, MoS_AP, MoS_ML
        assert bal["per_sequence"][q, 1] >= 5 and bk.same_bits(got, bal["per_sequence"][q, [4, 5, 6, 7, 8, 9, 14, 15, 16, 17]]), q


def test_bad_arguments_are_refused(pipe):
    t = np.ones((2, 8, 4))
    ok = dict(table=t, counts=[3, 8], cols=[1], B=10)
    pipe.bootstrap_table(**ok)
    for kw, word in ((dict(table=np.ones((2, 8))), "table"), (dict(table=np.ones((2, 1025, 4))), "max_rows"), (dict(table=np.ones((2, 8, 17))), "C 17"),
                     (dict(counts=[3]), "counts"), (dict(cols=[]), "n_cols"), (dict(cols=[0] * 9), "n_cols"), (dict(cols=[4]), "column"), (dict(cols=[-1]), "column"),
                     (dict(B=0), "B 0"), (dict(B=4097), "B 4097"), (dict(B=2.5), "B 2.5"), (dict(block=0), "block"), (dict(block=1025), "block"), (dict(seed=-1), "seed"),
                     (dict(seed=2**64), "seed"), (dict(stream=-1), "stream"), (dict(stream=65536), "stream"), (dict(quantiles=(1,) * 6), "n_q"),
                     (dict(quantiles=(-1,)), "quantile"), (dict(quantiles=(10001,)), "quantile")):
        with pytest.raises(ValueError, match=word):
            pipe.bootstrap_table(**{**ok, **kw})
    ev, rows = np.zeros(8, np.int32), np.zeros((8, 7))
    for args, kw, word in (((ev, rows[:, :6]), {}, "per_frame"), ((ev[:7], rows), {}, "events"), ((ev, rows), dict(lengths=[3, 4]), "lengths"), ((ev, rows), dict(fps=0.0), "fps"),
                           ((ev, rows), dict(fps=float("nan")), "fps"), ((ev, rows), dict(max_rows=0), "max_rows"), ((ev, rows), dict(max_rows=1025), "max_rows"),
                           ((ev, rows), dict(phase=ev[:7]), "phase"), ((ev, rows), dict(straight_only=True), "straight_only")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_step_tables(*args, **kw)


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """csrc/gait_bootstrap.h itself against the statement: one file per bootstrap case and per sequence of the table cases.  Every bit equal."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_bootstrap_check.cpp")
    exe = str(tmp_path / "gait_bootstrap_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for name, table, counts, kw in bk.cases():
        files.append(bk.write_bootstrap_case(str(tmp_path / f"{name}.bin"), table, counts, bk.statement(PKG_NAME, name), **kw))
    for name, events, rows, lengths, phase, max_rows, report in gait_cases(pipe):
        a = 0
        for q, n in enumerate(lengths):
            ph = None if phase is None else phase[a:a + n]
            host = pipe.gait_step_tables(events[a:a + n], rows[a:a + n], None, FPS, max_rows, ph, ph is not None)
            files.append(bk.write_tables_case(str(tmp_path / f"{name}{q}.bin"), events[a:a + n], rows[a:a + n], ph, FPS, max_rows, host, report[q]))
            a += n
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    print(f"{len(files)} files: {r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-200:]}")
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
