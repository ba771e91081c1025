"""What the bootstrap tests share: a plain-loop restatement of pipeline.bootstrap_table and pipeline.gait_step_tables in Python integers
and floats (one rounding per operation, like the statement's numpy and the header's C++), the faults compare must catch, the cases that the host
tests, the stand-alone checker and the GPU tests all run, and the writer of the files tests/helpers/gait_bootstrap_check.cpp reads.

There is no tolerance anywhere: the generator is integers, the statistics are + - * / sqrt in float64 in a fixed order, the selection names ONE
replicate.  Every comparison is of bits, a NaN equal to any NaN."""
import functools
import math

import numpy as np

from . import gait_checks as gc
from . import turn_checks as tc

NAN = float("nan")
MASK = 2**64 - 1
GOLDEN = 0x9E3779B97F4A7C15
# (seed, stream, r, j): u, index at n = 7, index at n = 1024 -- DESIGN 4.23's known answers, made with plain Python integers
KNOWN_U = (((0, 0, 1, 0), 0x2F101FE21496EA20, 1, 188), ((0, 0, 1, 1), 0xA00624088F65D5B6, 4, 640), ((0, 1, 1, 0), 0x882821205BABC31F, 3, 544),
           ((0, 0, 2, 0), 0x0B91752FD22FB56A, 0, 46), ((2023, 3, 4096, 1023), 0x507689E32221DAFD, 2, 321), ((2**64 - 1, 0, 1, 0), 0x85D74C1255584CAB, 3, 535))
# (block, r): idx of seed 0, stream 0, n = 10
KNOWN_IDX = (((1, 1), [1, 6, 4, 9, 3, 3, 1, 5, 7, 6]), ((1, 2), [0, 4, 6, 9, 0, 3, 4, 1, 4, 4]), ((3, 1), [1, 2, 3, 6, 7, 8, 4, 5, 6, 9]))
FAULTS = ("rank", "tie", "nan_f", "no_wrap", "stream")
QUANTILES = (0, 250, 5000, 9750, 10000)


def same_bits(a, b):
    return gc.same_bits(a, b)


# ----------------------------------------------------------------------------- the generator in Python integers
def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def u_of(seed, stream, r, j):
    key = mix((seed + GOLDEN * (stream + 1)) & MASK)
    key = mix((key + GOLDEN * (r + 1)) & MASK)
    return mix((key + GOLDEN * (j + 1)) & MASK)


def index_of(u, n):
    return ((u >> 32) * n) >> 32


def loops_indices(n, r, block=1, seed=0, stream=0, fault=None):
    if r == 0:
        return list(range(n))
    if fault == "stream":
        stream = 0
    idx = []
    for p in range(n):
        start = index_of(u_of(seed, stream, r, p // block), n)
        idx.append(min(start + p % block, n - 1) if fault == "no_wrap" else (start + p % block) % n)
    return idx


# ----------------------------------------------------------------------------- the statistics and the selection in plain loops
def _div(a, b):
    """a / b as IEEE 754 divides, where Python raises."""
    if b != 0:
        return a / b
    if a != a or a == 0:
        return NAN
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def loops_statistics(values):
    """(mean, SD, CV) of the values in the order given, NaN skipped: gait_strides' operations in its order."""
    s, m = 0.0, 0
    for v in values:
        if v != v:
            continue
        s = s + v
        m += 1
    if m == 0:
        return NAN, NAN, NAN
    mean = s / m
    acc = 0.0
    for v in values:
        if v != v:
            continue
        d = v - mean
        acc = acc + d * d
    sd = math.sqrt(acc / m)
    return mean, sd, _div(100.0 * sd, mean)


def loops_select(values, quantiles, fault=None):
    """[f, the quantiles] by COUNTING RANKS, as the kernel does: value under <, then replicate number."""
    kept = [(v, i) for i, v in enumerate(values) if v == v]
    f = len(values) if fault == "nan_f" else len(kept)
    out = [float(f)] + [NAN] * len(quantiles)
    for v, i in kept:
        if fault == "tie":
            rank = sum(1 for b, j in kept if b < v or (b == v and j > i))      # ties the other way round: the VALUES are in order all the same
        else:
            rank = sum(1 for b, j in kept if b < v or (b == v and j < i))
        for k, q in enumerate(quantiles):
            want = (q * (f - 1)) // 10000 + (fault == "rank")
            if rank == want:
                out[1 + k] = v
    return out


def sorted_select(values, quantiles):
    """[f, the quantiles] by a SORT on (value, replicate number) -- Python compares -0.0 and 0.0 equal, so the number decides between them.  The
    other method the specification allows: it must name the same replicate's bits as counting ranks."""
    kept = sorted((v, i) for i, v in enumerate(values) if v == v)
    return [float(len(kept))] + [kept[(q * (len(kept) - 1)) // 10000][0] if kept else NAN for q in quantiles]


def loops_bootstrap(table, counts, cols, B=2000, block=1, seed=0, stream=0, quantiles=(250, 5000, 9750), fault=None, only=None):
    """pipeline.bootstrap_table in plain loops: {'out', 'replicates'}.  only: the replicates to make (None: all) -- with it 'out' is not made beyond
    replicate 0 and the replicates not asked for are NaN."""
    table = np.asarray(table, np.float64)
    n_seq, max_rows, _ = table.shape
    out = np.full((n_seq, len(cols), 3, 2 + len(quantiles)), NAN)
    reps = np.full((n_seq, len(cols), 3, B), NAN)
    wanted = range(B + 1) if only is None else sorted(set(only) | {0})
    for q in range(n_seq):
        n = min(max(int(counts[q]), 0), max_rows)
        idx = {r: loops_indices(n, r, block, seed, stream, fault) for r in wanted}
        for k, c in enumerate(cols):
            x = table[q, :n, c].tolist()
            for r in wanted:
                st = loops_statistics([x[i] for i in idx[r]])
                if r == 0:
                    out[q, k, :, 0] = st
                else:
                    reps[q, k, :, r - 1] = st
            if only is None:
                for s in range(3):
                    out[q, k, s, 1:] = loops_select(reps[q, k, s].tolist(), quantiles, fault)
    return {"out": out, "replicates": reps}


def compare(got, want, what=""):
    """Every bit of 'out' and, where both have them, of 'replicates'; the first difference is named."""
    for key in ("out", "replicates"):
        if key not in got or key not in want:
            continue
        g, w = np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)
        assert g.shape == w.shape, f"{what}{key}: shape {g.shape}, not {w.shape}"
        bad = ~((g.view(np.int64) == w.view(np.int64)) | (np.isnan(g) & np.isnan(w)))
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError(f"{what}{key}{list(at)} = {g[at]!r} ({g[at].hex() if g[at] == g[at] else 'nan'}), not {w[at]!r}; {int(bad.sum())} differ")


# ----------------------------------------------------------------------------- the step and stride tables in plain loops
def loops_step_tables(events, per_frame, lengths=None, fps=20.0, max_rows=256, phase=None, straight_only=False):
    events, rows = np.asarray(events), np.asarray(per_frame, np.float64)
    lengths = [len(events)] if lengths is None else list(lengths)
    steps = np.full((len(lengths), max_rows, 6), NAN)
    strides = np.full((len(lengths), max_rows, 4), NAN)
    counts = np.zeros((len(lengths), 2), np.int32)
    a = 0
    for q, T in enumerate(lengths):
        def straight(t1, t2):
            return not straight_only or all(int(phase[a + t]) == 0 for t in range(t1, t2 + 1))
        strikes = []
        for t in range(T):
            for foot in (0, 1):
                if int(events[a + t]) & (1 << foot):
                    strikes.append((t, foot))
        n = 0
        for (pt, pf), (t, foot) in zip(strikes[:-1], strikes[1:]):
            if pf != foot and straight(pt, t):
                if n < max_rows:
                    r = rows[a + t]
                    steps[q, n] = [pt, t, foot, float(t - pt) / fps, r[foot] - r[1 - foot], r[4]]
                n += 1
        m = 0
        for foot in (0, 1):
            own = [t for t, f in strikes if f == foot]
            for t0, t1 in zip(own[:-1], own[1:]):
                if straight(t0, t1):
                    if m < max_rows:
                        strides[q, m] = [t0, t1, foot, float(t1 - t0) / fps]
                    m += 1
        counts[q] = n, m
        a += T
    return {"steps": steps, "strides": strides, "counts": counts}


def compare_tables(got, want, what=""):
    assert np.array_equal(np.asarray(got["counts"]), np.asarray(want["counts"])), f"{what}counts {np.asarray(got['counts']).tolist()}, not {np.asarray(want['counts']).tolist()}"
    for key in ("steps", "strides"):
        assert same_bits(got[key], want[key]), f"{what}{key} differ in some bit"


# ----------------------------------------------------------------------------- the cases every layer runs
def _table(rng, n_seq, max_rows, C, counts):
    t = rng.normal(1.0, 0.3, (n_seq, max_rows, C))
    for q, n in enumerate(counts):
        t[q, min(max(n, 0), max_rows):] = NAN                  # the rows past the count, as the table calls leave them
    return t


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, table, counts, keywords)] of the GPU tests' bootstrap calls, made once.  Nobody writes into them."""
    rng = np.random.default_rng(423)
    made = []
    for n in (0, 1, 2, 3):
        for B in (1, 63, 64, 65):
            made.append((f"one_n{n}_B{B}", _table(rng, 1, 4, 3, [n]), [n], dict(cols=(0, 2), B=B, quantiles=(250, 5000, 9750))))
    four = _table(rng, 4, 80, 6, [0, 1, 17, 65])
    for block in (1, 2, 17, 100):
        made.append((f"four_block{block}", four, [0, 1, 17, 65], dict(cols=(3, 4, 5), B=200, block=block, seed=5, stream=2, quantiles=QUANTILES)))
    mixed = [(0, 3, 15, 40, 1, 27, 16, 2, 33, 8)[i % 10] for i in range(50)]
    made.append(("fifty", _table(rng, 50, 40, 4, mixed), mixed, dict(cols=(1, 3), B=100, block=2, seed=99, stream=7, quantiles=(250, 9750))))
    made.append(("cap", _table(rng, 1, 1024, 16, [1024]), [1024], dict(cols=(0, 2, 4, 6, 9, 11, 13, 15), B=4096, block=1, seed=2**63 + 11, stream=65535, quantiles=QUANTILES)))
    made.append(("patterns", patterns_table(), [6, 4], dict(cols=(0, 1, 2, 3, 4, 5), B=200, seed=3, quantiles=(0, 2500, 5000, 9750, 10000))))
    made.append(("patterns_block2", patterns_table(), [6, 4], dict(cols=(0, 1, 2, 3, 4, 5), B=65, block=2, seed=4, stream=1, quantiles=(0, 2500, 5000, 9750, 10000))))
    made.append(("negative_zeros", negative_zeros_table(), [4, 3], dict(cols=(0, 1, 2), B=65, seed=6, quantiles=QUANTILES)))
    over = _table(rng, 2, 12, 3, [12, 12])
    made.append(("count_above_max_rows", over, [17, 2**31 - 1], dict(cols=(1,), B=64, quantiles=(5000,))))
    return made


def negative_zeros_table():
    """Two sequences of 4 and 3 rows with samples of -0.0: column 0 all -0.0 (every sum begins at +0.0, so the mean is +0.0, never -0.0); column 1 a
    leading -0.0 among +0.0; column 2 a leading -0.0, a NaN and values that cancel to zero."""
    t = np.full((2, 4, 3), NAN)
    t[0, :, 0], t[1, :3, 0] = -0.0, -0.0
    t[0, :, 1], t[1, :3, 1] = [-0.0, 0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]
    t[0, :, 2], t[1, :3, 2] = [-0.0, NAN, 0.5, -0.5], [-0.0, NAN, -0.0]
    return t


def patterns_table():
    """Two sequences of 6 and 4 rows, six columns: 0 NaN in some rows; 1 all NaN (f = 0); 2 equal values (every replicate ties, SD = 0); 3 equal
    negative values (CV = -0); 4 a mean that crosses zero -- in the first sequence zeros, a 1 and a -1, so that a replicate's mean is 0 with SD > 0 (CV
    infinite, kept) or with SD = 0 (0 / 0, left out); in the second two 1 and two -1, so that SD = 0 comes with a mean of either sign and the zeros of
    CV with both signs, which only the order by replicate number tells apart; 5 ordinary."""
    t = np.full((2, 6, 6), NAN)
    t[0, :, 0] = [1.5, NAN, 0.25, NAN, 2.0, 1.0]
    t[1, :4, 0] = [NAN, NAN, 3.0, NAN]
    t[0, :, 2], t[1, :4, 2] = 0.75, 0.75                      # sums of these are exact, so that the mean is the value and SD = 0
    t[0, :, 3], t[1, :4, 3] = -0.25, -0.25
    t[0, :, 4] = [0.0, 0.0, 0.0, 0.0, 1.0, -1.0]
    t[1, :4, 4] = [1.0, 1.0, -1.0, -1.0]
    t[0, :, 5] = [1.08, 1.12, 1.05, 1.11, 1.09, 1.13]
    t[1, :4, 5] = [0.52, 0.55, 0.49, 0.5]
    return t


@functools.lru_cache(maxsize=None)
def statement(pkg_name, name):
    """The statement's result of a case, with its replicates, computed once and shared."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    _, table, counts, kw = next(c for c in cases() if c[0] == name)
    return pipe.bootstrap_table(table, counts, return_replicates=True, **kw)


@functools.lru_cache(maxsize=None)
def turning_case():
    """(joints, lengths) of a walker with one turn of 90 degrees to the left in the middle of 400 frames, and a straight one beside it."""
    a = tc.turning_walker(400, turns=((150, 60, 90.0),), theta0=0.3)[0]
    b = gc.walker(130, theta=0.7)[0]
    return np.concatenate([a, b]), [400, 130]



def excursion(window):
    return 0.005 if window == 1 else 0.05                      # three frames around a peak rise by 0.012 m only (the gait call's device tests)


@functools.lru_cache(maxsize=None)
def table_cases(pkg_name):
    """[(name, events, per_frame, lengths, phase or None, max_rows, report (n_seq,9))] made once on the host: the inputs of the table calls and what
    the gait call (with a phase: the turn call's straight columns) reports of them -- for hand-laid events, replicate 0 of the statement's tables."""
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    made = []
    at = list(GAIT_ROW_AT)
    for window in (5, 1):                                       # the seven sequences of the gait call's device tests: walks of 130 frames cross a word seam; 1, 2 w and 2 w + 1 frames
        table = gc.KINECTV2
        joints, _, lengths, _ = gc.build_call(window, J=25, table=table)
        gait = pipe.gait_parameters(joints, lengths=lengths, fps=20.0, sigma=0.0, window=window, min_excursion=excursion(window), joints=table)
        made.append((f"seven_w{window}", gait["events"], gait["per_frame"], lengths, None, 256, gait["per_sequence"][:, at]))
        if window == 5:
            seven = made[-1]
            strikes = np.flatnonzero(gait["events"][:130] & 3)
            assert (strikes < 64).any() and (strikes >= 64).any()
    lengths = [1, 2, 3, 4]
    rows = seven[2][:10].copy()
    events = np.array([1, 1, 2, 1, 2, 1, 2, 1, 3, 2], np.int32)  # 4 frames: right, left, both feet in one frame (the left first: a step of 0 frames), right
    made.append(("short", events, rows, lengths, None, 256, None))
    long_j = gc.walker(4200, theta=1.3, phi=-3.02)[0]
    short_j = gc.walker(65, theta=0.2)[0]
    joints, lengths = np.concatenate([short_j, long_j, short_j]), [65, 4200, 65]
    gait = pipe.gait_parameters(joints, lengths=lengths, fps=20.0, sigma=0.0)
    made.append(("long", gait["events"], gait["per_frame"], lengths, None, 1024, gait["per_sequence"][:, at]))
    made.append(("max_rows4", seven[1], seven[2], seven[3], None, 4, seven[6]))
    joints, lengths = turning_case()
    gait = pipe.gait_parameters(joints, lengths=lengths, fps=20.0)
    turns = pipe.gait_turns(joints, gait["events"], gait["per_frame"], lengths=lengths, fps=20.0)
    assert turns["per_sequence"][0, 0] == 1 and 0 < turns["per_sequence"][0, 11] < gait["per_sequence"][0, 4]
    made.append(("turn", gait["events"], gait["per_frame"], lengths, turns["phase"], 256, turns["per_sequence"][:, [c + 7 for c in at]]))
    done = []
    for name, events, rows, lengths, phase, max_rows, report in made:
        if report is None:
            t = pipe.gait_step_tables(events, rows, lengths, 20.0, max_rows)
            a = pipe.bootstrap_table(t["steps"], t["counts"][:, 0], [3, 4, 5], B=1, quantiles=())["out"][..., 0]
            b = pipe.bootstrap_table(t["strides"], t["counts"][:, 1], [3], B=1, quantiles=())["out"][..., 0]
            report = np.concatenate([a[:, :, :2].reshape(len(lengths), 6), b[:, 0, :]], axis=1)
        done.append((name, events, rows, lengths, phase, max_rows, report))
    return done


@functools.lru_cache(maxsize=None)
def tables_statement(pkg_name, name):
    import importlib
    pipe = importlib.import_module(pkg_name).pipeline
    _, events, rows, lengths, phase, max_rows, _ = next(c for c in table_cases(pkg_name) if c[0] == name)
    return pipe.gait_step_tables(events, rows, lengths, 20.0, max_rows, phase, phase is not None)


# ----------------------------------------------------------------------------- files for tests/helpers/gait_bootstrap_check.cpp
def write_bootstrap_case(path, table, counts, host, cols, B, block=1, seed=0, stream=0, quantiles=(250, 5000, 9750)):
    table = np.asarray(table, np.float64)
    n_seq, max_rows, C = table.shape
    with open(path, "wb") as f:
        f.write(np.array([0, n_seq, max_rows, C, len(cols), B, block, stream, len(quantiles)], "<i4").tobytes())
        f.write(np.array([seed], "<u8").tobytes() + np.asarray(cols, "<i4").tobytes() + np.asarray(quantiles, "<i4").tobytes())
        f.write(np.asarray(counts, "<i4").tobytes() + np.ascontiguousarray(table, "<f8").tobytes())
        f.write(np.ascontiguousarray(host["out"], "<f8").tobytes() + np.ascontiguousarray(host["replicates"], "<f8").tobytes())
    return path


def write_tables_case(path, events, per_frame, phase, fps, max_rows, host, row):
    """ONE sequence: its events, rows and (or None) phase, the statement's tables, and `row`: the 9 values [mean, SD of step time, length, width;
    mean, SD, CV of stride time] that gait_parameters (or, with a phase, gait_turns) reports -- replicate 0 must meet them in every bit."""
    T = len(events)
    with open(path, "wb") as f:
        f.write(np.array([1, T, max_rows, phase is not None], "<i4").tobytes() + np.array([fps], "<f8").tobytes())
        f.write(np.asarray(events, "<i4").tobytes())
        if phase is not None:
            f.write(np.asarray(phase, "<i4").tobytes())
        f.write(np.ascontiguousarray(per_frame, "<f8").tobytes())
        f.write(np.ascontiguousarray(host["steps"][0], "<f8").tobytes() + np.ascontiguousarray(host["strides"][0], "<f8").tobytes())
        f.write(np.asarray(host["counts"][0], "<i4").tobytes() + np.asarray(row, "<f8").tobytes())
    return path


GAIT_ROW_AT = (5, 6, 11, 12, 13, 14, 8, 9, 10)                # gait_parameters' columns of [step time mean, SD; length; width; stride mean, SD, CV]
