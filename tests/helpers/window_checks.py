"""A whole database window through the gait chain, shared by the host and the GPU tests: the windows, the chain as
batch_generation.prepare_data runs it, the teacher-forced walk and the comparison of two runs bit for bit.  Nothing here calls the code under test
but through the `calls` it is handed.  No bar is made here: every one is gait_checks', kinematics_checks', turn_checks' or contact_checks', or equality.

THE WINDOWS.  Every sequence is turn_checks.turning_walker.  Sequence q of T frames has theta0 = 0.37 q, phi = -3.02 - 0.6137 q and, from 127 frames
on, one turn (T // 4, 30, 90 degrees if q is odd, else -120).  trans is rounded through float32, as the database stores it, and the frames 5, 70 and
200 of the call are NaN.  build(name, other=True) is the same recipe at another theta0 and phi: the chain that runs BEFORE a checked one, so that the
scratch a stage does not write holds another body's numbers, not its own from the last test.
  window50    50 sequences, the production count (pipeline.MAX_VID), lengths on and around the 64-frame mask words and the 256-thread passes
  long_pairs  two sequences past the 4096 frames of the LDS arrays back to back, the first 65 * 64 frames long, so that the second one's words begin
              exactly where the first one's end; and two past gait_kinematics' 1024 frames, the first 17 * 64; short ones first, between and last
  many600     600 sequences of 1 .. 65 frames: the binary search over the offsets, the word and slot placement per sequence, a table of 2.4 KB

THE CHAIN.  chain() makes the six calls in prepare_data's order with the Window* classes' arguments: gait_parameters, then gait_kinematics,
gait_turns and gait_contacts on its events (turns on its per_frame rows too), then gait_regularity and gait_harmonics with the turns' phase as
exclude.  handoff "device" passes every returned tensor straight on (and trans as fit_translation returns it: three columns of a wider float64
buffer); "host" downloads it first, as prepare_data does with the phase; "strided" passes each as every second row of a doubled buffer.  It returns
{stage: {"inputs": ..., "outputs": ...}} in numpy, the inputs as the stage received them.

THE WALK.  walk() is teacher-forced: every stage's host statement is evaluated on the inputs that stage actually got from the device's earlier
stages, and compared by that stage's own rule; one stage's legitimate rounding (a smoothed signal within its bar) never becomes the next one's error,
and a fault is named at the stage that made it.  It also asserts that what a stage got IS what its producer returned, the margin conditions of the
gait, turns and contacts statements, and it prints every figure before it asserts and names all failing stages at once."""
import collections

import numpy as np

from . import contact_checks as cc
from . import gait_checks as gc
from . import kinematics_checks as kc
from . import turn_checks as tc

STAGES = ("gait", "kinematics", "turns", "contacts", "regularity", "harmonics")
ZERO = {stage: 0.0 for stage in STAGES}
PRODUCTION = dict(gait=2.0, kinematics=2.0, turns=8.0, contacts=0.0, regularity=0.0, harmonics=0.0)       # the Window* classes' defaults
FPS = 20.0
RULES = {"gait": dict(fps=FPS, window=5, min_excursion=0.05), "kinematics": dict(min_stride=8, max_stride=60),
         "turns": dict(fps=FPS, edge_rate=5.0, peak_rate=15.0, min_angle=45.0, min_frames=10, max_frames=200),
         "contacts": dict(fps=FPS, fraction=0.25, speed=0.0, reach=2, max_frames=20),
         "regularity": dict(fps=FPS, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20),
         "harmonics": dict(fps=FPS, n_harmonics=20, derivative=2, min_stride=8, max_stride=60)}
NAN_FRAMES = (5, 70, 200)
LENGTHS = {"window50": [[1, 2, 19, 20, 63, 64, 65, 127, 128, 129, 130, 200, 257][q % 13] for q in range(50)],
           "long_pairs": [65, 4160, 4200, 65, 1088, 1100, 64],
           "many600": [[1, 2, 3, 20, 65][q % 5] for q in range(600)]}
FRAMES = {"window50": 4363, "long_pairs": 10742, "many600": 10920}
Window = collections.namedtuple("Window", "joints trans lengths names")
same_bits = gc.same_bits


def build(name, other=False, P=21.7):
    """Window(joints (n,25,3) float32, trans (n,3) float64, lengths, names) of the window `name`; P: the gait's period in frames (the strides inside a
    turn: 30 P / 21.7), for the one test whose Gaussian would leave nothing of a period of 21.7 frames."""
    lengths = LENGTHS[name]
    assert sum(lengths) == FRAMES[name]
    made = []
    for q, T in enumerate(lengths):
        turns = ((T // 4, 30, 90.0 if q % 2 else -120.0),) if T >= 127 else ()
        theta0, phi = (1.1 + 0.53 * q, 1.9 - 0.4171 * q) if other else (0.37 * q, -3.02 - 0.6137 * q)
        made.append(tc.turning_walker(T, turns, theta0=theta0, phi=phi, P=P, turn_P=30.0 * P / 21.7))
    trans = np.concatenate([t for _, t in made]).astype(np.float32).astype(np.float64)
    trans[list(NAN_FRAMES)] = np.nan
    return Window(np.concatenate([j for j, _ in made]), trans, list(lengths), [f"{name}_{q:03d}_{T}" for q, T in enumerate(lengths)])


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def download(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def strided(v):
    """v as every second row of a doubled buffer (numpy or torch), other numbers between the rows."""
    shape = (2 * v.shape[0],) + tuple(v.shape[1:])
    buf = v.new_empty(shape) if hasattr(v, "new_empty") else np.empty(shape, v.dtype)
    buf[1::2] = 77
    buf[::2] = v
    return buf[::2]


def chain(calls, window, sigmas, handoff="device"):
    """The six calls on `calls` (a device model, or a stand-in of host statements such as HostCalls).  Nothing is downloaded before the last call is
    made, so with a device model and handoff "device" all six are in flight together."""
    give = {"device": lambda v: v, "host": download, "strided": strided}[handoff]
    joints, trans, lengths = window.joints, window.trans, window.lengths
    if hasattr(calls, "device"):                               # prepare_data's joints are on the device already
        import torch
        joints = torch.as_tensor(joints).to(calls.device)
        if handoff != "host":                                  # fit_translation's per_frame[:, :3]: float64, three columns of six
            wide = torch.full((trans.shape[0], 6), 77.0, dtype=torch.float64, device=calls.device)
            wide[:, :3] = torch.as_tensor(trans).to(calls.device)
            trans = wide[:, :3]
    run = {}

    def made(stage, method, inputs):
        run[stage] = {"inputs": inputs, "outputs": method(lengths=lengths, sigma=float(sigmas[stage]), **inputs, **RULES[stage])}
        return run[stage]["outputs"]
    gait = made("gait", calls.gait_parameters, dict(joints3d=joints, trans=trans))
    events, rows = give(gait["events"]), give(gait["per_frame"])
    made("kinematics", calls.gait_kinematics, dict(joints3d=joints, events=events))
    turns = made("turns", calls.gait_turns, dict(joints3d=joints, events=events, gait_rows=rows))
    made("contacts", calls.gait_contacts, dict(joints3d=joints, events=events))
    exclude = give(turns["phase"])
    made("regularity", calls.gait_regularity, dict(joints3d=joints, trans=trans, exclude=exclude))
    made("harmonics", calls.gait_harmonics, dict(joints3d=joints, events=events, trans=trans, exclude=exclude))
    return {stage: {side: {k: download(v) for k, v in part.items()} for side, part in both.items()} for stage, both in run.items()}


class HostCalls:
    """The stand-in of host statements: the six calls answered by pipeline.*, in numpy."""

    def __init__(self, pipe):
        self.pipe = pipe

    def gait_parameters(self, joints3d, lengths=None, trans=None, **kw):
        return self.pipe.gait_parameters(download(joints3d), lengths, None if trans is None else download(trans), **kw)

    def gait_kinematics(self, joints3d, events, lengths=None, **kw):
        return self.pipe.gait_kinematics(download(joints3d), download(events), lengths, **kw)

    def gait_turns(self, joints3d, events, gait_rows, lengths=None, **kw):
        return self.pipe.gait_turns(download(joints3d), download(events), download(gait_rows), lengths, **kw)

    def gait_contacts(self, joints3d, events, lengths=None, **kw):
        return self.pipe.gait_contacts(download(joints3d), download(events), lengths, **kw)

    def gait_regularity(self, joints3d, lengths=None, trans=None, exclude=None, **kw):
        return self.pipe.gait_regularity(download(joints3d), lengths, None if trans is None else download(trans), None if exclude is None else download(exclude), **kw)

    def gait_harmonics(self, joints3d, events, lengths=None, trans=None, exclude=None, **kw):
        return self.pipe.gait_harmonics(download(joints3d), download(events), lengths, None if trans is None else download(trans),
                                        None if exclude is None else download(exclude), **kw)


def same_bytes(a, b):
    """Equal shape, kind of number and bytes: a NaN must be the same NaN in the same place.  Integers are compared as int64, so that a host statement's
    integer type is not part of the comparison."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or (a.dtype.kind == "f") != (b.dtype.kind == "f"):
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a.astype(np.int64), b.astype(np.int64)))
    return a.dtype == b.dtype and bool(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)))


def differing(run_a, run_b, sides=("inputs", "outputs")):
    """["stage side name", ...] of everything that differs in some byte between two runs of chain()."""
    found = []
    for stage in STAGES:
        for side in sides:
            a, b = run_a[stage][side], run_b[stage][side]
            found += [f"{stage} {side} ?"] if sorted(a) != sorted(b) else [f"{stage} {side} {k}" for k in a if not same_bytes(a[k], b[k])]
    return found


def assert_same_runs(run_a, run_b, what=""):
    found = differing(run_a, run_b)
    assert not found, f"{what}: differ in some byte: {', '.join(found)}"


def cut(run, window, q):
    """What sequence q of a window's run looks like as a run of its own: the rows of every per-frame array, row q of every other."""
    off = offsets(window.lengths)
    a, b, n = int(off[q]), int(off[q + 1]), int(off[-1])
    return {stage: {side: {k: (v[a:b] if v.shape[0] == n else v[q:q + 1]) for k, v in part.items()} for side, part in both.items()} for stage, both in run.items()}


def alone(calls, window, run, q, sigmas):
    """Sequence q alone through each of the six calls, every call on the window's own slices of what it took there: a run like chain()'s."""
    part = cut(run, window, q)
    methods = dict(zip(STAGES, (calls.gait_parameters, calls.gait_kinematics, calls.gait_turns, calls.gait_contacts, calls.gait_regularity, calls.gait_harmonics)))
    out = {}
    for stage in STAGES:
        got = methods[stage](lengths=None, sigma=float(sigmas[stage]), **part[stage]["inputs"], **RULES[stage])
        out[stage] = {"inputs": part[stage]["inputs"], "outputs": {k: download(v) for k, v in got.items()}}
    return out


def _handed(run, stage, name, producer, key):
    assert same_bytes(run[stage]["inputs"][name], run[producer]["outputs"][key]), f"{stage} got as {name} something else than the {key} that {producer} returned"


def _signals_rule(got, host, raw, lengths, sigma, again, keys):
    """The rule of test_gpu_regularity.py and test_gpu_harmonics.py: per_frame within twice the Gaussian's bar (gait_checks.signal_bars; sigma 0: equal
    bits), everything else equal in every bit to what again(per_frame) makes of the result's own per_frame."""
    assert np.array_equal(np.isnan(got["per_frame"]), np.isnan(host["per_frame"])), "per_frame has a NaN on one side alone"
    worst, a = 0.0, 0
    for q, T in enumerate(lengths):
        b = gc.signal_bars(raw[a:a + T], sigma) if sigma > 0 else np.zeros(4)
        for k in range(4):
            g, h = got["per_frame"][a:a + T, k], host["per_frame"][a:a + T, k]
            fin = np.isfinite(h)
            if fin.any() and b[k] > 0:
                worst = max(worst, float(np.abs(g - h)[fin].max()) / b[k])
            else:
                assert same_bits(g, h), f"sequence {q}: per_frame column {k} differs in some bit"
        a += T
    rest = host if same_bits(got["per_frame"], host["per_frame"]) else again(got["per_frame"])
    for k in keys:
        assert got[k].shape == rest[k].shape, f"{k} has shape {got[k].shape}, not {rest[k].shape}"
        rows = [q for q in range(len(lengths)) if not same_bits(got[k][q], rest[k][q])]
        assert not rows, f"{k} differs in some bit from what the host makes of the same per_frame, in the sequences {rows[:8]}"
    return worst


def _walk_gait(run, pipe, w, sigma, margins):
    inp, got = run["gait"]["inputs"], run["gait"]["outputs"]
    host = pipe.gait_parameters(inp["joints3d"], w.lengths, inp["trans"], sigma=sigma, **RULES["gait"])
    raw = pipe.gait_parameters(inp["joints3d"], w.lengths, inp["trans"], sigma=0.0, **RULES["gait"])["per_frame"][:, :4] if sigma > 0 else None
    margins["gait"] = gc.assert_margin(host["per_frame"], w.lengths, RULES["gait"]["window"], RULES["gait"]["min_excursion"])
    return gc.compare(got, host, raw, w.lengths, sigma)


def _walk_kinematics(run, pipe, w, sigma, margins):
    _handed(run, "kinematics", "events", "gait", "events")
    inp, got = run["kinematics"]["inputs"], run["kinematics"]["outputs"]
    host = pipe.gait_kinematics(inp["joints3d"], inp["events"], w.lengths, sigma=sigma, **RULES["kinematics"])
    raw = pipe.gait_kinematics(inp["joints3d"], inp["events"], w.lengths, sigma=0.0, **RULES["kinematics"])["per_frame"] if sigma > 0 else None
    return kc.compare(got, host, raw, w.lengths, sigma)


def _walk_turns(run, pipe, w, sigma, margins):
    _handed(run, "turns", "events", "gait", "events")
    _handed(run, "turns", "gait_rows", "gait", "per_frame")
    inp, got = run["turns"]["inputs"], run["turns"]["outputs"]
    host = pipe.gait_turns(inp["joints3d"], inp["events"], inp["gait_rows"], w.lengths, sigma=sigma, **RULES["turns"])
    raw = pipe.gait_turns(inp["joints3d"], inp["events"], inp["gait_rows"], w.lengths, sigma=0.0, **RULES["turns"])["per_frame"][:, 1] if sigma > 0 else None
    margins["turns"] = tc.assert_margin(host["per_frame"], w.lengths, RULES["turns"]["edge_rate"], RULES["turns"]["peak_rate"], RULES["turns"]["min_angle"])
    return tc.compare(got, host, raw, w.lengths, sigma)


def _walk_contacts(run, pipe, w, sigma, margins):
    _handed(run, "contacts", "events", "gait", "events")
    inp, got = run["contacts"]["inputs"], run["contacts"]["outputs"]
    host = pipe.gait_contacts(inp["joints3d"], inp["events"], w.lengths, sigma=sigma, **RULES["contacts"])
    raw = pipe.gait_contacts(inp["joints3d"], inp["events"], w.lengths, sigma=0.0, **RULES["contacts"])["per_frame"][:, 1:4] if sigma > 0 else None
    margins["contacts"] = cc.assert_margin(host, w.lengths)
    return cc.compare(got, host, raw, w.lengths, sigma, fps=FPS, fraction=RULES["contacts"]["fraction"], speed=RULES["contacts"]["speed"])


def _walk_regularity(run, pipe, w, sigma, margins):
    _handed(run, "regularity", "exclude", "turns", "phase")
    inp, got = run["regularity"]["inputs"], run["regularity"]["outputs"]
    host = pipe.gait_regularity(inp["joints3d"], w.lengths, inp["trans"], inp["exclude"], sigma=sigma, **RULES["regularity"])
    raw = pipe.gait_regularity(inp["joints3d"], w.lengths, inp["trans"], sigma=0.0, **RULES["regularity"])["per_frame"] if sigma > 0 else None
    return _signals_rule(got, host, raw, w.lengths, sigma, lambda x: pipe.gait_autocorr(x, w.lengths, inp["exclude"], **RULES["regularity"]), ("acf", "per_sequence"))


def _walk_harmonics(run, pipe, w, sigma, margins):
    _handed(run, "harmonics", "events", "gait", "events")
    _handed(run, "harmonics", "exclude", "turns", "phase")
    inp, got = run["harmonics"]["inputs"], run["harmonics"]["outputs"]
    host = pipe.gait_harmonics(inp["joints3d"], inp["events"], w.lengths, inp["trans"], inp["exclude"], sigma=sigma, **RULES["harmonics"])
    raw = pipe.gait_regularity(inp["joints3d"], w.lengths, inp["trans"], sigma=0.0, **RULES["regularity"])["per_frame"] if sigma > 0 else None
    return _signals_rule(got, host, raw, w.lengths, sigma, lambda x: pipe.gait_stride_dft(x, inp["events"], w.lengths, inp["exclude"], **RULES["harmonics"]),
                         ("strides", "spectrum", "per_sequence"))


class StagesFailed(AssertionError):
    """walk()'s verdict; failed: {stage: why}."""

    def __init__(self, what, failed):
        super().__init__(f"{what}: failing stages: " + "; ".join(f"{stage} ({why})" for stage, why in failed.items()))
        self.failed = failed


_WALK = dict(zip(STAGES, (_walk_gait, _walk_kinematics, _walk_turns, _walk_contacts, _walk_regularity, _walk_harmonics)))


def walk(device_run, pipe, window, sigmas, margins=None, what=""):
    """{stage: worst error / bar} of a run of chain() (0.0 where every bit must be and is equal); margins, a dict, gains the decision margins of the
    gait, turns and contacts statements.  AssertionError names every failing stage."""
    margins = {} if margins is None else margins
    ratios, failed = {}, {}
    for stage in STAGES:
        try:
            ratios[stage] = float(_WALK[stage](device_run, pipe, window, float(sigmas[stage]), margins))
            if not ratios[stage] <= 1.0:
                failed[stage] = f"worst error / bar = {ratios[stage]:.3g}"
        except AssertionError as e:
            failed[stage] = str(e)
        margin = f", decision margin {margins[stage]:.3g}" if stage in margins else ""
        print(f"{what} {stage} sigma {sigmas[stage]:g}: " + (f"FAILED: {failed[stage]}" if stage in failed else f"worst error / bar = {ratios[stage]:.3g}") + margin)
    if failed:
        raise StagesFailed(what, failed)
    return ratios


def contents(run):
    """What a run holds, so that no comparison is empty-handed: steps, turns, double supports, used strides (of the ankles' separation) per sequence."""
    return {"steps": run["gait"]["outputs"]["per_sequence"][:, 4], "turns": run["turns"]["outputs"]["per_sequence"][:, 0],
            "double_supports": run["contacts"]["outputs"]["per_sequence"][:, 3] + run["contacts"]["outputs"]["per_sequence"][:, 4],
            "cycles": run["kinematics"]["outputs"]["per_sequence"][:, 0, 0], "used": run["harmonics"]["outputs"]["per_sequence"][:, 0, 1],
            "pairs": run["regularity"]["outputs"]["per_sequence"][:, 0, 0]}
