"""Movement smoothness of the gait signals on the host: pipeline.gait_smoothness and pipeline.gait_sparc, the numpy statements, against the
yardstick by numpy.fft of tests/helpers/smoothness_checks.py (the condition: a decision margin of at least 1e-9; the bar: 8 times the worst ratio
measured over the rule sets, profiles/gait_smoothness_bounds.txt); the exact properties that need no measured number; pipeline.smoothness_rows;
csrc/gait_smoothness.h, the arithmetic the kernels run, through tests/helpers/gait_smoothness_check.cpp: a stand-alone program (its own main, no HIP)
built with AddressSanitizer and UBSan and run directly on files this test writes, whose printed bits must be the statement's; every refusal, in the
same words from the statement and from the header.  Every figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import entropy_checks as ec
from .helpers import regularity_checks as rc
from .helpers import smoothness_checks as mc


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


@pytest.fixture(scope="module")
def noisy():
    joints, trans, lengths, names, ex, table = ec.noisy_call(25)
    return rc.signals_of(joints, trans, table), lengths, ex


def test_statement_against_the_yardstick(pipe, noisy):
    assert list(noisy[1]) == [130, 1, 19, 20, 64, 65, 400] and int((noisy[2] != 0).sum()) == 35
    worst, margin, lines = mc.measure_bound(pipe.gait_sparc, noisy)
    print("\n".join(lines))
    print(f"worst ratio {worst:.3e}, measured {mc.MEASURED:.1e}, bar {mc.BAR:.2e}, smallest margin {margin:.3e}")
    assert margin >= mc.MARGIN                                  # the condition on the inputs, not a tolerance
    assert worst <= mc.BAR
    assert mc.BAR == 8.0 * mc.MEASURED and mc.MEASURED < 1e-12      # the bar is a few roundings of a sum, not a tolerance of convenience


@pytest.mark.parametrize("J", (25, 49))
def test_the_call_on_joints_is_the_hook_on_its_signals(pipe, J):
    joints, trans, lengths, names, ex, table = ec.noisy_call(J)
    for with_trans, with_ex in ((True, True), (False, False)):
        tr, e = trans if with_trans else None, ex if with_ex else None
        want_frame = rc.signals_of(joints, tr, table)
        for r in mc.RULES[:3]:
            out = pipe.gait_smoothness(joints, lengths, tr, e, joints=table, **mc.rule_of(*r))
            hook = pipe.gait_sparc(want_frame, lengths, e, **mc.rule_of(*r))
            assert mc.same_bits(out["per_frame"], want_frame) and out["per_sequence"].shape == (7, 4, 10) and out["per_segment"].shape == (out["slot_offsets"][-1], 4, 8)
            assert all(mc.same_bits(out[k], hook[k]) for k in ("per_segment", "per_sequence", "ldlj", "ldlj_mean", "ldlj_sd")) and (out["slot_offsets"] == hook["slot_offsets"]).all()
    full = pipe.gait_smoothness(joints, lengths, trans, None, joints=table)      # the defaults: derivative 1, 64 frames, 1024 points, 10 Hz, 0.05
    q = names.index("walk400_back")
    row = dict(zip(pipe.SMOOTHNESS_COLUMNS, full["per_sequence"][q, 0]))
    print(row, full["ldlj_mean"][q, 0], full["ldlj_sd"][q, 0])
    assert full["slot_offsets"].tolist() == [0, 3, 3, 3, 3, 4, 5, 16]
    assert row["n"] == 399 and row["candidates"] == 11 and row["used"] == 11 and row["defined"] == 11 and row["dj_defined"] == 11
    assert row["sparc_min"] <= row["sparc_mean"] <= row["sparc_max"] < 0 and row["sparc_sd"] > 0 and 0 < row["last_hz_mean"] <= 10.0 and full["ldlj_mean"][q, 0] < 0
    assert pipe.smoothness_slots(lengths, 64, 32).tolist() == full["slot_offsets"].tolist()


def test_the_leakage_floor_of_a_noiseless_sinusoid(pipe):
    """DESIGN 4.24's caveat, on the project's walker without noise: sep's speed profile is a sinusoid, and the rectangular window of 64 frames alone
    gives SPARC = -3.96 +- 0.30 over its 11 segments (-4.43 to -3.65 by where the segment starts in the cycle), whatever the walker does."""
    joints, trans = rc.walker(400)
    out = pipe.gait_smoothness(joints, None, trans)
    row = dict(zip(pipe.SMOOTHNESS_COLUMNS, out["per_sequence"][0, 0]))
    print(row, out["ldlj_mean"][0, 0])
    assert row["used"] == 11 and abs(row["sparc_mean"] + 3.96) < 0.02 and abs(row["sparc_sd"] - 0.30) < 0.02 and abs(out["ldlj_mean"][0, 0] + 10.9) < 0.1


def test_exact_properties(pipe):
    # a bin-centred cosine with nfft = segment sits on its bin alone: the band is one bin and the arc has no length
    for k0 in (3, 11):
        out = pipe.gait_sparc(mc.centred_cosine(k0), **mc.rule_of(0, 64, 32, 64))
        seg = out["per_segment"][:, 0]
        print(k0, seg[0])
        assert (seg[:, 2] == k0).all() and (seg[:, 3] == k0).all() and (seg[:, 4] == k0).all() and (seg[:, 1] == 0.0).all() and not np.signbit(seg[:, 1]).any()
        assert (out["per_sequence"][0, :, 4:8] == 0.0).all() and mc.yardstick(mc.centred_cosine(k0)[:, 0], **mc.rule_of(0, 64, 32, 64))[4] >= 0.05 - 1e-12
    # an all-zero signal: no peak, NaN behind start, and nothing defined
    zero = pipe.gait_sparc(np.zeros((200, 4)), **mc.RULE)
    assert (zero["per_segment"][:, :, 0] == np.arange(0, 160, 32)[:, None]).all() and np.isnan(zero["per_segment"][:, :, 1:]).all()
    assert (zero["per_sequence"][0, :, :4] == [199, 5, 5, 0]).all() and np.isnan(zero["per_sequence"][0, :, 4:9]).all() and (zero["per_sequence"][0, :, 9] == 0).all()
    assert np.isnan(zero["ldlj"]).all() and np.isnan(zero["ldlj_mean"]).all()
    # amplitude = 1 leaves only the peak's bin
    x = np.random.default_rng(5).standard_normal((200, 4))
    one = pipe.gait_sparc(x, **mc.rule_of(1, 64, 32, 1024, amplitude=1.0))["per_segment"]
    assert (one[..., 2] == one[..., 4]).all() and (one[..., 3] == one[..., 4]).all() and (one[..., 1] == 0.0).all() and np.isfinite(one[..., 6]).all()
    # a power of two scales every product exactly: the ratios, the band and the jerk over the squared speed keep their bits
    a, b = pipe.gait_sparc(x, **mc.RULE)["per_segment"], pipe.gait_sparc(x * 2.0 ** -7, **mc.RULE)["per_segment"]
    assert mc.same_bits(a[..., :5], b[..., :5]) and mc.same_bits(a[..., 6], b[..., 6]) and mc.same_bits(a[..., 5] * 2.0 ** -7, b[..., 5])
    assert (a[..., 2] <= a[..., 4]).all() and (a[..., 4] <= a[..., 3]).all()
    # a sequence shorter than the segment has no slot
    short = pipe.gait_sparc(x[:63], **mc.RULE)
    assert short["per_segment"].shape == (0, 4, 8) and short["slot_offsets"].tolist() == [0, 0] and (short["per_sequence"][0, :, :3] == [62, 0, 0]).all()
    assert np.isnan(short["per_sequence"][0, :, 3:]).all()
    # min_segments above the candidates: a NaN row, the segment rows still there
    few = pipe.gait_sparc(x, **mc.rule_of(1, 64, 32, 1024, min_segments=6))
    assert (few["per_sequence"][0, :, :3] == [199, 5, 0]).all() and np.isnan(few["per_sequence"][0, :, 3:]).all() and np.isnan(few["ldlj_mean"]).all()
    assert mc.same_bits(few["per_segment"], a) and np.isfinite(few["ldlj"]).all()
    # NaN frames split the sequence into runs shorter and longer than the segment
    runs = pipe.gait_sparc(mc.runs_signal(), **mc.rule_of(0, 64, 32, 1024))
    assert runs["per_segment"][:, 0, 0].tolist()[:5] == [31.0, 160.0, 192.0, 224.0, 311.0] and np.isnan(runs["per_segment"][5:, 0]).all() and runs["per_segment"].shape[0] == 11


def test_sequences_do_not_see_each_other(pipe):
    joints, trans, lengths, names, ex, table = ec.noisy_call(25)
    for sigma in (0.0, 2.0):
        whole = pipe.gait_smoothness(joints, lengths, trans, ex, sigma=sigma, **mc.RULE)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_smoothness(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], sigma=sigma, **mc.RULE)
            lo, hi = whole["slot_offsets"][q:q + 2]
            assert mc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]) and mc.same_bits(whole["per_segment"][lo:hi], alone["per_segment"]), names[q]
            assert mc.same_bits(whole["per_sequence"][q], alone["per_sequence"][0]) and mc.same_bits(whole["ldlj_mean"][q], alone["ldlj_mean"][0]), names[q]
            a += n
        reg = pipe.gait_regularity(joints, lengths, trans, ex, sigma=sigma)
        assert mc.same_bits(whole["per_frame"], reg["per_frame"])


def test_smoothness_rows(pipe):
    seg = np.full((3, 4, 8), np.nan)
    rows = np.zeros((2, 4, 10))
    rows[0, :, 2] = 2
    seg[:, :, 6] = np.array([math.e, math.e ** 3, 0.0])[:, None]
    out = pipe.smoothness_rows(seg, rows, [0, 2, 3])
    print(out)
    assert np.allclose(out["ldlj"][:2], [[-1.0] * 4, [-3.0] * 4], rtol=0, atol=1e-15) and np.isnan(out["ldlj"][2]).all()
    assert np.allclose(out["ldlj_mean"][0], -2.0) and np.allclose(out["ldlj_sd"][0], 1.0) and np.isnan(out["ldlj_mean"][1]).all() and np.isnan(out["ldlj_sd"][1]).all()
    for bad in ((seg[:, :3], rows, [0, 2, 3]), (seg, rows[:, :, :9], [0, 2, 3]), (seg, rows, [0, 3]), (seg, rows, [0, 2, 4]), (seg, rows, [1, 2, 3])):
        with pytest.raises(ValueError, match="per_segment|slot_offsets"):
            pipe.smoothness_rows(*bad)


BAD = ((dict(fps=0.0), "fps must be positive and finite"), (dict(fps=float("nan")), "fps must be positive and finite"), (dict(fps=float("inf")), "fps must be positive and finite"),
       (dict(derivative=-1), "derivative outside [0, 2]"), (dict(derivative=3), "derivative outside [0, 2]"), (dict(segment=6, hop=3), "segment must be even and within [8, 256]"),
       (dict(segment=63), "segment must be even and within [8, 256]"), (dict(segment=258, hop=64), "segment must be even and within [8, 256]"),
       (dict(hop=7), "hop outside [segment / 8, segment]"), (dict(hop=65), "hop outside [segment / 8, segment]"),
       (dict(min_segments=0), "min_segments outside [1, 2^20]"), (dict(min_segments=2 ** 20 + 1), "min_segments outside [1, 2^20]"),
       (dict(nfft=62), "nfft must be even and within [segment, 4096]"), (dict(nfft=1023), "nfft must be even and within [segment, 4096]"),
       (dict(nfft=4098), "nfft must be even and within [segment, 4096]"), (dict(f_cut=0.0), "f_cut must obey 0 < f_cut <= fps / 2"),
       (dict(f_cut=10.5), "f_cut must obey 0 < f_cut <= fps / 2"), (dict(f_cut=float("nan")), "f_cut must obey 0 < f_cut <= fps / 2"),
       (dict(amplitude=0.0), "amplitude must be within (0, 1]"), (dict(amplitude=1.5), "amplitude must be within (0, 1]"), (dict(amplitude=float("nan")), "amplitude must be within (0, 1]"))
LONG = "sequence 0 has 32769 frames, more than 32768 (the work is quadratic in them)"


def test_bad_arguments_are_refused(pipe):
    joints, trans = rc.walker(30)
    for kw, why in BAD:
        for call in (lambda: pipe.gait_smoothness(joints, **kw), lambda: pipe.gait_sparc(np.zeros((30, 4)), **kw)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == why
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(sigma=-1.0), "sigma"),
                     (dict(sigma=float("nan")), "sigma"), (dict(sigma=16.5), "sigma"), (dict(segment=8.5), "whole"), (dict(nfft=256.5), "whole"), (dict(trans=np.zeros((29, 3))), "trans"),
                     (dict(exclude=np.zeros(29, np.int32)), "exclude")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_smoothness(joints, **kw)
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_smoothness(np.zeros((3, 25, 2)))
    with pytest.raises(ValueError, match="signals"):
        pipe.gait_sparc(np.zeros((30, 3)))
    for call in (lambda: pipe.gait_sparc(np.zeros((32769 + 5, 4)), lengths=[32769, 5]), lambda: pipe.gait_smoothness(np.zeros((32769, 25, 3), np.float32))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == LONG
    assert pipe.gait_sparc(np.zeros((30, 4)), fps=8.0)["per_sequence"].shape == (1, 4, 10)      # f_cut defaults to min(10, fps / 2)
    assert pipe.SMOOTHNESS_CHANNELS is pipe.REGULARITY_CHANNELS and len(pipe.SMOOTHNESS_COLUMNS) == 10 and len(pipe.SMOOTHNESS_SEGMENT_COLUMNS) == 8
    assert pipe.SMOOTHNESS_MAX_FRAMES == 32768


def test_header_on_the_host_under_sanitizers(pipe, noisy, tmp_path):
    """csrc/gait_smoothness.h itself against the statement: one file per sequence of every rule set on the noisy call's signals, with and without
    exclude, the centred cosine, the zeros, amplitude 1 and the runs; every refusal, in the statement's words."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_smoothness_check.cpp")
    exe = str(tmp_path / "gait_smoothness_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    signals, lengths, ex = noisy
    cases = [(f"noisy{k}", signals, lengths, ex if k % 2 == 0 else None, mc.rule_of(*r)) for k, r in enumerate(mc.RULES)]
    cases.append(("cosine", mc.centred_cosine(11), [200], None, mc.rule_of(0, 64, 32, 64)))
    cases.append(("zeros", np.zeros((200, 4)), [200], None, mc.RULE))
    cases.append(("one", np.random.default_rng(5).standard_normal((200, 4)), [200], None, mc.rule_of(1, 64, 32, 1024, amplitude=1.0)))
    cases.append(("runs", mc.runs_signal(), [400], None, mc.rule_of(0, 64, 32, 1024, min_segments=6)))
    files, want = [], {}
    for name, x, lens, e, rule in cases:
        host = pipe.gait_sparc(x, lens, e, **rule)
        a = 0
        for q, T in enumerate(lens):
            path = mc.write_case(str(tmp_path / f"{name}_{q}.bin"), x[a:a + T], None if e is None else e[a:a + T], rule)
            files.append(path)
            want[path] = (host["per_segment"][host["slot_offsets"][q]:host["slot_offsets"][q + 1]], host["per_sequence"][q])
            a += T
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
    got = mc.parse_output(r.stdout)
    assert len(got) == 8 * len(files)
    for path, (seg, rows) in want.items():
        for ch in range(4):
            assert mc.same_bits(got["seg", path, ch], seg[:, ch].reshape(-1)), (path, ch)
            assert mc.same_bits(got["row", path, ch], rows[ch]), (path, ch, got["row", path, ch], rows[ch])
    refused = [(mc.write_case(str(tmp_path / f"bad{k}.bin"), np.zeros((30, 4)), None, dict(mc.RULE, **kw), True), why) for k, (kw, why) in enumerate(BAD)]
    refused.append((mc.write_case(str(tmp_path / "long.bin"), np.zeros((32769, 4)), None, mc.RULE, True), LONG))
    r = subprocess.run([exe] + [path for path, _ in refused], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "ok" and lines[:-1] == [f"refused {path}: {why}" for path, why in refused], r.stdout[-4000:] + r.stderr[-4000:]
