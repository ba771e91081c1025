"""The Welch spectrum of the gait signals on the host: pipeline.gait_spectrum and pipeline.gait_welch, the numpy statements, against the
yardstick by numpy.fft of tests/helpers/spectrum_checks.py (the bar: 8 times the worst ratio measured over the shape set,
profiles/gait_spectrum_bounds.txt) and, where scipy imports, against scipy.signal.welch itself; the exact properties that need no measured number;
pipeline.spectrum_rows; csrc/gait_spectrum.h, the arithmetic the kernels run, through tests/helpers/gait_spectrum_check.cpp: a stand-alone program
(its own main, no HIP) built with AddressSanitizer and UBSan and run directly on files this test writes, whose printed bits must be the statement's;
every refusal, in the same words from the statement and from the header.  Every figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import entropy_checks as ec
from .helpers import regularity_checks as rc
from .helpers import spectrum_checks as sc


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


@pytest.fixture(scope="module")
def noisy():
    joints, trans, lengths, names, ex, table = ec.noisy_call(25)
    return rc.signals_of(joints, trans, table), lengths, ex


def test_statement_against_the_yardstick(pipe, noisy):
    worst, lines = sc.measure_bound(pipe.gait_welch, noisy)
    print("\n".join(lines))
    print(f"worst ratio {worst:.3e}, measured {sc.MEASURED:.1e}, bar {sc.BAR:.2e}")
    assert worst <= sc.BAR
    assert sc.BAR == 8.0 * sc.MEASURED and sc.MEASURED < 1e-13      # the bar is a few roundings of a sum, not a tolerance of convenience


@pytest.mark.parametrize("J", (25, 49))
def test_the_call_on_joints_is_the_hook_on_its_signals(pipe, J):
    joints, trans, lengths, names, ex, table = ec.noisy_call(J)
    for with_trans, with_ex in ((True, True), (False, False)):
        tr, e = trans if with_trans else None, ex if with_ex else None
        want_frame = rc.signals_of(joints, tr, table)
        for r in sc.RULES[:3]:
            out = pipe.gait_spectrum(joints, lengths, tr, e, joints=table, **sc.rule_of(*r))
            hook = pipe.gait_welch(want_frame, lengths, e, **sc.rule_of(*r))
            assert sc.same_bits(out["per_frame"], want_frame) and out["psd"].shape == (7, 4, r[3] // 2 + 1) and out["per_sequence"].shape == (7, 4, 13)
            assert all(sc.same_bits(out[k], hook[k]) for k in ("psd", "per_sequence", "spectral_entropy", "freqs"))
    full = pipe.gait_spectrum(joints, lengths, trans, None, joints=table)      # the defaults
    row = dict(zip(pipe.SPECTRUM_COLUMNS, full["per_sequence"][names.index("walk400_back"), 0]))
    print(row)
    assert row["n"] == 398 and row["candidates"] == 11 and row["used"] == 11 and abs(row["peak_hz"] - 20.0 / 27.3) < 0.5 * 20.0 / 256      # the walker's stride: 27.3 frames
    assert abs(row["cadence"] - 120.0 * 20.0 / 27.3) < 60.0 * 20.0 / 256 and 0 < row["peak_width_hz"] < 1.0 and 0 < full["spectral_entropy"][-1, 0] < 1
    assert sc.same_bits(full["freqs"], np.arange(129) * 20.0 / 256)


def test_scipy_welch_where_it_imports(pipe, noisy):
    """One valid run: scipy averages the segments of ONE run, as the statement does where the signal has one."""
    try:
        from scipy.signal import welch
    except ImportError:
        print("scipy does not import here: the numpy.fft yardstick stands alone")
        return
    x = np.random.default_rng(1967).standard_normal((400, 4))
    for d, L, hop, N in ((0, 64, 32, 256), (0, 8, 1, 8), (0, 256, 32, 1024), (0, 64, 64, 514)):
        out = pipe.gait_welch(x, **sc.rule_of(d, L, hop, N))
        for ch in range(4):
            f, want = welch(x[:, ch], fs=20.0, window="hann", nperseg=L, noverlap=L - hop, nfft=N, detrend="constant", scaling="density")
            worst = sc.ratio(out["psd"][0, ch], want)
            print(f"scipy: segment {L} hop {hop} nfft {N} channel {ch}: ratio {worst:.3e}")
            assert worst <= sc.BAR and np.allclose(f, out["freqs"], rtol=1e-15, atol=0)


def test_exact_bin_sinusoid(pipe):
    for k0 in (8, 13, 30, 38):
        out = pipe.gait_welch(sc.sinusoid(k0), **sc.rule_of(0, 64, 32, 256))
        row = out["per_sequence"][0]
        print(k0, dict(zip(pipe.SPECTRUM_COLUMNS, row[0])))
        assert (row[:, 5] == k0).all() and (np.abs(row[:, 6] - k0 * 20.0 / 256) <= 0.5 * 20.0 / 256).all()
        assert sc.same_bits(row[:3, 12], 120.0 * row[:3, 6]) and row[3, 12] == 60.0 * row[3, 6]
        assert (row[:, 4] >= row[:, 3]).all() and (row[:, 3] > 0).all() and (row[:, 9] <= 1).all()
        # the Hann main lobe of 64 frames at 20 fps: 1.44 bins of 20 / 64 Hz at half height, whatever the walker does
        assert (np.abs(row[:, 8] - 1.44 * 20.0 / 64) < 0.03).all()


def test_constant_signal_and_too_few_segments(pipe):
    flat = pipe.gait_welch(np.full((400, 4), 1.5), **sc.rule_of(0, 64, 32, 256))
    assert (flat["psd"] == 0).all() and (flat["per_sequence"][0, :, :5] == [400, 11, 11, 0, 0]).all() and np.isnan(flat["per_sequence"][0, :, 5:]).all()
    assert np.isnan(flat["spectral_entropy"]).all()
    x = np.random.default_rng(3).standard_normal((95, 4))
    short = pipe.gait_welch(x, **sc.rule_of(0, 64, 32, 256))
    assert np.isnan(short["psd"]).all() and (short["per_sequence"][0, :, :3] == [95, 1, 0]).all() and np.isnan(short["per_sequence"][0, :, 3:]).all()
    assert np.isnan(short["spectral_entropy"]).all()
    one = pipe.gait_welch(x, **sc.rule_of(0, 64, 32, 256, min_segments=1))
    assert np.isfinite(one["psd"]).all() and (one["per_sequence"][0, :, :3] == [95, 1, 1]).all() and (one["per_sequence"][0, :, 4] >= one["per_sequence"][0, :, 3]).all()
    single = pipe.gait_welch(x[:1], **sc.RULE)
    assert (single["per_sequence"][0, :, :3] == 0).all() and np.isnan(single["psd"]).all()


def test_segments_of_a_run(pipe):
    """A run one frame shorter than the segment lays none, a run of exactly the segment one, a run of segment + hop two; and the runs at the word
    boundary against the yardstick's plain loop."""
    for segment, hop, nfft in ((64, 32, 256), (8, 4, 32), (64, 8, 64)):
        x, lengths, ex = sc.runs_call(segment, hop)
        out = pipe.gait_welch(x, lengths, ex, **sc.rule_of(0, segment, hop, nfft, min_segments=1))
        assert out["per_sequence"][9:, 0, 1].tolist() == [1, 0, 2, 1, 3, 2]
        for d in (0, 1, 2):
            rule = sc.rule_of(d, segment, hop, nfft, min_segments=1)
            out = pipe.gait_welch(x, lengths, ex, **rule)
            a = 0
            for q, T in enumerate(lengths):
                want, n, candidates, used = sc.yardstick(x[a:a + T, 1], ex[a:a + T], **rule)
                assert out["per_sequence"][q, 1, :3].tolist() == [n, candidates, used] and sc.ratio(out["psd"][q, 1], want) <= sc.BAR
                a += T
    # a turn splits the walk into straight runs instead of discarding it: the segments of both runs are averaged
    x = np.random.default_rng(11).standard_normal((400, 4))
    ex = np.zeros(400, np.int32)
    ex[150:190] = 1
    out = pipe.gait_welch(x, exclude=ex, **sc.rule_of(0, 64, 32, 256))
    assert (out["per_sequence"][0, :, :3] == [360, 3 + 5, 8]).all()


def test_sequences_do_not_see_each_other(pipe):
    joints, trans, lengths, names, ex, table = ec.noisy_call(25)
    for sigma in (0.0, 2.0):
        whole = pipe.gait_spectrum(joints, lengths, trans, ex, sigma=sigma, **sc.RULE)
        a = 0
        for q, n in enumerate(lengths):
            alone = pipe.gait_spectrum(joints[a:a + n], None, trans[a:a + n], ex[a:a + n], sigma=sigma, **sc.RULE)
            assert sc.same_bits(whole["per_frame"][a:a + n], alone["per_frame"]) and sc.same_bits(whole["psd"][q], alone["psd"][0]), names[q]
            assert sc.same_bits(whole["per_sequence"][q], alone["per_sequence"][0]) and sc.same_bits(whole["spectral_entropy"][q], alone["spectral_entropy"][0]), names[q]
            a += n
        reg = pipe.gait_regularity(joints, lengths, trans, ex, sigma=sigma)
        assert sc.same_bits(whole["per_frame"], reg["per_frame"])


def test_spectrum_rows(pipe):
    psd = np.zeros((3, 129))
    rows = np.zeros((3, 13))
    rows[:, 2] = (4, 4, 0)
    psd[0, 7:39] = 1.0                                          # white inside the band 7 .. 38: entropy 1
    psd[1, 20] = 5.0                                            # one line: entropy 0
    psd[2, 7:39] = 1.0                                          # used is 0
    out = pipe.spectrum_rows(psd, rows)["spectral_entropy"]
    print(out)
    assert abs(out[0] - 1.0) < 1e-14 and out[1] == 0.0 and np.isnan(out[2])
    two = psd[:2].copy()
    two[0, 7:39] = np.arange(1, 33)
    p = np.arange(1, 33) / np.arange(1, 33).sum()
    assert abs(pipe.spectrum_rows(two, rows[:2])["spectral_entropy"][0] - float(-(p * np.log(p)).sum() / math.log(32))) < 1e-14
    assert np.isnan(pipe.spectrum_rows(psd, rows, f_lo=1.0, f_hi=1.05)["spectral_entropy"]).all()      # one bin (13) in the band
    assert pipe.spectrum_rows(psd.reshape(1, 3, 129), rows.reshape(1, 3, 13))["spectral_entropy"].shape == (1, 3)
    for bad in ((np.zeros((2, 129)), np.zeros((2, 12))), (np.zeros((2, 129)), np.zeros((3, 13))), (np.zeros((2, 3)), np.zeros((2, 13)))):
        with pytest.raises(ValueError, match="psd"):
            pipe.spectrum_rows(*bad)


BAD = ((dict(fps=0.0), "fps must be positive and finite"), (dict(fps=float("nan")), "fps must be positive and finite"), (dict(fps=float("inf")), "fps must be positive and finite"),
       (dict(derivative=-1), "derivative outside [0, 2]"), (dict(derivative=3), "derivative outside [0, 2]"), (dict(segment=6, hop=3), "segment must be even and within [8, 256]"),
       (dict(segment=63), "segment must be even and within [8, 256]"), (dict(segment=258, hop=64, nfft=512), "segment must be even and within [8, 256]"),
       (dict(hop=7), "hop outside [segment / 8, segment]"), (dict(hop=65), "hop outside [segment / 8, segment]"), (dict(nfft=62), "nfft must be even and within [segment, 1024]"),
       (dict(nfft=255), "nfft must be even and within [segment, 1024]"), (dict(nfft=1026), "nfft must be even and within [segment, 1024]"),
       (dict(f_lo=0.0), "f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2"), (dict(f_lo=3.0), "f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2"),
       (dict(f_hi=10.5), "f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2"), (dict(f_lo=float("nan")), "f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2"),
       (dict(min_segments=0), "min_segments outside [1, 2^20]"), (dict(min_segments=2 ** 20 + 1), "min_segments outside [1, 2^20]"))
LONG = "sequence 0 has 32769 frames, more than 32768 (the work is quadratic in them)"


def test_bad_arguments_are_refused(pipe):
    joints, trans = rc.walker(30)
    for kw, why in BAD:
        for call in (lambda: pipe.gait_spectrum(joints, **kw), lambda: pipe.gait_welch(np.zeros((30, 4)), **kw)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == why
    for kw, word in ((dict(joints=(0, 20, 12, 16, 14, 18, 15, 25)), "joints"), (dict(joints=(0, 1, 2)), "joints"), (dict(lengths=[10, 19]), "lengths"), (dict(sigma=-1.0), "sigma"),
                     (dict(sigma=float("nan")), "sigma"), (dict(sigma=16.5), "sigma"), (dict(segment=8.5), "whole"), (dict(nfft=256.5), "whole"), (dict(trans=np.zeros((29, 3))), "trans"),
                     (dict(exclude=np.zeros(29, np.int32)), "exclude")):
        with pytest.raises(ValueError, match=word):
            pipe.gait_spectrum(joints, **kw)
    with pytest.raises(ValueError, match="joints3d"):
        pipe.gait_spectrum(np.zeros((3, 25, 2)))
    with pytest.raises(ValueError, match="signals"):
        pipe.gait_welch(np.zeros((30, 3)))
    for call in (lambda: pipe.gait_welch(np.zeros((32769 + 5, 4)), lengths=[32769, 5]), lambda: pipe.gait_spectrum(np.zeros((32769, 25, 3), np.float32))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == LONG
    assert (pipe.gait_welch(np.zeros((32768, 4)), segment=256, hop=256, nfft=256)["per_sequence"][0, :, :3] == (32766, 127, 127)).all()        # the longest is taken
    assert pipe.SPECTRUM_CHANNELS == ("sep", "lift", "sway", "bob") and len(pipe.SPECTRUM_COLUMNS) == 13 and pipe.SPECTRUM_MAX_FRAMES == 32768


def test_header_on_the_host_under_sanitizers(pipe, noisy, tmp_path):
    """csrc/gait_spectrum.h itself against the statement: one file per sequence of every case of the shape set (the noisy call's signals over
    spectrum_checks.RULES, with and without exclude; the runs at the word boundary and of a segment's length), the exact-bin sinusoid and the
    constant signal; every refusal, in the statement's words."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_spectrum_check.cpp")
    exe = str(tmp_path / "gait_spectrum_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    cases = sc.shape_set(noisy)
    cases.append(("sine", sc.sinusoid(13), [400], None, sc.rule_of(0, 64, 32, 256)))
    cases.append(("flat", np.full((400, 4), 1.5), [400], None, sc.rule_of(0, 64, 32, 256)))
    files, want = [], {}
    for name, x, lengths, ex, rule in cases:
        host = pipe.gait_welch(x, lengths, ex, **rule)
        a = 0
        for q, T in enumerate(lengths):
            path = sc.write_case(str(tmp_path / f"{name}_{q}.bin"), x[a:a + T], None if ex is None else ex[a:a + T], rule)
            files.append(path)
            want[path] = (host["psd"][q], host["per_sequence"][q])
            a += T
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
    got = sc.parse_output(r.stdout)
    assert len(got) == 8 * len(files)
    for path, (psd, rows) in want.items():
        for ch in range(4):
            assert sc.same_bits(got["psd", path, ch], psd[ch]), (path, ch)
            assert sc.same_bits(got["row", path, ch], rows[ch]), (path, ch, got["row", path, ch], rows[ch])
    refused = [(sc.write_case(str(tmp_path / f"bad{k}.bin"), np.zeros((30, 4)), None, dict(sc.RULE, **kw), True), why) for k, (kw, why) in enumerate(BAD)]
    refused.append((sc.write_case(str(tmp_path / "long.bin"), np.zeros((32769, 4)), None, sc.RULE, True), LONG))
    r = subprocess.run([exe] + [path for path, _ in refused], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "ok" and lines[:-1] == [f"refused {path}: {why}" for path, why in refused], r.stdout[-4000:] + r.stderr[-4000:]
