"""The camera-space translation on the host: pipeline.fit_translation, the numpy float64 statement, against the golden reference
values (two bars: both sides err) and the exact checker tests/helpers/translation_checks.py (one bar, cond_2(A) 2^-52), with non-square centres
against the checker alone; the fill bit-identical to numpy.linspace; the status rules; and csrc/translation3.h, the arithmetic the kernels run,
through tests/helpers/translation3_check.cpp: a stand-alone program (its own main, no HIP, nothing of the library but that header) built with
AddressSanitizer and UBSan and run directly on cases written out here -- its rows must equal the statement's bit for bit, since both round once
per operation in the same order.  The C export is checked here too.  Every worst ratio is printed before it is asserted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import translation_checks as tc


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


def shown(worst):
    return {k: float(f"{v:.3g}") for k, v in worst.items()}


def test_export_and_pair_table(pkg, pipe):
    lib = pkg._lib.load()
    assert "grnet_fit_translation" in pkg._lib.EXPORTS and hasattr(lib, "grnet_fit_translation")
    assert len(pkg._lib.EXPORTS["grnet_fit_translation"][1]) == 18
    assert lib.grnet_fit_translation(None, None, 25, None, 25, 1, None, 1, None, 13, None, 0.1, 4, 0, 1, None, None, None) == pkg._lib.EINVAL
    assert pipe.BODY25_FROM_KINECTV2 == ((0, 8), (4, 5), (5, 6), (6, 7), (8, 2), (9, 3), (10, 4), (12, 12), (13, 13), (14, 14), (16, 9), (17, 10), (18, 11))
    assert hasattr(pkg.GRNet, "fit_translation")


def test_statement_against_golden_and_checker(pipe):
    g = np.load(os.path.join(ROOT, "tests", "golden", "translation.npz"))
    worst_golden = 0.0
    for ci in range(3):
        for K in (13, 25):
            name = f"c{ci}_k{K}"
            j3, j2, (size, f), t_ref = g[name + "_joints3d"], g[name + "_joints2d"], g[name + "_camera"], g[name + "_t"]
            pairs = np.stack([np.arange(K)] * 2, axis=1)
            kw = dict(focal_length=f, centre=(size / 2, size / 2), conf_threshold=0.0)
            out = pipe.fit_translation(j3, j2, pairs, **kw)
            fails, worst = tc.compare(out, j3, j2, pairs, **kw)
            assert (out["per_frame"][:, 5] == 0).all()
            for i in range(j3.shape[0]):                       # against the reference itself: twice the bar
                cond = tc.frame_truth(tc.widen(j3)[i], tc.widen(j2)[i], f, size / 2, size / 2, 0.0, 4)[3]
                worst_golden = max(worst_golden, np.abs(out["per_frame"][i, :3] - t_ref[i]).max() / np.abs(t_ref[i]).max() / (2 * cond * tc.EPS))
            print(name, shown(worst))
            assert fails == [], fails
    print(f"worst ratio to the golden bar: {worst_golden:.3g}")
    assert worst_golden <= 1.0


CASES = (   # P, K3, K2, n, lengths, (f, cx, cy) per sequence, image size, depth
    (13, 25, 25, 24, [24], [(2202.9, 960.0, 540.0)], (1920, 1080), (2.0, 8.0)),
    (25, 29, 25, 21, [1, 2, 18], [(1000.0, 960.0, 540.0), (1500.0, 640.0, 360.0), (2202.9, 900.0, 500.0)], (1920, 1080), (2.0, 8.0)),
    (64, 70, 66, 9, [4, 5], [(5000.0, 112.0, 96.0), (5000.0, 100.0, 112.0)], (224, 192), (30.0, 60.0)),
    (4, 6, 5, 12, [12], [(1200.0, 320.0, 240.0)], (640, 480), (2.0, 8.0)),
)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"P{c[0]}")
def test_statement_against_checker_with_non_square_centres(pipe, case):
    j3, j2, pairs, kw = tc.make_case(case, 3)
    if case[0] == 4:
        j2[5, pairs[0, 1], 2] = 0.0                            # three pairs left: too few for min_joints = 4
    out = pipe.fit_translation(j3, j2, pairs, **kw)
    fails, worst = tc.compare(out, j3, j2, pairs, **kw)
    print(shown(worst))
    assert fails == [], fails
    assert worst["cond"] <= tc.MAX_COND


def unfit(j2, frames):
    j2 = j2.copy()
    j2[list(frames), :, 2] = 0.0
    return j2


def test_fill_is_numpy_linspace_bit_for_bit(pipe):
    case = (13, 25, 25, 90, [90], [(2202.9, 960.0, 540.0)], (1920, 1080), (2.0, 8.0))
    j3, j2, pairs, kw = tc.make_case(case, 5)
    dead = [0, 1, 5, 9, 10] + list(range(14, 84)) + [88, 89]    # runs at the front and the end, inner runs of 1, 2 and 70
    j2 = unfit(j2, dead)
    out = pipe.fit_translation(j3, j2, pairs, **kw)
    rows = out["per_frame"]
    want = np.zeros(90)
    want[dead] = 3
    assert np.array_equal(rows[:, 5], want)
    assert np.array_equal(rows[0, :3], rows[2, :3]) and np.array_equal(rows[1, :3], rows[2, :3]) and np.array_equal(rows[89, :3], rows[87, :3])
    assert np.array_equal(rows[5, :3], np.linspace(rows[4, :3], rows[6, :3], 3)[1])
    assert np.array_equal(rows[14:84, :3], np.linspace(rows[13, :3], rows[84, :3], 72)[1:-1])
    assert np.isnan(rows[dead, 3]).all() and (rows[dead, 4] == 0).all()
    assert out["per_sequence"][0, :2].tolist() == [90 - len(dead), len(dead)]
    fails, worst = tc.compare(out, j3, j2, pairs, **kw)
    assert fails == [], fails
    plain = pipe.fit_translation(j3, j2, pairs, fill=False, **kw)
    assert (plain["per_frame"][dead, 5] == 1).all() and np.isnan(plain["per_frame"][dead, :4]).all() and plain["per_sequence"][0, 1] == 0
    live = np.setdiff1d(np.arange(90), dead)
    assert np.array_equal(plain["per_frame"][live], rows[live])
    assert tc.compare(plain, j3, j2, pairs, fill=False, **kw)[0] == []
    # a sequence without a fitted frame keeps its NaN rows and statuses; its neighbours are filled on their own
    kw3 = dict(kw, lengths=[30, 30, 30], focal_length=[2202.9] * 3, centre=[(960.0, 540.0)] * 3)
    none = pipe.fit_translation(j3, unfit(j2, range(30, 60)), pairs, **kw3)
    assert (none["per_frame"][30:60, 5] == 1).all() and np.isnan(none["per_frame"][30:60, :4]).all()
    assert none["per_sequence"][1, :2].tolist() == [0, 0] and np.isnan(none["per_sequence"][1, 2]) and none["per_sequence"][1, 3] == 0
    assert tc.compare(none, j3, unfit(j2, range(30, 60)), pairs, **kw3)[0] == []


def test_status_rules(pipe):
    case = (13, 25, 25, 8, [8], [(1000.0, 960.0, 540.0)], (1920, 1080), (2.0, 8.0))
    j3, j2, pairs, kw = tc.make_case(case, 7)
    j2[:, pairs[:, 1], 2] = 0.5
    thr = float(np.float32(0.25))
    j2[0, pairs[4:, 1], 2] = 0.0                                # exactly min_joints = 4 used pairs: fitted
    j2[1, pairs[3:, 1], 2] = 0.0                                # three: too few
    j2[2, pairs[:4, 1], 2] = thr                                # a confidence EQUAL to the threshold is not used ...
    j2[3, pairs[:4, 1], 2] = np.nextafter(np.float32(thr), np.float32(1))   # ... the next float32 above it is
    j2[4, pairs[0, 1], 2] = np.inf                              # a non-finite confidence drops the pair
    j2[4, pairs[1, 1], 2] = np.nan
    j3[5, pairs[:, 0], :2] *= -1.0                              # the body turned half round the optical axis: the detections are its mirror image
                                                                # through the centre, which a pinhole shows of a body BEHIND it -- the solve succeeds, Z + tz < 0
    j2[6, pairs[:, 1], :2] = (960.0, 540.0)                     # every detection at the centre: u = v = 0, the third pivot is exactly zero
    j3[7, pairs[2, 0], 1] = np.nan                              # a NaN coordinate of a used joint: a non-finite result
    kw = dict(kw, conf_threshold=thr, fill=False)
    rows = pipe.fit_translation(j3, j2, pairs, **kw)["per_frame"]
    assert rows[:, 5].tolist() == [0, 1, 0, 0, 0, 2, 2, 2]
    assert rows[:, 4].tolist() == [4, 3, 9, 13, 11, 13, 13, 13]
    assert np.isnan(rows[[1, 5, 6, 7], :4]).all() and np.isfinite(rows[[0, 2, 3, 4], :4]).all()
    assert tc.compare({"per_frame": rows, "per_sequence": pipe.fit_translation(j3, j2, pairs, **kw)["per_sequence"]}, j3, j2, pairs, **kw)[0] == []
    assert pipe.fit_translation(j3, j2, pairs, **dict(kw, min_joints=5))["per_frame"][0, 5] == 1


def test_bad_arguments_are_refused(pipe):
    j3, j2 = np.zeros((4, 25, 3)), np.ones((4, 25, 3))
    pairs = pipe.BODY25_FROM_KINECTV2
    for args, kw, word in (((j3[0], j2, pairs), {}, "joints3d"), ((j3, j2[:3], pairs), {}, "frames"), ((j3, j2, pairs), {"lengths": [2, 1]}, "lengths"),
                           ((j3, j2, [(0, 25)]), {}, "pair index"), ((j3, j2, [(25, 0)]), {}, "pair index"), ((j3, j2, np.zeros((65, 2), int)), {}, "pairs"),
                           ((j3, j2, np.zeros((0, 2), int)), {}, "pairs"), ((j3, j2, pairs), {"focal_length": 0.0}, "focal_length"),
                           ((j3, j2, pairs), {"focal_length": np.inf}, "focal_length"), ((j3, j2, pairs), {"focal_length": [1.0, 2.0]}, "focal_length"),
                           ((j3, j2, pairs), {"centre": (np.nan, 1.0)}, "centre"), ((j3, j2, pairs), {"min_joints": 1}, "min_joints"),
                           ((j3, j2, pairs), {"root": 25}, "root"), ((j3, j2, pairs), {"conf_threshold": -0.1}, "conf_threshold")):
        with pytest.raises(ValueError, match=word):
            pipe.fit_translation(*args, **kw)


def run_header(tmp_path, j3, j2, pairs, cam, threshold, min_joints, fills):
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "translation3_check.cpp")
    exe = str(tmp_path / "translation3_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    n = j3.shape[0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([n, j3.shape[1], j2.shape[1], len(pairs), min_joints, len(fills)], np.int32).tobytes())
        f.write(np.ascontiguousarray(pairs, np.int32).tobytes())
        f.write(np.array(list(cam) + [threshold], np.float64).tobytes())
        f.write(np.ascontiguousarray(j3, np.float32).tobytes())
        f.write(np.ascontiguousarray(j2, np.float32).tobytes())
        f.write(np.array(fills, np.float64).reshape(-1, 7).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
    out = np.fromfile(tmp_path / "out.bin", np.float64)
    rows, rest = out[:n * 6].reshape(n, 6), out[n * 6:]
    filled = []
    for c in fills:
        gap = int(c[6])
        filled.append(rest[:gap * 3].reshape(gap, 3))
        rest = rest[gap * 3:]
    assert rest.size == 0
    return rows, filled


def test_header_on_the_host_under_sanitizers(pipe, tmp_path):
    """The statement's cases, the status cases and the fills through translation3.h itself."""
    case = (25, 29, 25, 40, [40], [(1500.0, 640.0, 360.0)], (1280, 720), (2.0, 8.0))
    j3, j2, pairs, kw = tc.make_case(case, 9)
    j2[3, pairs[3:, 1], 2] = 0.0                                # too few
    j3[4, pairs[:, 0], :2] *= -1.0                              # behind the camera (the mirror image through the centre)
    j3[6, pairs[2, 0], 1] = np.nan                              # non-finite
    j2[7, pairs[0, 1], 2] = np.inf
    g = np.random.Generator(np.random.Philox(key=[9, 9]))
    fills = []
    for gap in (1, 2, 3, 7, 70, 399):
        prev, nxt = g.normal(0, 3, 3), g.normal(0, 3, 3)
        fills.append(list(prev) + list(nxt) + [gap])
    prev = g.normal(0, 3, 3)
    fills.append(list(prev) + [prev[0], 1.0, 2.0] + [5])       # an equal component: numpy's zero-step branch, for all three components
    fills.append(list(prev) + list(prev) + [4])
    rows, filled = run_header(tmp_path, j3, j2, pairs, (1500.0, 640.0, 360.0), 0.1, 4, fills)
    want = pipe.fit_translation(j3, j2, pairs, fill=False, **kw)["per_frame"]
    assert rows[:, 5].tolist() == want[:, 5].tolist() and rows[[3, 4, 6], 5].tolist() == [1, 2, 2] and rows[7, 4] == want[7, 4]
    assert np.array_equal(np.isnan(rows), np.isnan(want))
    live = ~np.isnan(want)
    assert np.array_equal(rows[live].view(np.int64), want[live].view(np.int64))       # the same roundings in the same order
    fails, worst = tc.compare({"per_frame": rows, "per_sequence": pipe.fit_translation(j3, j2, pairs, fill=False, **kw)["per_sequence"]}, j3, j2, pairs,
                              fill=False, **kw)
    print(shown(worst))
    assert fails == [], fails
    for c, got in zip(fills, filled):
        gap = int(c[6])
        line = np.linspace(np.array(c[:3]), np.array(c[3:6]), gap + 2)[1:-1]
        assert np.array_equal(got.view(np.int64), line.view(np.int64)), c


def test_header_has_no_include():
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "translation3.h")).read()
    assert not [ln for ln in src.splitlines() if ln.lstrip().startswith("#include")]
    assert "#if defined(__HIPCC__)" in src
