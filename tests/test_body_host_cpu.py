"""Mesh volume, centre of mass and second moments on the host: pipeline.mesh_moments, the numpy float64 statement, against the plain-loop
restatement of tests/helpers/body_checks.py and against csrc/mesh_moments.h, the arithmetic the kernel runs, through tests/helpers/gait_body_check.cpp:
a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on files this test writes.  All three agree IN
EVERY BIT on every case.  Then the yardsticks: math.fsum of the same terms within a derived bar, exact rational arithmetic on solids with float32-exact
corners, the 2 x 3 x 5 box, a translation, the NaN rules, the refusals, the closed-table rule and pipeline.body_rows.  Every figure is printed before it
is asserted."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import body_checks as bc

COUNTS = (4, 12, 1022, 1024, 1026, 13776, 13780)


@pytest.fixture(scope="module")
def pipe(pkg):
    return pkg.pipeline


@pytest.fixture(scope="module")
def made(pipe):
    """{F: (faces, verts of 2 frames, rows, sums)} of every case, computed once."""
    out = {}
    for F in COUNTS:
        faces, verts = bc.case(F, n=2, seed=F)
        out[F] = (faces, verts) + pipe.mesh_moments(verts, faces, return_sums=True)
    return out


def test_statement_equals_the_loops_and_fsum(pipe, made):
    """The derived bar: a term passes through ceil(F / 1024) additions in its column and 10 in the tree; one more for the yardstick's own rounding."""
    for F, (faces, verts, rows, sums) in made.items():
        f = faces.astype(np.int64)
        v = verts.astype(np.float64)
        o = v[:, f[0, 0]][:, None, :]
        terms = pipe.mesh_face_terms(v[:, f[:, 0]] - o, v[:, f[:, 1]] - o, v[:, f[:, 2]] - o)
        worst = bc.compare(rows, sums, verts, faces, terms)
        print(f"{F} faces: volume {rows[:, 0].tolist()}, equal bits; worst |S - fsum| is {worst * (-(-F // 1024) + 10):.2f} roundings of sum |t| "
              f"(bar {-(-F // 1024) + 10})")
        assert rows.shape == (2, 11) and sums.shape == (2, 11) and (rows[:, 0] > 0).all() and np.isfinite(rows).all()
    assert pipe.MESH_MOMENT_COLUMNS == ("volume", "com_x", "com_y", "com_z", "c_xx", "c_yy", "c_zz", "c_xy", "c_xz", "c_yz", "area")
    torus = made[13780][2][0]
    print(f"the torus over synth.make_faces(): volume {torus[0]:.4f} (2 pi^2 R r^2 = {2 * math.pi ** 2 * 0.6 * 0.04:.4f}), area {torus[10]:.4f}")
    assert abs(torus[0] - 0.4727) < 5e-5


def test_exact_rational_yardstick(pipe):
    """Volume, centre and moments of solids with float32-exact corners against fractions: the error in roundings of each quantity's own scale (the sum
    of the absolute terms behind it over its divisor, plus the magnitudes of what is added to it).  The bar is twice what was measured when the
    statement was written (profiles/mesh_moments_bounds.txt): the cases are a handful."""
    worst = {}
    for name, ratios in bc.measure_exact(pipe.mesh_moments):
        print(f"{name}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst: " + ", ".join(f"{k} {v:.3g} (measured {bc.MEASURED[k]}, bar {2 * bc.MEASURED[k]})" for k, v in worst.items()))
    assert all(worst[k] <= 2 * bc.MEASURED[k] for k in worst)


def test_the_box(pipe):
    """2 x 3 x 5 with a corner at the origin: every term is an integer, so the sums are exact; volume 30, the centre (1, 1.5, 2.5), C_yy = 9/12 and
    the three products of inertia 0 are exact; C_xx = fl(4/3) - 1 and C_zz = fl(25/3) - 6.25 carry the one rounding of E_kk, which is not a double."""
    faces, verts = bc.case(12)
    rows, sums = pipe.mesh_moments(verts, faces, return_sums=True)
    exact = bc.exact_moments(bc.box_points(), bc.BOX_FACES)
    print(rows[0].tolist(), sums[0].tolist())
    assert sums[0, 0] == 180.0 and Fraction(float(rows[0, 0])) == exact[0] == 30
    assert rows[0, 1:4].tolist() == [1.0, 1.5, 2.5] and rows[0, 5] == 0.75 and rows[0, 7:10].tolist() == [0.0, 0.0, 0.0] and rows[0, 10] == 62.0
    for col, side in ((4, 2.0), (6, 5.0)):
        assert abs(Fraction(float(rows[0, col])) - Fraction(side) ** 2 / 12) <= Fraction(bc.U) * Fraction(side) ** 2 / 3, col


def test_translation(pipe):
    """Vertices on a 2^-10 grid below 4 m, shifted by (64, -32, 16): every coordinate stays a float32, every corner relative to the origin is the same
    number, so volume, C and area keep every bit; the centre moves by the shift to within one rounding (2^-52) of the larger magnitude -- each of the two
    sums o + m rounds once, by half a unit in its last place."""
    nu, nv = bc.GRIDS[1026]
    index = bc.PERM[:nu * nv]
    faces = bc.grid_faces(nu, nv, index)
    points = np.round((bc.torus_points(nu, nv) + np.array([1.0, 1.5, 2.0])) * 1024.0) / 1024.0
    shift = np.array([64.0, -32.0, 16.0])
    here, there = bc.frames_of(points, index, 1, move=False), bc.frames_of(points + shift, index, 1, move=False)
    assert np.abs(points).max() < 4 and (there[0, index].astype(np.float64) == points + shift).all()
    a, b = pipe.mesh_moments(here, faces)[0], pipe.mesh_moments(there, faces)[0]
    print(a.tolist(), b.tolist())
    keep = [0, 4, 5, 6, 7, 8, 9, 10]
    assert bc.same_bits(a[keep], b[keep]) and a[0] > 0.4
    moved = np.abs(b[1:4] - (a[1:4] + shift))
    bar = 2.0 ** -52 * np.maximum(np.abs(a[1:4]), np.abs(b[1:4]))
    print(f"the centre moved by the shift to within {moved.tolist()} (bars {bar.tolist()})")
    assert (moved <= bar).all()
    # what forgetting rule 1 would do: the loops with the origin left in differ
    assert not bc.same_bits(bc.loops_moments(there, faces, "origin")[0][0][keep], b[keep])


def test_nan_rules(pipe, made):
    faces, verts, rows, sums = made[1026]
    three = np.concatenate([verts, verts[:1]])
    base = pipe.mesh_moments(three, faces, return_sums=True)
    spare = bc.unreferenced(faces)
    assert len(spare) == bc.V - 19 * 27
    dirty = three.copy()
    dirty[:, spare[::7]] = np.nan
    dirty[1, spare[3]] = np.inf
    got = pipe.mesh_moments(dirty, faces, return_sums=True)
    assert bc.same_bits(got[0], base[0]) and bc.same_bits(got[1], base[1])            # an unreferenced vertex changes no bit
    dirty = three.copy()
    dirty[1, faces[700, 1], 2] = np.nan
    got = pipe.mesh_moments(dirty, faces, return_sums=True)
    assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all()                    # a referenced one: the frame's row is NaN, by arithmetic alone
    assert bc.same_bits(got[0][[0, 2]], base[0][[0, 2]]) and bc.same_bits(got[1][[0, 2]], base[1][[0, 2]])
    flipped = pipe.mesh_moments(verts, faces[:, ::-1], return_sums=True)
    print(flipped[0][0].tolist())
    assert (flipped[0][:, 0] < 0).all() and np.isnan(flipped[0][:, 1:10]).all() and bc.same_bits(flipped[0][:, 10], rows[:, 10])


def test_closed_table_rule_and_refusals(pipe, pkg):
    for F in COUNTS:
        assert pipe.faces_closed(bc.case(F)[0]) == 0
    assert pipe.faces_closed(pkg.synth.make_faces()) == 0
    faces = bc.case(1026)[0]
    assert pipe.faces_closed(faces[:-1]) == 3                                          # one face removed: its three neighbours' edges lack their reverse
    assert pipe.faces_closed(np.concatenate([faces, faces[5:6]])) == 6                 # one face twice: both copies of its three edges
    turned = faces.copy()
    turned[9] = turned[9, ::-1]
    assert pipe.faces_closed(turned) == 6                                              # one face turned over: its edges double its neighbours' and lack reverses
    pinched = faces.copy()
    pinched[4, 1] = pinched[4, 0]
    assert pipe.faces_closed(pinched) > 0                                              # an edge from a vertex to itself
    verts = bc.case(1026)[1]
    for bad, text in ((faces[:-1], bc.OPEN_TEXT.format(3)), (np.concatenate([faces, faces[5:6]]), bc.OPEN_TEXT.format(6))):
        with pytest.raises(ValueError) as e:
            pipe.mesh_moments(verts, bad)
        assert str(e.value) == text
    wrong = faces.copy()
    wrong[7, 2] = bc.V
    with pytest.raises(ValueError) as e:
        pipe.mesh_moments(verts, wrong)
    assert str(e.value) == bc.INDEX_TEXT.format(7, bc.V, bc.V)
    with pytest.raises(ValueError) as e:
        pipe.mesh_moments(verts, np.zeros((0, 3), np.int32))
    assert str(e.value) == bc.EMPTY_TEXT.format(0)
    for bad in (verts[0], verts[:, :, :2], np.zeros((0, bc.V, 3), np.float32)):
        with pytest.raises(ValueError):
            pipe.mesh_moments(bad, faces)


def test_header_on_the_host_under_sanitizers(pipe, made, tmp_path):
    """csrc/mesh_moments.h itself against the statement on every case, on the NaN cases and the flipped mesh; its refusals in the library's words."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_body_check.cpp")
    exe = str(tmp_path / "gait_body_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files, tables = [], {}
    for F, (faces, verts, rows, sums) in made.items():
        files.append(bc.write_case(str(tmp_path / f"case{F}.bin"), faces, verts, (rows, sums)))
    faces, verts, rows, sums = made[1026]
    dirty = verts.copy()
    dirty[:, bc.unreferenced(faces)[::5]] = np.nan
    dirty[1, faces[700, 1], 2] = np.nan
    files.append(bc.write_case(str(tmp_path / "nan.bin"), faces, dirty, pipe.mesh_moments(dirty, faces, return_sums=True)))
    files.append(bc.write_case(str(tmp_path / "flipped.bin"), faces[:, ::-1], verts, pipe.mesh_moments(verts, faces[:, ::-1], return_sums=True)))
    big = np.ldexp(verts.astype(np.float64), 20).astype(np.float32)
    files.append(bc.write_case(str(tmp_path / "big.bin"), faces, big, pipe.mesh_moments(big, faces, return_sums=True)))
    wrong = faces.copy()
    wrong[7, 2] = -1
    for name, table, text in (("open", faces[:-1], bc.OPEN_TEXT.format(3)), ("twice", np.concatenate([faces, faces[5:6]]), bc.OPEN_TEXT.format(6)),
                              ("index", wrong, bc.INDEX_TEXT.format(7, -1, bc.V)), ("empty", np.zeros((0, 3), np.int32), bc.EMPTY_TEXT.format(0))):
        files.append(bc.write_case(str(tmp_path / f"{name}.bin"), table))
        tables[files[-1]] = text
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)       # run as a program: nothing is preloaded
    print(run.stdout[-3000:], run.stderr[-3000:])
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok"
    said = dict(line[len("table "):].split(": ", 1) for line in run.stdout.splitlines() if line.startswith("table "))
    assert len(said) == len(files)
    for path in files:
        assert said[path] == tables.get(path, "closed"), path
    # a wrong expectation must fail the program: it compares, it does not merely run
    rows2 = rows.copy()
    rows2[1, 4] = np.nextafter(rows2[1, 4], 1.0)
    bad = bc.write_case(str(tmp_path / "spoilt.bin"), faces, verts, (rows2, sums))
    run = subprocess.run([exe, bad], capture_output=True, text=True, timeout=300)
    assert run.returncode == 1 and "rows[1][4]" in run.stdout


def test_body_rows(pipe):
    """pipeline.body_rows against the same sums written out here, on rows made by hand: two videos, one with frames that have no volume."""
    rng = np.random.default_rng(3)
    n = 9
    joints = rng.standard_normal((n, 25, 3)).astype(np.float32)
    rows = np.abs(rng.standard_normal((n, 11))) + 0.1
    rows[2, 1:10] = np.nan                                     # a frame whose mesh was inside out
    rows[2, 0] = -0.07
    rows[6:] = np.nan                                          # a video without a valid frame
    joints[4, 3] = np.nan                                      # a frame whose table COM is NaN: out of the offsets only
    out = pipe.body_rows(rows, joints, lengths=[6, 3], density=1000.0)
    assert out.shape == (2, 15) and len(pipe.BODY_COLUMNS) == 15
    table = pipe.balance_table_com(joints.astype(np.float64), pipe.BALANCE_SEGMENTS_KINECTV2)
    assert np.isnan(table[4]).any()
    valid = [0, 1, 3, 4, 5]
    vol = [rows[k, 0] for k in valid]
    mean = sum(vol, 0.0) / 5
    sd = math.sqrt(sum(((v - mean) ** 2 for v in vol), 0.0) / 5)
    want = [6.0, 5.0, mean, sd, sd / mean, 1000.0 * mean, sum((rows[k, 10] for k in valid), 0.0) / 5]
    want += [sum((math.sqrt(rows[k, 4 + a]) for k in valid), 0.0) / 5 for a in range(3)]
    both = [0, 1, 3, 5]
    d = [[rows[k, 1 + a] - table[k, a] for a in range(3)] for k in both]
    want += [sum((x[a] for x in d), 0.0) / 4 for a in range(3)]
    dist = [math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) for x in d]
    want += [sum(dist, 0.0) / 4, max(dist)]
    print(out[0].tolist())
    assert bc.same_bits(out[0], want)
    assert out[1, 0] == 3 and out[1, 1] == 0 and np.isnan(out[1, 2:]).all()
    assert pipe.BODY_COLUMNS[:6] == ("frames", "frames_valid", "volume_mean", "volume_sd", "volume_cv", "mass") and pipe.BODY_DENSITY == 985.0
    for bad in (dict(density=0.0), dict(density=np.nan), dict(lengths=[5, 3])):
        with pytest.raises(ValueError):
            pipe.body_rows(rows, joints, **{"lengths": [6, 3], **bad})
    with pytest.raises(ValueError):
        pipe.body_rows(rows[:, :10], joints)


def test_balance_with_a_given_com(pipe):
    """pipeline.gait_balance(com=...): with rule 1's own centre of mass every bit of the call without it; segments beside com is refused."""
    from .helpers import balance_checks as bal
    name, joints, par = bal.walker_cases(200)[0]
    events = pipe.gait_parameters(joints, fps=bal.FPS)["events"]
    plain = pipe.gait_balance(joints, events, fps=bal.FPS)
    com = pipe.balance_table_com(np.asarray(joints, np.float32).astype(np.float64))
    given = pipe.gait_balance(joints, events, fps=bal.FPS, com=com)
    assert plain["per_sequence"][0, 1] > 5
    for key in plain:
        assert bc.same_bits(plain[key], given[key]), key
    shifted = pipe.gait_balance(joints, events, fps=bal.FPS, com=com + np.array([0.0, 0.1, 0.0]))
    assert bc.same_bits(shifted["rel"][:, :3], com + np.array([0.0, 0.1, 0.0])) and not bc.same_bits(shifted["per_sequence"], plain["per_sequence"])
    with pytest.raises(ValueError):
        pipe.gait_balance(joints, events, fps=bal.FPS, com=com, segments=pipe.BALANCE_SEGMENTS_KINECTV2)
    with pytest.raises(ValueError):
        pipe.gait_balance(joints, events, fps=bal.FPS, com=com[:-1])
