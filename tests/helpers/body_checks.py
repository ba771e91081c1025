"""Mesh volume, centre of mass and second moments: the cases, and the rule the tests hold pipeline.mesh_moments and the device to.

The cases are closed, consistently oriented tables over a subset of the 6890 vertices: a tetrahedron, a box, and torus grids of 2 nu nv faces whose
counts sit on either side of the first column seam (1022, 1024, 1026), at SMPL's own count (13 776) and at the synthetic table's (13 780).  The
vertices the table names lie on the solid; every other vertex is noise, so a kernel that reads one shows.

The rule (compare): rows and sums must equal, in every bit, a restatement in plain Python floats -- one face after the other, one column after the
other, the tree as DESIGN 4.25 rule 3 writes it.  loops_moments takes a `fault`: the same restatement with one thing wrong, as a wrong kernel or a
wrong statement would leave it; tests/test_body_checks_cpu.py shows that compare catches each."""
import math
from fractions import Fraction

import numpy as np

from . import gait_checks as gc

V = 6890
NCOL = 1024
U = 2.0 ** -53
PERM = np.random.default_rng(25).permutation(V)              # which vertices a small table names: not the first ones, not in order
SECOND = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
# profiles/mesh_moments_bounds.txt: measure_exact's worst ratios (volume, centre, moments) over the tetrahedron and the boxes, rounded up in the
# second place; the tests assert twice these
MEASURED = {"volume": 0.51, "com": 0.59, "second": 1.2}
FAULTS = ("origin", "no_ss", "div24", "skip_tail", "sequential", "twice", "area1", "uncentred")


def same_bits(a, b):
    return gc.same_bits(a, b)


# ----------------------------------------------------------------------------- tables
def grid_faces(nu, nv, index=None):
    """synth.make_faces' torus over the vertices index[i * nv + j] (default: PERM's first nu nv): 2 nu nv faces, closed and oriented."""
    index = PERM[:nu * nv] if index is None else np.asarray(index)
    idx = index.reshape(nu, nv)
    a, b = idx, np.roll(idx, -1, 0)
    c, d = np.roll(b, -1, 1), np.roll(idx, -1, 1)
    return np.ascontiguousarray(np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)]).astype(np.int32))


def torus_points(nu, nv, R=0.6, r=0.2):
    """Node (i, j) on a torus of radii R and r, the way round that gives grid_faces a positive volume: (nu nv, 3) float64."""
    th, ph = np.meshgrid(2.0 * np.pi * np.arange(nu) / nu, 2.0 * np.pi * np.arange(nv) / nv, indexing="ij")
    return np.stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th), r * np.sin(ph)], -1).reshape(-1, 3)


TETRA_FACES = np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.int32)        # over corners 0, x, y, z: outward
TETRA_POINTS = np.array([(0.5, 0.25, 0.125), (1.5, 0.25, 0.125), (0.5, 2.25, 0.125), (0.5, 0.25, 3.125)])
# corner number = x + 2 y + 4 z
BOX_FACES = np.array([(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)], np.int32)


def box_points(size=(2.0, 3.0, 5.0), corner=(0.0, 0.0, 0.0)):
    return np.array([[corner[0] + size[0] * (k & 1), corner[1] + size[1] * ((k >> 1) & 1), corner[2] + size[2] * ((k >> 2) & 1)] for k in range(8)])


def over(faces, index):
    """A table over corners 0 .. K-1 moved to the vertices index[0 .. K-1]."""
    return np.ascontiguousarray(np.asarray(index)[np.asarray(faces)].astype(np.int32))


def frames_of(points, index, n=1, seed=0, move=True):
    """verts (n,6890,3) float32: the vertices `index` carry `points`, in frame k > 0 scaled, turned about z and shifted (a body that walks through the
    camera's space); every other vertex is noise of the same size."""
    rng = np.random.default_rng(seed)
    verts = rng.standard_normal((n, V, 3)).astype(np.float32)
    for k in range(n):
        p = np.asarray(points, np.float64)
        if move and k:
            ang, scale = 0.37 * k, 1.0 + 0.01 * k
            rot = np.array([[math.cos(ang), -math.sin(ang), 0.0], [math.sin(ang), math.cos(ang), 0.0], [0.0, 0.0, 1.0]])
            p = scale * p @ rot.T + np.array([0.3 * k, -0.1 * k, 2.0 + 0.05 * k])
        verts[k, np.asarray(index)] = p.astype(np.float32)
    return verts


def grid_case(nu, nv, n=1, seed=0):
    """(faces, verts) of a torus grid over PERM's first nu nv vertices."""
    index = PERM[:nu * nv]
    return grid_faces(nu, nv, index), frames_of(torus_points(nu, nv), index, n, seed)


GRIDS = {1022: (7, 73), 1024: (16, 32), 1026: (19, 27), 13776: (82, 84), 13780: (65, 106)}


def case(F, n=1, seed=0):
    """(faces, verts) of the case with F faces: 4 the tetrahedron, 12 the 2 x 3 x 5 box, else the torus grid GRIDS[F] (13 780: synth.make_faces' own table)."""
    if F == 4:
        return over(TETRA_FACES, PERM[:4]), frames_of(TETRA_POINTS, PERM[:4], n, seed)
    if F == 12:
        return over(BOX_FACES, PERM[:8]), frames_of(box_points(), PERM[:8], n, seed)
    nu, nv = GRIDS[F]
    if F == 13780:
        index = np.arange(V)
        return grid_faces(nu, nv, index), frames_of(torus_points(nu, nv), index, n, seed)
    return grid_case(nu, nv, n, seed)


def unreferenced(faces):
    """The vertices no face names."""
    return np.setdiff1d(np.arange(V), np.unique(faces))


# ----------------------------------------------------------------------------- the rule
def face_terms(a, b, c, fault=None):
    d = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0])
    s = [(a[k] + b[k]) + c[k] for k in range(3)]
    t = [d] + [d * s[k] for k in range(3)]
    for k, l in SECOND:
        inner = (a[k] * a[l] + b[k] * b[l]) + c[k] * c[l]
        t.append(d * inner if fault == "no_ss" else d * (inner + s[k] * s[l]))
    u, w = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
    nx, ny, nz = u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]
    q = (nx * nx + ny * ny) + nz * nz
    t.append(math.sqrt(q) if q >= 0 else math.nan)           # q is NaN or >= 0; math.sqrt refuses nothing else
    return t


def div(a, b):
    """a / b as IEEE does it where Python raises."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def loops_frame(v, faces, fault=None):
    """(row, sums) of ONE frame v (6890,3) float32 in plain Python floats, DESIGN 4.25 rules 1 to 4 as they are written."""
    o = [0.0, 0.0, 0.0] if fault == "origin" else [float(x) for x in v[faces[0][0]]]
    F = len(faces)
    col = [[0.0] * 11 for _ in range(NCOL)]
    last = (F // NCOL) * NCOL if fault == "skip_tail" else F
    for i in range(last):
        face = faces[i - 1] if fault == "twice" and i == 5 else faces[i]
        p = [[float(v[face[k]][x]) - o[x] for x in range(3)] for k in range(3)]
        t = face_terms(p[0], p[1], p[2], fault)
        acc = col[i % NCOL]
        for k in range(11):
            acc[k] = acc[k] + t[k]
    if fault == "sequential":
        S = [0.0] * 11
        for l in range(NCOL):
            for k in range(11):
                S[k] = S[k] + col[l][k]
    else:
        h = NCOL // 2
        while h >= 1:
            for l in range(h):
                for k in range(11):
                    col[l][k] = col[l][k] + col[l + h][k]
            h //= 2
        S = col[0]
    row = [math.nan] * 11
    row[0] = S[0] / 6.0
    row[10] = S[10] if fault == "area1" else S[10] / 2.0
    if S[0] > 0:
        m = [div(S[1 + k], (24.0 if fault == "div24" else 4.0) * S[0]) for k in range(3)]
        for k in range(3):
            row[1 + k] = o[k] + m[k]
        for q, (k, l) in enumerate(SECOND):
            E = div(S[4 + q], 20.0 * S[0])
            row[4 + q] = E if fault == "uncentred" else E - m[k] * m[l]
    return row, list(S)


def loops_moments(verts, faces, fault=None):
    """(rows (n,11), sums (n,11)) of every frame by loops_frame."""
    faces = [tuple(int(x) for x in f) for f in np.asarray(faces)]
    made = [loops_frame(np.asarray(v, np.float32), faces, fault) for v in verts]
    return np.array([m[0] for m in made], np.float64), np.array([m[1] for m in made], np.float64)


def fsum_ratio(terms, sums):
    """The worst |S_k - fsum(t_k)| over its bar (ceil(F / 1024) + 10) 2^-53 sum |t_k| over the frames and the eleven sums (terms (n,F,11): the
    statement's own, pipeline.mesh_face_terms): a term passes through ceil(F / 1024) additions in its column and 10 in the tree, plus one."""
    n, F, K = terms.shape
    steps = -(-F // NCOL) + 10
    worst = 0.0
    for f in range(n):
        for k in range(K):
            col = terms[f, :, k].tolist()
            bar = steps * U * math.fsum(abs(x) for x in col)
            miss = abs(sums[f, k] - math.fsum(col))
            worst = max(worst, miss / bar if bar > 0 else (0.0 if miss == 0 else math.inf))
    return worst


def compare(rows, sums, verts, faces, terms=None):
    """AssertionError unless rows and sums (either may be None) equal loops_moments' in every bit and, with the statement's `terms`, the sums lie
    within the derived bar of math.fsum.  Returns the worst fsum ratio (0.0 without terms)."""
    want_rows, want_sums = loops_moments(verts, faces)
    if sums is not None:
        assert same_bits(sums, want_sums), "sums differ"
    if rows is not None:
        assert same_bits(rows, want_rows), "rows differ"
    worst = fsum_ratio(terms, want_sums if sums is None else np.asarray(sums)) if terms is not None else 0.0
    assert worst <= 1.0, f"a sum is {worst:.3g} of its bar away from math.fsum"
    return worst


# ----------------------------------------------------------------------------- exact rational arithmetic
def exact_moments(points, faces):
    """(volume, centre (3), C (6), sum |d|, sum |d s_k| (3), sum |d (..)| (6)) of float32-exact points in fractions, about the first face's first corner."""
    P = [[Fraction(float(np.float32(x))) for x in p] for p in points]
    o = P[faces[0][0]]
    S = [Fraction(0)] * 10
    A = [Fraction(0)] * 10
    for f in faces:
        a, b, c = ([P[i][x] - o[x] for x in range(3)] for i in f)
        d = a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0])
        s = [a[k] + b[k] + c[k] for k in range(3)]
        t = [d] + [d * s[k] for k in range(3)] + [d * (a[k] * a[l] + b[k] * b[l] + c[k] * c[l] + s[k] * s[l]) for k, l in SECOND]
        S = [x + y for x, y in zip(S, t)]
        A = [x + abs(y) for x, y in zip(A, t)]
    m = [S[1 + k] / (4 * S[0]) for k in range(3)]
    C = [S[4 + q] / (20 * S[0]) - m[k] * m[l] for q, (k, l) in enumerate(SECOND)]
    return S[0] / 6, [o[k] + m[k] for k in range(3)], C, m, A, S[0]


def exact_ratios(row, points, faces):
    """{'volume', 'com', 'second'}: the worst error of a statement's row against exact_moments, in roundings (2^-53) of the quantity's own scale: the
    sum of the absolute terms behind it over its divisor, plus for the centre |o_k + m_k| and for a moment |m_k m_l| + |C_kl|."""
    vol, com, C, m, A, S0 = exact_moments(points, faces)
    out = {"volume": float(abs(Fraction(row[0]) - vol) / (Fraction(U) * A[0] / 6))}
    out["com"] = max(float(abs(Fraction(row[1 + k]) - com[k]) / (Fraction(U) * (A[1 + k] / (4 * S0) + abs(com[k])))) for k in range(3))
    out["second"] = max(float(abs(Fraction(row[4 + q]) - C[q]) / (Fraction(U) * (A[4 + q] / (20 * S0) + abs(m[k] * m[l]) + abs(C[q])))) for q, (k, l) in enumerate(SECOND))
    return out


EXACT_CASES = (("tetrahedron", TETRA_POINTS, TETRA_FACES), ("box 2x3x5", box_points(), BOX_FACES),
               ("box off the origin", box_points((0.75, 1.5, 0.3125), (64.25, -31.5, 16.125)), BOX_FACES),
               ("thin box", box_points((1.0 / 1024, 2.0, 0.5), (-0.5, 1.0, 3.0)), BOX_FACES),
               ("tetrahedron far away", TETRA_POINTS * 0.3 + np.array([100.0, -50.0, 25.0]), TETRA_FACES),
               ("tetrahedron of random corners", TETRA_POINTS + 0.2 * np.random.default_rng(4).standard_normal((4, 3)), TETRA_FACES),
               ("box of random sides", box_points(tuple(np.random.default_rng(5).uniform(0.2, 1.8, 3)), tuple(np.random.default_rng(6).uniform(-3.0, 3.0, 3))), BOX_FACES))


def measure_exact(mesh_moments):
    """[(name, ratios)] of EXACT_CASES with the statement `mesh_moments`; the points are rounded to float32 first, which both sides then read."""
    made = []
    for name, points, faces in EXACT_CASES:
        p32 = np.asarray(points, np.float32)
        index = PERM[:len(p32)]
        row = mesh_moments(frames_of(p32, index, 1, move=False), over(faces, index))[0]
        made.append((name, exact_ratios(row, p32, faces)))
    return made


# ----------------------------------------------------------------------------- the stand-alone checker's files and lines
OPEN_TEXT = "the face table is not a closed, consistently oriented surface: {} directed edges are duplicated or lack their reverse edge"
INDEX_TEXT = "face {} names vertex {}, outside [0, {})"
EMPTY_TEXT = "n_faces {} < 1"


def write_case(path, faces, verts=None, want=None, n_verts=V):
    """The file tests/helpers/gait_body_check.cpp reads, little-endian: int32 [n, V, F] (n = 0: the table alone is judged), int32 faces[F 3], then
    float32 verts[n V 3] and the expected float64 rows[n 11] and sums[n 11]."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    n = 0 if verts is None else len(verts)
    with open(path, "wb") as f:
        f.write(np.array([n, n_verts, len(faces)], "<i4").tobytes())
        f.write(np.ascontiguousarray(faces, "<i4").tobytes())
        if n:
            f.write(np.ascontiguousarray(verts, "<f4").tobytes())
            f.write(np.ascontiguousarray(want[0], "<f8").tobytes())
            f.write(np.ascontiguousarray(want[1], "<f8").tobytes())
    return path
