"""tests/helpers/body_checks.py is worth what it catches: faults planted into the rule's subject -- the restatement of DESIGN 4.25 with one thing wrong,
as a wrong kernel or a wrong statement would leave it -- must each fail the comparison, and the unspoilt statement must pass it."""
import numpy as np
import pytest

from .helpers import body_checks as bc


@pytest.fixture(scope="module")
def subject():
    """The 1026-face torus in two frames, the second scaled, turned and moved: the last column step is partial, every column is used."""
    return bc.case(1026, n=2, seed=7)


def test_the_unspoilt_statement_passes(pkg, subject):
    faces, verts = subject
    rows, sums = pkg.pipeline.mesh_moments(verts, faces, return_sums=True)
    bc.compare(rows, sums, verts, faces)
    assert (rows[:, 0] > 0.4).all()


@pytest.mark.parametrize("fault", bc.FAULTS)
def test_a_planted_fault_is_caught(subject, fault):
    faces, verts = subject
    rows, sums = bc.loops_moments(verts, faces, fault)
    good = bc.loops_moments(verts, faces)
    changed = int(np.count_nonzero(~((rows == good[0]) | (np.isnan(rows) & np.isnan(good[0])))))
    print(f"{fault}: {changed} of {rows.size} row values differ")
    with pytest.raises(AssertionError):
        bc.compare(rows, sums, verts, faces)
    with pytest.raises(AssertionError):
        bc.compare(rows, None, verts, faces)                   # the rows alone give every fault away


def test_the_fsum_bar_catches_a_lost_term(pkg, subject):
    """A sum with one face's term missing lies outside the derived bar around math.fsum."""
    faces, verts = subject
    pipe = pkg.pipeline
    f, v = faces.astype(np.int64), verts.astype(np.float64)
    o = v[:, f[0, 0]][:, None, :]
    terms = pipe.mesh_face_terms(v[:, f[:, 0]] - o, v[:, f[:, 1]] - o, v[:, f[:, 2]] - o)
    sums = pipe.mesh_moments(verts, faces, return_sums=True)[1]
    assert bc.fsum_ratio(terms, sums) <= 1.0
    lost = sums.copy()
    lost[1, 10] -= terms[1, 40, 10]
    assert bc.fsum_ratio(terms, lost) > 1.0
