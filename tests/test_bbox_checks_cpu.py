"""The float64 checker of the box tests (tests/helpers/bbox_checks.py) on cases worked out by hand."""
import numpy as np

from .helpers import bbox_checks as bc


def test_row_cost_and_medoid_on_a_line():
    p = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [7, 0, 0]], np.float32)
    assert [bc.row_cost(p, i) for i in range(4)] == [11.0, 9.0, 9.0, 17.0]
    assert np.array_equal(bc.row_costs(p), [11.0, 9.0, 9.0, 17.0])
    assert np.array_equal(bc.row_costs(p, block=3), bc.row_costs(p))          # a block boundary changes nothing
    assert bc.medoid(p) == 1                                                   # rows 1 and 2 tie: the lower index
    assert bc.gap(p) == 0.0                                                    # row 2 has another x and the same cost


def test_the_score_is_a_coordinate_and_the_pad_is_not():
    p = np.array([[0, 0, 0, 9], [0, 0, 2, 9], [3, 4, 0, -9]], np.float32)
    assert bc.row_cost(p, 0) == 2.0 + 5.0
    assert bc.row_cost(p, 1) == 2.0 + np.sqrt(29.0)


def test_gap_skips_copies_of_the_medoid():
    # rows 0 and 1 are one point (a replaced joint): they tie exactly and give one centre; the gap is to the best OTHER (x, y)
    p = np.array([[1, 0, 0.5], [1, 0, 0.5], [0, 0, 0.5], [4, 0, 0.5]], np.float32)
    c = bc.row_costs(p)
    assert np.array_equal(c, [4.0, 4.0, 6.0, 10.0]) and bc.medoid(p, c) == 0
    assert bc.gap(p, c) == 0.5
    assert bc.gap(np.repeat(p[:1], 5, axis=0)) == float("inf")                 # nothing but copies


def test_prepare_applies_the_frame_rule():
    kp = np.zeros((2, 4, 3))
    kp[0] = [[10, 100, 0.05], [20, 200, 0.9], [30, 300, 0.9], [40, 50, 0.2]]  # joint 0 is below 0.1; joints 1 and 2 tie: the first
    kp[1] = [[1, 2, 0.01], [3, 4, 0.03], [5, 6, 0.02], [7, 8, 0.03]]          # every score below 0.1: all become joint 1
    pts, h = bc.prepare(kp)
    assert pts.dtype == np.float32 and pts.shape == (8, 3)
    assert np.array_equal(pts[0], np.float32([20, 200, 0.9])) and np.array_equal(pts[3], np.float32([40, 50, 0.2]))
    assert np.array_equal(pts[4:], np.tile(np.float32([3, 4, 0.03]), (4, 1)))
    ul = 50.0 - (300.0 - 50.0) * 0.10
    assert np.array_equal(h, [300.0 - ul, 0.0])
    assert kp[0, 0, 0] == 10                                                   # the caller's array is left alone
