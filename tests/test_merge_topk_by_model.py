"""CPU: the numpy model of the cosine rank (tests/merge_topk_by_helpers.py) on a row worked by hand.

Row 1 has the head pair (0, 16), so sqrt(total) = 4, and six pairs.  The totals of the columns: 2 -> 4, 3 -> 4, 4 -> 16, 5 -> 1,
6 -> 64; column 9 has no row (its total counts as 1).
    y = 2, v = 2:  den = 4 * 2 = 8    score 0.25
    y = 3, v = 2:  den = 4 * 2 = 8    score 0.25      (equal to column 2's: the lower column ranks first)
    y = 4, v = 8:  den = 4 * 4 = 16   score 0.5
    y = 5, v = 5:  den = 4 * 1 = 4    v > den: score 0
    y = 6, v = 4:  den = 4 * 8 = 32   score 0.125
    y = 9, v = 3:  den = 4 * 1 = 4    score 0.75
Best first: 9, 4, 2, 3, 6, 5.  By VALUE the order would be 4, 5, 6, 9, 2, 3."""
import numpy as np

from tests.merge_topk_by_helpers import scores_of, topk_cosine, totals_of

X = np.array([1, 1, 1, 1, 1, 1, 1, 2, 3, 4, 5, 6, 6], np.uint32)
Y = np.array([5, 0, 3, 9, 2, 6, 4, 0, 0, 0, 0, 0, 1], np.uint32)
V = np.array([5, 16, 2, 3, 2, 4, 8, 4, 4, 16, 1, 64, 7], np.uint32)
CAND = (X, Y, V)


def kept_columns(m, min_value=1):
    (x, y, v), dropped = topk_cosine(CAND, m, min_value)
    assert x.size + dropped == X.size
    return sorted(y[(x == 1) & (y != 0)].tolist()), (x, y, v)


def test_totals():
    assert totals_of(CAND, [1, 2, 3, 4, 5, 6, 9, 0]).tolist() == [16, 4, 4, 16, 1, 64, 0, 0]


def test_scores_of_the_hand_worked_row():
    s = scores_of(CAND)
    assert dict(zip(Y[:7].tolist(), s[:7].tolist())) == {5: 0.0, 0: s[1], 3: 0.25, 9: 0.75, 2: 0.25, 6: 0.125, 4: 0.5}
    assert s[12] == 7 / 32                                                # row 6: sqrt(64) * sqrt(16), column 1's total


def test_the_cut_falls_between_two_equal_scores():
    assert kept_columns(3)[0] == [2, 4, 9]                                # 0.75, 0.5 and the LOWER column of the two 0.25
    assert kept_columns(4)[0] == [2, 3, 4, 9]
    assert kept_columns(2)[0] == [4, 9]
    assert kept_columns(5)[0] == [2, 3, 4, 6, 9]                          # the v > den pair ranks last
    assert kept_columns(6)[0] == kept_columns(100)[0] == [2, 3, 4, 5, 6, 9]


def test_the_head_pair_is_kept_beside_the_m_and_the_raw_values_are_applied():
    cols, (x, y, v) = kept_columns(1)
    assert cols == [9]
    row = (x == 1)
    assert dict(zip(y[row].tolist(), v[row].tolist())) == {0: 16, 9: 3}
    assert dict(zip(y[x == 6].tolist(), v[x == 6].tolist())) == {0: 64, 1: 7}


def test_min_value_filters_before_the_rank():
    assert kept_columns(2, min_value=4)[0] == [4, 6]                      # eligible: 5 (score 0), 6 (0.125), 4 (0.5)
    cols, (x, y, v) = kept_columns(2, min_value=17)
    assert cols == [] and x.tolist() == [6]                               # only (6, 0, 64) is left
