"""CPU, no library: the numpy model of the similarity measures (tests/cf_sim_helpers.py) against the cosine model it extends,
against answers worked out by hand, and -- the contraction trap -- on the very data tests/test_gpu_cf_sim.py runs the kernels on:
that data holds pairs whose score changes when base + shrink is made with ONE fused multiply-add instead of a product rounded on
its own and an add, for COSINE at shrink 0.1 and for LIFT at shrink 0.5, so a kernel that contracts cannot pass there."""
from fractions import Fraction

import numpy as np
import pytest

from tests import cf_sim_helpers as H
from tests.merge_topk_by_helpers import scores_of, topk_cosine, totals_of


def random_candidates(seed):
    """400 rows over 300 columns, values 1..5 and a few too large for their totals; most ids have a head total, some have none"""
    rng = np.random.default_rng(seed)
    n = 6000
    key = np.unique(rng.integers(1, 401, n).astype(np.uint64) << np.uint64(32) | rng.integers(1, 301, n).astype(np.uint64))
    x, y = (key >> np.uint64(32)).astype(np.uint32), (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    v = rng.integers(0, 6, x.size).astype(np.uint32)
    v[::97] = 100000
    heads = rng.permutation(np.arange(1, 401, dtype=np.uint32))[:330]
    return (np.concatenate([x, heads]), np.concatenate([y, np.zeros(heads.size, np.uint32)]),
            np.concatenate([v, rng.integers(1, 60, heads.size).astype(np.uint32)]))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cosine_without_shrinkage_is_the_cosine_model_bit_for_bit(seed):
    cand = random_candidates(seed)
    assert H.scores_sim(cand, H.SIM_COSINE, 0.0).tobytes() == scores_of(cand).tobytes()
    assert H.scores_sim(cand, H.SIM_COSINE, -0.0).tobytes() == scores_of(cand).tobytes()
    for m, min_value in ((1, 1), (5, 0), (1000, 1)):
        (a, d), (b, e) = H.topk_sim(cand, H.SIM_COSINE, 0.0, m, min_value), topk_cosine(cand, m, min_value)
        assert d == e and all(u.tobytes() == w.tobytes() for u, w in zip(a, b))


# (ta, tb, cc, sim, shrink) -> the score, each worked out by hand from include/smatrix_batch.h
KNOWN = [
    (10, 6, 4, H.SIM_JACCARD, 0.0, 4 / 12),                     # 4 / (10 + 6 - 4)
    (10, 6, 4, H.SIM_JACCARD, 4.0, 4 / 16),
    (10, 6, 4, H.SIM_LIFT, 0.0, 4 / 60),
    (10, 6, 4, H.SIM_LIFT, 20.0, 4 / 80),
    (16, 4, 2, H.SIM_COSINE, 0.0, 2 / 8),
    (16, 4, 2, H.SIM_COSINE, 8.0, 2 / 16),
    (1, 1, 1, H.SIM_COSINE, 0.0, 1.0),                          # the pair shrinkage is for: seen once between two items seen once
    (1, 1, 1, H.SIM_COSINE, 10.0, 1 / 11),
    (1, 1, 1, H.SIM_JACCARD, 0.0, 1.0),
    (0, 6, 4, H.SIM_JACCARD, 0.0, 0.0),                         # ta == 0: 0 under every measure, whatever shrink makes of den
    (0, 6, 4, H.SIM_LIFT, 5.0, 0.0),
    (0, 6, 4, H.SIM_COSINE, 5.0, 0.0),
    (10, 0, 4, H.SIM_JACCARD, 0.0, 4 / 7),                      # tb == 0 counts as 1: 4 / (10 + 1 - 4)
    (10, 0, 4, H.SIM_LIFT, 0.0, 4 / 10),
    (9, 0, 2, H.SIM_COSINE, 1.0, 2 / 4),
    (2, 3, 7, H.SIM_LIFT, 0.0, 0.0),                            # cc > den: 7 > 6
    (2, 3, 7, H.SIM_LIFT, 1.0, 1.0),                            # ... and 7 / 7 once shrink lifts den to cc
    (2, 3, 3, H.SIM_JACCARD, 0.0, 0.0),                         # cc > den: 3 > 2 + 3 - 3
    (2, 3, 9, H.SIM_JACCARD, 0.0, 0.0),                         # a negative base: 2 + 3 - 9 = -4
    (2, 3, 9, H.SIM_JACCARD, 3.0, 0.0),                         # ... still negative with shrink: den = -1
    (2, 3, 9, H.SIM_JACCARD, 13.0, 1.0),                        # ... 9 / (-4 + 13)
    (2, 3, 5, H.SIM_JACCARD, 0.0, 0.0),                         # den == 0
    (2, 3, 0, H.SIM_JACCARD, 0.0, 0.0),                         # a dead cell
    (3, 7, 2, H.SIM_LIFT, 0.1, 2 / (21 + 0.1)),
]


@pytest.mark.parametrize("ta,tb,cc,sim,shrink,want", KNOWN)
def test_known_answers(ta, tb, cc, sim, shrink, want):
    got = H.score([ta], [tb], [cc], sim, shrink)
    assert got.dtype == np.float64 and got[0] == want, (got[0], want)
    assert 0.0 <= got[0] <= 1.0


def test_the_fused_denominator_is_the_other_one():
    """fused_den rounds once: (1 + 2^-52)^2 + 2^-53 is a tie that falls to even in two steps, and lies above the tie fused"""
    x = y = 1.0 + 2.0 ** -52
    h = 2.0 ** -53
    assert x * y + h == 1.0 + 2.0 ** -51 and H.fused_den(x, y, h) == 1.0 + 2.0 ** -51 + 2.0 ** -52
    assert H.fused_den(4.0, 0.25, 1.0) == 2.0


def test_topk_keeps_the_best_scores_and_breaks_ties_by_column():
    #        row 1: total 100;  columns 2, 3, 4 with totals 4, 9, 16, value 5 each;  column 5 without a total, value 1
    x = np.array([1, 1, 1, 1, 1, 2, 3, 4], np.uint32)
    y = np.array([0, 2, 3, 4, 5, 0, 0, 0], np.uint32)
    v = np.array([100, 5, 5, 5, 1, 4, 9, 16], np.uint32)
    cand = (x, y, v)
    (kx, ky, kv), dropped = H.topk_sim(cand, H.SIM_LIFT, 0.0, 2, 1)      # 5/400, 5/900, 5/1600, 1/100
    assert sorted(ky[kx == 1].tolist()) == [0, 2, 5] and dropped == 2
    (kx, ky, kv), dropped = H.topk_sim(cand, H.SIM_JACCARD, 0.0, 2, 1)   # 5/99, 5/104, 5/111, 1/100
    assert sorted(ky[kx == 1].tolist()) == [0, 2, 3]
    (kx, ky, kv), dropped = H.topk_sim(cand, H.SIM_LIFT, 1e9, 2, 1)      # shrink drowns the totals: all but column 5 tie nearly -- by value
    assert sorted(ky[kx == 1].tolist()) == [0, 2, 3]


def test_the_session_model_sums_left_to_right():
    ops = (np.array([1, 1, 2, 2, 3], np.uint32), np.array([0, 3, 0, 3, 0], np.uint32), np.array([10, 4, 6, 3, 5], np.uint32))
    model = H.SessionModel(H.sorted_export_of(ops))
    ids, sc = model.session([2, 1, 2], 5, H.SIM_LIFT, 0.0, w=[0.5, 2.0, 9.0])
    assert ids == [3] and sc[0] == 0.0 + 0.5 * (3 / 30) + 2.0 * (4 / 50)
    assert model.session([2, 1], 5, H.SIM_LIFT, 0.0, excl=[3])[0] == [] and model.session([2, 1], 5, H.SIM_LIFT, 0.0, deny=[3])[0] == []


# ---- the contraction trap, on the GPU tests' data -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    cand = H.world_contents()
    key = cand[0].astype(np.uint64) << np.uint64(32) | cand[1]
    assert np.unique(key).size == key.size                                # every (x, y) once: the contents are the ops
    return cand


@pytest.mark.parametrize("sim,shrink,rows", [(H.SIM_COSINE, 0.1, (11, 12, 13, 300)), (H.SIM_LIFT, 0.5, (17, 60001))])
def test_the_gpu_tests_data_tells_a_fused_denominator_from_the_two_step_one(world, sim, shrink, rows):
    x, y, v = world
    s = H.scores_sim(world, sim, shrink)
    live = np.flatnonzero((y != 0) & (s > 0) & np.isin(x, rows))
    differs = H.contraction_differs(totals_of(world, x[live]), totals_of(world, y[live]), v[live], sim, shrink)
    print("sim %d shrink %g: %d of %d scored pairs of rows %s change under contraction" % (sim, shrink, differs.sum(), live.size, rows))
    for r in rows:                                                        # in every one of these rows, which the GPU tests read
        assert differs[x[live] == r].any(), r


def test_the_world_has_the_shapes_the_gpu_tests_need(world):
    x, y, v = world
    pairs = lambda r: int(np.count_nonzero((x == r) & (y != 0)))          # noqa: E731
    assert pairs(10) <= H.M < pairs(11) <= 32 and 64 < pairs(12) <= 256 and pairs(13) > 4096
    assert totals_of(world, [H.NO_HEAD_ROW, H.NO_HEAD_ITEM, H.ABSENT, H.NO_ROW_COLUMN]).tolist() == [0, 0, 0, 0]
    assert np.count_nonzero((x == 15) & (v == 0)) == H.DEAD
    s = H.scores_sim(world, H.SIM_JACCARD, 10.0)
    assert np.unique(s[(x == 14) & (y != 0)]).size == 1 and s[(x == 14) & (y != 0)][0] > 0      # row 14: every score ties
    assert all(2 ** 26 <= t < 2 ** 28 for t in H.BIG_TOTALS.values())
