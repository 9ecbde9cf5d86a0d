"""GPU (-m gpu): smatrix_merge_topk_by (include/smatrix_batch.h; SparseMatrix.merge_topk / truncated with rank="cosine").  Every
case runs next to oracle_mod.Oracle() through check() of tests/merge_helpers.py, as tests/test_gpu_merge_topk.py does.

Expected ops: the numpy model of tests/merge_topk_by_helpers.py on the source oracle's candidates -- per row the eligible pairs
(y != 0, v >= min_value) by (score bits descending, column ascending), the first m kept, and the head pair beside them; fed to the
destination's oracle one by one as op(x, y, v) with the raw v.  Case 1 ties the model's score to the library's own, bit for bit.

Compared after every call, all exactly: n_ops and n_dropped; the row set; get of every candidate cell; size and used of rows
without a column-0 pair; the probe invariant of rows with one."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix
from tests.merge_helpers import (DECR, GET, INCR, M_MAX, OPS, REGIMES, SET, assert_export_equal, both, check,  # noqa: F401
                                 check_rows_around_one_step, device, one_row, ops_of, row_dict, u32)
from tests.merge_topk_by_helpers import RANK_COSINE, RANK_VALUE, scores_of, topk_cosine

pytestmark = pytest.mark.gpu


def merged_cos(dst, o_dst, src, cand, op, m, min_value, max_batch=0, tag=""):
    """dst.merge_topk(src, rank="cosine") next to the oracle; checks the counts and the result; returns (kept ops, n_dropped)"""
    before = ops_of(o_dst)
    ops, dropped = topk_cosine(cand, m, min_value)
    n, d = dst.merge_topk(src, m, op, min_value, max_batch=max_batch, rank="cosine")
    o_dst.apply(OPS[op], *ops)
    print("%s: %d candidates, %d applied, %d dropped (library: %d, %d)" % (tag, cand[0].size, ops[0].size, dropped, n, d))
    assert (n, d) == (ops[0].size, dropped), (tag, (n, d), (ops[0].size, dropped))
    check(dst, o_dst, (before, cand), set(), tag)
    return ops, d


def set_totals(m, o, ids, totals):
    ids = np.asarray(ids, np.uint32)
    both(m, o, SET, ids, np.zeros(ids.size, np.uint32), np.asarray(totals, np.uint32))


def library_scores(src, cand):
    """{(x, y): score} of every non-empty cell, from src.cf_neighbors_batch"""
    rows, counts = np.unique(cand[0], return_counts=True)
    off, ids, sc, cnt = src.cf_neighbors_batch(rows, caps=counts.astype(np.uint64) + 1)
    assert (cnt == counts).all()
    at = np.concatenate([np.arange(int(off[i]), int(off[i]) + int(cnt[i])) for i in range(rows.size)])
    return np.repeat(rows, cnt), ids[at], sc[at]


def assert_model_scores_are_the_librarys(src, cand, tag=""):
    x, y, s = library_scores(src, cand)
    want = scores_of(cand)
    ours = dict(zip(zip(cand[0].tolist(), cand[1].tolist()), want.view(np.uint64).tolist()))
    theirs = dict(zip(zip(x.tolist(), y.tolist()), s.view(np.uint64).tolist()))
    assert ours.keys() == theirs.keys(), tag
    bad = [k for k in ours if k[1] != 0 and ours[k] != theirs[k]]
    assert not bad, (tag, len(bad), bad[:5])


# ---- cases 1 and 2: the model's scores, the regimes ------------------------------------------------------------------------
# The row shapes of tests/merge_helpers.REGIMES: 16, 512 and 8192 slots (the wave path; 16: the keys held in registers), 16384 and
# 32768 (one workgroup, one segment), 65536 and 131072 (cut rows of 2 and 4 segments).  The columns come from a pool of 42000 ids of
# which 32000 have a row with a head total in 1..50 and 10000 have none (their total counts as 1); values 1..5, so a row of
# thousands of pairs has 250 different scores at most: ties everywhere.  Rows 10 (short) and 14 (long) have no head pair.
HEADS = {11: 400, 12: 1000, 13: 90, 15: 2500, 16: 37}
POOL0, POOL, WITH_ROW = 100000, 42000, 32000


@pytest.fixture(scope="module")
def regimes(oracle_mod):
    rng = np.random.default_rng(99)
    m, o = SparseMatrix(), oracle_mod.Oracle()
    pool = (POOL0 + rng.permutation(POOL)).astype(np.uint32)
    set_totals(m, o, pool[:WITH_ROW], rng.integers(1, 51, WITH_ROW))
    for x, (n, size) in REGIMES.items():
        ys = rng.permutation(pool)[:n]
        vs = rng.integers(0 if x == 11 else 1, 6, n)
        vs[:: max(n // 5, 1)] = 100000                                    # a few pairs with v > den: score 0
        one_row(m, o, x, ys, vs)
        assert m.row_info(x) == o.row_info(x) and o.row_info(x)[0] == size, (x, m.row_info(x), o.row_info(x))
    set_totals(m, o, list(HEADS), list(HEADS.values()))
    xs = np.repeat(np.arange(1000, 1300, dtype=np.uint32), 12)            # and 300 short rows without a head pair
    both(m, o, INCR, xs, rng.integers(1, 1 << 32, xs.size, dtype=np.uint32), rng.integers(1, 4, xs.size, dtype=np.uint32))
    made = (m, o, ops_of(o), m.export("table"))
    yield made
    m.close(); o.close()


def test_the_models_scores_are_the_librarys(regimes):
    src, o_src, cand, table = regimes
    s = scores_of(cand)
    live = cand[1] != 0
    assert np.count_nonzero(s[live & (cand[2] == 100000)]) == 0 and np.count_nonzero(s[live]) > 50000
    assert_model_scores_are_the_librarys(src, cand, "regimes")


@pytest.mark.parametrize("m", [1, 7, 64, 5000])
def test_truncated_copy_of_every_regime(oracle_mod, regimes, m):
    src, o_src, cand, table = regimes
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    ops, dropped = merged_cos(dst, o_dst, src, cand, "set", m, 1, tag="regimes m %d" % m)
    for x, (n, size) in REGIMES.items():
        kept = int(np.count_nonzero((ops[0] == x) & (ops[1] != 0)))
        elig = int(np.count_nonzero((cand[0] == x) & (cand[1] != 0) & (cand[2] >= 1)))
        assert kept == min(m, elig), (x, kept, elig)
        assert len(row_dict(dst, x)) == kept + (x in HEADS)
    if m == 5000:                                                         # the cut rows really lose pairs, the short ones none
        assert np.count_nonzero((ops[0] == 15) & (ops[1] != 0)) == 5000 < 20000
        assert np.count_nonzero((ops[0] == 16) & (ops[1] != 0)) == 5000 < 40000
        assert np.count_nonzero(ops[0] == 12) == 3001
    for x, t in HEADS.items():
        assert dst.get(x, 0) == t
    for x in (10, 14):                                                    # no head pair: score 0 everywhere, the lowest columns
        ys = np.sort(cand[1][cand[0] == x])
        assert sorted(row_dict(dst, x)) == ys[:m].tolist()
    assert_export_equal(src.export("table"), table, "the source")
    dst.close(); o_dst.close()


def test_rows_around_one_step_of_a_wave(oracle_mod):
    check_rows_around_one_step(oracle_mod, merged_cos, column_totals=True)


# ---- case 3: the digit passes ------------------------------------------------------------------------------------------------
def test_rows_whose_scores_differ_in_one_place_only(oracle_mod):
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    j = np.arange(1, 201, dtype=np.uint64)
    # row 1: v = j against a total of 3 j^2 -- 1 / (sa * sqrt(3)) in exact arithmetic for every j, so the scores are that number
    # rounded differently: the last mantissa byte only
    set_totals(src, o_src, 10000 + j, 3 * j * j)
    one_row(src, o_src, 1, 10000 + j, j)
    # row 2: v = 1, sa = 2^15, totals 4^k: the scores are 2^-(15 + k), k = 0 .. 15: the exponent only
    set_totals(src, o_src, 20000 + j, np.uint64(4) ** (j % np.uint64(16)))
    one_row(src, o_src, 2, 20000 + j, np.ones(200))
    # row 3: one value, one total: all scores equal, the column decides; row 4: no head pair, all scores 0
    set_totals(src, o_src, 30000 + j, np.full(200, 9))
    one_row(src, o_src, 3, (30000 + j) * 1, np.full(200, 2))
    one_row(src, o_src, 4, np.arange(1, 201) * 977, np.arange(1, 201))
    set_totals(src, o_src, [1, 2, 3], [49, 1 << 30, 100])
    cand = ops_of(o_src)
    bits = scores_of(cand).view(np.uint64)
    row = lambda x: bits[(cand[0] == x) & (cand[1] != 0)]                 # noqa: E731
    assert np.unique(row(1) >> 8).size == 1 and np.unique(row(1)).size > 1
    assert np.unique(row(2)).size == 16 and not (row(2) & ((1 << 52) - 1)).any()
    assert np.unique(row(3)).size == 1 and row(3)[0] != 0 and not row(4).any()
    assert_model_scores_are_the_librarys(src, cand, "digits")
    for m in (1, 100, 150):
        dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
        merged_cos(dst, o_dst, src, cand, "set", m, 0, tag="digits m %d" % m)
        for x in (1, 2, 3, 4):
            assert len(row_dict(dst, x)) == m + (x != 4)
        assert sorted(row_dict(dst, 3))[1:] == (30000 + j[:m]).tolist()    # equal scores: the lowest columns
        assert sorted(row_dict(dst, 4)) == (np.arange(1, m + 1) * 977).tolist()
        got = np.array(sorted(k for k in row_dict(dst, 2) if k), np.uint64) - 20000
        assert (np.sort(got % 16)[:m] == np.sort(j % 16)[:m]).all()        # the smallest totals score best
        dst.close(); o_dst.close()
    src.close(); o_src.close()


# ---- case 4: the edges -------------------------------------------------------------------------------------------------------
def edge_source(oracle_mod):
    """row 1: a head pair of 900, 20 live pairs (columns 6 .. 25, scores y / 30) and 5 dead cells; row 2: dead cells only;
    row 3: a head pair of 1 and two pairs with v > den; row 4: a head pair of 1000 and three pairs; rows 100..: 9 pairs each"""
    src, o = SparseMatrix(), oracle_mod.Oracle()
    one_row(src, o, 1, np.arange(1, 26), np.arange(1, 26))
    both(src, o, DECR, np.full(5, 1, np.uint32), np.arange(1, 6, dtype=np.uint32), np.arange(1, 6, dtype=np.uint32))
    one_row(src, o, 2, np.arange(1, 8), np.full(7, 6))
    both(src, o, DECR, np.full(7, 2, np.uint32), np.arange(1, 8, dtype=np.uint32), np.full(7, 6, np.uint32))
    one_row(src, o, 3, [0, 5, 6], [1, 4, 4])
    one_row(src, o, 4, [0, 5, 6, 7], [1000, 2, 9, 9])
    set_totals(src, o, [1], [900])
    xs = np.repeat(np.arange(100, 150, dtype=np.uint32), 9)
    both(src, o, SET, xs, np.tile(np.arange(1, 10, dtype=np.uint32), 50), (xs % 5 + 1).astype(np.uint32))
    return src, o


@pytest.mark.parametrize("m", [19, 20, 21, M_MAX])
def test_m_around_the_eligible_count(oracle_mod, m):
    src, o_src = edge_source(oracle_mod)
    cand = ops_of(o_src)
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    merged_cos(dst, o_dst, src, cand, "set", m, 1, tag="edges m %d" % m)
    assert len(row_dict(dst, 1)) == min(m, 20) + 1
    if m == 19:
        assert 6 not in row_dict(dst, 1)                                  # 6 / 30: the lowest score of the 20
    assert dst.row_info(2) is None                                        # a row of dead cells only, min_value 1: not created
    if m == M_MAX:                                                        # == merge_scaled(1, 1, min_value)
        ref = SparseMatrix()
        assert ref.merge_scaled(src, "set", 1, 1, 1) == dst.merge_topk(src, m, "set", 1, rank="cosine")
        assert_export_equal(ref.export("sorted"), dst.export("sorted"), "against merge_scaled")
        ref.close()
    for h in (src, o_src, dst, o_dst):
        h.close()


def test_dead_cells_head_pairs_and_refusals(oracle_mod):
    src, o_src = edge_source(oracle_mod)
    cand = ops_of(o_src)
    for min_value in (0, 1):                                              # 25 cells, 20 live: m = 22 takes two dead cells with min_value 0
        dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
        merged_cos(dst, o_dst, src, cand, "set", 22, min_value, tag="dead cells, min_value %d" % min_value)
        assert len(row_dict(dst, 1)) == (22 if min_value == 0 else 20) + 1
        if min_value == 0:
            assert dst.row_info(2) == o_dst.row_info(2) == (16, 7)
            assert sorted(row_dict(dst, 1))[:3] == [0, 1, 2]               # a dead cell scores 0: those of the lowest columns
        else:
            assert dst.row_info(2) is None
        dst.close(); o_dst.close()
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    merged_cos(dst, o_dst, src, cand, "set", 1, 2, tag="head pairs")
    assert row_dict(dst, 3) == {5: 4}                                       # head pair 1 < min_value 2: dropped, and still the row's total
    assert row_dict(dst, 4) == {0: 1000, 6: 9}                              # head pair beside the ONE best pair (9 at the lower column)
    # refusals: -1 and nothing changed
    before = dst.export("table")
    n, d = C.c_uint64(77), C.c_uint64(78)
    call = dst._lib.smatrix_merge_topk_by
    assert call(dst._h, src._h, SET, 2, 5, 1, 0, C.byref(n), C.byref(d)) == -1             # unknown rank
    assert call(dst._h, src._h, SET, -1, 5, 1, 0, C.byref(n), C.byref(d)) == -1
    for rank in (RANK_VALUE, RANK_COSINE):
        assert call(dst._h, src._h, SET, rank, 0, 1, 0, C.byref(n), C.byref(d)) == -1      # m == 0
        assert call(dst._h, dst._h, SET, rank, 5, 1, 0, C.byref(n), C.byref(d)) == -1      # dst is src
        assert call(dst._h, src._h, GET, rank, 5, 1, 0, C.byref(n), C.byref(d)) == -1
        assert call(dst._h, src._h, 4, rank, 5, 1, 0, None, None) == -1
    assert (n.value, d.value) == (77, 78)
    with pytest.raises(ValueError):
        dst.merge_topk(dst, 5, rank="cosine")
    assert dst.export("table")[2].tobytes() == before[2].tobytes()
    assert_export_equal(dst.export("table"), before)
    assert call(dst._h, src._h, INCR, RANK_COSINE, 5, 1, 0, None, None) == 0              # (both counts may be NULL)
    for h in (src, o_src, dst, o_dst):
        h.close()


# ---- case 5: rank VALUE is smatrix_merge_topk --------------------------------------------------------------------------------
def test_rank_value_is_merge_topk(regimes):
    src, o_src, cand, table = regimes
    a, b = SparseMatrix(), SparseMatrix()
    n, d = C.c_uint64(0), C.c_uint64(0)
    assert a._lib.smatrix_merge_topk_by(a._h, src._h, SET, RANK_VALUE, 64, 1, 0, C.byref(n), C.byref(d)) == 0
    assert (n.value, d.value) == b.merge_topk(src, 64, "set", 1)
    ea, eb = a.export("sorted"), b.export("sorted")
    assert all(u.tobytes() == w.tobytes() for u, w in zip(ea, eb))
    a.close(); b.close()


# ---- case 6: batches and history ---------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_max_batch(oracle_mod):
    # (a source of its own: with max_batch 1 every surviving row is a batch, and the regimes' source has 32000 of them)
    rng = np.random.default_rng(7)
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    pool = (POOL0 + rng.permutation(4000)).astype(np.uint32)
    set_totals(src, o_src, pool[:3000], rng.integers(1, 51, 3000))
    for x, n in ((10, 7), (11, 200), (12, 3000)):                         # the wave path; row 10 has no head pair
        one_row(src, o_src, x, rng.permutation(pool)[:n], rng.integers(1, 6, n))
    far = (POOL0 + 4000 + rng.permutation(1 << 18)[:6000]).astype(np.uint32)
    one_row(src, o_src, 13, np.concatenate([pool, far]), rng.integers(1, 6, 10000))   # one workgroup: 32768 slots
    set_totals(src, o_src, [11, 12, 13], [400, 1000, 90])
    assert src.row_info(13)[0] == 32768
    cand = ops_of(o_src)
    exports, grew = [], []
    for mb in (1, 1000, 0):
        dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
        b0 = dst.stats()["batches"]
        ops, _ = merged_cos(dst, o_dst, src, cand, "set", 64, 1, max_batch=mb, tag="max_batch %d" % mb)
        grew.append(dst.stats()["batches"] - b0)
        exports.append(dst.export("sorted"))
        dst.close(); o_dst.close()
    rows_kept = np.unique(ops[0]).size
    print("internal batches:", grew)
    assert grew[0] == rows_kept and grew[2] == 1 and grew[0] > grew[1] > grew[2]      # 1: a batch per surviving row; 0: one
    assert_export_equal(exports[0], exports[1]); assert_export_equal(exports[0], exports[2])
    src.close(); o_src.close()


def test_the_kept_set_depends_on_the_contents_alone():
    rng = np.random.default_rng(17)
    n = 60000
    x = np.concatenate([rng.integers(0, 400, n, dtype=np.uint32), np.full(12000, 7, np.uint32), np.arange(400, dtype=np.uint32)])
    y = np.concatenate([rng.integers(1, 3000, n, dtype=np.uint32), (rng.permutation(1 << 18)[:12000] + 1).astype(np.uint32),
                        np.zeros(400, np.uint32)])
    v = np.concatenate([rng.integers(1, 4, n + 12000, dtype=np.uint32), rng.integers(100, 200, 400, dtype=np.uint32)])
    a, b = SparseMatrix(), SparseMatrix()
    p = rng.permutation(x.size)
    a.apply_batch(INCR, x[p], y[p], v[p], results=False)                   # one batch, shuffled
    b.apply_batch(INCR, x[:10], y[:10], v[:10], results=False)            # a tiny first batch, then growth in steps
    for s in range(10, x.size, 9000):
        b.apply_batch(INCR, x[s:s + 9000], y[s:s + 9000], v[s:s + 9000], results=False)
    assert_export_equal(a.export("sorted"), b.export("sorted"), "the sources")
    assert a.row_info(7)[0] > 8192
    for m in (5, 300):
        ta, tb = a.truncated(m, rank="cosine"), b.truncated(m, rank="cosine")
        ea, eb = ta.export("sorted"), tb.export("sorted")
        assert all(u.tobytes() == w.tobytes() for u, w in zip(ea, eb)), m
        assert np.diff(ea[1].astype(np.int64)).max() == m + 1
        ta.close(); tb.close()
    a.close(); b.close()


# ---- case 7: the mirror ------------------------------------------------------------------------------------------------------
def test_a_total_set_by_the_scalar_call_is_the_one_that_ranks(oracle_mod):
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    set_totals(src, o_src, [1, 2, 3, 4], [100, 4, 9, 16])
    one_row(src, o_src, 1, [2, 3, 4], [5, 5, 5])                           # scores 5 / 20, 5 / 30, 5 / 40
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    merged_cos(dst, o_dst, src, ops_of(o_src), "set", 1, 1, tag="before the scalar set")
    assert row_dict(dst, 1) == {0: 100, 2: 5}
    dst.close(); o_dst.close()
    assert src.set(2, 0, 10000) == o_src.set(2, 0, 10000)                  # 5 / 1000: column 2 is the worst now
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    merged_cos(dst, o_dst, src, ops_of(o_src), "set", 1, 1, tag="after the scalar set")
    assert row_dict(dst, 1) == {0: 100, 3: 5} and dst.get(2, 0) == 10000
    for h in (src, o_src, dst, o_dst):
        h.close()


# ---- case 8: serving ---------------------------------------------------------------------------------------------------------
def sessions_uniform():
    rng = np.random.default_rng(5)
    return [rng.choice(np.arange(1, 301), 10, replace=False).astype(np.uint32) for _ in range(400)]


def sessions_zipf():
    rng = np.random.default_rng(5)
    p = 1.0 / np.arange(1, 301) ** 1.1
    return [rng.choice(np.arange(1, 301), 10, replace=False, p=p / p.sum()).astype(np.uint32) for _ in range(400)]


def neighbours(m, items):
    """per item: (ids, scores) of its non-head neighbours, best score first"""
    off, ids, sc, cnt = m.cf_neighbors_batch(items)
    out = []
    for i in range(items.size):
        s = slice(int(off[i]), int(off[i]) + int(cnt[i]))
        j, t = ids[s], sc[s]
        j, t = j[j != 0], t[j != 0]
        order = np.lexsort((j, -t))
        out.append((j[order], t[order]))
    return out


def served_like_the_source(t, full, items, k):
    """the items whose k best scores (and the ids, where a score is unique in the row) t serves as the full matrix does"""
    same = []
    for (jt, st), (jf, sf) in zip(neighbours(t, items), full):
        ok = st.size == min(k, sf.size) and st.tobytes() == sf[:k].tobytes()
        if ok:
            unique = np.array([np.count_nonzero(sf == s) == 1 for s in st], bool)
            ok = (jt[unique] == jf[:k][unique]).all()
        same.append(bool(ok))
    return np.array(same)


@pytest.mark.parametrize("make", [sessions_uniform, sessions_zipf])
def test_a_cosine_truncated_copy_serves_the_best_scores(make):
    sessions = make()
    total = SparseMatrix()
    total.cf_import_sessions(sessions)
    items = np.unique(np.concatenate(sessions))
    full = neighbours(total, items)
    t = total.truncated(8, rank="cosine")
    same = served_like_the_source(t, full, items, 8)
    assert same.all(), (items[~same][:10], np.count_nonzero(~same))
    tv = total.truncated(8)
    same_v = served_like_the_source(tv, full, items, 8)
    print("%s: %d items; the value-ranked copy serves %d of them as the source does" % (make.__name__, items.size, np.count_nonzero(same_v)))
    assert not same_v.all()
    ids, scores, counts = t.cf_recommend_batch(sessions[:50], 5)
    assert (counts > 0).all() and np.isfinite(scores).all()
    for h in (total, t, tv):
        h.close()


# ---- case 9: a file-backed copy ----------------------------------------------------------------------------------------------
def test_truncated_into_a_file(oracle_mod, regimes, tmp_path):
    src, o_src, cand, table = regimes
    path = str(tmp_path / "serving.smx")
    t = src.truncated(64, rank="cosine", filename=path)
    assert t.getFilename() == path
    want = t.export("sorted")
    ops, _ = topk_cosine(cand, 64, 1)
    assert want[2].shape[0] == ops[0].size
    t.close()
    back = SparseMatrix(path)
    assert_export_equal(back.export("sorted"), want, "reopened")
    assert (back.get_batch(ops[0], ops[1]) == ops[2]).all()
    back.close()
    r = oracle_mod.Oracle(path)                                           # the file is the reference's format
    assert (r.apply(GET, ops[0], ops[1]) == ops[2]).all()
    r.close()
