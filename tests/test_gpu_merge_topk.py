"""GPU (-m gpu): smatrix_merge_topk (include/smatrix_batch.h; SparseMatrix.merge_topk, SparseMatrix.truncated).  Every case runs
next to oracle_mod.Oracle(), in the manner of tests/test_gpu_merge_scaled.py, on the helpers of tests/merge_helpers.py.

Expected ops, from numpy alone: the source oracle's candidates (rows in list_rows() order, non-empty slots in slot order); per row
the eligible pairs (y != 0, v >= min_value) sorted by (-v, y), the first m of them kept; the head pair (y == 0) kept iff
v >= min_value and v != 0, beside the m; the kept pairs are fed to the destination's oracle one by one as op(x, y, v).

Compared after every call, all exactly: n_ops and n_dropped; the row set; get of every candidate cell; size and used of rows
without a column-0 pair; the probe invariant of rows with one."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix
from tests.merge_helpers import (DECR, GET, INCR, M_MAX, OPS, REGIMES, SET, assert_export_equal, both, check,  # noqa: F401
                                 check_rows_around_one_step, device, one_row, ops_of, row_dict, u32)

pytestmark = pytest.mark.gpu


def topk(cand, m, min_value):
    """candidates -> (the kept ops (x, y, v), the number dropped)"""
    x, y, v = cand
    keep = np.zeros(x.size, bool)
    keep[(y == 0) & (v >= min_value) & (v != 0)] = True
    elig = (y != 0) & (v >= np.uint32(min_value))
    for row in np.unique(x).tolist():
        idx = np.flatnonzero(elig & (x == row))
        order = np.lexsort((y[idx], -v[idx].astype(np.int64)))           # by -v, then by y
        keep[idx[order[:m]]] = True
    return (x[keep], y[keep], v[keep]), int(x.size - np.count_nonzero(keep))


def merged_topk(dst, o_dst, src, cand, op, m, min_value, max_batch=0, tag=""):
    """dst.merge_topk(src) next to the oracle; checks the counts and the result; returns (kept ops, n_dropped)"""
    before = ops_of(o_dst)
    ops, dropped = topk(cand, m, min_value)
    n, d = dst.merge_topk(src, m, op, min_value, max_batch=max_batch)
    o_dst.apply(OPS[op], *ops)
    print("%s: %d candidates, %d applied, %d dropped (library: %d, %d)" % (tag, cand[0].size, ops[0].size, dropped, n, d))
    assert (n, d) == (ops[0].size, dropped), (tag, (n, d), (ops[0].size, dropped))
    check(dst, o_dst, (before, cand), set(), tag)
    return ops, d


# ---- case 1: the regimes -----------------------------------------------------------------------------------------------------
# the row shapes of tests/merge_helpers.REGIMES.  Values 1..5 (and 0 in row 11): ties everywhere.


@pytest.fixture(scope="module")
def regimes(oracle_mod):
    rng = np.random.default_rng(99)
    m, o = SparseMatrix(), oracle_mod.Oracle()
    for x, (n, size) in REGIMES.items():
        ys = (rng.permutation(1 << 20)[:n] + 1).astype(np.uint32)
        one_row(m, o, x, ys, rng.integers(0 if x == 11 else 1, 6, n))
        assert m.row_info(x) == o.row_info(x) and o.row_info(x)[0] == size, (x, m.row_info(x), o.row_info(x))
    both(m, o, SET, u32(12, 15), u32(0, 0), u32(1000, 3))                  # head pairs: one large, one among the ties
    xs = np.repeat(np.arange(1000, 1300, dtype=np.uint32), 12)            # and 300 short rows, so that the row list is not 7 rows
    both(m, o, INCR, xs, rng.integers(1, 1 << 32, xs.size, dtype=np.uint32), rng.integers(1, 4, xs.size, dtype=np.uint32))
    made = (m, o, ops_of(o), m.export("table"))
    yield made
    m.close(); o.close()


@pytest.mark.parametrize("m", [1, 7, 64, 5000])
def test_truncated_copy_of_every_regime(oracle_mod, regimes, m):
    src, o_src, cand, table = regimes
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    ops, dropped = merged_topk(dst, o_dst, src, cand, "set", m, 1, tag="regimes m %d" % m)
    for x, (n, size) in REGIMES.items():
        kept = int(np.count_nonzero((ops[0] == x) & (ops[1] != 0)))
        elig = int(np.count_nonzero((cand[0] == x) & (cand[1] != 0) & (cand[2] >= 1)))
        assert kept == min(m, elig), (x, kept, elig)
        assert len(row_dict(dst, x)) == kept + (x in (12, 15))
    if m == 5000:                                                         # the cut rows really lose pairs, the short ones none
        assert np.count_nonzero((ops[0] == 15) & (ops[1] != 0)) == 5000 < 20000
        assert np.count_nonzero((ops[0] == 16) & (ops[1] != 0)) == 5000 < 40000
        assert np.count_nonzero(ops[0] == 12) == 3001
    assert dst.get(12, 0) == 1000 and dst.get(15, 0) == 3
    assert_export_equal(src.export("table"), table, "the source")
    dst.close(); o_dst.close()


def test_rows_around_one_step_of_a_wave(oracle_mod):
    check_rows_around_one_step(oracle_mod, merged_topk, column_totals=False)


# ---- case 2: the digit passes ------------------------------------------------------------------------------------------------
def test_rows_whose_keys_differ_in_one_byte_only(oracle_mod):
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    one_row(src, o_src, 1, np.arange(1, 201), np.full(200, 7))                                # the last byte of the key only
    one_row(src, o_src, 2, np.arange(1, 201) * 977, np.arange(1, 201, dtype=np.uint64) << 24 & 0xFFFFFFFF)  # the top byte only
    one_row(src, o_src, 3, [1, M_MAX, 5, 6, 7, 8], [M_MAX, M_MAX, M_MAX, 1, M_MAX - 1, 0])   # the extremes of both halves
    cand = ops_of(o_src)
    for x, m in ((1, 100), (2, 100), (3, 3)):
        dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
        sel = cand[0] == x
        ops, _ = merged_topk(dst, o_dst, src, cand, "set", m, 0, tag="digits row %d" % x)
        rows, ptr, pairs = dst.export("sorted")
        i = int(np.flatnonzero(rows == x)[0])
        got = pairs[int(ptr[i]):int(ptr[i + 1])]
        assert got.shape[0] == m
        if x == 1:
            assert (got[:, 0] == np.arange(1, 101)).all()                  # equal values: the lowest columns
        if x == 2:
            assert (np.sort(got[:, 1]) == np.sort(cand[2][sel])[-100:]).all()
        if x == 3:
            assert got.tolist() == [[1, M_MAX], [5, M_MAX], [M_MAX, M_MAX]]
        dst.close(); o_dst.close()
    src.close(); o_src.close()


# ---- case 3: the edges -------------------------------------------------------------------------------------------------------
def edge_source(oracle_mod):
    """row 1: 20 live pairs and 5 dead cells; row 2: dead cells only; row 3: a head pair of 1 and two pairs; row 4: a head pair of
    1000 and three pairs; rows 100..: 9 pairs each"""
    src, o = SparseMatrix(), oracle_mod.Oracle()
    one_row(src, o, 1, np.arange(1, 26), np.arange(1, 26))
    both(src, o, DECR, np.full(5, 1, np.uint32), np.arange(1, 6, dtype=np.uint32), np.arange(1, 6, dtype=np.uint32))
    one_row(src, o, 2, np.arange(1, 8), np.full(7, 6))
    both(src, o, DECR, np.full(7, 2, np.uint32), np.arange(1, 8, dtype=np.uint32), np.full(7, 6, np.uint32))
    one_row(src, o, 3, [0, 5, 6], [1, 4, 4])
    one_row(src, o, 4, [0, 5, 6, 7], [1000, 2, 9, 9])
    xs = np.repeat(np.arange(100, 150, dtype=np.uint32), 9)
    both(src, o, SET, xs, np.tile(np.arange(1, 10, dtype=np.uint32), 50), (xs % 5 + 1).astype(np.uint32))
    return src, o


@pytest.mark.parametrize("m", [19, 20, 21, M_MAX])
def test_m_around_the_eligible_count(oracle_mod, m):
    src, o_src = edge_source(oracle_mod)
    cand = ops_of(o_src)
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    merged_topk(dst, o_dst, src, cand, "set", m, 1, tag="edges m %d" % m)
    assert len(row_dict(dst, 1)) == min(m, 20)
    assert dst.row_info(2) is None                                        # a row of dead cells only, min_value 1: not created
    if m == M_MAX:                                                        # == merge_scaled(1, 1, min_value)
        ref = SparseMatrix()
        assert ref.merge_scaled(src, "set", 1, 1, 1) == dst.merge_topk(src, m, "set", 1)
        assert_export_equal(ref.export("sorted"), dst.export("sorted"), "against merge_scaled")
        ref.close()
    for h in (src, o_src, dst, o_dst):
        h.close()


def test_dead_cells_head_pairs_and_refusals(oracle_mod):
    src, o_src = edge_source(oracle_mod)
    cand = ops_of(o_src)
    for min_value in (0, 1):                                              # 25 cells, 20 live: m = 22 takes two dead cells with min_value 0
        dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
        merged_topk(dst, o_dst, src, cand, "set", 22, min_value, tag="dead cells, min_value %d" % min_value)
        assert dst.row_info(1) == o_dst.row_info(1) and len(row_dict(dst, 1)) == (22 if min_value == 0 else 20)
        if min_value == 0:
            assert dst.row_info(2) == o_dst.row_info(2) == (16, 7)
            assert sorted(row_dict(dst, 1))[:2] == [1, 2]                  # the dead cells of the lowest columns
        else:
            assert dst.row_info(2) is None
        dst.close(); o_dst.close()
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    merged_topk(dst, o_dst, src, cand, "set", 1, 2, tag="head pairs")
    assert row_dict(dst, 3) == {5: 4}                                       # head pair 1 < min_value 2: dropped
    assert row_dict(dst, 4) == {0: 1000, 6: 9}                              # head pair beside the ONE best pair (9 at the lower column)
    # refusals: -1 and nothing changed
    before = dst.export("table")
    n, d = C.c_uint64(77), C.c_uint64(78)
    call = dst._lib.smatrix_merge_topk
    assert call(dst._h, src._h, SET, 0, 1, 0, C.byref(n), C.byref(d)) == -1          # m == 0
    assert call(dst._h, dst._h, SET, 5, 1, 0, C.byref(n), C.byref(d)) == -1          # dst is src
    assert call(dst._h, src._h, GET, 5, 1, 0, C.byref(n), C.byref(d)) == -1
    assert call(dst._h, src._h, 4, 5, 1, 0, None, None) == -1
    assert (n.value, d.value) == (77, 78)
    with pytest.raises(ValueError):
        dst.merge_topk(dst, 5)
    with pytest.raises(ValueError):
        dst.merge_topk(src, 0)
    assert_export_equal(dst.export("table"), before)
    assert call(dst._h, src._h, INCR, 5, 1, 0, None, None) == 0                     # (both counts may be NULL)
    for h in (src, o_src, dst, o_dst):
        h.close()


# ---- case 4: INCR and DECR into a destination that holds something --------------------------------------------------------
def test_incr_then_decr_gives_the_old_values_back(oracle_mod):
    rng = np.random.default_rng(3)
    src, o_src, dst, o_dst = SparseMatrix(), oracle_mod.Oracle(), SparseMatrix(), oracle_mod.Oracle()
    n = 40000
    both(src, o_src, INCR, rng.integers(0, 300, n, dtype=np.uint32), rng.integers(1, 2000, n, dtype=np.uint32), rng.integers(0, 4, n, dtype=np.uint32))
    both(dst, o_dst, INCR, rng.integers(100, 400, n, dtype=np.uint32), rng.integers(1, 2000, n, dtype=np.uint32), np.ones(n, np.uint32))
    cand = ops_of(o_src)
    x, y, _ = cand
    old = dst.get_batch(x, y)
    ops, dropped = merged_topk(dst, o_dst, src, cand, "incr", 20, 1, tag="incr")
    assert 0 < dropped and ops[0].size > 0
    merged_topk(dst, o_dst, src, cand, "decr", 20, 1, tag="decr")
    assert (dst.get_batch(x, y) == old).all()
    for h in (src, o_src, dst, o_dst):
        h.close()


# ---- case 5: batches ---------------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_max_batch(oracle_mod, regimes):
    src, o_src, cand, table = regimes
    exports, grew = [], []
    for mb in (1, 1000, 0):
        dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
        b0 = dst.stats()["batches"]
        ops, _ = merged_topk(dst, o_dst, src, cand, "set", 64, 1, max_batch=mb, tag="max_batch %d" % mb)
        grew.append(dst.stats()["batches"] - b0)
        exports.append(dst.export("sorted"))
        dst.close(); o_dst.close()
    rows_kept = np.unique(ops[0]).size
    print("internal batches:", grew)
    assert grew[0] == rows_kept and grew[2] == 1 and grew[0] > grew[1] > grew[2]      # 1: a batch per surviving row; 0: one
    assert_export_equal(exports[0], exports[1]); assert_export_equal(exports[0], exports[2])


# ---- case 6: history independence --------------------------------------------------------------------------------------------
def test_the_kept_set_depends_on_the_contents_alone(oracle_mod):
    rng = np.random.default_rng(17)
    n = 60000
    x = np.concatenate([rng.integers(0, 400, n, dtype=np.uint32), np.full(12000, 7, np.uint32)])
    y = np.concatenate([rng.integers(1, 3000, n, dtype=np.uint32), (rng.permutation(1 << 18)[:12000] + 1).astype(np.uint32)])
    v = rng.integers(1, 4, x.size, dtype=np.uint32)
    a, b = SparseMatrix(), SparseMatrix()
    p = rng.permutation(x.size)
    a.apply_batch(INCR, x[p], y[p], v[p], results=False)                   # one batch, shuffled
    b.apply_batch(INCR, x[:10], y[:10], v[:10], results=False)            # a tiny first batch, then growth in steps
    for s in range(10, x.size, 9000):
        b.apply_batch(INCR, x[s:s + 9000], y[s:s + 9000], v[s:s + 9000], results=False)
    assert_export_equal(a.export("sorted"), b.export("sorted"), "the sources")
    assert a.row_info(7)[0] > 8192
    for m in (5, 300):
        ta, tb = a.truncated(m), b.truncated(m)
        ea, eb = ta.export("sorted"), tb.export("sorted")
        assert all(u.tobytes() == w.tobytes() for u, w in zip(ea, eb)), m
        assert np.diff(ea[1].astype(np.int64)).max() == m
        ta.close(); tb.close()
    a.close(); b.close()


# ---- case 7: serving ---------------------------------------------------------------------------------------------------------
def test_a_truncated_copy_serves_the_same_scores(oracle_mod):
    rng = np.random.default_rng(5)
    sessions = [rng.choice(np.arange(1, 301), 10, replace=False).astype(np.uint32) for _ in range(400)]
    total = SparseMatrix()
    total.cf_import_sessions(sessions)
    t = total.truncated(8)
    items = np.arange(1, 301, dtype=np.uint32)
    rows, ptr, pairs = t.export("sorted")
    assert np.diff(ptr.astype(np.int64)).max() == 9                       # 8 neighbours and the item's total
    assert (pairs[ptr[:-1].astype(np.int64), 0] == 0).all()               # every row kept its head pair
    off_t, ids_t, sc_t, cnt_t = t.cf_neighbors_batch(items)
    off_f, ids_f, sc_f, cnt_f = total.cf_neighbors_batch(items)
    seen = 0
    for i in range(items.size):
        full = dict(zip(ids_f[int(off_f[i]):int(off_f[i]) + int(cnt_f[i])].tolist(), sc_f[int(off_f[i]):int(off_f[i]) + int(cnt_f[i])].tolist()))
        for j, s in zip(ids_t[int(off_t[i]):int(off_t[i]) + int(cnt_t[i])].tolist(), sc_t[int(off_t[i]):int(off_t[i]) + int(cnt_t[i])].tolist()):
            assert full[j] == s, (int(items[i]), j, s, full[j])          # bit-equal: both totals survived
            seen += 1
    assert seen >= 8 * 150
    ids, scores, counts = t.cf_recommend_batch(sessions[:50], 5)
    assert (counts > 0).all() and np.isfinite(scores).all()
    total.close(); t.close()


# ---- case 8: a file-backed copy ----------------------------------------------------------------------------------------------
def test_truncated_into_a_file(oracle_mod, regimes, tmp_path):
    src, o_src, cand, table = regimes
    path = str(tmp_path / "serving.smx")
    t = src.truncated(64, filename=path)
    assert t.getFilename() == path
    want = t.export("sorted")
    ops, _ = topk(cand, 64, 1)
    assert want[2].shape[0] == ops[0].size
    t.close()
    back = SparseMatrix(path)
    assert_export_equal(back.export("sorted"), want, "reopened")
    assert (back.get_batch(ops[0], ops[1]) == ops[2]).all()
    back.close()
    r = oracle_mod.Oracle(path)                                           # the file is the reference's format
    assert (r.apply(GET, ops[0], ops[1]) == ops[2]).all()
    r.close()
