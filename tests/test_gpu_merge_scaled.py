"""GPU (-m gpu): smatrix_merge_scaled (include/smatrix_batch.h; SparseMatrix.merge_scaled, SparseMatrix.pruned).  Every case runs
next to oracle_mod.Oracle(), in the style of tests/test_gpu_merge.py.

Expected ops: the source oracle's rows in list_rows() order and each row's non-empty slots in slot order are the candidates
(x, y, v); v' = v * num // den in numpy uint64; a candidate is dropped when v' < min_value or when y == 0 and v' == 0; the
survivors are fed to the destination's oracle one by one as op(x, y, v').

Compared after every call (`check`): n_ops and n_dropped; for every row id of either side the row's existence (row_info); get of
every cell of the union; for rows that hold no column-0 pair on either side, size and used; for rows with a column-0 pair the
probe invariant (their `used` depends on the history in the reference itself, Q1/Q2).  All comparisons are exact.  The cases keep
column-0 values from returning to a STORED 0 (Q3): a source's (0, 1) cell that a decay takes to 0 is dropped, never stored."""
import ctypes as C
import functools

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix
from tests import merge_helpers as H
from tests.merge_helpers import (DECR, GET, INCR, OPS, SET, assert_export_equal, both, check, col0_rows, device, ops_of, u32)  # noqa: F401

pytestmark = pytest.mark.gpu

PARAMS = [(1, 1, 1), (1, 2, 0), (1, 2, 1), (9, 10, 2), (1, 3, 1)]


def scaled(cand, num, den, min_value):
    """candidates -> (the surviving ops (x, y, v'), the number dropped)"""
    x, y, v = cand
    w = (v.astype(np.uint64) * np.uint64(num) // np.uint64(den)).astype(np.uint32)
    keep = (w >= np.uint32(min_value)) & ((y != 0) | (w != 0))
    return (x[keep], y[keep], w[keep]), int(x.size - np.count_nonzero(keep))


def merged_scaled(dst, o_dst, src, cand, op, num, den, min_value, max_batch=0, tag=""):
    """dst.merge_scaled(src) next to the oracle; checks the counts and the result; returns (n_ops, n_dropped)"""
    before = ops_of(o_dst)
    ops, dropped = scaled(cand, num, den, min_value)
    n, d = dst.merge_scaled(src, op, num, den, min_value, max_batch=max_batch)
    o_dst.apply(OPS[op], *ops)
    print("%s: %d candidates, %d applied, %d dropped (library: %d, %d)" % (tag, cand[0].size, ops[0].size, dropped, n, d))
    assert (n, d) == (ops[0].size, dropped), (tag, (n, d), (ops[0].size, dropped))
    check(dst, o_dst, (before, cand), set(), tag)
    return n, d


# ---- the sources of case 1 -------------------------------------------------------------------------------------------------
# Every source gets the same additions (rows 3000000 and up), so that every parameter set drops some candidates and keeps others
# whatever the source's own values are: values of 1, 2, 3 and of 4 and more, dead cells (a non-zero key whose value went back to
# 0), a column-0 cell of value 1 (what (1, 2, 0) drops: it would be the empty slot) and one of value 1000, a row that holds dead
# cells only, and a row of 3000 cells of which 2995 are dead -- its table is 8192 slots in the source and 16 in a pruned copy.
def additions(m, o):
    rng = np.random.default_rng(1234)
    xs = np.repeat(np.arange(3000000, 3000200, dtype=np.uint32), 10)
    ys = rng.integers(1, 1 << 32, xs.size, dtype=np.uint32)
    both(m, o, INCR, xs, ys, np.tile(u32(1, 1, 2, 3, 4, 5, 9, 10, 1000, 0xFFFFFFFF), 200))
    both(m, o, DECR, xs[::10], ys[::10], np.ones(200, np.uint32))                    # the first cell of each row: dead
    both(m, o, SET, u32(3000000, 3000001), u32(0, 0), u32(1, 1000))
    both(m, o, INCR, np.full(7, 3000300, np.uint32), np.arange(1, 8, dtype=np.uint32), np.full(7, 6, np.uint32))
    both(m, o, DECR, np.full(7, 3000300, np.uint32), np.arange(1, 8, dtype=np.uint32), np.full(7, 6, np.uint32))
    ys = rng.permutation(1 << 20)[:3000].astype(np.uint32) + 1
    both(m, o, INCR, np.full(3000, 3000400, np.uint32), ys, np.full(3000, 2, np.uint32))
    both(m, o, DECR, np.full(2995, 3000400, np.uint32), ys[5:], np.full(2995, 2, np.uint32))


# (sizes: a third to a half of tests/test_gpu_merge.py's; the long row with small and dead values mixed into every segment)
SOURCES = {"src_quirks": functools.partial(H.src_quirks, additions=additions),
           "src_zipf": functools.partial(H.src_zipf, n=300000, chunk=100000, additions=additions),
           "src_dense": functools.partial(H.src_dense, n=400000, additions=additions),
           "src_one_long_row": functools.partial(H.src_one_long_row, small=True, additions=additions)}


@pytest.fixture(scope="module")
def sources(oracle_mod, golden):
    """name -> (matrix, oracle, candidates, TABLE export), built once: no case may modify a source, and every case checks that"""
    made = {}

    def get(name):
        if name not in made:
            m, o = SparseMatrix(), oracle_mod.Oracle()
            SOURCES[name](m, o, golden)
            made[name] = (m, o, ops_of(o), m.export("table"))
        return made[name]
    yield get
    for m, o, _, _ in made.values():
        m.close(); o.close()


# ---- case 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num, den, min_value", PARAMS)
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_pruned_or_decayed_copy_into_an_empty_matrix(oracle_mod, sources, source, num, den, min_value):
    src, o_src, cand, table = sources(source)
    tag = "%s %d/%d min %d" % (source, num, den, min_value)
    ops, dropped = scaled(cand, num, den, min_value)
    assert 0 < dropped < cand[0].size, (tag, dropped, cand[0].size)     # from the oracle's numbers alone
    if source == "src_one_long_row":
        assert o_src.row_info(7)[0] == 1 << 19
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    merged_scaled(dst, o_dst, src, cand, "set", num, den, min_value, tag=tag)
    rows, ptr, pairs = dst.export("sorted")
    assert pairs.shape[0] == ops[0].size
    if min_value >= 1:
        assert (pairs[:, 1] >= min_value).all()
    if (num, den, min_value) == (1, 1, 1):                             # every source holds dead cells (additions)
        assert np.count_nonzero(cand[2] == 0) > 0
        print("%s: mem %d -> %d (oracle %d -> %d)" % (tag, src.mem, dst.mem, o_src.mem(), o_dst.mem()))
        assert o_dst.mem() < o_src.mem()
        assert dst.mem < src.mem
        assert o_src.row_info(3000400)[0] == 8192
        assert dst.row_info(3000400) == o_dst.row_info(3000400) == (16, 5)
    if min_value >= 1:
        assert dst.row_info(3000300) is None                           # a row of dead cells only
    else:                                                              # min_value 0: a (y != 0, 0) result still creates its cell
        assert dst.row_info(3000300) == o_dst.row_info(3000300) == (16, 7) and dst.getRowLength(3000300) == 7
    assert_export_equal(src.export("table"), table, tag + ": the source")
    dst.close(); o_dst.close()


# ---- case 2 ----------------------------------------------------------------------------------------------------------------
def overlapping(oracle_mod):
    """a destination and a source that share rows and cells partly; the source's values are 0 (dead) .. 8"""
    rng = np.random.default_rng(21)
    dst, o_dst, src, o_src = SparseMatrix(), oracle_mod.Oracle(), SparseMatrix(), oracle_mod.Oracle()
    n = 60000
    both(dst, o_dst, INCR, rng.integers(0, 2000, n, dtype=np.uint32), rng.integers(1, 3001, n, dtype=np.uint32), np.ones(n, np.uint32))
    both(src, o_src, INCR, rng.integers(1000, 3000, n, dtype=np.uint32), rng.integers(1, 3001, n, dtype=np.uint32),
         rng.integers(0, 9, n, dtype=np.uint32))
    # rows 5000..5199: 6 keys here, 6 others there of which 4 survive a min_value of 2 -> 10 > 8: from 16 to 32 slots
    xs = np.repeat(np.arange(5000, 5200, dtype=np.uint32), 6)
    both(dst, o_dst, SET, xs, np.tile(np.arange(1, 7, dtype=np.uint32), 200), np.full(xs.size, 2, np.uint32))
    both(src, o_src, SET, xs, np.tile(np.arange(101, 107, dtype=np.uint32), 200), np.tile(u32(1, 2, 5, 5, 8, 9), 200))
    # column-0 pairs on both sides, on one side only (values that no op of the cases brings back to a stored 0)
    both(dst, o_dst, SET, np.arange(1500, 1520, dtype=np.uint32), np.zeros(20, np.uint32), np.full(20, 1000, np.uint32))
    both(src, o_src, SET, np.arange(1510, 1530, dtype=np.uint32), np.zeros(20, np.uint32), np.full(20, 7, np.uint32))
    return dst, o_dst, src, o_src


def state(m, o):
    ids = sorted(set(o.list_rows().tolist()))
    col0 = col0_rows(o)
    return m.export("sorted"), [m.row_info(x) for x in ids if x not in col0]


def test_identity_is_merge(oracle_mod):
    a, o_a, src, o_src = overlapping(oracle_mod)
    b, o_b, src2, o_src2 = overlapping(oracle_mod)
    cand = ops_of(o_src)
    n_merge = b.merge(src2, "incr")
    n, d = merged_scaled(a, o_a, src, cand, "incr", 1, 1, 0, tag="identity")
    assert (n, d) == (n_merge, 0) and n == cand[0].size
    o_b.apply(INCR, *ops_of(o_src2))
    sa, sb = state(a, o_a), state(b, o_b)
    assert_export_equal(sa[0], sb[0], "identity")
    assert sa[1] == sb[1]
    for h in (a, o_a, b, o_b, src, o_src, src2, o_src2):
        h.close()


# ---- case 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["incr", "decr", "set"])
def test_scaled_merge_into_an_overlapping_destination(oracle_mod, op):
    dst, o_dst, src, o_src = overlapping(oracle_mod)
    cand = ops_of(o_src)
    table = src.export("table")
    grown0 = dst.stats()["rows_grown"]
    n, d = merged_scaled(dst, o_dst, src, cand, op, 2, 3, 2, tag=op)    # 0, 1, 2 -> dropped; 3 .. 8 -> 2 .. 5
    assert 0 < d < cand[0].size
    assert dst.stats()["rows_grown"] > grown0
    assert dst.row_info(5000) == o_dst.row_info(5000) == (32, 10)
    assert_export_equal(src.export("table"), table, "the source")
    for h in (src, o_src, dst, o_dst):
        h.close()


# ---- case 4 ----------------------------------------------------------------------------------------------------------------
def test_the_sliding_window(oracle_mod):
    rng = np.random.default_rng(77)
    days = []
    for k in range(3):
        m, o = SparseMatrix(), oracle_mod.Oracle()
        n = 80000
        # day k: rows 1000 k .. 1000 k + 2499 -- day 1's first 1000 rows are in no later day
        both(m, o, INCR, rng.integers(1000 * k, 1000 * k + 2500, n, dtype=np.uint32), rng.integers(1, 2000, n, dtype=np.uint32),
             rng.integers(1, 5, n, dtype=np.uint32))
        if k == 1:
            both(m, o, SET, np.arange(1200, 1210, dtype=np.uint32), np.zeros(10, np.uint32), np.full(10, 3, np.uint32))
        days.append((m, o, ops_of(o)))
    total, o_total = SparseMatrix(), oracle_mod.Oracle()
    for m, o, cand in days:
        total += m
        o_total.apply(INCR, *cand)
    total -= days[0][0]
    o_total.apply(DECR, *days[0][2])
    cand = ops_of(o_total)
    check(total, o_total, (), set(), "total")
    assert np.count_nonzero(cand[2] == 0) > 0                           # day 1's own cells are dead now
    before = total.export("table")
    p = total.pruned()
    assert_export_equal(total.export("table"), before, "total is unchanged")
    o_p = oracle_mod.Oracle()
    ops, dropped = scaled(cand, 1, 1, 1)
    assert dropped == np.count_nonzero(cand[2] == 0)
    o_p.apply(SET, *ops)
    check(p, o_p, (cand,), set(), "pruned")
    fresh = oracle_mod.Oracle()                                         # d2 then d3, and nothing else ever
    fresh.apply(INCR, *days[1][2])
    fresh.apply(INCR, *days[2][2])
    fx, fy, fv = ops_of(fresh)
    assert (p.get_batch(fx, fy) == fv).all()
    rows, ptr, pairs = p.export("sorted")
    assert pairs.shape[0] == fx.size and (pairs[:, 1] != 0).all()
    assert (rows == np.sort(fresh.list_rows().astype(np.uint32))).all()
    col0 = col0_rows((fx, fy, fv))
    assert col0
    for x in rows.tolist():
        if x not in col0:
            assert p.row_info(x) == fresh.row_info(x), x
    assert p.row_info(5) is None and total.row_info(5) is not None      # a row of day 1 only
    assert p.mem < total.mem
    for h in [total, o_total, p, o_p, fresh] + [h for d in days for h in d[:2]]:
        h.close()


# ---- case 5 ----------------------------------------------------------------------------------------------------------------
def test_rows_that_lose_every_pair_are_not_created(oracle_mod):
    rng = np.random.default_rng(8)
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    # row 50: 10000 cells of value 1 and 5 of value 100 -> more than 8192 cells in the source, 5 survivors: a 16-slot table
    ys = rng.permutation(1 << 22)[:10005].astype(np.uint32) + 1
    both(src, o_src, SET, np.full(10005, 50, np.uint32), ys, np.concatenate([np.ones(10000, np.uint32), np.full(5, 100, np.uint32)]))
    # row 60: as large, nothing survives; rows 1000..1999: 5 cells of value 1 each, nothing survives; rows 2000..2099 keep 2 of 5
    both(src, o_src, SET, np.full(10000, 60, np.uint32), ys[:10000], np.ones(10000, np.uint32))
    xs = np.repeat(np.arange(1000, 2100, dtype=np.uint32), 5)
    vs = np.where(xs >= 2000, np.tile(u32(1, 1, 1, 2, 3), 1100), 1).astype(np.uint32)
    both(src, o_src, SET, xs, rng.integers(1, 1 << 32, xs.size, dtype=np.uint32), vs)
    both(src, o_src, SET, u32(70), u32(0), u32(1))                       # row 70: a column-0 cell only, dropped by the min_value
    assert o_src.row_info(50)[0] > 8192 and o_src.row_info(60)[0] > 8192
    cand = ops_of(o_src)
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    n, d = merged_scaled(dst, o_dst, src, cand, "incr", 1, 1, 2, tag="rows that lose every pair")
    assert (n, d) == (5 + 200, 10000 + 10000 + 5000 + 300 + 1)
    assert dst.row_info(50) == o_dst.row_info(50) == (16, 5)
    for x in (60, 70, 1000, 1500, 1999):
        assert dst.row_info(x) is None and src.row_info(x) is not None, x
    assert dst.stats()["rows"] == 101
    for h in (src, o_src, dst, o_dst):
        h.close()


# ---- case 6 ----------------------------------------------------------------------------------------------------------------
def internal_batches(src, num, den, min_value, max_batch):
    """the internal batches of a call: whole rows of the source's TABLE export, in its order, as many as fit into max_batch
    surviving ops and at least one; rows without survivors start no batch"""
    rows, ptr, pairs = src.export("table")
    idx = np.repeat(np.arange(rows.size, dtype=np.uint32), np.diff(ptr.astype(np.int64)))      # position in the row list
    (sidx, _, _), _ = scaled((idx, pairs[:, 0], pairs[:, 1]), num, den, min_value)
    counts = np.bincount(sidx, minlength=rows.size)
    B = max_batch if max_batch else 1 << 24
    left, nb = 0, 0
    for c in counts.tolist():
        if c and (left < c):                                            # the row does not fit behind the rows before it
            nb += 1
            left = max(B, c)
        left -= c
    return nb, int(counts.max())


def test_the_result_does_not_depend_on_max_batch(oracle_mod):
    results = []
    for mb in (1000, 1 << 16, 0):
        dst, o_dst, src, o_src = overlapping(oracle_mod)
        want, _ = internal_batches(src, 1, 2, 1, mb)
        b0 = dst.stats()["batches"]
        merged_scaled(dst, o_dst, src, ops_of(o_src), "incr", 1, 2, 1, max_batch=mb, tag="max_batch %d" % mb)
        print("max_batch %d: %d internal batches, stats().batches grew by %d" % (mb, want, dst.stats()["batches"] - b0))
        assert dst.stats()["batches"] - b0 == want
        results.append(state(dst, o_dst))
        for h in (src, o_src, dst, o_dst):
            h.close()
    for r in results[1:]:
        assert_export_equal(r[0], results[0][0])
        assert r[1] == results[0][1]


def test_a_surviving_row_longer_than_max_batch_is_one_internal_batch(oracle_mod, sources):
    src, o_src, cand, table = sources("src_one_long_row")
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    want, longest = internal_batches(src, 1, 1, 2, 1000)
    survivors7 = int(np.count_nonzero((cand[0] == 7) & (cand[2] >= 2)))
    assert longest == survivors7 > 100000                               # the long row is cut by nothing: it is one batch
    b0 = dst.stats()["batches"]
    merged_scaled(dst, o_dst, src, cand, "set", 1, 1, 2, max_batch=1000, tag="long row, max_batch 1000")
    print("long row: %d internal batches, stats().batches grew by %d" % (want, dst.stats()["batches"] - b0))
    assert dst.stats()["batches"] - b0 == want > 1
    assert dst.getRowLength(7) == survivors7
    assert_export_equal(src.export("table"), table, "the source")
    dst.close(); o_dst.close()


# ---- case 7 ----------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(oracle_mod):
    a, b = SparseMatrix(), SparseMatrix()
    a.incr_batch(np.arange(100, dtype=np.uint32), np.arange(1, 101, dtype=np.uint32), np.ones(100, np.uint32))
    b.incr_batch(np.arange(50, 150, dtype=np.uint32), np.arange(1, 101, dtype=np.uint32), np.full(100, 4, np.uint32))
    ea, eb = a.export("table"), b.export("table")
    n, d = C.c_uint64(77), C.c_uint64(78)
    call = a._lib.smatrix_merge_scaled
    assert call(a._h, b._h, INCR, 1, 0, 0, 0, C.byref(n), C.byref(d)) == -1         # den == 0
    assert call(a._h, b._h, INCR, 0, 0, 0, 0, C.byref(n), C.byref(d)) == -1
    assert call(a._h, b._h, INCR, 0, 2, 0, 0, C.byref(n), C.byref(d)) == -1         # num == 0
    assert call(a._h, b._h, INCR, 3, 2, 0, 0, C.byref(n), C.byref(d)) == -1         # num > den
    assert call(a._h, b._h, GET, 1, 2, 0, 0, C.byref(n), C.byref(d)) == -1          # op GET
    assert call(a._h, b._h, 4, 1, 2, 0, 0, None, None) == -1
    assert call(a._h, a._h, INCR, 1, 2, 0, 0, C.byref(n), C.byref(d)) == -1         # dst is src
    assert (n.value, d.value) == (77, 78)
    with pytest.raises(ValueError):
        a.merge_scaled(a, "incr", 1, 2)
    with pytest.raises(ValueError):
        a.merge_scaled(b, "get", 1, 2)
    with pytest.raises(ValueError):
        a.merge_scaled(b, "incr", 2, 1)
    assert_export_equal(a.export("table"), ea)
    assert_export_equal(b.export("table"), eb)
    assert call(a._h, b._h, INCR, 1, 2, 0, 0, None, None) == 0                      # (both counts may be NULL)
    assert a.get(50, 1) == 2 and a.get(0, 1) == 1 and a.get(149, 100) == 2
    a.close(); b.close()


# ---- case 8 ----------------------------------------------------------------------------------------------------------------
def test_scalar_mirror_before_and_after(oracle_mod):
    a, o_a, b, o_b = SparseMatrix(), oracle_mod.Oracle(), SparseMatrix(), oracle_mod.Oracle()
    for m, o in ((a, o_a), (b, o_b)):
        for x in range(1, 40):
            for y in range(1, 12):
                assert m.incr(x, y, x + y) == o.incr(x, y, x + y)
    for k in range(5):                                                  # these sit in the host mirrors when the call starts
        assert a.incr(3, 4, 1) == o_a.incr(3, 4, 1)
        assert b.incr(3, 4, 10) == o_b.incr(3, 4, 10)
        assert b.incr(3, 5, 100) == o_b.incr(3, 5, 100)
    assert b.set(1, 1, 1) == o_b.set(1, 1, 1)                           # 2 -> 1: halves to 0, dropped -- if the call sees it
    cand = ops_of(o_b)
    n, d = merged_scaled(a, o_a, b, cand, "incr", 1, 2, 1, tag="mirror")
    assert (n, d) == (39 * 11 - 1, 1)
    assert a.get(3, 4) == o_a.get(3, 4) == 7 + 5 + (7 + 50) // 2        # scalar gets straight after: no stale mirror
    assert a.get(3, 5) == o_a.get(3, 5) == 8 + (8 + 500) // 2
    assert a.get(1, 1) == o_a.get(1, 1) == 2
    assert a.incr(3, 4, 1) == o_a.incr(3, 4, 1)
    assert b.get(3, 4) == o_b.get(3, 4) == 7 + 50                       # the source is as it was
    assert b.get(1, 1) == 1
    for h in (a, o_a, b, o_b):
        h.close()


# ---- case 9 ----------------------------------------------------------------------------------------------------------------
def test_file_backed_source_and_pruned_file(oracle_mod, tmp_path, monkeypatch):
    monkeypatch.setenv("SMATRIX_FLUSH_MS", "0")                          # explicit flushes only: the source's file is compared byte for byte
    rng = np.random.default_rng(44)
    p_src, p_new = str(tmp_path / "src.smx"), str(tmp_path / "pruned.smx")
    src, o_src = SparseMatrix(p_src), oracle_mod.Oracle()
    n = 60000
    both(src, o_src, INCR, rng.integers(0, 1200, n, dtype=np.uint32), rng.integers(1, 3000, n, dtype=np.uint32), rng.integers(0, 6, n, dtype=np.uint32))
    both(src, o_src, SET, np.arange(2000, 2050, dtype=np.uint32), np.full(50, 9, np.uint32), np.ones(50, np.uint32))      # rows that go away
    src.flush()
    src_bytes = open(p_src, "rb").read()
    cand = ops_of(o_src)
    ops, dropped = scaled(cand, 2, 3, 2)
    assert 0 < dropped < cand[0].size
    new = src.pruned(2, 2, 3, filename=p_new)
    assert new.getFilename() == p_new
    o_new = oracle_mod.Oracle()
    o_new.apply(SET, *ops)
    check(new, o_new, (cand,), set(), "pruned file, before close")
    new.close()
    src.flush()
    assert open(p_src, "rb").read() == src_bytes                        # no row of src was DIRTY
    src.close()
    back = SparseMatrix(p_new)
    check(back, o_new, (cand,), set(), "pruned file, reopened")
    x, y, v = ops
    assert (back.get_batch(x, y) == v).all()
    rows = np.unique(x)
    assert (back.rowlen_batch(rows) == np.array([o_new.rowlen(int(r)) for r in rows], np.uint32)).all()
    assert_export_equal(back.export("sorted")[0:1], (np.sort(o_new.list_rows().astype(np.uint32)),))
    assert back.row_info(2000) is None
    back.close()
    r = oracle_mod.Oracle(p_new)                                        # the file is the reference's format
    assert (r.apply(GET, x, y) == v).all()
    r.close()
    o_src.close(); o_new.close()
