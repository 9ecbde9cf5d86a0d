"""GPU (-m gpu): smatrix_merge / smatrix_import_csr (include/smatrix_batch.h; SparseMatrix.merge, +=, -=, import_csr,
import_csr_dev, from_sparse_coo).  Every case runs next to oracle_mod.Oracle(): the expected state of the destination is the
oracle fed the same ops one by one -- for a merge the source oracle's rows in list_rows() order and each row's non-empty slots
in slot order.

Compared after every call (`check`): for every row id of either side the row's existence (row_info); get of every cell of the
union; for rows that hold no column-0 pair on either side, size and used; for rows with a column-0 pair `used` depends on the
history in the reference itself (Q1/Q2), so there the values and the probe invariant are checked instead (every key reachable
from y % size with no empty slot on the way, no key twice).  The cases keep column-0 values from returning to 0: a (0, v) cell
that goes back to (0, 0) cuts probe chains in the reference (Q3), and which ones depends on the order inside a batch."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix
from tests.merge_helpers import (DECR, GET, INCR, OPS, SET, assert_export_equal, both, check, col0_rows, device, ops_of,  # noqa: F401
                                 src_dense, src_one_long_row, src_quirks, src_zipf)

pytestmark = pytest.mark.gpu


def merged(dst, o_dst, src, o_src, op, max_batch=0, tag=""):
    """dst.merge(src) next to the oracle; checks the result; returns n_ops"""
    col0 = col0_rows(o_dst, o_src)
    x, y, v = ops_of(o_src)
    n = dst.merge(src, op, max_batch=max_batch)
    o_dst.apply(OPS[op], x, y, v)
    assert n == x.size, (tag, n, x.size)
    check(dst, o_dst, (o_dst, o_src), col0 | col0_rows(o_dst), tag)
    return n


def without_empty_rows(ex):
    rows, ptr, pairs = ex
    keep = np.diff(ptr.astype(np.int64)) > 0
    return rows[keep], np.concatenate([ptr[:1], ptr[1:][keep]]), pairs


# ---- case 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", [src_quirks, src_zipf, src_dense, src_one_long_row])
def test_merge_into_an_empty_matrix_reproduces_the_source(oracle_mod, golden, source):
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    source(src, o_src, golden)
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    merged(dst, o_dst, src, o_src, "incr", tag=source.__name__)
    assert_export_equal(dst.export("sorted"), without_empty_rows(src.export("sorted")), source.__name__)
    if source is src_dense:
        # the same again into the rows that now exist: every op walks the dense tables' long runs, which is what switches a
        # matrix into clustered mode
        merged(dst, o_dst, src, o_src, "incr", tag="dense, second time")
        print("clustered_mode after a dense-id merge:", dst.stats()["clustered_mode"], "long_probe_rounds:", dst.stats()["long_probe_rounds"])
        assert dst.stats()["clustered_mode"] == 1
    for h in (src, o_src, dst, o_dst):
        h.close()


# ---- case 2: a non-empty destination that overlaps the source partly -----------------------------------------------------
def overlapping(oracle_mod):
    rng = np.random.default_rng(21)
    dst, o_dst, src, o_src = SparseMatrix(), oracle_mod.Oracle(), SparseMatrix(), oracle_mod.Oracle()
    n = 150000
    # rows 0..1999 in dst, 1000..2999 in src; columns 1..5000: shared rows hold shared and new columns, and grow (64 -> 128 -> 256)
    both(dst, o_dst, INCR, rng.integers(0, 2000, n, dtype=np.uint32), rng.integers(1, 5001, n, dtype=np.uint32), np.ones(n, np.uint32))
    both(src, o_src, INCR, rng.integers(1000, 3000, n, dtype=np.uint32), rng.integers(1, 5001, n, dtype=np.uint32), np.full(n, 3, np.uint32))
    # rows 5000..5199: 6 keys here, 6 others there -> 12 > 8: the merge takes them from 16 to 32 slots
    xs = np.repeat(np.arange(5000, 5200, dtype=np.uint32), 6)
    both(dst, o_dst, SET, xs, np.tile(np.arange(1, 7, dtype=np.uint32), 200), np.full(xs.size, 2, np.uint32))
    both(src, o_src, SET, xs, np.tile(np.arange(101, 107, dtype=np.uint32), 200), np.full(xs.size, 5, np.uint32))
    # column-0 pairs on both sides, on one side only (values that no op of the cases brings back to 0)
    both(dst, o_dst, SET, np.arange(1500, 1520, dtype=np.uint32), np.zeros(20, np.uint32), np.full(20, 1000, np.uint32))
    both(src, o_src, SET, np.arange(1510, 1530, dtype=np.uint32), np.zeros(20, np.uint32), np.full(20, 7, np.uint32))
    return dst, o_dst, src, o_src


@pytest.mark.parametrize("op", ["incr", "decr", "set"])
def test_merge_into_an_overlapping_destination(oracle_mod, op):
    dst, o_dst, src, o_src = overlapping(oracle_mod)
    grown0 = dst.stats()["rows_grown"]
    merged(dst, o_dst, src, o_src, op, tag=op)
    assert dst.stats()["rows_grown"] > grown0
    assert dst.row_info(5000)[0] == 32 and o_dst.row_info(5000)[0] == 32
    if op == "decr":                                                   # 1 - 3 wraps (S2); a key only in src: 0 - 3
        x, y, v = ops_of(o_src)
        assert (o_dst.apply(GET, x, y) > 0x80000000).any()
    for h in (src, o_src, dst, o_dst):
        h.close()


# ---- case 3 ----------------------------------------------------------------------------------------------------------------
def test_add_then_subtract_restores_every_value(oracle_mod):
    rng = np.random.default_rng(33)
    a, o_a, b, o_b = SparseMatrix(), oracle_mod.Oracle(), SparseMatrix(), oracle_mod.Oracle()
    n = 100000
    both(a, o_a, INCR, rng.integers(0, 1500, n, dtype=np.uint32), rng.integers(1, 4000, n, dtype=np.uint32), rng.integers(1, 100, n, dtype=np.uint32))
    both(b, o_b, INCR, rng.integers(1000, 2500, n, dtype=np.uint32), rng.integers(1, 4000, n, dtype=np.uint32), rng.integers(1, 100, n, dtype=np.uint32))
    ax, ay, av = ops_of(o_a)
    bx, by, bv = ops_of(o_b)
    a += b
    o_a.apply(INCR, bx, by, bv)
    check(a, o_a, (o_a, o_b), set(), "a += b")
    a -= b
    o_a.apply(DECR, bx, by, bv)
    check(a, o_a, (o_a, o_b), set(), "a -= b")
    assert (a.get_batch(ax, ay) == av).all()
    created = ~np.isin(bx.astype(np.uint64) << 32 | by, ax.astype(np.uint64) << 32 | ay)
    assert created.any() and (a.get_batch(bx[created], by[created]) == 0).all()      # S3: the cells stay, with value 0
    rows = np.unique(np.concatenate([ax, bx]))
    want = np.array([o_a.rowlen(int(r)) for r in rows], np.uint32)
    assert (a.rowlen_batch(rows) == want).all()
    only_b = np.setdiff1d(bx, ax)
    assert only_b.size and all(a.getRowLength(int(r)) == np.count_nonzero(bx == r) for r in only_b[:20])
    for h in (a, o_a, b, o_b):
        h.close()


# ---- case 4 ----------------------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_max_batch(oracle_mod):
    results = []
    for mb in (1, 1000, 1 << 16, 0):
        dst, o_dst, src, o_src = overlapping(oracle_mod)
        merged(dst, o_dst, src, o_src, "incr", max_batch=mb, tag="max_batch %d" % mb)
        ids = sorted(set(o_dst.list_rows().tolist()))
        col0 = col0_rows(o_dst)
        results.append((dst.export("sorted"), [dst.row_info(x) for x in ids if x not in col0]))
        for h in (src, o_src, dst, o_dst):
            h.close()
    for r in results[1:]:
        assert_export_equal(r[0], results[0][0])
        assert r[1] == results[0][1]


def test_a_row_longer_than_max_batch_is_one_internal_batch(oracle_mod, golden):
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    src_one_long_row(src, o_src, golden)
    dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
    merged(dst, o_dst, src, o_src, "set", max_batch=1000, tag="long row, max_batch 1000")
    assert dst.stats()["batches"] > 1
    assert dst.getRowLength(7) == 200000
    for h in (src, o_src, dst, o_dst):
        h.close()


# ---- case 5: CSR import ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "table"])
def test_import_csr_is_the_inverse_of_export(oracle_mod, golden, order):
    import torch
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    src_one_long_row(src, o_src, golden)
    src_quirks(src, o_src, golden)
    want = src.export("sorted")
    a = SparseMatrix()
    n = a.import_csr(*src.export(order), max_batch=50000)
    assert n == want[2].shape[0]
    assert_export_equal(a.export("sorted"), without_empty_rows(want), order + " host")
    b = SparseMatrix()
    rows, ptr, pairs = src.export_dev(order)
    assert b.import_csr_dev(rows, ptr, pairs, max_batch=50000) == n
    assert_export_equal(b.export("sorted"), without_empty_rows(want), order + " dev")
    c = SparseMatrix()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rows2, ptr2, pairs2 = rows.clone(), ptr.clone(), pairs.clone()
    assert c.import_csr_dev(rows2, ptr2, pairs2, "incr", stream=st) == n
    assert_export_equal(c.export("sorted"), without_empty_rows(want), order + " dev, own stream")
    for h in (src, o_src, a, b, c):
        h.close()


def csr_ops(rows, ptr, pairs):
    x = np.repeat(np.asarray(rows, np.uint32), np.diff(np.asarray(ptr, np.int64)))
    p = np.asarray(pairs, np.uint32).reshape(-1, 2)
    return x, p[:, 0].copy(), p[:, 1].copy()


@pytest.mark.parametrize("flavour", ["host", "dev"])
def test_import_csr_repeats_empty_rows_and_bad_row_ptr(oracle_mod, flavour):
    import torch

    def imp(m, rows, ptr, pairs, op, mb):
        rows, ptr, pairs = np.asarray(rows, np.uint32), np.asarray(ptr, np.uint64), np.asarray(pairs, np.uint32).reshape(-1, 2)
        if flavour == "host":
            return m.import_csr(rows, ptr, pairs, op, max_batch=mb)
        t = lambda a, dt: torch.from_numpy(a.view(dt).copy()).cuda()
        return m.import_csr_dev(t(rows, np.int32), t(ptr, np.int64), t(pairs, np.int32), op, max_batch=mb)

    # row 9 twice, empty rows in front, between and behind, column 4 of row 9 three times (positions 1, 4 and 6)
    rows = [3, 9, 5, 5, 9, 8, 2]
    ptr = [0, 0, 3, 3, 3, 7, 8, 8]
    pairs = [[1, 10], [4, 11], [2, 12], [7, 13], [4, 14], [0xFFFFFFFF, 15], [4, 16], [1, 17]]
    x, y, v = csr_ops(rows, ptr, pairs)
    for op in ("set", "incr", "decr"):
        for mb in (1, 2, 3, 0):                                       # 1, 2, 3: the occurrences of (9, 4) land in different internal batches
            m, o = SparseMatrix(), oracle_mod.Oracle()
            both(m, o, INCR, np.array([9, 9, 8], np.uint32), np.array([4, 30, 1], np.uint32), np.array([100, 1, 1], np.uint32))
            assert imp(m, rows, ptr, pairs, op, mb) == 8
            o.apply(OPS[op], x, y, v)
            check(m, o, (o,), set(), "%s max_batch %d" % (op, mb))
            if op == "set":
                assert m.get(9, 4) == 16                                  # the last occurrence wins
            assert m.row_info(3) is None and m.row_info(5) is None and m.row_info(2) is None      # rows without pairs are not created
            m.close(); o.close()
    m = SparseMatrix()
    m.incr(1, 2, 3)
    before = m.export("sorted")
    assert imp(m, [], [0], [], "set", 0) == 0                             # n_rows == 0
    for bad_ptr in ([0, 2, 1, 8], [1, 2, 3, 8], [0, 9, 8, 8]):
        with pytest.raises(ValueError):
            imp(m, [1, 2, 3], bad_ptr, pairs + [[5, 5]], "set", 0)
    assert m._lib.smatrix_import_csr(m._h, GET, 0, None, None, None, 0, None) == -1
    assert_export_equal(m.export("sorted"), before)
    m.close()


def test_from_sparse_coo_round_trip(oracle_mod, golden):
    import torch
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    rng = np.random.default_rng(9)
    n = 50000
    both(src, o_src, INCR, rng.integers(0, 3000, n, dtype=np.uint32), rng.integers(0, 1 << 20, n, dtype=np.uint32), rng.integers(1, 1 << 32, n, dtype=np.uint32))
    both(src, o_src, SET, np.array([0x7FFFFFFF], np.uint32), np.array([0x7FFFFFFE], np.uint32), np.array([0xFFFFFFFF], np.uint32))
    t = src.to_sparse_coo()
    a = SparseMatrix()
    assert a.from_sparse_coo(t) == t._nnz()
    assert_export_equal(a.export("sorted"), src.export("sorted"))
    # uncoalesced: repeated indices are repeated ops
    idx = torch.tensor([[5, 5, 6], [1, 1, 2]], device="cuda")
    u = torch.sparse_coo_tensor(idx, torch.tensor([10, 20, 30], device="cuda"), size=(8, 8))
    b = SparseMatrix()
    assert b.from_sparse_coo(u) == 3 and b.get(5, 1) == 30 and b.get(6, 2) == 30
    assert b.from_sparse_coo(u, "set") == 3 and b.get(5, 1) == 20
    with pytest.raises(ValueError):
        b.from_sparse_coo(torch.sparse_coo_tensor(torch.tensor([[1 << 32], [1]], device="cuda"), torch.tensor([1], device="cuda"), size=((1 << 32) + 1, 4)))
    with pytest.raises(ValueError):
        b.from_sparse_coo(torch.sparse_coo_tensor(idx, torch.tensor([1.0, 2.0, 3.0], device="cuda"), size=(8, 8)))
    for h in (src, o_src, a, b):
        h.close()


# ---- case 6 ----------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(oracle_mod):
    a, b = SparseMatrix(), SparseMatrix()
    a.incr_batch(np.arange(100, dtype=np.uint32), np.arange(1, 101, dtype=np.uint32), np.ones(100, np.uint32))
    b.incr_batch(np.arange(50, 150, dtype=np.uint32), np.arange(1, 101, dtype=np.uint32), np.ones(100, np.uint32))
    ea, eb = a.export("table"), b.export("table")
    n = C.c_uint64(77)
    assert a._lib.smatrix_merge(a._h, a._h, INCR, 0, C.byref(n)) == -1
    assert a._lib.smatrix_merge(a._h, b._h, GET, 0, C.byref(n)) == -1
    assert a._lib.smatrix_merge(a._h, b._h, 4, 0, None) == -1
    with pytest.raises(ValueError):
        a.merge(a)
    with pytest.raises(ValueError):
        a.merge(b, "get")
    assert_export_equal(a.export("table"), ea)
    assert_export_equal(b.export("table"), eb)
    a.close(); b.close()


# ---- case 7 ----------------------------------------------------------------------------------------------------------------
def test_scalar_mirror_before_and_after(oracle_mod):
    a, o_a, b, o_b = SparseMatrix(), oracle_mod.Oracle(), SparseMatrix(), oracle_mod.Oracle()
    for m, o in ((a, o_a), (b, o_b)):
        for x in range(1, 40):
            for y in range(1, 12):
                assert m.incr(x, y, x + y) == o.incr(x, y, x + y)
    for k in range(5):                                                  # these sit in the host mirrors when the merge starts
        assert a.incr(3, 4, 1) == o_a.incr(3, 4, 1)
        assert b.incr(3, 4, 10) == o_b.incr(3, 4, 10)
        assert b.incr(3, 5, 100) == o_b.incr(3, 5, 100)
    assert merged(a, o_a, b, o_b, "incr", tag="mirror") == 39 * 11
    assert a.get(3, 4) == o_a.get(3, 4) == 2 * 7 + 5 + 50               # scalar gets straight after: no stale mirror
    assert a.get(3, 5) == o_a.get(3, 5) == 2 * 8 + 500
    assert a.incr(3, 4, 1) == o_a.incr(3, 4, 1)
    assert b.get(3, 4) == o_b.get(3, 4) == 7 + 50                       # the source is as it was
    for h in (a, o_a, b, o_b):
        h.close()


# ---- case 8 ----------------------------------------------------------------------------------------------------------------
def test_file_backed_destination_and_source(oracle_mod, tmp_path, monkeypatch):
    monkeypatch.setenv("SMATRIX_FLUSH_MS", "0")                          # explicit flushes only: the source's file is compared byte for byte
    rng = np.random.default_rng(44)
    p_dst, p_src = str(tmp_path / "dst.smx"), str(tmp_path / "src.smx")
    dst, o_dst, src, o_src = SparseMatrix(p_dst), oracle_mod.Oracle(), SparseMatrix(p_src), oracle_mod.Oracle()
    n = 60000
    both(dst, o_dst, INCR, rng.integers(0, 800, n, dtype=np.uint32), rng.integers(1, 3000, n, dtype=np.uint32), rng.integers(1, 50, n, dtype=np.uint32))
    both(src, o_src, INCR, rng.integers(400, 1200, n, dtype=np.uint32), rng.integers(1, 3000, n, dtype=np.uint32), rng.integers(1, 50, n, dtype=np.uint32))
    dst.flush(); src.flush()
    src_bytes = open(p_src, "rb").read()
    flushes0 = src.stats()["file_flushes"], src.stats()["file_rows_written"]
    merged(dst, o_dst, src, o_src, "incr", max_batch=20000, tag="file mode")
    src.flush()
    assert (src.stats()["file_flushes"], src.stats()["file_rows_written"])[1] == flushes0[1]       # no row of src was DIRTY
    assert open(p_src, "rb").read() == src_bytes
    dst.close(); src.close()
    assert open(p_src, "rb").read() == src_bytes
    x, y, v = ops_of(o_dst)
    back = SparseMatrix(p_dst)
    assert (back.get_batch(x, y) == v).all()
    rows = np.unique(x)
    assert (back.rowlen_batch(rows) == np.array([o_dst.rowlen(int(r)) for r in rows], np.uint32)).all()
    assert_export_equal(back.export("sorted")[0:1], (np.sort(o_dst.list_rows().astype(np.uint32)),))
    back.close()
    readers = [oracle_mod.Oracle] + ([oracle_mod.Reference] if oracle_mod.have_reference() else [])
    for k, reader in enumerate(readers):
        snap = str(tmp_path / ("snap%d.smx" % k))
        shutil.copy(p_dst, snap)
        r = reader(snap)
        assert (r.apply(GET, x, y) == v).all(), reader
        r.close()
    o_dst.close(); o_src.close()
