"""GPU (-m gpu): the whole-matrix export (include/smatrix_batch.h smatrix_export / smatrix_export_dev,
SparseMatrix.export / export_dev / to_sparse_coo).  Every case is built through the C ABI next to an oracle; the expected
export comes from the oracle's row list and its rows' non-empty slots."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix
from libsmatrix_amd import _lib
from libsmatrix_amd.stream import Stream

pytestmark = pytest.mark.gpu

SORTED, TABLE = "sorted", "table"


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


def nonempty(kv):
    return kv[(kv[:, 0] != 0) | (kv[:, 1] != 0)]


def oracle_sorted(o):
    """the SORTED export the oracle's contents call for"""
    xs = np.sort(o.list_rows().astype(np.uint32))
    ptr = np.zeros(xs.size + 1, np.uint64)
    parts = []
    for i, x in enumerate(xs.tolist()):
        ne = nonempty(o.row_slots(x))
        ne = ne[np.argsort(ne[:, 0], kind="stable")]
        parts.append(ne)
        ptr[i + 1] = ptr[i] + ne.shape[0]
    pairs = np.concatenate(parts).astype(np.uint32) if parts else np.zeros((0, 2), np.uint32)
    return xs, ptr, pairs


def assert_export_equal(a, b, tag=""):
    for k, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape, (tag, k, u.shape, v.shape)
        assert (u == v).all(), (tag, k)


def check_sorted_shape(rows, ptr, pairs):
    assert ptr[0] == 0 and ptr[-1] == pairs.shape[0]
    assert (np.diff(rows.astype(np.int64)) > 0).all()                 # ascending, unique
    cnt = np.diff(ptr.astype(np.int64))
    assert cnt.sum() == pairs.shape[0]
    if pairs.shape[0] > 1:                                            # columns strictly increase inside every row
        d = np.diff(pairs[:, 0].astype(np.int64))
        first = np.zeros(pairs.shape[0], bool)
        first[ptr[:-1][cnt > 0].astype(np.int64)] = True
        assert (d[~first[1:]] > 0).all()


def check_table_is_getrow(m, rows, ptr, pairs):
    """TABLE order: row for row, byte for byte what getrow_batch returns with exactly room enough"""
    cnt = np.diff(ptr.astype(np.int64)).astype(np.uint64)
    off, gp, gc = m.getrow_batch(rows, caps=cnt)
    assert (off == ptr).all()
    assert (gc.astype(np.uint64) == cnt).all()
    assert gp.tobytes() == pairs.tobytes()


def test_empty_matrix(oracle_mod):
    m = SparseMatrix()
    for order in (SORTED, TABLE):
        rows, ptr, pairs = m.export(order)
        assert rows.size == 0 and pairs.shape == (0, 2) and ptr.tolist() == [0]
    m.close()


def test_quirk_rows_through_the_scalar_abi(oracle_mod):
    m, o = SparseMatrix(), oracle_mod.Oracle()
    ops = [("set", 10, 0, 9), ("incr", 10, 3, 1), ("set", 10, 0, 0),        # Q1: the (0,v) cell, then back to empty
           ("incr", 11, 0, 4), ("incr", 11, 5, 2), ("incr", 11, 21, 6),      # a row whose (0, v) cell rowlen does not count
           ("set", 12, 0, 0),                                                 # Q3: a row with no pairs
           ("set", 13, 5, 0), ("incr", 13, 6, 1),                             # S3: a (5, 0) cell
           ("incr", 0, 1, 1), ("incr", 0xFFFFFFFF, 0xFFFFFFFF, 7), ("set", 0xFFFFFFFF, 2, 0xFFFFFFFF),
           ("incr", 14, 0xFFFFFFFF, 3)]
    for op, x, y, v in ops:
        assert getattr(m, op)(x, y, v) == getattr(o, op)(x, y, v), (op, x, y, v)
    want = oracle_sorted(o)
    got = m.export(SORTED)
    assert_export_equal(got, want, "sorted")
    rows, ptr, pairs = got
    assert {0, 12, 0xFFFFFFFF} <= set(rows.tolist())
    cnt = dict(zip(rows.tolist(), np.diff(ptr.astype(np.int64)).tolist()))
    assert cnt[12] == 0 and o.row_info(12) is not None
    assert cnt[11] == o.rowlen(11) + 1                                  # Q1: (0, v) is a pair, not part of rowlen
    i13 = rows.tolist().index(13)
    assert pairs[ptr[i13]:ptr[i13 + 1]].tolist() == [[5, 0], [6, 1]]   # S3: the (5, 0) cell is a pair
    # TABLE: scalar calls reproduce the reference's layout, so every row is the oracle's non-empty slots in slot order
    t_rows, t_ptr, t_pairs = m.export(TABLE)
    assert sorted(t_rows.tolist()) == rows.tolist()
    for i, x in enumerate(t_rows.tolist()):
        assert (t_pairs[t_ptr[i]:t_ptr[i + 1]] == nonempty(o.row_slots(x))).all(), x
    check_table_is_getrow(m, t_rows, t_ptr, t_pairs)
    m.close(); o.close()


def mixed_stream(seed, n, n_ids, scramble, rows_mod=None):
    gen = Stream("zipf", seed, n_ids, 1.1, scramble)
    x, y = gen.fill(0, n)
    if rows_mod:
        x = (x % rows_mod).astype(np.uint32)
    rng = np.random.default_rng(seed)
    ops = rng.choice([1, 2, 2, 2, 3], size=n // 200000 + 1)
    return x, y, ops


def apply_stream(m, o, x, y, ops, step=200000):
    for k, op in enumerate(ops.tolist()):
        xs, ys = x[k * step:(k + 1) * step], y[k * step:(k + 1) * step]
        if not xs.size:
            break
        v = ((xs ^ ys) % 5 + 1).astype(np.uint32) if op != 1 else (ys % 7).astype(np.uint32)
        m.apply_batch(op, xs, ys, v, results=False)
        o.apply(op, xs, ys, v)


@pytest.mark.parametrize("kind", ["scrambled", "dense"])
def test_differential_stream(oracle_mod, kind):
    m, o = SparseMatrix(), oracle_mod.Oracle()
    if kind == "scrambled":
        x, y, ops = mixed_stream(77, 3000000, 30000, 1)
    else:                                                              # dense ids on few rows: clustered tables
        x, y, ops = mixed_stream(4242, 2000000, 300000, 0, rows_mod=40)
    apply_stream(m, o, x, y, ops)
    if kind == "dense":
        assert m.stats()["clustered_mode"] == 1
    got = m.export(SORTED)
    check_sorted_shape(*got)
    assert_export_equal(got, oracle_sorted(o), kind)
    t1, t2 = m.export(TABLE), m.export(TABLE)
    assert_export_equal(t1, t2, "two TABLE exports")
    assert t1[2].shape == got[2].shape
    check_table_is_getrow(m, *t1)
    assert_export_equal(m.export(SORTED), got, "two SORTED exports")
    m.close(); o.close()


def test_batches_and_scalar_calls_export_the_same(oracle_mod):
    x, y, _ = mixed_stream(5, 60000, 2000, 1)
    v = ((x ^ y) % 3 + 1).astype(np.uint32)
    a, b = SparseMatrix(), SparseMatrix()
    for k in range(0, x.size, 20000):
        a.incr_batch(x[k:k + 20000], y[k:k + 20000], v[k:k + 20000])
    for xi, yi, vi in zip(x.tolist(), y.tolist(), v.tolist()):
        b.incr(xi, yi, vi)
    sa, sb = a.export(SORTED), b.export(SORTED)
    assert_export_equal(sa, sb, "batch vs scalar")
    for m, s in ((a, sa), (b, sb)):
        r, p, q = m.export(TABLE)                                     # the same cells in each matrix's own layout
        assert sorted(r.tolist()) == s[0].tolist() and q.shape == s[2].shape
    a.close(); b.close()


def test_big_row_among_small_rows(oracle_mod):
    m, o = SparseMatrix(), oracle_mod.Oracle()
    ncol = (1 << 20) + 3
    ys = np.arange(1, ncol + 1, dtype=np.uint32)
    xs = np.full(ncol, 7, np.uint32)
    rng = np.random.default_rng(3)
    sx = rng.integers(100, 5100, 200000, dtype=np.uint32)
    sy = rng.integers(0, 1 << 31, 200000, dtype=np.uint32)
    for xx, yy in ((xs, ys), (sx, sy)):
        v = (yy % 9 + 1).astype(np.uint32)
        m.incr_batch(xx, yy, v)
        o.apply(2, xx, yy, v)
    size, used = m.row_info(7)
    assert size >= 1 << 21 and used == ncol                            # sub-counters and an at-home bitmap sit behind its cells
    got = m.export(SORTED)
    check_sorted_shape(*got)
    assert_export_equal(got, oracle_sorted(o), "big row")
    rows, ptr, pairs = got
    i = int(np.searchsorted(rows, 7))
    assert int(ptr[i + 1] - ptr[i]) == ncol
    assert (pairs[ptr[i]:ptr[i + 1], 0] == ys).all()
    t = m.export(TABLE)
    check_table_is_getrow(m, *t)
    j = t[0].tolist().index(7)
    assert (t[2][t[1][j]:t[1][j + 1]] == nonempty(m.row_slots(7))).all()
    m.close(); o.close()


def test_scalar_writes_in_the_host_mirror_show(oracle_mod):
    m, o = SparseMatrix(), oracle_mod.Oracle()
    x = np.arange(50, dtype=np.uint32)
    m.incr_batch(x, x + 1, np.ones(50, np.uint32)); o.apply(2, x, x + 1, np.ones(50, np.uint32))
    for k in range(50):                                                # each cell touched twice, nothing in between
        for _ in range(2):
            assert m.incr(k, k + 1, 3) == o.incr(k, k + 1, 3)
    assert m.set(3, 4, 99) == o.set(3, 4, 99)
    assert_export_equal(m.export(SORTED), oracle_sorted(o), "mirror")
    m.close(); o.close()


def test_file_mode_round_trip(oracle_mod, tmp_path):
    fn = str(tmp_path / "export.smx")
    x, y, _ = mixed_stream(11, 400000, 20000, 1)
    m = SparseMatrix(fn)
    m.incr_batch(x, y, ((x + y) % 4 + 1).astype(np.uint32))            # no zero values: the loader keeps every cell
    before = m.export(SORTED)
    m.close()
    m = SparseMatrix(fn)
    assert_export_equal(m.export(SORTED), before, "reopened")
    m.close()


def test_capacity_too_small_and_size_query(oracle_mod):
    m = SparseMatrix()
    x, y, _ = mixed_stream(21, 100000, 5000, 1)
    m.incr_batch(x, y, np.ones(x.size, np.uint32))
    lib, h = _lib.load(), m._h
    n, z = C.c_uint64(0), C.c_uint64(0)
    assert lib.smatrix_export(h, 1, 0, 0, None, None, None, C.byref(n), C.byref(z)) == 0
    rows_w, ptr_w, pairs_w = m.export(SORTED)
    assert (n.value, z.value) == (rows_w.size, pairs_w.shape[0])
    for cr, cz in ((n.value - 1, z.value), (n.value, z.value - 1)):
        rows = np.full(n.value + 4, 0xA5A5A5A5, np.uint32)
        ptr = np.full(n.value + 5, 0x5A5A5A5A5A5A5A5A, np.uint64)
        pairs = np.full(2 * z.value + 8, 0xC3C3C3C3, np.uint32)
        n2, z2 = C.c_uint64(0), C.c_uint64(0)
        rc = lib.smatrix_export(h, 0, cr, cz, rows.ctypes.data_as(_lib.u32p), ptr.ctypes.data_as(_lib.u64p),
                                pairs.ctypes.data_as(_lib.u32p), C.byref(n2), C.byref(z2))
        assert rc == 1 and (n2.value, z2.value) == (n.value, z.value)
        assert (rows == 0xA5A5A5A5).all() and (ptr == 0x5A5A5A5A5A5A5A5A).all() and (pairs == 0xC3C3C3C3).all()
    assert lib.smatrix_export(h, 2, 0, 0, None, None, None, C.byref(n), C.byref(z)) == -1
    assert lib.smatrix_export_dev(h, 0, 0, 0, None, None, None, C.byref(n), C.byref(z), None) == 0
    assert (n.value, z.value) == (rows_w.size, pairs_w.shape[0])
    m.close()


def test_export_dev_and_sparse_coo(oracle_mod):
    import torch
    m, o = SparseMatrix(), oracle_mod.Oracle()
    x, y, ops = mixed_stream(31, 600000, 20000, 0)                   # unscrambled ids: a shape torch can hold
    apply_stream(m, o, x, y, ops)
    want = m.export(SORTED)
    assert_export_equal(want, oracle_sorted(o), "dense ids")
    s = torch.cuda.Stream()
    rows, ptr, pairs = m.export_dev(SORTED, stream=s)
    assert rows.dtype == torch.int32 and ptr.dtype == torch.int64 and pairs.dtype == torch.int32
    got = (rows.cpu().numpy().view(np.uint32), ptr.cpu().numpy().astype(np.uint64), pairs.cpu().numpy().view(np.uint32))
    assert_export_equal(got, want, "export_dev")
    t = m.export_dev(TABLE, stream=s)
    assert_export_equal((t[0].cpu().numpy().view(np.uint32), t[1].cpu().numpy().astype(np.uint64), t[2].cpu().numpy().view(np.uint32)),
                        m.export(TABLE), "export_dev table")
    coo = m.to_sparse_coo()
    r, p, q = want
    assert coo.is_coalesced() and coo.dtype == torch.int64
    assert tuple(coo.shape) == (int(r.max()) + 1, int(q[:, 0].max()) + 1)
    idx, val = coo.indices().cpu().numpy(), coo.values().cpu().numpy()
    assert (idx[0] == np.repeat(r.astype(np.int64), np.diff(p.astype(np.int64)))).all()
    assert (idx[1] == q[:, 0].astype(np.int64)).all() and (val == q[:, 1].astype(np.int64)).all()
    big = (int(r.max()) + 1, int(q[:, 0].max()) + 6)
    assert tuple(m.to_sparse_coo(size=big).shape) == big
    with pytest.raises(ValueError):
        m.to_sparse_coo(size=(1 << 32, 1 << 32))
    m.close(); o.close()


def test_export_changes_nothing(oracle_mod):
    m, o = SparseMatrix(), oracle_mod.Oracle()
    x, y, ops = mixed_stream(41, 800000, 20000, 1)
    apply_stream(m, o, x, y, ops)
    m.export(TABLE)                                                    # (nothing waits in the host mirror from here on)
    st = m.stats()
    for order in (SORTED, TABLE, SORTED):
        m.export(order)
    assert m.stats() == st
    x2, y2, _ = mixed_stream(42, 400000, 20000, 1)
    v = ((x2 + y2) % 3 + 1).astype(np.uint32)
    m.incr_batch(x2, y2, v); o.apply(2, x2, y2, v)
    assert (m.get_batch(x2, y2) == o.apply(0, x2, y2)).all()
    assert (m.get_batch(x, y) == o.apply(0, x, y)).all()
    xs = np.unique(x2)[:2000]
    _, gp, gc = m.getrow_batch(xs)
    assert int(gc.astype(np.int64).sum()) == sum(nonempty(o.row_slots(int(r))).shape[0] for r in xs.tolist())
    assert_export_equal(m.export(SORTED), oracle_sorted(o), "after")
    m.close(); o.close()
