"""GPU (-m gpu): the whole-matrix export and getrow_batch at the edges their kernels have (kernels/export.hpp, smx_export.inc,
kernels/rows.hpp), against the host model of tests/export_helpers.py: the sort tiers at 512 / 4096 pairs, the LDS sorts' pad,
the radix sort's four passes, its tiles and segments, the scans' tiles and the 256-tile carry, the walkers' handover at 8192
cells and their cut at 65536, the scratch one handle keeps between calls, and the `rank < cap` guards of the row walkers.

Every comparison is exact and over every entry.  Every matrix is built once (module fixtures) and every export is made once;
the tests of one matrix look at the same arrays."""
import ctypes as C
import time

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix
from libsmatrix_amd import _lib
from tests import export_helpers as H

pytestmark = pytest.mark.gpu

SORTED, TABLE = "sorted", "table"
SENTINEL = 0xC3C3C3C3
ABSENT = 0xDEADBEEF                                                    # a row id no matrix of this file holds
GAP, MARGIN = 2, 64                                                    # pairs of room nobody may write: behind every request, behind the batch


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


def assert_export_equal(got, want, tag):
    for name, g, w in zip(("rows", "row_ptr", "pairs"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.size:
            bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))
            assert bad.size == 0, (tag, name, "%d entries differ, the first at %d" % (bad.size, bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist())


def check_sorted_shape(rows, ptr, pairs):
    assert ptr[0] == 0 and int(ptr[-1]) == pairs.shape[0]
    assert (np.diff(rows.astype(np.int64)) > 0).all()                  # strictly ascending
    cnt = np.diff(ptr.astype(np.int64))
    assert (cnt >= 0).all()
    if pairs.shape[0] > 1:                                             # columns strictly increase inside every row
        first = np.zeros(pairs.shape[0], bool)
        first[ptr[:-1][cnt > 0].astype(np.int64)] = True
        assert (np.diff(pairs[:, 0].astype(np.int64))[~first[1:]] > 0).all()


def check_table(m, table, model):
    """a TABLE export: the same row set as SORTED; row for row, byte for byte what getrow_batch returns with exactly room
    enough; and, put into SORTED order on the host, the model"""
    rows, ptr, pairs = table
    assert np.unique(rows).size == rows.size and (np.sort(rows) == model[0]).all()
    assert ptr[0] == 0 and int(ptr[-1]) == pairs.shape[0] and (np.diff(ptr.astype(np.int64)) >= 0).all()
    cnt = np.diff(ptr.astype(np.int64)).astype(np.uint64)
    off, gp, gc = m.getrow_batch(rows, caps=cnt)
    assert (off == ptr).all() and (gc.astype(np.uint64) == cnt).all()
    assert gp.tobytes() == pairs.tobytes()
    assert_export_equal(H.table_as_sorted(*table), model, "table, sorted on the host")


def dev_export(m, order, stream):
    r, p, q = m.export_dev(order, stream=stream)
    return r.cpu().numpy().view(np.uint32), p.cpu().numpy().astype(np.uint64), q.cpu().numpy().view(np.uint32)


# ---- tier edges ---------------------------------------------------------------------------------------------------------------

TIER_COUNTS = [1, 2, 3, 63, 64, 65, H.EX_LDS_SMALL - 1, H.EX_LDS_SMALL, H.EX_LDS_SMALL + 1, 1023, 1024, 1025,
               H.EX_LDS_MID - 1, H.EX_LDS_MID, H.EX_LDS_MID + 1,
               H.EX_LDS_MID + 2,                                        # 4097 keys fill 8192 cells; the next key makes it 16384: the walkers' handover
               H.GETROW_WAVE_MAX - 1, H.GETROW_WAVE_MAX, H.GETROW_WAVE_MAX + 1]
TIER_FIRST = (1 << 31) - 20                                             # adjacent ids, across the sign bit


@pytest.fixture(scope="module")
def tiers():
    counts = [c for c in TIER_COUNTS for _ in range(3)]
    x, y, v = H.rows_with_pair_counts(counts, 101, first_row=TIER_FIRST)
    start = np.concatenate([[0], np.cumsum(counts)])
    ones = []
    for c in (H.EX_LDS_SMALL - 1, H.EX_LDS_MID - 1, H.GETROW_WAVE_MAX + 1):   # one row of every sort tier, the first two with one pad
        i = int(start[counts.index(c) + 1])                            # the second row of that count: its first pair becomes all ones
        assert H.M32 not in y[start[counts.index(c) + 1]:start[counts.index(c) + 2]]
        y[i] = v[i] = H.M32
        ones.append(int(x[i]))
    nx = TIER_FIRST + len(counts)
    ex, ey, ev = H.rows_with_pair_counts([5, 4], 102, first_row=nx)    # two more rows for the scalar calls
    x, y, v = np.concatenate([x, ex]), np.concatenate([y, ey]), np.concatenate([v, ev])
    scalars = [(nx, 0, 4242), (nx + 1, 77, 0), (nx + 2, 0, 0)]         # a (0, v) pair; a (y, 0) pair; a row with no pairs (Q3)
    perm = np.random.default_rng(103).permutation(x.size)              # the rows' ops interleaved in the batch
    m = SparseMatrix()
    H.fill(m, x[perm], y[perm], v[perm], scalars)
    out = {"m": m, "counts": counts, "ones": ones, "extra": nx, "model": H.sorted_model(x, y, v, scalars),
           "sorted": m.export(SORTED), "table": m.export(TABLE)}
    yield out
    m.close()


def test_tier_edges_sorted(tiers):
    rows, ptr, pairs = tiers["sorted"]
    check_sorted_shape(rows, ptr, pairs)
    assert_export_equal(tiers["sorted"], tiers["model"], "tier edges")
    cnt = dict(zip(rows.tolist(), np.diff(ptr.astype(np.int64)).tolist()))
    for i, c in enumerate(tiers["counts"]):                            # the shape this test is about, not the code under test
        assert cnt[TIER_FIRST + i] == c
    nx = tiers["extra"]
    assert (cnt[nx], cnt[nx + 1], cnt[nx + 2]) == (6, 5, 0)
    for x in tiers["ones"]:
        i = int(np.searchsorted(rows, x))
        assert pairs[int(ptr[i + 1]) - 1].tolist() == [H.M32, H.M32]    # the pair that is the pad's bits: last in its row, and there once
        assert int(((pairs[:, 0] == H.M32) & (pairs[:, 1] == H.M32)).sum()) == len(tiers["ones"])
    i = int(np.searchsorted(rows, nx))
    assert pairs[int(ptr[i])].tolist() == [0, 4242]


def test_tier_edges_tables_stand_on_the_walkers_handover(tiers):
    m = tiers["m"]
    for i, c in enumerate(tiers["counts"]):
        assert m.row_info(TIER_FIRST + i) == (H.table_size_for(c), c), (i, c)
    sizes = {H.table_size_for(c) for c in tiers["counts"]}
    assert {H.GETROW_WAVE_MAX, 2 * H.GETROW_WAVE_MAX} <= sizes


def test_tier_edges_table(tiers):
    check_table(tiers["m"], tiers["table"], tiers["model"])
    rows, ptr, pairs = tiers["table"]
    m = tiers["m"]
    for i in np.flatnonzero(np.isin(rows, np.array(tiers["ones"] + [tiers["extra"] + k for k in range(3)], np.uint32))).tolist():
        assert (pairs[int(ptr[i]):int(ptr[i + 1])] == H.table_row_model(m.row_slots(int(rows[i])))).all(), int(rows[i])


def test_flavours_export_dev_on_a_stream(tiers):
    import torch
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    assert_export_equal(dev_export(tiers["m"], SORTED, s), tiers["sorted"], "export_dev sorted")
    assert_export_equal(dev_export(tiers["m"], TABLE, s), tiers["table"], "export_dev table")


def test_flavours_import_csr_round_trip(tiers):
    b = SparseMatrix()
    n_ops = b.import_csr(*tiers["sorted"])
    assert n_ops == tiers["sorted"][2].shape[0]
    got = b.export(SORTED)
    b.close()
    want = tiers["model"]
    empty = np.diff(want[1].astype(np.int64)) == 0                     # a CSR row without pairs has no op: the Q3 row does not come over
    assert empty.sum() == 1
    assert_export_equal(got, (want[0][~empty], np.delete(want[1], np.flatnonzero(empty) + 1), want[2]), "import_csr(export)")


# ---- the radix sort's passes ----------------------------------------------------------------------------------------------------

def test_radix_digits():
    """four rows just past the LDS tier whose columns differ in two bytes only -- (0,1), (1,2), (2,3), (3,0) --, so that of the
    four passes two decide the order and the other two see one digit and must keep what the earlier ones did; a fifth row
    with the top bit set in every column"""
    n = H.EX_LDS_MID + 1
    rng = np.random.default_rng(7)
    cols = [H.columns_varying_in_bytes(n, b0, b1) for b0, b1 in ((0, 1), (1, 2), (2, 3), (3, 0))]
    cols.append(H.distinct_columns(n, rng, lo=1 << 31))
    x = np.repeat(np.arange(300, 305, dtype=np.uint32), n)
    y = np.concatenate(cols)
    v = H.pair_value(x, y)
    perm = rng.permutation(x.size)
    m = SparseMatrix()
    H.fill(m, x[perm], y[perm], v[perm])
    got = m.export(SORTED)
    m.close()
    check_sorted_shape(*got)
    assert_export_equal(got, H.sorted_model(x, y, v), "radix digits")
    assert got[2].shape[0] == 5 * n and (got[2][4 * n:, 0] >= 1 << 31).all()


# ---- segments and tiles -----------------------------------------------------------------------------------------------------------

LONG = [H.EX_TILE + 1, 2 * H.EX_TILE, 2 * H.EX_TILE + 1, 3 * H.EX_TILE + 1]   # 2, 2, 3 and 4 tiles


ASCENDING = {1: [0], 2: [0, 3], 3: [1, 2, 3], 5: [0, 0, 1, 2, 3]}             # indices into LONG
MIXED = {1: [2], 2: [2, 1], 3: [2, 3, 1], 5: [2, 0, 3, 1, 0]}


def long_rows(n_long, order):
    if order == "mixed":
        return [LONG[i] for i in MIXED[n_long]]
    lens = [LONG[i] for i in ASCENDING[n_long]]
    if order == "descending":
        lens = [LONG[3]] if n_long == 1 else lens[::-1]
    return lens


@pytest.mark.parametrize("order", ["ascending", "descending", "mixed"])
@pytest.mark.parametrize("n_long", [1, 2, 3, 5])
def test_segments_and_tiles(n_long, order):
    lens = long_rows(n_long, order)
    assert len(lens) == n_long and set(lens) <= set(LONG)
    counts = [3]
    for k, c in enumerate(lens):                                       # short rows of every other tier between the long ones
        counts += [c, (1, 600, 2, 70, 513)[k]]
    x, y, v = H.rows_with_pair_counts(counts, 1000 + 10 * n_long + len(order), first_row=40)
    m = SparseMatrix()
    H.fill(m, x, y, v)
    got = m.export(SORTED)
    m.close()
    check_sorted_shape(*got)
    assert np.diff(got[1].astype(np.int64)).tolist() == counts
    assert_export_equal(got, H.sorted_model(x, y, v), (n_long, order))


# ---- the row list ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, H.EX_TILE - 1, H.EX_TILE, H.EX_TILE + 1, 40000])
def test_row_list(n):
    x = H.row_list_ids(n, 50 + n)
    y = (x % np.uint32(5) + np.uint32(1)).astype(np.uint32)
    v = H.pair_value(x, y)
    m = SparseMatrix()
    H.fill(m, x, y, v)
    got, table = m.export(SORTED), m.export(TABLE)
    model = H.sorted_model(x, y, v)
    check_sorted_shape(*got)
    assert_export_equal(got, model, ("row list", n))
    assert got[0].size == n and (got[1] == np.arange(n + 1, dtype=np.uint64)).all()
    assert H.M32 in got[0] and (n < 2 or got[0][0] == 0)
    check_table(m, table, model)
    m.close()


# ---- the scan's carry; scratch that one handle keeps between calls ------------------------------------------------------------

N_CARRY = (H.SCAN_PART_STEP * H.EX_TILE) + H.EX_TILE + 1               # 258 tiles of counts: two of them in k_ex_scan_part's second step


@pytest.fixture(scope="module")
def carry_data():
    assert N_CARRY == (1 << 20) + 4097
    x = H.row_list_ids(N_CARRY, 9)
    y = (x >> np.uint32(7) | np.uint32(1)).astype(np.uint32)
    v = H.pair_value(x, y)
    return x, y, v, H.sorted_model(x, y, v)


def test_scan_carry_table_on_a_fresh_handle(carry_data):
    """TABLE alone: no sort stands between the count scan and row_ptr, and none reads a row_ptr that a lost carry broke"""
    x, y, v, model = carry_data
    m = SparseMatrix()
    H.fill(m, x, y, v)
    table = m.export(TABLE)
    assert (table[1] == np.arange(N_CARRY + 1, dtype=np.uint64)).all()
    check_table(m, table, model)
    m.close()


@pytest.fixture(scope="module")
def carry(carry_data):
    """2^20 + 4097 one-pair rows; its SORTED export, then TABLE on the same handle"""
    x, y, v, model = carry_data
    m = SparseMatrix()
    t0 = time.perf_counter()
    H.fill(m, x, y, v)
    t1 = time.perf_counter()
    s = m.export(SORTED)
    t2 = time.perf_counter()
    t = m.export(TABLE)
    t3 = time.perf_counter()
    print("\nscan carry, %d one-pair rows: fill %.1f ms, SORTED export %.1f ms, TABLE export %.1f ms"
          % (N_CARRY, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)))
    yield {"m": m, "model": model, "sorted": s, "table": t}
    m.close()


def test_scan_carry_sorted(carry):
    rows, ptr, pairs = carry["sorted"]
    assert rows.size == N_CARRY
    assert (ptr == np.arange(N_CARRY + 1, dtype=np.uint64)).all()
    check_sorted_shape(rows, ptr, pairs)
    assert_export_equal(carry["sorted"], carry["model"], "scan carry")


def test_scratch_reuse_table_after_sorted(carry):
    """the SORTED call's sorts left their own tile sums in the scan scratch; the TABLE call on the same handle starts over"""
    rows, ptr, pairs = carry["table"]
    assert (ptr == np.arange(N_CARRY + 1, dtype=np.uint64)).all()
    check_table(carry["m"], carry["table"], carry["model"])


def test_scratch_reuse_after_trim_and_one_more_row():
    """a matrix whose export needs more than 64 MiB of pair scratch (released when the call ends), exported, then one more row,
    exported again: both equal their models"""
    n = (8 << 20) // 2 + 70001                                         # two long rows: 2 n pairs of 8 bytes > 64 MiB
    rng = np.random.default_rng(21)
    ys = [np.unique(rng.integers(1, 1 << 32, n + n // 8, dtype=np.uint64).astype(np.uint32))[:n] for _ in range(2)]
    assert all(c.size == n for c in ys)
    sx, sy, sv = H.rows_with_pair_counts([1, 600, 4097, 2, 8193], 22, first_row=10)
    x = np.concatenate([np.full(n, 5, np.uint32), np.full(n, 6, np.uint32), sx])
    y = np.concatenate(ys + [sy])
    v = H.pair_value(x, y)
    model = H.sorted_model(x, y, v)
    assert model[2].shape[0] * 8 > 64 << 20
    m = SparseMatrix()
    H.fill(m, x, y, v)
    first = m.export(SORTED)
    assert m.incr(H.M32 - 1, 9, 31) == 31
    second = m.export(SORTED)
    m.close()
    assert_export_equal(first, model, "big matrix")
    assert_export_equal(second, H.append_row(model, H.M32 - 1, [[9, 31]]), "big matrix and one more row")


# ---- getrow_batch under caps ------------------------------------------------------------------------------------------------------

CAP_SIZES = [16, 128, 256, H.GETROW_WAVE_MAX, 2 * H.GETROW_WAVE_MAX, H.GETROW_SEG, 2 * H.GETROW_SEG]
CAP_FIRST = 7000


@pytest.fixture(scope="module")
def caprows():
    """rows whose tables have CAP_SIZES cells, half full, columns over the whole range"""
    counts = [s // 2 for s in CAP_SIZES]
    x, y, v = H.rows_with_pair_counts(counts, 31, first_row=CAP_FIRST)
    m = SparseMatrix()
    H.fill(m, x, y, v)
    for i, s in enumerate(CAP_SIZES):
        assert m.row_info(CAP_FIRST + i) == (s, s // 2)
    assert m.row_info(ABSENT) is None
    slots = {CAP_FIRST + i: m.row_slots(CAP_FIRST + i) for i in range(len(CAP_SIZES))}
    for i, c in enumerate(counts):
        assert H.table_row_model(slots[CAP_FIRST + i]).shape[0] == c
    yield {"m": m, "slots": slots, "counts": counts}
    m.close()


def cap_batch(requests):
    """(x, cap) requests -> the batch's xs and caps: behind every request GAP pairs of room that belong to a row that does
    not exist, and MARGIN more of them as the batch's last entry"""
    xs = np.full(2 * len(requests) + 1, ABSENT, np.uint32)
    caps = np.full(2 * len(requests) + 1, GAP, np.uint64)
    xs[0:-1:2] = [r[0] for r in requests]
    caps[0:-1:2] = [r[1] for r in requests]
    caps[-1] = MARGIN
    return xs, caps


def run_getrow_dev(m, xs, offsets, n_words):
    import torch
    dx = torch.from_numpy(xs.view(np.int32)).cuda()
    doff = torch.from_numpy(offsets.view(np.int64)).cuda()
    dret = torch.full((n_words,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    dcnt = torch.full((xs.size,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.getrow_batch_dev(xs.size, dx.data_ptr(), doff.data_ptr(), dret.data_ptr(), dcnt.data_ptr())
    torch.cuda.synchronize()
    return dret.cpu().numpy().view(np.uint32), dcnt.cpu().numpy().view(np.uint32)


def check_whole_buffer(got, want, offsets, tag):
    bad = np.flatnonzero(got != want)
    if bad.size:
        r = int(np.searchsorted(offsets, bad[0] // 2, side="right")) - 1
        raise AssertionError((tag, "%d words differ; the first is word %d, in the room of entry %d" % (bad.size, bad[0], r),
                              hex(int(got[bad[0]])), hex(int(want[bad[0]]))))


def edge_requests(c):
    reqs = []
    for i, n in enumerate(c["counts"]):
        for _ in range(3 if CAP_SIZES[i] == 256 else 1):               # one row three times over
            reqs += [(CAP_FIRST + i, cap) for cap in H.edge_caps(n)]
    return reqs


def test_getrow_caps_dev(caprows):
    """the device flavour writes into the caller's own array: every word that is not a pair of the first min(cap, c) stays as
    it was -- the rest of the row's room, the gaps between the requests, the margin behind the batch"""
    xs, caps = cap_batch(edge_requests(caprows))
    offsets, want, counts = H.getrow_model(caprows["slots"], xs, caps, SENTINEL, MARGIN)
    got, cnt = run_getrow_dev(caprows["m"], xs, offsets, want.size)
    real = xs != ABSENT
    have = np.array([caprows["counts"][x - CAP_FIRST] for x in xs[real].tolist()], np.uint64)
    assert (counts[real] == np.minimum(caps[real], have)).all() and not counts[~real].any()
    assert (cnt == counts).all(), np.flatnonzero(cnt != counts)[:8]
    check_whole_buffer(got, want, offsets, "getrow_batch_dev")


def test_getrow_caps_host(caprows):
    """the host flavour stages the pairs in a device buffer of its own and copies the batch's whole room back: counts, every
    row's first min(cap, c) pairs, and the words behind the batch's room, which it must not touch (what lies between a row's
    count and its cap is not defined by include/smatrix_batch.h in this flavour; test_getrow_caps_dev holds the kernels to it)"""
    xs, caps = cap_batch(edge_requests(caprows))
    offsets, want, counts = H.getrow_model(caprows["slots"], xs, caps, SENTINEL, MARGIN)
    got = np.full(want.size, SENTINEL, np.uint32)
    cnt = np.full(xs.size, 0xFFFFFFFF, np.uint32)
    rc = _lib.load().smatrix_getrow_batch(caprows["m"]._h, xs.size, xs.ctypes.data_as(_lib.u32p), offsets.ctypes.data_as(_lib.u64p),
                                          got.ctypes.data_as(_lib.u32p), cnt.ctypes.data_as(_lib.u32p))
    assert rc == 0
    assert (cnt == counts).all(), np.flatnonzero(cnt != counts)[:8]
    defined = np.zeros(want.size, bool)
    defined[2 * int(offsets[-1]):] = True
    word = np.arange(want.size, dtype=np.int64)
    room = np.searchsorted(offsets, word[:2 * int(offsets[-1])] // 2, side="right") - 1
    defined[:2 * int(offsets[-1])] = word[:2 * int(offsets[-1])] < 2 * (offsets[room].astype(np.int64) + counts[room])
    assert defined.sum() == 2 * (int(counts.sum()) + MARGIN)
    check_whole_buffer(np.where(defined, got, want), want, offsets, "getrow_batch")


def test_getrow_caps_two_rows_in_flight(caprows):
    """a batch of more than 65536 entries: k_getrow's waves then hold two rows each, and where both have at most 256 cells
    they take its straight-line path, which has its own copy of the cap"""
    small = [i for i, s in enumerate(CAP_SIZES) if s <= 256]
    reqs = []
    for i in small:
        reqs += [(CAP_FIRST + i, cap) for cap in H.edge_caps(caprows["counts"][i]) if cap <= caprows["counts"][i] + 1]
    reqs = (reqs * (34816 // len(reqs) + 1))[:34816]
    xs, caps = cap_batch(reqs)
    assert xs.size > 65536 and xs[0] != ABSENT and xs[65536] != ABSENT  # entries r and r + 65536 share a wave: both are rows
    offsets, want, counts = H.getrow_model(caprows["slots"], xs, caps, SENTINEL, MARGIN)
    got, cnt = run_getrow_dev(caprows["m"], xs, offsets, want.size)
    assert (cnt == counts).all(), np.flatnonzero(cnt != counts)[:8]
    check_whole_buffer(got, want, offsets, "getrow_batch_dev, two rows in flight")
