"""A host model of the whole-matrix export and of getrow_batch (include/smatrix_batch.h smatrix_export /
smatrix_getrow_batch), numpy only: no oracle and no library call in it.

The SORTED export of a matrix depends only on its contents, so for a matrix that was filled with UNIQUE (x, y, v) triples the
model is those triples in another order: np.lexsort((y, x)).  TABLE order and getrow_batch depend on where the cells lie; the
model takes the row's slots as the caller read them (row_slots) and says which of them a row walk returns, in which order, under
which cap.

The constants are the edges of kernels/export.hpp and kernels/rows.hpp, restated: tests/test_export_model.py holds them to the
`constexpr` lines of those files, so that a test which claims to stand on an edge says so when the edge moves.  The builders
at the end make the rows and the ids that stand on those edges.
"""
import numpy as np

M32 = 0xFFFFFFFF

# kernels/export.hpp
EX_THREADS = 256
EX_PER_THREAD = 16
EX_TILE = EX_THREADS * EX_PER_THREAD         # entries per tile of the scans and of the segmented radix sort
EX_LDS_SMALL = 512                           # rows of 2 .. 512 pairs: sorted in LDS by a 64-lane workgroup
EX_LDS_MID = 4096                            # .. 4096 pairs: by a 256-lane workgroup; longer rows: the radix sort
# kernels/rows.hpp
GETROW_WAVE_MAX = 8192                       # cells a wave walks; longer rows go to the workgroup kernels
GETROW_SEG = 32768                           # cells per segment of a cut row (rows of 2 * GETROW_SEG cells and more are cut)
WAVE_STEP = 128                              # cells a wave compacts per step (two per lane)
SCAN_PART_STEP = EX_THREADS                  # tile sums k_ex_scan_part takes per step, with a carry between the steps
ROW_FIRST_SIZE = 16                          # a new row's table (the reference's SMATRIX_RMAP_INITIAL_SIZE)

SOURCE_CONSTANTS = {                         # file under libsmatrix_amd/csrc/kernels -> {constexpr name: value here}
    "export.hpp": {"EX_THREADS": EX_THREADS, "EX_PER_THREAD": EX_PER_THREAD, "EX_LDS_SMALL": EX_LDS_SMALL, "EX_LDS_MID": EX_LDS_MID},
    "rows.hpp": {"GETROW_WAVE_MAX": GETROW_WAVE_MAX, "GETROW_SEG": GETROW_SEG},
}


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def pair_value(x, y):
    """the value of cell (x, y) in every matrix the builders make: a fixed hash of both ids, never 0, so that a pair which lands
    in another row or at another column's place does not compare equal"""
    x, y = np.asarray(x).astype(np.uint64), np.asarray(y).astype(np.uint64)
    h = (x * np.uint64(0x9E3779B1) + y * np.uint64(0x85EBCA77) + np.uint64(0x27D4EB2F)) & np.uint64(M32)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(M32)
    h ^= h >> np.uint64(12)
    return np.where(h == 0, np.uint64(1), h).astype(np.uint32)


def table_size_for(n_keys):
    """cells of a row that took n_keys distinct columns != 0 one after the other: the table doubles when an insert finds
    used > size / 2 (src/smatrix.c:346), so size S holds up to S / 2 + 1 keys"""
    s = ROW_FIRST_SIZE
    while n_keys > s // 2 + 1:
        s *= 2
    return s


# ---- the matrix of a case: unique triples for one incr_batch, then scalar set calls ------------------------------------------

def fill(m, x, y, v, scalars=()):
    """into an EMPTY matrix (a SparseMatrix, or an oracle with .apply): the triples as one incr batch, then set(x, y, v) for
    every scalar"""
    x, y, v = _u32(x), _u32(y), _u32(v)
    if x.size:
        if hasattr(m, "incr_batch"):
            m.incr_batch(x, y, v)
        else:
            m.apply(2, x, y, v)
    for sx, sy, sv in scalars:
        m.set(int(sx), int(sy), int(sv))


def sorted_model(x, y, v, scalars=()):
    """the SORTED export of fill(empty, x, y, v, scalars): (rows uint32[n], row_ptr uint64[n + 1], pairs uint32[nnz, 2]).
    Batch triples: y >= 1, v != 0.  A scalar (x, y, v) names a cell of its own: a pair unless it is (y, v) == (0, 0), which
    only makes the row exist (quirk Q3); (y != 0, 0) and (0, v != 0) are pairs."""
    x, y, v = _u32(x), _u32(y), _u32(v)
    assert x.shape == y.shape == v.shape and x.ndim == 1
    assert (y >= 1).all() and (v != 0).all(), "batch triples have y >= 1 and v != 0; everything else goes in through set"
    sc = np.array(list(scalars), dtype=np.uint64).reshape(-1, 3)
    is_pair = (sc[:, 1] != 0) | (sc[:, 2] != 0)
    ax = np.concatenate([x, sc[is_pair, 0].astype(np.uint32)])
    ay = np.concatenate([y, sc[is_pair, 1].astype(np.uint32)])
    av = np.concatenate([v, sc[is_pair, 2].astype(np.uint32)])
    order = np.lexsort((ay, ax))
    ax, ay, av = ax[order], ay[order], av[order]
    key = ax.astype(np.uint64) << np.uint64(32) | ay
    assert (key[1:] != key[:-1]).all(), "cells must be unique: the model has no arithmetic in it"
    rows = np.unique(np.concatenate([ax, sc[:, 0].astype(np.uint32)]))
    counts = np.zeros(rows.size, np.uint64)
    if ax.size:
        ux, c = np.unique(ax, return_counts=True)
        counts[np.searchsorted(rows, ux)] = c.astype(np.uint64)
    row_ptr = np.zeros(rows.size + 1, np.uint64)
    np.cumsum(counts, out=row_ptr[1:])
    return rows, row_ptr, np.stack([ay, av], axis=1).astype(np.uint32).reshape(-1, 2)


def append_row(model, x, pairs):
    """the SORTED model with one more row whose id is above every other"""
    rows, row_ptr, old = model
    assert rows.size == 0 or int(x) > int(rows[-1])
    pairs = _u32(pairs).reshape(-1, 2)
    pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]
    return (np.append(rows, np.uint32(x)), np.append(row_ptr, np.uint64(int(row_ptr[-1]) + pairs.shape[0])),
            np.concatenate([old, pairs]))


# ---- TABLE order and getrow_batch ---------------------------------------------------------------------------------------------

def nonempty(slots):
    slots = np.asarray(slots).reshape(-1, 2)
    return slots[(slots[:, 0] != 0) | (slots[:, 1] != 0)]


def table_row_model(slots, cap=None):
    """what a row walk returns of a row whose cells are `slots` ((size, 2), as row_slots reads them; None: no such row): the
    first min(cap, pairs) non-empty cells, in slot order"""
    if slots is None:
        return np.zeros((0, 2), np.uint32)
    ne = nonempty(slots).astype(np.uint32)
    return ne if cap is None else ne[:int(cap)]


def table_as_sorted(rows, row_ptr, pairs):
    """a TABLE export put into SORTED order on the host: rows by id, every row's pairs by column.  Equal to the SORTED model
    exactly when every pair sits in its own row's range"""
    rows, pairs = _u32(rows), _u32(pairs).reshape(-1, 2)
    cnt = np.diff(row_ptr.astype(np.int64))
    assert row_ptr[0] == 0 and (cnt >= 0).all() and int(row_ptr[-1]) == pairs.shape[0]
    owner = np.repeat(rows, cnt)
    order = np.lexsort((pairs[:, 0], owner))
    by_id = np.argsort(rows, kind="stable")
    out_ptr = np.zeros(rows.size + 1, np.uint64)
    np.cumsum(cnt[by_id].astype(np.uint64), out=out_ptr[1:])
    return rows[by_id], out_ptr, pairs[order]


def getrow_model(slots_of, xs, caps, sentinel, margin):
    """getrow_batch of rows xs with room for caps[r] pairs each, into a buffer of sentinel words with `margin` more pairs
    behind the last row's room.  slots_of: {x: row_slots(x)}, an id that is not in it has no row.
    -> (offsets uint64[n + 1], buffer uint32[2 * (total + margin)] as it must look afterwards, counts uint32[n])"""
    xs = _u32(xs)
    offsets = np.zeros(xs.size + 1, np.uint64)
    np.cumsum(np.asarray(caps, dtype=np.uint64), out=offsets[1:])
    buf = np.full(2 * (int(offsets[-1]) + margin), sentinel, np.uint32)
    counts = np.zeros(xs.size, np.uint32)
    full = {x: table_row_model(s).reshape(-1) for x, s in slots_of.items()}
    for r, (x, cap) in enumerate(zip(xs.tolist(), np.asarray(caps).tolist())):
        row = full.get(x)
        if row is None:
            continue
        k = min(int(cap), row.size // 2)
        o = 2 * int(offsets[r])
        buf[o:o + 2 * k] = row[:2 * k]
        counts[r] = k
    return offsets, buf, counts


def edge_caps(c):
    """the caps at which a walk of a row of c pairs can go wrong: none, one, around the wave step, around the row's own length"""
    return sorted({0, 1, WAVE_STEP - 1, WAVE_STEP, WAVE_STEP + 1, max(c - 1, 0), c, c + 1})


# ---- builders -----------------------------------------------------------------------------------------------------------------

def distinct_columns(n, rng, lo=1, hi=1 << 32):
    """n distinct columns drawn from [lo, hi), in drawn (not ascending) order"""
    have = np.zeros(0, np.uint32)
    while have.size < n:
        draw = rng.integers(lo, hi, n - have.size + (n - have.size) // 16 + 16, dtype=np.uint64).astype(np.uint32)
        have = np.unique(np.concatenate([have, draw]))
    return rng.permutation(have)[:n]


def rows_with_pair_counts(counts, seed, first_row=1000):
    """rows first_row, first_row + 1, .. (adjacent ids: a neighbour's pairs would show) with counts[i] pairs each, columns
    over the whole uint32 range: -> (x, y, v) unique triples, in drawn order"""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    for i, c in enumerate(counts):
        xs.append(np.full(c, first_row + i, np.uint32))
        ys.append(distinct_columns(c, rng))
    x, y = np.concatenate(xs), np.concatenate(ys)
    return x, y, pair_value(x, y)


def columns_varying_in_bytes(n, b0, b1, fixed=0x5A):
    """n <= 65536 distinct columns that differ only in bytes b0 and b1 (0 = lowest); the other two bytes hold `fixed`.  The n
    values of the two free bytes are scattered over all 65536 (an odd multiplier is a bijection modulo 2^16)."""
    assert 0 < n <= 65536 and b0 != b1 and 0 <= b0 < 4 and 0 <= b1 < 4
    w = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(1)) & np.uint64(0xFFFF)
    col = np.uint64(0)
    for b in range(4):
        if b not in (b0, b1):
            col |= np.uint64(fixed << (8 * b))
    col = col | ((w & np.uint64(255)) << np.uint64(8 * b0)) | ((w >> np.uint64(8)) << np.uint64(8 * b1))
    assert (col != 0).all() and np.unique(col).size == n
    return col.astype(np.uint32)


def row_list_ids(n, seed):
    """n distinct row ids, in drawn order: the last id of the range (and id 0 from n = 2 on), from n = 4095 on a block of 256
    ids that differ only in their top byte, the rest over the whole uint32 range"""
    rng = np.random.default_rng(seed)
    ids = [np.array([M32], np.uint32)]
    if n >= 2:
        ids.append(np.array([0], np.uint32))
    if n >= 4095:
        ids.append((np.arange(256, dtype=np.uint32) << np.uint32(24)) | np.uint32(0x00C0FFEE))
    have = np.unique(np.concatenate(ids))
    while have.size < n:
        have = np.unique(np.concatenate([have, rng.integers(0, 1 << 32, n - have.size + 16, dtype=np.uint64).astype(np.uint32)]))
    if have.size > n:                                                  # drop drawn ids only, never the named ones
        named = np.unique(np.concatenate(ids))
        drawn = np.setdiff1d(have, named)
        have = np.concatenate([named, rng.permutation(drawn)[:n - named.size]])
    return rng.permutation(have)
