"""What tests/test_gpu_merge.py, test_gpu_merge_scaled.py, test_gpu_merge_topk.py and test_gpu_merge_topk_by.py share (a plain
module, no tests of its own): the op codes, the expected ops of a merge read from an oracle, the comparison of a matrix with its
oracle, the source builders, and of the two top-k files the row shapes and the case of the rows around one step of a wave.

A SIDE of a comparison is an oracle or a candidate list -- the triple (x, y, v) that ops_of() makes of one."""
import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix
from libsmatrix_amd.stream import Stream

GET, SET, INCR, DECR = 0, 1, 2, 3
OPS = {"set": SET, "incr": INCR, "decr": DECR}
M_MAX = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


def u32(*a):
    return np.array(a, np.uint32)


def nonempty(kv):
    return kv[(kv[:, 0] != 0) | (kv[:, 1] != 0)]


def ops_of(o):
    """the ops a merge of this oracle's matrix applies (the candidates of a filtered one): rows in list_rows() order,
    non-empty slots in slot order"""
    xs, ys, vs = [], [], []
    for x in o.list_rows().tolist():
        ne = nonempty(o.row_slots(x))
        xs.append(np.full(ne.shape[0], x, np.uint32)); ys.append(ne[:, 0]); vs.append(ne[:, 1])
    if not xs:
        z = np.zeros(0, np.uint32)
        return z, z, z
    return np.concatenate(xs), np.concatenate(ys).astype(np.uint32), np.concatenate(vs).astype(np.uint32)


def cand_of(side):
    return side if isinstance(side, tuple) else ops_of(side)


def col0_rows(*sides):
    """the rows that hold a column-0 pair on any of the sides"""
    out = set()
    for s in sides:
        x, y, _ = cand_of(s)
        out |= set(x[y == 0].tolist())
    return out


def probe_invariant(slots, x):
    size = slots.shape[0]
    occupied = (slots[:, 0] != 0) | (slots[:, 1] != 0)
    keys = slots[occupied, 0]
    assert np.unique(keys).size == keys.size, ("a key twice in row", x)
    for i in np.flatnonzero(occupied).tolist():
        p = int(slots[i, 0]) % size
        while p != i:
            assert occupied[p], ("an empty slot before key %d of row %d" % (slots[i, 0], x))
            p = (p + 1) % size


def check(m, o, sides, col0, tag):
    """m against o for every row / cell of the sides and of o itself: the row set; size and used of the rows that hold no
    column-0 pair on any side (nor are in col0: rows that held one before); the probe invariant of the others; get of every cell"""
    sides = [s for s in sides if s is not o]
    cands = [cand_of(s) for s in sides] + [ops_of(o)]
    ids = set(o.list_rows().tolist())
    for s, c in zip(sides, cands):
        ids |= set(np.unique(c[0]).tolist()) if isinstance(s, tuple) else set(s.list_rows().tolist())
    col0 = col0 | col0_rows(*cands)
    for x in sorted(ids):
        mi, oi = m.row_info(x), o.row_info(x)
        assert (mi is None) == (oi is None), (tag, "row set", x, mi, oi)
        if oi is None:
            continue
        if x not in col0:
            assert mi == oi, (tag, "size / used of row", x, mi, oi)
        else:
            probe_invariant(m.row_slots(x), x)
    cx, cy = np.concatenate([c[0] for c in cands]), np.concatenate([c[1] for c in cands])
    got, want = m.get_batch(cx, cy), o.apply(GET, cx, cy)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, bad.size, [(int(cx[i]), int(cy[i]), int(got[i]), int(want[i])) for i in bad[:8]])


def both(m, o, op, x, y, v):
    m.apply_batch(op, x, y, v, results=False)
    o.apply(op, x, y, v)


def row_dict(m, x):
    """the non-empty slots of row x as {column: value} (getRowLength is not the pair count in a row with a column-0 pair: Q1)"""
    kv = m.row_slots(x)
    return {int(k): int(v) for k, v in kv[(kv[:, 0] != 0) | (kv[:, 1] != 0)]}


def one_row(m, o, x, ys, vs):
    both(m, o, SET, np.full(len(ys), x, np.uint32), np.asarray(ys, np.uint32), np.asarray(vs, np.uint32))


def assert_export_equal(a, b, tag=""):
    for k, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape, (tag, k, u.shape, v.shape)
        assert (u == v).all(), (tag, k)


# ---- the sources: each fills a matrix and its oracle alike; `additions` (m, o), when given, runs last ---------------------------
def src_quirks(m, o, golden, additions=None):
    for op, args, _ in golden("quirks")["transcript"]:
        if op in ("set", "incr", "decr"):
            assert getattr(m, op)(*args) == getattr(o, op)(*args), (op, args)
    if additions:
        additions(m, o)


def src_zipf(m, o, golden, n=1000000, chunk=200000, additions=None):
    x, y = Stream("zipf", 12345, 1000000, 1.1, 1).fill(0, n)
    for k in range(n // chunk):
        s = slice(k * chunk, (k + 1) * chunk)
        both(m, o, INCR, x[s], y[s], np.ones(chunk, np.uint32))
    if additions:
        additions(m, o)


def src_dense(m, o, golden, n=800000, additions=None):
    x, y = Stream("zipf", 77, 300000, 1.1, 0).fill(0, n)
    x = (x % 40).astype(np.uint32)                                      # few rows -> large tables of dense (unscrambled) keys
    for k in range(n // 200000):
        s = slice(k * 200000, (k + 1) * 200000)
        both(m, o, INCR, x[s], y[s], ((x[s] + y[s]) % 3 + 1).astype(np.uint32))
    if additions:
        additions(m, o)


def src_one_long_row(m, o, golden, small=False, additions=None):
    """row 7: 200000 keys -> a table of 2^19 cells, 16 segments; small: half of its values are 0 (dead), 1, 2 or 3, mixed in
    every segment"""
    rng = np.random.default_rng(5)
    ys = (rng.permutation(1 << 20)[:200000] + 1).astype(np.uint32)
    vs = rng.integers(1, 1 << 32, ys.size, dtype=np.uint32)
    if small:
        few = rng.integers(0, 8, ys.size)
        vs = np.where(few < 4, few, vs).astype(np.uint32)
    both(m, o, INCR if small else SET, np.full(ys.size, 7, np.uint32), ys, vs)       # (an incr by 0 creates the cell)
    xs = np.repeat(np.arange(100000, 110000, dtype=np.uint32), 8)
    both(m, o, INCR, xs, rng.integers(1, 1 << 32, xs.size, dtype=np.uint32), rng.integers(1, 9, xs.size, dtype=np.uint32))
    if additions:
        additions(m, o)


# ---- the top-k merges: the row shapes of their `regimes` fixtures, and the case both files run on the rows around one step ------
# keys -> table: a table holds at most size / 2 keys, so these counts give 16, 512, 8192 (the wave path's last), 16384 and 32768
# (one workgroup, one segment), 65536 and 131072 slots (2 and 4 segments: cut rows).
REGIMES = {10: (7, 16), 11: (200, 512), 12: (3000, 8192), 13: (6000, 16384), 14: (12000, 32768), 15: (20000, 65536), 16: (40000, 131072)}
# A wave holds 128 cells at one step, and a rank whose keys cost a gather keeps those of such a row in registers: rows of 64 and 128
# slots on that path, 256 on the other.  Rows 20 and 22 have a head pair, 21 has none.
ONE_STEP = {20: (30, 64), 21: (60, 128), 22: (120, 256)}
ONE_STEP_HEADS = {20: 40, 22: 300}


def check_rows_around_one_step(oracle_mod, merged, column_totals):
    """merged = the file's merged_topk / merged_cos.  Values 1..5: ties everywhere; with column_totals the columns come from a pool
    of 400 ids of which 300 have a row with a head total in 1..50 (as the cosine file's regimes).  m = 1, half of and one less than
    every row's eligible count."""
    rng = np.random.default_rng(128)
    src, o_src = SparseMatrix(), oracle_mod.Oracle()
    pool = (50000 + rng.permutation(400)).astype(np.uint32)
    if column_totals:
        both(src, o_src, SET, pool[:300], np.zeros(300, np.uint32), rng.integers(1, 51, 300).astype(np.uint32))
    for x, (n, size) in ONE_STEP.items():
        one_row(src, o_src, x, rng.permutation(pool)[:n], rng.integers(1, 6, n))
        assert src.row_info(x) == o_src.row_info(x) and o_src.row_info(x)[0] == size, (x, src.row_info(x), o_src.row_info(x))
    both(src, o_src, SET, u32(*ONE_STEP_HEADS), np.zeros(len(ONE_STEP_HEADS), np.uint32), u32(*ONE_STEP_HEADS.values()))
    for x, (n, size) in ONE_STEP.items():                                 # the sizes of the source as it is merged
        assert src.row_info(x) == o_src.row_info(x) and o_src.row_info(x)[0] == size, (x, src.row_info(x), o_src.row_info(x))
    cand = ops_of(o_src)
    for m in sorted({k for n, _ in ONE_STEP.values() for k in (1, n // 2, n - 1)}):
        dst, o_dst = SparseMatrix(), oracle_mod.Oracle()
        ops, _ = merged(dst, o_dst, src, cand, "set", m, 1, tag="one step m %d" % m)
        for x, (n, size) in ONE_STEP.items():                             # (every pair is eligible: v >= 1)
            assert int(np.count_nonzero((ops[0] == x) & (ops[1] != 0))) == min(m, n), (x, m)
            assert len(row_dict(dst, x)) == min(m, n) + (x in ONE_STEP_HEADS), (x, m)
        dst.close(); o_dst.close()
    src.close(); o_src.close()
