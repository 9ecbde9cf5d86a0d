"""What tests/test_gpu_merge.py, test_gpu_merge_scaled.py and test_gpu_merge_topk.py share (a plain module, no tests of its own):
the op codes, the expected ops of a merge read from an oracle, the comparison of a matrix with its oracle, the source builders.

A SIDE of a comparison is an oracle or a candidate list -- the triple (x, y, v) that ops_of() makes of one."""
import numpy as np
import pytest

from libsmatrix_amd.stream import Stream

GET, SET, INCR, DECR = 0, 1, 2, 3
OPS = {"set": SET, "incr": INCR, "decr": DECR}


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
