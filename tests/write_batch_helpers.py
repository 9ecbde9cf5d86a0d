"""The model of a write batch at the edges of the fold kernels and of the growth tiers (kernels/ops.hpp: apply_agg_body, k_set_fold;
kernels/growth.hpp, prep_bulk.hpp), shared by tests/test_write_batch_model.py (no GPU: every case's precondition, on the oracle and on
this file alone) and tests/test_gpu_write_batch_edges.py (the kernels).

The model is the oracle (oracle/oracle.py) plus what it cannot say by itself:

    serialisable     whether SOME serial order of a key's incr / decr ops returns exactly what a batch returned (an unordered batch
                     may take any order, include/smatrix_batch.h; with mixed amounts the returns differ from order to order)
    slot_incr / slot_incr_clustered / slot_set
                     the LDS start slots of the folds, so that a case can put 2048 keys on ONE slot at the end of the table
    the builders     batches as (op, x, y, v) with the property each must have; rows are laid out so that every key that matters
                     sits at its home cell (keys below the row's size, or distinct residues): such tables are the same bytes in
                     every order, which the model file proves per case by applying it forward, reversed and shuffled

state_equal / per_key_sorted are the comparisons tests/test_gpu_parity.py has always used; they live here now and are imported there."""
import functools

import numpy as np

OP_GET, OP_SET, OP_INCR, OP_DECR = 0, 1, 2, 3
ALL_ONES = 0xFFFFFFFF

# The folds' constants.  None is exported through _lib; each is stated once, here.
AGG_MIN = 1024            # smx_runtime.hip, Matrix::agg_min: the lane-per-op kernel below it, the fold from it on
AGG_TILE = 2048           # ops.hpp: AGG_TILE = AGG_THREADS * AGG_OPT (1024 lanes x 2 ops)
AGG_SLOTS = 4096          # ops.hpp: AGG_SLOTS = 2 * AGG_TILE
ROW_FIRST = 16            # the reference's first row size (src/smatrix.c:641)

N_INCR = (1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 6143)
N_SET = (1023, 1024, 2048, 2049, 4097)
TIER_SIZES = (256, 512, 2048, 4096, 8192, 16384)      # GROW_LG0 / 1 / 2 at 256 / 2048 / 8192 old cells, chunked beyond; 16384 -> BIG_LG


def u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64) & np.uint64(0xFFFFFFFF), dtype=np.uint32)


def key64(x, y):
    return np.asarray(x, np.uint32).astype(np.uint64) << np.uint64(32) | np.asarray(y, np.uint32).astype(np.uint64)


# ---- the comparisons of test_gpu_parity.py -------------------------------------------------------------------------------------------
def per_key_sorted(x, y, ret):
    k = x.astype(np.uint64) << 32 | y.astype(np.uint64)
    o = np.lexsort((ret, k))
    return k[o], ret[o]


def state_equal(g, o, rows, exact_layout):
    for x in rows:
        gi, oi = g.row_info(x), o.row_info(x)
        assert gi == oi, ("row_info", x, gi, oi)
        a, b = np.asarray(g.row_slots(x)), np.asarray(o.row_slots(x))
        if exact_layout:
            assert (a == b).all(), ("layout", x)
        else:
            ka = a[(a[:, 0] != 0) | (a[:, 1] != 0)]; kb = b[(b[:, 0] != 0) | (b[:, 1] != 0)]
            ka = ka[np.lexsort((ka[:, 1], ka[:, 0]))]; kb = kb[np.lexsort((kb[:, 1], kb[:, 0]))]
            assert ka.shape == kb.shape and (ka == kb).all(), ("content", x)
            # and the table must be a valid `key % size` linear-probe layout (src/smatrix.c:363-380)
            size = a.shape[0]
            for p in np.nonzero(a[:, 0])[0]:
                q = int(a[p, 0]) % size
                while q != p:
                    assert a[q, 0] != 0 or a[q, 1] != 0, ("probe chain broken", x, int(a[p, 0]))
                    q = (q + 1) % size


# ---- serialisable --------------------------------------------------------------------------------------------------------------------
def serialisable(op, before, v, ret, after):
    """One key: the cell held `before`, the batch's ops on it carried the amounts v and returned ret, the cell holds `after`.  True
    exactly when some order of the ops returns these values, in uint32 arithmetic.  Every op is an edge  ret -+ v -> ret  of a
    multigraph over uint32 values; a serial order is an Eulerian trail from `before` to `after` over every edge: out - in is +1 at
    `before` and -1 at `after` (0 everywhere when they are one value) and all edges lie in the weakly connected component of
    `before` (with balanced degrees, weakly connected is strongly connected)."""
    assert op in (OP_INCR, OP_DECR)
    v, ret = u32(v), u32(ret)
    if v.shape != ret.shape:
        return False
    before, after = int(before) & ALL_ONES, int(after) & ALL_ONES
    n = v.size
    if n == 0:
        return before == after
    src = ret - v if op == OP_INCR else ret + v                       # (uint32 arrays wrap)
    nodes, inv = np.unique(np.concatenate([src, ret, np.array([before, after], np.uint32)]), return_inverse=True)
    s, d, b, a = inv[:n], inv[n:2 * n], int(inv[2 * n]), int(inv[2 * n + 1])
    bal = np.bincount(s, minlength=nodes.size).astype(np.int64) - np.bincount(d, minlength=nodes.size)
    want = np.zeros(nodes.size, np.int64)
    want[b] += 1; want[a] -= 1
    if (bal != want).any():
        return False
    parent = list(range(nodes.size))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i, j in zip(s.tolist(), d.tolist()):
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[ri] = rj
    root = find(b)
    return all(find(i) == root for i in set(s.tolist()))


def check_returns(op, x, y, v, ret, before, after, tag=""):
    """the returns of an incr / decr batch, key by key: serialisable from the key's value before the batch to its value after"""
    x, y, v, ret, before, after = (np.asarray(a, np.uint32) for a in (x, y, v, ret, before, after))
    k = key64(x, y)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    ends = np.r_[starts[1:], ks.size]
    single = ends - starts == 1
    i = order[starts[single]]
    src = ret[i] - v[i] if op == OP_INCR else ret[i] + v[i]
    bad = i[(src != before[i]) | (ret[i] != after[i])]
    assert bad.size == 0, (tag, "single ops", bad.size, [(int(x[j]), int(y[j]), int(before[j]), int(v[j]), int(ret[j]), int(after[j])) for j in bad[:6]])
    for s, e in zip(starts[~single].tolist(), ends[~single].tolist()):
        j = order[s:e]
        assert serialisable(op, before[j[0]], v[j], ret[j], after[j[0]]), \
            (tag, "no serial order returns this", int(x[j[0]]), int(y[j[0]]), int(before[j[0]]), int(after[j[0]]), j[:8].tolist(), v[j][:8].tolist(), ret[j][:8].tolist())


def last_wins(x, y, v):
    """a set batch's result: (x, y, v) of each key's LAST occurrence"""
    k = key64(x, y)
    uk, first_rev = np.unique(k[::-1], return_index=True)
    return (uk >> np.uint64(32)).astype(np.uint32), (uk & np.uint64(ALL_ONES)).astype(np.uint32), np.asarray(v, np.uint32)[::-1][first_rev]


# ---- the LDS slot functions ----------------------------------------------------------------------------------------------------------
def _mix(x, y):
    x, y = np.asarray(x, np.uint32), np.asarray(y, np.uint32)
    h = (x * np.uint32(0x9E3779B1)) ^ (y * np.uint32(0x85EBCA77))
    return h ^ (h >> np.uint32(15))


def slot_incr(x, y):
    """apply_agg_body, ops.hpp: h = X*0x9E3779B1 ^ Y*0x85EBCA77; h ^= h >> 15; h &= AGG_SLOTS - 1"""
    return _mix(x, y) & np.uint32(AGG_SLOTS - 1)


def slot_incr_clustered(x, y):
    """apply_agg_body<CLU>: Y >> 4 in the product, + (Y & 15) before the mask (a 128-byte line of a row takes 16 slots in a row)"""
    y = np.asarray(y, np.uint32)
    return (_mix(x, y >> np.uint32(4)) + (y & np.uint32(15))) & np.uint32(AGG_SLOTS - 1)


def slot_set(x, y):
    """k_set_fold, ops.hpp: its own line, the arithmetic of the plain increment fold (its empty marker is key 0, not all-ones)"""
    return _mix(x, y) & np.uint32(AGG_SLOTS - 1)


SLOT_FNS = {"incr": slot_incr, "clustered": slot_incr_clustered, "set": slot_set}
CROWD_ROW = {"incr": 7, "clustered": 8, "set": 7}
CROWD_TAIL = 100          # the start slot lies within the last 100 slots, so the chain of 2048 keys wraps the table's end


@functools.lru_cache(maxsize=None)
def crowd(which, count=AGG_TILE + 1):
    """`count` distinct keys of one row that all START on one LDS slot of the named fold, that slot within the last CROWD_TAIL of the
    AGG_SLOTS: the first AGG_TILE of them fill the table to load exactly 1/2 in one chain that wraps slot 4095 -> 0, and l_list to
    its last entry.  -> (x, y[count], slot)"""
    fn, x = SLOT_FNS[which], CROWD_ROW[which]
    y = np.arange(1, 1 << 24, dtype=np.uint32)
    s = fn(np.uint32(x), y)
    tail = np.bincount(s[s >= AGG_SLOTS - CROWD_TAIL], minlength=AGG_SLOTS)
    slot = int(np.argmax(tail))
    ys = y[s == slot][:count]
    assert ys.size == count, (which, slot, ys.size)
    return x, ys, slot


# ---- batches -------------------------------------------------------------------------------------------------------------------------
class Batch:
    """one call.  exact: the tables it leaves are order-independent, byte for byte (proved in the model file); study: an incr / decr
    batch whose returns are the point (the model file runs it in 20 orders); deferred: whether its round 0 must leave ops for the
    round loop (None: either)"""
    def __init__(self, name, op, x, y, v, exact=True, study=True, deferred=None):
        self.name, self.op, self.exact, self.study, self.deferred = name, op, exact, study, deferred
        self.x, self.y, self.v = u32(x), u32(y), u32(v)
        assert self.x.shape == self.y.shape == self.v.shape

    @property
    def n(self):
        return self.x.size

    def rows(self):
        return np.unique(self.x).tolist()

    def permuted(self, p):
        return Batch(self.name, self.op, self.x[p], self.y[p], self.v[p], self.exact, self.study, self.deferred)


def amounts(rng, n, zero_total_head=0):
    """n seeded 32-bit amounts, one in 16 of them 0; the first zero_total_head are pairs (v, 2^32 - v) and zeros in a seeded order,
    so that their total is 0 -> (v, generic) with generic[i]: op i is neither 0 nor one of a pair (the mutation tests pick those)"""
    v = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    generic = np.ones(n, bool)
    z = rng.random(n) < 1 / 16
    v[z] = 0; generic[z] = False
    h = min(zero_total_head, n)
    if h:
        pairs = h // 2 - h // 32
        a = rng.integers(1, 1 << 32, pairs, dtype=np.uint64).astype(np.uint32)
        head = np.concatenate([a, np.uint32(0) - a, np.zeros(h - 2 * pairs, np.uint32)])
        v[:h] = rng.permutation(head)
        generic[:h] = False
        assert int(v[:h].astype(np.uint64).sum()) % (1 << 32) == 0
    return v, generic


# rows of the increment and set scenarios (every key below its row's size: at home, whatever the order)
R_ONE = 11                              # the one-key batches: cell (11, 5) present, key (11, 6) absent
R_PRESENT = (20, 21, 22, 23)            # keys 1..40 in 128 cells
R_ROOM = (30, 31, 32, 33)               # keys 1..20 in 64 cells: room for 13 more
R_FULL = 40                             # keys 1..33 in 64 cells: used == size/2 + 1, the next new key doubles it
R_NEW = (50, 51, 52, 53)                # rows that do not exist
R_HEAD = (60, 61)                       # keys 1..5 and a head cell (0, 2^20): y == 0 ops find it, and it stays non-zero
R_ZERO = 0                              # row 0 (set scenario)
HEAD_VALUE = 1 << 20


def setup_batches(op):
    """the world before the studied batches, in two calls of distinct keys (one order only): every cell that must be present, the
    all-ones key among them; then the head cells.  The key that crosses zero starts near it: 100 for decr, 2^32 - 100 for incr."""
    xs, ys, vs = [], [], []

    def put(x, keys, val):
        keys = np.asarray(keys, np.uint32)
        xs.append(np.full(keys.size, x, np.uint32)); ys.append(keys); vs.append(u32(np.broadcast_to(val, keys.shape)))
    put(R_ONE, [5, 9, 12], [77, 1, 2])
    for r in R_PRESENT:
        put(r, np.arange(1, 41), 1000 + np.arange(1, 41))
    for r in R_ROOM:
        put(r, np.arange(1, 21), 5)
    put(R_FULL, np.arange(1, 34), 9)
    for r in R_HEAD:
        put(r, np.arange(1, 6), 3)
    put(R_ZERO, np.arange(1, 21), 11)
    put(ALL_ONES, [ALL_ONES, 1], [123456, 1])
    x, y, v = np.concatenate(xs), np.concatenate(ys), np.concatenate(vs)
    cross = (x == R_PRESENT[0]) & (y == 1)
    v[cross] = 100 if op == OP_DECR else (1 << 32) - 100
    world = Batch("setup", OP_INCR, x, y, v, study=False)
    heads = Batch("setup heads", OP_INCR, R_HEAD, [0] * len(R_HEAD), [HEAD_VALUE] * len(R_HEAD), study=False)
    return [world, heads]


def one_key_batches(op, n, seed):
    """all n ops on one key: a present cell, then an absent key of the same row.  The first tile's amounts total 0 (pairs v, 2^32 - v
    and zeros): for n <= 2048 the absent key ends as a live (6, 0) cell that counts in rowlen."""
    rng = np.random.default_rng(seed)
    out = []
    for name, y in (("one key, present", 5), ("one key, absent", 6)):
        v, _ = amounts(rng, n, AGG_TILE)
        out.append(Batch("%s, n=%d" % (name, n), op, np.full(n, R_ONE), np.full(n, y), v, deferred=False if y == 5 else None))
    return out


def mixed_batch(op, n, seed):
    """n ops, every kind in the first tile, duplicates included: a key at indices 0 and n - 1, one at 2047 and 2048 (n >= 2049), the
    all-ones key five times, a key that crosses zero, y == 0 ops on the head cells, present keys, absent keys of rows with room,
    absent keys of the row at its threshold and keys of rows that do not exist (the last two come back through the deferred list);
    the rest of the batch are hits on present keys."""
    rng = np.random.default_rng(seed)
    x = rng.choice(np.asarray(R_PRESENT[2:], np.uint32), n)                 # filler: hits on rows 22 / 23
    y = rng.integers(4, 41, n).astype(np.uint32)
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    kinds = []                                                               # (x, y, v) lists to be scattered over the first tile

    def add(xx, yy, vv):
        xx, yy = np.broadcast_arrays(u32(xx), u32(yy))
        kinds.append((xx, yy, u32(np.broadcast_to(vv, xx.shape))))
    add(ALL_ONES, [ALL_ONES] * 5, rng.integers(1, 1 << 32, 5))
    add(R_PRESENT[0], [1] * 40, rng.integers(1, 6, 40))                     # 100 -> below zero (decr); 2^32 - 100 -> past it (incr)
    for r in R_HEAD:
        add(r, [0] * 30, rng.integers(1, 4, 30))                            # 2^20 -+ at most 90: the head cell stays non-zero
    add(R_PRESENT[1], np.repeat(np.arange(4, 24), 4), rng.integers(0, 1 << 32, 80))
    for r in R_ROOM:
        add(r, np.repeat(np.arange(21, 31), 3), rng.integers(0, 1 << 32, 30))      # 10 new keys: used 30 <= 33, no growth
    add(R_FULL, np.repeat(np.arange(34, 41), 3), rng.integers(0, 1 << 32, 21))       # 7 new keys at the threshold: 64 -> 128 cells
    for r in R_NEW:
        add(r, np.repeat(np.arange(1, 9), 2), rng.integers(0, 1 << 32, 16))          # 8 keys: a new 16-cell row
    kx, ky, kv = (np.concatenate(a) for a in zip(*kinds))
    ends = [0, n - 1]                                                        # (20, 3): first and last op of the batch
    edge = [AGG_TILE - 1, AGG_TILE] if n > AGG_TILE else []                  # (21, 3): either side of the tile boundary
    free = np.array([i for i in range(min(n, AGG_TILE)) if i not in set(ends + edge)])
    at = rng.permutation(free)[:kx.size]
    assert at.size == kx.size
    x[at], y[at], v[at] = kx, ky, kv
    x[ends] = R_PRESENT[0]; y[ends] = 3
    if n == AGG_TILE + 1:
        edge = [0] + edge                                                    # (n - 1 IS the boundary's far side: one key has both properties)
    x[edge] = R_PRESENT[1]; y[edge] = 3
    return Batch("mixed, n=%d" % n, op, x, y, v, deferred=True)


def incr_scenario(op, n, seed=0):
    """the batches of one handle: setup, the one-key batches, the mixed batch, and the mixed batch's ops once more (all present now)"""
    m = mixed_batch(op, n, 1000 * n + op + seed)
    again = Batch("mixed again, n=%d" % n, op, m.x, m.y, m.v, deferred=False)
    return setup_batches(op) + one_key_batches(op, n, 77 * n + op + seed) + [m, again]


def crowd_scenario(op, seed=5):
    """per hash: its 2048 crowded keys once (a new row: everything deferred), once again (present: the fold's table at load exactly
    1/2, l_list full, the chain across slot 4095), each twice inside a tile, each twice in two tiles, and 2049 keys: one spills"""
    rng = np.random.default_rng(seed + op)
    out = []
    for which in ("incr", "clustered"):
        x, ys, _ = crowd(which)
        k = ys[:AGG_TILE]
        val = lambda m: rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)      # noqa: E731
        for name, yy, d in (("new", k, True), ("once", rng.permutation(k), False), ("twice in a tile", np.repeat(k, 2), False),
                            ("twice, two tiles", np.concatenate([k, rng.permutation(k)]), False), ("2049 keys", ys, None)):
            out.append(Batch("crowd %s: %s" % (which, name), op, np.full(yy.size, x), yy, val(yy.size), exact=False, deferred=d))
    return out


def set_scenario(n, seed=0):
    """setup; one key on all n ops; the mixed set batch; the same keys again (all present: the fold's own cell addresses hold)"""
    rng = np.random.default_rng(4000 + n + seed)
    out = setup_batches(OP_INCR)
    out.append(Batch("set: one key, n=%d" % n, OP_SET, np.full(n, R_ONE), np.full(n, 5), rng.integers(0, 1 << 32, n), study=False, deferred=False))
    x = rng.choice(np.asarray(R_PRESENT[2:], np.uint32), n)
    y = rng.integers(4, 41, n).astype(np.uint32)
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    kinds = []

    def add(xx, yy):
        xx, yy = np.broadcast_arrays(u32(xx), u32(yy))
        kinds.append((xx, yy))
    add(ALL_ONES, [ALL_ONES] * 5)
    add(R_ZERO, np.repeat(np.arange(1, 31), 2))                             # row 0: keys 1..20 present, 21..30 new (used 30 <= 33)
    add(R_FULL, np.repeat(np.arange(34, 38), 2))                            # absent, row at its threshold: deferred winners
    for r in R_NEW[:2]:
        add(r, np.repeat(np.arange(1, 9), 2))
    kx, ky = (np.concatenate(a) for a in zip(*kinds))
    # (21, 3): its two highest indices either side of the tile boundary (n >= 2049), else its last is the batch's last op
    # (40, 40): absent from the row at its threshold in tile 0 -- that winner is deferred -- and named again in tile 1 (n >= 2050)
    if n > AGG_TILE:
        k21, k40 = [0, 1, AGG_TILE - 1, AGG_TILE], [2] + ([AGG_TILE + 1] if n > AGG_TILE + 1 else [])
    else:
        k21, k40 = [0, 1, n - 1], [2, n - 2]
    free = np.array([i for i in range(min(n, AGG_TILE)) if i not in set(k21 + k40)])
    at = rng.permutation(free)[:kx.size + 2 * len(R_HEAD)]
    x[at[:kx.size]], y[at[:kx.size]] = kx, ky
    for i, r in enumerate(R_HEAD):                                          # y == 0 (the `own` path, applied unranked): two ops, ONE value
        j = at[kx.size + 2 * i: kx.size + 2 * i + 2]
        x[j], y[j], v[j] = r, 0, 700 + i
    x[k21] = R_PRESENT[1]; y[k21] = 3
    x[k40] = R_FULL; y[k40] = 40
    m = Batch("set: mixed, n=%d" % n, OP_SET, x, y, v, study=False, deferred=True)
    out.append(m)
    out.append(Batch("set: mixed again, n=%d" % n, OP_SET, m.x, m.y, m.v ^ np.uint32(0x5A5A5A5A), study=False, deferred=False))
    return out


# ---- tiers ---------------------------------------------------------------------------------------------------------------------------
TIER_SUBCASES = tuple((k, rep) for rep in (1, 3) for k in ("one", "fill", "spill"))      # the row of sub-case i is TIER_ROW0 + i
TIER_ROW0 = 101


class Tier:
    """one old size S: six rows built by ONE batch to used == S/2 + 1 in S cells, then one batch per row --
    one: 1 new key (one doubling); fill: S/2 new keys, all the doubled table may still take (one doubling, used == S + 1);
    spill: S/2 + 1 (a second doubling inside the batch); each with every new key once, and three times.
    Keys: dense (1, 2, ...: the clustered walk) or scrambled as residue + 2S * multiplier, the old keys' residues distinct below S and
    the new keys' distinct in [S, 2S): every key is at home at S, 2S and 4S cells, so each table is the same bytes in every order."""
    def __init__(self, size, dense, seed=0):
        self.size, self.dense = size, dense
        rng = np.random.default_rng(size + seed + (1 if dense else 0))
        half = size // 2
        self.build_x, self.build_y, self.cases = [], [], []
        for i, (kind, rep) in enumerate(TIER_SUBCASES):
            row = TIER_ROW0 + i
            k_new = {"one": 1, "fill": half, "spill": half + 1}[kind]
            if dense:
                old = np.arange(1, half + 2, dtype=np.uint32)
                new = np.arange(half + 2, half + 2 + k_new, dtype=np.uint32)
            else:
                mult = lambda m: rng.integers(0, 1 << 10, m).astype(np.uint32) * np.uint32(2 * size)      # noqa: E731
                old = (rng.permutation(np.arange(1, size, dtype=np.uint32))[:half + 1] + mult(half + 1)).astype(np.uint32)
                new = (rng.permutation(np.arange(size, 2 * size, dtype=np.uint32))[:k_new] + mult(k_new)).astype(np.uint32)
            self.build_x.append(np.full(old.size, row, np.uint32)); self.build_y.append(old)
            y = rng.permutation(np.tile(new, rep))
            b = Batch("tier %d %s: %s x%d" % (size, "dense" if dense else "scrambled", kind, rep), OP_INCR, np.full(y.size, row), y,
                      rng.integers(1, 1 << 32, y.size), deferred=True)
            b.row, b.doublings, b.used_after = row, 2 if kind == "spill" else 1, half + 1 + k_new
            self.cases.append(b)
        x, y = np.concatenate(self.build_x), np.concatenate(self.build_y)
        p = rng.permutation(x.size)
        self.build = Batch("tier %d build" % size, OP_INCR, x[p], y[p], rng.integers(1, 1 << 32, x.size), study=False)


def bulk_batch(op, seed=9):
    """4096 ops into an EMPTY matrix, every key twice: rows of 8, 9, 10 keys (either side of 16 -> 32 cells) and of 256, 257, 258
    (either side of 512 -> 1024, beyond the 512-cell limit of k_fix_*), two rows of each, filled up with 8-key rows.  Keys 1..k."""
    rng = np.random.default_rng(seed)
    counts = [8, 9, 10, 256, 257, 258] * 2
    counts += [8] * ((AGG_SLOTS // 2 - sum(counts)) // 8)
    counts.append(AGG_SLOTS // 2 - sum(counts))
    assert counts[-1] > 0 and sum(counts) == 2048
    x = np.concatenate([np.full(c, 1000 + i, np.uint32) for i, c in enumerate(counts)])
    y = np.concatenate([np.arange(1, c + 1, dtype=np.uint32) for c in counts])
    p = rng.permutation(2 * x.size) % x.size
    b = Batch("bulk", op, x[p], y[p], rng.integers(0, 1 << 32, p.size), deferred=True)
    b.counts = dict(zip(range(1000, 1000 + len(counts)), counts))
    return b


def rows_for(count):
    """cells of a row that took `count` distinct keys one by one: it doubles when used > size/2 before an insert (src/smatrix.c:346)"""
    size = ROW_FIRST
    while size // 2 + 1 < count:
        size *= 2
    return size


# ---- running a scenario on the oracle -------------------------------------------------------------------------------------------------
def apply_checked(o, b, tag=""):
    """one batch on the oracle (in index order) with its own returns checked: -> (returns, before, after)"""
    before = o.apply(OP_GET, b.x, b.y)
    ret = o.apply(b.op, b.x, b.y, b.v)
    after = o.apply(OP_GET, b.x, b.y)
    if b.op == OP_SET:
        assert (ret == b.v).all(), (tag, b.name)
        lx, ly, lv = last_wins(b.x, b.y, b.v)
        assert (o.apply(OP_GET, lx, ly) == lv).all(), (tag, b.name, "last occurrence")
    else:
        check_returns(b.op, b.x, b.y, b.v, ret, before, after, (tag, b.name))
    return ret, before, after


def dump_rows(m, rows):
    return {r: (m.row_info(r), np.asarray(m.row_slots(r)).tobytes()) for r in rows}
