"""The numpy model of the similarity measures of smatrix_cf_recommend_sim and smatrix_merge_topk_sim (include/smatrix_batch.h), for
tests/test_cf_sim_model.py and tests/test_gpu_cf_sim.py (a plain module, no tests of its own).

A candidate list is the triple (x, y, v) of tests/merge_topk_by_helpers.py; cand_of_export() makes one of SparseMatrix.export().
The score is IEEE double throughout.  numpy evaluates base and base + shrink as two array operations, each rounded to float64 on its
own: the two-step denominator of the contract, never a fused multiply-add.  fused_den() is the OTHER one, correctly rounded from
exact rationals: what a kernel that contracts a * b + c computes."""
from fractions import Fraction

import numpy as np

from tests.merge_topk_by_helpers import totals_of

SIM_COSINE, SIM_JACCARD, SIM_LIFT = 0, 1, 2
SIMS = {"cosine": SIM_COSINE, "jaccard": SIM_JACCARD, "lift": SIM_LIFT}


def factors(ta, tb, sim):
    """the two doubles whose product is the base of COSINE and LIFT (tb == 0 counted as 1)"""
    A = np.asarray(ta, np.uint32).astype(np.float64)
    tb = np.asarray(tb, np.uint32)
    B = np.where(tb == 0, 1, tb).astype(np.float64)
    return (np.sqrt(A), np.sqrt(B)) if sim == SIM_COSINE else (A, B)


def score(ta, tb, v, sim, shrink):
    """the score of pairs given as arrays of total(a), total(b) and the pair's value -> float64 array"""
    ta = np.asarray(ta, np.uint32)
    c = np.asarray(v, np.uint32).astype(np.float64)
    fa, fb = factors(ta, tb, sim)
    base = (fa + fb) - c if sim == SIM_JACCARD else fa * fb           # rounded on its own
    den = base + np.float64(shrink)                                   # then one add
    ok = (ta != 0) & (den != 0.0) & ~(c > den)
    return np.where(ok, c / np.where(ok, den, 1.0), 0.0)


def fused_den(x, y, shrink):
    """x * y + shrink rounded ONCE (a fused multiply-add), for doubles x, y"""
    return float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(shrink)))


def contraction_differs(ta, tb, v, sim, shrink):
    """per pair: would the score's bits change if the denominator of COSINE or LIFT were made with one fused multiply-add?"""
    assert sim in (SIM_COSINE, SIM_LIFT)
    ta, tb, v = (np.asarray(a, np.uint32) for a in (ta, tb, v))
    fa, fb = factors(ta, tb, sim)
    two_step = score(ta, tb, v, sim, shrink)
    out = np.zeros(ta.size, bool)
    for i in range(ta.size):
        den = fused_den(fa[i], fb[i], shrink)
        c = float(v[i])
        fused = c / den if (ta[i] != 0 and den != 0.0 and not c > den) else 0.0
        out[i] = np.float64(fused).view(np.uint64) != two_step[i].view(np.uint64)
    return out


def scores_sim(cand, sim, shrink):
    """the score of every candidate -> float64 array (the head pairs' entries mean nothing)"""
    x, y, v = cand
    return score(totals_of(cand, x), totals_of(cand, y), v, sim, shrink)


def topk_sim(cand, sim, shrink, m, min_value):
    """candidates -> (the kept ops (x, y, v), the number dropped): merge_topk_by_helpers.topk_cosine with scores_sim's bits"""
    x, y, v = cand
    bits = scores_sim(cand, sim, shrink).view(np.uint64)
    keep = (y == 0) & (v >= np.uint32(min_value)) & (v != 0)
    elig = (y != 0) & (v >= np.uint32(min_value))
    idx = np.flatnonzero(elig)
    order = idx[np.lexsort((y[idx], ~bits[idx], x[idx]))]                # by row, then by -score, then by column
    xs = x[order]
    first = np.flatnonzero(np.concatenate(([True], xs[1:] != xs[:-1]))) if xs.size else np.zeros(0, np.int64)
    rank_in_row = np.arange(xs.size) - np.repeat(first, np.diff(np.concatenate((first, [xs.size]))))
    keep[order[rank_in_row < m]] = True
    return (x[keep], y[keep], v[keep]), int(x.size - np.count_nonzero(keep))


def cand_of_export(export):
    """SparseMatrix.export() -> the candidate list (x, y, v)"""
    rows, row_ptr, pairs = export
    x = np.repeat(rows, np.diff(row_ptr.astype(np.int64)))
    return x, np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])


def sorted_export_of(ops):
    """ops (x, y, v), every (x, y) once -> what export("sorted") returns of a matrix that holds exactly them"""
    x, y, v = ops
    order = np.lexsort((y, x))
    x, y, v = x[order], y[order], v[order]
    rows, counts = np.unique(x, return_counts=True)
    row_ptr = np.zeros(rows.size + 1, np.uint64)
    np.cumsum(counts, out=row_ptr[1:])
    return rows.astype(np.uint32), row_ptr, np.stack([y, v], axis=1).astype(np.uint32)


class SessionModel:
    """smatrix_cf_recommend_sim restated over a matrix's contents: per session the distinct items in session order (first
    positions), the terms of an item's row -- score() of every pair (b != 0, cc), times the weight at the item's first position, the
    product a Python float of its own -- added left to right from 0.0; the session's items, the exclusion list and the denied ids
    removed; then (-score, id) and the cut at k."""

    def __init__(self, export):
        rows, row_ptr, pairs = export
        self.row = {int(a): pairs[int(row_ptr[i]):int(row_ptr[i + 1])] for i, a in enumerate(rows)}
        self.total = {a: int(p[p[:, 0] == 0, 1][0]) if (p[:, 0] == 0).any() else 0 for a, p in self.row.items()}
        self.cache = {}

    def terms(self, a, sim, shrink):
        """(columns, terms) of row a's pairs with a column != 0, as lists"""
        key = (a, sim, shrink)
        if key not in self.cache:
            p = self.row[a]
            p = p[p[:, 0] != 0]
            tb = np.array([self.total.get(int(b), 0) for b in p[:, 0]], np.uint32)
            t = score(np.full(p.shape[0], self.total[a], np.uint32), tb, p[:, 1], sim, shrink)
            self.cache[key] = (p[:, 0].tolist(), t.tolist())
        return self.cache[key]

    def ranking(self, sess, sim, shrink, w=None, excl=(), deny=()):
        own, gone = set(int(a) for a in sess), set(int(a) for a in excl) | set(int(a) for a in deny)
        total, done = {}, set()
        for i, a in enumerate(int(v) for v in sess):
            if a in done:
                continue
            done.add(a)
            if a not in self.row:
                continue
            wa = 1.0 if w is None else float(w[i])
            for b, t in zip(*self.terms(a, sim, shrink)):
                if b not in own:
                    total[b] = total.get(b, 0.0) + wa * t
        return sorted(((b, s) for b, s in total.items() if b not in gone), key=lambda kv: (-kv[1], kv[0]))

    def session(self, sess, k, sim, shrink, w=None, excl=(), deny=()):
        best = self.ranking(sess, sim, shrink, w, excl, deny)[:k]
        return [b for b, _ in best], np.array([s for _, s in best], np.float64)


# ---- the matrix both files look at -----------------------------------------------------------------------------------------------
# One matrix for the recommend call and for the truncation, given as SET ops with every (x, y) once, so that its contents are known
# without a GPU (sorted_export_of).  Values 1..5 nearly everywhere: ties are the rule.
#   POOL     400 column ids; the first 300 have a row that holds a head total in 1..400 and nothing else, the last 100 have no row
#            (total 0, counted as 1).  Totals in 1..400 are the range in which the fused cosine denominator differs at shrink 0.1.
#   BIG      8 ids with totals in 2^26..2^28 (A * B is beyond 2^53: it rounds, and the fused lift denominator differs at shrink 0.5),
#            each row holding the other seven; their totals are BIG_TOTALS and are NOT among the ops: the GPU fixture sets them with
#            the scalar call, world_contents() adds them.
#   rows 10 .. 17, by the shape the truncation meets (slots = cells; a table holds at most slots / 2 keys):
#     10   5 pairs: at most m = 8 eligible              11   30 pairs, 64 cells: the keys stay in registers
#     12   200 pairs, 512 cells: the wave path           13   5000 pairs, 16384 cells: the 1024-lane kernel; the recommend call's hot row
#     14   40 pairs of one value over columns of one total: every score ties, the columns decide
#     15   30 pairs of which 10 are dead cells (value 0): eligible with min_value 0 alone
#     16   20 pairs and no head pair: total 0, every score 0        17   25 pairs, a total of 2^27 + 12345, the BIG ids among its columns
#   SMALL    56 items whose rows hold 20 other SMALL ids, column 999 (no row: tb == 0) and two POOL columns: the LDS tier's sessions
#   7        a row of SMALL columns without a head pair: an item with ta == 0
M = 8
POOL = np.arange(50000, 50400, dtype=np.uint32)
POOL_WITH_ROW = 300
BIG = np.arange(60000, 60008, dtype=np.uint32)
BIG_TOTALS = {int(b): int(t) for b, t in zip(BIG, [1 << 26, (1 << 26) + 12345, 100000007, 123456789, (1 << 27) + 1, 200000033, 250000001,
                                                   (1 << 28) - 1])}
TIE_COLUMNS = np.arange(80000, 80040, dtype=np.uint32)      # row 14's: every one with the total 9
SMALL = np.arange(300, 356, dtype=np.uint32)
HOT, NO_HEAD_ROW, NO_HEAD_ITEM, ABSENT, NO_ROW_COLUMN = 13, 16, 7, 987654321, 999
HEADS = {10: 90, 11: 40, 12: 300, 13: 350, 14: 100, 15: 77, 17: (1 << 27) + 12345}
DEAD = 10                                                   # the first DEAD columns of row 15 end as dead cells


def world_ops():
    """-> (x, y, v) uint32 arrays: SET ops, every (x, y) once.  Row 15's dead cells are in them with the value they are decremented
    by afterwards (dead_cells())."""
    rng = np.random.default_rng(2718)
    xs, ys, vs = [], [], []

    def row(x, cols, vals):
        xs.append(np.full(len(cols), x, np.uint32)); ys.append(np.asarray(cols, np.uint32)); vs.append(np.asarray(vals, np.uint32))

    row_ids = POOL[:POOL_WITH_ROW]
    xs.append(row_ids); ys.append(np.zeros(row_ids.size, np.uint32)); vs.append(rng.integers(1, 401, row_ids.size).astype(np.uint32))
    xs.append(TIE_COLUMNS); ys.append(np.zeros(TIE_COLUMNS.size, np.uint32)); vs.append(np.full(TIE_COLUMNS.size, 9, np.uint32))
    for b in BIG:
        others = BIG[BIG != b]
        row(int(b), others, rng.integers(1, 6, others.size))
    row(10, rng.permutation(POOL)[:5], rng.integers(1, 6, 5))
    row(11, rng.permutation(POOL)[:30], rng.integers(1, 6, 30))
    row(12, rng.permutation(POOL)[:200], rng.integers(1, 6, 200))
    far = (70000 + rng.permutation(1 << 16)[:4600]).astype(np.uint32)
    far = far[~np.isin(far, TIE_COLUMNS)]
    row(13, np.concatenate([POOL, far]), rng.integers(1, 6, POOL.size + far.size))
    row(14, TIE_COLUMNS, np.full(TIE_COLUMNS.size, 2))
    row(15, rng.permutation(POOL)[:30], rng.integers(1, 6, 30))
    row(16, rng.permutation(POOL)[:20], rng.integers(1, 6, 20))
    row(17, np.concatenate([BIG, rng.permutation(POOL)[:17]]), rng.integers(1, 6, 25))
    for x, t in HEADS.items():
        row(x, [0], [t])
    for a in SMALL:
        others = rng.permutation(SMALL[SMALL != a])[:20]
        row(int(a), np.concatenate([others, [NO_ROW_COLUMN], rng.permutation(POOL)[:2], [0]]),
            np.concatenate([rng.integers(1, 31, 23), [rng.integers(1, 401)]]))
    row(NO_HEAD_ITEM, rng.permutation(SMALL)[:12], rng.integers(1, 6, 12))
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(vs)


def dead_cells(ops):
    """the (x, y, v) of row 15's first DEAD pairs: decrementing them by their own value leaves dead cells"""
    at = np.flatnonzero((ops[0] == 15) & (ops[1] != 0))[:DEAD]
    return ops[0][at], ops[1][at], ops[2][at]


def world_contents():
    """the candidates of the finished matrix: world_ops() with row 15's dead cells at 0 and the BIG totals set"""
    x, y, v = world_ops()
    v = v.copy()
    v[np.flatnonzero((x == 15) & (y != 0))[:DEAD]] = 0
    b = np.array(list(BIG_TOTALS), np.uint32)
    return (np.concatenate([x, b]), np.concatenate([y, np.zeros(b.size, np.uint32)]),
            np.concatenate([v, np.array(list(BIG_TOTALS.values()), np.uint32)]))


def lds_sessions():
    rng = np.random.default_rng(31)
    out = [[], [ABSENT], [0], [0, 0, 300], [NO_HEAD_ITEM], [303, 303, 305, 0, NO_HEAD_ITEM], [10, 11, 12, 11], [60000, 60001], [17, 60003, 14],
           [15, NO_HEAD_ROW, 10]]
    for _ in range(14):
        L = int(rng.integers(1, 12))
        s = rng.choice(SMALL, L).tolist()
        if L > 2:
            s[int(rng.integers(1, L))] = s[0]                       # a duplicate
        if L > 3 and rng.random() < 0.4:
            s[int(rng.integers(0, L))] = int(rng.choice([0, ABSENT, NO_HEAD_ITEM]))
        out.append([int(v) for v in s])
    return out


def global_sessions():
    return [[HOT], [HOT, 301, 302], [303, HOT, HOT, 0, ABSENT, 303], [12, HOT, NO_HEAD_ITEM, 60002]]


def all_sessions():
    q = lds_sessions()
    for i, s in enumerate(global_sessions()):
        q.insert(3 + 5 * i, s)
    return q
