"""The slot-order model of the item-neighbour calls (include/smatrix_batch.h smatrix_cf_neighbors_batch / _dev, smatrix_cf_topk_batch /
_dev; kernels/rows.hpp k_cf_neighbors, k_cf_topk), for tests/test_cf_neighbors_model.py and tests/test_gpu_cf_neighbors.py (a plain
module, no tests of its own).

NeighbourModel restates examples/cf_recommender.c:50-86 in numpy float64 over a matrix's own tables: the candidates of item a are the
non-empty cells of a's table in SLOT order, the (0, total) cell among them; score = val / (sqrt(total(a)) * sqrt(total(key))) with the
example's guards.  Scores are compared as uint64 bit patterns, never with a tolerance.

The guards matrix (guard_ops) holds one pair for every branch of the score that co-occurrence data built by incr 1 never reaches."""
import numpy as np

SET, DECR = 1, 3
STEP = 64                                                   # cells a wave of either kernel takes per step
JUNK_ID, JUNK_SCORE, JUNK_COUNT = 0x7a7a7a7a, -7.5, 99       # what a test puts where a call must not write


def bits(scores):
    return np.ascontiguousarray(scores, dtype=np.float64).view(np.uint64)


class Candidates:
    """an item's candidates in slot order: slot, id, val, ta (one number), tb (0 already counted as 1), den, score"""

    def __init__(self, slot, key, val, ta, tb):
        self.slot, self.id, self.val, self.ta, self.tb = slot, key, val, int(ta), tb
        num = val.astype(np.float64)
        self.den = np.sqrt(np.float64(self.ta)) * np.sqrt(tb.astype(np.float64))      # two roots, one product, each rounded on its own
        ok = (self.den != 0.0) & ~(num > self.den)
        self.score = np.where(ok, num / np.where(ok, self.den, 1.0), 0.0)
        self.size = 0

    def __len__(self):
        return self.id.size


class NeighbourModel:
    """slots_of(a) -> the (size, 2) {key, value} cells of a's table in slot order, or None for an item without a row;
    total_of(ids) -> get(id, 0) of every id of a uint32 array.  Everything is read once per item and kept: the model is of a
    matrix that does not change."""

    def __init__(self, slots_of, total_of):
        self.slots_of, self.total_of = slots_of, total_of
        self.cache = {}

    def candidates(self, a):
        a = int(a)
        if a not in self.cache:
            kv = self.slots_of(a)
            kv = np.zeros((0, 2), np.uint32) if kv is None else np.asarray(kv, np.uint32).reshape(-1, 2)
            at = np.flatnonzero((kv[:, 0] != 0) | (kv[:, 1] != 0))
            key, val = np.ascontiguousarray(kv[at, 0]), np.ascontiguousarray(kv[at, 1])
            ta = int(np.asarray(self.total_of(np.array([a], np.uint32)))[0]) if at.size else 0
            tb = np.asarray(self.total_of(key), np.uint32) if at.size else np.zeros(0, np.uint32)
            c = Candidates(at.astype(np.int64), key, val, ta, np.where(tb == 0, 1, tb).astype(np.uint32))
            c.size = kv.shape[0]
            self.cache[a] = c
        return self.cache[a]

    def entries(self, a):
        return len(self.candidates(a))

    def neighbours(self, a, cap):
        """the first cap candidates in slot order -> (ids uint32, scores float64)"""
        c = self.candidates(a)
        return c.id[:cap], c.score[:cap]

    def order(self, a):
        """the candidates' indices by (score bits descending, slot ascending)"""
        c = self.candidates(a)
        return np.lexsort((c.slot, ~bits(c.score)))

    def topk(self, a, k):
        c = self.candidates(a)
        o = self.order(a)[:k]
        return c.id[o], c.score[o]

    def skipped_steps(self, a, k):
        """the 64-cell steps of a's table none of whose candidates beats the k-th best of the steps before it: what k_cf_topk may
        pass over without a sort (a step without candidates counts)"""
        c = self.candidates(a)
        b = bits(c.score)
        out, best = [], np.zeros(0, np.uint64)                            # best: the k best bit patterns so far, descending
        for s in range((c.size + STEP - 1) // STEP):
            mine = b[(c.slot // STEP) == s]
            if best.size == k and not (mine > best[-1]).any():            # an equal score in a later slot does not beat it
                out.append(s)
                continue
            best = np.sort(np.concatenate([best, mine]))[::-1][:k]
        return out


def oracle_model(o):
    """the model fed from an Oracle (or Reference) instance's own row_slots and get"""
    return NeighbourModel(o.row_slots, lambda ids: np.array([o.get(int(b), 0) for b in ids], np.uint32))


def matrix_model(m):
    """the model fed from a SparseMatrix by read paths that share no code with the two kernels: row_slots and get_batch(ids, 0)"""
    return NeighbourModel(m.row_slots, lambda ids: m.get_batch(ids, np.zeros(len(ids), np.uint32)))


def table_export_agrees(m, model):
    """the non-empty cells of row_slots in order are export("table")'s pairs of that row, for every row -> the row ids"""
    rows, row_ptr, pairs = m.export("table")
    for i, a in enumerate(rows.tolist()):
        c = model.candidates(a)
        mine = pairs[int(row_ptr[i]):int(row_ptr[i + 1])]
        assert mine[:, 0].tobytes() == c.id.tobytes() and mine[:, 1].tobytes() == c.val.tobytes(), ("row_slots and export disagree", a)
    return rows


# ---- expected outputs, whole arrays ---------------------------------------------------------------------------------------------
def expected_neighbours(model, items, offsets, fill_id, fill_score, pad=0):
    """what smatrix_cf_neighbors_batch leaves in ids / scores [0, offsets[n] + pad) and counts: item i's first
    offsets[i+1] - offsets[i] candidates at offsets[i], the fill everywhere else"""
    items, offsets = np.asarray(items, np.uint32), np.asarray(offsets, np.uint64).astype(np.int64)
    ids, sc = np.full(int(offsets[-1]) + pad, fill_id, np.uint32), np.full(int(offsets[-1]) + pad, fill_score, np.float64)
    cnt = np.zeros(items.size, np.uint32)
    caps = np.diff(offsets)
    for a in np.unique(items).tolist():
        for i in np.flatnonzero(items == a).tolist():
            wi, ws = model.neighbours(a, int(caps[i]))
            ids[offsets[i]:offsets[i] + wi.size], sc[offsets[i]:offsets[i] + wi.size], cnt[i] = wi, ws, wi.size
    return ids, sc, cnt


def expected_topk(model, items, k, fill_id, fill_score):
    """what smatrix_cf_topk_batch leaves in ids / scores [n, k] and counts"""
    items = np.asarray(items, np.uint32)
    ids, sc, cnt = np.full((items.size, k), fill_id, np.uint32), np.full((items.size, k), fill_score, np.float64), np.zeros(items.size, np.uint32)
    for a in np.unique(items).tolist():
        wi, ws = model.topk(a, k)
        at = np.flatnonzero(items == a)
        ids[at, :wi.size], sc[at, :wi.size], cnt[at] = wi, ws, wi.size
    return ids, sc, cnt


def assert_same(got, want, tag):
    """(ids, scores, counts) against the expected arrays, byte for byte; names the first entry that differs"""
    for name, g, w in zip(("counts", "ids", "scores"), (got[2], got[0], got[1]), (want[2], want[0], want[1])):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            gv, wv = (g.view(np.uint64), w.view(np.uint64)) if g.dtype == np.float64 else (g, w)
            at = np.argwhere(gv != wv)[0].tolist()
            raise AssertionError((tag, name, "first difference at", at, "got", g[tuple(at)], "want", w[tuple(at)],
                                  "entries that differ", int((gv != wv).sum())))


# ---- the guards matrix ------------------------------------------------------------------------------------------------------------
# Every pair once, as SET ops in the order the scalar build issues them, then two decrements.  Totals (the head pair (x, 0)):
#   0     49: row 0 is an item, and get(0, 0) != 0 is the total of every other item's (0, total) entry -- item A's scores 25 / (5 * 7)
#   A     25    B 4 (its head set AFTER its pairs: the key-0 cell is not cell 0)    C 9    D 2, E 3, F 2, G 8: the two-step pairs
#   NOROW no row at all: tb == 0 counted as 1         NOHEAD a row of pairs without a head: ta == 0, and tb == 0 as a neighbour
#   Z     head 5, decremented to 0 afterwards: its key-0 cell is an empty cell again and leaves the list; ta == 0
#   DEADC column of a pair set to 4 and decremented by 4: a dead cell (key, 0), a candidate with score 0
#   HI = 2^31 and TOP = 2^32 - 2 with the total 2^32 - 1;  FF = 2^32 - 1, item and neighbour, total 16;  HI1 = 2^31 + 1, total 1
FF, HI, HI1, TOP = 0xFFFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE
A, B, C, D, E, F, G, NOROW, NOHEAD, Z, DEADC, ONLY_HEAD = 100, 101, 102, 103, 104, 110, 111, 105, 106, 107, 108, 112
GUARD_ABSENT = 424242
GUARD_SETS = [
    (0, 0, 49), (0, A, 10), (0, B, 3), (0, FF, 7), (0, NOROW, 2), (0, HI, 1),
    (A, 0, 25), (A, B, 7), (A, C, 15), (A, D, 99), (A, NOROW, 3), (A, Z, 2), (A, A, 5), (A, DEADC, 4), (A, FF, 8), (A, HI, 1), (A, NOHEAD, 1),
    (B, C, 6), (B, A, 11), (B, B, 4), (B, FF, 1), (B, ONLY_HEAD, 2), (B, 0, 4),
    (C, 0, 9),
    (D, 0, 2), (D, E, 1), (D, F, 2), (D, G, 4), (D, D, 1), (D, C, 5),
    (E, 0, 3), (E, D, 2), (F, 0, 2), (F, D, 1), (G, 0, 8), (G, D, 3), (G, F, 4),
    (NOHEAD, A, 3), (NOHEAD, B, 1), (NOHEAD, FF, 2), (NOHEAD, NOROW, 1),
    (Z, 0, 5), (Z, A, 2), (Z, C, 1), (Z, Z, 1),
    (HI, 0, FF), (HI, TOP, FF), (HI, HI, TOP), (HI, A, 3), (HI, HI1, 65535), (HI, FF, 262143), (HI, NOROW, 65536),
    (TOP, 0, FF), (TOP, HI, 1), (TOP, FF, FF),
    (FF, 0, 16), (FF, A, 20), (FF, FF, 3), (FF, HI, 2), (FF, NOROW, 4), (FF, DEADC, 5),
    (HI1, 0, 1), (HI1, NOROW, 1), (HI1, C, 2), (HI1, HI1, 1),
    (ONLY_HEAD, 0, 7),
]
GUARD_DECRS = [(A, DEADC, 4), (Z, 0, 5)]
GUARD_ITEMS = [0, A, B, C, D, E, F, G, NOROW, NOHEAD, Z, DEADC, HI, TOP, FF, HI1, ONLY_HEAD, GUARD_ABSENT, A, FF]


def build_scalar(m):
    """the guards matrix by one scalar call per op: works on an Oracle, a Reference, a SparseMatrix or a tests.gpu_adapter.GpuMatrix"""
    for x, y, v in GUARD_SETS:
        m.set(x, y, v)
    for x, y, v in GUARD_DECRS:
        m.decr(x, y, v)
    return m


def build_batch(m):
    """the same contents into a SparseMatrix by one set_batch (and the two decrements as one batch behind it): any layout may result"""
    x, y, v = (np.array(c, np.uint32) for c in zip(*GUARD_SETS))
    m.set_batch(x, y, v)
    x, y, v = (np.array(c, np.uint32) for c in zip(*GUARD_DECRS))
    m.decr_batch(x, y, v)
    return m


def guard_facts(model):
    """the properties the guards matrix exists for, each as the list of (item, neighbour) pairs of GUARD_ITEMS that show it"""
    f = {k: [] for k in ("val>den", "val==den", "two_step", "tb==0", "ta==0", "dead", "self", "ff_item", "ff_neighbour", "high_id",
                         "total_ff", "val_ff", "head_entry_scores")}
    for a in dict.fromkeys(GUARD_ITEMS):
        c = model.candidates(a)
        raw_tb = np.asarray(model.total_of(c.id), np.uint32) if len(c) else np.zeros(0, np.uint32)
        one = np.sqrt(np.float64(c.ta) * c.tb.astype(np.float64))                 # the OTHER denominator: one root of the product
        for i in range(len(c)):
            b, v, pair = int(c.id[i]), float(c.val[i]), (a, int(c.id[i]))
            if v > c.den[i]:
                f["val>den"].append(pair)
            if v == c.den[i] and c.score[i] == 1.0:
                f["val==den"].append(pair)
            alt = v / one[i] if one[i] != 0.0 and not v > one[i] else 0.0
            if bits(one[i:i + 1])[0] != bits(c.den[i:i + 1])[0] and bits([alt])[0] != bits(c.score[i:i + 1])[0]:
                f["two_step"].append(pair)
            if raw_tb[i] == 0 and b != 0 and c.score[i] > 0.0:
                f["tb==0"].append(pair)
            if c.ta == 0:
                f["ta==0"].append(pair)
            if b != 0 and v == 0:
                f["dead"].append(pair)
            if b == a:
                f["self"].append(pair)
            if a == FF:
                f["ff_item"].append(pair)
            if b == FF:
                f["ff_neighbour"].append(pair)
            if b >= 1 << 31 or a >= 1 << 31:
                f["high_id"].append(pair)
            if raw_tb[i] == FF or c.ta == FF:
                f["total_ff"].append(pair)
            if c.val[i] == FF:
                f["val_ff"].append(pair)
            if b == 0 and a != 0 and c.score[i] > 0.0:
                f["head_entry_scores"].append(pair)
    return f
