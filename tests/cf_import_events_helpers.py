"""The model of smatrix_cf_import_events (include/smatrix_batch.h) in plain Python loops, and what its tests share: the sessions, the
comparison of a GPU matrix with an oracle, row by row (a plain module, no tests of its own)."""
import numpy as np

FORWARD, NO_SELF = 1, 2                  # SMATRIX_IMPORT_FORWARD, SMATRIX_IMPORT_NO_SELF
OP_SET, OP_INCR, OP_DECR = 1, 2, 3


def model_ops(sessions, amounts=None, window=0, flags=0):
    """Session s is the positions p = 0 .. L-1 of its ids; its amounts are w_p = amounts[s][p], or 1 everywhere with amounts None.
    The call applies, each exactly once:
      head op   for every position p with w_p != 0:  op(id_p, 0, w_p).
      pair op   for every ordered pair of positions (p, q), p != q, with w_p != 0 and w_q != 0:  op(id_p, id_q, min(w_p, w_q)),
                provided that ALL of
                  window == 0 (no limit) or |p - q| <= window.  Distances are counted in positions; a position of amount 0 still
                      occupies its place;
                  with FORWARD, q > p: row a then holds what came AFTER a.  Without the flag both directions are applied;
                  with NO_SELF, id_p != id_q.  Without it an id that occurs twice counts against itself.
    An id of 0 is not special-cased.  -> the list of (x, y, v)"""
    ops = []
    for s, ids in enumerate(sessions):
        L = len(ids)
        w = [1] * L if amounts is None else [int(a) for a in amounts[s]]
        assert len(w) == L
        for p in range(L):
            if w[p] == 0:
                continue
            ops.append((int(ids[p]), 0, w[p]))
            for q in range(L):
                if q == p or w[q] == 0:
                    continue
                if window != 0 and abs(p - q) > window:
                    continue
                if (flags & FORWARD) and not q > p:
                    continue
                if (flags & NO_SELF) and ids[p] == ids[q]:
                    continue
                ops.append((int(ids[p]), int(ids[q]), min(w[p], w[q])))
    return ops


def apply_model(o, ops, op=OP_INCR):
    """the ops applied to an Oracle one by one: INCR in the model's order, DECR with the pair ops first and the head ops after
    them, the order the call promises for it (a head cell that reaches 0 is the empty slot, quirk Q3: it cuts the probe chains of
    its row, and a pair op applied after it would make a second cell)"""
    if op == OP_DECR:
        ops = [t for t in ops if t[1] != 0] + [t for t in ops if t[1] == 0]
    if ops:
        x, y, v = (np.array(c, np.uint32) for c in zip(*ops))
        o.apply(op, x, y, v)


def cells(slots):
    """the sorted non-empty {key, value} cells of a row's raw slots"""
    a = np.asarray(slots)
    a = a[(a[:, 0] != 0) | (a[:, 1] != 0)]
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def assert_rows_equal(g, o):
    """for every row the oracle lists the sorted non-empty cells are equal, and the row counts are (never rowlen: quirk Q2)"""
    rows = o.list_rows()
    assert g.stats()["rows"] == rows.size
    for r in rows.tolist():
        a, b = cells(g.row_slots(r)), cells(o.row_slots(r))
        assert a.shape == b.shape and (a == b).all(), r


SPECIAL = [[], [7], [9, 9], [3, 5, 3]]


def parity_sessions():
    """about 300 random sessions of 0..12 ids below 400, the four special ones, and one session of 40 distinct ids"""
    rng = np.random.default_rng(47)
    sessions = [list(s) for s in SPECIAL]
    for _ in range(300):
        sessions.append(rng.integers(1, 400, int(rng.integers(0, 13))).tolist())
    sessions.append((rng.choice(399, 40, replace=False) + 1).tolist())
    return sessions


def random_amounts(sessions, seed=53):
    """amounts in 0..3 per position, zeros present"""
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 4, len(s)).tolist() for s in sessions]
    assert any(0 in a for a in out)
    return out


def write_path_sessions():
    """the inputs of tests/test_gpu_parity.py::test_cf_recommender_write_path_on_device"""
    rng = np.random.default_rng(31)
    sessions = [[], [7], [9, 9], [3, 5, 3]]
    for _ in range(3000):
        L = int(rng.integers(0, 13))
        sessions.append((rng.integers(1, 400, L)).tolist())
    sessions.append((rng.choice(5000, 40, replace=False) + 1000).tolist())
    return sessions
