"""What tests/test_cf_explain_model.py and tests/test_gpu_cf_explain.py share (a plain module, no tests of its own): the expected
answer of smatrix_cf_explain (include/smatrix_batch.h), restated over cf_sim_helpers.SessionModel's rows and totals and
cf_sim_helpers.score, and the inputs the tests ask about.

One entry per (target, session position), session s's block at e_offsets[s], target j's L_s entries at e_offsets[s] + j * L_s.  An
entry is (+0.0, 0) for the target 0, a later occurrence of the position's id, an id without a row, a row without a cell of that key,
and a dead cell; otherwise (w * score, cc), score the two-step score of cf_sim_helpers, the product a float64 of its own, a weight
of -0.0 taken as 0.0."""
import numpy as np

from tests import cf_sim_helpers as H

MEASURES = [("cosine", 0.0), ("cosine", 0.1), ("jaccard", 0.0), ("jaccard", 0.5), ("lift", 0.0), ("lift", 0.5)]


def e_offsets_of(sessions, targets):
    e_off = np.zeros(len(sessions) + 1, np.uint64)
    np.cumsum([len(s) * len(t) for s, t in zip(sessions, targets)], out=e_off[1:])
    return e_off


def cell_of(model, a, t):
    """what smatrix_get(a, t) returns of the model's contents: the value of row a's pair with column t, 0 without one"""
    p = model.row.get(int(a))
    if p is None:
        return 0
    at = np.flatnonzero(p[:, 0] == t)
    return int(p[at[0], 1]) if at.size else 0


def live_entries(model, sessions, targets):
    """the entries that are not zero by rule -> parallel lists (entry, session, position, ta, tb, cc)"""
    e_off = e_offsets_of(sessions, targets)
    out = []
    for s, (sess, tg) in enumerate(zip(sessions, targets)):
        L = len(sess)
        first = first_positions(sess)
        for j, t in enumerate(int(t) for t in tg):
            if t == 0:
                continue
            for i in first:
                cc = cell_of(model, sess[i], t)
                if cc:
                    out.append((int(e_off[s]) + j * L + i, s, i, model.total[int(sess[i])], model.total.get(t, 0), cc))
    return out


def first_positions(sess):
    seen, out = set(), []
    for i, a in enumerate(int(a) for a in sess):
        if a not in seen:
            seen.add(a)
            out.append(i)
    return out


def expected(model, sessions, targets, sim, shrink, weights=None):
    """-> (terms float64[E], cc uint32[E], e_offsets uint64[n + 1]) as SparseMatrix.cf_explain returns them"""
    e_off = e_offsets_of(sessions, targets)
    terms, cc = np.zeros(int(e_off[-1]), np.float64), np.zeros(int(e_off[-1]), np.uint32)
    live = live_entries(model, sessions, targets)
    if live:
        e, s, i, ta, tb, c = (np.array(col) for col in zip(*live))
        sc = H.score(ta.astype(np.uint32), tb.astype(np.uint32), c.astype(np.uint32), H.SIMS[sim], shrink)
        w = np.ones(e.size) if weights is None else np.array([float(weights[a][b]) for a, b in zip(s, i)], np.float64)
        w = np.where(w == 0.0, 0.0, w)                                   # -0.0 acts as 0.0
        terms[e] = w * sc                                                 # one multiply, rounded to float64 on its own
        cc[e] = c
    return terms, cc, e_off


def fold(terms):
    """the left-to-right sum from 0.0, every add a float64 of its own -> its bits"""
    acc = np.float64(0.0)
    for t in np.asarray(terms, np.float64):
        acc = acc + t
    return int(np.float64(acc).view(np.uint64))


def weights_for(sessions):
    """per-position weights with a 0.0, a -0.0 and a 2.5 in every session long enough to hold them, multiples of 1 / 8 up to 4
    elsewhere"""
    rng = np.random.default_rng(97)
    out = []
    for s in sessions:
        w = (rng.integers(1, 33, len(s)) / 8.0).tolist()
        for i, v in zip((2, 1, 0), (-0.0, 0.0, 2.5)):
            if i < len(s):
                w[i] = v
        out.append(w)
    return out


# ---- first positions at every length: sessions across the 64-lane borders of the pre-pass ------------------------------------------
X, Y, Z, V = (int(a) for a in H.SMALL[:4])                      # ids that occur only where long_sessions() puts them
LONG_TARGETS = [H.NO_ROW_COLUMN, int(H.SMALL[10])]              # column 999 is in every SMALL row: every first position has a cc


def long_sessions():
    """sessions of 64, 65, 129 and 8200 ids drawn from SMALL.  Z at 0 and at the last position (64 in the 65-id session, 128 in the
    129-id one, 8199 in the longest: beyond REC_DEDUP_MAX); X at 63 and 64, Y at 127 and 128, V at 8191 and 8192 wherever both
    positions lie before the last one, else at the earlier position alone: a repeat straddles every 64-lane border"""
    rng = np.random.default_rng(5)
    out = []
    for L in (64, 65, 129, 8200):
        s = rng.choice(H.SMALL[4:], L).tolist()
        s[0] = s[L - 1] = Z
        for a, i in ((X, 63), (Y, 127), (V, 8191)):
            if i + 1 < L - 1:
                s[i] = s[i + 1] = a
            elif i < L - 1:
                s[i] = a
        out.append([int(a) for a in s])
    return out
