"""The models of smatrix_cf_popular and smatrix_cf_recommend_fill (include/smatrix_batch.h), and the data their tests run on, for
tests/test_cf_fill_model.py, tests/test_gpu_cf_popular.py and tests/test_gpu_cf_recommend_fill.py (a plain module, no tests of its
own).

popular()   the candidates of a matrix's export("sorted") -- the head pairs (column 0) with x != 0, a total >= max(min_total, 1) and
            an id that is not denied -- by (total descending, id ascending), cut at n.
fill()      a scored result of cf_sim_helpers.SessionModel.session with its free places filled from a list, in list order.
The fill call's matrix is the world of tests/cf_sim_helpers.py; the popular call's is popular_world()."""
import numpy as np

from tests import cf_sim_helpers as H


# ---- the models ----------------------------------------------------------------------------------------------------------------------
def heads_of(export_sorted):
    """export("sorted") -> (ids, totals) of the head pairs, in the export's order"""
    rows, row_ptr, pairs = export_sorted
    x = np.repeat(rows, np.diff(row_ptr.astype(np.int64)))
    sel = pairs[:, 0] == 0
    return x[sel].astype(np.uint32), pairs[sel, 1].astype(np.uint32)


def popular(export_sorted, n, deny=(), min_total=1):
    """-> (ids uint32[n_found], totals uint32[n_found]), best first"""
    ids, tot = heads_of(export_sorted)
    keep = (ids != 0) & (tot >= max(int(min_total), 1)) & ~np.isin(ids, np.asarray(list(deny), np.uint32))
    ids, tot = ids[keep], tot[keep]
    order = np.lexsort((ids, -tot.astype(np.int64)))[:n]
    return ids[order], tot[order]


def fill(result_ids, n_scored, session, exclude, deny, fill_ids, k):
    """the first n_scored ids of a result, then the ids of fill_ids in list order that are not 0, not an item of the session, not
    excluded, not denied and not in the result already, up to k -> the list of ids"""
    out = [int(b) for b in result_ids[:n_scored]]
    gone = set(int(a) for a in session) | set(int(a) for a in exclude) | set(int(a) for a in deny) | {0}
    for f in (int(v) for v in fill_ids):
        if len(out) >= k:
            break
        if f not in gone and f not in out:
            out.append(f)
    return out


def filled(model, sess, k, sim, shrink, fill_ids, w=None, excl=(), deny=()):
    """SessionModel.session, then fill() -> (ids, scores float64, n_scored)"""
    ids, sc = model.session(sess, k, sim, shrink, w, excl, deny)
    out = fill(ids, len(ids), sess, excl, deny, fill_ids, k)
    return out, np.concatenate([sc, np.zeros(len(out) - len(ids))]), len(ids)


# ---- the fill call's sessions and list, over the world of cf_sim_helpers ----------------------------------------------------------------
DENY = [H.HOT, 302, H.NO_ROW_COLUMN] + list(range(50001, 50400, 5)) + list(range(70001, 90000, 3))     # tests/test_gpu_cf_rank.py's
ROWLESS = list(range(900000, 900070))                       # more than 64 distinct ids without rows
LONG_EXCL = list(range(910000, 910300))
FRESH = list(range(920000, 920200))                         # ids the matrix has never seen
SHORT_ROW = 10                                              # a row of 5 pairs
# (session, exclusion list): each is left with fewer than 10 candidates
FILL_SESSIONS = [([], []), ([H.ABSENT, 987654322], []), ([SHORT_ROW], []), (ROWLESS, LONG_EXCL), ([SHORT_ROW, 0, SHORT_ROW, H.ABSENT], [])]
FILL_LENGTHS = [1, 63, 64, 65, 200]


def row_columns(a):
    x, y, _ = H.world_ops()
    return y[(x == a) & (y != 0)].tolist()


def fill_list():
    """200 ids: the id 0, session items, excluded ids, denied ids, ids that are scored results of [SHORT_ROW], repeats inside the first
    64 and across steps, ids absent from the matrix, ids with rows"""
    head = [0, SHORT_ROW, H.ABSENT, ROWLESS[3], LONG_EXCL[0], DENY[0], DENY[4]] + row_columns(SHORT_ROW)[:3]
    head += [FRESH[0], FRESH[0], FRESH[1], 0, 300, FRESH[1], ROWLESS[65], LONG_EXCL[299], 301, H.NO_HEAD_ITEM]
    body = FRESH[2:30] + [11, 12, 305] + FRESH[30:44]                      # up to entry 65
    tail = [FRESH[0], FRESH[2], 300, 0, DENY[1]] + FRESH[44:100] + [FRESH[50], LONG_EXCL[7]] + FRESH[100:130] + [FRESH[3], FRESH[60]] + FRESH[130:170]
    out = head + body + tail
    assert len(out) == 200, len(out)
    return out


def heavy_deny():
    """every column of the hot row but three, and more: a global-tier session is left with fewer than 10 candidates"""
    cols = sorted(row_columns(H.HOT))
    return cols[:1000] + cols[1003:] + [FRESH[5], 302]


# ---- the popular call's matrix ---------------------------------------------------------------------------------------------------------
N_ROWS = 10000


def popular_world(small=False):
    """-> dict: ops (x, y, v) SET ops, every (x, y) once; empty: ids made by the scalar set(x, 0, 0); zeroed: (x, y, v) DECR ops that
    bring a head to 0; totals: {id: total} of every head pair that ends non-zero (row 0's included).
    Totals are drawn from 1 .. 50 -- tie groups of about 200 ids --; the full variant adds a handful >= 2^24 and one 0xFFFFFFFF (the
    select starts at the top byte), the small variant stays below 256 (it starts at byte 4 of 8)."""
    rng = np.random.default_rng(99 if small else 98)
    ids = np.unique(rng.integers(1, 0xFFFFFFFF, N_ROWS + 200, dtype=np.uint64).astype(np.uint32))
    ids = rng.permutation(ids[ids != 0xFFFFFFFF])
    main, no_head, empty, zeroed = ids[:N_ROWS - 1], ids[N_ROWS:N_ROWS + 40], ids[N_ROWS + 40:N_ROWS + 43], ids[N_ROWS + 43:N_ROWS + 48]
    main = np.concatenate([main, np.array([0xFFFFFFFF], np.uint32)])
    tot = rng.integers(1, 51, main.size).astype(np.uint32)
    if small:
        tot[:4] = [255, 255, 254, 200]
    else:
        tot[:6] = [1 << 24, (1 << 24) + 5, 1 << 30, (1 << 31) + 7, 0xFFFFFFFF, 1 << 24]
    pairs = main[::7]
    xs = [main, pairs, np.zeros(2, np.uint32), no_head, zeroed, zeroed]
    ys = [np.zeros(main.size, np.uint32), np.full(pairs.size, 5, np.uint32), np.array([0, 9], np.uint32), np.full(no_head.size, 5, np.uint32),
          np.zeros(zeroed.size, np.uint32), np.full(zeroed.size, 6, np.uint32)]
    vs = [tot, np.full(pairs.size, 3, np.uint32), np.array([1000, 1], np.uint32), np.full(no_head.size, 2, np.uint32),
          np.full(zeroed.size, 7, np.uint32), np.ones(zeroed.size, np.uint32)]
    totals = dict(zip(main.tolist(), tot.tolist()))
    totals[0] = 1000
    return {"ops": tuple(np.concatenate(a).astype(np.uint32) for a in (xs, ys, vs)), "empty": empty.tolist(),
            "zeroed": (zeroed, np.zeros(zeroed.size, np.uint32), np.full(zeroed.size, 7, np.uint32)), "totals": totals,
            "no_head": no_head.tolist()}


def export_of_totals(totals):
    """{id: total} -> an export("sorted") that holds those head pairs and nothing else: what popular() reads of a matrix"""
    ids = np.array(sorted(totals), np.uint32)
    return H.sorted_export_of((ids, np.zeros(ids.size, np.uint32), np.array([totals[int(i)] for i in ids], np.uint32)))
