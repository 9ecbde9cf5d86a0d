"""The model of smatrix_cf_recommend_grouped_fill (include/smatrix_batch.h), the restated step rule of its kernel, and the data its
tests run on, for tests/test_cf_group_fill_model.py and tests/test_gpu_cf_recommend_grouped_fill.py (a plain module, no tests of its own).

walk()            the SERIAL walk of the contract behind a scored result: list order, running per-group counts.
grouped_filled()  cf_group_helpers.grouped(), then walk() -> (ids, scores, n_scored).
step_rule()       kernels/recommend.hpp k_rec_fill_grouped in numpy: the list in steps of 64, a lane per id, every verdict from two counts
                  -- the result's entries of the id's group, and the ok lanes below of it -- with no running state inside a step.
The matrix is the world of tests/cf_sim_helpers.py; the sessions are cf_fill_helpers.FILL_SESSIONS, cf_group_helpers.LDS_SESSION (warm,
cut short by the quotas) and [HOT] under cf_fill_helpers.heavy_deny() (the global tier); group_map() and fill_list() are described where
they are made."""
import functools

import numpy as np

from tests import cf_fill_helpers as F
from tests import cf_group_helpers as G
from tests import cf_sim_helpers as H

NONE = G.GROUP_NONE
K = 10
# (k, cap) of the GPU test's main cases
SHAPES = [(10, 1), (10, 2), (64, 1)]
# the groups of the list's own ids: X fills from two neighbours, Y is group 0 (a POOL id's too), Z holds the repeated id, W the long run
X, Y, Z, W = 1000, 0, 1001, 1003
POOL_GROUPS = (5, 0xFFFFFFFE)                               # POOL id p is in POOL_GROUPS[p % 2], but for the overrides of group_map()
FR = F.FRESH
MAP_END = FR[149] + 1                                       # FR[150:] lie beyond the map's end


# ---- the models ----------------------------------------------------------------------------------------------------------------------
def walk(result_ids, session, exclude, deny, fill_ids, k, arr, cap):
    """the scored ids, then the serial walk over fill_ids -> the list of ids"""
    out = [int(b) for b in result_ids]
    used = {}
    for b in out:
        g = G.group_of_id(arr, b)
        used[g] = used.get(g, 0) + 1
    gone = set(int(a) for a in session) | set(int(a) for a in exclude) | set(int(a) for a in deny) | {0}
    for f in (int(v) for v in fill_ids):
        if len(out) >= k:
            break
        if f in gone or f in out:
            continue
        g = G.group_of_id(arr, f)
        if g != NONE and used.get(g, 0) >= cap:
            continue                                                      # refused by its quota: the walk goes on
        out.append(f)
        used[g] = used.get(g, 0) + 1
    return out


def grouped_filled(model, sess, k, sim, shrink, group_of, cap, fill_ids, w=None, excl=(), deny=()):
    """-> (ids, scores float64, n_scored)"""
    arr = G.as_array(group_of)
    ids, sc, _ = G.grouped(model, sess, k, sim, shrink, arr, cap, w, excl, deny)
    out = walk(ids, sess, excl, deny, fill_ids, k, arr, cap)
    return out, np.concatenate([sc, np.zeros(len(out) - len(ids))]), len(ids)


def step_rule(result_ids, session, exclude, deny, fill_ids, k, arr, cap):
    """the kernel's rule -> the list of ids.  `mine` / `mg` are the result's ids and groups, a step's lanes are numpy arrays of 64"""
    mine = [int(b) for b in result_ids]
    mg = [G.group_of_id(arr, b) for b in mine]
    gone = np.array(sorted(set(int(a) for a in session) | set(int(a) for a in exclude) | set(int(a) for a in deny) | {0}), np.int64)
    fill_ids = np.asarray(list(fill_ids), np.int64)
    lane = np.arange(64)
    for j0 in range(0, fill_ids.size, 64):
        if len(mine) >= k:
            break
        fid = np.zeros(64, np.int64)
        fid[:min(64, fill_ids.size - j0)] = fill_ids[j0:j0 + 64]
        ok = ~np.isin(fid, gone) & ~np.isin(fid, np.array(mine, np.int64))
        ok &= ~((fid[None, :] == fid[:, None]) & (lane[None, :] < lane[:, None])).any(axis=1)      # a lane below holds the same id
        g = np.array([G.group_of_id(arr, int(f)) if o else NONE for f, o in zip(fid, ok)], np.int64)
        in_result = (np.array(mg, np.int64)[None, :] == g[:, None]).sum(axis=1)
        below = ((g[None, :] == g[:, None]) & ok[None, :] & (lane[None, :] < lane[:, None])).sum(axis=1)
        sv = ok & ((g == NONE) | (in_result + below < cap))
        for i in np.flatnonzero(sv)[:k - len(mine)]:                      # numbered behind `have`, cut at the room left
            mine.append(int(fid[i]))
            mg.append(int(g[i]))
    return mine


# ---- the data ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short_row_best():
    """the best candidate of [SHORT_ROW] under cf_fill_helpers.DENY: a POOL id, and a candidate of LDS_SESSION too (row 10 is in it)"""
    return G.cpu_model().ranking([F.SHORT_ROW], H.SIM_COSINE, 0.0, None, (), F.DENY)[0][0]


@functools.lru_cache(maxsize=None)
def hot_left():
    """the three candidates cf_fill_helpers.heavy_deny() leaves to the session [HOT]"""
    return sorted(F.row_columns(H.HOT))[1000:1003]


@functools.lru_cache(maxsize=None)
def group_map():
    """ONE dict {id: group} over the world's candidate ids and FRESH / ROWLESS.  It ends at FR[149]: FR[150:] and H.ABSENT lie beyond the
    map's end; ROWLESS, LONG_EXCL and the ids with rows below 50000 fall into its gaps and FR[5] and two candidates of LDS_SESSION are
    named GROUP_NONE; the group ids 0 (Y) and 0xFFFFFFFE are in use.
      POOL        p -> 5 or 0xFFFFFFFE by p % 2, so a warm session's 217 candidates are cut to a handful; the best candidate of
                  [SHORT_ROW] -> group 0, alone in it among the POOL ids: both sessions that hold row 10 have ONE scored result of group 0
      hot_left()  -> X: the global-tier session's scored results use the quota two list ids want
      FR          X: 10 .. 13; Y: 20 .. 23; Z: 30, 31; W: 40 .. 42 and 50 .. 149; FR[5]: GROUP_NONE; every other FR below 150 a group of its own"""
    m = {int(p): POOL_GROUPS[int(p) % 2] for p in H.POOL}
    m[short_row_best()] = Y
    lds = [b for b, _ in G.cpu_model().ranking(G.LDS_SESSION, H.SIM_COSINE, 0.0, None, (), F.DENY)]
    for b in [b for b in lds if b != short_row_best()][3:8:4]:
        m[b] = NONE
    for b in hot_left():
        m[b] = X
    for i in range(150):
        m[FR[i]] = 2000 + i
    for i in (10, 11, 12, 13):
        m[FR[i]] = X
    for i in (20, 21, 22, 23):
        m[FR[i]] = Y
    m[FR[30]] = m[FR[31]] = Z
    for i in [40, 41, 42] + list(range(50, 150)):
        m[FR[i]] = W
    m[FR[5]] = NONE
    assert max(m) + 1 == MAP_END
    return m


@functools.lru_cache(maxsize=None)
def group_array():
    return G.as_array(group_map())


@functools.lru_cache(maxsize=None)
def lds_refused():
    """the candidates of LDS_SESSION (under DENY) that the quota refuses at cap = 2, best first: refused at cap = 1 as well"""
    r = G.cpu_model().ranking(G.LDS_SESSION, H.SIM_COSINE, 0.0, None, (), F.DENY)
    kept = set(G.survivors(r, group_array(), 2).tolist())
    return [b for i, (b, _) in enumerate(r) if i not in kept]


@functools.lru_cache(maxsize=None)
def fill_list():
    """200 ids, as cf_fill_helpers.fill_list(): the id 0, session items, excluded ids, denied ids, scored results of [SHORT_ROW], repeats
    inside a step and across steps, ids absent from the matrix, ids with rows -- and, by entry:
        0 ..   2   the id 0, SHORT_ROW (an item of three sessions, ungrouped for the others), a denied id
        3 ..   6   candidates the quota refused for LDS_SESSION
        7,   8     FR[10], FR[11] of X side by side: cap = 1 takes the first alone
        9 ..  11   FR[20 .. 22] of Y = group 0: behind one scored result of group 0, cap = 2 takes the first alone
       12 ..  14   FR[30], FR[30], FR[31] of Z: the repeat counts once, so cap = 2 takes FR[30] and FR[31]
       15          FR[22] again: refused by its quota at 11 (behind a scored result of group 0, or at cap = 1), refused again
       16,  17     FR[5] (named GROUP_NONE) and FR[150] (beyond the map's end): never refused
       18,  19     FR[40], FR[41] of W: the group is full from here on at either cap
       20          FR[11] again: cap = 1 refused it at 8
       21 ..  32   ungrouped ids of every kind (absent, in a gap, with a row), excluded and denied ids, 0, three scored results of [SHORT_ROW]
       33 .. 132   FR[50 .. 149] of W: a hundred ids of one full group -- all of step 2 (64 .. 127) yields nothing
      133 .. 137   step 3: X again, FR[22] again, 0, a denied id, Y again
      138 .. 151   FR[151 .. 164], beyond the map's end
      152 .. 166   seven denied ids and eight ids of W again: a session with k = 64 is not full before step 4
      167 .. 187   ids in groups of their own
      188 .. 191   FR[180 .. 183]
      192 .. 199   step 4: X again, W again, two ungrouped ids, two groups of their own, FR[10] again (taken at 7), one ungrouped"""
    step1 = [0, F.SHORT_ROW, F.DENY[0]] + lds_refused()[:4] + [FR[10], FR[11], FR[20], FR[21], FR[22], FR[30], FR[30], FR[31], FR[22], FR[5], FR[150],
                                                               FR[40], FR[41], FR[11]]
    step1 += [H.ABSENT, F.ROWLESS[3], F.LONG_EXCL[0], F.DENY[4], H.NO_HEAD_ITEM, F.LONG_EXCL[299], 0, F.ROWLESS[65], 300] + F.row_columns(F.SHORT_ROW)[:3]
    assert len(step1) == 33, len(step1)
    run = FR[50:150]
    step3 = [FR[12], FR[22], 0, F.DENY[1], FR[23]] + FR[151:165] + F.DENY[5:12] + FR[60:68] + FR[0:5] + FR[6:10] + FR[14:20] + FR[24:30] + FR[180:184]
    step4 = [FR[13], FR[42], FR[187], FR[188], FR[32], FR[33], FR[10], FR[189]]
    out = step1 + run + step3 + step4
    assert len(out) == 200 and len(step1 + run + step3) == 192, len(out)
    return out


def sessions_and_lists():
    """cf_fill_helpers.FILL_SESSIONS and LDS_SESSION among the world's sessions of both tiers -> (sessions, exclusion lists)"""
    q = [(s, []) for s in H.all_sessions()]
    for i, se in enumerate(F.FILL_SESSIONS):
        q.insert(2 + 6 * i, se)
    assert G.LDS_SESSION in [s for s, _ in q]
    return [s for s, _ in q], [e for _, e in q]


HOT_SESSIONS = [[H.HOT], [H.HOT, 301, 302], [300, 301], []]               # with cf_fill_helpers.heavy_deny(): the first is in the global tier
