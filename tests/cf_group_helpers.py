"""The model of smatrix_cf_recommend_grouped (include/smatrix_batch.h) and the group maps its tests run on, for
tests/test_cf_group_model.py and tests/test_gpu_cf_recommend_grouped.py (a plain module, no tests of its own).

grouped()   cf_sim_helpers.SessionModel.ranking, then the CLOSED FORM of the contract: a grouped candidate survives iff fewer than cap
            candidates of its own group precede it in the ranking -- counted over ALL that precede it, taken or not, with no walk and
            no running result --, and the result is the first k survivors.
cases()     the maps (a) .. (h) of the issue over the world of tests/cf_sim_helpers.py, each a dict: name, group_of (an array or a
            dict, as SparseMatrix.cf_recommend_grouped takes them), cap, k, and the exclusion lists / deny list that go with it."""
import functools

import numpy as np

from tests import cf_sim_helpers as H

GROUP_NONE = 0xFFFFFFFF
LDS_SESSION = [10, 11, 12, 11]                              # 217 candidates, all POOL ids
TIE_SESSION = [17, 60003, 14]                               # row 14's 40 columns tie
N_IDS = 140000                                              # above every candidate id of the world


def as_array(group_of):
    """a map as the C call takes it: None -> None, a dict -> uint32 array with GROUP_NONE in the gaps"""
    if group_of is None or len(group_of) == 0:
        return None
    if not isinstance(group_of, dict):
        return np.ascontiguousarray(group_of, dtype=np.uint32)
    out = np.full(max(group_of) + 1, GROUP_NONE, np.uint32)
    for b, g in group_of.items():
        out[b] = g
    return out


def group_of_id(arr, b):
    return GROUP_NONE if arr is None or b >= arr.size else int(arr[b])


def survivors(ranking, arr, cap):
    """the indices into ranking of the candidates that survive, by the closed form"""
    g = np.array([group_of_id(arr, b) for b, _ in ranking], np.uint64)
    order = np.argsort(g, kind="stable")                                  # by group, ranking order inside a group
    gs = g[order]
    first = np.flatnonzero(np.concatenate(([True], gs[1:] != gs[:-1]))) if gs.size else np.zeros(0, np.int64)
    before = np.empty(g.size, np.int64)                                   # candidates of the own group that precede
    before[order] = np.arange(gs.size) - np.repeat(first, np.diff(np.concatenate((first, [gs.size]))))
    return np.flatnonzero((g == GROUP_NONE) | (before < cap))


def grouped(model, sess, k, sim, shrink, group_of, cap, w=None, excl=(), deny=()):
    """-> (ids, scores float64, the indices of the ids in the unconstrained ranking)"""
    r = model.ranking(sess, sim, shrink, w, excl, deny)
    at = survivors(r, as_array(group_of), cap)[:k]
    return [r[i][0] for i in at], np.array([r[i][1] for i in at], np.float64), at.tolist()


@functools.lru_cache(maxsize=None)
def cpu_model():
    """the SessionModel of the world's contents, without a GPU"""
    return H.SessionModel(H.sorted_export_of(H.world_contents()))


@functools.lru_cache(maxsize=None)
def cases():
    m = cpu_model()
    n = len(H.all_sessions())
    lds = [b for b, _ in m.ranking(LDS_SESSION, H.SIM_COSINE, 0.0)]
    hot = [b for b, _ in m.ranking([H.HOT], H.SIM_COSINE, 0.0)]
    out = []
    # (a) the best 64 of the LDS session in three groups, the rest in groups of twenty consecutive ranks
    out.append(dict(name="a", group_of={b: (i % 3 if i < 64 else 100 + i // 20) for i, b in enumerate(lds)}, cap=1, k=10))
    # (b) the hot session: one group but for the last twenty of its ranking, alternately ungrouped and in groups of their own
    g = np.full(N_IDS, 7, np.uint32)
    for i, b in enumerate(hot[-20:]):
        g[b] = GROUP_NONE if i % 2 else 1000 + i
    out.append(dict(name="b", group_of=g, cap=1, k=10))
    # (c) row 14's tied columns in two alternating groups
    out.append(dict(name="c", group_of={int(b): 5 + i % 2 for i, b in enumerate(H.TIE_COLUMNS)}, cap=3, k=10))
    # (d) every id in one group
    out.append(dict(name="d", group_of=np.full(N_IDS, 9, np.uint32), cap=2, k=10))
    # (e) two groups of the LDS session whose best are excluded (the session's list) and denied (everybody's)
    ge = {lds[0]: 21, lds[5]: 21, lds[9]: 21, lds[1]: 22, lds[6]: 22, lds[11]: 22}
    excl = [[lds[0]] if s == LDS_SESSION else [] for s in H.all_sessions()]
    out.append(dict(name="e", group_of=ge, cap=1, k=10, exclude=excl, deny=[lds[1]]))
    # (f) a map that ends at 50350, among the ids without a row that lead the rankings: ids below 50300 in group 2, 50300 .. 50324
    # GROUP_NONE, 50325 .. 50349 in group 1, the rest beyond it
    g = np.full(50350, 2, np.uint32)
    g[50300:50325] = GROUP_NONE
    g[50325:] = 1
    out.append(dict(name="f", group_of=g, cap=1, k=10))
    # (g) 97 groups, one result each, k = 64
    out.append(dict(name="g", group_of=(np.arange(N_IDS, dtype=np.uint64) % 97).astype(np.uint32), cap=1, k=64))
    # (h) the group ids 0 and 0xFFFFFFFE
    out.append(dict(name="h", group_of=np.where(np.arange(N_IDS) % 2 == 0, 0, 0xFFFFFFFE).astype(np.uint32), cap=2, k=10))
    for c in out:
        c.setdefault("exclude", None)
        c.setdefault("deny", None)
        assert c["exclude"] is None or len(c["exclude"]) == n
    return out


def case(name):
    return next(c for c in cases() if c["name"] == name)
