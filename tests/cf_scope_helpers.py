"""The model of smatrix_cf_recommend_scoped (include/smatrix_batch.h) and the data its tests run on, for tests/test_cf_scope_model.py
and tests/test_gpu_cf_recommend_scoped.py (a plain module, no tests of its own).

The model IS the header's equivalence: cf_group_fill_helpers.grouped_filled() -- cf_sim_helpers.SessionModel.ranking, the quotas'
closed form, the serial fill walk -- with the session's exclusion list extended by every id that is not allowed for it.  listed() and
allowed() state the contract in their own few lines; nothing is taken from the library.
The matrix is the world of tests/cf_sim_helpers.py.  scope_map() puts every id the tests can meet -- candidates, session items, the
fill list's ids -- into a "category"; universe() is the set of ids over which "every id that is not allowed" is taken."""
import functools

import numpy as np

from tests import cf_fill_helpers as F
from tests import cf_group_fill_helpers as GF
from tests import cf_group_helpers as G
from tests import cf_sim_helpers as H

NONE = G.GROUP_NONE
ONLY, EXCEPT = 0, 1
MODES = {"only": ONLY, "except": EXCEPT}
SCOPE_MAX = 64


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def group_of(arr, scope_n, b):
    """g(b): the map's entry for b < scope_n, else NONE (arr may be longer than scope_n: the call is given a prefix of it)"""
    return int(arr[b]) if arr is not None and b < scope_n else NONE


def listed(arr, scope_n, lst, b):
    g = group_of(arr, scope_n, b)
    return g != NONE and any(g == int(v) for v in lst)


def allowed(arr, scope_n, lst, mode, b):
    if len(lst) == 0:
        return True                                                       # unscoped, in both modes
    return listed(arr, scope_n, lst, b) == (mode == ONLY)


def not_allowed(arr, scope_n, lst, mode, ids):
    """the ids of `ids` that session's scope keeps from it, ascending"""
    return sorted(int(b) for b in set(int(v) for v in ids) if not allowed(arr, scope_n, lst, mode, b))


def scoped(model, sess, k, sim, shrink, arr, scope_n, lst, mode, universe, group_map=None, cap=64, fill=(), w=None, excl=(), deny=()):
    """-> (ids, scores float64, n_scored): the grouped fill model under the extended exclusion list"""
    more = list(excl) + not_allowed(arr, scope_n, lst, mode, universe)
    return GF.grouped_filled(model, sess, k, sim, shrink, group_map, cap, fill, w, more, deny)


# ---- the data ------------------------------------------------------------------------------------------------------------------------
N_CAT = 7                                                   # categories 0 .. 6 by id % 7, but for the overrides of scope_map()
FR = F.FRESH
SCOPE_N = FR[120] + 1                                       # the map's end: FR[120] is its last id, FR[121:] lie beyond it


@functools.lru_cache(maxsize=None)
def universe():
    """every id a scoped test can meet as a candidate or in a fill list: the world's columns and rows, and the lists' ids"""
    x, y, _ = H.world_contents()
    ids = set(x.tolist()) | set(y.tolist()) | set(GF.fill_list()) | set(F.fill_list()) | set(FR) | {H.ABSENT}
    ids.discard(0)
    return sorted(ids)


@functools.lru_cache(maxsize=None)
def scope_map():
    """uint32[SCOPE_N]: id b -> b % 7; ids 50300 .. 50319 (POOL ids without rows, the best of many rankings) and FR[5] are named NONE;
    the SMALL ids 300 .. 355 alternate between the categories 100 and 0xFFFFFFFE; FR[100 .. 120] are category 200.  H.ABSENT and
    FR[121:] lie beyond the end"""
    m = (np.arange(SCOPE_N, dtype=np.uint64) % N_CAT).astype(np.uint32)
    m[50300:50320] = NONE
    m[FR[5]] = NONE
    m[H.SMALL] = np.where(H.SMALL % 2 == 0, 100, 0xFFFFFFFE).astype(np.uint32)
    m[FR[100]:FR[120] + 1] = 200
    return m


def scope_lists(sessions, seed=5):
    """one list per session: session i is unscoped for i % 4 == 0; the others list 1 .. 4 categories, some with a repeat, a NONE or a
    group nobody has"""
    rng = np.random.default_rng(seed)
    out = []
    for i, _ in enumerate(sessions):
        if i % 4 == 0:
            out.append([])
            continue
        lst = rng.choice([0, 1, 2, 3, 4, 5, 6, 100, 0xFFFFFFFE, 200], int(rng.integers(1, 5)), replace=False).tolist()
        if i % 3 == 0:
            lst.append(lst[0])                                            # a repeat
        if i % 5 == 0:
            lst.insert(0, NONE)                                           # matches nothing
        if i % 7 == 0:
            lst.append(77777)                                             # a group without ids
        out.append([int(v) for v in lst])
    return out
