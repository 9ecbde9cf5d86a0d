"""CPU: the closed form of smatrix_cf_recommend_scoped (include/smatrix_batch.h) in tests/cf_scope_helpers.py, on the world of
tests/cf_sim_helpers.py: ONLY and EXCEPT, an empty list, SMATRIX_GROUP_NONE in a list, repeats in a list, ids at and beyond scope_n --
and that the map, the lists and the sessions the GPU test uses hold those cases.  The model is checked against a restatement that
filters the finished ranking instead of extending the exclusion list, and against the library's constants."""
import numpy as np
import pytest

from tests import cf_fill_helpers as F
from tests import cf_group_helpers as G
from tests import cf_scope_helpers as S
from tests import cf_sim_helpers as H

ARR, N = S.scope_map(), S.SCOPE_N


def test_the_constants_are_the_librarys():
    import libsmatrix_amd
    assert (libsmatrix_amd.SCOPE_MAX, libsmatrix_amd.SCOPE_ONLY, libsmatrix_amd.SCOPE_EXCEPT) == (S.SCOPE_MAX, S.ONLY, S.EXCEPT)
    assert libsmatrix_amd.GROUP_NONE == S.NONE


def test_listed_and_allowed_are_the_contracts():
    b = 50007                                                             # a POOL id; its category is read from the map
    g = int(ARR[b])
    assert S.listed(ARR, N, [g], b) and not S.listed(ARR, N, [g + 1], b)
    assert S.allowed(ARR, N, [g], S.ONLY, b) and not S.allowed(ARR, N, [g], S.EXCEPT, b)
    assert not S.allowed(ARR, N, [g + 1], S.ONLY, b) and S.allowed(ARR, N, [g + 1], S.EXCEPT, b)
    for mode in (S.ONLY, S.EXCEPT):                                       # an empty list: unscoped in both modes
        assert S.allowed(ARR, N, [], mode, b) and S.allowed(ARR, N, [], mode, 50300) and S.allowed(ARR, N, [], mode, H.ABSENT)
    # an ungrouped id (named NONE, or beyond the map's end) is listed nowhere, not even by a NONE in the list
    for u in (50300, S.FR[5], S.FR[121], H.ABSENT):
        assert S.group_of(ARR, N, u) == S.NONE
        assert not S.listed(ARR, N, [S.NONE, 1], u)
        assert not S.allowed(ARR, N, [S.NONE, 1], S.ONLY, u) and S.allowed(ARR, N, [S.NONE, 1], S.EXCEPT, u)
    assert not S.allowed(ARR, N, [S.NONE], S.ONLY, b) and S.allowed(ARR, N, [S.NONE], S.EXCEPT, b)      # a list of NONE alone matches nothing
    assert S.allowed(ARR, N, [g, g, g], S.ONLY, b) and not S.allowed(ARR, N, [g, 9, g], S.EXCEPT, b)    # repeats change nothing


def test_ids_at_and_beyond_scope_n():
    last, beyond = S.FR[120], S.FR[121]
    assert last == N - 1 and int(ARR[last]) == 200
    assert S.allowed(ARR, N, [200], S.ONLY, last) and not S.allowed(ARR, N, [200], S.ONLY, beyond)
    assert S.allowed(ARR, N - 1, [200], S.EXCEPT, last) and not S.allowed(ARR, N - 1, [200], S.ONLY, last)   # a shorter prefix of the map
    assert all(S.group_of(ARR, 0, b) == S.NONE for b in (1, last, beyond))                                   # scope_n == 0: nobody is grouped
    assert S.not_allowed(ARR, 0, [1, 2], S.ONLY, [5, 6, 7]) == [5, 6, 7] and S.not_allowed(ARR, 0, [1, 2], S.EXCEPT, [5, 6, 7]) == []


@pytest.mark.parametrize("mode", [S.ONLY, S.EXCEPT])
def test_the_model_is_the_filtered_ranking(mode):
    """extending the exclusion list (the header's equivalence) and filtering the finished ranking by allowed() give one result: an
    excluded id contributes nothing but its absence"""
    m = G.cpu_model()
    sessions = H.all_sessions()
    lists = S.scope_lists(sessions)
    cut = 0
    for sess, lst in zip(sessions, lists):
        for sim, shrink in ((H.SIM_COSINE, 0.0), (H.SIM_JACCARD, 10.0)):
            ids, sc, nsc = S.scoped(m, sess, 10, sim, shrink, ARR, N, lst, mode, S.universe())
            want = [(b, s) for b, s in m.ranking(sess, sim, shrink) if S.allowed(ARR, N, lst, mode, b)][:10]
            assert ids == [b for b, _ in want] and nsc == len(want)
            assert sc.tobytes() == np.array([s for _, s in want], np.float64).tobytes()
            cut += ids != [b for b, _ in m.ranking(sess, sim, shrink)[:10]]
    assert cut >= 4                                                       # the scopes change results


def test_the_data_holds_the_cases():
    sessions = H.all_sessions()
    lists = S.scope_lists(sessions)
    assert sum(1 for l in lists if not l) >= 5 and max(len(l) for l in lists) <= S.SCOPE_MAX
    assert any(S.NONE in l for l in lists) and any(len(set(l)) < len(l) for l in lists) and any(77777 in l for l in lists)
    m = G.cpu_model()
    hot = [b for b, _ in m.ranking([H.HOT], H.SIM_COSINE, 0.0)]
    assert any(S.group_of(ARR, N, b) == S.NONE for b in hot[:64])         # ungrouped ids lead a ranking
    assert set(F.fill_list()) <= set(S.universe()) | {0}
    own = [s for s, l in zip(sessions, lists) if l and any(a and not S.allowed(ARR, N, l, S.ONLY, a) for a in s)]
    assert own                                                            # a scoped session holds an item that is out of its scope


def test_a_fill_walks_past_ids_out_of_scope():
    m = G.cpu_model()
    fill = [S.FR[i] for i in range(0, 130)]
    lst = [int(ARR[S.FR[71]])]
    ids, sc, nsc = S.scoped(m, [H.ABSENT], 10, H.SIM_COSINE, 0.0, ARR, N, lst, S.ONLY, S.universe(), fill=fill)
    assert nsc == 0 and len(ids) == 10 and all(int(ARR[b]) == lst[0] for b in ids) and ids[0] > S.FR[0]
    assert ids == [b for b in fill if b < N and int(ARR[b]) == lst[0]][:10]
    ids, _, _ = S.scoped(m, [H.ABSENT], 10, H.SIM_COSINE, 0.0, ARR, N, [200], S.EXCEPT, S.universe(), fill=fill[95:])
    assert ids == fill[95:100] + fill[121:126]                            # FR[100 .. 120] are category 200; FR[121:] are ungrouped and pass
