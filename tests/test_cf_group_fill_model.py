"""CPU, no library call: the step rule of kernels/recommend.hpp k_rec_fill_grouped (cf_group_fill_helpers.step_rule) is the serial walk
of smatrix_cf_recommend_grouped_fill's contract (cf_group_fill_helpers.walk), and the map, the list and the sessions of
tests/test_gpu_cf_recommend_grouped_fill.py hold the hard cases that test is about -- shown with the models alone over the world's known
contents."""
import numpy as np
import pytest

from tests import cf_fill_helpers as F
from tests import cf_group_fill_helpers as GF
from tests import cf_group_helpers as G
from tests import cf_sim_helpers as H

COS = (H.SIM_COSINE, 0.0)
FR = GF.FR


def fill_cases():
    """(session, exclusion list, deny) of every session that is short under the quotas"""
    out = [(s, e, F.DENY) for s, e in F.FILL_SESSIONS] + [(G.LDS_SESSION, [], F.DENY)]
    return out + [(s, [], F.heavy_deny()) for s in GF.HOT_SESSIONS]


def run(sess, excl, deny, k, cap, n_fill=200):
    """-> (ids, n_scored, the list entries of the filled ids)"""
    lst = GF.fill_list()[:n_fill]
    ids, sc, ns = GF.grouped_filled(G.cpu_model(), sess, k, *COS, GF.group_array(), cap, lst, None, excl, deny)
    assert not sc[ns:].any() and sc.size == len(ids)
    return ids, ns, [lst.index(b) for b in ids[ns:]]


def test_the_step_rule_is_the_serial_walk_on_the_tests_data():
    arr, lst = GF.group_array(), GF.fill_list()
    for sess, excl, deny in fill_cases():
        for k, cap in GF.SHAPES + [(1, 1), (64, 2), (63, 3)]:
            scored = G.grouped(G.cpu_model(), sess, k, *COS, arr, cap, None, excl, deny)[0]
            for n_fill in F.FILL_LENGTHS:
                want = GF.walk(scored, sess, excl, deny, lst[:n_fill], k, arr, cap)
                assert GF.step_rule(scored, sess, excl, deny, lst[:n_fill], k, arr, cap) == want, (sess[:4], k, cap, n_fill)


def test_the_step_rule_is_the_serial_walk_on_200_random_cases():
    rng = np.random.default_rng(4711)
    pool = rng.permutation(np.arange(1, 5000))[:300]
    differs_from_plain_fill = 0
    for case in range(200):
        n_groups, cap = int(rng.integers(1, 9)), int(rng.integers(1, 5))
        k, n_fill = int(rng.choice([1, 10, 63, 64])), int(rng.choice([1, 63, 64, 65, 200]))
        arr = np.full(int(rng.integers(2000, 6000)), G.GROUP_NONE, np.uint32)          # some ids beyond the end, some in gaps
        inside = pool[pool < arr.size]
        grouped_ids = inside[rng.random(inside.size) < 0.85]
        arr[grouped_ids] = rng.choice([0, 0xFFFFFFFE, 3, 4, 5, 6, 7, 8][:n_groups], grouped_ids.size)
        sess, excl, deny = (rng.choice(pool, n).tolist() for n in rng.integers(0, 12, 3))
        lst = rng.choice(np.concatenate([pool, [0]]), n_fill).tolist()                  # repeats are the rule
        scored = GF.walk([], sess, excl, deny, rng.permutation(pool).tolist(), int(rng.integers(0, k + 1)), arr, cap)    # a result under the quotas
        want = GF.walk(scored, sess, excl, deny, lst, k, arr, cap)
        assert GF.step_rule(scored, sess, excl, deny, lst, k, arr, cap) == want, case
        g = [G.group_of_id(arr, b) for b in want]
        assert all(g.count(x) <= cap for x in set(g) - {G.GROUP_NONE}) and len(set(want)) == len(want) <= k
        differs_from_plain_fill += want != F.fill(scored, len(scored), sess, excl, deny, lst, k)
    assert differs_from_plain_fill > 50                                   # the quotas bind in the random cases


def test_a_map_that_cannot_bind_gives_the_fill_calls_model():
    m, lst = G.cpu_model(), GF.fill_list()
    for sess, excl, deny in fill_cases():
        for k in (10, 64):
            want = F.filled(m, sess, k, *COS, lst, None, excl, deny)
            for group_of, cap in ((None, 1), ({}, 2), (GF.group_array(), k), (GF.group_map(), 64)):
                got = GF.grouped_filled(m, sess, k, *COS, group_of, cap, lst, None, excl, deny)
                assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2] == want[2], (sess[:4], k, cap)


def test_an_empty_list_gives_the_grouped_calls_model():
    m = G.cpu_model()
    for sess, excl, deny in fill_cases():
        for k, cap in GF.SHAPES:
            want = G.grouped(m, sess, k, *COS, GF.group_array(), cap, None, excl, deny)
            got = GF.grouped_filled(m, sess, k, *COS, GF.group_map(), cap, [], None, excl, deny)
            assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2] == len(want[0])


def test_no_group_exceeds_cap_and_no_refused_candidate_is_ever_filled():
    m, arr = G.cpu_model(), GF.group_array()
    warm = 0
    for sess, excl, deny in fill_cases():
        for k, cap in GF.SHAPES:
            for n_fill in F.FILL_LENGTHS:
                ids, ns, _ = run(sess, excl, deny, k, cap, n_fill)
                g = [G.group_of_id(arr, b) for b in ids]
                assert all(g.count(x) <= cap for x in set(g) - {G.GROUP_NONE}), (sess[:4], k, cap)
                cands = set(b for b, _ in m.ranking(sess, *COS, None, excl, deny))
                assert not cands & set(ids[ns:]), (sess[:4], k, cap)      # a filled id is never one of the session's candidates
                warm += ns < k and len(cands) > ns and bool(cands & set(GF.fill_list()[:n_fill]))
    assert warm >= 10                                                     # ... although candidates were left behind and the list offers them


def test_the_map_has_every_kind_of_entry():
    gm, arr, lst = GF.group_map(), GF.group_array(), GF.fill_list()
    assert len(lst) == 200 and arr.size == GF.MAP_END
    assert any(b >= arr.size for b in lst) and FR[150] >= arr.size and H.ABSENT >= arr.size            # beyond the map's end
    assert gm[FR[5]] == G.GROUP_NONE and sum(v == G.GROUP_NONE for v in gm.values()) == 3              # named GROUP_NONE
    assert arr[F.ROWLESS[65]] == G.GROUP_NONE and F.ROWLESS[65] not in gm                              # ... and in a gap
    assert {0, 0xFFFFFFFE} <= set(gm.values())
    assert set(H.POOL.tolist()) <= set(gm) and set(FR[:150]) <= set(gm) and set(GF.hot_left()) <= set(gm)
    assert [b for b in H.POOL.tolist() if gm[b] == GF.Y] == [GF.short_row_best()]
    from libsmatrix_amd.matrix import _group_map
    assert _group_map(gm).tobytes() == arr.tobytes()


def test_the_list_offers_the_candidates_the_quota_refused():
    m, arr, lst = G.cpu_model(), GF.group_array(), GF.fill_list()
    refused = GF.lds_refused()
    assert len(refused) > 100 and lst[3:7] == refused[:4]
    for k, cap in GF.SHAPES:
        ids, ns, at = run(G.LDS_SESSION, [], F.DENY, k, cap)
        assert ns < k and not set(at) & {3, 4, 5, 6}, (k, cap)             # warm, cut short, and the refused stay refused
        plain = F.filled(m, G.LDS_SESSION, k, *COS, lst, None, [], F.DENY)
        assert plain[2] == k                                              # without quotas the session needs no list at all


def test_the_hard_steps_happen():
    lst = GF.fill_list()
    assert lst[7:9] == [FR[10], FR[11]] and lst[9:12] == FR[20:23] and lst[12:15] == [FR[30], FR[30], FR[31]] and lst[15] == FR[22] and lst[20] == FR[11]
    # two ids of one group inside one step at cap = 1; the repeat of the refused one is refused again
    _, ns, at = run(G.LDS_SESSION, [], F.DENY, 10, 1)
    assert ns == 5 and 7 in at and 8 not in at and 20 not in at
    # three ids of one group at cap = 2 behind ONE scored result of the group; then the repeated id of Z counts once
    ids, ns, at = run([F.SHORT_ROW], [], F.DENY, 10, 2)
    assert [G.group_of_id(GF.group_array(), b) for b in ids[:ns]].count(GF.Y) == 1
    assert 9 in at and 10 not in at and 11 not in at and 12 in at and 13 not in at and 14 in at and len(ids) == 10
    # the empty session takes two of Y; the cut at k = 10 falls inside step 1, with ids that could be taken behind it
    _, ns, at = run([], [], F.DENY, 10, 2)
    assert ns == 0 and {9, 10} <= set(at) and 11 not in at and max(at) < 16 and len(at) == 10
    # k = 64: W fills in step 1 and is offered in steps 2, 3 and 4; step 2 yields nothing; step 4 is reached and still refuses X and W
    for sess, excl, deny in fill_cases():
        ids, ns, at = run(sess, excl, deny, 64, 1)
        if ns >= 10:                                                      # (two of the hot sessions are half full: the cut at 64 falls in step 3)
            assert len(ids) == 64 and 133 <= max(at) < 192, sess[:4]
            continue
        assert not [i for i in at if 33 <= i < 133] and [i for i in at if 128 <= i < 192], sess[:4]
        assert len(ids) < 64 and 192 not in at and 193 not in at and 198 not in at and {194, 195, 199} <= set(at), sess[:4]
        assert 15 not in at and 134 not in at                             # a repeat of a refused id, inside the step and across steps
    assert all(GF.group_array()[b] == GF.W for b in lst[33:133]) and lst[193] == FR[42] and lst[192] == FR[13] and lst[198] == FR[10]


def test_the_global_tier_session_is_left_with_scored_results_of_x():
    m = G.cpu_model()
    for cap in (1, 2):
        ids, ns, at = run([H.HOT], [], F.heavy_deny(), 10, cap)
        assert ns == cap and ids[:ns] == GF.hot_left()[:cap] and len(ids) == 10
        assert 7 not in at and 8 not in at                                # X is full from the scored results
    assert len(m.ranking([H.HOT], *COS, None, (), F.heavy_deny())) == 3


@pytest.mark.parametrize("n_fill,full", [(1, False), (63, True), (64, True), (65, True), (200, True)])
def test_the_list_lengths(n_fill, full):
    for sess, excl, deny in fill_cases():
        ids, ns, _ = run(sess, excl, deny, 10, 1, n_fill)
        assert (len(ids) == 10) == (full or ns == 10), (sess[:4], n_fill)
