"""CPU: the data of tests/test_gpu_cf_popular.py and tests/test_gpu_cf_recommend_fill.py has the hard cases those tests are about,
shown with the models of tests/cf_fill_helpers.py alone (no library call)."""
import numpy as np
import pytest

from tests import cf_fill_helpers as F
from tests import cf_sim_helpers as H

K = 10


@pytest.fixture(scope="module")
def model():
    return H.SessionModel(H.sorted_export_of(H.world_contents()))


# ---- the popular call's matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [False, True])
def test_the_cuts_at_64_and_4096_fall_inside_a_tie_group(small):
    w = F.popular_world(small)
    ids, tot = F.popular(F.export_of_totals(w["totals"]), F.N_ROWS + 10)
    assert ids.size == F.N_ROWS and 0 not in ids.tolist()                 # row 0 has a head and is no candidate
    for n in (64, 4096):
        assert tot[n - 1] == tot[n] and ids[n - 1] < ids[n], n             # the ascending id decides
    assert (np.diff(tot.astype(np.int64)) <= 0).all()
    groups = np.unique(tot[tot <= 50], return_counts=True)[1]
    assert groups.size == 50 and groups.min() > 100                       # large tie groups


def test_the_ids_are_scattered_over_32_bits_and_the_totals_over_all_bytes():
    w = F.popular_world(False)
    ids = np.array(list(w["totals"]), np.uint64)
    assert 0xFFFFFFFF in w["totals"] and 0 in w["totals"] and (ids >= 1 << 31).sum() > 1000 and (ids < 1 << 16).sum() < 10
    tot = np.array(list(w["totals"].values()), np.uint64)
    assert (tot >= 1 << 24).sum() >= 5 and (tot == 0xFFFFFFFF).sum() == 1  # the select starts at the top byte
    small = np.array(list(F.popular_world(True)["totals"].values()))
    assert small[small != 1000].max() < 256                               # ... and at byte 4 (row 0's 1000 is no candidate's)
    x, y, v = w["ops"]
    assert len(set(zip(x.tolist(), y.tolist()))) == x.size                # every (x, y) once
    heads = set(x[y == 0].tolist())
    assert not heads & set(w["no_head"]) and not heads & set(w["empty"])
    assert set(w["zeroed"][0].tolist()) <= heads and not set(w["zeroed"][0].tolist()) & set(w["totals"])


def test_min_total_and_a_deny_list_cut():
    w = F.popular_world(False)
    ex = F.export_of_totals(w["totals"])
    top = F.popular(ex, 4096, min_total=50)
    assert 100 < top[0].size < 4096 and top[1].min() == 50
    deny = top[0][::2].tolist()
    got = F.popular(ex, 4096, deny=deny, min_total=50)
    assert got[0].tolist() == top[0][1::2].tolist()


# ---- the fill call's sessions and list -----------------------------------------------------------------------------------------------
def test_the_list_holds_every_kind_of_id():
    lst = F.fill_list()
    assert len(lst) == 200 and F.FILL_LENGTHS == [1, 63, 64, 65, 200]
    sess_items = set(a for s, _ in F.FILL_SESSIONS for a in s)
    assert 0 in lst and sess_items & set(lst) and set(F.LONG_EXCL) & set(lst) and set(F.DENY) & set(lst)
    assert set(F.row_columns(F.SHORT_ROW)) & set(lst)                     # ids that are scored results of [SHORT_ROW]
    first = lst[:64]
    assert any(first.count(f) > 1 for f in first if f)                    # a repeat inside one step of 64
    assert any(f and f in first for f in lst[64:128]) and any(f and f in lst[:128] for f in lst[128:])        # ... and across steps
    rows = set(H.world_contents()[0].tolist())
    assert any(f not in rows for f in lst) and any(f in rows for f in lst)


@pytest.mark.parametrize("deny", [(), F.DENY])
def test_the_fill_sessions_are_short_and_the_others_are_not(model, deny):
    for sess, excl in F.FILL_SESSIONS:
        assert len(model.ranking(sess, H.SIM_COSINE, 0.0, None, excl, deny)) < K, sess[:4]
    assert len(F.ROWLESS) > 64 and len(set(F.ROWLESS)) == len(F.ROWLESS) and len(F.LONG_EXCL) == 300
    assert sum(len(model.ranking(s, H.SIM_COSINE, 0.0, None, (), deny)) > K for s in H.lds_sessions()) >= 3
    assert all(len(model.ranking(s, H.SIM_COSINE, 0.0, None, (), deny)) > 64 for s in H.global_sessions())


def test_a_global_tier_session_is_denied_down_to_fewer_than_k(model):
    deny = F.heavy_deny()
    for sess in ([H.HOT], [H.HOT, 301, 302]):
        full, left = model.ranking(sess, H.SIM_COSINE, 0.0), model.ranking(sess, H.SIM_COSINE, 0.0, None, (), deny)
        assert len(full) > 4900 and 0 < len(left)
    assert len(model.ranking([H.HOT], H.SIM_COSINE, 0.0, None, (), deny)) == 3


def test_one_list_is_too_short_and_one_ends_in_the_middle_of_a_step(model):
    lst = F.fill_list()
    empty = lambda n, k: F.filled(model, [], k, H.SIM_COSINE, 0.0, lst[:n], None, (), F.DENY)      # noqa: E731
    assert len(empty(1, K)[0]) == 0                                       # the list [0]: nothing to take
    ids = empty(63, K)[0]
    assert len(ids) == K
    last = lst.index(ids[-1])
    assert last < 62 and len(F.fill([], 0, [], (), F.DENY, lst[last + 1:63], 64)) > 5      # takeable ids behind the cut, in the same step
    ids64 = empty(200, 64)[0]
    assert len(ids64) == 64 and 64 < lst.index(ids64[-1]) < 127            # k = 64: the cut falls in the second step
    assert len(empty(65, 64)[0]) < 64                                     # ... and 65 ids are too few
    for sess, excl in F.FILL_SESSIONS:                                    # every session fills up from the whole list
        assert len(F.filled(model, sess, K, H.SIM_COSINE, 0.0, lst, None, excl, F.DENY)[0]) == K
