"""CPU, no library call: what smatrix_cf_recommend_deep's contract ties together, restated on the model alone
(cf_sim_helpers.SessionModel.ranking(...)[:k]) over the world's known contents, and the preconditions that
tests/test_gpu_cf_deep.py relies on: which sessions have how many candidates, and where equal scores straddle a cut, so that a
selection of the k-th best must look at the ids."""
import numpy as np
import pytest

from tests import cf_deep_helpers as D
from tests import cf_sim_helpers as H


def ranking(sess, sim, shrink, **kw):
    return D.cpu_model().ranking(sess, H.SIMS[sim], shrink, **kw)


@pytest.mark.parametrize("sim,shrink", D.MEASURES)
def test_the_three_ties_of_the_contract_hold_on_the_model(sim, shrink):
    m = D.cpu_model()
    for sess in H.all_sessions():
        r = m.ranking(sess, H.SIMS[sim], shrink)
        ids64, sc64 = m.session(sess, 64, H.SIMS[sim], shrink)            # the sim call's model at k = 64
        c, t = np.array([b for b, _ in r], np.int64), np.array([s for _, s in r], np.float64)
        for k in D.KS:
            ids, sc = D.deep(m, sess, k, sim, shrink)
            assert len(ids) == min(k, len(r))                             # counts = min(k, n)
            assert ids[:64] == ids64 and sc[:64].tobytes() == sc64.tobytes()      # the prefix of 64
            assert len(set(ids)) == len(ids)
        for place, (b, s) in enumerate(zip(ids, sc)):                     # (k = 1024) entry r has the rank r: r candidates come before it
            assert int(np.count_nonzero((t > s) | ((t == s) & (c < b)))) == place, (sess, place)


@pytest.mark.parametrize("sim,shrink", D.MEASURES)
def test_the_lds_session_has_217_candidates_and_the_exact_one_64(sim, shrink):
    assert len(ranking(D.LDS_SESSION, sim, shrink)) == 217 and D.LDS_SESSION in H.lds_sessions()
    assert len(ranking(D.EXACT_64, sim, shrink)) == 64 and D.EXACT_64 in H.lds_sessions()


def test_the_lds_sessions_places_around_64_tie_with_the_cosine():
    r = ranking(D.LDS_SESSION, "cosine", 0.0)
    assert D.ties_across(r, 64) and D.ties_across(r, 65)                  # places 64 / 65 and 65 / 66, counted from 1


@pytest.mark.parametrize("sim,shrink", D.MEASURES)
def test_the_global_sessions_tie_across_every_cut(sim, shrink):
    sizes = {}
    for sess in D.GLOBAL_SESSIONS:
        assert list(sess) in H.global_sessions()
        r = ranking(list(sess), sim, shrink)
        sizes[tuple(sess)] = len(r)
        for cut in D.CUTS:
            if tuple(sess) == (12, 13, 7, 60002) and cut == 1024 and (sim, shrink) == ("jaccard", 0.5):
                continue                                                  # the one cut of the table that falls between two scores
            assert D.ties_across(r, cut), (sess, cut)
    assert sizes == {(13,): 4995, (13, 301, 302): 5029, (12, 13, 7, 60002): 5014}


def test_the_small_matrix_has_1350_candidates_of_few_scores():
    ops = D.small_ops()
    assert np.unique(np.stack([ops[0], ops[1]]), axis=1).shape[1] == ops[0].size      # every (x, y) once
    m = H.SessionModel(H.sorted_export_of(ops))
    for sim, shrink in D.MEASURES:
        r = m.ranking(D.SMALL_SESSION, H.SIMS[sim], shrink)
        assert len(r) == 1350 > D.DEEP_MAX
        assert len(set(s for _, s in r)) <= 9
        assert D.ties_across(r, D.DEEP_MAX)
    assert all(int(np.count_nonzero(ops[0] == x)) == D.SMALL_PAIRS + 1 for x in D.SMALL_ROWS)
