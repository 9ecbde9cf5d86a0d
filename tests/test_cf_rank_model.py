"""CPU, no library: the world of tests/cf_sim_helpers.py delivers what tests/test_gpu_cf_rank.py leans on -- for all three measures,
at shrink 0 and 10: rankings longer than 64 in both tiers, so that ranks beyond the recommend call's k exist, and scores that tie,
so that the order of equal scores (ascending id) decides ranks -- and the helpers of tests/cf_rank_helpers.py answer as the
contract says."""
import numpy as np
import pytest

from tests import cf_rank_helpers as R
from tests import cf_sim_helpers as H

MEASURES = [(sim, h) for sim in ("cosine", "jaccard", "lift") for h in (0.0, 10.0)]


@pytest.fixture(scope="module")
def model():
    return R.world_model()


@pytest.mark.parametrize("sim,shrink", MEASURES)
def test_the_lds_tiers_session_has_217_candidates_and_more_than_50_tied_scores(model, sim, shrink):
    ranking = model.ranking(R.LDS_TIE_SESSION, H.SIMS[sim], shrink)
    print(sim, shrink, len(ranking), R.tied(ranking), R.first_tie(ranking))
    assert len(ranking) == 217 and R.tied(ranking) > 50
    assert R.LDS_TIE_SESSION in H.lds_sessions()


@pytest.mark.parametrize("sim,shrink", MEASURES)
def test_the_global_tiers_sessions_have_about_5000_candidates_and_more_than_4600_ties(model, sim, shrink):
    assert len(H.global_sessions()) == 4
    for sess in H.global_sessions():
        ranking = model.ranking(sess, H.SIMS[sim], shrink)
        print(sim, shrink, sess, len(ranking), R.tied(ranking), R.first_tie(ranking))
        assert 4900 < len(ranking) < 5100 and R.tied(ranking) > 4600


@pytest.mark.parametrize("sim,shrink", MEASURES)
def test_the_target_lists_reach_past_64_and_hold_a_tie_pair_in_both_tiers(model, sim, shrink):
    for sess in [R.LDS_TIE_SESSION] + H.global_sessions():
        ranking = model.ranking(sess, H.SIMS[sim], shrink)
        targets = R.target_list(sess, ranking)
        ranks, scores = R.expected(targets, ranking)
        found = ranks[ranks != R.RANK_NONE].tolist()
        assert {0, 1, 63, 64, 65, len(ranking) // 2, len(ranking) - 1} <= set(found)
        t = R.first_tie(ranking)
        assert t is not None and {t, t + 1} <= set(found) and R.bits(ranking[t][1]) == R.bits(ranking[t + 1][1])
        assert ranking[t][0] < ranking[t + 1][0]                              # equal scores: the lower id first
        assert targets[-1] == targets[0] and ranks[-1] == ranks[0] == 0       # the repeated entry is answered like its first
        none = [i for i, b in enumerate(targets) if b in (0, H.ABSENT) or b in sess]
        assert len(none) >= 3 and (ranks[none] == R.RANK_NONE).all() and not scores[none].any()


def test_expected_answers_on_a_ranking_written_by_hand():
    ranking = [(7, 0.5), (3, 0.25), (9, 0.25), (4, 0.0)]
    ranks, scores = R.expected([9, 7, 1, 9, 0, 4], ranking)
    assert ranks.tolist() == [2, 0, R.RANK_NONE, 2, R.RANK_NONE, 3] and scores.tolist() == [0.25, 0.5, 0.0, 0.25, 0.0, 0.0]
    assert R.first_tie(ranking) == 1 and R.tied(ranking) == 2
    assert R.target_list([0, 5], ranking) == [7, 3, 9, 4, 0, H.ABSENT, 5, 7]
    assert R.target_list([0], []) == [0, H.ABSENT, 0]


def test_the_model_ranks_a_session_as_the_sim_call_would_return_it(model):
    """the ranking is the model of smatrix_cf_recommend_sim without its cut at k: session() is its head"""
    for sess in ([10, 11, 12, 11], [303, 303, 305, 0, H.NO_HEAD_ITEM]):
        ranking = model.ranking(sess, H.SIM_JACCARD, 10.0, excl=[50001], deny=[50002, 305])
        ids, sc = model.session(sess, 64, H.SIM_JACCARD, 10.0, excl=[50001], deny=[50002, 305])
        assert ids == [b for b, _ in ranking[:64]] and sc.tobytes() == np.array([s for _, s in ranking[:64]], np.float64).tobytes()
        assert not {50001, 50002, 305} & {b for b, _ in ranking}
