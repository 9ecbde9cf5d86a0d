"""CPU, no library: the expected answer of tests/cf_explain_helpers.py adds up to the scores of cf_sim_helpers.SessionModel.ranking --
the promise smatrix_cf_explain makes about smatrix_cf_rank, checked between the two models before tests/test_gpu_cf_explain.py holds
the kernels to either --, the fixture can tell a wrong kernel from a right one, and explain_table on arrays written by hand."""
import numpy as np
import pytest

from tests import cf_explain_helpers as E
from tests import cf_rank_helpers as R
from tests import cf_sim_helpers as H


@pytest.fixture(scope="module")
def model():
    return R.world_model()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sim,shrink", E.MEASURES)
def test_a_targets_terms_add_up_to_its_score_in_the_ranking(model, sim, shrink, weighted):
    sessions = H.all_sessions()
    weights = E.weights_for(sessions) if weighted else None
    rankings = [model.ranking(s, H.SIMS[sim], shrink, None if weights is None else weights[i]) for i, s in enumerate(sessions)]
    targets = [R.target_list(s, r) for s, r in zip(sessions, rankings)]
    terms, cc, e_off = E.expected(model, sessions, targets, sim, shrink, weights)
    assert not (terms.view(np.uint64) == np.float64(-0.0).view(np.uint64)).any()
    summed = 0
    for s, (sess, tg, r) in enumerate(zip(sessions, targets, rankings)):
        score = dict(r)
        block = terms[int(e_off[s]):int(e_off[s + 1])].reshape(len(tg), len(sess))
        for j, t in enumerate(tg):
            if t in score:
                assert E.fold(block[j]) == R.bits(score[t]), (sim, shrink, weighted, s, t)
                summed += 1
    assert summed > 100                                                       # (28 sessions, most with several ranked targets)


def test_explain_table_on_arrays_written_by_hand():
    from libsmatrix_amd import explain_table
    sessions, targets = [[5, 6, 5, 7], [], [9]], [[100, 200], [1], []]
    e_off = np.array([0, 8, 8, 8], np.uint64)
    terms = np.array([0.25, 0.5, 0.0, 0.25, 0.0, 0.0, 0.0, 0.0], np.float64)
    cc = np.array([3, 4, 0, 1, 0, 2, 0, 0], np.uint32)
    got = explain_table(sessions, targets, terms, cc, e_off)
    assert got == [[[(6, 4, 0.5), (5, 3, 0.25), (7, 1, 0.25)], [(6, 2, 0.0)]], [[]], []]     # term descending, then position; cc == 0 left out
    assert explain_table(sessions, targets, terms, cc, e_off, top=2) == [[[(6, 4, 0.5), (5, 3, 0.25)], [(6, 2, 0.0)]], [[]], []]
    assert explain_table(sessions, targets, terms, cc, e_off, top=0)[0] == [[], []]
    assert explain_table([], [], np.zeros(0), np.zeros(0, np.uint32), np.zeros(1, np.uint64)) == []


def test_the_fixture_tells_a_fused_denominator_from_the_two_step_one(model):
    sessions = H.all_sessions()
    targets = [R.target_list(s, model.ranking(s, H.SIM_COSINE, 0.0)) for s in sessions]
    _, _, _, ta, tb, c = (np.array(col) for col in zip(*E.live_entries(model, sessions, targets)))
    for sim, shrink in ((H.SIM_COSINE, 0.1), (H.SIM_LIFT, 0.5)):
        assert H.contraction_differs(ta, tb, c, sim, shrink).any(), (sim, shrink)


def test_the_fixture_has_a_repeated_id_whose_later_position_is_zero_and_whose_first_is_not(model):
    sessions = H.all_sessions() + E.long_sessions()
    targets = [R.target_list(s, model.ranking(s, H.SIM_COSINE, 0.0)) for s in H.all_sessions()] + [E.LONG_TARGETS] * 4
    terms, cc, e_off = E.expected(model, sessions, targets, "cosine", 0.0)
    found = 0
    for s, (sess, tg) in enumerate(zip(sessions, targets)):
        block = terms[int(e_off[s]):int(e_off[s + 1])].reshape(len(tg), len(sess))
        first = E.first_positions(sess)
        for i in set(range(len(sess))) - set(first):
            assert not block[:, i].any()
            found += bool(block[:, sess.index(sess[i])].any())
    assert found > 0
    long = E.long_sessions()
    assert [len(s) for s in long] == [64, 65, 129, 8200] and long[3][0] == long[3][8199] == E.Z
    assert long[1][63] == E.X and long[2][63] == long[2][64] == E.X and long[3][127] == long[3][128] == E.Y and long[3][8191] == long[3][8192] == E.V
    for s in long:                                                            # the marker ids are nowhere else
        assert [i for i, a in enumerate(s) if a == E.Z] == [0, len(s) - 1]
        assert all(sum(a == b for a in s) <= 2 for b in (E.X, E.Y, E.V))
