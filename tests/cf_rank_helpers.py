"""What tests/test_cf_rank_model.py and tests/test_gpu_cf_rank.py share (a plain module, no tests of its own): the expected answers of
smatrix_cf_rank (include/smatrix_batch.h) and the target lists the tests ask about.

The model is cf_sim_helpers.SessionModel.ranking -- a session's whole ranking, (score descending, id ascending) -- over the contents
of cf_sim_helpers' world: a target's expected rank is its index in that ranking and its score the ranking's, or RANK_NONE and 0.0
when it is not in it.  n_candidates is the ranking's length."""
import numpy as np

from tests import cf_sim_helpers as H

RANK_NONE = 0xFFFFFFFF
LDS_TIE_SESSION = [10, 11, 12, 11]                  # the LDS tier's session of 217 candidates, most of them tied


def world_model():
    """the model over the world's contents as they are known without a GPU"""
    return H.SessionModel(H.sorted_export_of(H.world_contents()))


def bits(score):
    return int(np.float64(score).view(np.uint64))


def tied(ranking):
    """the candidates of a ranking whose score bits another candidate has as well"""
    _, counts = np.unique(np.array([s for _, s in ranking], np.float64).view(np.uint64), return_counts=True)
    return int(counts[counts > 1].sum())


def first_tie(ranking):
    """the index of the first candidate whose successor has the same score bits, or None"""
    for i in range(len(ranking) - 1):
        if bits(ranking[i][1]) == bits(ranking[i + 1][1]):
            return i
    return None


def target_list(sess, ranking):
    """the ids a test asks session sess about, given its ranking: the candidates at the indices 0, 1, 63, 64, 65, the middle and the
    last one where they exist, both members of the first adjacent pair of equal score bits where there is one, the ids 0 and ABSENT,
    the session's first non-zero item, and the list's first entry once more"""
    n = len(ranking)
    at = []
    for i in (0, 1, 63, 64, 65, n // 2, n - 1):
        if 0 <= i < n and i not in at:
            at.append(i)
    t = first_tie(ranking)
    if t is not None:
        at += [i for i in (t, t + 1) if i not in at]
    ids = [int(ranking[i][0]) for i in at] + [0, H.ABSENT] + [int(a) for a in sess if int(a) != 0][:1]
    return ids + ids[:1]


def expected(targets, ranking):
    """-> (ranks uint32, scores float64) of the targets of one session"""
    where = {int(b): i for i, (b, _) in enumerate(ranking)}
    ranks = np.array([where.get(int(t), RANK_NONE) for t in targets], np.uint32)
    scores = np.array([ranking[where[int(t)]][1] if int(t) in where else 0.0 for t in targets], np.float64)
    return ranks, scores


def expected_all(model, sessions, targets, sim, shrink, weights=None, exclude=None, deny=()):
    """-> (ranks, scores, n_candidates) as SparseMatrix.cf_rank returns them, and the rankings"""
    rankings = [model.ranking(s, H.SIMS[sim], shrink, None if weights is None else weights[i], () if exclude is None else exclude[i], deny)
                for i, s in enumerate(sessions)]
    parts = [expected(t, r) for t, r in zip(targets, rankings)]
    ranks = np.concatenate([p[0] for p in parts] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    scores = np.concatenate([p[1] for p in parts] + [np.zeros(0, np.float64)]).astype(np.float64)
    return ranks, scores, np.array([len(r) for r in rankings], np.uint32), rankings
