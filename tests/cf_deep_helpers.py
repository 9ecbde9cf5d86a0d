"""What the tests of smatrix_cf_recommend_deep (include/smatrix_batch.h) share: tests/test_cf_deep_model.py (CPU) and
tests/test_gpu_cf_deep.py (a plain module, no tests of its own).

The model is cf_sim_helpers.SessionModel.ranking(...)[:k]: the sim call's model with another cut.  The world is cf_sim_helpers';
small_ops() is a second, small matrix whose one session stays in the LDS tier with more than DEEP_MAX candidates."""
import functools

import numpy as np

from tests import cf_sim_helpers as H

DEEP_MAX = 1024                                             # include/smatrix_batch.h SMATRIX_DEEP_MAX
KS = (65, 100, 217, 218, 1000, 1024)                        # the deep ending's k: around the 217-candidate session, and the ends
CUTS = (64, 65, 100, 128, 217, 256, 1000, 1024)             # places a cut may fall between two equal scores
MEASURES = [("cosine", 0.0), ("jaccard", 0.5), ("lift", 0.5)]
LDS_SESSION = [10, 11, 12, 11]                              # 217 candidates, LDS tier
EXACT_64 = [17, 60003, 14]                                  # exactly 64 candidates
GLOBAL_SESSIONS = ([13], [13, 301, 302], [12, 13, 7, 60002])


@functools.lru_cache(maxsize=None)
def cpu_model():
    """the SessionModel of the world's contents, without a GPU"""
    return H.SessionModel(H.sorted_export_of(H.world_contents()))


def deep(model, sess, k, sim, shrink, w=None, excl=(), deny=()):
    """-> (ids as a list, scores float64): the first k of the session's ranking"""
    best = model.ranking(sess, H.SIMS[sim] if isinstance(sim, str) else sim, shrink, w, excl, deny)[:k]
    return [b for b, _ in best], np.array([s for _, s in best], np.float64)


def ties_across(ranking, cut):
    """do the places cut - 1 and cut of the ranking hold one score?  Then the ids decide who is inside the cut"""
    return len(ranking) > cut and ranking[cut - 1][1] == ranking[cut][1]


# ---- the small matrix: an LDS-tier session with more than DEEP_MAX candidates -----------------------------------------------------
# Three rows of 450 pairs and a head total each (451 keys: 1024 cells), over disjoint columns without rows (their total counts as 1),
# values 1..3: 1350 candidates, 3 * 1024 slots + 3 items <= 4096, and at most 9 distinct scores under a measure.
SMALL_ROWS = (1, 2, 3)
SMALL_HEADS = {1: 4, 2: 9, 3: 16}
SMALL_PAIRS = 450
SMALL_SESSION = [1, 2, 3]


def small_ops():
    """-> (x, y, v) uint32 arrays: SET ops, every (x, y) once"""
    rng = np.random.default_rng(1024)
    cols = (1000 + rng.permutation(100000)[:SMALL_PAIRS * len(SMALL_ROWS)]).astype(np.uint32)
    xs, ys, vs = [], [], []
    for i, x in enumerate(SMALL_ROWS):
        xs.append(np.full(SMALL_PAIRS + 1, x, np.uint32))
        ys.append(np.concatenate([[0], cols[i * SMALL_PAIRS:(i + 1) * SMALL_PAIRS]]).astype(np.uint32))
        vs.append(np.concatenate([[SMALL_HEADS[x]], rng.integers(1, 4, SMALL_PAIRS)]).astype(np.uint32))
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(vs)
