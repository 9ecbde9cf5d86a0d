"""The numpy model of smatrix_merge_topk_by's cosine rank (include/smatrix_batch.h), for tests/test_merge_topk_by_model.py and
tests/test_gpu_merge_topk_by.py (a plain module, no tests of its own).

A candidate list is the triple (x, y, v) that tests/merge_helpers.ops_of() makes of an oracle.  total(i) is the value of row i's
head pair (y == 0), 0 without a row or a head pair -- what get(i, 0) returns.  The score is IEEE double throughout: numpy's
sqrt, * and / of float64 are correctly rounded, as the kernels' are."""
import numpy as np

RANK_VALUE, RANK_COSINE = 0, 1


def totals_of(cand, ids):
    """total(i) for every i of ids (uint32 array) -> uint32 array"""
    x, y, v = cand
    head = y == 0
    hx, hv = x[head], v[head]
    order = np.argsort(hx, kind="stable")
    hx, hv = hx[order], hv[order]
    ids = np.asarray(ids, np.uint32)
    if hx.size == 0:
        return np.zeros(ids.size, np.uint32)
    at = np.minimum(np.searchsorted(hx, ids), hx.size - 1)
    return np.where(hx[at] == ids, hv[at], 0).astype(np.uint32)


def scores_of(cand):
    """the score of every candidate, as k_cf_neighbors computes it -> float64 array (the head pairs' entries mean nothing)"""
    x, y, v = cand
    ta = totals_of(cand, x)
    tb = totals_of(cand, y)
    tb = np.where(tb == 0, 1, tb)
    den = np.sqrt(ta.astype(np.float64)) * np.sqrt(tb.astype(np.float64))
    num = v.astype(np.float64)
    ok = (den != 0.0) & ~(num > den)
    return np.where(ok, num / np.where(den != 0.0, den, 1.0), 0.0)


def topk_cosine(cand, m, min_value):
    """candidates -> (the kept ops (x, y, v), the number dropped): per row the eligible pairs (y != 0, v >= min_value) by
    (score bits descending, y ascending), the first m kept; the head pair kept iff v >= min_value and v != 0, beside the m"""
    x, y, v = cand
    bits = scores_of(cand).view(np.uint64)
    keep = (y == 0) & (v >= np.uint32(min_value)) & (v != 0)
    elig = (y != 0) & (v >= np.uint32(min_value))
    idx = np.flatnonzero(elig)
    order = idx[np.lexsort((y[idx], ~bits[idx], x[idx]))]                # by row, then by -score, then by column
    xs = x[order]
    first = np.flatnonzero(np.concatenate(([True], xs[1:] != xs[:-1]))) if xs.size else np.zeros(0, np.int64)
    rank_in_row = np.arange(xs.size) - np.repeat(first, np.diff(np.concatenate((first, [xs.size]))))
    keep[order[rank_in_row < m]] = True
    return (x[keep], y[keep], v[keep]), int(x.size - np.count_nonzero(keep))
