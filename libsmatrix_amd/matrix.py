"""SparseMatrix -- the host-side mirror of the reference's binding interface.

Same method names, argument meaning and error behaviour as the reference's Java
class (src/java/com/paulasmuth/libsmatrix/SparseMatrix.java:70-118) and Ruby class
(src/smatrix_ruby.c:166-174), over the drop-in C ABI (include/smatrix.h), plus the
batched calls (include/smatrix_batch.h) that feed the HIP kernels.  Everything
runs on the GPU through lib/smatrix.so; there is no CPU path here.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import _lib

OP_GET, OP_SET, OP_INCR, OP_DECR = 0, 1, 2, 3
EXPORT_TABLE, EXPORT_SORTED = 0, 1      # include/smatrix_batch.h SMATRIX_EXPORT_*
_EXPORT_ORDERS = {"table": EXPORT_TABLE, "sorted": EXPORT_SORTED}


def _export_order(order):
    if order not in _EXPORT_ORDERS:
        raise ValueError("order must be 'sorted' or 'table', not %r" % (order,))
    return _EXPORT_ORDERS[order]


_MERGE_OPS = {"set": OP_SET, "incr": OP_INCR, "decr": OP_DECR}


def _merge_op(op):
    """"set" / "incr" / "decr" (or the op code) -> op code; anything else, GET included, is a ValueError"""
    if op in _MERGE_OPS:
        return _MERGE_OPS[op]
    if isinstance(op, int) and not isinstance(op, bool) and op in _MERGE_OPS.values():
        return op
    raise ValueError("op must be 'set', 'incr' or 'decr', not %r" % (op,))


def _check_u32(name, val, lo=0):
    if not isinstance(val, (int, np.integer)) or isinstance(val, bool) or not lo <= val <= 0xFFFFFFFF:
        raise ValueError("%s must be an integer in %d .. 2**32 - 1, not %r" % (name, lo, val))


def _scale_args(num, den, min_value):
    """merge_scaled's num / den / min_value: uint32 each, 1 <= num <= den; anything else is a ValueError"""
    for name, val in (("num", num), ("den", den), ("min_value", min_value)):
        _check_u32(name, val)
    if not 1 <= num <= den:
        raise ValueError("1 <= num <= den is required, not %r / %r" % (num, den))


def _topk_args(m, min_value):
    """merge_topk's m / min_value: uint32 each, m >= 1; anything else is a ValueError"""
    _check_u32("m", m, 1)
    _check_u32("min_value", min_value)


_RANKS = {"value": 0, "cosine": 1}                      # SMATRIX_RANK_VALUE, SMATRIX_RANK_COSINE
_SIMS = {"cosine": 0, "jaccard": 1, "lift": 2}          # SMATRIX_SIM_COSINE, SMATRIX_SIM_JACCARD, SMATRIX_SIM_LIFT


def _rank(rank):
    """"value" / "cosine" / "jaccard" / "lift" -> the name; anything else is a ValueError"""
    if isinstance(rank, str) and (rank in _RANKS or rank in _SIMS):
        return rank
    raise ValueError("rank must be 'value', 'cosine', 'jaccard' or 'lift', not %r" % (rank,))


def _sim(sim):
    """"cosine" / "jaccard" / "lift" -> the measure's code; anything else is a ValueError"""
    if isinstance(sim, str) and sim in _SIMS:
        return _SIMS[sim]
    raise ValueError("sim must be 'cosine', 'jaccard' or 'lift', not %r" % (sim,))


def _shrink(shrink):
    """the shrinkage added to a score's denominator: a finite real number >= 0 -> float; anything else is a ValueError"""
    if isinstance(shrink, (bool, str)) or not isinstance(shrink, (int, float, np.integer, np.floating)):
        raise ValueError("shrink must be a finite number >= 0, not %r" % (shrink,))
    h = float(shrink)
    if not (h >= 0.0 and h != float("inf")):
        raise ValueError("shrink must be a finite number >= 0, not %r" % (shrink,))
    return h


def _rank_args(rank, shrink):
    """merge_topk's rank / shrink -> (rank name, shrink as float); shrink != 0 needs a rank that scores"""
    rank, h = _rank(rank), _shrink(shrink)
    if rank == "value" and h != 0.0:
        raise ValueError("shrink belongs to a score: rank='value' takes none")
    return rank, h


def _topk_by_args(rank, m, min_value):
    _topk_args(m, min_value)


def _topk_sim_args(sim, shrink, m, min_value):
    _topk_args(m, min_value)


RANK_NONE = 0xFFFFFFFF                                   # SMATRIX_RANK_NONE: the rank of a target that is no candidate


def rank_metrics(ranks, ks=(1, 10, 100)):
    """ranks as cf_rank returns them -> {"n": targets, "found": those with a rank, "hit_rate": {k: share with rank < k},
    "mrr": mean of 1 / (rank + 1), a target without a rank counting 0}; every share of an empty input is 0.0"""
    r = np.asarray(ranks, dtype=np.uint32).ravel().astype(np.int64)
    found = r != RANK_NONE
    n = int(r.size)
    rr = np.where(found, 1.0 / (r.astype(np.float64) + 1.0), 0.0)
    return {"n": n, "found": int(np.count_nonzero(found)),
            "hit_rate": {int(k): (float(np.count_nonzero(found & (r < int(k)))) / n if n else 0.0) for k in ks},
            "mrr": float(rr.sum() / n) if n else 0.0}


def explain_table(sessions, targets, terms, cc, e_offsets, top=None):
    """what cf_explain returns, as something to show: per session a list with one entry per target, each a list of
    (item, cc, term) tuples -- the session's items that put the target where it is, by term descending, equal terms by ascending
    position; entries with cc == 0 (the item's row does not hold the target, or a later occurrence of the item) are left out; cut
    at `top` entries when given.  Pure numpy, no library call"""
    terms, cc = np.asarray(terms, dtype=np.float64).ravel(), np.asarray(cc, dtype=np.uint32).ravel()
    out = []
    for s, (sess, tg) in enumerate(zip(sessions, targets)):
        items, L, e0 = np.asarray(sess, dtype=np.uint32), len(sess), int(e_offsets[s])
        rows = []
        for j in range(len(tg)):
            t, c = terms[e0 + j * L:e0 + (j + 1) * L], cc[e0 + j * L:e0 + (j + 1) * L]
            at = np.flatnonzero(c != 0)
            at = at[np.argsort(-t[at], kind="stable")][:top]
            rows.append([(int(items[i]), int(c[i]), float(t[i])) for i in at])
        out.append(rows)
    return out


def _sessions(sessions):
    """a list of id sequences -> (offsets uint64[n+1], ids uint32[total])"""
    lens = np.array([len(s) for s in sessions], dtype=np.uint64)
    offsets = np.zeros(len(sessions) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    ids = _u32(np.concatenate([np.asarray(s, dtype=np.uint32) for s in sessions]) if len(sessions) else np.zeros(0, np.uint32))
    return offsets, ids


def _check_k(k):
    if not 1 <= int(k) <= 64:
        raise ValueError("k must be 1..64, not %r" % (k,))


def _weights_shape(weights, sessions):
    if len(weights) != len(sessions) or any(len(w) != len(s) for w, s in zip(weights, sessions)):
        raise ValueError("weights must hold one sequence per session, of the session's length")


def _weights(weights, sessions):
    """per-session weight sequences shaped like sessions -> float64[total]; a shape that differs, a negative or a non-finite
    weight is a ValueError"""
    _weights_shape(weights, sessions)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(w, dtype=np.float64) for w in weights]) if len(weights)
                                else np.zeros(0, np.float64))
    if not (np.isfinite(flat) & (flat >= 0)).all():
        raise ValueError("weights must be finite and >= 0")
    return flat


IMPORT_FORWARD, IMPORT_NO_SELF = 1, 2                    # include/smatrix_batch.h SMATRIX_IMPORT_*


def _amounts(amounts, sessions):
    """cf_import_events' amounts -> uint32[total]: one entry per session, either a sequence of the session's length or one
    integer for all its positions; integers in 0 .. 2**32 - 1.  Anything else is a ValueError"""
    if isinstance(amounts, (str, bytes)) or not hasattr(amounts, "__len__") or len(amounts) != len(sessions):
        raise ValueError("amounts must hold one entry per session: a sequence of the session's length, or one integer")
    flat = []
    for w, s in zip(amounts, sessions):
        a = np.asarray(w)
        if a.ndim == 0:
            a = np.repeat(a, len(s))
        if a.ndim != 1 or a.size != len(s):
            raise ValueError("amounts must hold one entry per session: a sequence of the session's length, or one integer")
        if a.size:
            if a.dtype.kind not in "iu":
                raise ValueError("amounts must be integers in 0 .. 2**32 - 1, not %r" % (a.dtype,))
            wide = a.astype(np.int64 if a.dtype.kind == "i" else np.uint64)
            if (wide < 0).any() or (wide > 0xFFFFFFFF).any():
                raise ValueError("amounts must be integers in 0 .. 2**32 - 1")
        flat.append(a.astype(np.uint32))
    return _u32(np.concatenate(flat) if flat else np.zeros(0, np.uint32))


def _import_flags(forward, no_self):
    return (IMPORT_FORWARD if forward else 0) | (IMPORT_NO_SELF if no_self else 0)


POPULAR_MAX = 4096                                       # include/smatrix_batch.h SMATRIX_POPULAR_MAX


def _popular_args(n, min_total):
    """cf_popular's n / min_total: n an integer in 1 .. POPULAR_MAX, min_total a uint32; anything else is a ValueError"""
    if not isinstance(n, (int, np.integer)) or isinstance(n, bool) or not 1 <= n <= POPULAR_MAX:
        raise ValueError("n must be an integer in 1 .. %d, not %r" % (POPULAR_MAX, n))
    _check_u32("min_total", min_total)


TREND_GAIN, TREND_RATIO, TREND_ZSCORE = 0, 1, 2          # include/smatrix_batch.h SMATRIX_TREND_*
_TRENDS = {"gain": TREND_GAIN, "ratio": TREND_RATIO, "zscore": TREND_ZSCORE}


def _trend(measure):
    """"gain" / "ratio" / "zscore" -> the measure's code; anything else is a ValueError"""
    if isinstance(measure, str) and measure in _TRENDS:
        return _TRENDS[measure]
    raise ValueError("measure must be 'gain', 'ratio' or 'zscore', not %r" % (measure,))


def _trending_args(base, n, measure, num, den, shrink, min_total, min_gain):
    """cf_trending's arguments behind the matrix itself: base another SparseMatrix, n and min_total as cf_popular's, min_gain a
    uint32, 1 <= num <= den as merge_scaled's -> (the measure's code, shrink as float); anything else is a ValueError"""
    if not isinstance(base, SparseMatrix):
        raise ValueError("base must be a SparseMatrix, not %r" % (base,))
    _popular_args(n, min_total)
    _check_u32("min_gain", min_gain)
    _scale_args(num, den, 0)
    return _trend(measure), _shrink(shrink)


def _fill_ids(fill):
    """cf_recommend_filled's list -> uint32[n_fill]: a flat sequence of integers in 0 .. 2**32 - 1, which may be empty.  Anything
    else is a ValueError"""
    if fill is None or isinstance(fill, (str, bytes)) or not hasattr(fill, "__len__"):
        raise ValueError("fill must be a sequence of ids, not %r" % (fill,))
    a = np.asarray(fill)
    if a.ndim != 1 or a.size > 0xFFFFFFFF:
        raise ValueError("fill must be a flat sequence of fewer than 2**32 ids")
    if a.size == 0:
        return np.zeros(0, np.uint32)
    if a.dtype.kind not in "iu":
        raise ValueError("fill must hold integers in 0 .. 2**32 - 1, not %r" % (a.dtype,))
    wide = a.astype(np.int64 if a.dtype.kind == "i" else np.uint64)
    if (wide < 0).any() or (wide > 0xFFFFFFFF).any():
        raise ValueError("fill must hold integers in 0 .. 2**32 - 1")
    return _u32(a)


GROUP_NONE = 0xFFFFFFFF                                  # SMATRIX_GROUP_NONE: the entry of an id that belongs to no group


def _group_map(group_of):
    """cf_recommend_grouped's map -> uint32[group_n], or None for no map: None, a flat sequence of integers in 0 .. 2**32 - 1 (entry
    i the group of id i, GROUP_NONE for none), or a dict {id: group} (the ids not named get GROUP_NONE).  Anything else is a
    ValueError"""
    if group_of is None:
        return None
    if isinstance(group_of, dict):
        if not group_of:
            return None
        ids, groups = _group_ints(list(group_of.keys())), _group_ints(list(group_of.values()))
        out = np.full(int(ids.max()) + 1, GROUP_NONE, dtype=np.uint32)
        out[ids] = groups
        return out
    if isinstance(group_of, (str, bytes)) or not hasattr(group_of, "__len__"):
        raise ValueError("group_of must be None, a sequence of group ids or a dict {id: group}, not %r" % (group_of,))
    if len(group_of) == 0:
        return None
    return _u32(_group_ints(group_of))


def _group_ints(values):
    a = np.asarray(values)
    if a.ndim != 1 or a.size > 1 << 32 or a.dtype.kind not in "iu":
        raise ValueError("group_of must hold integers in 0 .. 2**32 - 1, one per id")
    wide = a.astype(np.int64 if a.dtype.kind == "i" else np.uint64)
    if (wide < 0).any() or (wide > 0xFFFFFFFF).any():
        raise ValueError("group_of must hold integers in 0 .. 2**32 - 1")
    return wide.astype(np.uint32)


def _check_cap(cap):
    if not isinstance(cap, (int, np.integer)) or isinstance(cap, bool) or not 1 <= cap <= 64:
        raise ValueError("cap must be an integer in 1 .. 64, not %r" % (cap,))


SCOPE_MAX = 64                                           # include/smatrix_batch.h SMATRIX_SCOPE_MAX
SCOPE_ONLY, SCOPE_EXCEPT = 0, 1                          # SMATRIX_SCOPE_ONLY, SMATRIX_SCOPE_EXCEPT
_SCOPE_MODES = {"only": SCOPE_ONLY, "except": SCOPE_EXCEPT}


def _scope_mode(mode):
    try:
        return _SCOPE_MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("mode must be 'only' or 'except', not %r" % (mode,)) from None


def _scope_lists(scope, sessions):
    """cf_recommend_scoped's scope -> (sc_offsets uint64[n+1], sc_groups uint32[total]), or (None, None) when no session is scoped:
    one entry per session, None or a flat sequence of at most SCOPE_MAX integers in 0 .. 2**32 - 1.  Anything else is a ValueError"""
    if scope is None or isinstance(scope, (str, bytes)) or not hasattr(scope, "__len__") or len(scope) != len(sessions):
        raise ValueError("scope must hold one list of group ids (or None) per session")
    lists = []
    for one in scope:
        if one is None:
            one = ()
        if isinstance(one, (str, bytes)) or not hasattr(one, "__len__"):
            raise ValueError("a session's scope must be a sequence of group ids, not %r" % (one,))
        if len(one) > SCOPE_MAX:
            raise ValueError("a session's scope holds at most %d groups, not %d" % (SCOPE_MAX, len(one)))
        a = np.asarray(one)
        if a.size:
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise ValueError("a session's scope must hold integers in 0 .. 2**32 - 1")
            wide = a.astype(np.int64 if a.dtype.kind == "i" else np.uint64)
            if (wide < 0).any() or (wide > 0xFFFFFFFF).any():
                raise ValueError("a session's scope must hold integers in 0 .. 2**32 - 1")
        lists.append(a.astype(np.uint32).reshape(-1))
    if not any(a.size for a in lists):
        return None, None
    return _sessions(lists)


DEEP_MAX = 1024                                          # include/smatrix_batch.h SMATRIX_DEEP_MAX


def _check_deep_k(k):
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= DEEP_MAX:
        raise ValueError("k must be an integer in 1 .. %d, not %r" % (DEEP_MAX, k))


def _deny_bitmap(deny):
    """a sequence of ids -> (bitmap uint32[(deny_n + 31) / 32], deny_n = the largest id + 1); (None, 0) for no id"""
    ids = np.unique(_u32(deny))
    if ids.size == 0:
        return None, 0
    deny_n = int(ids[-1]) + 1
    bits = np.zeros((deny_n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(bits, ids >> 5, np.uint32(1) << (ids & np.uint32(31)))
    return bits, deny_n


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p(a, to=_lib.u32p):
    return None if a is None else a.ctypes.data_as(to)


_DP = C.POINTER(C.c_double)


def _topk_outputs(n, k):
    """the outputs of a top-k-shaped session call: -> (ids[n,k], scores[n,k] float64, counts[n]), zeros"""
    return np.zeros((n, k), dtype=np.uint32), np.zeros((n, k), dtype=np.float64), np.zeros(n, dtype=np.uint32)


def _map_args(m):
    """a checked group or scope map (_group_map's) as the C calls take it: (map, map_n), (NULL, 0) for none"""
    return _p(m), 0 if m is None else int(m.size)


def _fill_args(fill):
    """a checked fill list (_fill_ids') as the C calls take it: (fill_ids, n_fill), (NULL, 0) for an empty one"""
    return _p(fill) if fill.size else None, int(fill.size)


_DEV_BAD = "bad k, n, weights, exclusion lists, deny bitmap, "      # how the _dev recommend calls' refusals begin


def _stream_ptr(stream):
    """a _dev method's stream as the C call takes it: a torch.cuda.Stream's handle, or a hipStream_t as int or None as they are"""
    return getattr(stream, "cuda_stream", stream)


class SparseMatrix:
    def __init__(self, filename=None):
        """filename None = in-memory (SparseMatrix.java:70-77); else open-or-create the file."""
        self._lib = _lib.load()
        self.filename = filename
        env = os.environ.get("SMATRIX_DEVICE")
        self._device = int(env) if env else None      # the matrix's GPU: SMATRIX_DEVICE, else the current device at open
        if self._device is None and "torch" in sys.modules and sys.modules["torch"].cuda.is_initialized():
            self._device = sys.modules["torch"].cuda.current_device()
        self._h = self._lib.smatrix_open(filename.encode() if filename else None)
        if not self._h:
            # smatrix_jni.c:61-62 turns a NULL handle into IllegalArgumentException
            raise ValueError("smatrix_open() failed (no HIP device, or cannot open %r)" % (filename,))

    # ---- the reference binding's methods ---------------------------------
    def get(self, x, y):
        return self._lib.smatrix_get(self._h, x, y)

    def set(self, x, y, v):
        return self._lib.smatrix_set(self._h, x, y, v)

    def incr(self, x, y, v):
        return self._lib.smatrix_incr(self._h, x, y, v)

    def decr(self, x, y, v):
        return self._lib.smatrix_decr(self._h, x, y, v)

    def getRowLength(self, x):
        return self._lib.smatrix_rowlen(self._h, x)

    def getRow(self, x, maxlen=0):
        """SortedMap<Integer,Integer> in Java (SparseMatrix.java:102-112): a dict sorted by key.
        Buffer sizing and the maxlen cut follow smatrix_jni.c:130-144."""
        pairs = self.getrow_raw(x, self.getRowLength(x) * 8)
        if maxlen > 0:
            pairs = pairs[:maxlen]
        return dict(sorted((int(k), int(v)) for k, v in pairs))

    def getFilename(self):
        return self.filename

    def close(self):
        if self._h:
            self._lib.smatrix_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- C-ABI level helpers ---------------------------------------------
    def getrow_raw(self, x, ret_len_bytes):
        """smatrix_getrow with a caller buffer of ret_len_bytes: (n,2) pairs in slot order."""
        buf = np.zeros(ret_len_bytes // 4 + 4, dtype=np.uint32)   # slack: S4 may overrun by one pair
        n = self._lib.smatrix_getrow(self._h, x, _p(buf), ret_len_bytes)
        return buf[: 2 * n].reshape(n, 2).copy()

    @property
    def mem(self):
        return int(self._h.contents.mem)

    # ---- batched API --------------------------------------------------------
    def apply_batch(self, op, x, y, v=None, results=True, out=None):
        """results=False: no result array is passed (include/smatrix_batch.h: the table ends in the same state, the
        kernels skip the results) and None is returned; out: the caller's own result array (uint32, same length)"""
        x, y = _u32(x), _u32(y)
        if x.shape != y.shape:
            raise ValueError("x and y must have the same shape")
        if out is not None:
            # (explicit checks, not asserts: python -O strips those, and a raw pointer goes to C -- ADVICE r5)
            if not results:
                raise ValueError("out given with results=False")
            if not isinstance(out, np.ndarray) or out.dtype != np.uint32 or out.shape != x.shape or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous uint32 array of the batch's shape")
        else:
            out = np.empty_like(x) if results else None
        vv = _u32(v) if v is not None else None
        self._lib.smatrix_apply_batch(self._h, op, x.size, _p(x), _p(y),
                                      _p(vv) if vv is not None else None, _p(out) if results else None)
        return out

    def get_batch(self, x, y, out=None):
        return self.apply_batch(OP_GET, x, y, out=out)

    def set_batch(self, x, y, v):
        return self.apply_batch(OP_SET, x, y, v)

    def incr_batch(self, x, y, v, out=None):
        return self.apply_batch(OP_INCR, x, y, v, out=out)

    def decr_batch(self, x, y, v):
        return self.apply_batch(OP_DECR, x, y, v)

    def rowlen_batch(self, xs):
        xs = _u32(xs)
        out = np.empty_like(xs)
        self._lib.smatrix_rowlen_batch(self._h, xs.size, _p(xs), _p(out))
        return out

    def getrow_batch(self, xs, caps=None):
        """returns (offsets[n+1], pairs[total,2], counts[n]); row r's pairs are
        pairs[offsets[r]:offsets[r]+counts[r]].  caps default: rowlen+1 (quirk Q5)."""
        xs = _u32(xs)
        if caps is None:
            caps = self.rowlen_batch(xs).astype(np.uint64) + 1
        offsets = np.zeros(xs.size + 1, dtype=np.uint64)
        np.cumsum(np.asarray(caps, dtype=np.uint64), out=offsets[1:])
        pairs = np.zeros((int(offsets[-1]), 2), dtype=np.uint32)
        counts = np.zeros(xs.size, dtype=np.uint32)
        self._lib.smatrix_getrow_batch(self._h, xs.size, _p(xs), offsets.ctypes.data_as(_lib.u64p),
                                       pairs.ctypes.data_as(_lib.u32p), _p(counts))
        return offsets, pairs, counts

    def cf_neighbors_batch(self, items, caps=None):
        """CF-recommender read path (examples/cf_recommender.c:50-86), fused on the GPU:
        -> (offsets[n+1], ids[total], scores[total] float64, counts[n])"""
        items = _u32(items)
        if caps is None:
            caps = self.rowlen_batch(items).astype(np.uint64) + 1
        offsets = np.zeros(items.size + 1, dtype=np.uint64)
        np.cumsum(np.asarray(caps, dtype=np.uint64), out=offsets[1:])
        ids = np.zeros(int(offsets[-1]), dtype=np.uint32)
        scores = np.zeros(int(offsets[-1]), dtype=np.float64)
        counts = np.zeros(items.size, dtype=np.uint32)
        self._lib.smatrix_cf_neighbors_batch(self._h, items.size, _p(items), offsets.ctypes.data_as(_lib.u64p),
                                             _p(ids), scores.ctypes.data_as(C.POINTER(C.c_double)), _p(counts))
        return offsets, ids, scores, counts

    def cf_topk_batch(self, items, k):
        """the k best neighbours per item (k <= 64): -> (ids[n,k], scores[n,k] float64, counts[n])"""
        items = _u32(items)
        ids = np.zeros((items.size, k), dtype=np.uint32)
        scores = np.zeros((items.size, k), dtype=np.float64)
        counts = np.zeros(items.size, dtype=np.uint32)
        if self._lib.smatrix_cf_topk_batch(self._h, items.size, _p(items), k, ids.ctypes.data_as(_lib.u32p),
                                           scores.ctypes.data_as(C.POINTER(C.c_double)), _p(counts)) != 0:
            raise ValueError("k must be 1..64")
        return ids, scores, counts

    def cf_topk_batch_dev(self, n, items_ptr, k, ids_ptr, scores_ptr, cnt_ptr, stream=None):
        self._lib.smatrix_cf_topk_batch_dev(self._h, n, items_ptr, k, ids_ptr, scores_ptr, cnt_ptr, stream)

    def cf_recommend_batch(self, sessions, k):
        """session recommendations (include/smatrix_batch.h smatrix_cf_recommend_batch): every session is a sequence of
        item ids; its k <= 64 best candidates over its items' rows, by the sum of their cosines, its own items and id 0 left
        out: -> (ids[n,k], scores[n,k] float64, counts[n]); best first, equal scores by ascending id"""
        _check_k(k)
        offsets, items = _sessions(sessions)
        n = len(sessions)
        ids, scores, counts = _topk_outputs(n, k)
        if n and self._lib.smatrix_cf_recommend_batch(self._h, n, offsets.ctypes.data_as(_lib.u64p), _p(items), k,
                                                      ids.ctypes.data_as(_lib.u32p),
                                                      scores.ctypes.data_as(C.POINTER(C.c_double)), _p(counts)) != 0:
            raise ValueError("smatrix_cf_recommend_batch: k must be 1..64 and n_sessions < 2^32")
        return ids, scores, counts

    def cf_recommend_batch_dev(self, n, off_ptr, items_ptr, k, ids_ptr, scores_ptr, cnt_ptr, stream=None):
        """the same on device arrays (raw pointers): offsets uint64[n+1], items uint32, ids uint32[n*k], scores float64[n*k],
        counts uint32[n].  stream: a torch.cuda.Stream or a hipStream_t as int (None: the legacy default stream, synchronised)"""
        _check_k(k)
        self._cf_recommend_dev("smatrix_cf_recommend_batch_dev", "k must be 1..64 and n < 2^32",
                               (n, off_ptr, items_ptr, k, ids_ptr, scores_ptr, cnt_ptr), stream)

    def _cf_front(self, sessions, weights, exclude, deny, sim, shrink, targets=None):
        """what cf_recommend_filtered, cf_rank and cf_explain do before their call: the arguments checked (every check before any
        library call) and flattened.  -> (n, (sim's code, shrink), sess, filt, tgt, offsets, t_off): sess, filt and tgt are the C
        arguments self .. weights, ex_offsets .. deny_n and t_offsets, targets (NULL for what was not given), offsets and t_off
        the sessions' and the targets' offset arrays (t_off None without targets)"""
        measure = _sim(sim), _shrink(shrink)
        n = len(sessions)
        w = None if weights is None else _weights(weights, sessions)
        if targets is not None and len(targets) != n:
            raise ValueError("targets must hold one id sequence per session")
        if exclude is not None and len(exclude) != n:
            raise ValueError("exclude must hold one id sequence per session")
        offsets, items = _sessions(sessions)
        t_off, tg = _sessions(targets) if targets is not None else (None, None)
        ex_off, ex = _sessions(exclude) if exclude is not None else (None, None)
        bits, deny_n = _deny_bitmap(deny) if deny is not None else (None, 0)
        return (n, measure, (self._h, n, _p(offsets, _lib.u64p), _p(items), _p(w, _DP)), (_p(ex_off, _lib.u64p), _p(ex), _p(bits), deny_n),
                (_p(t_off, _lib.u64p), _p(tg)), offsets, t_off)

    def cf_recommend_filtered(self, sessions, k, weights=None, exclude=None, deny=None, sim="cosine", shrink=0.0):
        """cf_recommend_batch with "not these" and recency (include/smatrix_batch.h smatrix_cf_recommend_filtered), applied on
        the GPU before the k best are taken.  weights: per-session sequences shaped like sessions, finite and >= 0 (the term of
        an item is multiplied by the weight at its first position); exclude: one id sequence per session, never given to it;
        deny: ids given to no session.  -> (ids[n,k], scores[n,k] float64, counts[n]) as cf_recommend_batch.
        sim, shrink (smatrix_cf_recommend_sim): the score of a pair (b, cc) of item a is cc / (base + shrink) with base =
        sqrt(A) * sqrt(B) ("cosine"), A + B - cc ("jaccard") or A * B ("lift") over the totals A = self[a, 0], B = self[b, 0];
        shrink is a finite number >= 0.  The defaults make the call above"""
        _check_k(k)
        front = (sessions, weights, exclude, deny, sim, shrink)
        if (_sim(sim), _shrink(shrink)) != (0, 0.0):
            return self._cf_recommend("smatrix_cf_recommend_sim", front, k)
        n, _, sess, filt, _, _, _ = self._cf_front(*front)
        ids, scores, counts = _topk_outputs(n, k)
        if n and self._lib.smatrix_cf_recommend_filtered(*sess, *filt, k, _p(ids), _p(scores, _DP), _p(counts)) != 0:
            raise ValueError("smatrix_cf_recommend_filtered: bad k, n_sessions, weights, exclusion lists or deny bitmap")
        return ids, scores, counts

    def _cf_recommend(self, sym, front, k, extra=(), words="sim or shrink", n_scored=False):
        """the host flavour of every recommend call that takes a measure, behind its own checks: `front` is _cf_front's arguments,
        `extra` the checked C arguments between deny_n and the measure (scope, group, fill, in that order), `words` what the
        refusal names behind the deny bitmap.  -> (ids[n,k], scores[n,k] float64, counts[n]), and n_scored[n] where the call has it;
        without sessions no library call"""
        n, measure, sess, filt, _, _, _ = self._cf_front(*front)
        out = _topk_outputs(n, k) + ((np.zeros(n, dtype=np.uint32),) if n_scored else ())
        if n and getattr(self._lib, sym)(*sess, *filt, *extra, *measure, k, _p(out[0]), _p(out[1], _DP), *map(_p, out[2:])) != 0:
            raise ValueError("%s: bad k, n_sessions, weights, exclusion lists, deny bitmap, %s" % (sym, words))
        return out

    def _cf_recommend_dev(self, sym, words, args, stream):
        """the _dev flavour of a recommend call behind its own checks: `args` the C arguments between the handle and the stream,
        `words` what the refusal says went wrong"""
        if getattr(self._lib, sym)(self._h, *args, _stream_ptr(stream)) != 0:
            raise ValueError("%s: %s" % (sym, words))

    def cf_recommend_filtered_dev(self, n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, k, ids_ptr,
                                  scores_ptr, cnt_ptr, stream=None):
        """the same on device arrays (raw pointers, None for what is not given): cf_recommend_batch_dev's, and weights
        float64 per item, ex_off uint64[n+1], ex_items uint32, deny uint32[(deny_n + 31) / 32].  A bad weight is found on the
        device: ValueError, the outputs' contents unspecified"""
        _check_k(k)
        self._cf_recommend_dev("smatrix_cf_recommend_filtered_dev", "bad k, n, weights, exclusion lists or deny bitmap",
                               (n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, k, ids_ptr, scores_ptr, cnt_ptr),
                               stream)

    def cf_recommend_sim_dev(self, n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, sim, shrink, k,
                             ids_ptr, scores_ptr, cnt_ptr, stream=None):
        """cf_recommend_filtered_dev with cf_recommend_filtered's sim and shrink (smatrix_cf_recommend_sim_dev)"""
        _check_k(k)
        self._cf_recommend_dev("smatrix_cf_recommend_sim_dev", _DEV_BAD + "sim or shrink",
                               (n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, _sim(sim), _shrink(shrink), k,
                                ids_ptr, scores_ptr, cnt_ptr), stream)

    def cf_popular(self, n, deny=None, min_total=1):
        """the most popular items (include/smatrix_batch.h smatrix_cf_popular): the up to n <= POPULAR_MAX ids x != 0 with the
        largest totals self[x, 0] >= max(min_total, 1), the ids of `deny` left out, selected on the GPU over the whole matrix.
        -> (ids uint32[n_found], totals uint32[n_found]), total descending, equal totals by ascending id"""
        _popular_args(n, min_total)
        bits, deny_n = _deny_bitmap(deny) if deny is not None else (None, 0)
        ids = np.zeros(int(n), dtype=np.uint32)
        totals = np.zeros(int(n), dtype=np.uint32)
        found = C.c_uint32(0)
        if self._lib.smatrix_cf_popular(self._h, _p(bits), deny_n, int(min_total), int(n), _p(ids), _p(totals), C.byref(found)) != 0:
            raise ValueError("smatrix_cf_popular: bad n or deny bitmap")
        return ids[:found.value].copy(), totals[:found.value].copy()

    def cf_popular_dev(self, n, deny_ptr, deny_n, min_total, ids_ptr, totals_ptr, n_found_ptr, stream=None):
        """the same on device arrays (raw pointers; deny_ptr None with deny_n 0 for no bitmap): deny uint32[(deny_n + 31) / 32],
        ids uint32[n], totals uint32[n], n_found uint32[1].  No read-back: nothing is returned, the entries beyond n_found are
        left as they were"""
        _popular_args(n, min_total)
        if self._lib.smatrix_cf_popular_dev(self._h, deny_ptr, deny_n, int(min_total), int(n), ids_ptr, totals_ptr, n_found_ptr,
                                            _stream_ptr(stream)) != 0:
            raise ValueError("smatrix_cf_popular_dev: bad n, deny bitmap or outputs")

    def cf_trending(self, base, n, measure="zscore", num=1, den=1, shrink=0.0, deny=None, min_total=1, min_gain=1):
        """the trending items (include/smatrix_batch.h smatrix_cf_trending): the up to n <= POPULAR_MAX ids x != 0 of this matrix
        whose totals T = self[x, 0] >= max(min_total, 1) grew most against E = floor(base[x, 0] * num / den) -- `base` another
        SparseMatrix, the older window --, by G = T - E >= max(min_gain, 1) ("gain"), G / D ("ratio") or G / sqrt(D) ("zscore") with
        D = E + shrink (0 counted as 1); the ids of `deny` left out.  Joined and selected on the GPU over both matrices.
        -> (ids uint32[n_found], scores float64[n_found], totals uint32[n_found], expected uint32[n_found]), score descending,
        equal scores by ascending id"""
        code, h = _trending_args(base, n, measure, num, den, shrink, min_total, min_gain)
        if base is self:
            raise ValueError("base must be another matrix than this one")
        bits, deny_n = _deny_bitmap(deny) if deny is not None else (None, 0)
        ids, scores = np.zeros(int(n), dtype=np.uint32), np.zeros(int(n), dtype=np.float64)
        totals, expected = np.zeros(int(n), dtype=np.uint32), np.zeros(int(n), dtype=np.uint32)
        found = C.c_uint32(0)
        if self._lib.smatrix_cf_trending(self._h, base._h, code, int(num), int(den), h, _p(bits), deny_n, int(min_total), int(min_gain), int(n),
                                         _p(ids), _p(scores, _DP), _p(totals), _p(expected), C.byref(found)) != 0:
            raise ValueError("smatrix_cf_trending: bad base, n, num / den, shrink or deny bitmap")
        f = found.value
        return ids[:f].copy(), scores[:f].copy(), totals[:f].copy(), expected[:f].copy()

    def cf_trending_dev(self, base, n, measure, num, den, shrink, deny_ptr, deny_n, min_total, min_gain, ids_ptr, scores_ptr, totals_ptr,
                        expected_ptr, n_found_ptr, stream=None):
        """the same on device arrays (raw pointers; deny_ptr None with deny_n 0 for no bitmap): deny uint32[(deny_n + 31) / 32],
        ids uint32[n], scores float64[n], totals uint32[n], expected uint32[n], n_found uint32[1].  No read-back: nothing is returned,
        the entries beyond n_found are left as they were.  With a stream the work is enqueued on return: neither matrix may be
        written or closed until the stream has passed it"""
        code, h = _trending_args(base, n, measure, num, den, shrink, min_total, min_gain)
        if base is self:
            raise ValueError("base must be another matrix than this one")
        if self._lib.smatrix_cf_trending_dev(self._h, base._h, code, int(num), int(den), h, deny_ptr, deny_n, int(min_total), int(min_gain), int(n),
                                             ids_ptr, scores_ptr, totals_ptr, expected_ptr, n_found_ptr, _stream_ptr(stream)) != 0:
            raise ValueError("smatrix_cf_trending_dev: bad base, n, num / den, shrink, deny bitmap or outputs")

    def cf_recommend_filled(self, sessions, k, fill, weights=None, exclude=None, deny=None, sim="cosine", shrink=0.0):
        """cf_recommend_filtered, then the free places of a short result filled from `fill` (include/smatrix_batch.h
        smatrix_cf_recommend_fill): a sequence of ids -- cf_popular's, trending, editorial --, walked in order; an id is appended
        with score 0.0 unless it is 0, an item of the session, excluded, denied or in the result already.
        -> (ids[n,k], scores[n,k] float64, counts[n], n_scored[n]): the first n_scored[s] entries of session s are
        cf_recommend_filtered's, the entries up to counts[s] are filled"""
        _check_k(k)
        return self._cf_recommend("smatrix_cf_recommend_fill", (sessions, weights, exclude, deny, sim, shrink), k,
                                  _fill_args(_fill_ids(fill)), "fill, sim or shrink", n_scored=True)

    def cf_recommend_fill_dev(self, n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, fill_ptr, n_fill, sim,
                              shrink, k, ids_ptr, scores_ptr, cnt_ptr, n_scored_ptr, stream=None):
        """the same on device arrays (raw pointers, None for what is not given): cf_recommend_sim_dev's, and fill uint32[n_fill]
        (None with n_fill 0: no list), n_scored uint32[n]"""
        _check_k(k)
        self._cf_recommend_dev("smatrix_cf_recommend_fill_dev", _DEV_BAD + "fill, sim or shrink",
                               (n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, fill_ptr, n_fill, _sim(sim),
                                _shrink(shrink), k, ids_ptr, scores_ptr, cnt_ptr, n_scored_ptr), stream)

    def cf_recommend_grouped(self, sessions, k, group_of, cap, weights=None, exclude=None, deny=None, sim="cosine", shrink=0.0):
        """cf_recommend_filtered with at most `cap` results of a session from one group -- brand, category, seller -- (include/
        smatrix_batch.h smatrix_cf_recommend_grouped), applied on the GPU over the session's whole ranking before the cut at k.
        group_of: a uint32 sequence, entry i the group of id i (GROUP_NONE: none; ids beyond its end: none), or a dict {id: group},
        or None for no grouping; cap: 1 .. 64.  A candidate is taken iff it is ungrouped or fewer than cap candidates of its group
        come before it in the ranking.  -> (ids[n,k], scores[n,k] float64, counts[n]); counts[s] may be < k although the session
        has k candidates and more"""
        _check_k(k)
        _check_cap(cap)
        return self._cf_recommend("smatrix_cf_recommend_grouped", (sessions, weights, exclude, deny, sim, shrink), k,
                                  (*_map_args(_group_map(group_of)), int(cap)), "group map, cap, sim or shrink")

    def cf_recommend_grouped_dev(self, n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, group_ptr, group_n, cap,
                                 sim, shrink, k, ids_ptr, scores_ptr, cnt_ptr, stream=None):
        """the same on device arrays (raw pointers, None for what is not given): cf_recommend_sim_dev's, and group uint32[group_n]
        (None with group_n 0: no grouping)"""
        _check_k(k)
        _check_cap(cap)
        self._cf_recommend_dev("smatrix_cf_recommend_grouped_dev", _DEV_BAD + "group map, cap, sim or shrink",
                               (n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, group_ptr, group_n, int(cap),
                                _sim(sim), _shrink(shrink), k, ids_ptr, scores_ptr, cnt_ptr), stream)

    def cf_recommend_grouped_filled(self, sessions, k, group_of, cap, fill, weights=None, exclude=None, deny=None, sim="cosine", shrink=0.0):
        """cf_recommend_grouped, then the free places of a short result filled from `fill` under the same quotas (include/
        smatrix_batch.h smatrix_cf_recommend_grouped_fill): k results, and still at most `cap` of one group.  group_of and cap are
        cf_recommend_grouped's, fill is cf_recommend_filled's; an id of the list is appended with score 0.0 iff cf_recommend_filled
        would append it and it is ungrouped or fewer than cap entries of the result so far, scored and filled, share its group.
        -> (ids[n,k], scores[n,k] float64, counts[n], n_scored[n]) as cf_recommend_filled: the first n_scored[s] entries of session
        s are cf_recommend_grouped's"""
        _check_k(k)
        _check_cap(cap)
        return self._cf_recommend("smatrix_cf_recommend_grouped_fill", (sessions, weights, exclude, deny, sim, shrink), k,
                                  (*_map_args(_group_map(group_of)), int(cap), *_fill_args(_fill_ids(fill))),
                                  "group map, cap, fill, sim or shrink", n_scored=True)

    def cf_recommend_grouped_fill_dev(self, n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, group_ptr, group_n,
                                      cap, fill_ptr, n_fill, sim, shrink, k, ids_ptr, scores_ptr, cnt_ptr, n_scored_ptr, stream=None):
        """the same on device arrays (raw pointers, None for what is not given): cf_recommend_grouped_dev's, and fill uint32[n_fill]
        (None with n_fill 0: no list), n_scored uint32[n]"""
        _check_k(k)
        _check_cap(cap)
        self._cf_recommend_dev("smatrix_cf_recommend_grouped_fill_dev", _DEV_BAD + "group map, cap, fill, sim or shrink",
                               (n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, group_ptr, group_n, int(cap),
                                fill_ptr, n_fill, _sim(sim), _shrink(shrink), k, ids_ptr, scores_ptr, cnt_ptr, n_scored_ptr), stream)

    def cf_recommend_scoped(self, sessions, k, scope_of, scope, mode="only", group_of=None, cap=None, fill=None, weights=None, exclude=None,
                            deny=None, sim="cosine", shrink=0.0):
        """cf_recommend_grouped_filled from these categories only (include/smatrix_batch.h smatrix_cf_recommend_scoped): a scope per
        session, applied on the GPU where a candidate is made, before the cut at k.  scope_of: a second map as group_of (a uint32
        sequence or a dict {id: group}; ids beyond its end and GROUP_NONE entries are ungrouped); scope: one list of at most SCOPE_MAX
        group ids per session, None or [] for an unscoped session.  mode "only": a scoped session is given the ids whose group is in
        its list and no ungrouped id; "except": every id but those.  An id out of scope is treated as an id of the session's
        exclusion list.  group_of / cap (None: no quotas) and fill (None: no list) are cf_recommend_grouped_filled's.
        -> (ids[n,k], scores[n,k] float64, counts[n], n_scored[n])"""
        _check_k(k)
        code = _scope_mode(mode)
        if cap is None:
            if group_of is not None:
                raise ValueError("group_of needs a cap")
            cap = 64
        _check_cap(cap)
        groups = _group_map(group_of)
        scopes = _group_map(scope_of)
        fill = _fill_ids(() if fill is None else fill)
        sc_off, sc_gr = _scope_lists(scope, sessions)
        if sc_off is None:
            scopes = None                                                 # nobody is scoped: the C call takes a map with lists alone
        return self._cf_recommend("smatrix_cf_recommend_scoped", (sessions, weights, exclude, deny, sim, shrink), k,
                                  (*_map_args(scopes), _p(sc_off, _lib.u64p), _p(sc_gr), code, *_map_args(groups), int(cap), *_fill_args(fill)),
                                  "scope map, scope lists, mode, group map, cap, fill, sim or shrink", n_scored=True)

    def cf_recommend_scoped_dev(self, n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, scope_ptr, scope_n,
                                sc_off_ptr, sc_groups_ptr, mode, group_ptr, group_n, cap, fill_ptr, n_fill, sim, shrink, k, ids_ptr, scores_ptr,
                                cnt_ptr, n_scored_ptr, stream=None):
        """the same on device arrays (raw pointers, None for what is not given), the C order: cf_recommend_grouped_fill_dev's, and behind
        deny_n scope uint32[scope_n], sc_off uint64[n+1], sc_groups uint32, mode "only" or "except".  A list longer than SCOPE_MAX
        is found on the device: ValueError, the outputs' contents unspecified"""
        _check_k(k)
        _check_cap(cap)
        scope_code = _scope_mode(mode)
        self._cf_recommend_dev("smatrix_cf_recommend_scoped_dev", _DEV_BAD + "scope map, scope lists, mode, group map, cap, fill, sim or shrink",
                               (n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, scope_ptr, scope_n, sc_off_ptr,
                                sc_groups_ptr, scope_code, group_ptr, group_n, int(cap), fill_ptr, n_fill, _sim(sim), _shrink(shrink), k,
                                ids_ptr, scores_ptr, cnt_ptr, n_scored_ptr), stream)

    def cf_recommend_deep(self, sessions, k, weights=None, exclude=None, deny=None, sim="cosine", shrink=0.0):
        """cf_recommend_filtered with up to DEEP_MAX = 1024 results per session (include/smatrix_batch.h smatrix_cf_recommend_deep):
        the candidates for a second-stage ranker, for re-ranking on the caller's side, for recall@k beyond 64.  Every argument is
        cf_recommend_filtered's but k, an integer in 1 .. DEEP_MAX.  -> (ids[n,k], scores[n,k] float64, counts[n]) as there: the
        first 64 entries of a session are cf_recommend_filtered's with k = 64, and cf_rank answers ids[s, r] with the rank r"""
        _check_deep_k(k)
        return self._cf_recommend("smatrix_cf_recommend_deep", (sessions, weights, exclude, deny, sim, shrink), int(k))

    def cf_recommend_deep_dev(self, n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, sim, shrink, k,
                              ids_ptr, scores_ptr, cnt_ptr, stream=None):
        """the same on device arrays (raw pointers, None for what is not given): cf_recommend_sim_dev's, with k up to DEEP_MAX;
        ids uint32[n*k], scores float64[n*k]"""
        _check_deep_k(k)
        self._cf_recommend_dev("smatrix_cf_recommend_deep_dev", _DEV_BAD + "sim or shrink",
                               (n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, _sim(sim), _shrink(shrink), int(k),
                                ids_ptr, scores_ptr, cnt_ptr), stream)

    def cf_rank(self, sessions, targets, weights=None, exclude=None, deny=None, sim="cosine", shrink=0.0):
        """where given items land in each session's ranking (include/smatrix_batch.h smatrix_cf_rank): cf_recommend_filtered's
        arguments without k, and targets, one id sequence per session (it may be empty or repeat an id).
        -> (ranks uint32[T], scores float64[T], n_candidates uint32[n]), the T answers concatenated in session order: the rank of
        a target is the number of the session's candidates that come before it (the position cf_recommend_filtered would give it,
        numbered on past 64) and its score the one returned there; RANK_NONE and 0.0 for a target that is no candidate (the id 0,
        an id in no scanned row, an item of the session, an excluded or denied id).  n_candidates is uncapped"""
        n, measure, sess, filt, tgt, _, t_off = self._cf_front(sessions, weights, exclude, deny, sim, shrink, targets)
        ranks = np.full(int(t_off[-1]), RANK_NONE, dtype=np.uint32)
        scores = np.zeros(ranks.size, dtype=np.float64)
        ncand = np.zeros(n, dtype=np.uint32)
        if n and self._lib.smatrix_cf_rank(*sess, *filt, *measure, *tgt, _p(ranks), _p(scores, _DP), _p(ncand)) != 0:
            raise ValueError("smatrix_cf_rank: bad n_sessions, weights, exclusion lists, deny bitmap, sim or shrink")
        return ranks, scores, ncand

    def cf_rank_dev(self, n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, sim, shrink, t_off_ptr,
                    targets_ptr, ranks_ptr, scores_ptr, ncand_ptr, stream=None):
        """the same on device arrays (raw pointers, None for a filter that is not given): cf_recommend_sim_dev's inputs, and
        t_off uint64[n+1], targets uint32, ranks uint32 and scores float64 parallel to targets, ncand uint32[n]"""
        code, h = _sim(sim), _shrink(shrink)
        if self._lib.smatrix_cf_rank_dev(self._h, n, off_ptr, items_ptr, weights_ptr, ex_off_ptr, ex_items_ptr, deny_ptr, deny_n, code, h,
                                         t_off_ptr, targets_ptr, ranks_ptr, scores_ptr, ncand_ptr, _stream_ptr(stream)) != 0:
            raise ValueError("smatrix_cf_rank_dev: bad n, weights, exclusion lists, deny bitmap, sim, shrink or targets")

    def cf_explain(self, sessions, targets, weights=None, sim="cosine", shrink=0.0):
        """each session item's share of a target's score (include/smatrix_batch.h smatrix_cf_explain): sessions, weights, sim and
        shrink as cf_recommend_filtered takes them, targets one id sequence per session (it may be empty or repeat an id); no
        filters.  -> (terms float64[E], cc uint32[E], e_offsets uint64[n + 1]): session s's block terms[e_offsets[s]:e_offsets[s + 1]]
        reshapes to (its targets, its length); the entry of target t and the position holding item a is w * score(a, t) and
        self[a, t], or 0.0 and 0 when t is 0, a occurred earlier in the session, or a's row does not hold t.  Added left to right,
        a target's terms give the bytes of the score cf_recommend_filtered and cf_rank return for it; explain_table turns the
        arrays into sorted (item, cc, term) lists"""
        n, measure, sess, _, tgt, offsets, t_off = self._cf_front(sessions, weights, None, None, sim, shrink, targets)
        e_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.diff(offsets) * np.diff(t_off), out=e_off[1:])
        terms = np.zeros(int(e_off[-1]), dtype=np.float64)
        cc = np.zeros(int(e_off[-1]), dtype=np.uint32)
        if n and self._lib.smatrix_cf_explain(*sess, *measure, *tgt, _p(terms, _DP), _p(cc)) != 0:
            raise ValueError("smatrix_cf_explain: bad n_sessions, weights, sim or shrink")
        return terms, cc, e_off

    def cf_explain_dev(self, n, off_ptr, items_ptr, weights_ptr, sim, shrink, t_off_ptr, targets_ptr, e_off_ptr, total, terms_ptr,
                       cc_ptr, stream=None):
        """the same on device arrays (raw pointers, None for no weights): off uint64[n+1], items uint32, weights float64 per item,
        t_off uint64[n+1], targets uint32, e_off uint64[n+1] (e_off[s] = the sum of targets * length over the sessions before s),
        total = e_off[n], terms float64[total], cc uint32[total].  A bad weight is found on the device: ValueError, the outputs'
        contents unspecified"""
        code, h = _sim(sim), _shrink(shrink)
        if self._lib.smatrix_cf_explain_dev(self._h, n, off_ptr, items_ptr, weights_ptr, code, h, t_off_ptr, targets_ptr, e_off_ptr, total,
                                            terms_ptr, cc_ptr, _stream_ptr(stream)) != 0:
            raise ValueError("smatrix_cf_explain_dev: bad n, weights, sim, shrink, targets or entry offsets")

    def cf_recommend_explained(self, sessions, k, weights=None, exclude=None, deny=None, sim="cosine", shrink=0.0):
        """cf_recommend_filtered, and cf_explain for what it returned: each session's k returned ids are its targets (unused
        slots hold the id 0 and explain to zeros).  -> (ids[n,k], scores[n,k], counts[n], terms, cc, e_offsets): session s's block
        of terms and cc reshapes to (k, its length)"""
        ids, scores, counts = self.cf_recommend_filtered(sessions, k, weights=weights, exclude=exclude, deny=deny, sim=sim, shrink=shrink)
        terms, cc, e_off = self.cf_explain(sessions, list(ids), weights=weights, sim=sim, shrink=shrink)
        return ids, scores, counts, terms, cc, e_off

    def cf_evaluate(self, sessions, ks=(1, 10, 100), **measure):
        """held-out evaluation of the read path's dials: of every session with at least two distinct ids the LAST id is hidden
        and ranked (cf_rank) against the rest of the session, the hidden id's other occurrences removed from it; -> rank_metrics
        of those ranks (hit rate at each k of ks, MRR).  measure: cf_rank's weights (shaped like sessions: a removed position's
        weight goes with it), exclude, deny, sim, shrink.
        Caveat (leave-one-out): sessions that are already counted in the matrix flatter the result -- the hidden id's
        co-occurrence with the rest of its session is in the very counts it is ranked by.  Evaluate with sessions that were not
        imported"""
        weights, exclude = measure.pop("weights", None), measure.pop("exclude", None)
        if weights is not None:
            _weights_shape(weights, sessions)
        if exclude is not None and len(exclude) != len(sessions):
            raise ValueError("exclude must hold one id sequence per session")
        q, tg, qw, qe = [], [], [], []
        for i, s in enumerate(sessions):
            s = np.asarray(s, dtype=np.uint32)
            if np.unique(s).size < 2:
                continue
            keep = s != s[-1]
            q.append(s[keep]); tg.append(s[-1:])
            if weights is not None:
                qw.append(np.asarray(weights[i], dtype=np.float64)[keep])
            if exclude is not None:
                qe.append(exclude[i])
        ranks, _, _ = self.cf_rank(q, tg, weights=qw if weights is not None else None, exclude=qe if exclude is not None else None, **measure)
        return rank_metrics(ranks, ks)

    def cf_import_sessions(self, sessions):
        """CF-recommender write path (examples/cf_recommender.c:36-47): every session is a sequence of item ids; all
        their L*L incr ops are generated and applied on the GPU"""
        offsets, ids = _sessions(sessions)
        if self._lib.smatrix_cf_import_sessions(self._h, len(sessions), offsets.ctypes.data_as(_lib.u64p), _p(ids)) != 0:
            raise ValueError("smatrix_cf_import_sessions")

    def cf_import_sessions_dev(self, n_sessions, off_ptr, ids_ptr, op_off_ptr, total_ops, stream=None):
        self._lib.smatrix_cf_import_sessions_dev(self._h, n_sessions, off_ptr, ids_ptr, op_off_ptr, total_ops, stream)

    def cf_import_events(self, sessions, amounts=None, window=0, forward=False, no_self=False, forget=False, max_batch=0):
        """the write path with a window, amounts and a way back (include/smatrix_batch.h smatrix_cf_import_events): per position
        p with amount w_p != 0 the head op (id_p, 0, w_p), per ordered pair of positions p != q with non-zero amounts the pair op
        (id_p, id_q, min(w_p, w_q)) -- within `window` positions of each other (0: no limit), only q > p with forward, only
        id_p != id_q with no_self.  amounts: one entry per session, a sequence of the session's length or one integer for all
        its positions (None: 1 everywhere).  forget: the ops are decr, which takes an earlier import with the same arguments
        out again, exactly.  Generated and applied on the GPU in internal batches of at most max_batch ops (0: 2**25).
        -> the number of ops applied.  The defaults apply cf_import_sessions' ops"""
        _check_u32("window", window)
        if amounts is not None:
            amounts = _amounts(amounts, sessions)
        offsets, ids = _sessions(sessions)
        n_ops = C.c_uint64(0)
        if self._lib.smatrix_cf_import_events(self._h, OP_DECR if forget else OP_INCR, len(sessions), offsets.ctypes.data_as(_lib.u64p),
                                              _p(ids), _p(amounts), int(window), _import_flags(forward, no_self), int(max_batch),
                                              C.byref(n_ops)) != 0:
            raise ValueError("smatrix_cf_import_events refused: more than 2**32 - 1 sessions, or 2**63 slots or more")
        return n_ops.value

    def cf_forget_sessions(self, sessions, **kw):
        """cf_import_events(sessions, ..., forget=True): takes out what cf_import_events with the same arguments put in"""
        return self.cf_import_events(sessions, **dict(kw, forget=True))

    def cf_import_events_dev(self, op, n, off_ptr, ids_ptr, amounts_ptr, window, flags, max_batch=0, stream=None):
        """the same on device arrays (raw pointers; amounts_ptr None: every amount 1; op OP_INCR or OP_DECR; flags IMPORT_FORWARD |
        IMPORT_NO_SELF): -> the number of ops applied; the work is complete on `stream` when this returns"""
        _check_u32("window", window)
        n_ops = C.c_uint64(0)
        if self._lib.smatrix_cf_import_events_dev(self._h, int(op), n, off_ptr, ids_ptr, amounts_ptr, int(window), int(flags), int(max_batch),
                                                  C.byref(n_ops), stream) != 0:
            raise ValueError("smatrix_cf_import_events_dev refused: op, flags, n, offsets that decrease, or 2**63 slots or more")
        return n_ops.value

    # device-pointer flavours (raw pointers; stream = hipStream_t as int or None)
    def apply_batch_dev(self, op, n, x_ptr, y_ptr, v_ptr, out_ptr, stream=None):
        self._lib.smatrix_apply_batch_dev(self._h, op, n, x_ptr, y_ptr, v_ptr, out_ptr, stream)

    def apply_packed_dev(self, op, n, rec_ptr, width, out_ptr, stream=None):
        """n records {x,y} (width 2, get) or {x,y,v} (width 3) in ONE device array"""
        if self._lib.smatrix_apply_packed_dev(self._h, op, n, rec_ptr, width, out_ptr, stream):
            raise ValueError("smatrix_apply_packed_dev: bad width / op")

    def rowlen_batch_dev(self, n, x_ptr, out_ptr, stream=None):
        self._lib.smatrix_rowlen_batch_dev(self._h, n, x_ptr, out_ptr, stream)

    def getrow_batch_dev(self, n, x_ptr, off_ptr, ret_ptr, cnt_ptr, stream=None):
        self._lib.smatrix_getrow_batch_dev(self._h, n, x_ptr, off_ptr, ret_ptr, cnt_ptr, stream)

    def cf_neighbors_batch_dev(self, n, items_ptr, off_ptr, ids_ptr, scores_ptr, cnt_ptr, stream=None):
        self._lib.smatrix_cf_neighbors_batch_dev(self._h, n, items_ptr, off_ptr, ids_ptr, scores_ptr, cnt_ptr, stream)

    # ---- whole-matrix export (include/smatrix_batch.h smatrix_export) -------------------
    def export(self, order="sorted"):
        """every row and its pairs as CSR: -> (rows uint32[n], row_ptr uint64[n+1], pairs uint32[nnz, 2] {column, value}).
        "sorted": rows by id, pairs by column; "table": directory-slot order, each row's pairs in table-slot order
        (getrow_batch's bytes).  A size query, then the export; a matrix that grew in between raises."""
        o = _export_order(order)
        n, nnz = C.c_uint64(0), C.c_uint64(0)
        self._lib.smatrix_export(self._h, o, 0, 0, None, None, None, C.byref(n), C.byref(nnz))
        rows = np.zeros(n.value, np.uint32)
        row_ptr = np.zeros(n.value + 1, np.uint64)
        pairs = np.zeros((nnz.value, 2), np.uint32)
        n2, nnz2 = C.c_uint64(0), C.c_uint64(0)
        rc = self._lib.smatrix_export(self._h, o, n.value, nnz.value, _p(rows), row_ptr.ctypes.data_as(_lib.u64p),
                                      pairs.ctypes.data_as(_lib.u32p), C.byref(n2), C.byref(nnz2))
        if rc != 0:
            raise RuntimeError("smatrix_export: the matrix grew between the size query (%d rows, %d pairs) and the export "
                               "(%d rows, %d pairs)" % (n.value, nnz.value, n2.value, nnz2.value))
        return rows, row_ptr, pairs

    def export_dev(self, order="sorted", stream=None):
        """the same on the matrix's GPU: -> torch tensors (rows int32[n] (the uint32 ids' bits), row_ptr int64[n+1],
        pairs int32[nnz, 2]).  stream: a torch.cuda.Stream (None: the legacy default stream); the export has completed on it
        when this returns."""
        import torch
        o = _export_order(order)
        dev = torch.device("cuda", self._device if self._device is not None else torch.cuda.current_device())
        sp = stream.cuda_stream if stream is not None else None
        n, nnz = C.c_uint64(0), C.c_uint64(0)
        self._lib.smatrix_export_dev(self._h, o, 0, 0, None, None, None, C.byref(n), C.byref(nnz), sp)
        with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.default_stream(dev)):
            rows = torch.empty(n.value, dtype=torch.int32, device=dev)
            row_ptr = torch.empty(n.value + 1, dtype=torch.int64, device=dev)
            pairs = torch.empty((nnz.value, 2), dtype=torch.int32, device=dev)
        n2, nnz2 = C.c_uint64(0), C.c_uint64(0)
        rc = self._lib.smatrix_export_dev(self._h, o, n.value, nnz.value, rows.data_ptr(), row_ptr.data_ptr(), pairs.data_ptr(),
                                          C.byref(n2), C.byref(nnz2), sp)
        if rc != 0:
            raise RuntimeError("smatrix_export_dev: the matrix grew between the size query (%d rows, %d pairs) and the export "
                               "(%d rows, %d pairs)" % (n.value, nnz.value, n2.value, nnz2.value))
        return rows, row_ptr, pairs

    def to_sparse_coo(self, size=None):
        """the matrix as a coalesced torch.sparse_coo_tensor on its GPU, from the SORTED export: indices int64 [2, nnz]
        (row, column), values int64 (the uint32 values, zero-extended).  size: default (largest row id + 1, largest column
        + 1) -- torch needs rows * columns < 2**63, so the whole id space (2**32, 2**32) is not a shape it can hold."""
        import torch
        rows, row_ptr, pairs = self.export_dev("sorted")
        mask = 0xFFFFFFFF
        x = torch.repeat_interleave(rows.to(torch.int64) & mask, row_ptr[1:] - row_ptr[:-1])
        y = pairs[:, 0].to(torch.int64) & mask
        v = pairs[:, 1].to(torch.int64) & mask
        if size is None:
            size = (int(x.max().item()) + 1 if x.numel() else 0, int(y.max().item()) + 1 if y.numel() else 0)
        if size[0] * size[1] >= 1 << 63:
            raise ValueError("to_sparse_coo: a %d x %d tensor is beyond torch's element count (rows * columns < 2**63)" % tuple(size))
        return torch.sparse_coo_tensor(torch.stack([x, y]), v, size=tuple(size), is_coalesced=True)

    # ---- merge of two matrices, CSR import (include/smatrix_batch.h smatrix_merge / smatrix_import_csr) ----
    def _merge_call(self, name, other, op, *args, check=None, max_batch=0):
        """smatrix_<name>(self, other, op, *args, max_batch, &n_ops[, &n_dropped]) behind the checks, none of which touches a
        handle: the op, the flavour's own arguments (check), other's type.  check given: the flavour drops pairs, and
        -> (ops applied, pairs dropped); else -> ops applied."""
        o = _merge_op(op)
        if check:
            check(*args)
        if not isinstance(other, SparseMatrix):
            raise TypeError("%s needs another SparseMatrix, not %r" % (name, type(other).__name__))
        out = [C.c_uint64(0) for _ in range(2 if check else 1)]
        if getattr(self._lib, "smatrix_" + name)(self._h, other._h, o, *(a if isinstance(a, float) else int(a) for a in args), int(max_batch), *map(C.byref, out)) != 0:
            raise ValueError("smatrix_%s refused: a matrix cannot be merged into itself, and both must be on one device" % name)
        return tuple(v.value for v in out) if check else out[0].value

    def _copy_by(self, method, filename, *args):
        """a NEW matrix (filename: see SparseMatrix) filled by method(new, self, *args); closed again if that raises"""
        m = SparseMatrix(filename)
        try:
            method(m, self, *args)
        except Exception:
            m.close()
            raise
        return m

    def merge(self, other, op="incr", max_batch=0):
        """self[x, y] op= other[x, y] for every pair of other, on the GPU in internal batches of at most
        max(max_batch, other's longest row) ops (0: 2**24): -> the number of ops applied.  other is not modified."""
        return self._merge_call("merge", other, op, max_batch=max_batch)

    def merge_scaled(self, other, op="incr", num=1, den=1, min_value=0, max_batch=0):
        """merge with a decay and a filter: every pair (y, v) of other becomes v' = v * num // den and is dropped when
        v' < min_value (or when it would be the empty cell (0, 0)); the others are applied as self[x, y] op= v'.
        1 <= num <= den <= 2**32 - 1.  -> (ops applied, pairs dropped).  other is not modified."""
        return self._merge_call("merge_scaled", other, op, num, den, min_value, check=_scale_args, max_batch=max_batch)

    def pruned(self, min_value=1, num=1, den=1, filename=None):
        """a NEW matrix (in memory, or file-backed when filename is given) that holds self's pairs scaled by num / den, without
        those below min_value: no dead cells, row tables as small as the survivors allow -- the end of a sliding-window cycle
        (total += today; total -= day_30; total = total.pruned()).  self is not modified."""
        _scale_args(num, den, min_value)
        return self._copy_by(SparseMatrix.merge_scaled, filename, "set", num, den, min_value)

    def merge_topk(self, other, m, op="set", min_value=1, max_batch=0, rank="value", shrink=0.0):
        """merge that keeps the m heaviest pairs of every row of other: of the pairs (y != 0, v >= min_value) those of the largest
        v, equal values by ascending column; the column-0 pair (the CF total) is kept beside them when v >= min_value.  The kept
        pairs are applied as self[x, y] op= v.  1 <= m <= 2**32 - 1.  -> (ops applied, pairs dropped).  other is not modified.
        rank="cosine" (smatrix_merge_topk_by): the m pairs that SCORE best in cf_neighbors_batch / cf_topk_batch /
        cf_recommend_batch, v / (sqrt(other[x, 0]) * sqrt(other[y, 0])) with their guards, equal scores by ascending column;
        the values applied are still the raw v.
        rank="jaccard" / "lift", and any scoring rank with shrink > 0 (smatrix_merge_topk_sim): the m pairs that score best in
        cf_recommend_filtered(sim=rank, shrink=shrink), whose score it is."""
        rank, h = _rank_args(rank, shrink)
        if rank == "value":
            return self._merge_call("merge_topk", other, op, m, min_value, check=_topk_args, max_batch=max_batch)
        if rank == "cosine" and h == 0.0:
            return self._merge_call("merge_topk_by", other, op, _RANKS[rank], m, min_value, check=_topk_by_args, max_batch=max_batch)
        return self._merge_call("merge_topk_sim", other, op, _SIMS[rank], h, m, min_value, check=_topk_sim_args, max_batch=max_batch)

    def truncated(self, m, min_value=1, filename=None, rank="value", shrink=0.0):
        """a NEW matrix (in memory, or file-backed when filename is given) that holds, of every row of self, the m heaviest pairs
        of at least min_value and the column-0 pair: at most m + 1 pairs per row, the serving copy of an item-kNN recommender
        (total += today; total -= day_30; serving = total.truncated(m)).  self is not modified.
        rank="cosine": the m best-scoring pairs instead of the m heaviest, so that the copy's cf_topk_batch(items, k <= m)
        returns the scores self's does.  rank="jaccard" / "lift" and shrink: as merge_topk -- the copy serves
        cf_recommend_filtered(sim=rank, shrink=shrink) of one-item sessions, k <= m, as self does."""
        _rank_args(rank, shrink)
        _topk_args(m, min_value)
        return self._copy_by(SparseMatrix.merge_topk, filename, m, "set", min_value, 0, rank, shrink)

    def __iadd__(self, other):
        if not isinstance(other, SparseMatrix):
            return NotImplemented
        self.merge(other, "incr")
        return self

    def __isub__(self, other):
        if not isinstance(other, SparseMatrix):
            return NotImplemented
        self.merge(other, "decr")
        return self

    def import_csr(self, rows, row_ptr, pairs, op="set", max_batch=0):
        """the inverse of export(): one op per pair of the CSR (rows uint32[n], row_ptr uint64[n+1], pairs uint32[nnz, 2]
        {column, value}); a row id or a column may repeat (set: the last occurrence wins): -> the number of ops applied"""
        o = _merge_op(op)
        rows = _u32(rows)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        pairs = _u32(pairs)
        if row_ptr.size != rows.size + 1:
            raise ValueError("row_ptr must hold len(rows) + 1 entries")
        if rows.size and 2 * int(row_ptr[-1]) > pairs.size:
            raise ValueError("pairs holds %d pairs, row_ptr[-1] names %d" % (pairs.size // 2, int(row_ptr[-1])))
        n = C.c_uint64(0)
        if self._lib.smatrix_import_csr(self._h, o, rows.size, _p(rows), row_ptr.ctypes.data_as(_lib.u64p), _p(pairs),
                                        int(max_batch), C.byref(n)) != 0:
            raise ValueError("smatrix_import_csr refused: row_ptr must start at 0 and never decrease")
        return n.value

    def import_csr_dev(self, rows, row_ptr, pairs, op="set", max_batch=0, stream=None, n_rows=None):
        """the same on device arrays: torch tensors as export_dev() returns them (rows int32[n], row_ptr int64[n+1],
        pairs int32[nnz, 2], contiguous, on the matrix's GPU), or raw device pointers with n_rows given.  stream: a
        torch.cuda.Stream or a hipStream_t as int (None: the legacy default stream); the import has completed on it when
        this returns."""
        o = _merge_op(op)
        if n_rows is None:
            for name, t, size in (("rows", rows, 4), ("row_ptr", row_ptr, 8), ("pairs", pairs, 4)):
                if not t.is_cuda or not t.is_contiguous() or t.element_size() != size or t.is_floating_point():
                    raise ValueError("%s must be a contiguous %d-byte integer tensor on the GPU" % (name, size))
            n_rows = rows.numel()
            if row_ptr.numel() != n_rows + 1:
                raise ValueError("row_ptr must hold len(rows) + 1 entries")
            if n_rows and 2 * int(row_ptr[-1].item()) > pairs.numel():
                raise ValueError("pairs holds %d pairs, row_ptr[-1] names %d" % (pairs.numel() // 2, int(row_ptr[-1].item())))
            rows, row_ptr, pairs = rows.data_ptr(), row_ptr.data_ptr(), pairs.data_ptr()
        sp = getattr(stream, "cuda_stream", stream)
        n = C.c_uint64(0)
        if self._lib.smatrix_import_csr_dev(self._h, o, int(n_rows), rows, row_ptr, pairs, int(max_batch), C.byref(n), sp) != 0:
            raise ValueError("smatrix_import_csr_dev refused: row_ptr must start at 0 and never decrease")
        return n.value

    def from_sparse_coo(self, t, op="incr", max_batch=0):
        """the inverse of to_sparse_coo(): one op per stored element of a 2-d torch.sparse_coo_tensor of integer values on
        the matrix's GPU, coalesced or not (an uncoalesced tensor's repeated indices are repeated ops).  Values are taken
        modulo 2**32; an index beyond uint32 raises ValueError: -> the number of ops applied"""
        import torch
        o = _merge_op(op)
        if t.layout != torch.sparse_coo or t.dim() != 2 or t.dense_dim() != 0:
            raise ValueError("from_sparse_coo needs a 2-d torch.sparse_coo_tensor")
        if not t.is_cuda or (self._device is not None and t.device.index != self._device):
            raise ValueError("from_sparse_coo: the tensor must be on the matrix's GPU")
        idx, val = t._indices(), t._values()
        if val.is_floating_point() or val.is_complex() or val.dtype == torch.bool:
            raise ValueError("from_sparse_coo: integer values only, not %s" % (val.dtype,))
        if idx.numel() and (int(idx.min().item()) < 0 or int(idx.max().item()) > 0xFFFFFFFF):
            raise ValueError("from_sparse_coo: an index is beyond uint32")
        nnz = idx.shape[1]
        # every element a row of its own: rows = x, row_ptr = 0..nnz, pairs = {y, v}
        def low32(a):       # the low 32 bits of an int64 tensor as int32 bits
            return (((a & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000).to(torch.int32)
        rows = low32(idx[0]).contiguous()
        row_ptr = torch.arange(nnz + 1, dtype=torch.int64, device=idx.device)
        pairs = torch.stack([low32(idx[1]), low32(val.to(torch.int64))], dim=1).contiguous()
        return self.import_csr_dev(rows, row_ptr, pairs, o, max_batch)

    # ---- introspection --------------------------------------------------------
    def stats(self):
        st = _lib.Stats()
        self._lib.smatrix_stats_sz(self._h, C.byref(st), C.sizeof(st))
        out = {n: getattr(st, n) for n, t in _lib.Stats._fields_ if t is C.c_uint64 or t is C.c_double}
        for i, op in enumerate(("get", "set", "incr", "decr")):
            out["kernel_ms_" + op] = st.kernel_ms[i]
            out["kernel_launches_" + op] = st.kernel_launches[i]
            out["kernel_ops_" + op] = st.kernel_ops[i]
        return out

    def reserve(self, nbytes):
        """capacity hint: map at least nbytes of device memory for row tables now (include/smatrix_batch.h smatrix_reserve)"""
        self._lib.smatrix_reserve(self._h, int(nbytes))

    def flush(self):
        """file mode: dirty rows reach the backing file now (include/smatrix_batch.h smatrix_flush)"""
        self._lib.smatrix_flush(self._h)

    def compact(self):
        """file mode: rewrite the backing file without leaked blocks (include/smatrix_batch.h smatrix_compact)"""
        if self._lib.smatrix_compact(self._h) != 0:
            raise RuntimeError("smatrix_compact did nothing: it is experimental and needs SMATRIX_EXPERIMENTAL=1 in the environment")

    def profile(self, on=True):
        self._lib.smatrix_profile(self._h, int(on))

    def row_info(self, x):
        size, used = C.c_uint32(0), C.c_uint32(0)
        ok = self._lib.smatrix_row_info(self._h, x, C.byref(size), C.byref(used))
        return (size.value, used.value) if ok else None

    def row_slots(self, x):
        info = self.row_info(x)
        if info is None:
            return None
        kv = np.zeros(2 * info[0], dtype=np.uint32)
        self._lib.smatrix_row_slots(self._h, x, _p(kv), info[0])
        return kv.reshape(-1, 2)


def device_available():
    return bool(_lib.load().smatrix_device_available())
