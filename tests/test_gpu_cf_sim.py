"""GPU (-m gpu): the similarity calls (include/smatrix_batch.h smatrix_cf_recommend_sim / _dev, smatrix_merge_topk_sim;
SparseMatrix.cf_recommend_filtered(sim=, shrink=), cf_recommend_sim_dev, merge_topk / truncated(rank=, shrink=)).

Expected results: the numpy model of tests/cf_sim_helpers.py over the matrix's own export("sorted") -- scores in float64 with the
two-step denominator, a session's terms added left to right, a row's kept pairs by (score bits descending, column ascending).
Ids, counts and the scores' BYTES must match.  The matrix is cf_sim_helpers.world_ops(): tests/test_cf_sim_model.py shows, without
a GPU, that it holds pairs whose score changes under a fused denominator for COSINE at shrink 0.1 and for LIFT at shrink 0.5, in
rows that cases 2, 3 and 4 read."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix, _lib
from tests import cf_sim_helpers as H
from tests.test_gpu_merge_topk_by import sessions_uniform, sessions_zipf

pytestmark = pytest.mark.gpu

SET, DECR = 1, 3
DP = C.POINTER(C.c_double)
LDS_SLOTS = 4096                                  # kernels/recommend.hpp REC_LDS_SLOTS
MEASURES = [(sim, h) for sim in ("cosine", "jaccard", "lift") for h in (0.0, 0.1, 10.0)]


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


class World:
    pass


@pytest.fixture(scope="module")
def world():
    w = World()
    w.m = SparseMatrix()
    ops = H.world_ops()
    w.m.apply_batch(SET, *ops, results=False)
    w.m.apply_batch(DECR, *H.dead_cells(ops), results=False)
    for b, t in H.BIG_TOTALS.items():                                     # the scalar call: the mirror's values are the ones that score
        w.m.set(b, 0, t)
    w.cand = H.world_contents()
    w.export = w.m.export("sorted")
    for got, want in zip(w.export, H.sorted_export_of(w.cand)):
        assert got.tobytes() == want.tobytes()                            # the matrix holds what the model test looked at
    w.model = H.SessionModel(w.export)
    assert w.m.row_info(H.HOT)[0] == 16384 and w.m.row_info(11)[0] == 64 and w.m.row_info(12)[0] == 512
    yield w
    w.m.close()


def need(m, sess, E=0):
    """k_rec_bound's sum: the slots of the distinct items' rows + the session's length + its exclusion list's"""
    return sum((m.row_info(a) or (0, 0))[0] for a in set(int(v) for v in sess)) + len(sess) + E


def flat(sessions, dtype):
    off = np.zeros(len(sessions) + 1, np.uint64)
    np.cumsum([len(s) for s in sessions], out=off[1:])
    return off, np.ascontiguousarray(np.concatenate([np.asarray(s, dtype) for s in sessions] + [np.zeros(0, dtype)]), dtype=dtype)


def compare(w, got, sessions, k, sim, shrink, weights=None, exclude=None, deny=(), tag=""):
    ids, sc, cnt = got
    for s, sess in enumerate(sessions):
        wi, ws = w.model.session(sess, k, H.SIMS[sim], shrink, None if weights is None else weights[s],
                                 () if exclude is None else exclude[s], deny)
        c = int(cnt[s])
        assert c == len(wi), (tag, sim, shrink, s, c, len(wi))
        assert ids[s, :c].tolist() == wi, (tag, sim, shrink, s)
        assert sc[s, :c].tobytes() == ws.tobytes(), (tag, sim, shrink, s, sc[s, :c], ws)
        assert not ids[s, c:].any() and not sc[s, c:].any(), (tag, s)      # the host flavour zero-fills


def raw_sim(m, sessions, k, sim, shrink, out=None):
    """smatrix_cf_recommend_sim itself, nothing filtered -> (return code, ids, scores, counts)"""
    off, items = flat(sessions, np.uint32)
    n = len(sessions)
    ids, sc, cnt = out or (np.zeros((n, k), np.uint32), np.zeros((n, k), np.float64), np.zeros(n, np.uint32))
    rc = m._lib.smatrix_cf_recommend_sim(m._h, n, off.ctypes.data_as(_lib.u64p), items.ctypes.data_as(_lib.u32p), None, None, None, None, 0,
                                         sim, shrink, k, ids.ctypes.data_as(_lib.u32p), sc.ctypes.data_as(DP), cnt.ctypes.data_as(_lib.u32p))
    return rc, ids, sc, cnt


def same_bytes(a, b):
    return all(u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes() for u, v in zip(a, b))


# ---- 1: (COSINE, 0.0) is the existing calls -----------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [sessions_uniform, sessions_zipf])
def test_cosine_without_shrinkage_is_the_existing_calls(make):
    sessions = make()
    total = SparseMatrix()
    total.cf_import_sessions(sessions)
    rng = np.random.default_rng(1)
    q = [s.tolist() for s in sessions[:60]] + [[int(sessions[0][0])], []]
    weights = [(rng.random(len(s)) * 4).tolist() for s in q]
    exclude = [rng.integers(1, 301, 5).tolist() for _ in q]
    deny = list(range(3, 300, 7))
    n, k = len(q), 10
    off, items = flat(q, np.uint32)
    _, wf = flat(weights, np.float64)
    ex_off, ex = flat(exclude, np.uint32)
    bits, deny_n = np.zeros(10, np.uint32), 300
    for b in deny:
        bits[b >> 5] |= np.uint32(1 << (b & 31))
    p32, p64 = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p))
    for given in (False, True):
        want = total.cf_recommend_filtered(q, k, **(dict(weights=weights, exclude=exclude, deny=deny) if given else {}))
        got = (np.zeros((n, k), np.uint32), np.zeros((n, k), np.float64), np.zeros(n, np.uint32))
        rc = total._lib.smatrix_cf_recommend_sim(total._h, n, p64(off), p32(items), wf.ctypes.data_as(DP) if given else None,
                                                 p64(ex_off) if given else None, p32(ex) if given else None, p32(bits) if given else None,
                                                 deny_n if given else 0, H.SIM_COSINE, 0.0, k, p32(got[0]), got[1].ctypes.data_as(DP), p32(got[2]))
        assert rc == 0 and same_bytes(want, got), given
        assert want[2].sum() > 0
    for m in (8, 1000):
        a, b = SparseMatrix(), SparseMatrix()
        na, nb = C.c_uint64(0), C.c_uint64(0)
        da, db = C.c_uint64(0), C.c_uint64(0)
        assert a._lib.smatrix_merge_topk_sim(a._h, total._h, SET, H.SIM_COSINE, 0.0, m, 1, 0, C.byref(na), C.byref(da)) == 0
        assert b._lib.smatrix_merge_topk_by(b._h, total._h, SET, 1, m, 1, 0, C.byref(nb), C.byref(db)) == 0
        assert (na.value, da.value) == (nb.value, db.value) and na.value > 0
        assert same_bytes(a.export("sorted"), b.export("sorted")), m
        a.close(); b.close()
    total.close()


# ---- 2: the recommend call against the model ----------------------------------------------------------------------------------
def test_the_sessions_reach_both_tiers(world):
    w = world
    assert max(need(w.m, s) for s in H.lds_sessions()) <= LDS_SLOTS
    assert all(need(w.m, s) > LDS_SLOTS for s in H.global_sessions())


@pytest.mark.parametrize("sim,shrink", MEASURES)
def test_recommendations_are_the_models_bit_for_bit(world, sim, shrink):
    w = world
    sessions = H.all_sessions()
    for k in (10, 64):
        got = w.m.cf_recommend_filtered(sessions, k, sim=sim, shrink=shrink)
        compare(w, got, sessions, k, sim, shrink, tag="k %d" % k)
        again = w.m.cf_recommend_filtered(sessions, k, sim=sim, shrink=shrink)
        assert same_bytes(got, again)                                     # the same input twice gives the same bytes
    assert got[2].sum() > 100


@pytest.mark.parametrize("sim,shrink", [("jaccard", 10.0), ("lift", 0.5), ("cosine", 0.1)])
def test_weights_exclusion_lists_and_deny_with_another_measure_and_the_dev_flavour(world, sim, shrink):
    import torch
    w = world
    rng = np.random.default_rng(6)
    sessions = H.all_sessions()
    k, n = 10, len(sessions)
    weights = [(rng.random(len(s)) * 4).tolist() for s in sessions]
    weights[sessions.index([303, H.HOT, H.HOT, 0, H.ABSENT, 303])] = [0.5, 3.0, 0.0, 0.25, 1.0, 7.0]      # the first position's weight counts
    exclude = [[b for b, _ in w.model.ranking(s, H.SIMS[sim], shrink)[:7]] + [0, 305] for s in sessions]
    deny = [H.HOT, 302, H.NO_ROW_COLUMN] + list(range(50001, 50400, 5)) + list(range(70001, 90000, 3))
    got = w.m.cf_recommend_filtered(sessions, k, weights=weights, exclude=exclude, deny=deny, sim=sim, shrink=shrink)
    compare(w, got, sessions, k, sim, shrink, weights, exclude, deny, tag="filtered")
    ids, sc, cnt = got
    off, items = flat(sessions, np.uint32)
    _, wf = flat(weights, np.float64)
    ex_off, ex_ids = flat(exclude, np.uint32)
    deny_n = max(deny) + 1
    bits = np.zeros((deny_n + 31) // 32, np.uint32)
    for b in deny:
        bits[b >> 5] |= np.uint32(1 << (b & 31))
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.Stream(device=dev)
    outs = []
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)             # noqa: E731
        d_off, d_items, d_w = up(off, np.int64), up(items, np.int32), torch.from_numpy(wf).to(dev)
        d_exoff, d_ex, d_bits = up(ex_off, np.int64), up(ex_ids, np.int32), up(bits, np.int32)
        for _ in range(2):
            d_ids = torch.zeros(n * k, dtype=torch.int32, device=dev)
            d_sc = torch.zeros(n * k, dtype=torch.float64, device=dev)
            d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
            w.m.cf_recommend_sim_dev(n, d_off.data_ptr(), d_items.data_ptr(), d_w.data_ptr(), d_exoff.data_ptr(), d_ex.data_ptr(),
                                     d_bits.data_ptr(), deny_n, sim, shrink, k, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), stream=st)
            outs.append((d_ids, d_sc, d_cnt))
    st.synchronize()
    for d_ids, d_sc, d_cnt in outs:                 # (the outputs were zeroed, so the whole arrays match the host flavour's)
        assert d_ids.cpu().numpy().tobytes() == ids.tobytes()
        assert d_sc.cpu().numpy().tobytes() == sc.tobytes()
        assert d_cnt.cpu().numpy().tobytes() == cnt.tobytes()


# ---- 3: the truncation against the model --------------------------------------------------------------------------------------
def truncate(w, sim, shrink, m, min_value, max_batch=0):
    """dst.merge_topk(rank=sim, shrink=shrink) into an empty matrix, compared with the model -> dst's export("sorted")"""
    ops, dropped = H.topk_sim(w.cand, H.SIMS[sim], shrink, m, min_value)
    dst = SparseMatrix()
    n, d = dst.merge_topk(w.m, m, "set", min_value, max_batch=max_batch, rank=sim, shrink=shrink)
    got = dst.export("sorted")
    dst.close()
    tag = (sim, shrink, m, min_value, max_batch)
    print("%s: %d candidates, %d kept, %d dropped (library: %d, %d)" % (tag, w.cand[0].size, ops[0].size, dropped, n, d))
    assert (n, d) == (ops[0].size, dropped), tag
    want = H.sorted_export_of(ops)
    assert got[0].tobytes() == want[0].tobytes(), (tag, "the rows")
    assert got[1].tobytes() == want[1].tobytes(), (tag, "the rows' pair counts")
    assert got[2].tobytes() == want[2].tobytes(), (tag, "the pairs")
    return got


@pytest.mark.parametrize("sim,shrink", [("jaccard", 0.0), ("lift", 0.0), ("cosine", 0.1), ("jaccard", 10.0), ("lift", 0.5), ("cosine", 10.0)])
def test_the_truncation_keeps_the_models_pairs(world, sim, shrink):
    w = world
    for min_value in (1, 0):                                              # 0: row 15's dead cells are eligible, and score 0
        rows, row_ptr, pairs = truncate(w, sim, shrink, H.M, min_value)
        kept = dict(zip(rows.tolist(), np.diff(row_ptr.astype(np.int64)).tolist()))
        assert kept[10] == 5 + 1                                          # at most m eligible pairs: all of them
        assert kept[11] == kept[12] == kept[H.HOT] == kept[14] == kept[17] == H.M + 1
        assert kept[H.NO_HEAD_ROW] == H.M
        assert kept[15] == H.M + 1
        r14 = pairs[int(row_ptr[rows.tolist().index(14)]):int(row_ptr[rows.tolist().index(14) + 1]), 0]
        assert r14.tolist() == [0] + H.TIE_COLUMNS[:H.M].tolist()         # every score ties: the lowest columns


def test_a_row_of_dead_cells_and_few_live_ones_takes_dead_cells_at_min_value_0(world):
    w = world
    m = 25                                                                # row 15: 20 live pairs, 10 dead cells
    for min_value, want in ((0, 25), (1, 20)):
        rows, row_ptr, pairs = truncate(w, "lift", 0.5, m, min_value)
        i = rows.tolist().index(15)
        p = pairs[int(row_ptr[i]):int(row_ptr[i + 1])]
        assert p.shape[0] == want + 1 and np.count_nonzero(p[:, 1] == 0) == want - 20


def test_the_truncation_does_not_depend_on_max_batch(world):
    w = world
    a = truncate(w, "jaccard", 10.0, H.M, 1, max_batch=0)
    for mb in (1, 100):
        assert same_bytes(a, truncate(w, "jaccard", 10.0, H.M, 1, max_batch=mb)), mb


# ---- 4: the lift contraction case ---------------------------------------------------------------------------------------------
def test_totals_beyond_2_to_the_26_score_with_the_two_step_denominator(world):
    """A * B is beyond 2^53 between two BIG items: it rounds before 0.5 is added.  The model test shows that rows 17 and 60001 hold
    pairs whose score differs under a fused denominator; here the library's scores of exactly those rows are the model's bits"""
    w = world
    sessions = [[17], [60001], [int(b) for b in H.BIG], [60003, 17]]
    got = w.m.cf_recommend_filtered(sessions, 64, sim="lift", shrink=0.5)
    compare(w, got, sessions, 64, "lift", 0.5, tag="lift, big totals")
    assert got[2][0] == 25 and got[2][1] == 7 and (got[1][1, :7] > 0).all()
    truncate(w, "lift", 0.5, 3, 1)


# ---- 5: serving -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [sessions_uniform, sessions_zipf])
def test_a_truncated_copy_serves_one_item_sessions_as_the_source_does(make):
    sessions = make()
    assert all(np.unique(s).size == s.size for s in sessions)             # repetition-free: the source holds no self-pair
    total = SparseMatrix()
    total.cf_import_sessions(sessions)
    items = np.unique(np.concatenate(sessions))
    q = [[int(a)] for a in items]
    for sim in ("jaccard", "lift"):
        for shrink in (0.0, 10.0):
            t = total.truncated(8, rank=sim, shrink=shrink)
            for k in (8, 3):
                want = total.cf_recommend_filtered(q, k, sim=sim, shrink=shrink)
                got = t.cf_recommend_filtered(q, k, sim=sim, shrink=shrink)
                assert same_bytes(want, got), (sim, shrink, k)
                assert (want[2] > 0).all()
            t.close()
    total.close()


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(world):
    import torch
    w = world
    sessions = [[300, 301, 302], [H.HOT, 303], [310]]
    n, k = len(sessions), 10
    sentinel = lambda: (np.full((n, k), 0xabcdef, np.uint32), np.full((n, k), -7.5), np.full(n, 99, np.uint32))   # noqa: E731
    off, items = flat(sessions, np.uint32)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_off, d_items = torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(items.view(np.int32)).to(dev)
    d_ids = torch.full((n * k,), 0xabcdef, dtype=torch.int32, device=dev)
    d_sc = torch.full((n * k,), -7.5, dtype=torch.float64, device=dev)
    d_cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
    bad = [(H.SIM_LIFT, -1.0), (H.SIM_LIFT, float("nan")), (H.SIM_LIFT, float("inf")), (H.SIM_COSINE, -1.0), (3, 0.0), (-1, 1.0), (7, float("nan"))]
    for sim, shrink in bad:
        rc, *got = raw_sim(w.m, sessions, k, sim, shrink, out=sentinel())
        assert rc == -1, (sim, shrink)
        assert same_bytes(got, sentinel()), (sim, shrink)                 # the outputs as they were
        rc = w.m._lib.smatrix_cf_recommend_sim_dev(w.m._h, n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, sim, shrink, k,
                                                   d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == -1, (sim, shrink)
        assert (d_ids.cpu().numpy() == 0xabcdef).all() and (d_sc.cpu().numpy() == -7.5).all() and (d_cnt.cpu().numpy() == 99).all()
    for kk in (0, 65):                                                    # the filtered call's refusals
        assert raw_sim(w.m, sessions, kk, H.SIM_LIFT, 1.0, out=sentinel())[0] == -1
    rc, *got = raw_sim(w.m, sessions, k, H.SIM_LIFT, -0.0)                # -0.0 acts as 0.0
    assert rc == 0 and same_bytes(got, w.m.cf_recommend_filtered(sessions, k, sim="lift"))
    compare(w, got, sessions, k, "lift", 0.0)
    # the truncation: -1, the counts and dst untouched
    src = SparseMatrix()
    src.apply_batch(SET, np.array([1, 1, 1, 2], np.uint32), np.array([0, 2, 3, 0], np.uint32), np.array([9, 2, 3, 4], np.uint32), results=False)
    dst = src.truncated(1, rank="lift")
    before = dst.export("table")
    nn, dd = C.c_uint64(77), C.c_uint64(78)
    call = dst._lib.smatrix_merge_topk_sim
    for sim, shrink in bad:
        assert call(dst._h, src._h, SET, sim, shrink, 5, 1, 0, C.byref(nn), C.byref(dd)) == -1, (sim, shrink)
    for sim, shrink in ((H.SIM_COSINE, 0.0), (H.SIM_JACCARD, 1.0)):
        assert call(dst._h, src._h, SET, sim, shrink, 0, 1, 0, C.byref(nn), C.byref(dd)) == -1      # m == 0
        assert call(dst._h, dst._h, SET, sim, shrink, 5, 1, 0, C.byref(nn), C.byref(dd)) == -1      # dst is src
        assert call(dst._h, src._h, 0, sim, shrink, 5, 1, 0, C.byref(nn), C.byref(dd)) == -1        # get is no merge op
    assert (nn.value, dd.value) == (77, 78)
    assert same_bytes(dst.export("table"), before)
    by = dst._lib.smatrix_merge_topk_by                                   # merge_topk_by still knows its two ranks and no other
    assert by(dst._h, src._h, SET, 2, 5, 1, 0, C.byref(nn), C.byref(dd)) == -1 and (nn.value, dd.value) == (77, 78)
    assert call(dst._h, src._h, SET, H.SIM_JACCARD, 1.0, 5, 1, 0, None, None) == 0                  # (both counts may be NULL)
    assert same_bytes(dst.export("sorted"), src.export("sorted"))
    src.close(); dst.close()
