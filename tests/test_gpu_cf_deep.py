"""GPU (-m gpu): the deep call (include/smatrix_batch.h smatrix_cf_recommend_deep / _dev; SparseMatrix.cf_recommend_deep,
cf_recommend_deep_dev): up to DEEP_MAX = 1024 ranked results per session.

Expected results: tests/cf_deep_helpers.py deep() -- cf_sim_helpers.SessionModel.ranking over the matrix's own export("sorted"), cut
at k.  Ids and counts must be equal and the scores' BYTES must match.  The matrix is the world of tests/test_gpu_cf_sim.py, built as
tests/test_gpu_cf_rank.py builds it; tests/test_cf_deep_model.py shows, without a GPU, that its sessions hold the hard cases: equal
scores across every cut, in both tiers.  Every call takes cf_sim_helpers.all_sessions(): both tiers in one call."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import DEEP_MAX, SparseMatrix, _lib
from tests import cf_deep_helpers as D
from tests import cf_group_helpers as G
from tests import cf_sim_helpers as H
from tests.test_gpu_cf_rank import bitmap, build_world
from tests.test_gpu_cf_sim import LDS_SLOTS, World, flat, need, same_bytes

pytestmark = pytest.mark.gpu

SET = 1
DP = C.POINTER(C.c_double)
p32, p64, pd = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p)), (lambda a: a.ctypes.data_as(DP))
JUNK_ID, JUNK_SCORE = 0x7a7a7a7a, -7.5


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


@pytest.fixture(scope="module")
def world():
    w = World()
    w.m = build_world()
    w.export = w.m.export("sorted")
    for got, want in zip(w.export, H.sorted_export_of(H.world_contents())):
        assert got.tobytes() == want.tobytes()                            # the matrix holds what the model test looked at
    w.model = H.SessionModel(w.export)
    w.rankings = {}                                                       # (sim, shrink, session) -> the unfiltered ranking, made once
    yield w
    w.m.close()


def ranking(w, sess, sim, shrink, wts=None, excl=(), deny=()):
    if wts is not None or excl or deny:
        return w.model.ranking(sess, H.SIMS[sim], shrink, wts, excl, deny)
    key = (sim, shrink, tuple(sess))
    if key not in w.rankings:
        w.rankings[key] = w.model.ranking(sess, H.SIMS[sim], shrink)
    return w.rankings[key]


def compare(model_ranking, got, sessions, k, zero_filled=True, tag=""):
    """got against model_ranking(s, session)[:k]: counts, ids, the scores as uint64 bit patterns, and the unused entries"""
    ids, sc, cnt = got
    assert ids.dtype == np.uint32 and sc.dtype == np.float64 and cnt.dtype == np.uint32 and ids.shape == sc.shape == (len(sessions), k)
    for s, sess in enumerate(sessions):
        best = model_ranking(s, sess)[:k]
        c = int(cnt[s])
        assert c == len(best), (tag, s, c, len(best))
        assert ids[s, :c].tolist() == [b for b, _ in best], (tag, s)
        assert sc[s, :c].view(np.uint64).tolist() == np.array([v for _, v in best], np.float64).view(np.uint64).tolist(), (tag, s)
        if zero_filled:
            assert not ids[s, c:].any() and sc[s, c:].tobytes() == bytes(8 * (k - c)), (tag, s)
        else:                                                             # _dev leaves what it does not own
            assert (ids[s, c:] == JUNK_ID).all() and (sc[s, c:] == JUNK_SCORE).all(), (tag, s)


def on_device(m, method, sessions, k, sim, shrink, weights=None, exclude=None, deny=None, own_stream=True):
    """SparseMatrix.cf_recommend_deep_dev or cf_recommend_sim_dev on torch tensors, on a stream of its own or on the NULL stream; the
    outputs start as junk"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    off, items = flat(sessions, np.uint32)
    n = len(sessions)
    st = torch.cuda.Stream(device=dev) if own_stream else torch.cuda.default_stream(dev)
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)             # noqa: E731
        d_off, d_items = up(off, np.int64), up(items, np.int32)
        d_w = d_exoff = d_ex = d_bits = None
        deny_n = 0
        if weights is not None:
            d_w = torch.from_numpy(flat(weights, np.float64)[1]).to(dev)
        if exclude is not None:
            ex_off, ex = flat(exclude, np.uint32)
            d_exoff, d_ex = up(ex_off, np.int64), up(ex, np.int32)
        if deny is not None:
            bits, deny_n = bitmap(deny)
            d_bits = up(bits, np.int32)
        d_ids = torch.full((n, k), JUNK_ID, dtype=torch.int32, device=dev)
        d_sc = torch.full((n, k), JUNK_SCORE, dtype=torch.float64, device=dev)
        d_cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()               # noqa: E731
        if not own_stream:
            torch.cuda.synchronize()
        getattr(m, method)(n, d_off.data_ptr(), d_items.data_ptr(), ptr(d_w), ptr(d_exoff), ptr(d_ex), ptr(d_bits), deny_n, sim, shrink, k,
                           d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), stream=st if own_stream else None)
    st.synchronize()
    return d_ids.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)


def test_the_sessions_reach_both_tiers(world):
    w = world
    assert max(need(w.m, s) for s in H.lds_sessions()) <= LDS_SLOTS
    assert all(need(w.m, s) > LDS_SLOTS for s in H.global_sessions())
    assert D.LDS_SESSION in H.lds_sessions() and D.EXACT_64 in H.lds_sessions()
    assert all(list(s) in H.global_sessions() for s in D.GLOBAL_SESSIONS)


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", D.KS)
@pytest.mark.parametrize("sim,shrink", D.MEASURES)
def test_both_flavours_are_the_models_bytes(world, sim, shrink, k):
    w = world
    sessions = H.all_sessions()
    model = lambda s, sess: ranking(w, sess, sim, shrink)                 # noqa: E731
    got = w.m.cf_recommend_deep(sessions, k, sim=sim, shrink=shrink)
    compare(model, got, sessions, k, tag=("host", sim, k))
    dev = on_device(w.m, "cf_recommend_deep_dev", sessions, k, sim, shrink)
    compare(model, dev, sessions, k, zero_filled=False, tag=("dev", sim, k))
    assert got[2].tobytes() == dev[2].tobytes() and int(got[2].max()) == k and int(got[2].min()) == 0


def test_unused_entries_the_host_flavour_zero_fills_and_dev_leaves(world):
    """the 64-candidate session at k = 65 and the sessions without a candidate"""
    w = world
    sessions = H.all_sessions()
    i = sessions.index(D.EXACT_64)
    empty = [s for s, sess in enumerate(sessions) if not ranking(w, sess, "cosine", 0.0)]
    assert len(empty) >= 3 and sessions.index([]) in empty
    ids, sc, cnt = w.m.cf_recommend_deep(sessions, 65)
    assert int(cnt[i]) == 64 and ids[i, 63] != 0 and ids[i, 64] == 0 and sc[i, 64].tobytes() == bytes(8)
    assert not cnt[empty].any() and not ids[empty].any() and sc[empty].tobytes() == bytes(8 * 65 * len(empty))
    ids, sc, cnt = on_device(w.m, "cf_recommend_deep_dev", sessions, 65, "cosine", 0.0)
    assert int(cnt[i]) == 64 and ids[i, 63] != JUNK_ID and ids[i, 64] == JUNK_ID and sc[i, 64] == JUNK_SCORE
    assert not cnt[empty].any() and (ids[empty] == JUNK_ID).all() and (sc[empty] == JUNK_SCORE).all()


# ---- prefix and identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink", D.MEASURES)
def test_the_first_64_entries_are_the_sim_calls_and_up_to_64_the_call_is_the_sim_call(world, sim, shrink):
    w = world
    sessions = H.all_sessions()
    deep = on_device(w.m, "cf_recommend_deep_dev", sessions, DEEP_MAX, sim, shrink)
    sim64 = on_device(w.m, "cf_recommend_sim_dev", sessions, 64, sim, shrink)
    assert deep[0][:, :64].tobytes() == sim64[0].tobytes() and deep[1][:, :64].tobytes() == sim64[1].tobytes()   # (junk beyond the counts in both)
    assert np.minimum(deep[2], 64).tobytes() == sim64[2].tobytes()
    for k in (1, 10, 64):
        assert same_bytes(on_device(w.m, "cf_recommend_deep_dev", sessions, k, sim, shrink), on_device(w.m, "cf_recommend_sim_dev", sessions, k, sim, shrink)), k
        assert same_bytes(w.m.cf_recommend_deep(sessions, k, sim=sim, shrink=shrink), w.m.cf_recommend_filtered(sessions, k, sim=sim, shrink=shrink)), k


# ---- the rank call ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink", D.MEASURES)
def test_the_rank_call_answers_every_returned_id_with_its_place(world, sim, shrink):
    w = world
    sessions = H.all_sessions()
    ids, sc, cnt = w.m.cf_recommend_deep(sessions, DEEP_MAX, sim=sim, shrink=shrink)
    targets = [ids[s, :int(cnt[s])].tolist() for s in range(len(sessions))]
    ranks, scores, ncand = w.m.cf_rank(sessions, targets, sim=sim, shrink=shrink)
    assert ranks.tolist() == [r for s in range(len(sessions)) for r in range(int(cnt[s]))]
    assert scores.tobytes() == np.concatenate([sc[s, :int(cnt[s])] for s in range(len(sessions))]).tobytes()
    assert np.minimum(ncand, DEEP_MAX).tobytes() == cnt.tobytes() and int(ncand.max()) > 5000


# ---- filters ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink", [("cosine", 0.0), ("lift", 0.5)])
def test_weights_exclusion_lists_and_the_deny_bitmap(world, sim, shrink):
    w = world
    rng = np.random.default_rng(7)
    sessions = H.all_sessions()
    k = 128
    weights = [(0.25 + rng.random(len(s)) * 4).tolist() for s in sessions]
    weights[sessions.index([303, H.HOT, H.HOT, 0, H.ABSENT, 303])] = [0.5, 3.0, 0.0, 0.25, 1.0, 7.0]      # the first position's weight counts
    weights[sessions.index([H.HOT, 301, 302])] = [1.0, 0.0, 2.0]          # a zero weight: 301's candidates stay, with terms of 0.0
    i = sessions.index(D.LDS_SESSION)
    r = ranking(w, D.LDS_SESSION, sim, shrink, weights[i])
    assert len(r) == 217
    exclude = [[0, 305] for _ in sessions]
    exclude[i] = [r[0][0], r[64][0], r[100][0]]                           # places 0, 64 and 100 of the 217-candidate session
    hot = ranking(w, [H.HOT], sim, shrink, weights[sessions.index([H.HOT])])
    deny = [b for b, _ in hot[63:71]]                                     # places 63 .. 70 of [13]'s ranking
    model = lambda s, sess: ranking(w, sess, sim, shrink, weights[s], exclude[s], deny)   # noqa: E731
    got = w.m.cf_recommend_deep(sessions, k, weights=weights, exclude=exclude, deny=deny, sim=sim, shrink=shrink)
    compare(model, got, sessions, k, tag=("host", sim))
    assert int(got[2][i]) == k and not set(exclude[i]) & set(got[0][i].tolist())
    j = sessions.index([H.HOT])
    assert got[0][j, :63].tolist() == [b for b, _ in hot[:63]] and got[0][j, 63:k].tolist() == [b for b, _ in hot[71:k + 8]]
    dev = on_device(w.m, "cf_recommend_deep_dev", sessions, k, sim, shrink, weights=weights, exclude=exclude, deny=deny)
    compare(model, dev, sessions, k, zero_filled=False, tag=("dev", sim))


# ---- an LDS-tier session with more than DEEP_MAX candidates -----------------------------------------------------------------------
def test_an_lds_tier_session_with_more_candidates_than_deep_max():
    m = SparseMatrix()
    m.apply_batch(SET, *D.small_ops(), results=False)
    slots = sum(m.row_slots(x).shape[0] for x in D.SMALL_ROWS)
    assert slots == 3 * 1024 and slots + len(D.SMALL_SESSION) <= LDS_SLOTS    # k_rec_bound's sum: the LDS tier
    export = m.export("sorted")
    for got, want in zip(export, H.sorted_export_of(D.small_ops())):
        assert got.tobytes() == want.tobytes()
    model = H.SessionModel(export)
    sessions = [D.SMALL_SESSION, [2], []]
    for sim, shrink in D.MEASURES:
        r = model.ranking(D.SMALL_SESSION, H.SIMS[sim], shrink)
        assert len(r) == 1350 and D.ties_across(r, DEEP_MAX)
        by_model = lambda s, sess: model.ranking(sess, H.SIMS[sim], shrink)   # noqa: E731
        got = m.cf_recommend_deep(sessions, DEEP_MAX, sim=sim, shrink=shrink)
        compare(by_model, got, sessions, DEEP_MAX, tag=("small", sim))
        assert got[2].tolist() == [DEEP_MAX, 450, 0]
        dev = on_device(m, "cf_recommend_deep_dev", sessions, DEEP_MAX, sim, shrink)
        compare(by_model, dev, sessions, DEEP_MAX, zero_filled=False, tag=("small, dev", sim))
    with pytest.raises(ValueError):
        m.cf_recommend_deep(sessions, DEEP_MAX + 1)
    off, items = flat(sessions, np.uint32)
    k = DEEP_MAX + 1
    out = (np.full((3, k), 0xabcdef, np.uint32), np.full((3, k), -7.5), np.full(3, 99, np.uint32))
    assert m._lib.smatrix_cf_recommend_deep(m._h, 3, p64(off), p32(items), None, None, None, None, 0, 0, 0.0, k, p32(out[0]), pd(out[1]), p32(out[2])) == -1
    assert (out[0] == 0xabcdef).all() and (out[1] == -7.5).all() and (out[2] == 99).all()
    m.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_each_refusal_leaves_the_outputs_as_they_were(world):
    import torch
    w = world
    lib, h = w.m._lib, w.m._h
    sessions = [[300, 301, 302], [H.HOT, 303], []]
    n, K = len(sessions), 100
    off, items = flat(sessions, np.uint32)
    room = DEEP_MAX + 1                                                   # the outputs hold n * (DEEP_MAX + 1) entries: a refusal is not relied on
    sentinel = lambda: (np.full((n, room), 0xabcdef, np.uint32), np.full((n, room), -7.5), np.full(n, 99, np.uint32))   # noqa: E731
    untouched = lambda got: all(a.tobytes() == b.tobytes() for a, b in zip(got, sentinel()))                         # noqa: E731

    def host(sim=0, shrink=0.0, k=K, deny_n=0, weights=None, ex_off=None, call=lib.smatrix_cf_recommend_deep):
        out = sentinel()
        rc = call(h, n, p64(off), p32(items), None if weights is None else pd(weights), ex_off, None, None, deny_n, sim, shrink, k, p32(out[0]),
                  pd(out[1]), p32(out[2]))
        return rc, out

    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)                 # noqa: E731
    d_off, d_items = up(off, np.int64), up(items, np.int32)
    d_out = [torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else a.dtype)).to(dev) for a in sentinel()]

    def on_dev(sim=0, shrink=0.0, k=K, deny_n=0, ex_off=None, call=lib.smatrix_cf_recommend_deep_dev):
        rc = call(h, n, d_off.data_ptr(), d_items.data_ptr(), None, ex_off, None, None, deny_n, sim, shrink, k, d_out[0].data_ptr(),
                  d_out[1].data_ptr(), d_out[2].data_ptr(), None)
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy().view(np.uint32 if t.dtype == torch.int32 else np.float64) for t in d_out]

    bad = [dict(k=0), dict(k=DEEP_MAX + 1), dict(k=0xFFFFFFFF), dict(sim=3), dict(sim=-1), dict(shrink=-1.0), dict(shrink=float("nan")),
           dict(shrink=float("inf")), dict(deny_n=5), dict(ex_off=p64(off))]
    for case in bad:
        for call in (host, on_dev):
            kw = dict(case)
            if call is on_dev and "ex_off" in kw:
                kw["ex_off"] = d_off.data_ptr()
            rc, got = call(**kw)
            assert rc == -1 and untouched(got), (call.__name__, case)
    for wbad in (-1.0, float("nan"), float("inf")):                       # a bad weight, the host flavour: before the device is touched
        weights = np.ones(items.size)
        weights[2] = wbad
        rc, got = host(weights=weights)
        assert rc == -1 and untouched(got), wbad
    for kw in (dict(call=lib.smatrix_cf_recommend_sim), dict(call=lib.smatrix_cf_recommend_sim, sim=2, shrink=0.5)):   # the existing calls are untouched
        rc, got = host(k=65, **kw)
        assert rc == -1 and untouched(got)
    rc, got = on_dev(k=65, call=lib.smatrix_cf_recommend_sim_dev)
    assert rc == -1 and untouched(got)
    with pytest.raises(ValueError):
        w.m.cf_recommend_sim_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, 65, d_out[0].data_ptr(),
                                 d_out[1].data_ptr(), d_out[2].data_ptr())
    for k in (0, DEEP_MAX + 1):
        with pytest.raises(ValueError):
            w.m.cf_recommend_deep(sessions, k)
    assert lib.smatrix_cf_recommend_deep(h, 0, None, None, None, None, None, None, 0, 0, 0.0, K, None, None, None) == 0
    out = (np.full((n, K), 0xabcdef, np.uint32), np.full((n, K), -7.5), np.full(n, 99, np.uint32))   # ... and the good call behind the refusals
    rc = lib.smatrix_cf_recommend_deep(h, n, p64(off), p32(items), None, None, None, None, 0, 0, 0.0, K, p32(out[0]), pd(out[1]), p32(out[2]))
    assert rc == 0 and same_bytes(out, w.m.cf_recommend_deep(sessions, K))
    compare(lambda s, sess: ranking(w, sess, "cosine", 0.0), out, sessions, K, tag="behind the refusals")
    assert out[2].tolist() == [46, K, 0]                                  # (a session of 46 candidates, one of thousands, an empty one)


# ---- determinism and scratch --------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_and_a_deep_call_between_a_rank_call_and_a_grouped_call(world):
    w = world
    sessions = H.all_sessions()
    c = G.case("a")
    kw = dict(sim="lift", shrink=0.5)
    first = w.m.cf_recommend_filtered(sessions, 64, **kw)
    targets = [first[0][s, :int(first[2][s])][::7].tolist() + [50001, 0] for s in range(len(sessions))]
    rank_alone = w.m.cf_rank(sessions, targets, **kw)
    grouped_alone = w.m.cf_recommend_grouped(sessions, c["k"], c["group_of"], c["cap"], **kw)
    a = w.m.cf_recommend_deep(sessions, 1000, **kw)
    assert same_bytes(a, w.m.cf_recommend_deep(sessions, 1000, **kw))
    d1 = on_device(w.m, "cf_recommend_deep_dev", sessions, 1000, "lift", 0.5)
    d2 = on_device(w.m, "cf_recommend_deep_dev", sessions, 1000, "lift", 0.5, own_stream=False)
    assert same_bytes(d1, d2) and d1[2].tobytes() == a[2].tobytes()
    rank = w.m.cf_rank(sessions, targets, **kw)
    deep = w.m.cf_recommend_deep(sessions, 1000, **kw)
    grouped = w.m.cf_recommend_grouped(sessions, c["k"], c["group_of"], c["cap"], **kw)
    assert same_bytes(rank, rank_alone) and same_bytes(deep, a) and same_bytes(grouped, grouped_alone)
    plain = w.m.cf_recommend_filtered(sessions, 64, **kw)                 # ... and the top-k ending behind the deep one (lk / li)
    assert plain[0].tobytes() == a[0][:, :64].tobytes() and plain[1].tobytes() == a[1][:, :64].tobytes()
