"""GPU (-m gpu): the fill call (include/smatrix_batch.h smatrix_cf_recommend_fill / _dev; SparseMatrix.cf_recommend_filled,
cf_recommend_fill_dev).

Expected results: tests/cf_fill_helpers.py filled() -- cf_sim_helpers.SessionModel.session over the matrix's own export("sorted"), then
the free places from the list in list order.  Ids, counts and n_scored must be equal and the scores' BYTES must match.  The matrix is
the world of tests/test_gpu_cf_sim.py, built as tests/test_gpu_cf_rank.py builds it; tests/test_cf_fill_model.py shows, without a GPU,
that the sessions and the list hold the hard cases."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix, _lib
from tests import cf_fill_helpers as F
from tests import cf_sim_helpers as H
from tests.test_gpu_cf_rank import MEASURES, bitmap, build_world
from tests.test_gpu_cf_sim import LDS_SLOTS, World, flat, need, same_bytes

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
p32, p64, pd = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p)), (lambda a: a.ctypes.data_as(DP))
K = 10


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
    w.list = F.fill_list()
    yield w
    w.m.close()


def sessions_and_lists():
    """the world's sessions of both tiers with the sessions that need filling among them -> (sessions, exclusion lists)"""
    q = [(s, []) for s in H.all_sessions()]
    for i, se in enumerate(F.FILL_SESSIONS):
        q.insert(2 + 6 * i, se)
    return [s for s, _ in q], [e for _, e in q]


def compare(w, got, sessions, k, sim, shrink, fill, weights=None, exclude=None, deny=(), tag="", zero_filled=True):
    ids, sc, cnt, nsc = got
    assert ids.dtype == np.uint32 and sc.dtype == np.float64 and cnt.dtype == np.uint32 and nsc.dtype == np.uint32
    for s, sess in enumerate(sessions):
        wi, ws, wn = F.filled(w.model, sess, k, H.SIMS[sim], shrink, fill, None if weights is None else weights[s],
                              () if exclude is None else exclude[s], deny)
        assert (int(nsc[s]), int(cnt[s])) == (wn, len(wi)), (tag, s, int(nsc[s]), int(cnt[s]), wn, len(wi))
        assert ids[s, :len(wi)].tolist() == wi, (tag, s)
        assert sc[s, :len(wi)].tobytes() == ws.tobytes(), (tag, s)
        if zero_filled:
            assert not ids[s, len(wi):].any() and sc[s, len(wi):].tobytes() == bytes(8 * (k - len(wi))), (tag, s)


def fill_dev(m, sessions, k, fill, sim, shrink, weights=None, exclude=None, deny=None):
    """SparseMatrix.cf_recommend_fill_dev on torch tensors, on a stream of its own; the outputs start as junk"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    off, items = flat(sessions, np.uint32)
    n = len(sessions)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)             # noqa: E731
        d_off, d_items = up(off, np.int64), up(items, np.int32)
        d_w = d_exoff = d_ex = d_bits = d_fill = None
        deny_n = 0
        if weights is not None:
            d_w = torch.from_numpy(flat(weights, np.float64)[1]).to(dev)
        if exclude is not None:
            ex_off, ex = flat(exclude, np.uint32)
            d_exoff, d_ex = up(ex_off, np.int64), up(ex, np.int32)
        if deny is not None:
            bits, deny_n = bitmap(deny)
            d_bits = up(bits, np.int32)
        if len(fill):
            d_fill = up(np.asarray(fill, np.uint32), np.int32)
        d_ids = torch.full((n, k), 0x7a7a7a7a, dtype=torch.int32, device=dev)
        d_sc = torch.full((n, k), -7.5, dtype=torch.float64, device=dev)
        d_cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
        d_nsc = torch.full((n,), 98, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()               # noqa: E731
        m.cf_recommend_fill_dev(n, d_off.data_ptr(), d_items.data_ptr(), ptr(d_w), ptr(d_exoff), ptr(d_ex), ptr(d_bits), deny_n, ptr(d_fill),
                                len(fill), sim, shrink, k, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), d_nsc.data_ptr(), stream=st)
    st.synchronize()
    return d_ids.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32), d_nsc.cpu().numpy().view(np.uint32)


def test_the_sessions_reach_both_tiers_and_the_fill_sessions_are_short(world):
    w = world
    assert max(need(w.m, s) for s in H.lds_sessions()) <= LDS_SLOTS
    assert all(need(w.m, s) > LDS_SLOTS for s in H.global_sessions() + [[H.HOT]])
    assert need(w.m, F.ROWLESS, len(F.LONG_EXCL)) <= LDS_SLOTS


@pytest.mark.parametrize("n_fill", F.FILL_LENGTHS)
def test_full_sessions_are_the_sim_calls_bytes_and_short_ones_are_filled_in_list_order(world, n_fill):
    w = world
    sessions, exclude = sessions_and_lists()
    fill = w.list[:n_fill]
    for k in (K, 64):
        got = w.m.cf_recommend_filled(sessions, k, fill, exclude=exclude, deny=F.DENY)
        compare(w, got, sessions, k, "cosine", 0.0, fill, exclude=exclude, deny=F.DENY, tag=("host", n_fill, k))
        ids, sc, cnt, nsc = got
        plain = w.m.cf_recommend_filtered(sessions, k, exclude=exclude, deny=F.DENY)
        assert nsc.tobytes() == plain[2].tobytes()
        full = nsc == k
        assert full.sum() >= 5 and (~full).sum() >= len(F.FILL_SESSIONS)
        assert ids[full].tobytes() == plain[0][full].tobytes() and sc[full].tobytes() == plain[1][full].tobytes()
        for s in np.flatnonzero(~full):                                   # the scored part of a short result is the sim call's, too
            assert ids[s, :nsc[s]].tobytes() == plain[0][s, :nsc[s]].tobytes() and sc[s, :nsc[s]].tobytes() == plain[1][s, :nsc[s]].tobytes()
        if n_fill == 1:
            assert cnt.tobytes() == nsc.tobytes()                         # the list [0]: too short for anyone
        if n_fill == 200:
            assert (cnt == k).all()
        dev = fill_dev(w.m, sessions, k, fill, "cosine", 0.0, exclude=exclude, deny=F.DENY)
        compare(w, dev, sessions, k, "cosine", 0.0, fill, exclude=exclude, deny=F.DENY, tag=("dev", n_fill, k), zero_filled=False)
        for s in range(len(sessions)):                                    # _dev leaves what it does not own
            assert (dev[0][s, cnt[s]:] == 0x7a7a7a7a).all() and (dev[1][s, cnt[s]:] == -7.5).all()


def test_an_empty_list_gives_the_sim_calls_bytes(world):
    w = world
    sessions, exclude = sessions_and_lists()
    plain = w.m.cf_recommend_filtered(sessions, K, exclude=exclude, deny=F.DENY, sim="lift", shrink=0.5)
    for fill in ([], np.zeros(0, np.uint32)):
        got = w.m.cf_recommend_filled(sessions, K, fill, exclude=exclude, deny=F.DENY, sim="lift", shrink=0.5)
        assert same_bytes(got[:3], plain) and got[3].tobytes() == plain[2].tobytes()
    dev = fill_dev(w.m, sessions, K, [], "lift", 0.5, exclude=exclude, deny=F.DENY)
    assert dev[2].tobytes() == plain[2].tobytes() == dev[3].tobytes()
    for s in range(len(sessions)):
        c = int(plain[2][s])
        assert dev[0][s, :c].tobytes() == plain[0][s, :c].tobytes() and dev[1][s, :c].tobytes() == plain[1][s, :c].tobytes()


@pytest.mark.parametrize("sim,shrink", MEASURES)
def test_every_measure_with_weights(world, sim, shrink):
    w = world
    rng = np.random.default_rng(12)
    sessions, exclude = sessions_and_lists()
    weights = [(rng.random(len(s)) * 4).tolist() for s in sessions]
    for s in weights:
        if len(s) > 1:
            s[1] = 0.0                                                    # an item of weight 0 is still an item: never filled in
    kw = dict(weights=weights, exclude=exclude, deny=F.DENY)
    got = w.m.cf_recommend_filled(sessions, K, w.list, sim=sim, shrink=shrink, **kw)
    compare(w, got, sessions, K, sim, shrink, w.list, tag=("host", sim, shrink), **kw)
    dev = fill_dev(w.m, sessions, K, w.list, sim, shrink, **kw)
    compare(w, dev, sessions, K, sim, shrink, w.list, tag=("dev", sim, shrink), zero_filled=False, **kw)
    assert (got[2] == K).all() and (got[3] < K).sum() >= len(F.FILL_SESSIONS)


def test_a_global_tier_session_denied_down_to_fewer_than_k(world):
    w = world
    deny = F.heavy_deny()
    sessions = [[H.HOT], [H.HOT, 301, 302], [300, 301], []]
    for fill in (w.list, w.list[:3], sorted(F.row_columns(H.HOT))[990:1010] + w.list):
        got = w.m.cf_recommend_filled(sessions, K, fill, deny=deny)
        compare(w, got, sessions, K, "cosine", 0.0, fill, deny=deny, tag="heavy deny")
        assert got[3][0] == 3 and got[3][1] == K and got[3][3] == 0
        dev = fill_dev(w.m, sessions, K, fill, "cosine", 0.0, deny=deny)
        compare(w, dev, sessions, K, "cosine", 0.0, fill, deny=deny, tag="heavy deny, dev", zero_filled=False)
    assert got[2][0] == K and F.FRESH[5] not in got[0][0].tolist()          # a denied id of the list is never filled in


def test_popular_items_fill_end_to_end(world):
    w = world
    sessions, exclude = sessions_and_lists()
    pop_ids, pop_tot = w.m.cf_popular(1024, deny=F.DENY)
    want = F.popular(w.export, 1024, deny=F.DENY)
    assert pop_ids.tolist() == want[0].tolist() and pop_tot.tolist() == want[1].tolist() and 300 < pop_ids.size < 1024
    got = w.m.cf_recommend_filled(sessions, K, pop_ids, exclude=exclude, deny=F.DENY, sim="jaccard", shrink=10.0)
    compare(w, got, sessions, K, "jaccard", 10.0, want[0].tolist(), exclude=exclude, deny=F.DENY, tag="popular")
    assert (got[2] == K).all()
    empty = sessions.index([])
    assert got[0][empty].tolist() == pop_ids[:K].tolist() and not got[1][empty].any()


def test_each_refusal_leaves_the_outputs_as_they_were(world):
    import torch
    w = world
    lib, h = w.m._lib, w.m._h
    sessions = [[300, 301, 302], [H.HOT, 303], []]
    n = len(sessions)
    off, items = flat(sessions, np.uint32)
    fill = np.asarray(w.list, np.uint32)
    sentinel = lambda: (np.full((n, K), 0xabcdef, np.uint32), np.full((n, K), -7.5), np.full(n, 99, np.uint32), np.full(n, 98, np.uint32))   # noqa: E731
    untouched = lambda got: all(a.tobytes() == b.tobytes() for a, b in zip(got, sentinel()))                   # noqa: E731

    def host(sim=0, shrink=0.0, k=K, fill_ptr=True, n_fill=fill.size, nsc=True, deny_n=0, weights=None, ex_off=None):
        out = sentinel()
        rc = lib.smatrix_cf_recommend_fill(h, n, p64(off), p32(items), None if weights is None else pd(weights), ex_off, None, None, deny_n,
                                           p32(fill) if fill_ptr else None, n_fill, sim, shrink, k, p32(out[0]), pd(out[1]), p32(out[2]),
                                           p32(out[3]) if nsc else None)
        return rc, out

    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)                 # noqa: E731
    d_off, d_items, d_fill = up(off, np.int64), up(items, np.int32), up(fill, np.int32)
    d_out = [torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else a.dtype)).to(dev) for a in sentinel()]

    def on_device(sim=0, shrink=0.0, k=K, fill_ptr=True, n_fill=fill.size, nsc=True, deny_n=0, ex_off=None):
        rc = lib.smatrix_cf_recommend_fill_dev(h, n, d_off.data_ptr(), d_items.data_ptr(), None, ex_off, None, None, deny_n,
                                               d_fill.data_ptr() if fill_ptr else None, n_fill, sim, shrink, k, d_out[0].data_ptr(),
                                               d_out[1].data_ptr(), d_out[2].data_ptr(), d_out[3].data_ptr() if nsc else None, None)
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy().view(np.uint32 if t.dtype == torch.int32 else np.float64) for t in d_out]

    bad = [dict(nsc=False), dict(fill_ptr=False), dict(n_fill=1 << 32), dict(sim=3), dict(shrink=-1.0), dict(shrink=float("nan")), dict(k=0), dict(k=65),
           dict(deny_n=5), dict(ex_off=p64(off))]
    for case in bad:
        for call in (host, on_device):
            kw = dict(case)
            if call is on_device and "ex_off" in kw:
                kw["ex_off"] = d_off.data_ptr()
            rc, got = call(**kw)
            assert rc == -1 and untouched(got), (call.__name__, case)
    for wbad in (-1.0, float("nan"), float("inf")):                       # a bad weight, the host flavour: before the device is touched
        weights = np.ones(items.size)
        weights[2] = wbad
        rc, got = host(weights=weights)
        assert rc == -1 and untouched(got), wbad
    rc, got = host(fill_ptr=False, n_fill=0)                              # NULL with no ids is the empty list
    plain = w.m.cf_recommend_filtered(sessions, K)
    assert rc == 0 and same_bytes(got[:3], plain) and got[3].tobytes() == plain[2].tobytes()
    assert lib.smatrix_cf_recommend_fill(h, 0, None, None, None, None, None, None, 0, None, 0, 0, 0.0, K, None, None, None, p32(got[3])) == 0
