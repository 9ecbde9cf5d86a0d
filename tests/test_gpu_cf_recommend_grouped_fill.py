"""GPU (-m gpu): the grouped fill call (include/smatrix_batch.h smatrix_cf_recommend_grouped_fill / _dev;
SparseMatrix.cf_recommend_grouped_filled, cf_recommend_grouped_fill_dev).

Expected results: tests/cf_group_fill_helpers.py grouped_filled() -- cf_group_helpers.grouped() over the matrix's own export("sorted"),
then the serial walk of the contract under running per-group counts.  Ids, counts and n_scored must be equal and the scores' BYTES must
match.  The matrix is the world of tests/test_gpu_cf_sim.py, built as tests/test_gpu_cf_rank.py builds it;
tests/test_cf_group_fill_model.py shows, without a GPU, that the map, the list and the sessions hold the hard cases."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import _lib
from tests import cf_fill_helpers as F
from tests import cf_group_fill_helpers as GF
from tests import cf_group_helpers as G
from tests import cf_sim_helpers as H
from tests.test_gpu_cf_rank import bitmap, build_world
from tests.test_gpu_cf_recommend_fill import fill_dev
from tests.test_gpu_cf_recommend_grouped import grouped_dev
from tests.test_gpu_cf_sim import LDS_SLOTS, World, flat, need, same_bytes

pytestmark = pytest.mark.gpu

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
    w.list = GF.fill_list()
    w.map = GF.group_map()                                                # the dict; the model takes the array
    w.arr = GF.group_array()
    yield w
    w.m.close()


def compare(w, got, sessions, k, cap, sim, shrink, fill, weights=None, exclude=None, deny=(), tag="", zero_filled=True, group_of=None):
    ids, sc, cnt, nsc = got
    assert ids.dtype == np.uint32 and sc.dtype == np.float64 and cnt.dtype == np.uint32 and nsc.dtype == np.uint32
    assert ids.shape == sc.shape == (len(sessions), k)
    for s, sess in enumerate(sessions):
        wi, ws, wn = GF.grouped_filled(w.model, sess, k, H.SIMS[sim], shrink, w.arr if group_of is None else group_of, cap, fill,
                                       None if weights is None else weights[s], () if exclude is None else exclude[s], deny)
        assert (int(nsc[s]), int(cnt[s])) == (wn, len(wi)), (tag, s, int(nsc[s]), int(cnt[s]), wn, len(wi))
        assert ids[s, :len(wi)].tolist() == wi, (tag, s)
        assert sc[s, :len(wi)].tobytes() == ws.tobytes(), (tag, s)
        if zero_filled:
            assert not ids[s, len(wi):].any() and sc[s, len(wi):].tobytes() == bytes(8 * (k - len(wi))), (tag, s)
        else:                                                             # _dev leaves what it does not own
            assert (ids[s, len(wi):] == JUNK_ID).all() and (sc[s, len(wi):] == JUNK_SCORE).all(), (tag, s)


def both_dev(m, sessions, k, group_of, cap, fill, sim, shrink, weights=None, exclude=None, deny=None):
    """SparseMatrix.cf_recommend_grouped_fill_dev on torch tensors, on a stream of its own; the outputs start as junk"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    off, items = flat(sessions, np.uint32)
    n = len(sessions)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)             # noqa: E731
        d_off, d_items = up(off, np.int64), up(items, np.int32)
        d_w = d_exoff = d_ex = d_bits = d_grp = d_fill = None
        deny_n = group_n = 0
        if weights is not None:
            d_w = torch.from_numpy(flat(weights, np.float64)[1]).to(dev)
        if exclude is not None:
            ex_off, ex = flat(exclude, np.uint32)
            d_exoff, d_ex = up(ex_off, np.int64), up(ex, np.int32)
        if deny is not None:
            bits, deny_n = bitmap(deny)
            d_bits = up(bits, np.int32)
        arr = G.as_array(group_of)
        if arr is not None:
            d_grp, group_n = up(arr, np.int32), int(arr.size)
        if len(fill):
            d_fill = up(np.asarray(fill, np.uint32), np.int32)
        d_ids = torch.full((n, k), JUNK_ID, dtype=torch.int32, device=dev)
        d_sc = torch.full((n, k), JUNK_SCORE, dtype=torch.float64, device=dev)
        d_cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
        d_nsc = torch.full((n,), 98, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()               # noqa: E731
        m.cf_recommend_grouped_fill_dev(n, d_off.data_ptr(), d_items.data_ptr(), ptr(d_w), ptr(d_exoff), ptr(d_ex), ptr(d_bits), deny_n,
                                        ptr(d_grp), group_n, cap, ptr(d_fill), len(fill), sim, shrink, k, d_ids.data_ptr(), d_sc.data_ptr(),
                                        d_cnt.data_ptr(), d_nsc.data_ptr(), stream=st)
    st.synchronize()
    return d_ids.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32), d_nsc.cpu().numpy().view(np.uint32)


def test_the_sessions_reach_both_tiers_and_the_warm_session_is_cut_short(world):
    w = world
    assert max(need(w.m, s) for s in H.lds_sessions()) <= LDS_SLOTS and G.LDS_SESSION in H.lds_sessions()
    assert all(need(w.m, s) > LDS_SLOTS for s in H.global_sessions() + [[H.HOT]])
    assert need(w.m, F.ROWLESS, len(F.LONG_EXCL)) <= LDS_SLOTS
    got = w.m.cf_recommend_grouped([G.LDS_SESSION], 10, w.map, 2, deny=F.DENY)
    assert got[2][0] < 10 and w.m.cf_recommend_filtered([G.LDS_SESSION], 10, deny=F.DENY)[2][0] == 10


@pytest.mark.parametrize("n_fill", F.FILL_LENGTHS)
def test_both_flavours_are_the_models_bytes(world, n_fill):
    w = world
    sessions, exclude = GF.sessions_and_lists()
    fill = w.list[:n_fill]
    kw = dict(exclude=exclude, deny=F.DENY)
    for k, cap in GF.SHAPES:
        got = w.m.cf_recommend_grouped_filled(sessions, k, w.map, cap, fill, **kw)
        compare(w, got, sessions, k, cap, "cosine", 0.0, fill, tag=("host", n_fill, k, cap), **kw)
        ids, sc, cnt, nsc = got
        scored = w.m.cf_recommend_grouped(sessions, k, w.arr, cap, **kw)    # the scored part is the grouped call's, in both tiers
        assert nsc.tobytes() == scored[2].tobytes()
        for s in range(len(sessions)):
            assert ids[s, :nsc[s]].tobytes() == scored[0][s, :nsc[s]].tobytes() and sc[s, :nsc[s]].tobytes() == scored[1][s, :nsc[s]].tobytes()
        full = nsc == k
        assert full.sum() >= 3 and (~full).sum() >= len(F.FILL_SESSIONS) + 1
        assert ids[full].tobytes() == scored[0][full].tobytes() and cnt[full].tobytes() == nsc[full].tobytes()      # untouched by the list
        if n_fill == 1:
            assert cnt.tobytes() == nsc.tobytes()                         # the list [0]: too short for anyone
        if n_fill == 200 and k == 10:
            assert (cnt == k).all()
        dev = both_dev(w.m, sessions, k, w.arr, cap, fill, "cosine", 0.0, **kw)
        compare(w, dev, sessions, k, cap, "cosine", 0.0, fill, tag=("dev", n_fill, k, cap), zero_filled=False, **kw)
        assert same_bytes(dev[2:], got[2:])


def test_k_1(world):
    w = world
    sessions, exclude = GF.sessions_and_lists()
    kw = dict(exclude=exclude, deny=F.DENY)
    got = w.m.cf_recommend_grouped_filled(sessions, 1, w.map, 1, w.list, **kw)      # cap >= k: the fill call
    compare(w, got, sessions, 1, 1, "cosine", 0.0, w.list, tag="k = 1", **kw)
    assert same_bytes(got, w.m.cf_recommend_filled(sessions, 1, w.list, **kw)) and (got[2] == 1).all()
    dev = both_dev(w.m, sessions, 1, w.map, 1, w.list, "cosine", 0.0, **kw)
    assert same_bytes(dev, got)


def test_weights_and_another_measure(world):
    w = world
    rng = np.random.default_rng(12)
    sessions, exclude = GF.sessions_and_lists()
    weights = [(rng.random(len(s)) * 4).tolist() for s in sessions]
    for s in weights:
        if len(s) > 1:
            s[1] = 0.0                                                    # an item of weight 0 is still an item: never filled in
    kw = dict(weights=weights, exclude=exclude, deny=F.DENY)
    got = w.m.cf_recommend_grouped_filled(sessions, 10, w.map, 2, w.list, sim="jaccard", shrink=10.0, **kw)
    compare(w, got, sessions, 10, 2, "jaccard", 10.0, w.list, tag="host, jaccard", **kw)
    dev = both_dev(w.m, sessions, 10, w.map, 2, w.list, "jaccard", 10.0, **kw)
    compare(w, dev, sessions, 10, 2, "jaccard", 10.0, w.list, tag="dev, jaccard", zero_filled=False, **kw)
    assert (got[2] == 10).all() and (got[3] < 10).sum() >= len(F.FILL_SESSIONS) + 1


def test_no_map_and_a_cap_of_k_or_more_are_the_fill_calls_bytes(world):
    w = world
    sessions, exclude = GF.sessions_and_lists()
    kw = dict(exclude=exclude, deny=F.DENY)
    for k in (10, 64):
        want = fill_dev(w.m, sessions, k, w.list, "lift", 0.5, **kw)
        host = w.m.cf_recommend_filled(sessions, k, w.list, sim="lift", shrink=0.5, **kw)
        for group_of, cap in [(None, 1), ({}, 3), (w.map, k), (w.arr, 64)]:
            dev = both_dev(w.m, sessions, k, group_of, cap, w.list, "lift", 0.5, **kw)
            assert same_bytes(dev, want), (k, cap)                        # junk beyond counts included: _dev leaves it
            got = w.m.cf_recommend_grouped_filled(sessions, k, group_of, cap, w.list, sim="lift", shrink=0.5, **kw)
            assert same_bytes(got, host), (k, cap)


def test_an_empty_list_gives_the_grouped_calls_bytes(world):
    w = world
    sessions, exclude = GF.sessions_and_lists()
    kw = dict(exclude=exclude, deny=F.DENY)
    for k, cap in GF.SHAPES:
        want = grouped_dev(w.m, sessions, k, w.arr, cap, "cosine", 0.1, **kw)
        dev = both_dev(w.m, sessions, k, w.arr, cap, [], "cosine", 0.1, **kw)
        assert same_bytes(dev[:3], want) and dev[3].tobytes() == dev[2].tobytes()
        host = w.m.cf_recommend_grouped(sessions, k, w.map, cap, sim="cosine", shrink=0.1, **kw)
        for fill in ([], np.zeros(0, np.uint32)):
            got = w.m.cf_recommend_grouped_filled(sessions, k, w.map, cap, fill, sim="cosine", shrink=0.1, **kw)
            assert same_bytes(got[:3], host) and got[3].tobytes() == host[2].tobytes()


def test_the_global_tier_session_is_filled_under_the_quotas(world):
    w = world
    deny = F.heavy_deny()
    sessions = GF.HOT_SESSIONS
    for k, cap in GF.SHAPES:
        for fill in (w.list, w.list[:3], sorted(F.row_columns(H.HOT))[990:1010] + w.list):
            got = w.m.cf_recommend_grouped_filled(sessions, k, w.map, cap, fill, deny=deny)
            compare(w, got, sessions, k, cap, "cosine", 0.0, fill, deny=deny, tag=("heavy deny", k, cap))
            assert got[3][0] == cap and got[3][3] == 0                    # of the three candidates left, all of group X, cap are scored
            dev = both_dev(w.m, sessions, k, w.arr, cap, fill, "cosine", 0.0, deny=deny)
            compare(w, dev, sessions, k, cap, "cosine", 0.0, fill, deny=deny, tag=("heavy deny, dev", k, cap), zero_filled=False)
        assert not set(GF.hot_left()[cap:]) & set(got[0][0].tolist())     # the candidates the quota refused are offered by the last list
        assert GF.FR[10] not in got[0][0].tolist()                        # ... and X is full from the scored results


def test_the_same_call_twice_gives_the_same_bytes(world):
    w = world
    sessions, exclude = GF.sessions_and_lists()
    kw = dict(exclude=exclude, deny=F.DENY)
    a = w.m.cf_recommend_grouped_filled(sessions, 10, w.map, 1, w.list, **kw)
    b = w.m.cf_recommend_grouped_filled(sessions, 10, w.map, 1, w.list, **kw)
    assert same_bytes(a, b)
    c = both_dev(w.m, sessions, 64, w.arr, 1, w.list, "cosine", 0.0, **kw)
    d = both_dev(w.m, sessions, 64, w.arr, 1, w.list, "cosine", 0.0, **kw)
    assert same_bytes(c, d)


def test_each_refusal_leaves_the_outputs_as_they_were(world):
    import torch
    w = world
    lib, h = w.m._lib, w.m._h
    sessions = [[300, 301, 302], [H.HOT, 303], []]
    n, K = len(sessions), 10
    off, items = flat(sessions, np.uint32)
    grp, fill = w.arr, np.asarray(w.list, np.uint32)
    sentinel = lambda: (np.full((n, K), 0xabcdef, np.uint32), np.full((n, K), -7.5), np.full(n, 99, np.uint32), np.full(n, 98, np.uint32))   # noqa: E731
    untouched = lambda got: all(a.tobytes() == b.tobytes() for a, b in zip(got, sentinel()))                   # noqa: E731

    def host(sim=0, shrink=0.0, k=K, cap=1, grp_ptr=True, group_n=grp.size, fill_ptr=True, n_fill=fill.size, nsc=True, deny_n=0, weights=None,
             ex_off=None):
        out = sentinel()
        rc = lib.smatrix_cf_recommend_grouped_fill(h, n, p64(off), p32(items), None if weights is None else pd(weights), ex_off, None, None, deny_n,
                                                   p32(grp) if grp_ptr else None, group_n, cap, p32(fill) if fill_ptr else None, n_fill, sim,
                                                   shrink, k, p32(out[0]), pd(out[1]), p32(out[2]), p32(out[3]) if nsc else None)
        return rc, out

    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)                 # noqa: E731
    d_off, d_items, d_grp, d_fill = up(off, np.int64), up(items, np.int32), up(grp, np.int32), up(fill, np.int32)
    d_out = [torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else a.dtype)).to(dev) for a in sentinel()]

    def on_device(sim=0, shrink=0.0, k=K, cap=1, grp_ptr=True, group_n=grp.size, fill_ptr=True, n_fill=fill.size, nsc=True, deny_n=0, ex_off=None):
        rc = lib.smatrix_cf_recommend_grouped_fill_dev(h, n, d_off.data_ptr(), d_items.data_ptr(), None, ex_off, None, None, deny_n,
                                                       d_grp.data_ptr() if grp_ptr else None, group_n, cap, d_fill.data_ptr() if fill_ptr else None,
                                                       n_fill, sim, shrink, k, d_out[0].data_ptr(), d_out[1].data_ptr(), d_out[2].data_ptr(),
                                                       d_out[3].data_ptr() if nsc else None, None)
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy().view(np.uint32 if t.dtype == torch.int32 else np.float64) for t in d_out]

    bad = [dict(cap=0), dict(cap=65), dict(cap=0xFFFFFFFF), dict(group_n=(1 << 32) + 1), dict(grp_ptr=False), dict(grp_ptr=False, group_n=1),   # the grouped call's
           dict(nsc=False), dict(fill_ptr=False), dict(n_fill=1 << 32),                                                                       # the fill call's
           dict(sim=3), dict(shrink=-1.0), dict(shrink=float("nan")), dict(k=0), dict(k=65), dict(deny_n=5), dict(ex_off=p64(off))]           # the sim call's
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
    want = w.m.cf_recommend_grouped(sessions, K, grp, 1)
    assert rc == 0 and same_bytes(got[:3], want) and got[3].tobytes() == want[2].tobytes()
    rc, got = host(grp_ptr=False, group_n=0, cap=64)                      # NULL with no ids is no grouping
    assert rc == 0 and same_bytes(got, w.m.cf_recommend_filled(sessions, K, fill))
    rc, got = host()                                                      # ... and the good call behind the refusals
    assert rc == 0 and same_bytes(got, w.m.cf_recommend_grouped_filled(sessions, K, grp, 1, fill)) and (got[2] == K).all()
    assert lib.smatrix_cf_recommend_grouped_fill(h, 0, None, None, None, None, None, None, 0, None, 0, 1, None, 0, 0, 0.0, K, None, None, None,
                                                 p32(got[3])) == 0
    with pytest.raises(ValueError):
        w.m.cf_recommend_grouped_filled(sessions, K, grp, 0, fill)
    with pytest.raises(ValueError):
        w.m.cf_recommend_grouped_filled(sessions, K, grp, 1, None)
