"""GPU (-m gpu): the grouped call (include/smatrix_batch.h smatrix_cf_recommend_grouped / _dev; SparseMatrix.cf_recommend_grouped,
cf_recommend_grouped_dev).

Expected results: tests/cf_group_helpers.py grouped() -- cf_sim_helpers.SessionModel.ranking over the matrix's own export("sorted"),
then the closed form of the contract.  Ids and counts must be equal and the scores' BYTES must match.  The matrix is the world of
tests/test_gpu_cf_sim.py, built as tests/test_gpu_cf_rank.py builds it; tests/test_cf_group_model.py shows, without a GPU, that the
maps hold the hard cases.  Every call takes cf_sim_helpers.all_sessions(): both tiers in one call."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import GROUP_NONE, _lib
from tests import cf_group_helpers as G
from tests import cf_sim_helpers as H
from tests.test_gpu_cf_rank import bitmap, build_world
from tests.test_gpu_cf_sim import LDS_SLOTS, World, flat, need, same_bytes

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
p32, p64, pd = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p)), (lambda a: a.ctypes.data_as(DP))
# one measure per case: all three, shrink 0 and > 0, with weights (odd places) and without
MEASURES = [("cosine", 0.0), ("cosine", 0.1), ("jaccard", 10.0), ("lift", 0.5), ("jaccard", 0.0), ("lift", 0.0), ("cosine", 10.0), ("lift", 0.1)]
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
    yield w
    w.m.close()


def weights_for(sessions):
    rng = np.random.default_rng(12)
    return [(rng.random(len(s)) * 4).tolist() for s in sessions]


def compare(w, got, sessions, c, sim, shrink, weights=None, tag="", zero_filled=True):
    ids, sc, cnt = got
    k = c["k"]
    assert ids.dtype == np.uint32 and sc.dtype == np.float64 and cnt.dtype == np.uint32 and ids.shape == sc.shape == (len(sessions), k)
    for s, sess in enumerate(sessions):
        wi, ws, _ = G.grouped(w.model, sess, k, H.SIMS[sim], shrink, c["group_of"], c["cap"], None if weights is None else weights[s],
                              () if c["exclude"] is None else c["exclude"][s], c["deny"] or ())
        assert int(cnt[s]) == len(wi), (tag, s, int(cnt[s]), len(wi))
        assert ids[s, :len(wi)].tolist() == wi, (tag, s)
        assert sc[s, :len(wi)].tobytes() == ws.tobytes(), (tag, s)
        if zero_filled:
            assert not ids[s, len(wi):].any() and sc[s, len(wi):].tobytes() == bytes(8 * (k - len(wi))), (tag, s)
        else:                                                             # _dev leaves what it does not own
            assert (ids[s, len(wi):] == JUNK_ID).all() and (sc[s, len(wi):] == JUNK_SCORE).all(), (tag, s)


def grouped_dev(m, sessions, k, group_of, cap, sim, shrink, weights=None, exclude=None, deny=None, own_stream=True):
    """SparseMatrix.cf_recommend_grouped_dev on torch tensors, on a stream of its own or on the NULL stream; the outputs start as junk"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    off, items = flat(sessions, np.uint32)
    n = len(sessions)
    st = torch.cuda.Stream(device=dev) if own_stream else torch.cuda.default_stream(dev)
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)             # noqa: E731
        d_off, d_items = up(off, np.int64), up(items, np.int32)
        d_w = d_exoff = d_ex = d_bits = d_grp = None
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
        d_ids = torch.full((n, k), JUNK_ID, dtype=torch.int32, device=dev)
        d_sc = torch.full((n, k), JUNK_SCORE, dtype=torch.float64, device=dev)
        d_cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()               # noqa: E731
        if not own_stream:
            torch.cuda.synchronize()
        m.cf_recommend_grouped_dev(n, d_off.data_ptr(), d_items.data_ptr(), ptr(d_w), ptr(d_exoff), ptr(d_ex), ptr(d_bits), deny_n, ptr(d_grp),
                                   group_n, cap, sim, shrink, k, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(),
                                   stream=st if own_stream else None)
    st.synchronize()
    return d_ids.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)


def test_the_sessions_reach_both_tiers(world):
    w = world
    assert max(need(w.m, s) for s in H.lds_sessions()) <= LDS_SLOTS
    assert all(need(w.m, s) > LDS_SLOTS for s in H.global_sessions())
    assert G.LDS_SESSION in H.lds_sessions() and G.TIE_SESSION in H.lds_sessions() and [H.HOT] in H.global_sessions()


@pytest.mark.parametrize("i", range(8), ids=[c["name"] for c in G.cases()])
def test_both_flavours_are_the_models_bytes(world, i):
    w, c = world, G.cases()[i]
    sim, shrink = MEASURES[i]
    sessions = H.all_sessions()
    weights = weights_for(sessions) if i % 2 else None
    kw = dict(weights=weights, exclude=c["exclude"], deny=c["deny"])
    got = w.m.cf_recommend_grouped(sessions, c["k"], c["group_of"], c["cap"], sim=sim, shrink=shrink, **kw)
    compare(w, got, sessions, c, sim, shrink, weights, tag=("host", c["name"]))
    again = w.m.cf_recommend_grouped(sessions, c["k"], c["group_of"], c["cap"], sim=sim, shrink=shrink, **kw)
    assert same_bytes(got, again)                                         # the same input twice gives the same bytes
    dev = grouped_dev(w.m, sessions, c["k"], c["group_of"], c["cap"], sim, shrink, **kw)
    compare(w, dev, sessions, c, sim, shrink, weights, tag=("dev", c["name"]), zero_filled=False)


@pytest.mark.parametrize("sim,shrink", [("cosine", 0.0), ("lift", 0.5)])
def test_no_map_and_a_cap_of_k_or_more_are_the_sim_calls_bytes(world, sim, shrink):
    w = world
    sessions = H.all_sessions()
    weights = weights_for(sessions)
    deny = G.case("e")["deny"]
    for k in (10, 64):
        plain = w.m.cf_recommend_filtered(sessions, k, weights=weights, deny=deny, sim=sim, shrink=shrink)
        for group_of, cap in [(None, 1), ({}, 3), (G.case("d")["group_of"], k), (G.case("g")["group_of"], 64), (G.case("a")["group_of"], k)]:
            got = w.m.cf_recommend_grouped(sessions, k, group_of, cap, weights=weights, deny=deny, sim=sim, shrink=shrink)
            assert same_bytes(got, plain), (k, cap)
            dev = grouped_dev(w.m, sessions, k, group_of, cap, sim, shrink, weights=weights, deny=deny)
            assert dev[2].tobytes() == plain[2].tobytes()
            for s in range(len(sessions)):
                n = int(plain[2][s])
                assert dev[0][s, :n].tobytes() == plain[0][s, :n].tobytes() and dev[1][s, :n].tobytes() == plain[1][s, :n].tobytes()


@pytest.mark.parametrize("name,sim,shrink,weighted", [("a", "cosine", 0.0, False), ("b", "lift", 0.5, True), ("e", "jaccard", 10.0, True),
                                                      ("g", "cosine", 0.1, True)])
def test_the_rank_call_agrees_without_the_model(world, name, sim, shrink, weighted):
    """the same arguments to both calls: the filters of the case, and a measure and weights that reach the _sim instances"""
    w, c = world, G.case(name)
    sessions = H.all_sessions()
    kw = dict(exclude=c["exclude"], deny=c["deny"], sim=sim, shrink=shrink, weights=weights_for(sessions) if weighted else None)
    ids, sc, cnt = w.m.cf_recommend_grouped(sessions, c["k"], c["group_of"], c["cap"], **kw)
    targets = [ids[s, :int(cnt[s])].tolist() for s in range(len(sessions))]
    ranks, scores, ncand = w.m.cf_rank(sessions, targets, **kw)
    assert scores.tobytes() == np.concatenate([sc[s, :int(cnt[s])] for s in range(len(sessions))]).tobytes()
    arr = G.as_array(c["group_of"])
    j = 0
    beyond = 0
    for s in range(len(sessions)):
        r = ranks[j:j + int(cnt[s])].astype(np.int64)
        j += int(cnt[s])
        assert (np.diff(r) > 0).all() and (r < int(ncand[s])).all(), s    # in ranking order, every one a candidate
        beyond += int((r >= 64).sum())
        g = [G.group_of_id(arr, b) for b in targets[s]]
        assert all(g.count(x) <= c["cap"] for x in set(g) - {GROUP_NONE}), s
    assert beyond >= 5 or name in "be"                                    # (a: the model test's ranks; g: 64 groups) results no cut at 64 could have held


def test_the_null_stream_gives_the_same_bytes(world):
    w, c = world, G.case("g")
    sessions = H.all_sessions()
    a = grouped_dev(w.m, sessions, c["k"], c["group_of"], c["cap"], "cosine", 0.1)
    b = grouped_dev(w.m, sessions, c["k"], c["group_of"], c["cap"], "cosine", 0.1, own_stream=False)
    assert same_bytes(a, b)
    compare(w, b, sessions, c, "cosine", 0.1, tag="NULL stream", zero_filled=False)


def test_each_refusal_leaves_the_outputs_as_they_were(world):
    import torch
    w = world
    lib, h = w.m._lib, w.m._h
    sessions = [[300, 301, 302], [H.HOT, 303], []]
    n, K = len(sessions), 10
    off, items = flat(sessions, np.uint32)
    grp = G.case("d")["group_of"]                                         # one group for everybody: a cap of 1 leaves one result
    sentinel = lambda: (np.full((n, K), 0xabcdef, np.uint32), np.full((n, K), -7.5), np.full(n, 99, np.uint32))   # noqa: E731
    untouched = lambda got: all(a.tobytes() == b.tobytes() for a, b in zip(got, sentinel()))                   # noqa: E731

    def host(sim=0, shrink=0.0, k=K, cap=1, grp_ptr=True, group_n=grp.size, deny_n=0, weights=None, ex_off=None):
        out = sentinel()
        rc = lib.smatrix_cf_recommend_grouped(h, n, p64(off), p32(items), None if weights is None else pd(weights), ex_off, None, None, deny_n,
                                              p32(grp) if grp_ptr else None, group_n, cap, sim, shrink, k, p32(out[0]), pd(out[1]), p32(out[2]))
        return rc, out

    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)                 # noqa: E731
    d_off, d_items, d_grp = up(off, np.int64), up(items, np.int32), up(grp, np.int32)
    d_out = [torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else a.dtype)).to(dev) for a in sentinel()]

    def on_device(sim=0, shrink=0.0, k=K, cap=1, grp_ptr=True, group_n=grp.size, deny_n=0, ex_off=None):
        rc = lib.smatrix_cf_recommend_grouped_dev(h, n, d_off.data_ptr(), d_items.data_ptr(), None, ex_off, None, None, deny_n,
                                                  d_grp.data_ptr() if grp_ptr else None, group_n, cap, sim, shrink, k, d_out[0].data_ptr(),
                                                  d_out[1].data_ptr(), d_out[2].data_ptr(), None)
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy().view(np.uint32 if t.dtype == torch.int32 else np.float64) for t in d_out]

    bad = [dict(cap=0), dict(cap=65), dict(cap=0xFFFFFFFF), dict(group_n=(1 << 32) + 1), dict(grp_ptr=False), dict(grp_ptr=False, group_n=1),
           dict(sim=3), dict(shrink=-1.0), dict(shrink=float("nan")), dict(k=0), dict(k=65), dict(deny_n=5), dict(ex_off=p64(off))]
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
    plain = w.m.cf_recommend_filtered(sessions, K)
    rc, got = host(grp_ptr=False, group_n=0, cap=64)                      # NULL with no ids is no grouping
    assert rc == 0 and same_bytes(got, plain)
    rc, got = host()                                                      # ... and the good call behind the refusals
    want = w.m.cf_recommend_grouped(sessions, K, grp, 1)
    assert rc == 0 and same_bytes(got, want) and not same_bytes(got, plain)
    assert lib.smatrix_cf_recommend_grouped(h, 0, None, None, None, None, None, None, 0, None, 0, 1, 0, 0.0, K, None, None, None) == 0
    for kw in (dict(cap=0), dict(cap=65), dict(cap=True), dict(cap=1.5)):
        with pytest.raises(ValueError):
            w.m.cf_recommend_grouped(sessions, K, grp, kw["cap"])
    with pytest.raises(ValueError):
        w.m.cf_recommend_grouped(sessions, K, [1, -1], 1)
