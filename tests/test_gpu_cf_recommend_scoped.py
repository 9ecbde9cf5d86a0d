"""GPU (-m gpu): the scoped call (include/smatrix_batch.h smatrix_cf_recommend_scoped / _dev; SparseMatrix.cf_recommend_scoped,
cf_recommend_scoped_dev).

Expected results: tests/cf_scope_helpers.py scoped() -- the grouped fill model over the matrix's own export("sorted") with the session's
exclusion list extended by every id that is not allowed for it.  Ids, counts and n_scored must be equal and the scores' BYTES must
match.  The matrix is the world of tests/test_gpu_cf_sim.py, built as tests/test_gpu_cf_rank.py builds it; its sessions reach both
tiers (tests/test_gpu_cf_sim.py shows that); tests/test_cf_scope_model.py shows, without a GPU, that the map and the lists hold the
hard cases.  The world is built from SET ops: no row of it holds a key twice."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import _lib
from tests import cf_fill_helpers as F
from tests import cf_group_fill_helpers as GF
from tests import cf_group_helpers as G
from tests import cf_scope_helpers as S
from tests import cf_sim_helpers as H
from tests.test_gpu_cf_rank import bitmap, build_world
from tests.test_gpu_cf_sim import LDS_SLOTS, World, flat, need, same_bytes

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
p32, p64, pd = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p)), (lambda a: a.ctypes.data_as(DP))
JUNK_ID, JUNK_SCORE = 0x7a7a7a7a, -7.5
ARR, N = S.scope_map(), S.SCOPE_N
SESSIONS = H.all_sessions()
LISTS = S.scope_lists(SESSIONS)


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


def compare(w, got, sessions, lists, mode, k, sim="cosine", shrink=0.0, arr=ARR, scope_n=N, group_of=None, cap=64, fill=(), weights=None,
            exclude=None, deny=(), tag="", zero_filled=True):
    ids, sc, cnt, nsc = got
    assert ids.dtype == np.uint32 and sc.dtype == np.float64 and cnt.dtype == np.uint32 and nsc.dtype == np.uint32
    assert ids.shape == sc.shape == (len(sessions), k)
    for s, sess in enumerate(sessions):
        wi, ws, wn = S.scoped(w.model, sess, k, H.SIMS[sim], shrink, arr, scope_n, lists[s] or [], S.MODES[mode], S.universe(), G.as_array(group_of),
                              cap, fill, None if weights is None else weights[s], () if exclude is None else exclude[s], deny)
        assert (int(nsc[s]), int(cnt[s])) == (wn, len(wi)), (tag, s, int(nsc[s]), int(cnt[s]), wn, len(wi))
        assert ids[s, :len(wi)].tolist() == wi, (tag, s)
        assert sc[s, :len(wi)].tobytes() == ws.tobytes(), (tag, s)
        if zero_filled:
            assert not ids[s, len(wi):].any() and sc[s, len(wi):].tobytes() == bytes(8 * (k - len(wi))), (tag, s)
        else:                                                             # _dev leaves what it does not own
            assert (ids[s, len(wi):] == JUNK_ID).all() and (sc[s, len(wi):] == JUNK_SCORE).all(), (tag, s)


def scoped_dev(m, sessions, k, arr, scope_n, lists, mode, group_of=None, cap=64, fill=(), sim="cosine", shrink=0.0, weights=None, exclude=None,
               deny=None, expect_error=False):
    """SparseMatrix.cf_recommend_scoped_dev on torch tensors, on a stream of its own; the outputs start as junk.  lists None: no scope"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    off, items = flat(sessions, np.uint32)
    n = len(sessions)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)             # noqa: E731
        d_off, d_items = up(off, np.int64), up(items, np.int32)
        d_w = d_exoff = d_ex = d_bits = d_grp = d_fill = d_scp = d_scoff = d_scgr = None
        deny_n = group_n = 0
        if weights is not None:
            d_w = torch.from_numpy(flat(weights, np.float64)[1]).to(dev)
        if exclude is not None:
            ex_off, ex = flat(exclude, np.uint32)
            d_exoff, d_ex = up(ex_off, np.int64), up(ex, np.int32)
        if deny is not None:
            bits, deny_n = bitmap(deny)
            d_bits = up(bits, np.int32)
        garr = G.as_array(group_of)
        if garr is not None:
            d_grp, group_n = up(garr, np.int32), int(garr.size)
        if len(fill):
            d_fill = up(np.asarray(fill, np.uint32), np.int32)
        if lists is not None:
            sc_off, sc_gr = flat([l or [] for l in lists], np.uint32)
            d_scoff, d_scgr = up(sc_off, np.int64), up(np.concatenate([sc_gr, np.zeros(1, np.uint32)]), np.int32)
            if scope_n:
                d_scp = up(np.ascontiguousarray(arr[:scope_n]), np.int32)
        else:
            scope_n = 0
        d_ids = torch.full((n, k), JUNK_ID, dtype=torch.int32, device=dev)
        d_sc = torch.full((n, k), JUNK_SCORE, dtype=torch.float64, device=dev)
        d_cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
        d_nsc = torch.full((n,), 98, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()               # noqa: E731
        args = (n, d_off.data_ptr(), d_items.data_ptr(), ptr(d_w), ptr(d_exoff), ptr(d_ex), ptr(d_bits), deny_n, ptr(d_scp), scope_n, ptr(d_scoff),
                ptr(d_scgr), mode, ptr(d_grp), group_n, cap, ptr(d_fill), len(fill), sim, shrink, k, d_ids.data_ptr(), d_sc.data_ptr(),
                d_cnt.data_ptr(), d_nsc.data_ptr())
        if expect_error:
            with pytest.raises(ValueError):
                m.cf_recommend_scoped_dev(*args, stream=st)
        else:
            m.cf_recommend_scoped_dev(*args, stream=st)
    st.synchronize()
    return d_ids.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32), d_nsc.cpu().numpy().view(np.uint32)


def extended(sessions, lists, mode, arr=ARR, scope_n=N, exclude=None):
    """the explicit exclusion lists of the header's equivalence: every id of the universe that is not allowed, behind the session's own"""
    return [list(() if exclude is None else exclude[s]) + S.not_allowed(arr, scope_n, lists[s] or [], S.MODES[mode], S.universe())
            for s in range(len(sessions))]


# ---- 1: both modes, every measure, weights: the model's bytes in both tiers ------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink", [(sim, h) for sim in ("cosine", "jaccard", "lift") for h in (0.0, 10.0)])
@pytest.mark.parametrize("mode", ["only", "except"])
def test_both_modes_are_the_models_bytes(world, mode, sim, shrink):
    w = world
    rng = np.random.default_rng(3)
    weights = [(rng.random(len(s)) * 4).tolist() for s in SESSIONS]
    assert max(need(w.m, s) for s in H.lds_sessions()) <= LDS_SLOTS and all(need(w.m, s) > LDS_SLOTS for s in H.global_sessions())
    got = w.m.cf_recommend_scoped(SESSIONS, 10, ARR, LISTS, mode, weights=weights, sim=sim, shrink=shrink)
    compare(w, got, SESSIONS, LISTS, mode, 10, sim, shrink, weights=weights, tag=(mode, sim, shrink))
    assert got[3].tobytes() == got[2].tobytes()                           # no fill list: everything is scored
    if shrink == 0.0:
        dev = scoped_dev(w.m, SESSIONS, 10, ARR, N, LISTS, mode, sim=sim, shrink=shrink, weights=weights)
        compare(w, dev, SESSIONS, LISTS, mode, 10, sim, shrink, weights=weights, tag=("dev", mode, sim), zero_filled=False)


# ---- 2: one batch, sessions side by side ----------------------------------------------------------------------------------------
def test_every_session_reads_its_own_list(world):
    w = world
    sess = [10, 11, 12, 11]                                               # 217 candidates, all POOL ids: categories 0 .. 6 and NONE
    sessions = [sess, sess, sess, sess, [H.HOT], [H.HOT], [H.HOT]]
    lists = [None, [1, 2], [3, 4, 5], [77777, S.NONE], [6], [], [0]]
    for k in (10, 64):
        got = w.m.cf_recommend_scoped(sessions, k, ARR, lists, "only")
        compare(w, got, sessions, lists, "only", k, tag=("side by side", k))
        ids, _, cnt, _ = got
        assert cnt[3] == 0 and cnt[0] == k and cnt[1] > 0 and cnt[2] > 0
        assert set(ARR[ids[1, :cnt[1]]].tolist()) <= {1, 2} and set(ARR[ids[2, :cnt[2]]].tolist()) <= {3, 4, 5}
        assert set(ARR[ids[4, :cnt[4]]].tolist()) == {6} and set(ARR[ids[6, :cnt[6]]].tolist()) == {0}
        assert ids[5].tobytes() == w.m.cf_recommend_filtered([[H.HOT]], k)[0][0].tobytes()
        dev = scoped_dev(w.m, sessions, k, ARR, N, lists, "only")
        compare(w, dev, sessions, lists, "only", k, tag=("side by side, dev", k), zero_filled=False)
    got = w.m.cf_recommend_scoped(sessions, 10, ARR, lists, "except")
    compare(w, got, sessions, lists, "except", 10, tag="side by side, except")
    assert same_bytes([got[0][3]], [got[0][0]])                           # a list that matches nothing excepts nothing


# ---- 3: the longest lists -----------------------------------------------------------------------------------------------------------
def test_lists_of_1_63_64_entries_and_the_refusal_of_65(world):
    w = world
    sess = [10, 11, 12, 11]
    pad = list(range(1000, 1100))                                         # groups nobody has
    lists = [[3], pad[:62] + [3], pad[:63] + [3], []]
    sessions = [sess, sess, sess, [H.HOT, 301]]
    for mode in ("only", "except"):
        got = w.m.cf_recommend_scoped(sessions, 10, ARR, lists, mode)
        compare(w, got, sessions, lists, mode, 10, tag=("long lists", mode))
        assert same_bytes([got[0][0], got[1][0]], [got[0][1], got[1][1]]) and same_bytes([got[0][0], got[1][0]], [got[0][2], got[1][2]])
        dev = scoped_dev(w.m, sessions, 10, ARR, N, lists, mode)
        compare(w, dev, sessions, lists, mode, 10, tag=("long lists, dev", mode), zero_filled=False)
    lists[1] = pad[:64] + [3]                                             # 65: refused by both flavours
    with pytest.raises(ValueError):
        w.m.cf_recommend_scoped(sessions, 10, ARR, lists, "only")
    off, items = flat(sessions, np.uint32)
    sc_off, sc_gr = flat(lists, np.uint32)
    out = (np.full((4, 10), 0xabcdef, np.uint32), np.full((4, 10), -7.5), np.full(4, 99, np.uint32), np.full(4, 98, np.uint32))
    rc = w.m._lib.smatrix_cf_recommend_scoped(w.m._h, 4, p64(off), p32(items), None, None, None, None, 0, p32(ARR), N, p64(sc_off), p32(sc_gr), 0, None,
                                              0, 64, None, 0, 0, 0.0, 10, p32(out[0]), pd(out[1]), p32(out[2]), p32(out[3]))
    assert rc == -1                                                       # the host flavour walks sc_offsets before the device is touched
    assert (out[0] == 0xabcdef).all() and (out[1] == -7.5).all() and (out[2] == 99).all() and (out[3] == 98).all()
    scoped_dev(w.m, sessions, 10, ARR, N, lists, "only", expect_error=True)
    scoped_dev(w.m, sessions, 10, ARR, N, lists, "only", fill=[S.FR[0], S.FR[1]], expect_error=True)


# ---- 4: items out of scope, the map's end, no map ---------------------------------------------------------------------------------------
def test_an_item_out_of_scope_still_scores_and_the_maps_end(world):
    w = world
    sess = [300, 301, 304]                                                # SMALL items: 300 and 304 in category 100, 301 in 0xFFFFFFFE
    sessions, lists = [sess, sess], [[0xFFFFFFFE], [0xFFFFFFFE]]
    got = w.m.cf_recommend_scoped(sessions, 10, ARR, lists, "only")
    compare(w, got, sessions, lists, "only", 10, tag="items out of scope")
    ids, sc, cnt, _ = got
    assert cnt[0] > 0 and not set(ids[0, :cnt[0]].tolist()) & set(sess) and all(b % 2 == 1 for b in ids[0, :cnt[0]].tolist())
    only301 = w.m.cf_recommend_scoped([[301]], 10, ARR, [[0xFFFFFFFE]], "only")
    assert sc[0].tobytes() != only301[1][0].tobytes()                     # the rows of 300 and 304 contribute although both are out of scope
    # the map's end: a candidate at scope_n - 1 is grouped, the same id at scope_n is not
    r = [b for b, _ in w.model.ranking([H.HOT], 0, 0.0)]
    b = next(c for c in r[:10] if int(ARR[c]) != S.NONE)                  # among the ten best, so in or out of the result by its scope alone
    g = int(ARR[b])
    for scope_n, inside in ((b + 1, True), (b, False)):
        for mode in ("only", "except"):
            got = w.m.cf_recommend_scoped([[H.HOT]], 10, ARR[:scope_n], [[g]], mode)
            compare(w, got, [[H.HOT]], [[g]], mode, 10, scope_n=scope_n, tag=("map end", scope_n, mode))
            assert (b in got[0][0].tolist()) == (inside == (mode == "only"))
            dev = scoped_dev(w.m, [[H.HOT]], 10, ARR, scope_n, [[g]], mode)
            compare(w, dev, [[H.HOT]], [[g]], mode, 10, scope_n=scope_n, tag=("map end, dev", scope_n, mode), zero_filled=False)
    # scope_n == 0 with lists given: everything is ungrouped -- nothing for ONLY, everything for EXCEPT
    for mode in ("only", "except"):
        got = w.m.cf_recommend_scoped(SESSIONS, 10, None, LISTS, mode)
        compare(w, got, SESSIONS, LISTS, mode, 10, arr=None, scope_n=0, tag=("no map", mode))
        dev = scoped_dev(w.m, SESSIONS, 10, ARR, 0, LISTS, mode)
        compare(w, dev, SESSIONS, LISTS, mode, 10, arr=None, scope_n=0, tag=("no map, dev", mode), zero_filled=False)
    scoped_sessions = [i for i, l in enumerate(LISTS) if l]
    assert not w.m.cf_recommend_scoped(SESSIONS, 10, None, LISTS, "only")[2][scoped_sessions].any()


# ---- 5: scope with quotas ---------------------------------------------------------------------------------------------------------------
def test_an_out_of_scope_candidate_consumes_no_quota(world):
    w = world
    sess = [10, 11, 12, 11]
    r = [b for b, _ in w.model.ranking(sess, 0, 0.0)]
    best = r[0]
    brands = {int(b): 500 + i // 8 for i, b in enumerate(r)}              # brand = eight consecutive ranks: `best` leads brand 500
    scope = ARR.copy()
    scope[best] = 6000                                                    # a category of its own, which the session excepts
    sessions, lists = [sess, [H.HOT], sess], [[6000], [6000, 1], []]
    for cap in (1, 2):
        got = w.m.cf_recommend_scoped(sessions, 10, scope, lists, "except", group_of=brands, cap=cap)
        compare(w, got, sessions, lists, "except", 10, arr=scope, group_of=brands, cap=cap, tag=("quotas", cap))
        assert best not in got[0][0].tolist() and got[0][0][:cap].tolist() == r[1:1 + cap]      # brand 500's quota goes to the next of it
        assert got[0][2][:cap].tolist() == r[:cap]                        # ... and the unscoped session beside it still gets `best`
        dev = scoped_dev(w.m, sessions, 10, scope, N, lists, "except", group_of=brands, cap=cap)
        compare(w, dev, sessions, lists, "except", 10, arr=scope, group_of=brands, cap=cap, tag=("quotas, dev", cap), zero_filled=False)
    # ... and once with ONE array as both maps: at most cap results per category, from the listed categories
    lists = [[1, 2, 3], [4], None]
    got = w.m.cf_recommend_scoped(sessions, 10, ARR, lists, "only", group_of=ARR, cap=2)
    compare(w, got, sessions, lists, "only", 10, group_of=ARR, cap=2, tag="one array twice")
    assert got[2].tolist()[:2] == [6, 2]
    d_arr = scoped_dev(w.m, sessions, 10, ARR, N, lists, "only", group_of=ARR, cap=2)
    compare(w, d_arr, sessions, lists, "only", 10, group_of=ARR, cap=2, tag="one array twice, dev", zero_filled=False)


# ---- 6: scope with fill -----------------------------------------------------------------------------------------------------------------
def test_the_fill_walks_past_ids_out_of_scope(world):
    w = world
    FR = S.FR
    cat = int(ARR[FR[71]])
    step = [b for b in FR[:121] if int(ARR[b]) != cat][:64]               # a step of 64 list ids, all out of the scope [cat]
    fill = [0, 10, FR[71]] + step[:61] + step + [FR[1], FR[8], 50301, FR[121], FR[78], FR[85], FR[92], FR[99], FR[15], FR[22], FR[29], FR[36], FR[43]]
    assert len(fill) >= 128 and int(ARR[FR[1]]) == cat and not set(fill[64:128]) & {b for b in FR[:121] if int(ARR[b]) == cat}
    sessions = [[], [H.ABSENT], [10], [10, 0, 10, H.ABSENT], [H.HOT], [300, 301]]
    hot_cat = int(ARR[GF.hot_left()[0]])                                  # heavy_deny() leaves [HOT] three candidates: one of them stays in scope
    lists = [[cat], [cat, 5000], [cat], [], [hot_cat, cat], [200, cat]]
    deny = F.heavy_deny()
    assert hot_cat != S.NONE
    for mode in ("only", "except"):
        for k in (10, 64):
            got = w.m.cf_recommend_scoped(sessions, k, ARR, lists, mode, fill=fill, deny=deny)
            compare(w, got, sessions, lists, mode, k, fill=fill, deny=deny, tag=("fill", mode, k))
            dev = scoped_dev(w.m, sessions, k, ARR, N, lists, mode, fill=fill, deny=deny)
            compare(w, dev, sessions, lists, mode, k, fill=fill, deny=deny, tag=("fill, dev", mode, k), zero_filled=False)
            assert same_bytes(dev[2:], got[2:])
    ids, _, cnt, nsc = w.m.cf_recommend_scoped(sessions, 10, ARR, lists, "only", fill=fill, deny=deny)
    assert nsc[0] == 0 and ids[0, :cnt[0]].tolist()[:3] == [FR[71], FR[1], FR[8]]     # an in-scope id without a row is filled, past the empty step
    assert FR[121] not in ids[0].tolist() and 50301 not in ids[0].tolist()            # ungrouped: beyond the map's end, named NONE
    assert (nsc < 10).all() and nsc[4] > 0 and cnt[4] == 10                           # n_scored is the scored count, in the global tier too
    # ... and under quotas, through the one scoped fill kernel with a map that binds
    brands = {FR[i]: 900 + i // 14 for i in range(121)}
    got = w.m.cf_recommend_scoped(sessions, 10, ARR, lists, "only", group_of=brands, cap=1, fill=fill, deny=deny)
    compare(w, got, sessions, lists, "only", 10, group_of=brands, cap=1, fill=fill, deny=deny, tag="fill under quotas")
    dev = scoped_dev(w.m, sessions, 10, ARR, N, lists, "only", group_of=brands, cap=1, fill=fill, deny=deny)
    compare(w, dev, sessions, lists, "only", 10, group_of=brands, cap=1, fill=fill, deny=deny, tag="fill under quotas, dev", zero_filled=False)


# ---- 7: the equivalence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["only", "except"])
def test_the_call_is_grouped_fill_under_extended_exclusion_lists(world, mode):
    w = world
    sessions, exclude = GF.sessions_and_lists()
    lists = S.scope_lists(sessions, seed=9)
    more = extended(sessions, lists, mode, exclude=exclude)
    moved = [s for s, (se, e, m) in enumerate(zip(sessions, exclude, more)) if lists[s] and need(w.m, se, len(e)) <= LDS_SLOTS < need(w.m, se, len(m))]
    assert moved or mode == "except"                                      # ONLY: the explicit lists move sessions to the global tier
    kw = dict(deny=F.DENY, sim="cosine", shrink=0.1)
    for k, cap in ((10, 2), (64, 1)):
        got = w.m.cf_recommend_scoped(sessions, k, ARR, lists, mode, group_of=GF.group_map(), cap=cap, fill=GF.fill_list(), exclude=exclude, **kw)
        want = w.m.cf_recommend_grouped_filled(sessions, k, GF.group_map(), cap, GF.fill_list(), exclude=more, **kw)
        assert same_bytes(got, want), (mode, k, cap)


# ---- 8: no scope ---------------------------------------------------------------------------------------------------------------------------
def test_no_scope_is_the_grouped_fill_call(world):
    w = world
    sessions, exclude = GF.sessions_and_lists()
    kw = dict(exclude=exclude, deny=F.DENY)
    for k, cap, sim, shrink in ((10, 2, "cosine", 0.0), (64, 1, "lift", 0.5)):
        want = w.m.cf_recommend_grouped_filled(sessions, k, GF.group_map(), cap, GF.fill_list(), sim=sim, shrink=shrink, **kw)
        empty = [[] for _ in sessions]
        for scope_of, scope in ((None, [None] * len(sessions)), (ARR, empty)):
            got = w.m.cf_recommend_scoped(sessions, k, scope_of, scope, "only", group_of=GF.group_map(), cap=cap, fill=GF.fill_list(), sim=sim,
                                          shrink=shrink, **kw)
            assert same_bytes(got, want), (k, cap)
        null = scoped_dev(w.m, sessions, k, ARR, N, None, "except", group_of=GF.group_map(), cap=cap, fill=GF.fill_list(), sim=sim, shrink=shrink, **kw)
        lists = scoped_dev(w.m, sessions, k, ARR, N, empty, "except", group_of=GF.group_map(), cap=cap, fill=GF.fill_list(), sim=sim, shrink=shrink, **kw)
        assert same_bytes(null, lists)                                    # sc_offsets NULL, and every list empty through the scoped kernels
        for s in range(len(sessions)):
            c = int(want[2][s])
            assert null[0][s, :c].tobytes() == want[0][s, :c].tobytes() and null[1][s, :c].tobytes() == want[1][s, :c].tobytes()
        assert same_bytes(null[2:], want[2:])
    # without quotas and without a list it is the sim call
    got = w.m.cf_recommend_scoped(sessions, 10, None, [None] * len(sessions), sim="jaccard", shrink=10.0, **kw)
    sim_call = w.m.cf_recommend_filtered(sessions, 10, sim="jaccard", shrink=10.0, **kw)
    assert same_bytes(got[:3], sim_call) and got[3].tobytes() == got[2].tobytes()
    # one scoped session, no quotas: the scoped fill kernel against the plain one, which is given what the scope keeps out as a list
    one = [l if s == 11 else [] for s, l in enumerate(S.scope_lists(sessions, seed=9))]
    for k in (10, 64):
        got = w.m.cf_recommend_scoped(sessions, k, ARR, one, "only", fill=GF.fill_list(), **kw)
        want = w.m.cf_recommend_filled(sessions, k, GF.fill_list(), exclude=extended(sessions, one, "only", exclude=exclude), deny=F.DENY)
        assert one[11] and 0 < got[3][11] < got[2][11]                    # the session is scoped, scores some results and fills some
        assert same_bytes(got, want), k


# ---- 9: offsets that do not start at 0 ---------------------------------------------------------------------------------------------------
def test_the_host_flavour_takes_a_window_of_the_lists(world):
    w = world
    n, K = len(SESSIONS), 10
    off, items = flat(SESSIONS, np.uint32)
    sc_off, sc_gr = flat([l or [] for l in LISTS], np.uint32)
    shifted_off = sc_off + np.uint64(5)
    shifted_gr = np.concatenate([np.full(5, 3, np.uint32), sc_gr])        # five entries in front that belong to nobody
    out = (np.zeros((n, K), np.uint32), np.zeros((n, K)), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    rc = w.m._lib.smatrix_cf_recommend_scoped(w.m._h, n, p64(off), p32(items), None, None, None, None, 0, p32(ARR), N, p64(shifted_off), p32(shifted_gr),
                                              0, None, 0, 64, None, 0, 0, 0.0, K, p32(out[0]), pd(out[1]), p32(out[2]), p32(out[3]))
    assert rc == 0 and same_bytes(out, w.m.cf_recommend_scoped(SESSIONS, K, ARR, LISTS, "only"))


# ---- 10, 11: twice, and another stream -----------------------------------------------------------------------------------------------------
def test_the_same_call_twice_and_the_dev_flavour_on_a_stream_of_its_own(world):
    w = world
    kw = dict(group_of=GF.group_map(), cap=2, fill=GF.fill_list(), deny=F.DENY)
    a = w.m.cf_recommend_scoped(SESSIONS, 10, ARR, LISTS, "only", **kw)
    b = w.m.cf_recommend_scoped(SESSIONS, 10, ARR, LISTS, "only", **kw)
    assert same_bytes(a, b)
    c = scoped_dev(w.m, SESSIONS, 10, ARR, N, LISTS, "only", **kw)        # (scoped_dev runs on a torch.cuda.Stream of its own)
    d = scoped_dev(w.m, SESSIONS, 10, ARR, N, LISTS, "only", **kw)
    assert same_bytes(c, d) and same_bytes(c[2:], a[2:])
    for s in range(len(SESSIONS)):
        n = int(a[2][s])
        assert c[0][s, :n].tobytes() == a[0][s, :n].tobytes() and c[1][s, :n].tobytes() == a[1][s, :n].tobytes()
