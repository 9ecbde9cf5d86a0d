"""GPU (-m gpu): filtered, weighted session recommendations (include/smatrix_batch.h smatrix_cf_recommend_filtered / _dev,
SparseMatrix.cf_recommend_filtered / cf_recommend_filtered_dev).  The expected result is Expect.session of
test_gpu_cf_recommend.py restated with three changes: a term is multiplied by the weight at its item's first position, as a
Python float, before it is added; candidates on the session's exclusion list or in the deny set are removed; then the sort by
(-score, id) and the cut at k.  The terms are the oracle's (ora_cf_neighbors).  Ids, counts and the scores' BYTES must match, in
the LDS tier and in the global tier alike."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix, _lib

pytestmark = pytest.mark.gpu

ABSENT = 987654321
HUB = 1
SMALL = np.arange(300, 356)                       # 56 items that all meet each other: rows of at most 128 slots
LDS_SLOTS = 4096                                  # kernels/recommend.hpp REC_LDS_SLOTS
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


def import_sessions(rng):
    """about 60 small items; a hub whose row has more than 4096 slots (250 sessions of [hub] + 30 ids drawn from 20 000);
    item 0 in a few"""
    sess = [[HUB] + rng.integers(1000, 21000, 30).tolist() for _ in range(250)]
    sess += [rng.choice(SMALL, int(rng.integers(2, 8)), replace=False).tolist() for _ in range(400)]
    sess += [[0, 300, 301], [0, 305, 7], [7, 7, 9]]
    return sess


class Model:
    """the contract, restated over the oracle (built once per module and never changed: the neighbour lists are cached)"""

    def __init__(self, oracle_mod, o):
        self.O, self.o, self.nb = oracle_mod, o, {}

    def neighbours(self, a):
        if a not in self.nb:
            wi, ws = self.O.cf_neighbors(self.o, a, 1 << 16)
            self.nb[a] = (wi.tolist(), ws.tolist())
        return self.nb[a]

    def ranking(self, sess, w=None, excl=(), deny=()):
        own, gone = set(int(a) for a in sess), set(int(a) for a in excl) | set(int(a) for a in deny)
        score, done = {}, set()
        for i, a in enumerate(int(v) for v in sess):
            if a in done:
                continue
            done.add(a)
            wa = 1.0 if w is None else float(w[i])
            for b, t in zip(*self.neighbours(a)):
                if b != 0 and b not in own:
                    score[b] = score.get(b, 0.0) + wa * t
        return sorted(((b, s) for b, s in score.items() if b not in gone), key=lambda kv: (-kv[1], kv[0]))

    def session(self, sess, k, w=None, excl=(), deny=()):
        best = self.ranking(sess, w, excl, deny)[:k]
        return [b for b, _ in best], np.array([s for _, s in best], np.float64)


class World:
    pass


@pytest.fixture(scope="module")
def world(oracle_mod):
    rng = np.random.default_rng(17)
    w = World()
    w.imported = import_sessions(rng)
    w.m, w.o = SparseMatrix(), oracle_mod.Oracle()
    w.m.cf_import_sessions(w.imported)
    for s in w.imported:
        oracle_mod.cf_import_preference_set(w.o, s)
    w.model = Model(oracle_mod, w.o)
    w.tail = sorted(set(int(w.imported[i][1]) for i in range(20)))    # ids of 20 hub sessions: small rows that hold the hub
    assert w.m.row_info(HUB)[0] > LDS_SLOTS
    yield w
    w.m.close(); w.o.close()


def need(m, sess, E=0):
    """k_rec_bound's sum: the slots of the distinct items' rows + the session's length + its exclusion list's"""
    return sum((m.row_info(a) or (0, 0))[0] for a in set(int(v) for v in sess)) + len(sess) + E


def lds_sessions(rng, w, n=40):
    out = [[], [ABSENT], [0], [0, 0, 300], [3, 3, 5, 0, 7], list(w.tail)]
    for _ in range(n):
        L = int(rng.integers(1, 25))
        s = rng.choice(SMALL, L).tolist()
        if L > 2:
            s[int(rng.integers(1, L))] = s[0]                       # a duplicate
        if L > 3 and rng.random() < 0.3:
            s[int(rng.integers(0, L))] = int(rng.choice([0, ABSENT, 7]))
        out.append([int(v) for v in s])
    return out


def global_sessions(w):
    return [[HUB], [HUB, 301, 302], [303, HUB, HUB, 0, ABSENT, 303], w.tail[:5] + [HUB] + [310, 311, 310]]


def both_tiers(rng, w):
    q = lds_sessions(rng, w)
    assert max(need(w.m, s) for s in q) <= LDS_SLOTS
    assert all(need(w.m, s) > LDS_SLOTS for s in global_sessions(w))
    for i, s in enumerate(global_sessions(w)):
        q.insert(3 + 9 * i, s)
    return q


def check(w, sessions, k, weights=None, exclude=None, deny=None, tag=""):
    ids, sc, cnt = w.m.cf_recommend_filtered(sessions, k, weights=weights, exclude=exclude, deny=deny)
    assert ids.shape == (len(sessions), k) and sc.shape == (len(sessions), k) and cnt.shape == (len(sessions),)
    compare(w, (ids, sc, cnt), sessions, k, weights, exclude, deny or (), tag)
    return ids, sc, cnt


def compare(w, got, sessions, k, weights, exclude, deny, tag=""):
    ids, sc, cnt = got
    for s, sess in enumerate(sessions):
        wi, ws = w.model.session(sess, k, None if weights is None else weights[s], () if exclude is None else exclude[s], deny)
        c = int(cnt[s])
        assert c == len(wi), (tag, k, s, c, len(wi))
        assert ids[s, :c].tolist() == wi, (tag, k, s)
        assert sc[s, :c].tobytes() == ws.tobytes(), (tag, k, s)
        assert not ids[s, c:].any() and not sc[s, c:].any(), (tag, k, s)       # the host flavour zero-fills


def flat(sessions, dtype):
    off = np.zeros(len(sessions) + 1, np.uint64)
    np.cumsum([len(s) for s in sessions], out=off[1:])
    return off, np.ascontiguousarray(np.concatenate([np.asarray(s, dtype) for s in sessions] + [np.zeros(0, dtype)]), dtype=dtype)


def raw_host(m, sessions, k, weights=None, ex=None, deny=None, out=None):
    """the C ABI itself: weights a flat float64 array, ex = (offsets, ids) where either may be None, deny = (bits, deny_n)
    where bits may be None -> (return code, ids, scores, counts)"""
    off, items = flat(sessions, np.uint32)
    n = len(sessions)
    ids, sc, cnt = out or (np.zeros((n, k), np.uint32), np.zeros((n, k), np.float64), np.zeros(n, np.uint32))
    ex_off, ex_ids = ex or (None, None)
    bits, deny_n = deny or (None, 0)
    rc = m._lib.smatrix_cf_recommend_filtered(
        m._h, n, off.ctypes.data_as(_lib.u64p), items.ctypes.data_as(_lib.u32p), None if weights is None else weights.ctypes.data_as(DP),
        None if ex_off is None else ex_off.ctypes.data_as(_lib.u64p), None if ex_ids is None else ex_ids.ctypes.data_as(_lib.u32p),
        None if bits is None else bits.ctypes.data_as(_lib.u32p), deny_n, k, ids.ctypes.data_as(_lib.u32p), sc.ctypes.data_as(DP),
        cnt.ctypes.data_as(_lib.u32p))
    return rc, ids, sc, cnt


def bitmap(ids, deny_n):
    bits = np.zeros((deny_n + 31) // 32, np.uint32)
    for b in ids:
        bits[b >> 5] |= np.uint32(1 << (b & 31))
    return bits


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_no_options_is_cf_recommend_batch(world):
    """all options None, and weights all 1.0, give cf_recommend_batch's bytes, in both tiers"""
    w = world
    sessions = both_tiers(np.random.default_rng(1), w)
    ones = [[1.0] * len(s) for s in sessions]
    for k in (1, 10, 64):
        want = w.m.cf_recommend_batch(sessions, k)
        for got in (w.m.cf_recommend_filtered(sessions, k), w.m.cf_recommend_filtered(sessions, k, weights=ones),
                    w.m.cf_recommend_filtered(sessions, k, exclude=[[] for _ in sessions], deny=[])):
            for a, b in zip(want, got):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    compare(w, want, sessions, 64, None, None, ())                    # (the model restates the unfiltered contract too)


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_weights(world):
    w = world
    rng = np.random.default_rng(2)
    sessions = both_tiers(rng, w)
    menu = np.array([0.0, 0.25, 0.5, 1.0, 3.0, 1e-3])
    for draw, tag in ((lambda L: rng.choice(menu, L).tolist(), "menu"), (lambda L: (rng.random(L) * 8).tolist(), "random")):
        weights = [draw(len(s)) for s in sessions]
        # the first position's weight counts: [303, HUB, HUB, 0, ABSENT, 303] and the LDS sessions' duplicates of s[0]
        g = sessions.index([303, HUB, HUB, 0, ABSENT, 303])
        weights[g] = [0.5, 3.0, 0.0, 0.25, 1.0, 7.0]
        h = sessions.index([3, 3, 5, 0, 7])
        weights[h] = [1.0, 2.0, -0.0, 0.5, 0.0]                      # -0.0, and an item (7) of weight 0: still an item
        t = sessions.index(list(w.tail))
        weights[t] = [0.0] + weights[t][1:]                           # a weight-0 item whose row's keys stay candidates
        for k in (10, 64):
            ids, sc, cnt = check(w, sessions, k, weights=weights, tag=tag)
        assert 7 not in ids[h, :cnt[h]].tolist()
    # a different weight at the second position of a duplicate changes nothing
    a = w.m.cf_recommend_filtered([[HUB, 301, HUB], [320, 321, 320]], 10, weights=[[2.0, 0.5, 9.0], [2.0, 0.5, 9.0]])
    b = w.m.cf_recommend_filtered([[HUB, 301, HUB], [320, 321, 320]], 10, weights=[[2.0, 0.5, 0.0], [2.0, 0.5, 0.0]])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_exclusion_beyond_k(world):
    """the first 200 of the unfiltered ranking excluded, k = 10: ranks 201 to 210, which no sequence of unfiltered calls gives"""
    w = world
    sessions = [list(w.tail), [HUB, 300, 301]]
    assert need(w.m, sessions[0], 200) <= LDS_SLOTS < need(w.m, sessions[1])
    ranks = [w.model.ranking(s) for s in sessions]
    assert all(len(r) >= 210 for r in ranks)
    exclude = [[b for b, _ in r[:200]] for r in ranks]
    ids, sc, cnt = check(w, sessions, 10, exclude=exclude)
    for s, r in enumerate(ranks):
        assert cnt[s] == 10 and ids[s].tolist() == [b for b, _ in r[200:210]]
        assert sc[s].tobytes() == np.array([v for _, v in r[200:210]]).tobytes()
    # a ranking shorter than that: all but its last 5
    few = [[300, 301, 302]]
    r = w.model.ranking(few[0])
    assert 5 < len(r) < 200
    ids, sc, cnt = check(w, few, 10, exclude=[[b for b, _ in r[:-5]]])
    assert cnt[0] == 5 and ids[0, :5].tolist() == [b for b, _ in r[-5:]]


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_exclusion_lists(world):
    w = world
    rng = np.random.default_rng(4)
    sessions = both_tiers(rng, w)
    exclude = []
    for i, s in enumerate(sessions):
        if i % 4 == 0:
            exclude.append([])                                        # an empty list beside full ones
            continue
        cand = [b for b, _ in w.model.ranking(s)]
        take = rng.choice(cand, min(len(cand), int(rng.integers(1, 40))), replace=False).tolist() if cand else []
        exclude.append([0, ABSENT + 1] + take + take[:3] + [int(v) for v in s[:2]])    # 0, absent, repeats, session items
    for k in (10, 64):
        check(w, sessions, k, exclude=exclude)
    # an excluded session item still contributes its row: excluding it changes nothing
    s = [[300, 301, 302], [HUB, 301]]
    a = w.m.cf_recommend_filtered(s, 10, exclude=[[300], [HUB]])
    b = w.m.cf_recommend_batch(s, 10)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # every candidate excluded
    every = [[b for b, _ in w.model.ranking(x)] for x in s]
    ids, sc, cnt = check(w, s, 10, exclude=every)
    assert cnt.tolist() == [0, 0]
    # a session of the LDS tier that its list moves to the global tier
    small = [SMALL[:30].tolist()]
    long_list = [331, 340] + rng.integers(356, 40000, 9998).tolist()
    assert need(w.m, small[0]) <= LDS_SLOTS < need(w.m, small[0], len(long_list))
    ids, sc, cnt = check(w, small + [[300, 301]], 64, exclude=[long_list, [302]])
    assert 0 < cnt[0] == len(w.model.ranking(small[0])) - 2


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_deny_bitmap(world):
    w = world
    rng = np.random.default_rng(5)
    sessions = both_tiers(rng, w)
    # through SparseMatrix: deny and exclude together; denied ids that are session items (300, HUB) or excluded as well
    deny = [HUB, 300, 301, 7] + list(range(306, 330, 2)) + list(range(1000, 15000, 3))
    exclude = [[330, 331, 306, 1000] for _ in sessions]
    for k in (10, 64):
        check(w, sessions, k, exclude=exclude, deny=deny)
    check(w, sessions, 10, deny=deny, weights=[[0.5] * len(s) for s in sessions])
    # through the C ABI: deny_n = 333 is no multiple of 32; the last word's bits past deny_n (ids 333 .. 351) are set and must not count
    deny_n = 333
    denied = [b for b in deny if b < deny_n]
    bits = bitmap(denied + list(range(deny_n, 352)), 352)[:(deny_n + 31) // 32].copy()
    rc, ids, sc, cnt = raw_host(w.m, sessions, 64, deny=(bits, deny_n))
    assert rc == 0
    compare(w, (ids, sc, cnt), sessions, 64, None, None, denied)
    assert any(340 in ids[s, :cnt[s]].tolist() for s in range(len(sessions)))      # a candidate >= deny_n stays
    # deny_n <= 2^32: the bound itself (2^32 + 1 is refused before the bitmap is read)
    rc, *_ = raw_host(w.m, sessions[:2], 10, deny=(bits, (1 << 32) + 1))
    assert rc == -1


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_dev_flavour_on_a_stream(world):
    import torch
    w = world
    rng = np.random.default_rng(6)
    sessions = both_tiers(rng, w)
    k, n = 10, len(sessions)
    weights = [(rng.random(len(s)) * 4).tolist() for s in sessions]
    exclude = [[b for b, _ in w.model.ranking(s)[:7]] + [0, 305] for s in sessions]
    deny = [HUB, 302] + list(range(1001, 9000, 5))
    ids, sc, cnt = check(w, sessions, k, weights=weights, exclude=exclude, deny=deny)
    off, items = flat(sessions, np.uint32)
    _, wf = flat(weights, np.float64)
    ex_off, ex_ids = flat(exclude, np.uint32)
    deny_n = max(deny) + 1
    bits = bitmap(deny, deny_n)
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.Stream(device=dev)
    outs = []
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)
        d_off, d_items, d_w = up(off, np.int64), up(items, np.int32), torch.from_numpy(wf).to(dev)
        d_exoff, d_ex, d_bits = up(ex_off, np.int64), up(ex_ids, np.int32), up(bits, np.int32)
        for _ in range(2):
            d_ids = torch.zeros(n * k, dtype=torch.int32, device=dev)
            d_sc = torch.zeros(n * k, dtype=torch.float64, device=dev)
            d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
            w.m.cf_recommend_filtered_dev(n, d_off.data_ptr(), d_items.data_ptr(), d_w.data_ptr(), d_exoff.data_ptr(), d_ex.data_ptr(),
                                          d_bits.data_ptr(), deny_n, k, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), stream=st)
            outs.append((d_ids, d_sc, d_cnt))
    st.synchronize()
    for d_ids, d_sc, d_cnt in outs:                 # (the outputs were zeroed, so the whole arrays match the host flavour's)
        assert d_ids.cpu().numpy().tobytes() == ids.tobytes()
        assert d_sc.cpu().numpy().tobytes() == sc.tobytes()
        assert d_cnt.cpu().numpy().tobytes() == cnt.tobytes()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(world):
    import torch
    w = world
    sessions = [[300, 301, 302], [HUB, 303], [310]]
    n, k = len(sessions), 10
    off, items = flat(sessions, np.uint32)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_off, d_items = torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(items.view(np.int32)).to(dev)
    d_ids = torch.zeros(n * k, dtype=torch.int32, device=dev)
    d_sc = torch.zeros(n * k, dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)

    def dev_call(d_w=None, d_exoff=None, d_ex=None, d_bits=None, deny_n=0):
        p = lambda t: None if t is None else t.data_ptr()
        rc = w.m._lib.smatrix_cf_recommend_filtered_dev(w.m._h, n, d_off.data_ptr(), d_items.data_ptr(), p(d_w), p(d_exoff), p(d_ex),
                                                        p(d_bits), deny_n, k, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    def valid_call_is_correct():
        check(w, sessions, k, weights=[[1.0, 0.5, 2.0], [0.25, 1.0], [1.0]], exclude=[[303], [], [311]], deny=[304])

    sentinel = lambda: (np.full((n, k), 0xabcdef, np.uint32), np.full((n, k), -7.5), np.full(n, 99, np.uint32))
    for bad in (-1.0, float("nan"), float("inf")):
        for pos in (0, 4, 5):                                         # in an LDS-tier session, a global-tier one, the last entry
            wf = np.ones(items.size)
            wf[pos] = bad
            out = sentinel()
            rc, *got = raw_host(w.m, sessions, k, weights=wf, out=out)
            assert rc == -1, (bad, pos)
            for a, b in zip(got, sentinel()):                         # the host flavour leaves the outputs as they were
                assert a.tobytes() == b.tobytes(), (bad, pos)
            assert dev_call(d_w=torch.from_numpy(wf).to(dev)) == -1, (bad, pos)
        valid_call_is_correct()
    ex_off = np.zeros(n + 1, np.uint64)
    some = np.zeros(4, np.uint32)
    assert raw_host(w.m, sessions, k, ex=(ex_off, None))[0] == -1
    assert raw_host(w.m, sessions, k, ex=(None, some))[0] == -1
    assert raw_host(w.m, sessions, k, deny=(None, 5))[0] == -1
    assert dev_call(d_exoff=torch.zeros(n + 1, dtype=torch.int64, device=dev)) == -1
    assert dev_call(d_ex=torch.zeros(4, dtype=torch.int32, device=dev)) == -1
    assert dev_call(deny_n=5) == -1
    assert dev_call(d_bits=torch.zeros(4, dtype=torch.int32, device=dev), deny_n=(1 << 32) + 1) == -1
    for kk in (0, 65):
        assert w.m._lib.smatrix_cf_recommend_filtered(w.m._h, n, off.ctypes.data_as(_lib.u64p), items.ctypes.data_as(_lib.u32p), None, None,
                                                      None, None, 0, kk, None, None, None) == -1
    valid_call_is_correct()
    assert dev_call() == 0                                            # nothing given: cf_recommend_batch_dev's bytes
    want = w.m.cf_recommend_batch(sessions, k)
    c = d_cnt.cpu().numpy().view(np.uint32)
    assert c.tobytes() == want[2].tobytes()
    for s in range(n):
        assert d_ids.cpu().numpy().view(np.uint32)[s * k: s * k + c[s]].tobytes() == want[0][s, :c[s]].tobytes()
        assert d_sc.cpu().numpy()[s * k: s * k + c[s]].tobytes() == want[1][s, :c[s]].tobytes()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_file_backed_matrix(world, tmp_path):
    w = world
    rng = np.random.default_rng(8)
    sessions = both_tiers(rng, w)
    weights = [(rng.random(len(s)) * 2).tolist() for s in sessions]
    exclude = [[b for b, _ in w.model.ranking(s)[:3]] for s in sessions]
    deny = [HUB, 300] + list(range(1000, 12000, 7))
    want = check(w, sessions, 10, weights=weights, exclude=exclude, deny=deny)
    f = SparseMatrix(str(tmp_path / "cf.smx"))
    f.cf_import_sessions(w.imported)
    got = f.cf_recommend_filtered(sessions, 10, weights=weights, exclude=exclude, deny=deny)
    f.close()
    for a, b in zip(want, got):
        assert a.tobytes() == b.tobytes()
