"""GPU (-m gpu): session recommendations (include/smatrix_batch.h smatrix_cf_recommend_batch / _dev,
SparseMatrix.cf_recommend_batch / cf_recommend_batch_dev).  The expected result of a session comes from the oracle's
neighbour lists (ora_cf_neighbors) of its distinct items, in session order: id 0 and the session's own items dropped, the
terms summed with Python floats from 0.0, the candidates sorted by (-score, id).  Ids, counts and the scores' BYTES must
match, in the LDS tier and in the global tier alike."""
import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix

pytestmark = pytest.mark.gpu

ABSENT = 987654321


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


class Expect:
    """the contract, restated over an oracle; neighbour lists are cached until the oracle changes (reset())"""

    def __init__(self, oracle_mod, o):
        self.O, self.o, self.nb = oracle_mod, o, {}

    def reset(self):
        self.nb = {}

    def neighbours(self, a):
        if a not in self.nb:
            wi, ws = self.O.cf_neighbors(self.o, a, 1 << 22)
            self.nb[a] = (wi.tolist(), ws.tolist())
        return self.nb[a]

    def session(self, sess, k):
        excl = set(int(a) for a in sess)
        score, done = {}, set()
        for a in (int(v) for v in sess):
            if a in done:
                continue
            done.add(a)
            for b, t in zip(*self.neighbours(a)):
                if b != 0 and b not in excl:
                    score[b] = score.get(b, 0.0) + t
        best = sorted(score.items(), key=lambda kv: (-kv[1], kv[0]))[:k]
        return [b for b, _ in best], np.array([s for _, s in best], np.float64)


def check(m, ex, sessions, k, tag=""):
    ids, sc, cnt = m.cf_recommend_batch(sessions, k)
    assert ids.shape == (len(sessions), k) and sc.shape == (len(sessions), k) and cnt.shape == (len(sessions),)
    for s, sess in enumerate(sessions):
        wi, ws = ex.session(sess, k)
        c = int(cnt[s])
        assert c == len(wi), (tag, k, s, c, len(wi))
        assert ids[s, :c].tolist() == wi, (tag, k, s)
        assert sc[s, :c].tobytes() == ws.tobytes(), (tag, k, s)
        assert not ids[s, c:].any() and not sc[s, c:].any(), (tag, k, s)       # the host flavour zero-fills
    return ids, sc, cnt


def small_sessions(rng, universe, n, extra=()):
    """lengths 0..64, duplicates, absent items, item 0"""
    out = [[], [ABSENT], [0], [0, 0], list(extra)]
    for _ in range(n):
        L = int(rng.integers(0, 65))
        s = rng.choice(universe, size=L).tolist()
        if L > 2 and rng.random() < 0.3:
            s[int(rng.integers(0, L))] = s[0]                 # a duplicate
        if L > 1 and rng.random() < 0.2:
            s[int(rng.integers(0, L))] = ABSENT
        if L > 1 and rng.random() < 0.2:
            s[int(rng.integers(0, L))] = 0
        out.append([int(v) for v in s])
    return out


def import_both(m, o, oracle_mod, sessions):
    m.cf_import_sessions(sessions)
    for s in sessions:
        oracle_mod.cf_import_preference_set(o, s)


def test_one_op_per_call(oracle_mod):
    """(a) tables built one scalar op at a time, as the example's loop does"""
    rng = np.random.default_rng(5)
    m, o = SparseMatrix(), oracle_mod.Oracle()
    for _ in range(150):
        ids = (rng.choice(60, size=int(rng.integers(2, 8)), replace=False)).tolist()
        for a in ids:
            m.incr(a, 0, 1); o.incr(a, 0, 1)
            for b in ids:
                if a != b:
                    m.incr(a, b, 1); o.incr(a, b, 1)
    ex = Expect(oracle_mod, o)
    sessions = small_sessions(rng, np.arange(0, 64), 120, extra=[3, 3, 5, 0, 7])
    for k in (1, 10, 64):
        check(m, ex, sessions, k, "scalar")
    m.close(); o.close()


def build_cf(oracle_mod, rng, perm=None, fname=None):
    """sessions of a hub item (>= 50 000 distinct neighbours), of mid-size items, small ones; item 0 in a few"""
    hub, mids = 1, np.arange(2, 102)
    sess = []
    for _ in range(2100):
        sess.append([hub] + rng.integers(1000, 201000, 30).tolist())
    for _ in range(1500):
        sess.append(rng.choice(mids, 5, replace=False).tolist() + rng.integers(1000, 201000, 10).tolist())
    for _ in range(3000):
        sess.append(rng.integers(300, 900, int(rng.integers(1, 9))).tolist())
    sess += [[0, 5, 7], [0, 300, 301, 302], [7, 7, 9]]
    if perm is not None:
        sess = [[perm(v) for v in s] for s in sess]
    m, o = SparseMatrix(fname), oracle_mod.Oracle()
    import_both(m, o, oracle_mod, sess)
    return m, o, hub, mids


def query_sessions(rng, hub, mids, perm=None):
    """small sessions (LDS tier) and big ones (global tier) in one call"""
    q = small_sessions(rng, np.arange(295, 905), 200)
    big = [[hub], [hub, 301, 302], [303, hub, hub, 0, ABSENT],
           mids[:40].tolist(), rng.choice(mids, 25).tolist() + [hub],
           rng.choice(mids, 12, replace=False).tolist() + rng.integers(300, 900, 20).tolist()]
    out = []
    for i, s in enumerate(q):
        out.append(s)
        if i % 35 == 0 and big:
            out.append(big.pop())
    out += big
    if perm is not None:
        out = [[perm(v) if v not in (0, ABSENT) else v for v in s] for s in out]
    return out


def scramble():
    def perm(v):
        v = int(v)
        return 0 if v == 0 else ((v * 2654435761) & 0xffffffff) or 1
    return perm


@pytest.mark.parametrize("ids", ["dense", "scrambled"])
def test_imported_matrix_both_tiers(oracle_mod, ids):
    """(b) built by cf_import_sessions, dense and scrambled ids; (c) sessions beyond the LDS tier in the same calls"""
    rng = np.random.default_rng(11)
    perm = scramble() if ids == "scrambled" else None
    m, o, hub, mids = build_cf(oracle_mod, rng, perm)
    P = perm or (lambda v: v)
    assert m.rowlen_batch(np.array([P(hub)], np.uint32))[0] >= 50000
    ex = Expect(oracle_mod, o)
    sessions = query_sessions(rng, hub, mids, perm)
    for k in (1, 10, 64):
        check(m, ex, sessions, k, ids)
    m.close(); o.close()


def test_single_item_equals_cf_neighbors(oracle_mod):
    """(d) a one-item session is that item's cf_neighbors_batch list minus ids 0 and the item, re-sorted by (-score, id)"""
    rng = np.random.default_rng(3)
    m, o, hub, mids = build_cf(oracle_mod, rng)
    items = np.array([hub, 0, 5, 7, 300, 301, 450, ABSENT] + mids[:10].tolist(), np.uint32)
    off, nid, nsc, ncnt = m.cf_neighbors_batch(items)
    for k in (10, 64):
        ids, sc, cnt = m.cf_recommend_batch([[int(a)] for a in items], k)
        for i, a in enumerate(items.tolist()):
            wi, ws = nid[off[i]: off[i] + ncnt[i]], nsc[off[i]: off[i] + ncnt[i]]
            keep = (wi != 0) & (wi != a)
            wi, ws = wi[keep], ws[keep]
            order = np.lexsort((wi, -ws))[:k]
            assert cnt[i] == order.size, (a, k)
            assert ids[i, :cnt[i]].tolist() == wi[order].tolist(), (a, k)
            assert sc[i, :cnt[i]].tobytes() == ws[order].tobytes(), (a, k)
    m.close(); o.close()


def test_scalar_writes_are_seen_and_dev_on_a_stream(oracle_mod):
    """(e) scalar incr calls on mirrored cells show in the next result; (f) _dev on a side stream gives the host flavour's
    bytes, twice"""
    import torch
    rng = np.random.default_rng(21)
    m, o, hub, mids = build_cf(oracle_mod, rng)
    ex = Expect(oracle_mod, o)
    sessions = query_sessions(rng, hub, mids)
    check(m, ex, sessions, 10, "before")
    for a, b, v in ((300, 301, 40), (301, 300, 40), (302, 0, 7), (450, 451, 90), (5, 0, 3), (int(mids[0]), 302, 1000)):
        for _ in range(3):
            m.incr(a, b, v); o.incr(a, b, v)
            assert m.get(a, b) == o.get(a, b)
    ex.reset()
    ids, sc, cnt = check(m, ex, sessions, 10, "after")
    # (f)
    k, n = 10, len(sessions)
    lens = np.array([len(s) for s in sessions], np.int64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    flat = np.concatenate([np.asarray(s, np.int64) for s in sessions]).astype(np.uint32).view(np.int32)
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.Stream(device=dev)
    outs = []
    with torch.cuda.stream(st):
        d_off = torch.from_numpy(off).to(dev)
        d_items = torch.from_numpy(flat.copy()).to(dev)
        for _ in range(2):
            d_ids = torch.zeros(n * k, dtype=torch.int32, device=dev)
            d_sc = torch.zeros(n * k, dtype=torch.float64, device=dev)
            d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
            m.cf_recommend_batch_dev(n, d_off.data_ptr(), d_items.data_ptr(), k, d_ids.data_ptr(), d_sc.data_ptr(),
                                     d_cnt.data_ptr(), stream=st)
            outs.append((d_ids, d_sc, d_cnt))
    st.synchronize()
    for d_ids, d_sc, d_cnt in outs:
        assert d_ids.cpu().numpy().tobytes() == ids.tobytes()
        assert d_sc.cpu().numpy().tobytes() == sc.tobytes()
        assert d_cnt.cpu().numpy().tobytes() == cnt.tobytes()
    with pytest.raises(ValueError):
        m.cf_recommend_batch(sessions, 65)
    m.close(); o.close()


def test_file_backed_reopen(oracle_mod, tmp_path):
    """(g) a file-backed matrix gives the same result before and after close and reopen"""
    rng = np.random.default_rng(8)
    fname = str(tmp_path / "cf.smx")
    m, o, hub, mids = build_cf(oracle_mod, rng, fname=fname)
    ex = Expect(oracle_mod, o)
    sessions = query_sessions(rng, hub, mids)
    first = check(m, ex, sessions, 64, "file")
    m.close()
    m = SparseMatrix(fname)
    again = m.cf_recommend_batch(sessions, 64)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    m.close(); o.close()
