"""GPU (-m gpu): the host flavours of the session calls read WINDOWS of the caller's arrays (include/smatrix_batch.h
smatrix_cf_recommend_batch, _filtered, _sim, smatrix_cf_rank, smatrix_cf_explain): offsets[0], ex_offsets[0] and t_offsets[0] need
not be 0, the weights lie at the sessions' offsets, and nothing outside a window is read or written.

Every list-of-lists argument is embedded in a longer array with junk on both sides, the three windows starting at different
places; the outputs must have the bytes of the SparseMatrix method on the plain lists (other tests tie those to the CPU models), and
every output element the call does not own must keep its sentinel.  The matrix is tiny: the staging does not depend on the tier.

The item-neighbour calls and the old import (smatrix_cf_neighbors_batch, smatrix_cf_topk_batch, smatrix_cf_import_sessions) stage
through the same scope and the same buffers: the second half of the file holds their host flavours against their _dev flavours,
byte for byte, calls of every kind one after the other on one scratch, and a host call right behind a _dev call on another stream."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import RANK_NONE, SparseMatrix, _lib

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
p32, p64, pd = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p)), (lambda a: a.ctypes.data_as(DP))
K, PAD = 4, 3
SIM_COSINE, SIM_JACCARD = 0, 1
QUERY = [[3, 7, 12], [], [5], [9, 2, 9, 30], [1, 40, 17, 22, 8]]          # one empty, one of length 1, one with a duplicate
WEIGHTS = [[1.0, 0.5, 0.25], [], [2.0], [0.0, 1.5, 3.0, 0.125], [1.0, 1.0, 0.75, 0.5, 0.1]]
DENY = [4, 33]
JUNK_IDS = ([6, 11, 21], [13, 14])                                        # real items: read, they would change the answers
U32_MARK, F64_MARK = 0xabcdef, -7.5


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


class Case:
    pass


@pytest.fixture(scope="module")
def case():
    c = Case()
    rng = np.random.default_rng(7)
    c.m = SparseMatrix()
    c.sessions = [rng.choice(np.arange(1, 41), size=int(rng.integers(2, 7)), replace=False).tolist() for _ in range(36)]
    c.m.cf_import_sessions(c.sessions)
    best = c.m.cf_recommend_batch(QUERY, K)[0]
    c.targets = [[int(t) for t in best[s, :3]] + [0, (q[0] if q else 5)] for s, q in enumerate(QUERY)]
    c.targets[2] = []                                                     # a session without targets
    c.exclude = [[int(best[s, 1])] if s % 2 == 0 else [] for s in range(len(QUERY))]
    c.exclude[4] += [19, 19]
    yield c
    c.m.close()


def embed(lists, before, after):
    """lists inside a longer array -> (offsets, starting at len(before); values)"""
    off = np.full(len(lists) + 1, len(before), np.uint64)
    off[1:] += np.cumsum([len(v) for v in lists], dtype=np.uint64)
    return off, np.array(list(before) + [t for v in lists for t in v] + list(after), np.uint32)


def windows(c, weights=WEIGHTS, junk_weight=9.0):
    """sessions at 3, exclusion lists at 5, targets at 2 of their arrays; the weights parallel to the items' array"""
    w = Case()
    w.off, w.items = embed(QUERY, JUNK_IDS[0], JUNK_IDS[1])
    w.ex_off, w.ex = embed(c.exclude, [1, 2, 3, 4, 5], [6])
    w.t_off, w.tg = embed(c.targets, [2, 3], [5, 7, 9])
    assert len({int(w.off[0]), int(w.ex_off[0]), int(w.t_off[0])}) == 3 and w.off[0] and w.ex_off[0] and w.t_off[0]
    flat = [t for v in weights for t in v]
    w.w = np.array([junk_weight] * len(JUNK_IDS[0]) + flat + [junk_weight] * len(JUNK_IDS[1]), np.float64)
    deny_n = max(DENY) + 1
    w.bits = np.zeros((deny_n + 31) // 32, np.uint32)
    for b in DENY:
        w.bits[b >> 5] |= np.uint32(1 << (b & 31))
    w.deny_n = deny_n
    return w


def topk_out(n):
    return np.full(n * K + PAD, U32_MARK, np.uint32), np.full(n * K + PAD, F64_MARK), np.full(n + PAD, 99, np.uint32)


def check_topk(out, want, tag):
    n = len(QUERY)
    ids, scores, counts = out
    assert ids[:n * K].tobytes() == want[0].tobytes() and scores[:n * K].tobytes() == want[1].tobytes(), tag
    assert counts[:n].tobytes() == want[2].tobytes(), tag
    assert (ids[n * K:] == U32_MARK).all() and (scores[n * K:] == F64_MARK).all() and (counts[n:] == 99).all(), tag


def raw_batch(c, w):
    out = topk_out(len(QUERY))
    rc = c.m._lib.smatrix_cf_recommend_batch(c.m._h, len(QUERY), p64(w.off), p32(w.items), K, p32(out[0]), pd(out[1]), p32(out[2]))
    return rc, out


def raw_filtered(c, w, sim=None):
    out = topk_out(len(QUERY))
    front = (c.m._h, len(QUERY), p64(w.off), p32(w.items), pd(w.w), p64(w.ex_off), p32(w.ex), p32(w.bits), w.deny_n)
    back = (K, p32(out[0]), pd(out[1]), p32(out[2]))
    if sim is None:
        return c.m._lib.smatrix_cf_recommend_filtered(*front, *back), out
    return c.m._lib.smatrix_cf_recommend_sim(*front, sim[0], sim[1], *back), out


def raw_rank(c, w):
    out = np.full(w.tg.size, U32_MARK, np.uint32), np.full(w.tg.size, F64_MARK), np.full(len(QUERY) + PAD, 99, np.uint32)
    rc = c.m._lib.smatrix_cf_rank(c.m._h, len(QUERY), p64(w.off), p32(w.items), pd(w.w), p64(w.ex_off), p32(w.ex), p32(w.bits), w.deny_n,
                                  SIM_JACCARD, 2.0, p64(w.t_off), p32(w.tg), p32(out[0]), pd(out[1]), p32(out[2]))
    return rc, out


def raw_explain(c, w):
    total = sum(len(q) * len(t) for q, t in zip(QUERY, c.targets))
    out = np.full(total + PAD, F64_MARK), np.full(total + PAD, U32_MARK, np.uint32)
    rc = c.m._lib.smatrix_cf_explain(c.m._h, len(QUERY), p64(w.off), p32(w.items), pd(w.w), SIM_JACCARD, 2.0, p64(w.t_off), p32(w.tg),
                                     pd(out[0]), p32(out[1]))
    return rc, out, total


def test_the_plain_call_reads_its_window(case):
    c = case
    rc, out = raw_batch(c, windows(c))
    assert rc == 0
    want = c.m.cf_recommend_batch(QUERY, K)
    assert want[2].tolist()[1] == 0 and want[2].max() == K               # the empty session, and full answers
    check_topk(out, want, "batch")


def test_the_filtered_and_the_sim_call_read_their_windows(case):
    c = case
    for sim, kw in ((None, {}), ((SIM_JACCARD, 2.0), {"sim": "jaccard", "shrink": 2.0}), ((SIM_COSINE, 0.0), {})):
        rc, out = raw_filtered(c, windows(c), sim)
        assert rc == 0, sim
        want = c.m.cf_recommend_filtered(QUERY, K, weights=WEIGHTS, exclude=c.exclude, deny=DENY, **kw)
        check_topk(out, want, sim)
    plain = c.m.cf_recommend_batch(QUERY, K)
    assert want[0].tobytes() != plain[0].tobytes()                        # the filters and weights were not idle


def test_the_rank_call_reads_and_writes_its_windows(case):
    c = case
    w = windows(c)
    rc, (ranks, scores, ncand) = raw_rank(c, w)
    assert rc == 0
    want = c.m.cf_rank(QUERY, c.targets, weights=WEIGHTS, exclude=c.exclude, deny=DENY, sim="jaccard", shrink=2.0)
    t0, t1, n = int(w.t_off[0]), int(w.t_off[-1]), len(QUERY)
    assert (want[0] != RANK_NONE).sum() >= 4 and (want[0] == RANK_NONE).any()
    assert ranks[t0:t1].tobytes() == want[0].tobytes() and scores[t0:t1].tobytes() == want[1].tobytes()
    assert ncand[:n].tobytes() == want[2].tobytes() and (ncand[n:] == 99).all()
    for buf, mark in ((ranks, U32_MARK), (scores, F64_MARK)):             # nothing outside [t_offsets[0], t_offsets[n])
        assert (buf[:t0] == mark).all() and (buf[t1:] == mark).all() and buf[t1:].size == 3 and t0 == 2


def test_the_explain_call_reads_its_windows(case):
    c = case
    rc, (terms, cc), total = raw_explain(c, windows(c))
    assert rc == 0
    want = c.m.cf_explain(QUERY, c.targets, weights=WEIGHTS, sim="jaccard", shrink=2.0)
    assert int(want[2][-1]) == total and np.count_nonzero(want[1]) >= 4
    assert terms[:total].tobytes() == want[0].tobytes() and cc[:total].tobytes() == want[1].tobytes()
    assert (terms[total:] == F64_MARK).all() and (cc[total:] == U32_MARK).all()


def test_a_bad_weight_counts_inside_the_window_only(case):
    c = case
    calls = (lambda w: raw_filtered(c, w), lambda w: raw_filtered(c, w, (SIM_JACCARD, 2.0)), lambda w: raw_rank(c, w),
             lambda w: raw_explain(c, w))
    good = [call(windows(c)) for call in calls]
    for i, call in enumerate(calls):
        got = call(windows(c, junk_weight=float("nan")))                  # NaN before and behind the window: never looked at
        assert got[0] == 0, i
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[1], good[i][1])), i
        for bad in (float("nan"), -1.0, float("inf")):
            weights = [list(v) for v in WEIGHTS]
            weights[4][4] = bad                                           # the window's last weight
            got = call(windows(c, weights=weights))
            assert got[0] == -1, (i, bad)
            assert not any((a != a[-1]).any() for a in got[1]), (i, bad)  # the outputs as they were: one sentinel each


def test_a_recommend_round_after_an_explain_call_gives_the_same_bytes(case):
    c = case
    w = windows(c)
    first = raw_filtered(c, w)
    assert raw_explain(c, w)[0] == 0                                      # the same scratch, the next call on it
    second = raw_filtered(c, w)
    plain = raw_batch(c, w), raw_batch(c, w)
    for a, b in (first, second), plain:
        assert a[0] == 0 and b[0] == 0 and all(u.tobytes() == v.tobytes() for u, v in zip(a[1], b[1]))


# ---- the item-neighbour calls and the old import: the host flavours against the _dev flavours --------------------------------------------
ITEMS = [3, 999, 0, 3, 17]                                                # 999 has no row, 0 is no item, 3 comes twice


def nb_caps(m):
    """rowlen + 1, 0, 1, 2 (below the row's length), rowlen"""
    rl = m.rowlen_batch(ITEMS)
    assert rl[0] > 2 and rl[1] == 0 and rl[4] > 0
    return [int(rl[0]) + 1, 0, 1, 2, int(rl[4])]


def entries(c, item):
    """the entries of an item's row: the ids it shares a session with and its total in column 0 (no session: no row)"""
    with_item = [s for s in c.sessions if item in s]
    return len({t for s in with_item for t in s}) if with_item else 0


def host_neighbors(m, first):
    """smatrix_cf_neighbors_batch with offsets[0] = first -> (rc, (ids, scores, counts) with PAD sentinels behind, offsets)"""
    off = np.full(len(ITEMS) + 1, first, np.uint64)
    off[1:] += np.cumsum(nb_caps(m), dtype=np.uint64)
    end, n = int(off[-1]), len(ITEMS)
    out = np.full(end + PAD, U32_MARK, np.uint32), np.full(end + PAD, F64_MARK), np.full(n + PAD, 99, np.uint32)
    rc = m._lib.smatrix_cf_neighbors_batch(m._h, n, p32(np.array(ITEMS, np.uint32)), p64(off), p32(out[0]), pd(out[1]), p32(out[2]))
    return rc, out, off


def dev_neighbors(m, off):
    """the _dev flavour on torch tensors, the same items and offsets; the answers start as zeros, the host flavour's contract"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    end, n = int(off[-1]), len(ITEMS)
    d_items = torch.tensor(ITEMS, dtype=torch.int32, device=dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ids = torch.zeros(max(end, 1), dtype=torch.int32, device=dev)
    d_sc = torch.zeros(max(end, 1), dtype=torch.float64, device=dev)
    d_cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m.cf_neighbors_batch_dev(n, d_items.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), None)
    torch.cuda.synchronize()
    return d_ids.cpu().numpy().view(np.uint32)[:end], d_sc.cpu().numpy()[:end], d_cnt.cpu().numpy().view(np.uint32)


def host_topk(m, items, k):
    n = len(items)
    out = np.full(n * k + PAD, U32_MARK, np.uint32), np.full(n * k + PAD, F64_MARK), np.full(n + PAD, 99, np.uint32)
    rc = m._lib.smatrix_cf_topk_batch(m._h, n, p32(np.array(items, np.uint32)), k, p32(out[0]), pd(out[1]), p32(out[2]))
    return rc, out


def dev_topk(m, items, k):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n = len(items)
    d_items = torch.tensor(items, dtype=torch.int32, device=dev)
    d_ids = torch.zeros(n * k, dtype=torch.int32, device=dev)
    d_sc = torch.zeros(n * k, dtype=torch.float64, device=dev)
    d_cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m.cf_topk_batch_dev(n, d_items.data_ptr(), k, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), None)
    torch.cuda.synchronize()
    return d_ids.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)


def check_owned(out, want, n_out, n, tag):
    """out: the host flavour's arrays with sentinels behind the owned ranges [0, n_out) and [0, n); want: the _dev flavour's"""
    ids, scores, counts = out
    assert ids[:n_out].tobytes() == want[0].tobytes() and scores[:n_out].tobytes() == want[1].tobytes(), tag
    assert counts[:n].tobytes() == want[2].tobytes(), tag
    assert (ids[n_out:] == U32_MARK).all() and (scores[n_out:] == F64_MARK).all() and (counts[n:] == 99).all(), tag
    assert ids[n_out:].size == PAD and counts[n:].size == PAD, tag


@pytest.mark.parametrize("first", [0, 2])
def test_the_neighbours_call_owns_its_output_offsets_whole(case, first):
    m = case.m
    rc, out, off = host_neighbors(m, first)
    assert rc == 0
    want = dev_neighbors(m, off)
    assert want[2].tolist() == [min(cap, entries(case, i)) for cap, i in zip(nb_caps(m), ITEMS)] and want[2][3] == 2 < want[2][0]
    check_owned(out, want, int(off[-1]), len(ITEMS), first)
    assert not out[0][:first].any() and not out[1][:first].any()          # [0, offsets[0]) is the call's too: zeros
    assert out[0][int(off[2]):int(off[3])].tolist() == [0]                # the place nothing was written to reads 0


@pytest.mark.parametrize("k", [1, 64])
def test_the_topk_call_against_its_dev_flavour(case, k):
    m = case.m
    rc, out = host_topk(m, ITEMS, k)
    assert rc == 0
    want = dev_topk(m, ITEMS, k)
    assert want[2].tolist() == [min(k, entries(case, i)) for i in ITEMS] and want[2][1] == 0 and want[2][4] == min(k, 11)
    check_owned(out, want, len(ITEMS) * k, len(ITEMS), k)
    for bad in (0, 65):                                                   # refused before anything is touched
        rc, out = host_topk(m, ITEMS, bad)
        assert rc == -1 and (out[0] == U32_MARK).all() and (out[1] == F64_MARK).all() and (out[2] == 99).all()


def same_export(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def test_the_import_call_reads_its_window():
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    lists = [[5, 9, 5], [], [7]]
    off, ids = embed(lists, JUNK_IDS[0], JUNK_IDS[1])
    assert off[0] == 3
    a, b = SparseMatrix(), SparseMatrix()
    try:
        assert a._lib.smatrix_cf_import_sessions(a._h, len(lists), p64(off), p32(ids)) == 0
        flat = [t for v in lists for t in v]
        lens = np.array([len(v) for v in lists], np.int64)
        d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(dev)
        d_op = torch.from_numpy(np.concatenate([[0], np.cumsum(lens * lens)])).to(dev)
        d_ids = torch.tensor(flat, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        b.cf_import_sessions_dev(len(lists), d_off.data_ptr(), d_ids.data_ptr(), d_op.data_ptr(), int((lens * lens).sum()), None)
        torch.cuda.synchronize()
        got, want = a.export("sorted"), b.export("sorted")
        assert want[0].tolist() == [5, 7, 9] and same_export(got, want)   # no junk id has a row
        assert a.get(5, 0) == 2 and a.get(5, 5) == 2 and a.get(5, 9) == 2 and a.get(9, 5) == 2 and a.get(7, 0) == 1
        got = a.export("sorted")
        down = np.array([3, 6, 5, 7], np.uint64)                          # offsets that decrease: refused, nothing written
        assert a._lib.smatrix_cf_import_sessions(a._h, 3, p64(down), p32(ids)) == -1
        flat_off = np.array([4, 4, 4], np.uint64)                         # no ops, and no sessions: 0, nothing written
        assert a._lib.smatrix_cf_import_sessions(a._h, 2, p64(flat_off), p32(ids)) == 0
        assert a._lib.smatrix_cf_import_sessions(a._h, 0, p64(off), p32(ids)) == 0
        assert same_export(a.export("sorted"), got)
    finally:
        a.close(); b.close()


def test_calls_of_every_kind_share_one_scratch(case):
    """a smaller call behind a larger one must not see the larger one's leftovers: every call of the sequence gives the bytes it
    gives as the first read call on a fresh handle over the same data"""
    c = case
    one = [ITEMS[4]]
    calls = (lambda m: host_topk(m, ITEMS, 64)[1],
             lambda m: m.cf_recommend_batch(QUERY, K),
             lambda m: host_neighbors(m, 0)[1],
             lambda m: m.cf_rank(QUERY, c.targets),
             lambda m: host_topk(m, one, 1)[1])
    seq = SparseMatrix()
    seq.cf_import_sessions(c.sessions)
    try:
        for i, call in enumerate(calls):
            fresh = SparseMatrix()
            try:
                fresh.cf_import_sessions(c.sessions)
                want = call(fresh)
            finally:
                fresh.close()
            got = call(seq)
            assert len(got) == len(want) and all(u.tobytes() == v.tobytes() for u, v in zip(got, want)), i
    finally:
        seq.close()


def test_a_host_call_waits_for_the_dev_call_before_it_on_another_stream(case):
    import torch
    c = case
    dev = torch.device("cuda", torch.cuda.current_device())
    n = len(QUERY)
    alone_rec = c.m.cf_recommend_batch(QUERY, K)
    alone_top = host_topk(c.m, ITEMS, 64)[1]
    off, items = embed(QUERY, [], [])
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_items = torch.from_numpy(items.view(np.int32)).to(dev)
    d_ids = torch.full((n * K,), 0x7a7a7a7a, dtype=torch.int32, device=dev)
    d_sc = torch.full((n * K,), -7.5, dtype=torch.float64, device=dev)
    d_cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    c.m.cf_recommend_batch_dev(n, d_off.data_ptr(), d_items.data_ptr(), K, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), st)
    rc, top = host_topk(c.m, ITEMS, 64)                                   # at once: no synchronisation of the test's in between
    st.synchronize()
    assert rc == 0 and all(u.tobytes() == v.tobytes() for u, v in zip(top, alone_top))
    cnt = d_cnt.cpu().numpy().view(np.uint32)
    assert cnt.tobytes() == alone_rec[2].tobytes()
    used = np.arange(K)[None, :] < cnt[:, None]                           # the _dev flavour writes counts[s] entries a session
    assert d_ids.cpu().numpy().view(np.uint32).reshape(n, K)[used].tobytes() == alone_rec[0][used].tobytes()
    assert d_sc.cpu().numpy().reshape(n, K)[used].tobytes() == alone_rec[1][used].tobytes()
