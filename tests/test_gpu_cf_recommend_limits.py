"""GPU (-m gpu): session recommendations at their limits -- calls on different streams back to back (the per-matrix scratch is
ordered across them), sessions that repeat a hot item many times (the bound counts an item once), and a query whose
global-tier tables exceed one group (REC_GROUP_SLOTS, 2^25 slots) and whose (position, session) plan is cut into blocks
(REC_PLAN_MAX, 2^24).  Expected results as in test_gpu_cf_recommend.py: the oracle's neighbour lists, exact bytes."""
import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix
from tests.test_gpu_cf_recommend import ABSENT, Expect, build_cf, check, query_sessions

pytestmark = pytest.mark.gpu

LDS_SLOTS, GL_MIN, GROUP_SLOTS, PLAN_MAX = 4096, 8192, 1 << 25, 1 << 24     # kernels/recommend.hpp, smx_recommend.inc


class CachedExpect(Expect):
    """the same contract; the result of a session that repeats an earlier one is taken from a cache"""

    def __init__(self, oracle_mod, o):
        super().__init__(oracle_mod, o)
        self.memo = {}

    def session(self, sess, k):
        key = (tuple(int(v) for v in sess), k)
        if key not in self.memo:
            self.memo[key] = super().session(sess, k)
        return self.memo[key]


def table_slots(m, sess, sizes):
    """the global-tier table of a session as k_rec_bound sizes it (0: the LDS tier or no candidate); sizes: a row-size cache"""
    bound = 0
    for a in dict.fromkeys(int(v) for v in sess):
        if a not in sizes:
            info = m.row_info(a)
            sizes[a] = info[0] if info else 0
        bound += sizes[a]
    need = bound + len(sess)
    if bound == 0 or need <= LDS_SLOTS:
        return 0
    t = GL_MIN
    while t < need:
        t *= 2
    return t


def test_calls_on_two_streams_back_to_back(oracle_mod):
    """a call on stream A, at once a smaller one on stream B, no synchronisation in between: both give the host flavour's bytes"""
    import torch
    rng = np.random.default_rng(41)
    m, o, hub, mids = build_cf(oracle_mod, rng)
    qa = query_sessions(rng, hub, mids) * 3
    qb = query_sessions(rng, hub, mids)[:150]
    k = 10
    want = [m.cf_recommend_batch(q, k) for q in (qa, qb)]
    dev = torch.device("cuda", torch.cuda.current_device())
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    bufs = []
    for q, st in zip((qa, qb), streams):
        off = np.zeros(len(q) + 1, np.int64)
        np.cumsum([len(s) for s in q], out=off[1:])
        flat = np.concatenate([np.asarray(s, np.int64) for s in q]).astype(np.uint32).view(np.int32)
        with torch.cuda.stream(st):
            bufs.append((len(q), torch.from_numpy(off).to(dev), torch.from_numpy(flat.copy()).to(dev),
                         torch.zeros(len(q) * k, dtype=torch.int32, device=dev), torch.zeros(len(q) * k, dtype=torch.float64, device=dev),
                         torch.zeros(len(q), dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    for rnd in range(2):
        for (n, d_off, d_items, d_ids, d_sc, d_cnt), st in zip(bufs, streams):
            d_ids.zero_(); d_sc.zero_(); d_cnt.zero_()
        torch.cuda.synchronize()
        for (n, d_off, d_items, d_ids, d_sc, d_cnt), st in zip(bufs, streams):
            m.cf_recommend_batch_dev(n, d_off.data_ptr(), d_items.data_ptr(), k, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(),
                                     stream=st)
        for st in streams:
            st.synchronize()
        for (ids, sc, cnt), (n, d_off, d_items, d_ids, d_sc, d_cnt) in zip(want, bufs):
            assert d_ids.cpu().numpy().tobytes() == ids.tobytes(), rnd
            assert d_sc.cpu().numpy().tobytes() == sc.tobytes(), rnd
            assert d_cnt.cpu().numpy().tobytes() == cnt.tobytes(), rnd
    m.close(); o.close()


def test_a_hot_item_repeated(oracle_mod):
    """the hub (>= 50 000 neighbours) 1025 times in one session (exact duplicate detection) and 40 000 times (longer than
    REC_DEDUP_MAX: the bound is cut to the matrix's cells); the results are those of the hub once"""
    rng = np.random.default_rng(43)
    m, o, hub, mids = build_cf(oracle_mod, rng)
    ex = CachedExpect(oracle_mod, o)
    sessions = [[hub] * 1025 + [301], [hub], [302, 303], [hub] * 40000, [int(mids[0])] * 3000 + [hub, 0, ABSENT] * 5,
                [hub] + [301] * 9000]
    for k in (10, 64):
        ids, sc, cnt = check(m, ex, sessions, k, "repeated")
        assert ids[3].tobytes() == ids[1].tobytes() and sc[3].tobytes() == sc[1].tobytes()
    m.close(); o.close()


def test_global_tier_in_groups_and_plan_blocks(oracle_mod):
    """4 400 global-tier sessions (tables of more than 2^25 slots in all: several groups) and one of 4 001 items (4 401 sessions x
    4 001 positions > 2^24: the plan in blocks), small sessions in between"""
    rng = np.random.default_rng(47)
    m, o, hub, mids = build_cf(oracle_mod, rng)
    ex = CachedExpect(oracle_mod, o)
    combos = [rng.choice(mids, 5, replace=False).tolist() for _ in range(40)]
    small = [[int(v) for v in rng.integers(300, 900, int(rng.integers(1, 30)))] for _ in range(40)]
    sessions = []
    for i in range(4400):
        sessions.append(combos[i % len(combos)])
        if i % 100 == 0:
            sessions.append(small[(i // 100) % len(small)])
    sessions.insert(1234, [int(v) for v in mids[:3]] + rng.integers(300, 900, 3998).tolist())
    sizes = {}
    slots = [table_slots(m, s, sizes) for s in sessions]
    n_big = sum(1 for t in slots if t)
    assert sum(slots) > GROUP_SLOTS, sum(slots)
    assert n_big * max(len(s) for s, t in zip(sessions, slots) if t) > PLAN_MAX
    for k in (10, 64):
        check(m, ex, sessions, k, "groups")
    m.close(); o.close()
