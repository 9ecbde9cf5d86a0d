"""GPU (-m gpu): the rank call (include/smatrix_batch.h smatrix_cf_rank / _dev; SparseMatrix.cf_rank, cf_rank_dev, cf_evaluate).

Expected results: tests/cf_rank_helpers.py -- a target's index in cf_sim_helpers.SessionModel.ranking over the matrix's own
export("sorted"), or RANK_NONE.  Ranks and candidate counts must be equal and the scores' BYTES must match.  The matrix is the world
of tests/test_gpu_cf_sim.py, rebuilt here; tests/test_cf_rank_model.py shows, without a GPU, that its sessions have rankings longer
than 64 with tied scores in both tiers."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import RANK_NONE, SparseMatrix, _lib, rank_metrics
from tests import cf_rank_helpers as R
from tests import cf_sim_helpers as H
from tests.test_gpu_cf_sim import LDS_SLOTS, World, flat, need

pytestmark = pytest.mark.gpu

SET, DECR = 1, 3
DP = C.POINTER(C.c_double)
p32, p64, pd = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p)), (lambda a: a.ctypes.data_as(DP))
MEASURES = [("cosine", 0.0), ("cosine", 0.1), ("jaccard", 10.0), ("lift", 0.5)]
DENY = [H.HOT, 302, H.NO_ROW_COLUMN] + list(range(50001, 50400, 5)) + list(range(70001, 90000, 3))


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


def build_world():
    m = SparseMatrix()
    ops = H.world_ops()
    m.apply_batch(SET, *ops, results=False)
    m.apply_batch(DECR, *H.dead_cells(ops), results=False)
    for b, t in H.BIG_TOTALS.items():
        m.set(b, 0, t)
    return m


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


def check(got, want, tag):
    """(ranks, scores, n_candidates) against the model's"""
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float64 and got[2].dtype == np.uint32
    assert got[2].tolist() == want[2].tolist(), (tag, "n_candidates")
    assert got[0].tolist() == want[0].tolist(), (tag, "ranks")
    assert got[1].tobytes() == want[1].tobytes(), (tag, "scores")


def bitmap(deny):
    deny_n = max(deny) + 1
    bits = np.zeros((deny_n + 31) // 32, np.uint32)
    for b in deny:
        bits[b >> 5] |= np.uint32(1 << (b & 31))
    return bits, deny_n


def rank_dev(m, sessions, targets, sim, shrink, weights=None, exclude=None, deny=None):
    """SparseMatrix.cf_rank_dev on torch tensors, on a stream of its own; the outputs start as junk"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    off, items = flat(sessions, np.uint32)
    t_off, tg = flat(targets, np.uint32)
    n = len(sessions)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)             # noqa: E731
        d_off, d_items, d_toff, d_tg = up(off, np.int64), up(items, np.int32), up(t_off, np.int64), up(tg, np.int32)
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
        d_ranks = torch.full((tg.size,), 7, dtype=torch.int32, device=dev)
        d_sc = torch.full((tg.size,), -7.5, dtype=torch.float64, device=dev)
        d_nc = torch.full((n,), 99, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()               # noqa: E731
        m.cf_rank_dev(n, d_off.data_ptr(), d_items.data_ptr(), ptr(d_w), ptr(d_exoff), ptr(d_ex), ptr(d_bits), deny_n, sim, shrink,
                      d_toff.data_ptr(), d_tg.data_ptr(), d_ranks.data_ptr(), d_sc.data_ptr(), d_nc.data_ptr(), stream=st)
    st.synchronize()
    return d_ranks.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_nc.cpu().numpy().view(np.uint32)


# ---- 1: model parity --------------------------------------------------------------------------------------------------------------
def test_the_sessions_reach_both_tiers(world):
    w = world
    assert max(need(w.m, s) for s in H.lds_sessions()) <= LDS_SLOTS
    assert all(need(w.m, s) > LDS_SLOTS for s in H.global_sessions())
    assert R.LDS_TIE_SESSION in H.lds_sessions()


@pytest.mark.parametrize("sim,shrink", MEASURES)
def test_ranks_scores_and_counts_are_the_models(world, sim, shrink):
    w = world
    sessions = H.all_sessions()
    rankings = [w.model.ranking(s, H.SIMS[sim], shrink) for s in sessions]
    targets = [R.target_list(s, r) for s, r in zip(sessions, rankings)]
    want = R.expected_all(w.model, sessions, targets, sim, shrink)
    assert (want[0][want[0] != RANK_NONE] >= 64).sum() >= 10              # ranks the recommend call cannot give
    got = w.m.cf_rank(sessions, targets, sim=sim, shrink=shrink)
    check(got, want, ("host", sim, shrink))
    check(rank_dev(w.m, sessions, targets, sim, shrink), want, ("dev", sim, shrink))
    again = w.m.cf_rank(sessions, targets, sim=sim, shrink=shrink)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))    # the same input twice gives the same bytes


# ---- 2: agreement with the serving call, no model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink", [("cosine", 0.0), ("lift", 0.5)])
@pytest.mark.parametrize("filtered", [False, True])
def test_what_the_recommend_call_returns_at_r_has_the_rank_r(world, sim, shrink, filtered):
    w = world
    rng = np.random.default_rng(8)
    sessions = H.all_sessions()
    kw = dict(sim=sim, shrink=shrink)
    if filtered:
        plain = w.m.cf_recommend_filtered(sessions, 10, **kw)
        kw.update(weights=[(rng.random(len(s)) * 4).tolist() for s in sessions],
                  exclude=[plain[0][i, :int(plain[2][i])][::3].tolist() + [0, 305] for i in range(len(sessions))], deny=DENY)
    ids, sc, cnt = w.m.cf_recommend_filtered(sessions, 64, **kw)
    assert (cnt == 64).sum() >= 5 and 0 < (cnt < 64).sum()
    targets = [ids[i, :int(cnt[i])].tolist() for i in range(len(sessions))]
    ranks, scores, ncand = w.m.cf_rank(sessions, targets, **kw)
    assert ranks.tolist() == [r for c in cnt.tolist() for r in range(c)]
    assert scores.tobytes() == np.concatenate([sc[i, :int(cnt[i])] for i in range(len(sessions))]).tobytes()
    assert (np.minimum(ncand, 64) == cnt).all() and ncand.max() > 3000


# ---- 3: filters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink", [("cosine", 0.0), ("jaccard", 10.0)])
def test_filtered_targets_have_no_rank_and_the_others_move_up_by_the_filtered_before_them(world, sim, shrink):
    w = world
    sessions = H.all_sessions()
    rankings = [w.model.ranking(s, H.SIMS[sim], shrink) for s in sessions]
    exclude = [[int(r[i][0]) for i in (0, 2, 70) if i < len(r)] + [0, 305] for r in rankings]
    asked = [R.target_list(s, r) for s, r in zip(sessions, rankings)]
    targets = [t + e[:3] + DENY[:4] for t, e in zip(asked, exclude)]
    for flavour in ("host", "dev"):
        got = (w.m.cf_rank if flavour == "host" else lambda *a, **k: rank_dev(w.m, *a, sim, shrink, **k))(
            sessions, targets, exclude=exclude, deny=DENY, **(dict(sim=sim, shrink=shrink) if flavour == "host" else {}))
        check(got, R.expected_all(w.model, sessions, targets, sim, shrink, exclude=exclude, deny=DENY), (flavour, sim, shrink))
        ranks, scores, ncand = got
        j = 0
        moved = 0
        for s, (r, t, e) in enumerate(zip(rankings, targets, exclude)):
            gone = set(e) | set(DENY)
            where = {int(b): i for i, (b, _) in enumerate(r)}
            lost = sorted(where[b] for b in gone if b in where)           # the unfiltered ranks of the candidates the filters took
            assert int(ncand[s]) == len(r) - len(lost), (flavour, s)
            for b in t:
                if b in gone or b not in where:
                    assert ranks[j] == RANK_NONE and scores[j] == 0.0, (flavour, s, b)
                else:
                    before = int(np.searchsorted(lost, where[b]))
                    assert int(ranks[j]) == where[b] - before, (flavour, s, b)
                    moved += before > 0
                j += 1
        assert j == ranks.size and moved > 20


# ---- 4: more than one batch of targets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink", [("cosine", 0.0), ("lift", 0.5)])
def test_every_candidate_as_a_target_in_shuffled_order(world, sim, shrink):
    w = world
    rng = np.random.default_rng(4)
    sessions = [R.LDS_TIE_SESSION, [H.HOT], [12], [12]]
    rankings = [w.model.ranking(s, H.SIMS[sim], shrink) for s in sessions]
    assert [len(r) for r in rankings[:1] + rankings[2:]] == [217, 200, 200] and len(rankings[1]) > 4900
    every = [rng.permutation([b for b, _ in r]).tolist() for r in rankings]
    targets = [every[0], every[1], every[2][:64], every[3][:65]]          # 4 and 79 batches, exactly one, one and a target
    want = R.expected_all(w.model, sessions, targets, sim, shrink)
    for got in (w.m.cf_rank(sessions, targets, sim=sim, shrink=shrink), rank_dev(w.m, sessions, targets, sim, shrink)):
        check(got, want, (sim, shrink))
        t_off = np.cumsum([0] + [len(t) for t in targets])
        for s in (0, 1):
            assert np.sort(got[0][t_off[s]:t_off[s + 1]]).tolist() == list(range(len(rankings[s])))
        assert got[2].tolist() == [217, len(rankings[1]), 200, 200]


# ---- 5: edges -----------------------------------------------------------------------------------------------------------------------
def test_no_sessions_empty_lists_and_sessions_without_candidates(world):
    w = world
    got = w.m.cf_rank([], [])
    assert [a.size for a in got] == [0, 0, 0]
    z64, z32 = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    assert w.m._lib.smatrix_cf_rank(w.m._h, 0, p64(z64), p32(z32), None, None, None, None, 0, 0, 0.0, p64(z64), p32(z32), p32(z32),
                                    pd(np.zeros(1)), p32(z32)) == 0
    assert w.m._lib.smatrix_cf_rank_dev(w.m._h, 0, None, None, None, None, None, None, 0, 0, 0.0, 1, 1, None, None, None, None) == 0
    sessions = [[300, 301], [], [H.HOT], [H.ABSENT], [0], [302, 303], [11]]
    rankings = [w.model.ranking(s, H.SIM_COSINE, 0.0) for s in sessions]
    targets = [R.target_list(sessions[0], rankings[0]), [300, 0, H.ABSENT], [], [310, 0], [310, H.ABSENT, 0], [], R.target_list([11], rankings[6])]
    want = R.expected_all(w.model, sessions, targets, "cosine", 0.0)
    assert want[2][[1, 3, 4]].tolist() == [0, 0, 0] and want[2][2] > 4900 and want[2][5] > 0
    for got in (w.m.cf_rank(sessions, targets), rank_dev(w.m, sessions, targets, "cosine", 0.0)):
        check(got, want, "edges")
    n_first = len(targets[0])
    assert (got[0][n_first:n_first + 8] == RANK_NONE).all() and not got[1][n_first:n_first + 8].any()


def test_the_host_flavour_owns_the_entries_between_its_first_and_last_offset(world):
    w = world
    sessions = [[300, 301, 302], [H.HOT, 303], [310]]
    rankings = [w.model.ranking(s, H.SIM_LIFT, 0.5) for s in sessions]
    targets = [R.target_list(s, r) for s, r in zip(sessions, rankings)]
    want = w.m.cf_rank(sessions, targets, sim="lift", shrink=0.5)
    check(want, R.expected_all(w.model, sessions, targets, "lift", 0.5), "plain")
    off, items = flat(sessions, np.uint32)
    t_off, tg = flat(targets, np.uint32)
    T, n = tg.size, len(sessions)
    items = np.concatenate([np.array([H.HOT, 11], np.uint32), items, np.array([12], np.uint32)])          # what lies outside is not read
    tg = np.concatenate([np.array([50000, 50001, 50002], np.uint32), tg, np.array([50003, 50004], np.uint32)])
    off, t_off = off + np.uint64(2), t_off + np.uint64(3)
    ranks, scores, ncand = np.full(T + 5, 0xabcdef, np.uint32), np.full(T + 5, -7.5), np.full(n, 99, np.uint32)
    rc = w.m._lib.smatrix_cf_rank(w.m._h, n, p64(off), p32(items), None, None, None, None, 0, H.SIM_LIFT, 0.5, p64(t_off), p32(tg), p32(ranks),
                                  pd(scores), p32(ncand))
    assert rc == 0
    assert ranks[3:3 + T].tobytes() == want[0].tobytes() and scores[3:3 + T].tobytes() == want[1].tobytes() and ncand.tobytes() == want[2].tobytes()
    assert (ranks[:3] == 0xabcdef).all() and (ranks[3 + T:] == 0xabcdef).all() and (scores[:3] == -7.5).all() and (scores[3 + T:] == -7.5).all()


# ---- 6: refusals through the raw C call ---------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(world):
    import torch
    w = world
    sessions, targets = [[300, 301, 302], [H.HOT, 303], [310]], [[303, 304], [50001], [311, 0]]
    n = len(sessions)
    off, items = flat(sessions, np.uint32)
    t_off, tg = flat(targets, np.uint32)
    T = tg.size
    sentinel = lambda: (np.full(T, 0xabcdef, np.uint32), np.full(T, -7.5), np.full(n, 99, np.uint32))       # noqa: E731
    untouched = lambda got: all(a.tobytes() == b.tobytes() for a, b in zip(got, sentinel()))                # noqa: E731

    def host(sim, shrink, weights=None, targets_ptr=True, out=None):
        out = out or sentinel()
        rc = w.m._lib.smatrix_cf_rank(w.m._h, n, p64(off), p32(items), None if weights is None else pd(weights), None, None, None, 0, sim, shrink,
                                      p64(t_off), p32(tg) if targets_ptr else None, p32(out[0]), pd(out[1]), p32(out[2]))
        return rc, out

    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)                 # noqa: E731
    d_off, d_items, d_toff, d_tg = up(off, np.int64), up(items, np.int32), up(t_off, np.int64), up(tg, np.int32)
    d_ranks = torch.full((T,), 0xabcdef, dtype=torch.int32, device=dev)
    d_sc = torch.full((T,), -7.5, dtype=torch.float64, device=dev)
    d_nc = torch.full((n,), 99, dtype=torch.int32, device=dev)

    def on_device(sim, shrink, targets_ptr=True):
        rc = w.m._lib.smatrix_cf_rank_dev(w.m._h, n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, sim, shrink, d_toff.data_ptr(),
                                          d_tg.data_ptr() if targets_ptr else None, d_ranks.data_ptr(), d_sc.data_ptr(), d_nc.data_ptr(), None)
        torch.cuda.synchronize()
        return rc, (d_ranks.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_nc.cpu().numpy().view(np.uint32))

    for sim, shrink in [(3, 0.0), (-1, 1.0), (H.SIM_LIFT, -1.0), (H.SIM_COSINE, -1.0), (H.SIM_LIFT, float("nan")), (H.SIM_JACCARD, float("inf"))]:
        for call in (host, on_device):
            rc, got = call(sim, shrink)
            assert rc == -1 and untouched(got), (call.__name__, sim, shrink)
    for bad in (-1.0, float("nan"), float("inf")):                        # a bad weight, the host flavour: before the device is touched
        weights = np.ones(items.size)
        weights[3] = bad
        rc, got = host(H.SIM_COSINE, 0.0, weights=weights)
        assert rc == -1 and untouched(got), bad
    for call in (host, on_device):                                        # NULL targets
        rc, got = call(H.SIM_COSINE, 0.0, targets_ptr=False)
        assert rc == -1 and untouched(got), call.__name__
    assert w.m._lib.smatrix_cf_rank(w.m._h, n, p64(off), p32(items), None, None, None, None, 0, 0, 0.0, None, p32(tg), None, None, None) == -1
    assert w.m._lib.smatrix_cf_rank(w.m._h, n, p64(off), p32(items), None, p64(off), None, None, 0, 0, 0.0, p64(t_off), p32(tg), None, None, None) == -1
    assert w.m._lib.smatrix_cf_rank(w.m._h, n, p64(off), p32(items), None, None, None, None, 5, 0, 0.0, p64(t_off), p32(tg), None, None, None) == -1
    want = w.m.cf_rank(sessions, targets, sim="lift")
    for call in (host, on_device):                                        # -0.0 acts as 0.0, and the sentinels are all overwritten
        rc, got = call(H.SIM_LIFT, -0.0)
        assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), call.__name__
    check(want, R.expected_all(w.model, sessions, targets, "lift", 0.0), "lift 0")


# ---- 7: the mirror ------------------------------------------------------------------------------------------------------------------
def test_a_total_set_through_the_scalar_call_scores_the_next_rank_call():
    m = build_world()
    sessions = [[11, 12], [H.HOT]]
    model = H.SessionModel(m.export("sorted"))
    b = next(c for c, _ in model.ranking(sessions[0], H.SIM_COSINE, 0.0) if model.total.get(c, 0) > 0)       # its best candidate that has a total
    targets = [[b] + R.target_list(s, model.ranking(s, H.SIM_COSINE, 0.0)) for s in sessions]
    before = m.cf_rank(sessions, targets)
    check(before, R.expected_all(model, sessions, targets, "cosine", 0.0), "before")
    m.set(b, 0, model.total[b] * 9 + 1)                                   # stays in the host mirror until a batch call writes it back
    after = m.cf_rank(sessions, targets)
    fresh = H.SessionModel(m.export("sorted"))
    assert fresh.total[b] == model.total[b] * 9 + 1
    check(after, R.expected_all(fresh, sessions, targets, "cosine", 0.0), "after")
    assert after[1][0] < before[1][0] and after[0][0] > before[0][0]      # a larger total: a smaller cosine, a later rank
    m.close()


# ---- 8: truncation serves ranks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank,shrink", [("cosine", 0.0), ("lift", 0.5)])
def test_what_a_truncated_copy_ranks_the_full_matrix_ranks_the_same(world, rank, shrink):
    w = world
    t = w.m.truncated(H.M, rank=rank, shrink=shrink)
    for a in (11, 12, 13, 17):
        ids, sc, cnt = t.cf_recommend_filtered([[a]], H.M, sim=rank, shrink=shrink)
        assert cnt[0] == H.M
        targets = [ids[0].tolist() + [0, H.ABSENT]]
        small = t.cf_rank([[a]], targets, sim=rank, shrink=shrink)
        full = w.m.cf_rank([[a]], targets, sim=rank, shrink=shrink)
        assert small[0].tolist() == list(range(H.M)) + [RANK_NONE] * 2 and small[1][:H.M].tobytes() == sc[0].tobytes()
        assert full[0].tobytes() == small[0].tobytes() and full[1].tobytes() == small[1].tobytes(), (rank, shrink, a)
        assert small[2][0] == H.M and full[2][0] > H.M
    t.close()


# ---- cf_evaluate ----------------------------------------------------------------------------------------------------------------
def test_cf_evaluate_hides_the_last_id_and_ranks_it_against_the_rest(world):
    w = world
    c12 = next(int(c) for c in w.model.row[12][:, 0] if c)                # a column of row 12
    sessions = [[10, 11, 12, 11], [300], [301, 301], [H.HOT, 301, H.HOT, 50399], [c12, 12, c12], []]
    queries, hidden = [[10, 12], [H.HOT, 301, H.HOT], [12]], [[11], [50399], [c12]]
    ranks, _, _ = w.m.cf_rank(queries, hidden, sim="jaccard", shrink=10.0)
    assert ranks.tolist() == R.expected_all(w.model, queries, hidden, "jaccard", 10.0)[0].tolist()
    got = w.m.cf_evaluate(sessions, ks=(1, 100), sim="jaccard", shrink=10.0)
    assert got == rank_metrics(ranks, (1, 100)) and got["n"] == 3 and got["found"] == 2 and ranks[0] == RANK_NONE
