"""GPU (-m gpu): the explain call (include/smatrix_batch.h smatrix_cf_explain / _dev; SparseMatrix.cf_explain, cf_explain_dev,
cf_recommend_explained).

Expected results: tests/cf_explain_helpers.py over the matrix's own export("sorted"); terms must match BYTE for byte and cc exactly.
Against the library itself: the numpy left fold of a target's terms has the bytes of the score cf_rank and cf_recommend_filtered
return for it.  The matrix is the world of tests/test_gpu_cf_rank.py, built as there; tests/test_cf_explain_model.py shows, without
a GPU, that its expected terms change under a fused denominator and that its sessions repeat ids."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import RANK_NONE, _lib, explain_table
from tests import cf_explain_helpers as E
from tests import cf_rank_helpers as R
from tests import cf_sim_helpers as H
from tests.test_gpu_cf_rank import DENY, build_world
from tests.test_gpu_cf_sim import World, flat

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
p32, p64, pd = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p)), (lambda a: a.ctypes.data_as(DP))
NEG_ZERO = int(np.float64(-0.0).view(np.uint64))
GUARD = 8                                           # guard words on either side of the _dev outputs


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
    w.sessions = H.all_sessions()
    w.targets = [R.target_list(s, w.model.ranking(s, H.SIM_COSINE, 0.0)) for s in w.sessions]
    w.weights = E.weights_for(w.sessions)
    yield w
    w.m.close()


def check(got, want, tag):
    assert got[0].dtype == np.float64 and got[1].dtype == np.uint32 and got[2].dtype == np.uint64
    assert got[2].tolist() == want[2].tolist(), (tag, "e_offsets")
    assert got[1].tolist() == want[1].tolist(), (tag, "cc")
    assert got[0].tobytes() == want[0].tobytes(), (tag, "terms")
    assert not (got[0].view(np.uint64) == NEG_ZERO).any(), (tag, "-0.0")


def explain_dev(m, sessions, targets, sim, shrink, weights=None, short=0, rc_only=False):
    """SparseMatrix.cf_explain_dev on torch tensors, on a stream of its own; the outputs start as junk between guard words;
    short: total is passed that many entries too small -> (terms, cc, e_offsets, the two whole buffers)"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    off, items = flat(sessions, np.uint32)
    t_off, tg = flat(targets, np.uint32)
    e_off = E.e_offsets_of(sessions, targets)
    total = int(e_off[-1])
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)             # noqa: E731
        d_off, d_items, d_toff, d_tg, d_eoff = up(off, np.int64), up(items, np.int32), up(t_off, np.int64), up(tg, np.int32), up(e_off, np.int64)
        d_w = None if weights is None else torch.from_numpy(flat(weights, np.float64)[1]).to(dev)
        d_terms = torch.full((total + 2 * GUARD,), -7.5, dtype=torch.float64, device=dev)
        d_cc = torch.full((total + 2 * GUARD,), 0xabcdef, dtype=torch.int32, device=dev)
        args = (len(sessions), d_off.data_ptr(), d_items.data_ptr(), None if d_w is None else d_w.data_ptr())
        back = (d_toff.data_ptr(), d_tg.data_ptr(), d_eoff.data_ptr(), total - short, d_terms.data_ptr() + 8 * GUARD, d_cc.data_ptr() + 4 * GUARD)
        if rc_only:
            rc = m._lib.smatrix_cf_explain_dev(m._h, *args, H.SIMS[sim], shrink, *back, st.cuda_stream)
            st.synchronize()
            return rc
        m.cf_explain_dev(*args, sim, shrink, *back, stream=st)
    st.synchronize()
    terms, cc = d_terms.cpu().numpy(), d_cc.cpu().numpy().view(np.uint32)
    return terms[GUARD:GUARD + total], cc[GUARD:GUARD + total], e_off, (terms, cc)


def folds(terms, e_off, s, T, L):
    """the numpy left fold of each of session s's T targets' L terms -> a list of bit patterns"""
    block = terms[int(e_off[s]):int(e_off[s + 1])].reshape(T, L)
    return [E.fold(block[j]) for j in range(T)]


# ---- 1: model parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sim,shrink", E.MEASURES)
def test_terms_and_cc_are_the_models(world, sim, shrink, weighted):
    w = world
    weights = w.weights if weighted else None
    want = E.expected(w.model, w.sessions, w.targets, sim, shrink, weights)
    assert np.count_nonzero(want[1]) > 100 and np.count_nonzero(want[0]) > 50
    got = w.m.cf_explain(w.sessions, w.targets, weights=weights, sim=sim, shrink=shrink)
    check(got, want, (sim, shrink, weighted))
    again = w.m.cf_explain(w.sessions, w.targets, weights=weights, sim=sim, shrink=shrink)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))    # the same input twice gives the same bytes


# ---- 2: the terms add up to the rank call's score ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink,filtered", [("cosine", 0.0, False), ("cosine", 0.1, False), ("jaccard", 0.5, False), ("lift", 0.5, False),
                                                 ("cosine", 0.0, True), ("lift", 0.5, True)])
def test_the_left_fold_of_a_targets_terms_has_the_bytes_of_its_score_in_cf_rank(world, sim, shrink, filtered):
    w = world
    kw = dict(sim=sim, shrink=shrink)
    if filtered:
        kw["weights"] = w.weights
    terms, cc, e_off = w.m.cf_explain(w.sessions, w.targets, **kw)
    if filtered:
        kw.update(exclude=[t[1:2] + [0, 305] for t in w.targets], deny=DENY)
    ranks, scores, _ = w.m.cf_rank(w.sessions, w.targets, **kw)
    j0 = answered = 0
    for s, (sess, tg) in enumerate(zip(w.sessions, w.targets)):
        f = folds(terms, e_off, s, len(tg), len(sess))
        for j in range(len(tg)):
            if ranks[j0 + j] != RANK_NONE:
                assert f[j] == int(scores[j0 + j].view(np.uint64)), (sim, shrink, filtered, s, tg[j])
                answered += 1
        j0 += len(tg)
    assert answered > 50                                                  # (28 sessions, most with several ranked targets left)


# ---- 3: end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink,filtered", [("cosine", 0.0, False), ("lift", 0.5, True)])
def test_recommend_explained_returns_terms_that_add_up_to_the_scores_it_returns(world, sim, shrink, filtered):
    w = world
    k = 10
    kw = dict(sim=sim, shrink=shrink)
    if filtered:
        kw.update(weights=w.weights, exclude=[t[:1] for t in w.targets], deny=DENY)
    ids, scores, counts, terms, cc, e_off = w.m.cf_recommend_explained(w.sessions, k, **kw)
    plain = w.m.cf_recommend_filtered(w.sessions, k, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((ids, scores, counts), plain))
    assert e_off.tolist() == E.e_offsets_of(w.sessions, [[0] * k] * len(w.sessions)).tolist()
    assert (counts == k).sum() >= 5 and 0 < (counts < k).sum()
    for s, sess in enumerate(w.sessions):
        f = folds(terms, e_off, s, k, len(sess))
        block_cc = cc[int(e_off[s]):int(e_off[s + 1])].reshape(k, len(sess))
        for r in range(k):
            if r < counts[s]:
                assert f[r] == int(scores[s, r].view(np.uint64)), (sim, s, r)
                assert block_cc[r].any()                                  # some item of the session holds what was recommended
            else:
                assert ids[s, r] == 0 and f[r] == 0 and not block_cc[r].any()       # an unused slot explains to zeros
    table = explain_table(w.sessions, list(ids), terms, cc, e_off, top=3)
    s = next(i for i in range(len(w.sessions)) if counts[i] == k)
    assert len(table[s]) == k and all(1 <= len(row) <= 3 and row[0][0] in w.sessions[s] for row in table[s])


# ---- 4: the _dev flavour ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim,shrink,weighted", [("cosine", 0.0, False), ("jaccard", 0.5, True), ("lift", 0.5, True)])
def test_the_dev_flavour_writes_the_host_flavours_bytes_and_nothing_else(world, sim, shrink, weighted):
    w = world
    weights = w.weights if weighted else None
    want = w.m.cf_explain(w.sessions, w.targets, weights=weights, sim=sim, shrink=shrink)
    total = int(want[2][-1])
    for short in (0, 77):
        terms, cc, e_off, (all_terms, all_cc) = explain_dev(w.m, w.sessions, w.targets, sim, shrink, weights, short=short)
        n = total - short
        assert terms[:n].tobytes() == want[0][:n].tobytes() and cc[:n].tobytes() == want[1][:n].tobytes(), (sim, short)
        for buf, junk in ((all_terms, -7.5), (all_cc, 0xabcdef)):         # the guard words, and everything from total on
            assert (buf[:GUARD] == junk).all() and (buf[GUARD + n:] == junk).all(), (sim, short)


# ---- 5: layout edges ------------------------------------------------------------------------------------------------------------------
def test_empty_lists_repeats_and_the_special_ids(world):
    w = world
    col = lambda a, dead=False: next(int(c) for c, v in w.model.row[a] if c != 0 and (v == 0) == dead)      # noqa: E731
    sessions = [[300, 301], [], [302], [303, 304, 303], [], [H.NO_HEAD_ITEM, 305], [15], [310, 0, H.ABSENT], [], [311]]
    targets = [[], [300, H.NO_ROW_COLUMN], [H.NO_ROW_COLUMN, H.NO_ROW_COLUMN, 0, H.ABSENT], [303, H.NO_ROW_COLUMN, col(303)], [],
               [col(H.NO_HEAD_ITEM), H.NO_ROW_COLUMN], [col(15, dead=True), col(15)], [H.NO_ROW_COLUMN, 311, 0], [], []]
    e_off = E.e_offsets_of(sessions, targets)
    assert e_off.tolist() == [0, 0, 0, 4, 13, 13, 17, 19, 28, 28, 28]     # runs of equal offsets: T == 0, L == 0, both
    for sim, shrink in (("cosine", 0.0), ("lift", 0.5)):
        want = E.expected(w.model, sessions, targets, sim, shrink)
        got = w.m.cf_explain(sessions, targets, sim=sim, shrink=shrink)
        check(got, want, ("host", sim))
        check(explain_dev(w.m, sessions, targets, sim, shrink)[:3], want, ("dev", sim))
    terms, cc, _ = w.m.cf_explain(sessions, targets)
    assert terms[0] == terms[1] != 0.0 and cc[0] == cc[1] != 0 and not terms[2:4].any() and not cc[2:4].any()    # a repeated target; 0, ABSENT
    tb1 = cc[0] / np.sqrt(np.float64(w.model.total[302]))                 # column 999 has no row: tb == 0 is counted as 1
    assert terms[0] == tb1
    assert cc[4] == 0 and cc[6] == 0                                      # the target 303 in session [303, 304, 303]: no row holds its own id
    assert cc[7] != 0 and cc[8] != 0 and cc[9] == 0 and terms[9] == 0.0   # ... column 999: both first positions, not the repeat
    assert cc[13] != 0 and terms[13] == 0.0 and cc[15] == 0 and cc[16] != 0           # NO_HEAD_ITEM: ta == 0 scores 0, cc is there (its row has no 999)
    assert cc[17] == 0 and terms[17] == 0.0 and cc[18] != 0 and terms[18] > 0.0       # a dead cell of row 15, a live one


def test_a_target_that_is_an_item_of_the_session_is_answered_like_any_other(world):
    w = world
    a = int(H.SMALL[0])
    b = next(int(c) for c, v in w.model.row[a] if c in H.SMALL)           # a SMALL column of row a
    sessions, targets = [[a, b]], [[b, a]]
    got = w.m.cf_explain(sessions, targets, sim="jaccard", shrink=0.5)
    check(got, E.expected(w.model, sessions, targets, "jaccard", 0.5), "item as target")
    assert got[1][0] == w.m.get(a, b) != 0 and got[0][0] > 0.0
    ranks, _, _ = w.m.cf_rank(sessions, targets, sim="jaccard", shrink=0.5)
    assert (ranks == RANK_NONE).all()                                     # the rank call does not answer it: no filter here


# ---- 6: first positions at every length ---------------------------------------------------------------------------------------------
def test_first_positions_are_exact_at_every_length(world):
    w = world
    sessions = E.long_sessions()
    targets = [E.LONG_TARGETS] * len(sessions)
    want = E.expected(w.model, sessions, targets, "cosine", 0.1)
    got = w.m.cf_explain(sessions, targets, sim="cosine", shrink=0.1)
    check(got, want, "host")
    check(explain_dev(w.m, sessions, targets, "cosine", 0.1)[:3], want, "dev")
    terms, cc, e_off = got
    for s, sess in enumerate(sessions):                                   # target 999: every first position has a cell, no later one is answered
        first = set(E.first_positions(sess))
        row = cc[int(e_off[s]):int(e_off[s]) + len(sess)]
        assert [i for i in range(len(sess)) if row[i] != 0] == sorted(first), s
    L = len(sessions[3])
    row = cc[int(e_off[3]):int(e_off[3]) + L]
    assert row[0] != 0 and row[L - 1] == 0 and row[63] != 0 and row[64] == 0 and row[8191] != 0 and row[8192] == 0


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(world):
    w = world
    sessions, targets = [[300, 301, 302], [H.HOT, 303], [310]], [[303, 304], [50001], [311, 0]]
    n = len(sessions)
    off, items = flat(sessions, np.uint32)
    t_off, tg = flat(targets, np.uint32)
    total = int(E.e_offsets_of(sessions, targets)[-1])
    sentinel = lambda: (np.full(total, -7.5), np.full(total, 0xabcdef, np.uint32))                           # noqa: E731
    untouched = lambda got: all(a.tobytes() == b.tobytes() for a, b in zip(got, sentinel()))                # noqa: E731
    before = w.m.export("sorted")

    def host(sim, shrink, weights=None, null=None):
        out = sentinel()
        a = dict(t_off=p64(t_off), tg=p32(tg), terms=pd(out[0]), cc=p32(out[1]))
        if null:
            a[null] = None
        rc = w.m._lib.smatrix_cf_explain(w.m._h, n, p64(off), p32(items), None if weights is None else pd(weights), sim, shrink, a["t_off"], a["tg"],
                                         a["terms"], a["cc"])
        return rc, out

    for sim, shrink in [(3, 0.0), (-1, 1.0), (H.SIM_LIFT, -1.0), (H.SIM_COSINE, -1.0), (H.SIM_LIFT, float("nan")), (H.SIM_JACCARD, float("inf"))]:
        rc, got = host(sim, shrink)
        assert rc == -1 and untouched(got), (sim, shrink)
        assert w.m._lib.smatrix_cf_explain_dev(w.m._h, n, 1, 1, None, sim, shrink, 1, 1, 1, total, 1, 1, None) == -1     # (before the device is touched)
    for null in ("t_off", "tg", "terms", "cc"):
        rc, got = host(H.SIM_COSINE, 0.0, null=null)
        assert rc == -1 and untouched(got), null
    assert w.m._lib.smatrix_cf_explain_dev(w.m._h, n, 1, 1, None, 0, 0.0, 1, 1, None, total, 1, 1, None) == -1           # d_e_offsets NULL
    for bad in (-1.0, float("nan"), float("inf")):                        # a bad weight, the host flavour: before the device is touched
        weights = np.ones(items.size)
        weights[3] = bad
        rc, got = host(H.SIM_COSINE, 0.0, weights=weights)
        assert rc == -1 and untouched(got), bad
        per_session = [weights[int(off[s]):int(off[s + 1])].tolist() for s in range(n)]
        with pytest.raises(ValueError):
            w.m.cf_explain(sessions, targets, weights=per_session)
        assert explain_dev(w.m, sessions, targets, "cosine", 0.0, per_session, rc_only=True) == -1           # ... _dev: found on the device
    rc, got = host(H.SIM_LIFT, -0.0)                                      # -0.0 acts as 0.0, and the sentinels are all overwritten
    want = w.m.cf_explain(sessions, targets, sim="lift")
    assert rc == 0 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert explain_dev(w.m, sessions, targets, "cosine", 0.0, rc_only=True) == 0
    after = w.m.export("sorted")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))                                    # the matrix is untouched


def test_no_sessions_and_no_entries(world):
    w = world
    got = w.m.cf_explain([], [])
    assert [a.size for a in got] == [0, 0, 1] and got[0].dtype == np.float64 and got[1].dtype == np.uint32 and got[2].tolist() == [0]
    z64, z32, zd = np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1)
    assert w.m._lib.smatrix_cf_explain(w.m._h, 0, p64(z64), p32(z32), None, 0, 0.0, p64(z64), p32(z32), pd(zd), p32(z32)) == 0
    assert w.m._lib.smatrix_cf_explain_dev(w.m._h, 0, None, None, None, 0, 0.0, 1, 1, 1, 0, 1, 1, None) == 0
    for sessions, targets in (([[300, 301], []], [[], [5, 6]]), ([[]], [[]])):      # sessions, and no entry: total == 0
        got = w.m.cf_explain(sessions, targets)
        assert got[0].size == 0 and got[1].size == 0 and got[2].tolist() == [0] * (len(sessions) + 1)
        if sum(len(t) for t in targets):                                  # (an empty torch tensor has no address, and NULL targets are a refusal)
            assert explain_dev(w.m, sessions, targets, "cosine", 0.0, rc_only=True) == 0


# ---- 8: the mirror ------------------------------------------------------------------------------------------------------------------------
def test_scalar_writes_are_seen_and_the_call_changes_nothing():
    m = build_world()
    a = int(H.SMALL[5])
    model = H.SessionModel(m.export("sorted"))
    t = next(int(c) for c, v in model.row[a] if c in H.SMALL)             # a SMALL column of row a: it has a row and a total
    sessions, targets = [[a, int(H.SMALL[6])], [H.HOT]], [[t, H.NO_ROW_COLUMN], [50001]]
    before = m.cf_explain(sessions, targets)
    check(before, E.expected(model, sessions, targets, "cosine", 0.0), "before")
    m.incr(a, t, 1)                                                       # both stay in the host mirror until a batch call writes them back
    m.set(t, 0, model.total[t] * 9 + 1)
    after = m.cf_explain(sessions, targets)
    rows = m.stats()["rows"]
    export = m.export("sorted")
    fresh = H.SessionModel(export)
    assert E.cell_of(fresh, a, t) == E.cell_of(model, a, t) + 1 and fresh.total[t] == model.total[t] * 9 + 1
    check(after, E.expected(fresh, sessions, targets, "cosine", 0.0), "after")
    assert after[1][0] == before[1][0] + 1 and after[0][0] < before[0][0]            # one more co-occurrence, a far larger total
    again = m.cf_explain(sessions, targets, weights=[[0.5, 2.0], [1.0]], sim="lift", shrink=0.5)
    assert again[1].tolist() == after[1].tolist()
    assert all(u.tobytes() == v.tobytes() for u, v in zip(export, m.export("sorted"))) and m.stats()["rows"] == rows
    m.close()
