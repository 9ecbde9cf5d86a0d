"""GPU (-m gpu): the item-neighbour calls (include/smatrix_batch.h smatrix_cf_neighbors_batch / _dev, smatrix_cf_topk_batch / _dev;
kernels/rows.hpp k_cf_neighbors, k_cf_topk) against the slot-order model of tests/cf_neighbors_helpers.py.

The model is fed from the matrix under test by read paths that share no code with the two kernels: the tables from row_slots (checked
once per fixture against export("table")), the totals from get_batch(ids, 0).  Every comparison is of WHOLE output arrays, byte for
byte: ids, counts, the scores' bits, and every entry no neighbour is written to -- zeros from the host flavour, the test's own
sentinel from the _dev flavour, the sentinel behind the call's last entry from both.  tests/test_cf_neighbors_model.py ties the model
to the oracle's restatement of the example and shows that the guards matrix holds every branch of the score."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix, _lib
from tests import cf_neighbors_helpers as N
from tests import cf_sim_helpers as H
from tests.cf_neighbors_helpers import JUNK_COUNT, JUNK_ID, JUNK_SCORE, STEP

pytestmark = pytest.mark.gpu

PAD = 5
DP = C.POINTER(C.c_double)
p32, p64, pd = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p)), (lambda a: a.ctypes.data_as(DP))
FLAVOURS = ("host", "dev")


@pytest.fixture(scope="module")
def G():
    from tests.gpu_adapter import GpuMatrix
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"
    return GpuMatrix


# ---- the four calls, every output starting as the sentinel ------------------------------------------------------------------------
def junk(n_out, n):
    return np.full(n_out + PAD, JUNK_ID, np.uint32), np.full(n_out + PAD, JUNK_SCORE, np.float64), np.full(n + PAD, JUNK_COUNT, np.uint32)


def on_device(arrays, stream):
    """numpy arrays -> torch tensors of the same bits on the current device, made on `stream` (None: the default stream)"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.float64): np.float64}
    with torch.cuda.stream(stream if stream is not None else torch.cuda.default_stream(dev)):
        out = [torch.from_numpy(a.view(view[a.dtype])).to(dev) for a in arrays]
    if stream is None:
        torch.cuda.synchronize()
    return out


def back(tensors, dtypes):
    return tuple(t.cpu().numpy().view(d) for t, d in zip(tensors, dtypes))


def neighbours(m, items, offsets, flavour, stream=None):
    """-> (rc, (ids, scores, counts)): offsets[n] + PAD entries, n + PAD counts"""
    items, offsets = np.ascontiguousarray(items, np.uint32), np.ascontiguousarray(offsets, np.uint64)
    n = items.size
    out = junk(int(offsets[-1]), n)
    if flavour == "host":
        rc = m._lib.smatrix_cf_neighbors_batch(m._h, n, p32(items), p64(offsets), p32(out[0]), pd(out[1]), p32(out[2]))
        return rc, out
    d = on_device((items, offsets) + out, stream)
    rc = m._lib.smatrix_cf_neighbors_batch_dev(m._h, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                               None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    return rc, back(d[2:], (np.uint32, np.float64, np.uint32))


def topk(m, items, k, flavour, stream=None, size_k=None):
    """-> (rc, (ids, scores, counts)): n * k + PAD entries, flat; size_k sizes the outputs of a call that must be refused"""
    items = np.ascontiguousarray(items, np.uint32)
    n = items.size
    out = junk(n * (k if size_k is None else size_k), n)
    if flavour == "host":
        rc = m._lib.smatrix_cf_topk_batch(m._h, n, p32(items), k, p32(out[0]), pd(out[1]), p32(out[2]))
        return rc, out
    d = on_device((items,) + out, stream)
    rc = m._lib.smatrix_cf_topk_batch_dev(m._h, n, d[0].data_ptr(), k, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                          None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    else:
        import torch
        torch.cuda.synchronize()
    return rc, back(d[1:], (np.uint32, np.float64, np.uint32))


def behind(want, n):
    """the expected arrays with the sentinels that lie behind the call's last entry and last count"""
    ids, sc, cnt = want
    return (np.concatenate([ids.ravel(), np.full(PAD, JUNK_ID, np.uint32)]), np.concatenate([sc.ravel(), np.full(PAD, JUNK_SCORE)]),
            np.concatenate([cnt, np.full(PAD, JUNK_COUNT, np.uint32)]))


def fills(flavour):
    return (0, 0.0) if flavour == "host" else (JUNK_ID, JUNK_SCORE)


def offsets_of(caps, first=0):
    off = np.full(len(caps) + 1, first, np.uint64)
    off[1:] += np.cumsum(np.asarray(caps, np.uint64), dtype=np.uint64)
    return off


def check_neighbours(m, model, items, caps, tag, first=0, stream=None, flavours=FLAVOURS):
    off = offsets_of(caps, first)
    got = {}
    for flavour in flavours:
        rc, got[flavour] = neighbours(m, items, off, flavour, stream if flavour == "dev" else None)
        assert rc == 0, (tag, flavour)
        N.assert_same(got[flavour], behind(N.expected_neighbours(model, items, off, *fills(flavour)), len(items)), (tag, "neighbours", flavour))
    return got


def check_topk(m, model, items, k, tag, stream=None, flavours=FLAVOURS):
    got = {}
    for flavour in flavours:
        rc, got[flavour] = topk(m, items, k, flavour, stream if flavour == "dev" else None)
        assert rc == 0, (tag, flavour, k)
        N.assert_same(got[flavour], behind(N.expected_topk(model, items, k, *fills(flavour)), len(items)), (tag, "topk", k, flavour))
    return got


def check_all(m, model, items, ks, tag):
    """both calls in both flavours: every item's whole list (cap = entries + 1), and the k best for every k"""
    check_neighbours(m, model, items, [model.entries(a) + 1 for a in items], tag)
    for k in ks:
        check_topk(m, model, items, k, tag)


class Case:
    pass


# ---- a: the sim world -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(G):
    from tests.test_gpu_cf_rank import build_world
    w = Case()
    w.m = build_world()
    w.model = N.matrix_model(w.m)
    w.rows = N.table_export_agrees(w.m, w.model)
    yield w
    w.m.close()


def test_the_sim_world_in_slot_order(world):
    w = world
    pool_without_row = int(H.POOL[-1])
    assert w.m.row_info(pool_without_row) is None and w.m.row_info(H.NO_ROW_COLUMN) is None and w.m.row_info(H.ABSENT) is None
    items = w.rows.tolist() + [0, H.ABSENT, H.NO_ROW_COLUMN, pool_without_row, 12, 12, 12]
    assert {15, 16, 7, 13, int(H.POOL[0]), int(H.SMALL[0])} <= set(items)
    # what the batch holds: dead cells, rows whose scores are all 0, a column without a row, a row of more than 250 steps, a lone head
    c = w.model.candidates(15)
    dead = (c.val == 0) & (c.id != 0)
    assert dead.sum() == H.DEAD and not c.score[dead].any() and c.score[~dead].any()
    for a in (H.NO_HEAD_ROW, H.NO_HEAD_ITEM):
        c = w.model.candidates(a)
        assert len(c) >= 12 and c.ta == 0 and not c.score.any(), a
    scored = 0
    for a in H.SMALL.tolist():
        c = w.model.candidates(a)
        at = c.id.tolist().index(H.NO_ROW_COLUMN)
        assert c.tb[at] == 1 and c.den[at] == np.sqrt(np.float64(c.ta)), a
        scored += c.score[at] > 0.0
    assert scored >= 3
    assert w.model.candidates(H.HOT).size // STEP > 250 and w.model.entries(H.HOT) > 4900
    c = w.model.candidates(int(H.POOL[0]))
    assert len(c) == 1 and c.id[0] == 0 and c.val[0] > 0
    check_all(w.m, w.model, items, (1, 2, 10, 63, 64), "world")


# ---- b: the guards matrix, twice --------------------------------------------------------------------------------------------------
def test_guards_built_by_scalar_calls_are_the_oracles_lists_order_included(G, oracle_mod):
    g, o = N.build_scalar(G()), N.build_scalar(oracle_mod.Oracle())
    m = g.m
    for a in dict.fromkeys(N.GUARD_ITEMS):
        assert g.row_info(a) == o.row_info(a), a
        if o.row_info(a) is not None:
            assert np.asarray(g.row_slots(a)).tobytes() == o.row_slots(a).tobytes(), ("layout", a)
    items = N.GUARD_ITEMS
    full = [oracle_mod.cf_neighbors(o, a, 1 << 20) for a in items]
    caps = [wi.size + 1 for wi, _ in full]
    off = offsets_of(caps)
    for flavour in FLAVOURS:
        rc, (ids, sc, cnt) = neighbours(m, items, off, flavour)
        assert rc == 0 and cnt[:len(items)].tolist() == [wi.size for wi, _ in full]
        for i, (wi, ws) in enumerate(full):
            at = int(off[i])
            assert ids[at:at + wi.size].tolist() == wi.tolist(), (flavour, items[i])
            assert N.bits(sc[at:at + wi.size]).tolist() == N.bits(ws).tolist(), (flavour, items[i])
        for k in (1, 2, 3, 64):
            rc, (ids, sc, cnt) = topk(m, items, k, flavour)
            assert rc == 0
            for i, (wi, ws) in enumerate(full):
                order = sorted(range(wi.size), key=lambda j: (-ws[j], j))[:k]
                assert cnt[i] == len(order), (flavour, k, items[i])
                assert ids[i * k:i * k + len(order)].tolist() == wi[order].tolist(), (flavour, k, items[i])
                assert N.bits(sc[i * k:i * k + len(order)]).tolist() == N.bits(ws[order]).tolist(), (flavour, k, items[i])
    model = N.matrix_model(m)
    N.table_export_agrees(m, model)
    check_all(m, model, items, (1, 2, 3, 64), "guards, scalar")
    # the (0, total) entry of A is scored against get(0, 0) = 49
    wi, ws = full[items.index(N.A)]
    assert ws[wi.tolist().index(0)] == 25.0 / 35.0
    g.close(); o.close()


@pytest.fixture(scope="module")
def guards(G):
    c = Case()
    c.m = N.build_batch(SparseMatrix())
    c.model = N.matrix_model(c.m)
    N.table_export_agrees(c.m, c.model)
    yield c
    c.m.close()


def test_guards_built_by_one_batch_match_the_model_over_their_own_tables(guards):
    c = guards
    f = N.guard_facts(c.model)
    assert all(f.values()), [k for k, v in f.items() if not v]            # whatever the layout, every branch is still there
    assert 0 not in c.model.candidates(N.Z).id.tolist() and c.model.candidates(N.Z).ta == 0
    a = c.model.candidates(N.A)
    assert a.score[a.id.tolist().index(0)] == 25.0 / 35.0 and a.score[a.id.tolist().index(N.C)] == 1.0
    check_all(c.m, c.model, N.GUARD_ITEMS, (1, 2, 3, 64), "guards, batch")


# ---- c, d, e: ties across steps, k against the row's length, caps -----------------------------------------------------------------
# Columns TC: 300 ids with the total 9, three apart: in a table of 1024 cells (identity hash) their homes run from cell 320 round
# the table's end to cell 193, about 21 to a step.  Rows:
#   T1   (T1, c, 2) for every c of TC, head 100: 300 candidates of one score
#   T2   the same and three better pairs (values 3, 4, 5) whose homes are cells 11, 600 and 1015
#   T3   a head (cell 0) and key 31 (cell 15 of 16): candidates in the first and in the last cell only
#   L63, L64, L65   62, 63 and 64 pairs over TC and a head: 63, 64 and 65 candidates;   L1 a head alone, L2 a head and a pair
TC = (200000 + 3 * np.arange(300)).astype(np.uint32)
T1, T2, T3, L63, L64, L65, L1, L2 = 1000, 1001, 1002, 1010, 1011, 1012, 1013, 1014
BETTER = {300043: 3, 300632: 4, 300023: 5}                                # homes 11, 600, 1015 of 1024
TIE_ABSENT = 77777


def tie_ops():
    rng = np.random.default_rng(5)
    x, y, v = [TC], [np.zeros(TC.size, np.uint32)], [np.full(TC.size, 9, np.uint32)]
    for b in BETTER:
        x.append([b]); y.append([0]); v.append([9])

    def row(a, cols, vals, head):
        x.append(np.full(len(cols) + 1, a, np.uint32)); y.append(np.concatenate([cols, [0]]).astype(np.uint32))
        v.append(np.concatenate([vals, [head]]).astype(np.uint32))

    row(T1, TC, np.full(TC.size, 2), 100)
    row(T2, np.concatenate([TC, list(BETTER)]), np.concatenate([np.full(TC.size, 2), list(BETTER.values())]), 100)
    row(T3, [31], [2], 16)
    for a, n in ((L63, 62), (L64, 63), (L65, 64)):
        row(a, rng.permutation(TC)[:n], rng.integers(1, 4, n), 50)
    row(L1, [], [], 7)
    row(L2, [int(TC[7])], [2], 36)
    return tuple(np.concatenate([np.asarray(p, np.uint32) for p in part]) for part in (x, y, v))


@pytest.fixture(scope="module")
def ties(G):
    c = Case()
    c.m = SparseMatrix()
    c.m.set_batch(*tie_ops())
    c.model = N.matrix_model(c.m)
    N.table_export_agrees(c.m, c.model)
    yield c
    c.m.close()


def test_tied_scores_leave_in_slot_order_across_skipped_steps(ties):
    c, model = ties, ties.model
    t1 = model.candidates(T1)
    tied = t1.id != 0
    assert tied.sum() == 300 and np.unique(N.bits(t1.score[tied])).size == 1 and t1.score[tied][0] == 2.0 / 30.0
    assert np.unique(t1.slot[tied] // STEP).size >= 4 and tied.sum() > 64 and t1.size >= 512
    t2 = model.candidates(T2)
    assert len(t2) == 304
    where = {b: int(t2.slot[t2.id.tolist().index(b)]) for b in BETTER}
    last_step = t2.size // STEP - 1
    ks = (1, 5, 63, 64)
    assert any(s // STEP == last_step for s in where.values()), where
    for k in ks:
        skipped = model.skipped_steps(T2, k)
        assert skipped and any(s // STEP > skipped[0] for s in where.values()), (k, where, skipped)
        assert model.topk(T2, k)[0][:3].tolist()[:min(k, 3)] == [300023, 300632, 300043][:min(k, 3)]
        assert len(model.skipped_steps(T1, k)) >= 4
    t3 = model.candidates(T3)
    assert t3.slot.tolist() == [0, t3.size - 1] and t3.id.tolist() == [0, 31] and t3.score.tolist() == [0.0, 0.5]
    items = [T1, T2, T3, TIE_ABSENT, T2, T1]
    for k in ks:
        got = check_topk(c.m, model, items, k, "ties")
        ids = got["host"][0][:len(items) * k].reshape(len(items), k)
        assert ids[0].tolist() == t1.id[tied][:k].tolist()                # T1: the first k ties in slot order, the head's 0.0 last
    check_neighbours(c.m, model, items, [model.entries(a) + 1 for a in items], "ties")


def test_k_below_at_and_above_the_rows_length(ties):
    c, model = ties, ties.model
    assert [model.entries(a) for a in (L63, L64, L65, TIE_ABSENT, L1, L2)] == [63, 64, 65, 0, 1, 2]
    assert model.candidates(L1).size < STEP and model.candidates(L2).size < STEP and model.candidates(L63).size > STEP
    items = [L63, L64, L65, TIE_ABSENT, L1, L2, T3]
    for k in (64, 1, 63, 2):
        got = check_topk(c.m, model, items, k, "lengths")
        assert got["host"][2][:len(items)].tolist() == [min(k, e) for e in (63, 64, 65, 0, 1, 2, 2)]


def test_k_0_and_k_65_are_refused_and_nothing_is_written(ties):
    c = ties
    items = [L64, T1, L1]
    for k in (0, 65):
        for flavour in FLAVOURS:
            rc, got = topk(c.m, items, k, flavour, size_k=65)
            assert rc == -1, (k, flavour)
            for g, w in zip(got, junk(len(items) * 65, len(items))):
                assert g.tobytes() == w.tobytes(), (k, flavour)


def test_caps_per_item_in_one_batch(ties):
    c, model = ties, ties.model
    t1 = model.candidates(T1)
    entries = len(t1)
    per_step = np.bincount(t1.slot // STEP, minlength=t1.size // STEP)
    assert t1.size // STEP >= 4 and per_step[0] >= 2 and per_step[2] >= 2                  # several steps; the caps below are distinct
    mid_third = int(per_step[0] + per_step[1] + per_step[2] // 2)
    assert per_step[0] + per_step[1] < mid_third < per_step[0] + per_step[1] + per_step[2]
    t1_caps = [0, 1, entries - 1, entries, entries + 1, int(per_step[0]), int(per_step[0]) + 1, int(per_step[0]) - 1, mid_third]
    items = [T2, T1, T1, TIE_ABSENT, T1, T1, T1, T3, T1, T1, T1, L65, T1, L1]
    caps = [5] + t1_caps[:2] + [4] + t1_caps[2:5] + [1] + t1_caps[5:8] + [0] + t1_caps[8:] + [3]
    assert len(caps) == len(items) and len(set(caps)) >= 10
    got = check_neighbours(c.m, model, items, caps, "caps", first=3)
    for flavour in FLAVOURS:
        assert got[flavour][2][:len(items)].tolist() == [min(cap, model.entries(a)) for a, cap in zip(items, caps)]
    assert not got["host"][0][:3].any() and (got["dev"][0][:3] == JUNK_ID).all() and (got["dev"][1][:3] == JUNK_SCORE).all()


# ---- f: a big row -----------------------------------------------------------------------------------------------------------------
BIG_ITEM = 5000


def test_a_row_with_sub_counters_and_a_bitmap_behind_its_cells_ends_at_its_size(G):
    rng = np.random.default_rng(77)
    cols = (1000000 + rng.permutation(1 << 20)[:20000]).astype(np.uint32)
    m = SparseMatrix()
    for part in (cols[:10000], cols[10000:]):                             # two batches: the row grows in between
        m.set_batch(np.full(part.size, BIG_ITEM, np.uint32), part, rng.integers(1, 6, part.size).astype(np.uint32))
    with_total = rng.permutation(cols)[:500]
    m.set_batch(np.concatenate([with_total, [BIG_ITEM]]).astype(np.uint32), np.zeros(501, np.uint32),
                np.concatenate([rng.integers(1, 400, 500), [400]]).astype(np.uint32))
    size = m.row_info(BIG_ITEM)[0]
    assert size >= 1 << 15 and size == 65536
    model = N.matrix_model(m)
    N.table_export_agrees(m, model)
    entries = model.entries(BIG_ITEM)
    assert entries == 20001
    items = [int(with_total[0]), BIG_ITEM, 0, BIG_ITEM]
    got = check_neighbours(m, model, items, [model.entries(a) + 1 for a in items], "big row")
    for flavour in FLAVOURS:
        assert got[flavour][2][:4].tolist() == [1, entries, 0, entries]
    got = check_topk(m, model, items, 64, "big row")
    allowed = set(cols.tolist()) | {0}
    for flavour in FLAVOURS:
        ids, sc, cnt = got[flavour]
        assert cnt[1] == 64 and set(ids[64:128].tolist()) <= allowed and (sc[64:128] > 0).all()        # nothing from behind the cells
    m.close()


# ---- g: more items than the grid has waves ----------------------------------------------------------------------------------------
def test_items_beyond_the_grids_65536_waves(world):
    w = world
    n, waves = 70000, 65536
    base = np.concatenate([w.rows, [0, H.ABSENT]]).astype(np.uint32)
    items = np.resize(base, waves)
    items = np.concatenate([items, items[:n - waves]])
    assert items.size == n and {0, H.ABSENT, H.HOT} <= set(items[waves:].tolist()) and (items[waves:] == items[:n - waves]).all()
    got = check_topk(w.m, w.model, items, 3, "beyond the grid")
    for flavour in FLAVOURS:
        ids, sc, cnt = got[flavour]
        assert ids[:3 * (n - waves)].tobytes() == ids[3 * waves:3 * n].tobytes() and sc[:3 * (n - waves)].tobytes() == sc[3 * waves:3 * n].tobytes()
        assert cnt[:n - waves].tobytes() == cnt[waves:n].tobytes() and cnt[waves:n].any()
    got = check_neighbours(w.m, w.model, items, np.full(n, 2), "beyond the grid")
    for flavour in FLAVOURS:
        ids, sc, cnt = got[flavour]
        assert ids[:2 * (n - waves)].tobytes() == ids[2 * waves:2 * n].tobytes() and sc[:2 * (n - waves)].tobytes() == sc[2 * waves:2 * n].tobytes()
        assert cnt[:n - waves].tobytes() == cnt[waves:n].tobytes() and (cnt[waves:n] == 2).any()


# ---- h: the mirror and a side stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_call", ["neighbours", "topk"])
def test_scalar_writes_score_in_the_next_dev_call(first_call):
    m = N.build_batch(SparseMatrix())
    before = N.matrix_model(m)
    a = before.candidates(N.A)
    assert a.score[a.id.tolist().index(N.C)] == 1.0 and a.score[a.id.tolist().index(N.B)] == 0.7
    items = [N.A, N.B, N.C, 0]
    caps = [before.entries(b) + 1 for b in items]
    m.set(N.C, 0, 36)                                                     # both stay in the host mirror until a batch call writes them back
    m.incr(N.A, N.B, 1)
    off = offsets_of(caps)
    if first_call == "neighbours":
        got = [neighbours(m, items, off, "dev"), topk(m, items, 3, "dev")]
    else:
        got = [topk(m, items, 3, "dev"), neighbours(m, items, off, "dev")][::-1]
    after = N.matrix_model(m)                                             # read only now: nothing but the _dev call has synchronised
    a = after.candidates(N.A)
    assert a.score[a.id.tolist().index(N.C)] == 0.5 and a.score[a.id.tolist().index(N.B)] == 0.8
    assert got[0][0] == 0 and got[1][0] == 0
    N.assert_same(got[0][1], behind(N.expected_neighbours(after, items, off, JUNK_ID, JUNK_SCORE), 4), ("mirror", "neighbours", first_call))
    N.assert_same(got[1][1], behind(N.expected_topk(after, items, 3, JUNK_ID, JUNK_SCORE), 4), ("mirror", "topk", first_call))
    at = int(off[0]) + a.id.tolist().index(N.C)
    assert got[0][1][0][at] == N.C and got[0][1][1][at] == 0.5
    m.close()


def test_dev_flavours_on_a_side_stream_give_the_host_flavours_bytes(guards, ties):
    import torch
    for c, items, k in ((guards, N.GUARD_ITEMS, 3), (ties, [T1, T2, T3, TIE_ABSENT, L65], 64)):
        st = torch.cuda.Stream(device=torch.device("cuda", torch.cuda.current_device()))
        caps = [c.model.entries(a) + 1 for a in items]
        got = check_neighbours(c.m, c.model, items, caps, "side stream", stream=st)
        host, dev = got["host"], got["dev"]
        off = offsets_of(caps)
        for i in range(len(items)):
            lo, hi = int(off[i]), int(off[i]) + int(host[2][i])
            assert dev[0][lo:hi].tobytes() == host[0][lo:hi].tobytes() and dev[1][lo:hi].tobytes() == host[1][lo:hi].tobytes()
        assert dev[2].tobytes() == host[2].tobytes()
        got = check_topk(c.m, c.model, items, k, "side stream", stream=st)
        host, dev = got["host"], got["dev"]
        for i in range(len(items)):
            lo, hi = i * k, i * k + int(host[2][i])
            assert dev[0][lo:hi].tobytes() == host[0][lo:hi].tobytes() and dev[1][lo:hi].tobytes() == host[1][lo:hi].tobytes()
        assert dev[2].tobytes() == host[2].tobytes()


# ---- i: file-backed ---------------------------------------------------------------------------------------------------------------
def test_a_reopened_file_backed_matrix(tmp_path):
    path = str(tmp_path / "guards.smx")
    m = N.build_batch(SparseMatrix(path))
    m.close()
    m = SparseMatrix(path)
    model = N.matrix_model(m)
    N.table_export_agrees(m, model)
    assert model.entries(N.A) >= 10 and model.entries(N.FF) >= 5 and model.entries(0) == 6 and model.candidates(N.Z).ta == 0
    a = model.candidates(N.A)
    assert a.score[a.id.tolist().index(0)] == 25.0 / 35.0
    check_all(m, model, N.GUARD_ITEMS, (1, 3, 64), "reopened")
    m.close()
