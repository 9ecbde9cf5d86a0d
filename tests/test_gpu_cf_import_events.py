"""GPU (-m gpu): the event import (include/smatrix_batch.h smatrix_cf_import_events / _dev; SparseMatrix.cf_import_events,
cf_forget_sessions, cf_import_events_dev).

Expected results: the ops of tests/cf_import_events_helpers.py model_ops applied to the oracle one by one (tests/
test_cf_import_events_model.py ties that model to the reference's example without a GPU).  Every comparison is exact: for each row
the oracle lists the sorted non-empty {key, value} cells of row_slots are equal and the row counts are; rowlen is never compared
(quirk Q2: with y = 0 in a row it depends on WHEN the row last grew, and a batch is one legal order)."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import IMPORT_FORWARD, IMPORT_NO_SELF, OP_DECR, OP_GET, OP_INCR, OP_SET, SparseMatrix, _lib
from tests import cf_import_events_helpers as I
from tests import cf_sim_helpers as H

pytestmark = pytest.mark.gpu

p32, p64 = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p))
SENTINEL = 0xDEADBEEF12345678


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


@pytest.fixture(scope="module")
def G():
    from tests.gpu_adapter import GpuMatrix
    return GpuMatrix


@pytest.fixture(scope="module")
def data():
    sessions = I.parity_sessions()
    assert max(len(s) for s in sessions) == 40 and sum(len(s) == 12 for s in sessions) > 5
    return sessions, I.random_amounts(sessions)


def flags_of(forward, no_self):
    return (IMPORT_FORWARD if forward else 0) | (IMPORT_NO_SELF if no_self else 0)


def same_exports(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def export_of_ops(ops):
    """what export("sorted") returns of a matrix to which the ops were added (uint32, wrapping)"""
    acc = {}
    for x, y, v in ops:
        acc[(x, y)] = (acc.get((x, y), 0) + v) & 0xFFFFFFFF
    keys = sorted(acc)
    return H.sorted_export_of((np.array([k[0] for k in keys], np.uint32), np.array([k[1] for k in keys], np.uint32),
                               np.array([acc[k] for k in keys], np.uint32)))


# ---- 1: model parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_amounts", [False, True])
@pytest.mark.parametrize("forward,no_self", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("window", [0, 1, 2, 11, 12, 50])
def test_the_matrix_is_the_models(G, oracle_mod, data, window, forward, no_self, with_amounts):
    sessions, amounts = data
    amounts = amounts if with_amounts else None
    ops = I.model_ops(sessions, amounts, window, flags_of(forward, no_self))
    g, o = G(), oracle_mod.Oracle()
    n_ops = g.m.cf_import_events(sessions, amounts=amounts, window=window, forward=forward, no_self=no_self)
    I.apply_model(o, ops)
    assert n_ops == len(ops) > 1000
    I.assert_rows_equal(g, o)
    g.close(); o.close()


# ---- 2: chunk seams -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_batch(data):
    m = SparseMatrix()
    n_ops = m.cf_import_events(data[0])
    out = (n_ops, m.export("sorted"), m.stats()["batches"])
    m.close()
    return out


@pytest.mark.parametrize("max_batch", [1, 7, 64, 0])
def test_the_result_does_not_depend_on_max_batch(data, one_batch, max_batch):
    """at the defaults every slot is an op, so the batches are exactly ceil(n_ops / max_batch): with 64 the 40-id session's 1600 ops
    alone straddle 25 of them"""
    n_want, want, b_want = one_batch
    assert b_want == 1
    m = SparseMatrix()
    n_ops = m.cf_import_events(data[0], max_batch=max_batch)
    batches = m.stats()["batches"]
    assert n_ops == n_want == sum(len(s) ** 2 for s in data[0])
    assert same_exports(m.export("sorted"), want)
    assert batches == (-(-n_ops // max_batch) if max_batch else 1)
    assert max_batch != 64 or batches >= 25
    m.close()


@pytest.mark.parametrize("max_batch", [1, 7, 64])
def test_chunks_that_compact_to_fewer_ops_or_to_none(data, max_batch):
    """window 1, FORWARD, amounts with zeros: most chunks hold fewer ops than slots, and with max_batch 1 a chunk whose slot is no op
    is no batch at all"""
    sessions, amounts = data[0][:80] + data[0][-1:], data[1][:80] + data[1][-1:]
    kw = dict(amounts=amounts, window=1, forward=True)
    a, b = SparseMatrix(), SparseMatrix()
    n_a = a.cf_import_events(sessions, **kw)
    n_b = b.cf_import_events(sessions, max_batch=max_batch, **kw)
    slots = sum(len(s) * min(len(s), 2) for s in sessions)
    assert n_a == n_b == len(I.model_ops(sessions, amounts, 1, IMPORT_FORWARD)) < slots
    assert same_exports(a.export("sorted"), b.export("sorted"))
    assert 0 < b.stats()["batches"] <= -(-slots // max_batch)
    assert max_batch != 1 or b.stats()["batches"] == n_b
    a.close(); b.close()


# ---- 3: the defaults are the old call -----------------------------------------------------------------------------------------------
def test_the_defaults_apply_the_old_calls_ops(data, one_batch):
    m = SparseMatrix()
    m.cf_import_sessions(data[0])
    assert same_exports(m.export("sorted"), one_batch[1])
    assert one_batch[0] == sum(len(s) ** 2 for s in data[0])
    m.close()


# ---- 4: forget ----------------------------------------------------------------------------------------------------------------------
def test_forgetting_sessions_takes_them_out_exactly(data):
    sessions, amounts = data
    A, wA, B, wB = sessions[:150], amounts[:150], sessions[150:], amounts[150:]
    kw = dict(window=3, no_self=True)
    ops_a, ops_b = I.model_ops(A, wA, 3, IMPORT_NO_SELF), I.model_ops(B, wB, 3, IMPORT_NO_SELF)
    only_a, both = SparseMatrix(), SparseMatrix()
    only_a.cf_import_events(A, amounts=wA, **kw)
    assert both.cf_import_events(A, amounts=wA, **kw) == len(ops_a)
    assert both.cf_import_events(B, amounts=wB, **kw) == len(ops_b)
    assert both.cf_forget_sessions(B, amounts=wB, max_batch=97, **kw) == len(ops_b)     # (in batches that cut sessions)
    cells_a, cells_b = {(x, y) for x, y, _ in ops_a}, {(x, y) for x, y, _ in ops_b}
    union = sorted(cells_a | cells_b)
    x, y = np.array([c[0] for c in union], np.uint32), np.array([c[1] for c in union], np.uint32)
    assert both.get_batch(x, y).tolist() == only_a.get_batch(x, y).tolist()
    # the cells only B touched are there, dead
    rows, row_ptr, pairs = both.export("sorted")
    have = {(int(r), int(c)): int(v) for i, r in enumerate(rows) for c, v in pairs[int(row_ptr[i]):int(row_ptr[i + 1])]}
    only_b = {c for c in cells_b - cells_a if c[1] != 0}                  # (a head cell at 0 is the empty slot, quirk Q3)
    assert len(only_b) > 100 and all(have.get(c, None) == 0 for c in only_b)
    pa, pb = only_a.pruned(1), both.pruned(1)
    assert same_exports(pa.export("sorted"), pb.export("sorted"))
    for m in (pa, pb, only_a, both):
        m.close()


def test_forgetting_what_was_never_imported_wraps(data):
    sessions, amounts = data[0][:40], data[1][:40]
    m = SparseMatrix()
    ops = I.model_ops(sessions, amounts, 2, 0)
    assert m.cf_forget_sessions(sessions, amounts=amounts, window=2) == len(ops)
    rows, row_ptr, pairs = export_of_ops(ops)
    x = np.repeat(rows, np.diff(row_ptr.astype(np.int64)))
    got = m.get_batch(x, np.ascontiguousarray(pairs[:, 0]))
    assert got.tolist() == ((1 << 32) - pairs[:, 1].astype(np.int64)).tolist()
    m.close()


# ---- 5: the _dev flavour ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_amounts", [False, True])
def test_the_dev_flavour_on_a_stream_of_its_own(data, with_amounts):
    import torch
    sessions, amounts = data[0], (data[1] if with_amounts else None)
    host = SparseMatrix()
    n_want = host.cf_import_events(sessions, amounts=amounts, window=4, forward=True)
    want = host.export("sorted")
    host.close()
    dev = torch.device("cuda", torch.cuda.current_device())
    off = np.zeros(len(sessions) + 1, np.int64)
    np.cumsum([len(s) for s in sessions], out=off[1:])
    ids = np.concatenate([np.asarray(s, np.int64) for s in sessions]).astype(np.int32)
    qx = np.repeat(want[0], np.diff(want[1].astype(np.int64)))
    qy = np.ascontiguousarray(want[2][:, 0])
    m = SparseMatrix()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        d_off, d_ids = torch.from_numpy(off).to(dev), torch.from_numpy(ids).to(dev)
        d_amt = None if amounts is None else torch.from_numpy(np.concatenate([np.asarray(a, np.int64) for a in amounts]).astype(np.int32)).to(dev)
        d_x, d_y = torch.from_numpy(qx.view(np.int32)).to(dev), torch.from_numpy(qy.view(np.int32)).to(dev)
        d_out = torch.full((qx.size,), -1, dtype=torch.int32, device=dev)
        n_ops = m.cf_import_events_dev(OP_INCR, len(sessions), d_off.data_ptr(), d_ids.data_ptr(), None if d_amt is None else d_amt.data_ptr(),
                                       4, IMPORT_FORWARD, stream=st.cuda_stream)
        m.apply_batch_dev(OP_GET, qx.size, d_x.data_ptr(), d_y.data_ptr(), None, d_out.data_ptr(), st.cuda_stream)   # no sync in between
    st.synchronize()
    assert n_ops == n_want
    assert d_out.cpu().numpy().view(np.uint32).tolist() == want[2][:, 1].tolist()
    assert same_exports(m.export("sorted"), want)
    m.close()


# ---- 6: refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_leave_n_ops_alone():
    import torch
    m = SparseMatrix()
    m.cf_import_events([[1, 2, 3], [4, 5]])
    before = m.export("sorted")
    off, ids = np.array([0, 3, 5], np.uint64), np.array([1, 2, 3, 4, 5], np.uint32)
    bad_off = np.array([0, 3, 2], np.uint64)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_off, d_bad, d_ids = (torch.from_numpy(a.view(t)).to(dev) for a, t in ((off, np.int64), (bad_off, np.int64), (ids, np.int32)))
    torch.cuda.synchronize()

    def host(op, flags, offsets):
        n = C.c_uint64(SENTINEL)
        return m._lib.smatrix_cf_import_events(m._h, op, 2, p64(offsets), p32(ids), None, 0, flags, 0, C.byref(n)), n.value

    def on_device(op, flags, offsets):
        n = C.c_uint64(SENTINEL)
        return m._lib.smatrix_cf_import_events_dev(m._h, op, 2, offsets.data_ptr(), d_ids.data_ptr(), None, 0, flags, 0, C.byref(n), None), n.value

    for call, good, bad in ((host, off, bad_off), (on_device, d_off, d_bad)):
        assert call(OP_SET, 0, good) == (-1, SENTINEL)
        assert call(OP_GET, 0, good) == (-1, SENTINEL)
        assert call(OP_INCR, 4, good) == (-1, SENTINEL)
        assert call(OP_INCR, 0, bad) == (-1, SENTINEL)
        assert call(OP_DECR, 0, bad) == (-1, SENTINEL)
        assert same_exports(m.export("sorted"), before)
    with pytest.raises(ValueError):
        m.cf_import_events_dev(OP_INCR, 2, d_bad.data_ptr(), d_ids.data_ptr(), None, 0, 0)
    assert same_exports(m.export("sorted"), before)
    assert host(OP_INCR, 0, off) == (0, 13) and on_device(OP_DECR, 3, d_off) == (0, 5 + 3 + 1)       # and the good calls are not refused
    m.close()


def test_no_sessions_is_no_error():
    m = SparseMatrix()
    assert m.cf_import_events([]) == 0 and m.cf_import_events([[], []]) == 0 and m.cf_forget_sessions([[]], window=3) == 0
    assert m.cf_import_events([[5, 6]], amounts=[[0, 0]]) == 0
    assert m.stats()["rows"] == 0 and m.stats()["batches"] == 0
    m.close()


# ---- 7: the read path on top --------------------------------------------------------------------------------------------------------
def test_what_came_next_is_what_is_recommended(data):
    sessions = data[0]
    ops = I.model_ops(sessions, None, 2, IMPORT_FORWARD)
    m = SparseMatrix()
    assert m.cf_import_events(sessions, window=2, forward=True) == len(ops)
    export = m.export("sorted")
    assert same_exports(export, export_of_ops(ops))
    model = H.SessionModel(export)
    items = [a for a in sorted(model.row) if 2 <= sum(1 for b in model.row[a][:, 0] if b not in (0, a)) <= 64][:60]
    assert len(items) >= 40
    ids, scores, counts = m.cf_recommend_filtered([[a] for a in items], 64)
    for i, a in enumerate(items):
        want_ids, want_scores = model.session([a], 64, H.SIM_COSINE, 0.0)
        assert sorted(want_ids) == sorted(int(b) for b in model.row[a][:, 0] if b not in (0, a))     # exactly the ids of row a's cells
        assert ids[i, :counts[i]].tolist() == want_ids
        assert scores[i, :counts[i]].tobytes() == want_scores.tobytes()
    m.close()


# ---- 8: file-backed -----------------------------------------------------------------------------------------------------------------
def test_a_file_backed_matrix_keeps_what_was_imported(data, tmp_path):
    sessions, amounts = data
    kw = dict(amounts=amounts, window=5, max_batch=1000)
    mem = SparseMatrix()
    n_want = mem.cf_import_events(sessions, **kw)
    want = mem.export("sorted")
    mem.close()
    path = str(tmp_path / "events.smx")
    f = SparseMatrix(path)
    assert f.cf_import_events(sessions, **kw) == n_want
    assert same_exports(f.export("sorted"), want)
    f.close()
    f = SparseMatrix(path)
    assert same_exports(f.export("sorted"), want)
    f.close()


# ---- 9: the scalar mirror -----------------------------------------------------------------------------------------------------------
def test_scalar_calls_around_the_import_see_each_other(G, oracle_mod, data):
    sessions = data[0][:60]
    g, o = G(), oracle_mod.Oracle()
    for x, y, v in ((3, 5, 10), (3, 0, 7), (9, 9, 1)):
        assert g.incr(x, y, v) == o.incr(x, y, v)
    ops = I.model_ops(sessions, None, 2, 0)
    I.apply_model(o, ops)
    n_ops = g.m.cf_import_events(sessions, window=2)                   # the mirror holds those three cells when the call starts
    assert g.get(3, 5) == o.get(3, 5) >= 11                            # [3, 5, 3] is among the sessions
    assert n_ops == len(ops)
    for x, y in ((3, 5), (3, 0), (9, 9), (5, 3), (7, 0), (9, 0)):
        assert g.get(x, y) == o.get(x, y), (x, y)
    assert g.incr(3, 5, 1) == o.incr(3, 5, 1)
    g.m.cf_forget_sessions(sessions, window=2)
    I.apply_model(o, ops, I.OP_DECR)
    assert g.get(3, 5) == o.get(3, 5) == 11 and g.get(3, 0) == o.get(3, 0) == 7
    I.assert_rows_equal(g, o)
    g.close(); o.close()
