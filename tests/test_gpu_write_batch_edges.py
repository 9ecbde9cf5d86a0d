"""GPU (-m gpu): the kernels that WRITE the tables (kernels/ops.hpp: k_apply_agg / k_apply_agg_clu / k_set_fold and the lane-per-op
kernel below agg_min; growth.hpp; prep_bulk.hpp) at the constants of the fold and of the growth tiers, through the C ABI.

The cases are tests/write_batch_helpers.py's; tests/test_write_batch_model.py proves without a GPU that each stands where it claims
(and that the checker rejects what it must).  After EVERY batch, setup batches included:

    returns    incr / decr: per key, serialisable(before, amounts, returns, after) -- some serial order of the key's ops returns
               exactly these values (mixed amounts: no multiset comparison can say that); set: out == v
    values     get of every key named == the oracle's
    rows       row_info (size, used) exact; rowlen; cells as a set plus the probe invariant, and the slot dump BYTE for byte where
               the model file proved the case order-independent
    the path   from SMATRIX_TRACE_ROUNDS=1 and stats(): whether round 0 left ops for the round loop, the bulk path, clustered mode
               (forced at open, which also makes the hint table), rows grown, the set fold keeping its own cell addresses (set_located_by_fold)

Which of the two round-0 kernels ran (lane per op below 1024 ops, the fold from 1024 on) is the host's dispatch on n alone and has
no counter of its own for incr / decr; for set, set_located_by_fold counts exactly the batches that k_set_fold completed."""
import re

import numpy as np
import pytest

from tests import write_batch_helpers as W

pytestmark = pytest.mark.gpu

VARIANTS = ("plain", "packed", "nores", "packed_nores", "clustered")
_ROUND0 = re.compile(r"\[smatrix\] batch \d+ (?:round 0|chain)[^\n]*? deferred=(\d+)")
_BULK = re.compile(r"\[smatrix\] batch \d+ bulk path: (\d+) deferred ops grouped by row, (\d+) handed back")


@pytest.fixture
def G():
    from tests.gpu_adapter import GpuMatrix
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"
    return GpuMatrix


class Run:
    """one handle under test (and, for the variants without results, a second one that takes the plain call), the oracle, the trace"""
    def __init__(self, G, oracle_mod, capfd, monkeypatch, variant="plain", env=()):
        monkeypatch.setenv("SMATRIX_TRACE_ROUNDS", "1")
        if variant == "clustered":
            monkeypatch.setenv("SMATRIX_CLUSTERED", "1")       # (forced at open, where the hint table is made: k_apply_agg_clu from the first batch on)
            monkeypatch.setenv("SMATRIX_HINT_LG", "16")
        else:
            monkeypatch.delenv("SMATRIX_CLUSTERED", raising=False)
        for k, v in env:
            monkeypatch.setenv(k, v)
        self.variant, self.capfd = variant, capfd
        self.g, self.o = G(), oracle_mod.Oracle()
        self.g2 = G() if variant.endswith("nores") else None
        self.trace = ""

    def close(self):
        for m in (self.g, self.g2, self.o):
            if m is not None:
                m.close()

    def call(self, b):
        """the batch through the variant's entry point -> its returns (None: the variant asks for none)"""
        m = self.g.m
        if not self.variant.startswith("packed"):
            return m.apply_batch(b.op, b.x, b.y, b.v, results=not self.variant.endswith("nores"))
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        rec = torch.from_numpy(np.stack([b.x, b.y, b.v], 1).view(np.int32)).to(dev).contiguous()
        out = None if self.variant.endswith("nores") else torch.full((b.n,), 0x5EED, dtype=torch.int32, device=dev)
        m.apply_packed_dev(b.op, b.n, rec.data_ptr(), 3, out.data_ptr() if out is not None else None, None)
        torch.cuda.synchronize()
        assert (rec.cpu().numpy().view(np.uint32) == np.stack([b.x, b.y, b.v], 1)).all(), (b.name, "the records were written to")
        return None if out is None else out.cpu().numpy().view(np.uint32)

    def batch(self, b):
        g, o, tag = self.g, self.o, (self.variant, b.name)
        before = o.apply(W.OP_GET, b.x, b.y)
        self.capfd.readouterr()
        ret = self.call(b)
        err = self.capfd.readouterr().err
        self.trace += err
        want = o.apply(b.op, b.x, b.y, b.v)
        after = o.apply(W.OP_GET, b.x, b.y)
        if ret is not None and b.op == W.OP_SET:
            assert (ret == b.v).all() and (want == b.v).all(), tag
        elif ret is not None:
            W.check_returns(b.op, b.x, b.y, b.v, ret, before, after, tag)
        got = g.apply(W.OP_GET, b.x, b.y)
        bad = np.flatnonzero(got != after)
        assert bad.size == 0, (tag, "gets", bad.size, [(int(b.x[i]), int(b.y[i]), int(got[i]), int(after[i])) for i in bad[:6]])
        rows = b.rows()
        for m in (g, self.g2):
            if m is None:
                continue
            if m is self.g2:
                m.apply(b.op, b.x, b.y, b.v)                                  # the plain call, same ops: the state the variant must reach
            W.state_equal(m, o, rows, exact_layout=b.exact)
            assert m.m.rowlen_batch(np.asarray(rows, np.uint32)).tolist() == [o.rowlen(r) for r in rows], tag
        if self.g2 is not None:
            for r in rows:
                a, c = np.asarray(g.row_slots(r)), np.asarray(self.g2.row_slots(r))
                if b.exact:
                    assert a.tobytes() == c.tobytes(), (tag, r, "not the plain call's table")
                else:
                    assert np.array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], c[np.lexsort((c[:, 1], c[:, 0]))]), (tag, r)
        # the path
        mt, bulk = _ROUND0.search(err), _BULK.search(err)
        assert mt or bulk, (tag, "no round-0 line in the trace", err[-1500:])
        deferred0 = int(bulk.group(1)) if bulk else int(mt.group(1))
        if b.deferred is not None:
            assert (deferred0 > 0) == b.deferred, (tag, "round 0 deferred %d ops" % deferred0, err[-1500:])
        return ret, err

    def clustered_path_ran(self):
        assert self.g.stats()["clustered_mode"] == 1, self.trace[-1500:]


# ---- returns of the increment fold ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", W.N_INCR)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("op", (W.OP_INCR, W.OP_DECR), ids=("incr", "decr"))
def test_increment_fold_returns(G, oracle_mod, capfd, monkeypatch, op, variant, n):
    """setup; all n ops on one present cell, then on one absent key (amounts: seeded 32-bit, zeros, pairs v / 2^32 - v that bring the
    first tile's total to 0); the mixed batch (every kind of key in the first tile, a key at 0 and n - 1, one at 2047 / 2048, the
    all-ones key, a value that crosses zero, y == 0 on head cells; round 0 must defer); the same ops again (all present: nothing
    deferred).  Every table is compared byte for byte."""
    w = Run(G, oracle_mod, capfd, monkeypatch, variant)
    try:
        for b in W.incr_scenario(op, n):
            w.batch(b)
        if variant == "clustered":
            w.clustered_path_ran()
    finally:
        w.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("op", (W.OP_INCR, W.OP_DECR), ids=("incr", "decr"))
def test_increment_fold_crowded_slot(G, oracle_mod, capfd, monkeypatch, op, variant):
    """2048 distinct keys that all start on ONE slot among the last 100 of the LDS table, for the plain hash and for the clustered
    one: as a new row, then present -- the table at load exactly 1/2, l_list to its last entry, a probe chain of 2048 slots across
    4095 -> 0 --, each key twice inside a tile, each twice in two tiles, and 2049 keys (the last one spills into the next tile)"""
    w = Run(G, oracle_mod, capfd, monkeypatch, variant)
    try:
        for b in W.crowd_scenario(op):
            w.batch(b)
        if variant == "clustered":
            w.clustered_path_ran()
    finally:
        w.close()


# ---- set fold ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", W.N_SET)
@pytest.mark.parametrize("locate", ("0", "1"))
@pytest.mark.parametrize("variant", ("plain", "packed"))
def test_set_fold(G, oracle_mod, capfd, monkeypatch, variant, locate, n):
    """one key on all n ops (n = 4097: every op of three tiles); the mixed set batch -- a key whose two highest indices are 2047 and
    2048, a key absent from the row at its threshold in tile 0 (that winner is deferred) and named again in tile 1, y == 0 ops,
    row 0, the all-ones key, new rows --; the same keys again with other values.  out == v, every key holds its LAST occurrence
    (numpy; the oracle in index order agrees), tables byte for byte."""
    w = Run(G, oracle_mod, capfd, monkeypatch, variant, env=(("SMATRIX_SET_LOCATE", locate),))
    try:
        for b in W.set_scenario(n):
            by_fold0 = w.g.stats()["set_located_by_fold"]
            w.batch(b)
            if b.op != W.OP_SET:
                continue
            lx, ly, lv = W.last_wins(b.x, b.y, b.v)
            got = w.g.apply(W.OP_GET, lx, ly)
            assert (got == lv).all() and (w.o.apply(W.OP_GET, lx, ly) == lv).all(), (b.name, np.flatnonzero(got != lv)[:8].tolist())
            # k_set_fold ran and round 0 completed the batch: its own cell addresses were ranked (unless SMATRIX_SET_LOCATE=1)
            kept = w.g.stats()["set_located_by_fold"] - by_fold0
            assert kept == (1 if b.deferred is False and n >= W.AGG_MIN and locate == "0" else 0), (b.name, kept)
    finally:
        w.close()


# ---- tiers in one batch -----------------------------------------------------------------------------------------------------------------
TIER_MODES = {"scrambled": (False, "plain", ()), "clustered": (True, "clustered", ()),
              "rest_slice": (True, "clustered", (("SMATRIX_REST_SLICE", "64"),))}


@pytest.mark.parametrize("size", W.TIER_SIZES)
@pytest.mark.parametrize("mode", tuple(TIER_MODES))
def test_growth_tiers_in_one_batch(G, oracle_mod, capfd, monkeypatch, mode, size):
    """six rows built by ONE batch to used == size/2 + 1, then one batch per row: 1 new key, as many as the doubled table may still
    take, one more (a second doubling inside the batch), each once and with every new key three times (the keys that wait for the
    doubling are grouped by key: k_pend_group sees duplicates).  16384 -> 32768 cells and beyond: the row gains sub-counters.
    Clustered: dense keys 1..k under SMATRIX_CLUSTERED=1 (k_grow_move_home, k_grow_rest_lds), also with 64-cell slices.  Every key is
    at home at every size: all six tables, old cells and new, byte for byte after every batch."""
    dense, variant, env = TIER_MODES[mode]
    t = W.Tier(size, dense)
    w = Run(G, oracle_mod, capfd, monkeypatch, variant, env=env)
    try:
        w.batch(t.build)
        rows = t.build.rows()
        for c in t.cases:
            assert w.g.row_info(c.row) == (size, size // 2 + 1), c.name
        for c in t.cases:
            grown0 = w.g.stats()["rows_grown"]
            w.batch(c)
            assert w.g.row_info(c.row) == (size << c.doublings, c.used_after), (c.name, w.g.row_info(c.row))
            assert w.g.stats()["rows_grown"] - grown0 >= c.doublings, c.name
            W.state_equal(w.g, w.o, rows, exact_layout=True)
        if variant == "clustered":
            w.clustered_path_ran()
    finally:
        w.close()


@pytest.mark.parametrize("op", (W.OP_INCR, W.OP_DECR), ids=("incr", "decr"))
def test_bulk_path_row_sizes(G, oracle_mod, capfd, monkeypatch, op):
    """4096 ops into an EMPTY matrix through the bulk path (SMATRIX_BULK_MIN lowered): rows of 8, 9, 10 keys (16 -> 32 cells) and of
    256, 257, 258 (512 cells, and past the 512-cell limit of k_fix_*: handed back), every key twice with two amounts"""
    w = Run(G, oracle_mod, capfd, monkeypatch, env=(("SMATRIX_BULK_MIN", "1024"), ("SMATRIX_BULK_SHARE", "1000000000")))
    try:
        b = W.bulk_batch(op)
        _, err = w.batch(b)
        st = w.g.stats()
        mt = _BULK.search(err)
        assert st["bulk_rounds"] == 1 and mt and int(mt.group(1)) == b.n, (st["bulk_rounds"], err[-1500:])      # the whole batch was grouped by row
        back = int(mt.group(2))
        assert back > 0, "the 258-key rows outgrow the bulk path: their surplus comes back"
        assert st["bulk_ops"] == b.n - back, (st["bulk_ops"], back)                                              # (bulk_ops: what the path finished itself)
        for row, c in b.counts.items():
            assert w.g.row_info(row) == (W.rows_for(c), c), (row, c)
        w.batch(W.Batch("bulk again", op, b.x, b.y, b.v, deferred=False))
    finally:
        w.close()
