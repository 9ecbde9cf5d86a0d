"""GPU (-m gpu): the code that answers an op whose key does NOT sit at its home cell (kernels/ops.hpp: the lane's budget in apply_row,
k_get_clu, hint_find / hint_way / hint_put, coop_probe's window and bitmap phases; the at-home bitmap's writers in ops.hpp, growth.hpp
and the loader), next to the oracle, at the exact distances where each phase begins and ends.

The rows are tests/probe_helpers.py's; tests/test_probe_model.py proves without a GPU that every distance class is there.  Every
comparison is exact and over every key named: returns, gets, row_info, and the slot dump byte for byte wherever the table was built
one key per row and call.  Which kernel ran is selected by the environment (smx_runtime.hip launch_apply) and asserted from stats()
and the round trace."""
import re

import numpy as np
import pytest

from tests import probe_helpers as P
from tests.write_batch_helpers import state_equal

pytestmark = pytest.mark.gpu

_ROUND0 = re.compile(r"\[smatrix\] batch \d+ (?:round 0|chain)[^\n]*? deferred=(\d+)")
_PASS = re.compile(r"pass in front of prep \(it took (\d+) ops|\(the pass in front of prep took (\d+)\)")
_REBUILT = re.compile(r"at-home bitmaps of (\d+) rows rebuilt")


@pytest.fixture
def G():
    from tests.gpu_adapter import GpuMatrix
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"
    return GpuMatrix


class World:
    """one handle under test next to the oracle.  mode: plain (SMATRIX_CLUSTERED=0: k_apply<OP>, no hint table, windows only),
    clustered (=1 from open: hint table, bitmaps, k_get_clu, the retry kernels), auto (the data decides)"""
    def __init__(self, G, oracle_mod, capfd, monkeypatch, mode, env=(), cs=None, fname=None):
        monkeypatch.setenv("SMATRIX_TRACE_ROUNDS", "1")
        for k in ("SMATRIX_CLUSTERED", "SMATRIX_HINT_LG", "SMATRIX_FAR_JOIN", "SMATRIX_BULK_MIN", "SMATRIX_REST_SLICE", "SMATRIX_SCALAR_CACHE"):
            monkeypatch.delenv(k, raising=False)
        if mode != "auto":
            monkeypatch.setenv("SMATRIX_CLUSTERED", "1" if mode == "clustered" else "0")
        if mode == "clustered":
            monkeypatch.setenv("SMATRIX_HINT_LG", "16")
        for k, v in env:
            monkeypatch.setenv(k, v)
        self.G, self.mode, self.capfd, self.fname = G, mode, capfd, fname
        self.cs = P.cases() if cs is None else cs
        self.rows = [c.row for c in self.cs]
        self.g, self.o = G(fname), oracle_mod.Oracle()
        self.trace = ""

    def close(self):
        for m in (self.g, self.o):
            if m is not None:
                m.close()
        self.trace += self.capfd.readouterr().err

    def reopen(self):
        """close the handle (the flush barrier) and open the file again: the loader's tables, an all-zero bitmap, clustered_sync"""
        self.g.close()
        self.g = self.G(self.fname)

    def last_trace(self):
        err = self.capfd.readouterr().err
        self.trace += err
        return err

    def apply(self, op, x, y, v=None, via="batch", tag=""):
        """the same call on both sides; the returns are compared op by op -> (returns, this call's trace)"""
        x, y = P.u32(x), P.u32(y)
        v = np.zeros_like(x) if v is None else P.u32(v)
        self.last_trace()
        if via == "batch":
            got = self.g.m.apply_batch(op, x, y, v)
        elif via == "scalar":
            f = (lambda a, b, c: self.g.get(a, b), self.g.set, self.g.incr, self.g.decr)[op]
            got = np.array([f(int(a), int(b), int(c)) for a, b, c in zip(x, y, v)], np.uint32)
        else:
            got = self.packed(op, x, y, v)
        err = self.last_trace()
        want = self.o.apply(op, x, y, v)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (tag, self.mode, via, "op %d: %d of %d differ" % (op, bad.size, x.size),
                               [(int(x[i]), int(y[i]), int(got[i]), int(want[i])) for i in bad[:8]], err[-800:])
        return got, err

    def packed(self, op, x, y, v):
        """{x, y} records (gets, in_stride == 2) / {x, y, v} records in one device array"""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        cols = [x, y] if op == P.OP_GET else [x, y, v]
        rec = torch.from_numpy(np.stack(cols, 1).view(np.int32)).to(dev).contiguous()
        out = torch.full((x.size,), 0x5EED, dtype=torch.int32, device=dev)
        self.g.m.apply_packed_dev(op, x.size, rec.data_ptr(), len(cols), out.data_ptr(), None)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32)

    def build(self, how="steps"):
        steps = P.steps(self.cs)
        for op, x, y, v in steps:
            self.o.apply(op, x, y, v)
        self.last_trace()
        for op, x, y, v in (steps if how == "steps" else P.steps(self.cs, how)):
            self.g.m.apply_batch(op, x, y, v, results=False)
        err = self.last_trace()
        self.state(exact=how == "steps", tag="build " + how)
        return err

    def state(self, exact=True, tag=""):
        try:
            state_equal(self.g, self.o, self.rows, exact_layout=exact)
        except AssertionError as e:
            raise AssertionError((tag, self.mode) + e.args) from None
        assert self.g.m.rowlen_batch(np.asarray(self.rows, np.uint32)).tolist() == [self.o.rowlen(r) for r in self.rows], tag

    def gets(self, via="batch", tag=""):
        x, y = P.queries(self.cs)
        return self.apply(P.OP_GET, x, y, via=via, tag=tag or "gets")

    def far_exist(self):
        """the precondition of every bitmap case, on the handle's OWN tables: keys behind the first window on rows with a bitmap
        (the rows whose pile lies behind its run in slot order: a doubling leaves those keys displaced)"""
        for c in self.cs:
            if c.size >= 1 << P.HOME_LG and not c.wrap:
                _, _, d = P.distances(self.g.row_slots(c.row))
                assert d.max() > P.first_bitmap_distance(True), c.name

    def absent_inserts(self, via="batch", pad=0, exact=True, count=None, tag="", ops=(P.OP_INCR, P.OP_SET), check=None):
        """per class: ONE new key per row and call (incr and set in turn), padded to `pad` ops with hits on the runs' home cells that
        change nothing (incr by 0, set to the value held); every key must land in the oracle's slot.  check(k, op, x, y, trace): the
        caller's look at the call's trace"""
        traces = []
        for k in (range(P.N_ABSENT) if count is None else P.ABSENT_PICK[:count]):
            x, y, ends = P.absent_batch(self.o, k, self.cs)
            op = ops[k % len(ops)]
            v = P.value_of(y)
            xx, yy, vv = padded(self.cs, x, y, v, pad, op)
            _, err = self.apply(op, xx, yy, vv, via=via, tag=(tag, "absent class", k))
            traces.append(err)
            if check:
                check(k, op, x, y, err)
            if exact:
                for r, key, e in zip(x.tolist(), y.tolist(), ends):
                    held = int(P.value_of(key)) if op != P.OP_DECR else -int(P.value_of(key)) & 0xFFFFFFFF
                    assert np.asarray(self.g.row_slots(r))[e[0]].tolist() == [key, held], (tag, k, r, key, e)
            self.state(exact=exact, tag=(tag, "absent class", k))
        return traces


# ---- 1. gets, every class, every read kernel -------------------------------------------------------------------------------------------
GET_SETTINGS = {"plain": ("plain", "batch", ()), "clustered": ("clustered", "batch", ()), "packed": ("clustered", "packed", ()),
                "packed plain": ("plain", "packed", ()), "scalar": ("clustered", "scalar", (("SMATRIX_SCALAR_CACHE", "0"),)),
                "scalar plain": ("plain", "scalar", (("SMATRIX_SCALAR_CACHE", "0"),))}


@pytest.mark.parametrize("setting", tuple(GET_SETTINGS))
def test_gets_at_every_class(G, oracle_mod, capfd, monkeypatch, setting):
    """present keys at every distance class, absent keys whose probe ends on a free cell at every class, (row, 0), rows that do not
    exist: k_apply<GET> (budget 48, windows only), k_get_clu (budget 8, U = 4, bitmap), {x, y} records, k_scalar (no hand-over).
    Twice: the second time a clustered matrix answers the far keys from its hint table."""
    mode, via, env = GET_SETTINGS[setting]
    w = World(G, oracle_mod, capfd, monkeypatch, mode, env)
    try:
        w.build()
        st0 = w.g.stats()
        assert st0["clustered_mode"] == (1 if mode == "clustered" else 0), st0["clustered_mode"]
        w.far_exist()
        w.gets(via, "first")
        w.gets(via, "second")
        st = w.g.stats()
        assert st["clustered_mode"] == st0["clustered_mode"] and st["rows_grown"] == st0["rows_grown"]
        if via == "scalar":
            assert st["scalar_cache_hits"] == 0, "the scalar kernel was to answer every get"
        w.state(tag="after the gets")
    finally:
        w.close()


# ---- 2. hints -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint_lg", ("6", "16"))
def test_hints_remembered_evicted_and_stale(G, oracle_mod, capfd, monkeypatch, hint_lg):
    """every far key read three times: the walk that remembers, the hint, and -- after every row has doubled -- the stale base.
    64 slots of two entries against 3000 far keys: nearly every hint has been evicted, and every answer stays exact.  Then one op
    leaves a (0, 0) cell behind (y0_zeroed: hints off for the matrix) and the gets are repeated."""
    w = World(G, oracle_mod, capfd, monkeypatch, "clustered", (("SMATRIX_HINT_LG", hint_lg),))
    try:
        w.build()
        fx, fy = P.far_keys(w.cs)
        assert fy.size > P.HINT_WAYS * 64 * len(w.cs) // 2
        for turn in ("walk", "hinted"):
            w.apply(P.OP_GET, fx, fy, tag=turn)
            w.gets(tag=turn)
        # writers through the hints: each far key once (k_apply<OP, true> below 1024 ops, the fold and its retry above)
        w.apply(P.OP_INCR, fx[:700], fy[:700], np.arange(700) + 1, tag="incr by hint, lane per op")
        w.apply(P.OP_INCR, fx, fy, np.arange(fx.size) + 5, tag="incr by hint, fold")
        w.state(tag="after hinted writes")
        x, y, v = P.grow_batch(w.o, w.cs)
        grown0 = w.g.stats()["rows_grown"]
        w.apply(P.OP_INCR, x, y, v, tag="doubling")
        assert w.g.stats()["rows_grown"] - grown0 >= len(w.cs)
        for c in w.cs:
            assert w.g.row_info(c.row) == w.o.row_info(c.row) == (2 * c.size, c.size // 2 + 2)
        for turn in ("stale", "walk again", "hinted again"):
            w.apply(P.OP_GET, fx, fy, tag=turn)
        w.gets(tag="after the doubling")
        # a (0, v) cell whose value returns to 0
        r = w.cs[1].row
        w.apply(P.OP_INCR, [r], [0], [5], tag="(0, 5)")
        w.apply(P.OP_DECR, [r], [0], [5], tag="(0, 0)")
        w.apply(P.OP_GET, fx, fy, tag="hints off")
        w.gets(tag="hints off")
        assert w.g.stats()["clustered_mode"] == 1
    finally:
        w.close()


def test_hint_names_a_cell_of_a_reused_block(G, oracle_mod, capfd, monkeypatch):
    """a hint is {tag(block, key), cell}: row A's far keys are remembered, A doubles and its block goes back to the free list; row B
    -- the same keys, piled in the REVERSE order, so each lies in another cell -- then grows into a block of that size.  Whatever
    block it got: every get and every write on B's far keys is exact, and no key exists twice (used, the slot dump)."""
    a = P.Case(1, 4096)
    w = World(G, oracle_mod, capfd, monkeypatch, "clustered", cs=(a,))
    try:
        w.build()
        fx, fy = P.far_keys(w.cs)
        w.apply(P.OP_GET, fx, fy, tag="A remembered")
        x, y, v = P.grow_batch(w.o, w.cs)
        w.apply(P.OP_INCR, x, y, v, tag="A doubles")
        brow = np.full(a.run.size, 2, np.uint32)
        w.apply(P.OP_INCR, brow, a.run, P.value_of(a.run), tag="B: the run")
        for k in a.pile[::-1].tolist():
            w.apply(P.OP_INCR, [2], [k], [7], tag="B: the pile, reversed")
        w.rows = [2]                                         # (A has doubled: its displaced keys lie in the batch's own order)
        assert w.o.row_info(2) == (a.size, a.n_keys)
        w.state(tag="B built")
        bx = np.full(fy.size, 2, np.uint32)
        w.apply(P.OP_INCR, bx[:500], fy[:500], np.arange(500) + 1, tag="B incr, lane per op")
        w.apply(P.OP_DECR, bx, fy, np.arange(fy.size) + 3, tag="B decr, fold")
        w.apply(P.OP_GET, bx, fy, tag="B gets")
        w.state(tag="B written")
    finally:
        w.close()


# ---- 3. writers on far keys ------------------------------------------------------------------------------------------------------------
def writer_keys(cs, kind):
    """(x, y) of the present keys a writer case names, each ONCE: every pile key, or (lane per op / scalar) the classes and edges"""
    if kind in ("fold", "far"):
        return (np.concatenate([np.full(P.PILE, c.row, np.uint32) for c in cs]), np.concatenate([c.pile for c in cs]))
    idx = sorted(set(P.SPECIAL) | set(P.GROUP_EDGES) | {P.PILE - 1})
    return (np.concatenate([np.full(len(idx), c.row, np.uint32) for c in cs]), np.concatenate([c.pile[idx] for c in cs]))


def padded(cs, x, y, v, n, op):
    """the ops inside a batch of n: the rest are hits on the runs' home cells that change nothing"""
    if n <= x.size:
        return x, y, v
    px = np.concatenate([np.full(c.run.size, c.row, np.uint32) for c in cs])
    py = np.concatenate([c.run for c in cs])
    j = np.arange(n - x.size) % px.size
    at = np.sort(np.random.default_rng(n).permutation(n)[:x.size])
    xx, yy, vv = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint32)
    rest = np.ones(n, bool); rest[at] = False
    xx[rest], yy[rest], vv[rest] = px[j], py[j], (P.value_of(py[j]) if op == P.OP_SET else 0)
    xx[at], yy[at], vv[at] = x, y, v
    return xx, yy, vv


# far join: the keys the scan did not find are placed by k_far_place before the pass; "claims" (SMATRIX_FAR_PLACE=0): the pass inserts
# them itself -- coop_probe by the occupancy words from the key's home (start = pb, the first word masked), then far_claim_insert
WRITER_KINDS = {"lane per op": ("batch", 0, ()), "fold and retry": ("batch", P.AGG_MIN, ()), "far join": ("batch", P.FAR_JOIN_MIN, ()),
                "far join, claims": ("batch", P.FAR_JOIN_MIN, (("SMATRIX_FAR_PLACE", "0"),)), "scalar": ("scalar", 0, ())}
_FOLD_DEFERRED = re.compile(r"the folding kernel deferred (\d+) ops")
_OVERFLOWED = "OVERFLOWED"
_ROUND1 = re.compile(r"\[smatrix\] batch \d+ round 1 [^\n]*?ops=(\d+) deferred=(\d+)")
_GROW = re.compile(r"\[smatrix\] batch \d+ (?:round \d+|chain)[^\n]*? grow=(\d+)")


@pytest.mark.parametrize("kind", tuple(WRITER_KINDS))
@pytest.mark.parametrize("mode,far_join", (("clustered", "1"), ("clustered", "0"), ("plain", "1")))
def test_writers_on_far_keys(G, oracle_mod, capfd, monkeypatch, mode, far_join, kind):
    """incr, decr and set on PRESENT keys at every class (each key once per call: the returns have one order), then incr / set of
    ABSENT keys at every class, one new key per row and call: returns, gets, row_info and the slot dump byte for byte.  Through the
    lane-per-op kernel, through the fold (whose slow keys go to k_apply_short and k_apply_wpo on a clustered table), through a batch
    of 2^16 ops (the pass in front of prep: k_apply_wpo_far, the occupancy-word walk, far_claim_insert) and through the scalar call."""
    via, pad, env = WRITER_KINDS[kind]
    far = kind.startswith("far join")
    joined = far and mode == "clustered" and far_join == "1"
    w = World(G, oracle_mod, capfd, monkeypatch, mode, (("SMATRIX_FAR_JOIN", far_join), ("SMATRIX_SCALAR_CACHE", "0")) + env)
    n_join_rows = sum(c.size >= 1 << P.FAR_ROW_LG for c in w.cs)             # rows the join indexes
    assert n_join_rows >= 4

    def absent_path(k, op, x, y, err):
        """one new key per row, 2^16 ops: the fold defers the new keys (their probe outruns the lane), the pass takes that list"""
        if not joined:
            assert not any(int(a or b) for a, b in _PASS.findall(err)), err[-1500:]
            return
        if k < len(P.ABSENT_D) and P.ABSENT_D[k] <= P.HINT_BUDGET:
            return                                           # (within the lane's budget: the fold inserts the key itself)
        deferred = [int(a) for a in _FOLD_DEFERRED.findall(err)]
        took = [int(a or b) for a, b in _PASS.findall(err)]
        left = [int(a) for a in _ROUND0.findall(err)]
        # ... and leaves nothing for prep: every new key was inserted by the pass -- on the rows the join indexes by k_far_place, or
        # (claims) by the walk over the occupancy words and far_claim_insert
        assert deferred == [x.size] and took == [x.size] and left == [0] and _OVERFLOWED not in err and x.size > n_join_rows, (k, deferred, took, left, err[-1500:])

    def retry_path(k, op, x, y, err):
        """a batch of 1024 ops on a clustered table: the fold defers the far new keys, the retry (k_apply_short, k_apply_wpo) inserts them"""
        if mode != "clustered" or op != P.OP_INCR or (k < len(P.ABSENT_D) and P.ABSENT_D[k] <= P.HINT_BUDGET):
            return
        left = [int(a) for a in _ROUND0.findall(err)]
        if "chain:" in err:                                  # (the chained shape: the wave-per-op pass runs in front of prep and leaves it nothing)
            assert left == [0], (k, err[-1500:])
        else:
            assert left == [x.size] and _ROUND1.findall(err) == [(str(x.size), "0")], (k, err[-1500:])
    try:
        w.build()
        x, y = writer_keys(w.cs, "far" if pad >= P.AGG_MIN else "few")
        took = []
        for op, amount in ((P.OP_INCR, 3), (P.OP_DECR, 0x80000001), (P.OP_SET, 0xC0FFEE), (P.OP_INCR, 0xFFFFFFF0)):
            v = P.u32(np.arange(x.size, dtype=np.uint64) * 7 + amount)
            xx, yy, vv = padded(w.cs, x, y, v, pad, op)
            _, err = w.apply(op, xx, yy, vv, via=via, tag=("present", op))
            took += [int(a or b) for a, b in _PASS.findall(err)]
            if kind == "fold and retry" and mode == "clustered" and amount == 3:
                # the first call, nothing remembered yet: the fold settles what the lane reaches and defers the rest, the retry
                # kernels finish those (and remember them: the later calls may be settled by the hint table alone)
                d0, r1 = [int(a) for a in _ROUND0.findall(err)], _ROUND1.findall(err)
                assert len(d0) == 1 and d0[0] > 0 and r1 == [(str(d0[0]), "0")], (op, err[-1500:])
            w.apply(P.OP_GET, x, y, tag=("present, gets after", op))
            w.state(tag=("present", op))
        # (the pass in front of prep is for incr / decr: the far-join kinds insert with those two)
        traces = w.absent_inserts(via=via, pad=pad, tag=kind, ops=(P.OP_INCR, P.OP_DECR) if far else (P.OP_INCR, P.OP_SET),
                                  check=absent_path if far else retry_path if kind == "fold and retry" else None)
        took += [int(a or b) for t in traces for a, b in _PASS.findall(t)]
        for c in w.cs:
            assert w.g.row_info(c.row) == (c.size, c.n_keys + len(c.absent)), c.name
        w.gets(tag="after the writers")
        st = w.g.stats()
        assert st["clustered_mode"] == (1 if mode == "clustered" else 0)
        if far:
            assert (sum(took) > 0) == joined, ("the pass in front of prep took", took, w.trace[-1500:])
        if kind == "scalar":
            assert st["scalar_cache_hits"] == 0
    finally:
        w.close()


# ---- 4. the bitmap under each of its writers -------------------------------------------------------------------------------------------
def _grown(w):
    """every row doubles once, in ONE growth round (the trace's grow=): 2048 / 4096 cells through k_grow_lds, 16384 / 32768 through the
    chunked passes, on a clustered matrix with k_grow_move_home + k_grow_rest_lds -- the tiers of write_batch_helpers.TIER_SIZES"""
    x, y, v = P.grow_batch(w.o, w.cs)
    grown0 = w.g.stats()["rows_grown"]
    _, err = w.apply(P.OP_INCR, x, y, v, tag="doubling")
    assert sum(int(a) for a in _GROW.findall(err)) == len(w.cs) and w.g.stats()["rows_grown"] - grown0 == len(w.cs), err[-1500:]
    for c in w.cs:
        assert w.g.row_info(c.row) == (2 * c.size, c.size // 2 + 2), c.name


BITMAP_WRITERS = {
    "single calls": ("clustered", (), "steps"),                                                  # mark_home in apply_row
    "one batch": ("clustered", (), "one batch"),                                                 # the clustered fold + k_insert_keys
    "bulk path": ("clustered", (("SMATRIX_BULK_MIN", "1"),), "one batch"),
    "doubled": ("clustered", (), "steps"),                                                       # k_grow_lds, move_home + rest_lds, chunked
    "doubled, 64-cell slices": ("clustered", (("SMATRIX_REST_SLICE", "64"),), "steps"),
    "switched on by the data": ("auto", (), "steps"),                                            # k_home_rebuild
    "reopened": ("clustered", (), "steps"),                                                      # the loader's all-zero bitmap + clustered_sync
}


@pytest.mark.parametrize("writer", tuple(BITMAP_WRITERS))
def test_bitmap_under_each_writer(G, oracle_mod, capfd, monkeypatch, tmp_path, writer):
    """the gets of case 1 and the absent-key inserts of case 3 after the at-home bitmap was written by each of its writers.  A false
    bit makes a probe step over a key (a get returns 0) or over the free cell that ends it (the new key lands one cell late)."""
    mode, env, how = BITMAP_WRITERS[writer]
    w = World(G, oracle_mod, capfd, monkeypatch, mode, env, fname=str(tmp_path / "m.smx") if writer == "reopened" else None)
    try:
        err = w.build(how)
        exact = how == "steps"
        if writer == "bulk path":
            assert w.g.stats()["bulk_rounds"] >= 1, err[-1500:]
        if writer.startswith("doubled"):
            _grown(w)
            exact = False                                   # (a doubling re-inserts displaced keys in the batch's own order)
        if writer == "switched on by the data":
            # far present keys and one key of a row that does not exist (round 0 defers it: the host looks at the evidence).  The
            # calls of the build may have been evidence enough already: the switch and its k_home_rebuild are looked for in both.
            w.gets(tag="before the evidence")
            fx, fy = P.far_keys(w.cs, hinted=False)
            _, err2 = w.apply(P.OP_INCR, np.r_[fx[:800], np.uint32(777)], np.r_[fy[:800], np.uint32(5)], np.r_[np.ones(800, np.uint32), np.uint32(9)], tag="evidence")
            assert w.g.stats()["clustered_mode"] == 1 and _REBUILT.search(err + err2), (err + err2)[-1500:]
        if writer == "reopened":
            w.reopen()
            w.state(tag="reopened")
        assert w.g.stats()["clustered_mode"] == 1
        w.far_exist()
        w.gets(tag=writer)
        w.gets(tag=writer + ", hinted")
        w.absent_inserts(exact=exact, count=4 if not exact else None, tag=writer)
        w.gets(tag=writer + ", after the inserts")
        if writer == "reopened":
            w.reopen()
            w.gets(tag="reopened again")
    finally:
        w.close()


# ---- the column-0 entry far from slot 0 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("clustered", "plain"))
def test_column_zero_entry_far_from_slot_zero(G, oracle_mod, capfd, monkeypatch, mode):
    """the pile lies on slots 0 .. 399, then set(x, 0, v) as a call of its own: the (0, v) entry sits 400 cells from slot 0, and
    get(x, 0) walks there for Y == 0, for which the hint table is never asked"""
    cs = tuple(c for c in P.cases() if c.wrap)
    w = World(G, oracle_mod, capfd, monkeypatch, mode, cs=cs)
    try:
        w.build()
        rows = np.asarray(w.rows, np.uint32)
        zero = np.zeros_like(rows)
        for via in ("batch", "scalar"):
            w.apply(P.OP_GET, rows, zero, via=via, tag="before: the free cell")
        w.apply(P.OP_SET, rows[::2], zero[::2], rows[::2] + 70, tag="set (x, 0), batch")
        w.apply(P.OP_SET, rows[1::2], zero[1::2], rows[1::2] + 70, via="scalar", tag="set (x, 0), scalar")
        for c in cs:
            assert np.asarray(w.g.row_slots(c.row))[c.end].tolist() == [0, c.row + 70] and w.g.row_info(c.row) == (c.size, c.n_keys)
        for via in ("batch", "scalar", "packed"):
            w.apply(P.OP_GET, rows, zero, via=via, tag="get (x, 0)")
        w.apply(P.OP_INCR, rows, zero, rows, tag="incr (x, 0)")
        w.gets(tag="with the (0, v) cell")                   # (absent keys now walk across it: not a free cell)
        w.absent_inserts(count=3, tag="behind the (0, v) cell")
        w.state()
    finally:
        w.close()


# ---- 5. one shuffled batch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("clustered", "plain"))
def test_one_shuffled_batch_against_each_query_alone(G, oracle_mod, capfd, monkeypatch, mode):
    """every query of the cases above on ONE matrix in one batch, shuffled: long probes of all kinds share a wave and `todo` in
    coop_probe serves them one after the other -- against the oracle and against each query sent alone (a wave with one op).  The
    matrix has been through the cases first: far keys remembered, written through the hints, new keys inserted at three classes;
    then every row doubles (each remembered cell is stale) and the same batch is sent again."""
    w = World(G, oracle_mod, capfd, monkeypatch, mode)
    try:
        w.build()
        fx, fy = P.far_keys(w.cs)
        w.apply(P.OP_GET, fx[::2], fy[::2], tag="half the far keys remembered")
        w.apply(P.OP_INCR, fx[::3], fy[::3], np.arange(fx[::3].size) + 1, tag="a third written")
        new = []
        w.absent_inserts(count=3, tag="new keys", check=lambda k, op, x, y, err: new.append((x, y)))
        qx, qy = P.queries(w.cs)
        x = np.concatenate([qx, fx] + [a for a, _ in new])
        y = np.concatenate([qy, fy] + [b for _, b in new])
        p = np.random.default_rng(11).permutation(x.size)
        x, y = x[p], y[p]
        for turn in ("as built", "doubled"):
            mixed, _ = w.apply(P.OP_GET, x, y, tag=("shuffled", turn))
            alone = np.array([int(w.g.m.apply_batch(P.OP_GET, x[i:i + 1], y[i:i + 1])[0]) for i in range(x.size)], np.uint32)
            assert (alone == mixed).all(), (turn, np.flatnonzero(alone != mixed)[:8].tolist())
            for lo in range(0, x.size, 61):                  # ... and in waves of 61: every lane's neighbours change
                w.apply(P.OP_GET, x[lo:lo + 61], y[lo:lo + 61], tag=("wave", turn, lo))
            if turn == "as built":
                _grown(w)
    finally:
        w.close()
