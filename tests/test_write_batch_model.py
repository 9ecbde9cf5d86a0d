"""No GPU: every case of tests/write_batch_helpers.py stands where it claims, on the oracle and on the helper alone, so that a failure
of tests/test_gpu_write_batch_edges.py can only mean the kernel.

    serialisable accepts the oracle's own returns for every studied batch applied in 20 seeded orders, and rejects five mutations
    of such a transcript; the crowded keys share ONE start slot near the end of the LDS table; every case marked exact leaves the
    same bytes forward, reversed and shuffled; every tier case has the old size, the used counter, the new size and the number of
    doublings it is named after; the bulk batch creates the row sizes either side of its limits."""
import numpy as np
import pytest

from tests import write_batch_helpers as W

INCR_OPS = (W.OP_INCR, W.OP_DECR)


def fresh(oracle_mod, batches):
    o = oracle_mod.Oracle()
    for b in batches:
        o.apply(b.op, b.x, b.y, b.v)
    return o


def scenarios():
    for op in INCR_OPS:
        for n in W.N_INCR:
            yield "incr op %d n %d" % (op, n), W.incr_scenario(op, n)
        yield "crowd op %d" % op, W.crowd_scenario(op)
        yield "bulk op %d" % op, [W.bulk_batch(op)]
    for n in W.N_SET:
        yield "set n %d" % n, W.set_scenario(n)


# ---- serialisable ----------------------------------------------------------------------------------------------------------------------
def test_serialisable_by_hand():
    S = W.serialisable
    assert S(W.OP_INCR, 5, [], [], 5) and not S(W.OP_INCR, 5, [], [], 6)
    assert S(W.OP_INCR, 5, [1, 2], [6, 8], 8) and S(W.OP_INCR, 5, [1, 2], [8, 7], 8)          # both orders
    assert not S(W.OP_INCR, 5, [1, 2], [7, 8], 8)                                               # 2-then-1 returns swapped
    assert S(W.OP_DECR, 1, [3, 0], [0xFFFFFFFE, 0xFFFFFFFE], 0xFFFFFFFE)                        # below zero; amount 0 is a self-loop
    assert S(W.OP_DECR, 1, [3, 0], [0xFFFFFFFE, 1], 0xFFFFFFFE)                                 # ... on either value it may pass
    assert not S(W.OP_DECR, 1, [3, 0], [0xFFFFFFFE, 7], 0xFFFFFFFE)                             # a self-loop nobody reaches
    assert S(W.OP_INCR, 0xFFFFFFFF, [1, 0xFFFFFFFF], [0, 0xFFFFFFFF], 0xFFFFFFFF)               # v and 2^32 - v: a cycle
    assert S(W.OP_INCR, 9, [4, 4, 4], [17, 13, 21], 21) and not S(W.OP_INCR, 9, [4, 4, 4], [13, 13, 21], 21)
    # two cycles that do not touch: balanced everywhere, yet no serial order
    assert not S(W.OP_INCR, 0, [1, 0xFFFFFFFF, 1, 0xFFFFFFFF], [1, 0, 101, 100], 0)


@pytest.mark.parametrize("op", INCR_OPS)
def test_serialisable_accepts_the_oracle_in_20_orders(oracle_mod, op):
    n_checked = 0
    for tag, batches in scenarios():
        for i, b in enumerate(batches):
            if not b.study or b.op != op:
                continue
            for seed in range(20):
                o = fresh(oracle_mod, batches[:i])
                p = np.random.default_rng(seed).permutation(b.n)
                W.apply_checked(o, b.permuted(p), (tag, "order", seed))
                o.close()
                n_checked += 1
    assert n_checked >= 20 * (4 * len(W.N_INCR) + 10 + 1)


def transcript(oracle_mod, op, n):
    """one key, n ops in a seeded order on the oracle -> (before, v, ret, after, generic)"""
    rng = np.random.default_rng(n + op)
    v, generic = W.amounts(rng, n, min(n, W.AGG_TILE) // 2)
    o = fresh(oracle_mod, W.setup_batches(op))
    x, y = np.full(n, W.R_ONE, np.uint32), np.full(n, 5, np.uint32)
    before = o.get(W.R_ONE, 5)
    ret = o.apply(op, x, y, v)
    after = o.get(W.R_ONE, 5)
    o.close()
    return before, v, ret, after, generic


@pytest.mark.parametrize("op", INCR_OPS)
@pytest.mark.parametrize("n", (2, 3, 1023, 2049, 6143))
def test_serialisable_rejects_every_mutant(oracle_mod, op, n):
    before, v, ret, after, generic = transcript(oracle_mod, op, n)
    if n <= 3:                                   # (too short for the seeded classes: every op generic, amounts distinct)
        v = np.array([7, 1000, 31][:n], np.uint32)
        ret = before + np.cumsum(v).astype(np.uint32) if op == W.OP_INCR else before - np.cumsum(v).astype(np.uint32)
        ret = ret.astype(np.uint32); after = int(ret[-1]); generic = np.ones(n, bool)
    S = W.serialisable
    assert S(op, before, v, ret, after)
    g = np.flatnonzero(generic)
    rng = np.random.default_rng(99 + n)
    for trial in range(8):
        i, j = (int(a) for a in rng.choice(g, 2, replace=False))
        assert v[i] != v[j]
        m = ret.copy(); m[i], m[j] = ret[j], ret[i]
        assert not S(op, before, v, m, after), ("two returns swapped", i, j)
        m = ret.copy(); m[i] += np.uint32(1)
        assert not S(op, before, v, m, after), ("one return off by one", i)
        if i == 0:
            i = j if j else int(g[g > 0][0])
        r_i, v_i = int(ret[i]), int(v[i])
        prefix = (r_i - v_i - before if op == W.OP_INCR else before - r_i - v_i) & W.ALL_ONES
        assert prefix != 0
        m = ret.copy(); m[i] = (r_i + prefix if op == W.OP_INCR else r_i - prefix) & W.ALL_ONES
        assert not S(op, before, v, m, after), ("one op's prefix counted twice", i)
        assert not S(op, before, v, ret, (after + 1) & W.ALL_ONES), "the final value changed"
        keep = np.arange(n) != i
        assert not S(op, before, v[keep], ret[keep], after), ("one op dropped", i)


# ---- the crowded slot ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("incr", "clustered", "set"))
def test_crowded_keys_share_one_start_slot_near_the_end(which):
    x, ys, slot = W.crowd(which)
    assert ys.size == W.AGG_TILE + 1 and np.unique(ys).size == ys.size and (ys != 0).all()
    s = W.SLOT_FNS[which](np.uint32(x), ys)
    assert (s == slot).all() and W.AGG_SLOTS - W.CROWD_TAIL <= slot < W.AGG_SLOTS
    # 2048 keys from one start slot: a chain of 2048 slots that wraps 4095 -> 0, the table at load exactly 1/2
    assert slot + W.AGG_TILE > W.AGG_SLOTS and 2 * W.AGG_TILE == W.AGG_SLOTS
    # the arithmetic, once by hand (python ints) against the numpy line
    X, Y = x, int(ys[17])
    if which == "clustered":
        h = (X * 0x9E3779B1 ^ (Y >> 4) * 0x85EBCA77) & 0xFFFFFFFF
        assert ((h ^ h >> 15) + (Y & 15)) & 4095 == slot
    else:
        h = (X * 0x9E3779B1 ^ Y * 0x85EBCA77) & 0xFFFFFFFF
        assert (h ^ h >> 15) & 4095 == slot


# ---- the cases' own properties ------------------------------------------------------------------------------------------------------------
def test_batch_shapes():
    for op in INCR_OPS:
        for n in W.N_INCR:
            for b in W.incr_scenario(op, n)[2:]:
                assert b.n == n and b.op == op, b.name
            m = W.mixed_batch(op, n, 1)
            k = W.key64(m.x, m.y)
            first = np.arange(n) < W.AGG_TILE
            at = lambda x, y: np.flatnonzero(k == W.key64(np.uint32(x), np.uint32(y))).tolist()      # noqa: E731
            if n > W.AGG_TILE:
                assert {W.AGG_TILE - 1, W.AGG_TILE} <= set(at(W.R_PRESENT[1], 3))
            both_ends = at(W.R_PRESENT[1], 3) if n == W.AGG_TILE + 1 else at(W.R_PRESENT[0], 3)
            assert {0, n - 1} <= set(both_ends)
            assert len(at(W.ALL_ONES, W.ALL_ONES)) == 5 and first[at(W.ALL_ONES, W.ALL_ONES)].all()
            for rows in ((W.R_FULL,), W.R_ROOM, W.R_NEW, W.R_HEAD):          # all four kinds and the y == 0 ops: in tile 0, duplicated
                sel = np.isin(m.x, rows)
                assert first[sel].all() and np.unique(k[sel]).size < sel.sum()
            assert (m.y[np.isin(m.x, W.R_HEAD)] == 0).all()
        for b in W.crowd_scenario(op):
            assert b.n in (W.AGG_TILE, 2 * W.AGG_TILE, W.AGG_TILE + 1)
        assert W.bulk_batch(op).n == 4096
    for n in W.N_SET:
        sc = W.set_scenario(n)
        assert [b.n for b in sc[2:]] == [n, n, n]
        m = sc[3]
        k = W.key64(m.x, m.y)
        i21 = np.flatnonzero(k == W.key64(np.uint32(W.R_PRESENT[1]), np.uint32(3)))
        i40 = np.flatnonzero(k == W.key64(np.uint32(W.R_FULL), np.uint32(40)))
        if n > W.AGG_TILE:
            assert i21[-2:].tolist() == [W.AGG_TILE - 1, W.AGG_TILE] and i21.size >= 4
        if n > W.AGG_TILE + 1:
            assert i40.tolist() == [2, W.AGG_TILE + 1]
        assert ((m.y == 0) & np.isin(m.x, W.R_HEAD)).sum() == 4 and (m.x == W.R_ZERO).any() and (k == W.key64(np.uint32(W.ALL_ONES), np.uint32(W.ALL_ONES))).sum() == 5


def test_head_cells_stay_nonzero_and_the_threshold_row_stands_at_it(oracle_mod):
    for op in INCR_OPS:
        for n in (1023, 6143):
            sc = W.incr_scenario(op, n)
            o = fresh(oracle_mod, sc[:2])
            assert o.row_info(W.R_FULL) == (64, 33) and all(o.row_info(r) == (64, 20) for r in W.R_ROOM)
            assert all(o.row_info(r) is None for r in W.R_NEW) and o.get(W.ALL_ONES, W.ALL_ONES) == 123456
            for r in W.R_HEAD:
                assert np.asarray(o.row_slots(r))[0].tolist() == [0, W.HEAD_VALUE]
            for b in sc[2:]:
                o.apply(b.op, b.x, b.y, b.v)
            assert o.row_info(W.R_FULL) == (128, 40) and all(o.row_info(r) == (64, 30) for r in W.R_ROOM)
            assert all(o.row_info(r) == (16, 8) for r in W.R_NEW)
            total = 2 * 90                                                    # no order can bring a head cell to 0 on the way
            for r in W.R_HEAD:
                assert abs(o.get(r, 0) - W.HEAD_VALUE) <= total < W.HEAD_VALUE
            # the absent key of the one-key batches is a live cell: (6, total), counted in rowlen
            cells = np.asarray(o.row_slots(W.R_ONE))
            assert cells[6, 0] == 6 and o.rowlen(W.R_ONE) == 4
            if n <= W.AGG_TILE:
                assert cells[6, 1] == 0                                       # ... a live (6, 0)
            crossed = o.get(W.R_PRESENT[0], 1)
            assert crossed > (1 << 31) if op == W.OP_DECR else crossed < (1 << 31)
            o.close()


def test_exact_cases_are_order_independent(oracle_mod):
    """forward, reversed and one seeded shuffle of every batch marked exact (the batches before it forward): one slot dump"""
    n_exact = 0
    for tag, batches in scenarios():
        for i, b in enumerate(batches):
            if not b.exact:
                continue
            dumps = []
            for p in (np.arange(b.n), np.arange(b.n)[::-1], np.random.default_rng(i).permutation(b.n)):
                o = fresh(oracle_mod, batches[:i])
                q = b.permuted(p)
                o.apply(q.op, q.x, q.y, q.v)
                if b.op == W.OP_SET:                                  # (a set batch is ordered by index: only the cells' places are free)
                    lx, ly, lv = W.last_wins(b.x, b.y, b.v)
                    o.apply(W.OP_SET, lx, ly, lv)
                dumps.append(W.dump_rows(o, o.list_rows().tolist()))
                o.close()
            assert dumps[0] == dumps[1] == dumps[2], (tag, b.name)
            n_exact += 1
    assert n_exact > 100


@pytest.mark.parametrize("dense", (False, True))
@pytest.mark.parametrize("size", W.TIER_SIZES)
def test_tier_cases_land_where_they_say(oracle_mod, size, dense):
    t = W.Tier(size, dense)
    built = fresh(oracle_mod, [t.build])
    for c in t.cases:
        assert built.row_info(c.row) == (size, size // 2 + 1), c.name
    base = W.dump_rows(built, built.list_rows().tolist())
    built.close()
    for p in (np.arange(t.build.n)[::-1], np.random.default_rng(4).permutation(t.build.n)):       # the build is order-independent too
        o = fresh(oracle_mod, [t.build.permuted(p)])
        assert W.dump_rows(o, o.list_rows().tolist()) == base
        o.close()
    assert any(c.n == 1 for c in t.cases) and any(c.doublings == 2 for c in t.cases)
    for c in t.cases:
        dumps = []
        for p in (np.arange(c.n), np.arange(c.n)[::-1], np.random.default_rng(3).permutation(c.n)):
            o = fresh(oracle_mod, [t.build])
            q = c.permuted(p)
            W.apply_checked(o, q, c.name)
            assert o.row_info(c.row) == (size << c.doublings, c.used_after), (c.name, o.row_info(c.row))
            if c.doublings == 1 and c.n > 3:
                full = c.used_after == size + 1
                assert full == ("fill" in c.name), c.name                # exactly what the doubled table may still take
            dumps.append(W.dump_rows(o, [c.row]))
            o.close()
        assert dumps[0] == dumps[1] == dumps[2], c.name
    assert max(size << c.doublings for c in t.cases) <= 65536


@pytest.mark.parametrize("op", INCR_OPS)
def test_bulk_batch_rows(oracle_mod, op):
    b = W.bulk_batch(op)
    o = fresh(oracle_mod, [b])
    sizes = {c: W.rows_for(c) for c in (8, 9, 10, 256, 257, 258)}
    assert sizes == {8: 16, 9: 16, 10: 32, 256: 512, 257: 512, 258: 1024}
    for row, c in b.counts.items():
        assert o.row_info(row) == (W.rows_for(c), c), (row, c)
    assert np.unique(W.key64(b.x, b.y), return_counts=True)[1].tolist() == [2] * 2048
    o.close()
