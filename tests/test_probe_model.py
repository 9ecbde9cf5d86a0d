"""No GPU: tests/probe_helpers.py stands where it claims -- every constant on its source line, every case's distance classes read back
from the oracle's own slot dump -- so that a failure of tests/test_gpu_probe_edges.py can only mean the kernel."""
import os
import re

import numpy as np
import pytest

from tests import probe_helpers as P

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libsmatrix_amd", "csrc")


def source(name):
    with open(os.path.join(KERNELS, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def built(oracle_mod):
    o = oracle_mod.Oracle()
    for op, x, y, v in P.steps():
        o.apply(op, x, y, v)
    yield o
    o.close()


# ---- the constants --------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    ops, layout, rt = source("kernels/ops.hpp"), source("kernels/layout.hpp"), source("smx_runtime.hip")
    define = lambda text, name: int(re.search(r"^#define %s (\d+)" % name, text, re.M).group(1))      # noqa: E731
    assert define(ops, "SMX_HINT_BUDGET") == P.HINT_BUDGET and "constexpr uint32_t HINT_BUDGET = SMX_HINT_BUDGET;" in ops
    assert define(ops, "SMX_PROBE_BUDGET") == P.PROBE_BUDGET and "constexpr uint32_t PROBE_BUDGET = SMX_PROBE_BUDGET;" in ops
    assert define(layout, "SMX_HOME_LG") == P.HOME_LG and define(layout, "SMX_BIG_LG") == P.BIG_LG
    assert define(ops, "SMX_GET_WALK_U") * P.WORD == P.CAND_U4 and "template <int U = 1>\n__device__ inline uint32_t coop_probe(" in ops
    # the lane: `step >= budget` after the step's cell (get), `steps > budget` (writers): budget + 1 cells, hand-over behind them
    assert "if (MODE && step >= budget) { *lp = LongProbe{true, cells, mask, pos}; return 0; }" in ops
    assert "if (MODE && steps > budget) { *lp = LongProbe{true, cells, mask, pos}; return 0; }" in ops
    assert "const uint32_t budget = WPO && FAR ? 0u : has_hints ? HINT_BUDGET : PROBE_BUDGET;" in ops
    # k_get_clu: home, then HINT_BUDGET cells from home + 1, hand-over at home + 1 + HINT_BUDGET
    assert "for (uint32_t i = 0; i < HINT_BUDGET; i++) c[i] = cells[(home + 1u + i) & mask];" in ops
    assert "lp = LongProbe{true, cells, mask, (home + 1u + HINT_BUDGET) & mask};" in ops
    assert "coop_probe<SMX_GET_WALK_U>(lp.need, lp.cells, lp.mask, Y, lp.pos, use_home, nullptr)" in ops
    # the window phase: 4 x 64 cells per step, `off <= mb`
    assert "done += %d)" % P.WINDOW in ops and "const uint64_t off = done + (uint32_t)w * 64u + lane;" in ops and "ok[w] = off <= mb;" in ops
    assert "for (int w = 0; w < 4; w++)" in ops and 4 * P.WORD == P.WINDOW
    # the bitmap phase: where it starts, the first word's mask, the group, the candidate loop
    assert "const bool by_bits = by_occ || (use_home && mb + 1u >= (1u << HOME_LG));" in ops
    assert "const uint32_t start = by_occ ? pb : (pb + %du) & mb;" % P.WINDOW in ops
    assert "if (wi == 0) cand &= ~0ull << (start & 63u);" in ops
    assert "wd += %d)" % P.GROUP_WORDS in ops and "cand = ~hb[(w0 + wi) & wmask];" in ops
    assert "base += 64 * U)" in ops and P.CAND_U1 == P.WORD
    # the hint table: two {tag, cell} entries per slot, the cell decides
    assert "return e.x == tag && e.y <= mask ? e.y : e.z == tag && e.w <= mask ? e.w : 0xFFFFFFFFu;" in ops and P.HINT_WAYS == 2
    assert "*slot = e.x == tag ? uint4{tag, pos, e.z, e.w} : uint4{tag, pos, e.x, e.y};" in ops
    assert "return cell_key(cells[p]) == Y ? p : 0xFFFFFFFFu;" in ops
    # mark_home, and where the bitmap lies
    assert "if (mark_home && lg >= HOME_LG && pos == (Y & mask)) atomicOr(&row_home(arena, s.z, lg)[pos >> 6], 1ull << (pos & 63u));" in ops
    assert "units_of_lg(lg) + (lg >= BIG_LG ? SUB_UNITS : 0)) * UNIT_BYTES" in layout
    # the far join's threshold and the lane-per-op kernel's
    assert "m->home_on && m->far_join && n >= (1u << 16)" in rt and P.FAR_JOIN_MIN == 1 << 16
    assert define(ops, "SMX_FAR_ROW_LG") == P.FAR_ROW_LG and "meta_lg(s.x) < FAR_ROW_LG) continue;" in ops
    assert "const uint32_t start = by_occ ? pb :" in ops and "bool far_place = true;" in rt
    assert re.search(r"agg_min = %d\b" % P.AGG_MIN, rt)
    assert P.SIZES == (2048, 1 << P.HOME_LG, 4 << P.HOME_LG, 1 << P.BIG_LG)


def test_classes_by_hand():
    assert P.classes(True, 4096) == {"home": 0, "lane first": 1, "lane last": 8, "window first": 9, "window last": 264, "behind the window": 265,
                                     "start word, bit before": 264, "start word, first bit": 265}
    assert P.start_bit(4096, 4096 * 7 + 100) == (100 + 265) & 63
    assert P.classes(True, 16384)["second group"] == 9 + 256 + 4096
    assert sorted(P.classes(False, 2048).values()) == [0, 48, 49, 304, 305, 560, 561]
    assert P.first_bitmap_distance(True) == 265 and P.first_bitmap_distance(False) == 305
    both = set(P.classes(True, 4096).values()) | set(P.classes(False, 4096).values())
    assert both - {0} <= set(P.SPECIAL.values()) and both <= set(P.ABSENT_D)
    assert not set(P.GROUP_EDGES) & set(P.SPECIAL) and max(P.GROUP_EDGES) < P.PILE


def test_reading_a_dump_by_hand():
    s = np.zeros((16, 2), np.uint32)
    s[3], s[4], s[5], s[15], s[0] = (3, 7), (19, 1), (35, 2), (31, 9), (47, 4)
    key, at, d = P.distances(s)
    assert dict(zip(key.tolist(), zip(at.tolist(), d.tolist()))) == {47: (0, 1), 3: (3, 0), 19: (4, 1), 35: (5, 2), 31: (15, 0)}
    assert P.probe_end(s, 35) == (5, 2, True) and P.probe_end(s, 51) == (6, 3, False) and P.probe_end(s, 63) == (1, 2, False)
    assert P.probe_end(s, 0) == (1, 1, False)                                 # y == 0: the first cell whose key field is 0
    s[1] = (0, 5)
    assert P.probe_end(s, 0) == (1, 1, True) and P.probe_end(s, 63) == (2, 3, False)      # a (0, v) cell is not a free cell


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def test_cases_cover_the_sizes_and_placements():
    cs = P.cases()
    assert {(c.size, c.wrap) for c in cs} == {(s, w) for s in P.SIZES for w in (False, True)}
    assert any(c.second for c in cs) and len({c.row for c in cs}) == len(cs) and not {c.row for c in cs} & set(P.MISSING_ROWS)


@pytest.mark.parametrize("i", range(len(P.cases())), ids=[c.name for c in P.cases()])
def test_case_stands_where_it_claims(built, i):
    c = P.cases()[i]
    S = c.size
    size, used = built.row_info(c.row)
    assert size == S and used == c.n_keys and S // 4 + 1 < used <= S // 2 + 1            # the oracle ends at exactly this size
    assert c.room >= len(c.absent_d) + 8                                                  # room for the inserts of the GPU tests
    slots = np.asarray(built.row_slots(c.row))
    key, at, d = P.distances(slots)
    assert key.size == used < S                                                          # the table keeps free cells
    where = dict(zip(key.tolist(), zip(at.tolist(), d.tolist())))
    assert all(where[int(k)][1] == 0 for k in c.run)                                     # the runs are at home
    assert all(where[k] == c.pile_at[k] for k in c.pile.tolist())                        # the pile lies as planned
    pile_d = {where[k][1] for k in c.pile.tolist()}
    for hinted in (True, False):
        claims = c.claims(hinted)
        assert set(P.classes(hinted, S)) == set(claims), "a class this row cannot hold"
        for name, dist in claims.items():
            if name == "second group":                                                   # (from this distance on, not at it)
                assert max(pile_d) >= dist, (c.name, name, dist)
            else:
                assert dist in pile_d | {0}, (c.name, hinted, name, dist)
    # the word the bitmap walk starts in: the keys at 264 and 265 share a home, `start` is not a word's first bit, so the key on the
    # bit before `start` and the key on bit `start & 63` lie in ONE word -- the one coop_probe masks
    k264, k265 = (next(k for k in c.pile.tolist() if where[k][1] == dd and c.pile_at[k][0] >= 270) for dd in (264, 265))
    assert k264 & (S - 1) == k265 & (S - 1) and P.start_bit(S, k265) != 0
    assert where[k264][0] >> 6 == where[k265][0] >> 6 and where[k265][0] & 63 == P.start_bit(S, k265) == (where[k264][0] & 63) + 1
    # the group edges: keys reached after exactly 63 / 64 / 65 and 255 / 256 / 257 cells that are not at home
    if S >= 1 << P.HOME_LG:
        ranks = {P.not_home_before(slots, k) for k in c.pile.tolist()}
        assert set(P.GROUP_EDGES) <= ranks, (c.name, sorted(set(P.GROUP_EDGES) - ranks))
        assert max(pile_d) > P.first_bitmap_distance(True)
    # the walk starts inside a word, and the cell in front of the run is free (the occupancy walk's first word has bits to mask)
    assert c.a & 63 and not slots[(c.a - 1) % S].any()
    # absent keys: the probe ends on a free cell at every class
    ends = [P.probe_end(slots, int(y)) for y in c.absent]
    assert [e[1] for e in ends] == list(c.absent_d) and not any(e[2] for e in ends) and {e[0] for e in ends} == {c.end}
    assert set(P.ABSENT_D) <= set(c.absent_d) and max(c.absent_d) == c.r + P.PILE + (c.RUN2 if c.second else 0)
    assert not set(c.absent.tolist()) & set(key.tolist())
    if c.wrap:
        # keys whose walk crosses slot S-1 -> 0 inside the lane's cells, inside the window, inside the bitmap phase
        off = {k: S - (k & (S - 1)) for k in c.pile.tolist() if (k & (S - 1)) + where[k][1] >= S}
        assert any(o <= P.HINT_BUDGET for o in off.values())
        assert any(P.HINT_BUDGET < o <= P.HINT_BUDGET + P.WINDOW for o in off.values())
        assert any(o > P.HINT_BUDGET + P.WINDOW for o in off.values())
        assert slots[S - 1].any() and slots[0].any()
    if c.second:
        # the pile flows around the second run: keys behind it are reached across set bits
        run2 = c.run[c.r:]
        assert any(where[k][0] > int(run2[-1]) for k in c.pile.tolist()) and any(where[k][0] < int(run2[0]) for k in c.pile.tolist())


def test_queries_name_every_class(built):
    x, y = P.queries()
    for c in P.cases():
        mine = set(y[x == c.row].tolist())
        assert set(c.pile.tolist()) | set(c.absent.tolist()) | {0, int(c.run[0]), int(c.run[c.r - 1])} <= mine
    assert set(P.MISSING_ROWS) <= set(x.tolist()) and all(built.row_info(r) is None for r in P.MISSING_ROWS)
    fx, fy = P.far_keys()
    assert np.unique(fy[fx == P.cases()[1].row]).size > P.HINT_WAYS * 64            # more far keys than a 64-slot hint table holds


def test_one_batch_build_holds_the_same_keys(oracle_mod, built):
    (op, x, y, v), = P.steps(how="one batch")
    assert x.size == sum(s[1].size for s in P.steps())
    o = oracle_mod.Oracle()
    o.apply(op, x, y, v)
    qx, qy = P.queries()
    assert (o.apply(P.OP_GET, qx, qy) == built.apply(P.OP_GET, qx, qy)).all()
    for c in P.cases():
        assert o.row_info(c.row) == built.row_info(c.row)
        # whatever order the batch took, a key with the run's first cell as its home lies behind the whole run
        _, _, d = P.distances(o.row_slots(c.row))
        assert d.max() >= c.r > P.first_bitmap_distance(False)
    o.close()


def test_column_zero_entry_far_from_slot_zero(oracle_mod):
    cs = [c for c in P.cases() if c.wrap]
    o = oracle_mod.Oracle()
    for op, x, y, v in P.steps(cs):
        o.apply(op, x, y, v)
    for c in cs:
        assert P.probe_end(o.row_slots(c.row), 0) == (c.end, c.end, False) and c.end >= P.PILE
        assert o.set(c.row, 0, 77) == 77
        s = np.asarray(o.row_slots(c.row))
        assert s[c.end].tolist() == [0, 77] and P.probe_end(s, 0) == (c.end, c.end, True)
        assert o.get(c.row, 0) == 77 and o.row_info(c.row)[1] == c.n_keys            # (nothing was inserted: quirk Q1)
    o.close()


def test_grow_and_absent_batches(oracle_mod):
    o = oracle_mod.Oracle()
    for op, x, y, v in P.steps():
        o.apply(op, x, y, v)
    before = {c.row: o.row_info(c.row) for c in P.cases()}
    for k in (0, 7, P.N_ABSENT - 1, 7):
        x, y, ends = P.absent_batch(o, k)
        assert np.unique(x).size == x.size and all(e[1] == P.ABSENT_D[k] for e in ends if k < len(P.ABSENT_D))
        o.apply(P.OP_INCR, x, y, P.value_of(y))
        for r, k, e in zip(x.tolist(), y.tolist(), ends):
            assert np.asarray(o.row_slots(r))[e[0]].tolist() == [k, int(P.value_of(k))]
    x, y, v = P.grow_batch(o)
    o.apply(P.OP_INCR, x, y, v)
    for c in P.cases():
        assert o.row_info(c.row) == (2 * c.size, c.size // 2 + 2), (c.name, before[c.row])
        _, _, d = P.distances(o.row_slots(c.row))
        if not c.wrap:                               # (a wrapped pile lies in front of its run in slot order: the doubling puts it at home)
            assert d.max() > P.first_bitmap_distance(True), c.name                     # far keys remain after the doubling
    o.close()
