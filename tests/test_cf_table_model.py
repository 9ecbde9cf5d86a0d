"""CPU: the host model of the session tables (tests/cf_table_helpers.py) against the kernels' own constants, read as source text, and
every case of tests/test_gpu_cf_table_edges.py built over the oracle: its exact need, tier and table size, its load, its candidate
counts, its probe chains -- and the condition that lets it run at all, one free slot more than the table has keys."""
import os
import re

import numpy as np
import pytest

from tests import cf_group_helpers as G
from tests import cf_sim_helpers as H
from tests import cf_table_helpers as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libsmatrix_amd", "csrc")


def constexpr(text, ctype, name):
    hit = re.findall(r"constexpr\s+%s\s+%s\s*=\s*([^;]+);" % (ctype, name), text)
    assert len(hit) == 1, (name, hit)
    return hit[0].strip()


def test_constants_are_the_kernels():
    with open(os.path.join(CSRC, "kernels", "recommend.hpp")) as f:
        rec = f.read()
    with open(os.path.join(CSRC, "smx_recommend.inc")) as f:
        inc = f.read()
    for name, value in T.SOURCE_CONSTANTS.items():
        assert int(constexpr(rec, "uint32_t", name)) == value, name
    assert int(constexpr(rec, "uint64_t", "REC_DEDUP_MAX")) == T.REC_DEDUP_MAX
    assert constexpr(inc, "uint64_t", "REC_GROUP_SLOTS") == "1ull << 25" and T.REC_GROUP_SLOTS == 1 << 25
    assert "tlg[s] = (uint8_t)rec_lg(need, 6);" in rec and T.REC_LDS_MIN_LG == 6
    assert "rec_lg(need, REC_GL_MIN_LG)" in rec and "if (need <= REC_LDS_SLOTS)" in rec
    assert "const bool exact = L <= REC_DEDUP_MAX;" in rec and "if (bound > all_cells) bound = all_cells;" in rec
    assert "uint64_t need = bound + L;" in rec and "need += f.ex_off[s + 1] - f.ex_off[s];" in rec
    assert "if (bound == 0) { counts[s] = 0; continue; }" in rec
    assert "(1u << meta_lg(sn.x)) + REC_CHUNK - 1) / REC_CHUNK" in rec                  # k_rec_gl_plan's chunks
    body = rec[rec.index("void k_rec_scope_bound"):rec.index("__global__", rec.index("void k_rec_scope_bound"))]
    assert "REC_SCOPE_MAX" in body and "need" not in body and "tlg" not in body         # it measures the lists and sizes nothing
    with open(os.path.join(CSRC, "kernels", "layout.hpp")) as f:
        assert "h ^= h >> 16; h *= 0x85ebca6bU; h ^= h >> 13; h *= 0xc2b2ae35U; h ^= h >> 16;" in f.read()


def test_fmix32_and_its_inverse():
    rng = np.random.default_rng(1)
    x = np.concatenate([[0, 1, T.M32, 1 << 31, 0x12345678], rng.integers(0, 1 << 32, 100000, dtype=np.uint64)]).astype(np.uint32)
    assert (T.unfmix32(T.fmix32(x)) == x).all() and (T.fmix32(T.unfmix32(x)) == x).all()
    assert int(T.fmix32(np.uint32(1))) == 0x514E28B7                       # murmur3's finalizer of 1
    assert T.fmix32(np.arange(1 << 16)).dtype == np.uint32 and np.unique(T.fmix32(np.arange(1 << 16))).size == 1 << 16


def test_crafted_ids_land_on_their_home_slots():
    for slot, lg in ((0, 12), (4095, 12), (8191, 13), (8176, 13), (100, 13), (12345, 15)):
        ids = T.ids_homed_at(slot, lg, 7, skip=2)
        assert ids.size == 7 == np.unique(ids).size and (ids >= T.FLOOR).all() and (ids < T.CEIL).all()
        assert (T.home(ids, lg) == slot).all()
        assert not set(ids.tolist()) & set(T.ids_homed_at(slot, lg, 2).tolist())
        for smaller in range(6, lg):
            assert (T.home(ids, smaller) == slot % (1 << smaller)).all()
    last16 = set(T.LAST16)
    for ids in (T.CHAIN_COLS, T.CHAIN_ITEMS, T.CHAIN_EXCL, T.CHAIN_ABSENT):
        assert set(T.home(ids, 13).tolist()) == last16 and set(T.home(ids, 12).tolist()) == set(range(4080, 4096))
    assert T.home(T.NEAR_COLS, 13).tolist() == list(range(8136, 8160))
    assert T.home(T.SEG0_COLS, 13).tolist() == list(range(100, 170)) and T.home(T.SEG1_COLS, 13).tolist() == list(range(5000, 5005))
    crafted = np.concatenate([T.CHAIN_COLS, T.CHAIN_ITEMS, T.CHAIN_EXCL, T.CHAIN_ABSENT, T.NEAR_COLS, T.SEG0_COLS, T.SEG1_COLS])
    assert np.unique(crafted).size == crafted.size
    x, y, _ = T.world_contents()
    others = np.concatenate([x, y[~np.isin(y, crafted)], T.ROWLESS, [T.ABSENT]])
    assert int(others[others != T.M32].max()) < T.FLOOR <= int(crafted.min())            # they collide with nothing else
    assert not np.isin(T.CHAIN_ABSENT, np.concatenate([x, y])).any() and not np.isin(T.ROWLESS, np.concatenate([x, y])).any()


def test_occupied_runs():
    occ = np.zeros(16, bool)
    occ[[14, 15, 0, 1, 2, 7, 8]] = True
    assert T.wrap_run(occ) == (2, 3) and T.longest_run(occ) == (14, 5) and T.run_end(occ, 15) == 4 and T.run_end(occ, 3) == 0
    keys = T.ids_homed_at(4095, 12, 5)                                   # (homed at slot 63 of a 64-slot table as well)
    assert np.flatnonzero(T.occupied(keys, 6)).tolist() == [0, 1, 2, 3, 63]
    with pytest.raises(AssertionError):
        T.occupied(T.ids_homed_at(0, 12, 64), 6)


class World:
    pass


@pytest.fixture(scope="module")
def world(oracle_mod):
    w = World()
    w.m = oracle_mod.Oracle()
    T.build(w.m)
    w.export = T.oracle_sorted_export(w.m)
    for got, want in zip(w.export, H.sorted_export_of(T.world_contents())):
        assert got.tobytes() == want.tobytes()
    w.model = H.SessionModel(w.export)
    w.cases = T.all_cases(w.m, w.model)
    yield w
    w.m.close()


def ranking(w, c):
    return w.model.ranking(c.sess, H.SIM_COSINE, 0.0, None, c.excl, T.DENY)


def test_plan_agrees_with_the_sim_files_need(oracle_mod):
    from tests.test_gpu_cf_sim import LDS_SLOTS, need
    o = oracle_mod.Oracle()
    ops = H.world_ops()
    o.apply(1, *ops)
    o.apply(3, *H.dead_cells(ops))
    assert o.row_info(H.HOT)[0] == 16384 and o.row_info(11)[0] == 64 and o.row_info(12)[0] == 512
    seen = set()
    for s in H.all_sessions():
        for E in (0, 9):
            n, p = need(o, s, E), T.plan(o, s, E)
            if not any(o.row_info(a) for a in s):
                assert p is None and T.need_of(o, s, E) == 0               # no row: no table (need() still counts L + E)
                continue
            assert T.need_of(o, s, E) == n
            assert p == ((T.LDS, T.rec_lg(n, 6)) if n <= LDS_SLOTS else (T.GLOBAL, T.rec_lg(n, 13)))
            seen.add(p[0])
    assert seen == {T.LDS, T.GLOBAL} and LDS_SLOTS == T.REC_LDS_SLOTS
    assert T.plan(o, [H.HOT], 0, scope=list(range(65))) == (T.REFUSED, None) and T.plan(o, [H.HOT], 0, scope=list(range(64)))[0] == T.GLOBAL
    hot = o.row_info(H.HOT)[0]
    long = [H.HOT] * 3 + [H.ABSENT] * 8190                                 # above REC_DEDUP_MAX a repeated row counts again ...
    assert T.need_of(o, long) == 3 * hot + 8193 and T.need_of(o, long[2:]) == hot + 8191
    assert T.need_of(o, long, cells=1000) == 1000 + 8193                   # ... and the sum is cut to the arena's cells
    o.close()


def test_the_world_holds_the_row_sizes_the_cases_stand_on(world):
    w = world
    for a, slots in T.EXPECTED_SLOTS.items():
        assert w.m.row_info(a)[0] == slots, a
    assert all(w.m.row_info(int(a))[0] == 16 for a in T.ITEM16)
    assert len(w.m.list_rows()) < 5000
    assert max(c.want[1] for cs in w.cases.values() for c in cs if c.want) == 15        # the largest table: 32768 slots


def test_every_case_stands_where_it_claims_and_its_table_is_never_full(world):
    w = world
    names = [c.name for cs in w.cases.values() for c in cs]
    assert len(set(names)) == len(names)
    total = 0
    for cs in w.cases.values():
        for c in cs:
            lg, keys = T.check_case(w.m, w.model, c)
            if c.want and c.want[0] == T.GLOBAL:
                total += 1 << lg
    assert total < T.REC_GROUP_SLOTS                                       # one group: the mixed batch's global sessions share one buffer


def test_tier_cut_and_size_steps(world):
    w = world
    a, b, c, d = w.cases["cut"]
    assert [x.need for x in (a, b, c, d)] == [4095, 4096, 4097, 4097]
    assert [x.want for x in (a, b, c, d)] == [(T.LDS, 12), (T.LDS, 12), (T.GLOBAL, 13), (T.GLOBAL, 13)]
    assert len(c.excl) == len(b.excl) + 1 and c.sess == b.sess and len(d.sess) == len(b.sess) + 1 and d.excl == b.excl
    r = ranking(w, a)
    assert len(r) > 200 and all(ranking(w, x) == r for x in (b, c, d))     # the added ids are no candidates
    assert a.sess[0] == a.sess[1] and a.sess.count(a.sess[2]) == 2         # an adjacent repeat and a later one
    steps = w.cases["steps"]
    assert [x.need for x in steps] == [64, 65, 2048, 2049, 8192, 8193, 16384, 16385]
    assert [x.want for x in steps] == [(T.LDS, 6), (T.LDS, 7), (T.LDS, 11), (T.LDS, 12), (T.GLOBAL, 13), (T.GLOBAL, 14), (T.GLOBAL, 14),
                                       (T.GLOBAL, 15)]
    assert [(1 << x.want[1]) // T.REC_SEG for x in steps[4:]] == [2, 4, 4, 8]          # k_rec_gl_merge's lists
    for lo, hi in zip(steps[::2], steps[1::2]):
        assert ranking(w, lo) == ranking(w, hi) and len(ranking(w, lo)) > 0


def test_load(world):
    w = world
    for c, need in zip(w.cases["load"], (4096, 8192)):
        lg, keys = T.check_case(w.m, w.model, c)
        assert c.need == need == 1 << lg and w.m.row_info(c.sess[0])[0] == 16
        free = (1 << lg) - keys.size
        assert 1 <= free <= 16 and T.load(w.model, c.sess, c.excl, lg) > 0.996         # full to within the row's free slots
        targets, inside, (start, length) = T.load_targets(w.model, c, lg)
        assert length > 500 and len(inside) >= 8 and not set(inside) & set(keys.tolist())
        occ = T.occupied(keys, lg)
        assert all(T.run_end(occ, int(T.home(np.uint32(b), lg))) > 0 for b in inside)  # their probes start on filled slots
        assert len(ranking(w, c)) >= 3


def test_wrap(world):
    w = world
    for c, lg in zip(w.cases["wrap"], (12, 13)):
        got, keys = T.check_case(w.m, w.model, c)
        assert got == lg
        homes = T.home(keys, lg)
        assert int((homes >= (1 << lg) - 16).sum()) >= 80                  # the chain: homed in the last 16 slots
        back, front = T.wrap_run(T.occupied(keys, lg))
        assert back >= 16 and front >= 64                                  # ... it crosses the last slot and goes on from slot 0
        chain = set(keys[homes >= (1 << lg) - 16].tolist())
        r = [b for b, _ in ranking(w, c)]
        assert len(chain & set(r)) >= 30 and len(chain & set(c.sess)) == 16 and len(chain & set(T.CHAIN_EXCL.tolist()) & set(c.excl)) == 32
        assert len(chain & set(T.DENY)) == 12 and not chain & set(T.DENY) & set(r)
        absent = [t for t in c.targets if t in T.CHAIN_ABSENT.tolist()]
        assert len(absent) == 2 and not set(absent) & set(keys.tolist())   # rank targets that hash into the chain and are not there
        near = [b for b in T.NEAR_COLS.tolist() if b in r[:64]]
        assert len(near) == 24                                             # candidates in the last 64 slots of a segment, all in the top 64
        # the exclusion ids are in the table before any row is read, and WRAP's other columns are homed behind these slots: a slot of
        # the last 64 in front of the chain that only fills when NEAR_COLS go in holds one of them, whatever the order
        size = 1 << lg
        before = T.occupied(keys[~np.isin(keys, T.NEAR_COLS)], lg)
        assert int((T.occupied(keys, lg) & ~before)[size - 64:size - 16].sum()) >= 8


def test_dedup_edge(world):
    w = world
    a, b = w.cases["dedup"]
    assert len(a.sess) == T.REC_DEDUP_MAX and len(b.sess) == T.REC_DEDUP_MAX + 1
    assert a.need == 4096 + 8192 and b.need == 3 * 4096 + 8193 and a.want == (T.GLOBAL, 14) and b.want == (T.GLOBAL, 15)
    once = w.model.ranking([T.HUB], H.SIM_COSINE, 0.0, None, (), T.DENY)
    assert ranking(w, a) == once and ranking(w, b) == once and len(once) > 1000


def test_global_tasks(world):
    w = world
    small, mid, one_seg, few = w.cases["tasks"]
    assert all(w.m.row_info(a)[0] == 16 < T.REC_CHUNK for a in small.sess) and small.want == (T.GLOBAL, 13)
    assert sorted(w.m.row_info(a)[0] for a in mid.sess) == [512, 512, 1024, 1024] and mid.want == (T.GLOBAL, 13)
    for c, in_seg1 in ((one_seg, 0), (few, 5)):
        lg, keys = T.check_case(w.m, w.model, c)
        assert lg == 13
        occ = T.occupied(keys, lg)
        r = [b for b, _ in ranking(w, c)]
        seg = [(int(T.home(np.uint32(b), lg)), T.run_end(occ, int(T.home(np.uint32(b), lg)))) for b in r]
        assert all(h // T.REC_SEG == (h + d) // T.REC_SEG for h, d in seg)             # no candidate can be pushed across the cut
        assert [h // T.REC_SEG for h, _ in seg].count(1) == in_seg1 and len(r) == 70 + in_seg1
        assert all(h < T.REC_SEG for h, _ in seg[:64])                                 # the 64 best: all of segment 0


def test_endings(world):
    w = world
    by = {c.name: c for c in w.cases["endings"]}
    for tier in (T.LDS, T.GLOBAL):
        assert len(ranking(w, by["64 candidates, " + tier])) == 64 and len(ranking(w, by["65 candidates, " + tier])) == 65
        r = ranking(w, by["tie at 63 .. 65, " + tier])
        assert [b for b, _ in r[62:65]] == [T.T1, T.T2, T.M32] and len({s for _, s in r[62:65]}) == 1
        assert r[61][1] > r[62][1] > r[65][1]
        r = ranking(w, by["tie at 62 .. 64, " + tier])
        assert [b for b, _ in r[61:64]] == [T.T1, T.T2, T.M32] and r[60][1] > r[61][1] > r[64][1]
        assert by["[0, a], " + tier].sess[0] == 0 and by["[a, 0, 0], " + tier].sess[1:3] == [0, 0] and by["[0], " + tier].sess[0] == 0
        assert len(ranking(w, by["[0], " + tier])) >= 5
        assert all(by[n + tier].want[0] == tier for n in ("64 candidates, ", "[0], ", "tie at 63 .. 65, "))
    assert by["64 candidates in a 4096-slot LDS table"].want == (T.LDS, 12)
    for c in w.cases["targets"]:
        n = int(c.name.split()[0])
        r = [b for b, _ in ranking(w, c)]
        assert len(c.targets) == n and c.targets[-1] in r
        present = sum(t in r for t in c.targets)
        assert 30 <= present <= n - 28                                     # present and absent ones mixed
    assert {c.want[0] for c in w.cases["targets"]} == {T.LDS, T.GLOBAL}


def test_the_group_cap_binds_and_the_scope_bites(world):
    w = world
    arr = T.group_map()
    c = w.cases["cut"][0]
    r = ranking(w, c)
    assert G.survivors(r, arr, T.GROUP_CAP)[:64].tolist() != list(range(64))           # the grouped call's result is not the top-k's
    scope = T.scope_map()
    kept = [b for b, _ in r if b < scope.size and int(scope[b]) in T.SCOPE_LIST]
    assert 0 < len(kept) < len(r)
    assert any(b in set(x for x, _ in r) for b in T.fill_list()) and T.M32 in T.fill_list()
