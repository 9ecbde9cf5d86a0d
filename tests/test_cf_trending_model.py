"""CPU: the model of smatrix_cf_trending (tests/cf_trending_helpers.py trending()) over trending_world() meets the hard cases that
tests/test_gpu_cf_trending.py relies on -- shown on the model alone, without a GPU:
  * for each measure and each (num, den, shrink) of PARAMS the cuts at n = 64 and n = 4096 fall inside tie groups: the entry behind
    the cut has the score of the last entry kept, so the id bytes of the key decide;
  * the floor matters under 1/7 and 3/7, and D == 0 occurs with shrink 0;
  * the world holds every kind of row the issue names, and the 64-bit product is needed;
  * a group's RATIO scores differ in the lowest mantissa byte alone, and an n exists that cuts it;
  * with an empty base and GAIN the model is cf_fill_helpers.popular;
  * ZSCORE, RATIO and GAIN order the world differently."""
import numpy as np
import pytest

from tests import cf_fill_helpers as F
from tests import cf_trending_helpers as T


@pytest.fixture(scope="module")
def world():
    w = T.trending_world()
    w["e_now"], w["e_base"] = T.export_of(w["now"]), T.export_of(w["base"])
    return w


def all_of(w, measure, num=1, den=1, shrink=0.0, **kw):
    return T.trending(w["e_now"], w["e_base"], 1 << 20, measure, num, den, shrink, **kw)


@pytest.mark.parametrize("measure", T.MEASURES)
@pytest.mark.parametrize("num,den,shrink", T.PARAMS)
def test_the_cuts_fall_inside_tie_groups(world, measure, num, den, shrink):
    ids, score, _, _ = all_of(world, measure, num, den, shrink)
    assert ids.size > 4096 + 100
    for n in (64, 4096):
        assert score[n - 1] == score[n], (n, score[n - 1], score[n])
        assert score[n - 2] == score[n - 1] or score[n] == score[n + 1]      # a group of three at least
        assert ids[n - 1] < ids[n]
    twins = set(world["twins"].tolist())
    assert ids[63] in twins and ids[64] in twins                          # one T, one B: the id bytes alone decide at 64


def test_the_floor_matters_and_a_zero_denominator_occurs(world):
    now, base = world["now"]["totals"], world["base"]["totals"]
    B = np.array([base.get(x, 0) for x in now], np.uint64)
    for num, den in ((1, 7), (3, 7)):
        assert ((B * np.uint64(num)) % np.uint64(den) != 0).sum() > 5000    # E is a floor for most ids
        ids, _, tot, exp = all_of(world, "ratio", num, den)
        assert all(int(e) == base.get(int(x), 0) * num // den and now[int(x)] == int(t) for x, t, e in zip(ids[:500], tot[:500], exp[:500]))
    ids, score, tot, exp = all_of(world, "zscore")
    zero = exp == 0
    assert zero.sum() > 900 and (score[zero] == tot[zero]).all()           # D == 0 counts as 1: the score is the gain itself
    assert 0xFFFFFFFF * 3 > 1 << 32 and int(world["big"][4]) in all_of(world, "gain", 3, 7)[0].tolist()   # B * num needs 64 bits
    assert int(world["big"][4]) not in all_of(world, "gain")[0].tolist()   # E > T at 1/1


def test_the_world_holds_every_kind_of_row(world):
    now, base = world["now"]["totals"], world["base"]["totals"]
    T_of = np.array(list(now.values()), np.uint64)
    B_of = np.array([base.get(x, 0) for x in now], np.uint64)
    assert (T_of == B_of).sum() > 100 and (T_of < B_of).sum() > 100         # E == T and E > T
    assert len(now) > 10000 and world["absent"].size > 900
    assert not set(world["absent"].tolist()) & set(base) and set(world["absent"].tolist()) <= set(now)
    assert not set(world["only_base"].tolist()) & set(now) and set(world["only_base"].tolist()) <= set(base)
    for name in ("base_no_head", "base_zeroed", "base_empty"):
        assert world[name].size >= 3 and set(world[name].tolist()) <= set(now) and not set(world[name].tolist()) & set(base)
    assert not set(world["now_no_candidates"].tolist()) & set(now)
    for m in (now, base):
        assert sum(1 for v in m.values() if v >= 1 << 24) >= 5 and 0xFFFFFFFF in m.values()
    assert now[0xFFFFFFFF] == 0xFFFFFFFF                                   # the largest id: its key's low word is 0
    ids = all_of(world, "gain")[0]
    assert not set(ids.tolist()) & set(world["only_base"].tolist()) and 0 not in ids.tolist()
    assert world["twins"].size == 300 and len({(now[x], base[x]) for x in world["twins"].tolist()}) == 1


def test_a_group_differs_in_the_lowest_mantissa_byte_alone(world):
    ids, score, _, _ = all_of(world, "ratio")
    at = np.flatnonzero(np.isin(ids, world["close"]))
    assert at.size == T.N_CLOSE and (np.diff(at) == 1).all() and 64 < at[0] and at[-1] < 4096
    raw = score[at].view(np.uint8).reshape(-1, 8)                          # little-endian: byte 0 is the lowest
    assert len({r[1:].tobytes() for r in raw}) == 1 and len(set(raw[:, 0].tolist())) == T.N_CLOSE


def test_an_empty_base_under_gain_is_the_popular_model(world):
    empty = F.export_of_totals({})
    deny = world["twins"][::3].tolist()
    for n, kw in ((64, {}), (4096, {}), (500, dict(min_total=9)), (4096, dict(deny=deny))):
        ids, score, tot, exp = T.trending(world["e_now"], empty, n, "gain", **kw)
        p_ids, p_tot = F.popular(world["e_now"], n, **kw)
        assert ids.tolist() == p_ids.tolist() and tot.tolist() == p_tot.tolist() and not exp.any()
        assert score.tolist() == p_tot.astype(np.float64).tolist()


def test_the_measures_order_the_world_differently(world):
    lists = {m: all_of(world, m)[0] for m in T.MEASURES}
    assert sorted(lists["gain"].tolist()) == sorted(lists["zscore"].tolist()) == sorted(lists["ratio"].tolist())
    for a, b in (("gain", "zscore"), ("gain", "ratio"), ("ratio", "zscore")):
        for n in (64, 4096):
            assert lists[a][:n].tolist() != lists[b][:n].tolist(), (a, b, n)
    for num, den, shrink in T.PARAMS[1:]:
        assert all_of(world, "zscore", num, den, shrink)[0][:4096].tolist() != lists["zscore"][:4096].tolist()


def test_min_gain_min_total_and_deny_cut(world):
    c = all_of(world, "zscore", min_gain=8)[0].size
    assert 100 < c < 4000
    assert all_of(world, "zscore", min_gain=0)[0].size == all_of(world, "zscore")[0].size      # 0 is 1
    assert 100 < all_of(world, "zscore", min_total=10)[0].size < all_of(world, "zscore")[0].size
    some = all_of(world, "ratio")[0][:600:2].tolist()
    assert not set(all_of(world, "ratio", deny=some)[0].tolist()) & set(some)
