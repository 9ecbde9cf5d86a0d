"""GPU (-m gpu): the trending call (include/smatrix_batch.h smatrix_cf_trending / _dev; SparseMatrix.cf_trending, cf_trending_dev).

Expected results: tests/cf_trending_helpers.py trending() over the two matrices' own export("sorted").  For EVERY returned entry the
id, the score's bytes, the total and the expected value must be the model's, and their number too.  The matrices are
cf_trending_helpers.trending_world(): two of about 10 000 rows of scattered 32-bit ids (65 536 directory slots: 256 workgroups of
keys); tests/test_cf_trending_model.py shows, without a GPU, that the cuts at n = 64 and n = 4096 fall inside tie groups for each
measure and parameter set, and that the world holds the rows the contract names."""
import ctypes as C

import numpy as np
import pytest

from libsmatrix_amd import POPULAR_MAX, SparseMatrix, _lib
from tests import cf_fill_helpers as F
from tests import cf_sim_helpers as H
from tests import cf_trending_helpers as T

pytestmark = pytest.mark.gpu

SET, DECR = 1, 3
p32 = lambda a: a.ctypes.data_as(_lib.u32p)                               # noqa: E731
pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                    # noqa: E731
CODES = {"gain": 0, "ratio": 1, "zscore": 2}


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


def build(recipe, chunks=1, reverse=False):
    m = SparseMatrix()
    x, y, v = recipe["ops"]
    order = np.arange(x.size)[::-1] if reverse else np.arange(x.size)
    for part in np.array_split(order, chunks):                            # (several batches: another insertion and growth history)
        m.apply_batch(SET, x[part], y[part], v[part], results=False)
    for e in (recipe["empty"][::-1] if reverse else recipe["empty"]):
        m.set(e, 0, 0)                                                    # an empty row (quirk Q3)
    m.apply_batch(DECR, *recipe["zeroed"], results=False)                 # heads decremented to 0
    return m


class World:
    def want(self, n, measure="zscore", num=1, den=1, shrink=0.0, **kw):
        return T.trending(self.e_now, self.e_base, n, measure, num, den, shrink, **kw)


@pytest.fixture(scope="module")
def world():
    w = World()
    w.spec = T.trending_world()
    w.now, w.base = build(w.spec["now"]), build(w.spec["base"])
    w.e_now, w.e_base = w.now.export("sorted"), w.base.export("sorted")
    for m, e, name in ((w.now, w.e_now, "now"), (w.base, w.e_base, "base")):
        ids, tot = F.heads_of(e)
        keep = tot != 0
        assert dict(zip(ids[keep].tolist(), tot[keep].tolist())) == w.spec[name]["totals"]    # the matrices hold what the model test looked at
    for x in w.spec["base_no_head"].tolist() + w.spec["base_zeroed"].tolist() + w.spec["base_empty"].tolist():
        assert w.base.row_info(x) is not None and w.base.get(x, 0) == 0   # rows in base, and no total
    for x in w.spec["absent"][:20].tolist():
        assert w.base.row_info(x) is None
    yield w
    w.now.close()
    w.base.close()


def check(got, want, tag):
    assert [a.dtype for a in got] == [np.uint32, np.float64, np.uint32, np.uint32]
    assert got[0].size == want[0].size, (tag, "n_found", got[0].size, want[0].size)
    assert got[0].tolist() == want[0].tolist(), (tag, "ids")
    assert got[1].tobytes() == want[1].tobytes(), (tag, "scores")
    assert got[2].tolist() == want[2].tolist(), (tag, "totals")
    assert got[3].tolist() == want[3].tolist(), (tag, "expected")


JUNK = (0x7a7a7a7a, 12345.678, 0x5b5b5b5b, 0x3c3c3c3c)


def trending_dev(now, base, n, measure="zscore", num=1, den=1, shrink=0.0, deny=None, min_total=1, min_gain=1):
    """SparseMatrix.cf_trending_dev on torch tensors, on a stream of its own; the outputs start as junk
    -> (ids, scores, totals, expected, n_found), whole"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        d_bits, deny_n = None, 0
        if deny is not None:
            from libsmatrix_amd.matrix import _deny_bitmap
            bits, deny_n = _deny_bitmap(deny)
            d_bits = torch.from_numpy(bits.view(np.int32)).to(dev)
        d_ids = torch.full((n,), JUNK[0], dtype=torch.int32, device=dev)
        d_sc = torch.full((n,), JUNK[1], dtype=torch.float64, device=dev)
        d_tot = torch.full((n,), JUNK[2], dtype=torch.int32, device=dev)
        d_exp = torch.full((n,), JUNK[3], dtype=torch.int32, device=dev)
        d_nf = torch.full((1,), 77, dtype=torch.int32, device=dev)
        now.cf_trending_dev(base, n, measure, num, den, shrink, None if d_bits is None else d_bits.data_ptr(), deny_n, min_total, min_gain,
                            d_ids.data_ptr(), d_sc.data_ptr(), d_tot.data_ptr(), d_exp.data_ptr(), d_nf.data_ptr(), stream=st)
    st.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32)                         # noqa: E731
    return u(d_ids), d_sc.cpu().numpy(), u(d_tot), u(d_exp), int(u(d_nf)[0])


@pytest.mark.parametrize("measure", T.MEASURES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_the_n_best_are_the_models(world, measure, n):
    w = world
    want = w.want(n, measure)
    assert want[0].size == n
    got = w.now.cf_trending(w.base, n, measure)
    check(got, want, (measure, n))
    again = w.now.cf_trending(w.base, n, measure)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("measure", T.MEASURES)
@pytest.mark.parametrize("num,den,shrink", T.PARAMS[1:])
def test_each_scale_and_shrinkage(world, measure, num, den, shrink):
    w = world
    for n in (64, 4096):
        want = w.want(n, measure, num, den, shrink)
        assert want[0].size == n
        check(w.now.cf_trending(w.base, n, measure, num, den, shrink), want, (measure, num, den, shrink, n))


def test_the_default_measure_is_the_z_score_and_minus_zero_shrinks_like_zero(world):
    w = world
    check(w.now.cf_trending(w.base, 500), w.want(500, "zscore"), "defaults")
    check(w.now.cf_trending(w.base, 500, "ratio", shrink=-0.0), w.want(500, "ratio"), "-0.0")


def test_n_at_and_above_the_candidate_count_under_a_min_gain_that_cuts(world):
    w = world
    c = w.want(POPULAR_MAX, "zscore", min_gain=8)[0].size
    assert 100 < c < 4000
    for measure in T.MEASURES:
        for n in (c - 1, c, c + 1, POPULAR_MAX):
            want = w.want(n, measure, min_gain=8)
            assert want[0].size == min(n, c) and (want[2] - want[3]).min() == 8
            check(w.now.cf_trending(w.base, n, measure, min_gain=8), want, ("min_gain 8", measure, n))
    check(w.now.cf_trending(w.base, 64, min_gain=0), w.want(64), "min_gain 0 is 1")
    check(w.now.cf_trending(w.base, 64, "ratio", 3, 7, 0.1, min_gain=0xFFFFFFFF), w.want(64, "ratio", 3, 7, 0.1, min_gain=0xFFFFFFFF), "the largest gain alone")


def test_a_min_total_that_cuts(world):
    w = world
    for measure, n in (("zscore", 4096), ("ratio", 64), ("gain", 2000)):
        want = w.want(n, measure, min_total=10)
        assert want[2].min() >= 10 and 64 <= want[0].size and (n < 4096 or (want[0].size < n and want[2].min() == 10))
        check(w.now.cf_trending(w.base, n, measure, min_total=10), want, ("min_total 10", measure, n))
    check(w.now.cf_trending(w.base, 64, min_total=0), w.want(64), "min_total 0 is 1")
    assert w.now.cf_trending(w.base, 10, min_total=0xFFFFFFFF)[0].tolist() == [0xFFFFFFFF]


def test_the_select_descends_into_the_lowest_score_byte(world):
    """an n that cuts the group whose RATIO scores differ in their lowest mantissa byte alone (tests/test_cf_trending_model.py)"""
    w = world
    ids = w.want(POPULAR_MAX, "ratio")[0]
    at = np.flatnonzero(np.isin(ids, w.spec["close"]))
    assert at.size == T.N_CLOSE
    for n in (int(at[0]) + 1, int(at[3]) + 1, int(at[-1]), int(at[-1]) + 1):
        check(w.now.cf_trending(w.base, n, "ratio"), w.want(n, "ratio"), ("close", n))


def test_fewer_candidates_than_n_and_exactly_n_plus_one():
    n_ops, b_ops = T.three_row_world()
    now, base = SparseMatrix(), SparseMatrix()
    now.apply_batch(SET, *n_ops, results=False)
    base.apply_batch(SET, *b_ops, results=False)
    e_now, e_base = now.export("sorted"), base.export("sorted")
    u, f = (lambda a: np.array(a, np.uint32)), (lambda a: np.array(a, np.float64))
    check(now.cf_trending(base, 10, "gain"), (u([5, 9, 700]), f([20, 20, 8]), u([30, 30, 8]), u([10, 10, 0])), "three, gain")
    check(now.cf_trending(base, 10, "ratio"), (u([700, 5, 9]), f([8, 2, 2]), u([8, 30, 30]), u([0, 10, 10])), "three, ratio")
    for measure in T.MEASURES:
        for n in (1, 2, 3, 4, 4096):                                      # n = 2: exactly n + 1 candidates
            check(now.cf_trending(base, n, measure), T.trending(e_now, e_base, n, measure), ("three", measure, n))
    got = trending_dev(now, base, 10, "zscore")
    assert got[4] == 3 and got[0][:3].tolist() == T.trending(e_now, e_base, 10)[0].tolist()
    assert now.cf_trending(base, 10, deny=[5, 9, 700, 701])[0].size == 0
    check(now.cf_trending(base, 10, "gain", deny=[5, 9]), (u([700]), f([8]), u([8]), u([0])), "700 is beyond deny_n")
    assert base.cf_trending(now, 10, "gain")[0].tolist() == [12]          # the other way round: 12 is the only id that grew
    now.close()
    base.close()


def test_n_plus_one_candidates_in_the_large_world(world):
    w = world
    c = w.want(POPULAR_MAX, "zscore", min_gain=8)[0].size
    for measure in T.MEASURES:
        check(w.now.cf_trending(w.base, c - 1, measure, 3, 7, 10.0, min_gain=8), w.want(c - 1, measure, 3, 7, 10.0, min_gain=8), ("n + 1", measure))


def test_a_deny_bitmap_with_deny_n_below_the_largest_id(world):
    w = world
    best = w.want(600, "zscore")[0]
    low = best[best < (1 << 28)]
    deny = low[::2].tolist() + [int(low.max()) + 1]                       # (an id without a row closes the bitmap)
    assert 10 < len(deny) and max(deny) < (1 << 28) + 1 < int(best.max())
    for measure, n in (("zscore", 64), ("gain", 4096), ("ratio", 4096)):
        want = w.want(n, measure, deny=deny)
        assert not set(want[0].tolist()) & set(deny) and int(want[0].max()) > max(deny)
        check(w.now.cf_trending(w.base, n, measure, deny=deny), want, ("deny", measure, n))
    got = trending_dev(w.now, w.base, 64, "ratio", 1, 7, 0.0, deny=deny, min_total=2)
    assert got[4] == 64
    check(got[:4], w.want(64, "ratio", 1, 7, 0.0, deny=deny, min_total=2), "deny, dev")


def test_an_empty_base_under_gain_is_the_popular_call(world):
    w = world
    empty = SparseMatrix()
    for n, kw in ((64, {}), (4096, {}), (500, dict(min_total=9))):
        ids, sc, tot, exp = w.now.cf_trending(empty, n, "gain", **kw)
        p_ids, p_tot = w.now.cf_popular(n, **kw)
        assert ids.tobytes() == p_ids.tobytes() and tot.tobytes() == p_tot.tobytes() and ids.size == n
        assert not exp.any() and sc.tobytes() == p_tot.astype(np.float64).tobytes()
    empty.close()


def test_an_empty_now_finds_nothing(world):
    empty = SparseMatrix()
    assert all(a.size == 0 for a in empty.cf_trending(world.base, 64))
    assert trending_dev(empty, world.base, 4096)[4] == 0
    empty.close()


def test_the_same_contents_in_another_order_give_the_same_bytes(world):
    w = world
    now2, base2 = build(w.spec["now"], chunks=5, reverse=True), build(w.spec["base"], chunks=3, reverse=True)
    for measure, num, den, shrink in (("zscore", 1, 1, 0.0), ("ratio", 3, 7, 0.1), ("gain", 1, 7, 0.0)):
        want = w.now.cf_trending(w.base, 4096, measure, num, den, shrink)
        for a, b in ((now2, base2), (w.now, base2), (now2, w.base)):
            got = a.cf_trending(b, 4096, measure, num, den, shrink)
            assert all(g.tobytes() == x.tobytes() for g, x in zip(got, want)), measure
    now2.close()
    base2.close()


def test_a_scalar_write_left_in_either_mirror_is_seen_by_the_next_call():
    n_ops, b_ops = T.three_row_world()
    now, base = SparseMatrix(), SparseMatrix()
    now.apply_batch(SET, *n_ops, results=False)
    base.apply_batch(SET, *b_ops, results=False)
    assert now.cf_trending(base, 10, "gain")[0].tolist() == [5, 9, 700]
    assert base.incr(9, 0, 15) == 25                                      # stays in base's host mirror until a batch call writes it back
    ids, sc, tot, exp = now.cf_trending(base, 10, "gain")
    assert (ids.tolist(), sc.tolist(), tot.tolist(), exp.tolist()) == ([5, 700, 9], [20.0, 8.0, 5.0], [30, 8, 30], [10, 0, 25])
    now.set(700, 0, 1000)                                                 # ... and in now's
    base.incr(700, 0, 1)                                                  # a row that base did not have
    got = now.cf_trending(base, 10, "gain")
    check(got, T.trending(now.export("sorted"), base.export("sorted"), 10, "gain"), "after")
    assert got[0].tolist() == [700, 5, 9] and got[3].tolist() == [1, 10, 25]
    now.close()
    base.close()


def test_the_dev_flavour_leaves_the_unused_entries_and_the_host_flavour_zero_fills_them(world):
    w = world
    c = w.want(POPULAR_MAX, "zscore", min_gain=8)[0].size
    for n, measure, min_gain in ((4096, "zscore", 1), (65, "ratio", 1), (c + 100, "gain", 8), (4096, "zscore", 8)):
        want = w.want(n, measure, min_gain=min_gain)
        ids, sc, tot, exp, nf = trending_dev(w.now, w.base, n, measure, min_gain=min_gain)
        assert nf == want[0].size
        check((ids[:nf], sc[:nf], tot[:nf], exp[:nf]), want, ("dev", n, measure))
        assert (ids[nf:] == JUNK[0]).all() and (sc[nf:] == JUNK[1]).all() and (tot[nf:] == JUNK[2]).all() and (exp[nf:] == JUNK[3]).all()
    n = c + 100
    raw = [np.full(n, 9, np.uint32), np.full(n, 9.5), np.full(n, 9, np.uint32), np.full(n, 9, np.uint32), np.full(1, 9, np.uint32)]
    assert w.now._lib.smatrix_cf_trending(w.now._h, w.base._h, 0, 1, 1, 0.0, None, 0, 1, 8, n, p32(raw[0]), pd(raw[1]), p32(raw[2]), p32(raw[3]),
                                          p32(raw[4])) == 0
    assert int(raw[4][0]) == c
    check(tuple(a[:c] for a in raw[:4]), w.want(n, "gain", min_gain=8), "host, raw")
    assert all(a[c:].tobytes() == bytes(a[c:].nbytes) for a in raw[:4])   # the host flavour zero-fills


def test_each_refusal_leaves_the_outputs_as_they_were(world):
    import torch
    w = world
    lib, now, base = w.now._lib, w.now._h, w.base._h
    bits = np.zeros(4, np.uint32)
    sentinel = lambda: (np.full(8, 0xabcdef, np.uint32), np.full(8, 2.5), np.full(8, 0x123456, np.uint32), np.full(8, 0x654321, np.uint32),  # noqa: E731
                        np.full(1, 99, np.uint32))
    ptr = lambda a: pd(a) if a.dtype == np.float64 else p32(a)            # noqa: E731
    dev = torch.device("cuda", torch.cuda.current_device())
    d = [torch.from_numpy(a if a.dtype == np.float64 else a.view(np.int32)).to(dev) for a in sentinel()]
    d_bits = torch.from_numpy(bits.view(np.int32)).to(dev)
    bad = [dict(n=0), dict(n=POPULAR_MAX + 1), dict(base=None), dict(base=now), dict(num=0), dict(den=0), dict(num=0, den=0), dict(num=8, den=7),
           dict(measure=3), dict(measure=-1), dict(shrink=-1.0), dict(shrink=float("nan")), dict(shrink=float("inf")), dict(shrink=-1e-300),
           dict(deny_n=(1 << 32) + 1, deny=True), dict(deny_n=5, deny=False)] + [dict(null=i) for i in range(5)]
    for case in bad:
        args = (case.get("measure", 2), case.get("num", 1), case.get("den", 1), case.get("shrink", 0.0))
        n, deny_n, b = case.get("n", 8), case.get("deny_n", 0), case.get("base", base)
        out = sentinel()
        ptrs = [ptr(a) for a in out]
        dptrs = [t.data_ptr() for t in d]
        if "null" in case:
            ptrs[case["null"]] = None
            dptrs[case["null"]] = None
        assert lib.smatrix_cf_trending(now, b, *args, p32(bits) if case.get("deny") else None, deny_n, 1, 1, n, *ptrs) == -1, case
        assert all(a.tobytes() == s.tobytes() for a, s in zip(out, sentinel())), case
        assert lib.smatrix_cf_trending_dev(now, b, *args, d_bits.data_ptr() if case.get("deny") else None, deny_n, 1, 1, n, *dptrs, None) == -1, case
        torch.cuda.synchronize()
        assert all(t.cpu().numpy().tobytes() == s.tobytes() for t, s in zip(d, sentinel())), case
    out = sentinel()                                                      # what is allowed passes: -0.0, num == den, deny_n == 0
    assert lib.smatrix_cf_trending(now, base, 2, 7, 7, -0.0, None, 0, 1, 1, 8, *[ptr(a) for a in out]) == 0 and out[4][0] == 8
    check(tuple(a for a in out[:4]), w.want(8, "zscore"), "allowed")
    with pytest.raises(ValueError):
        w.now.cf_trending(w.now, 8)


def test_trending_items_fill_cold_sessions_end_to_end():
    """cf_recommend_filled(sessions, k, fill = the trending ids) on the cold sessions of the cf_sim_helpers world equals the same call
    given the model's list"""
    from tests.test_gpu_cf_rank import build_world
    K = 10
    now = build_world()
    base = SparseMatrix()
    rng = np.random.default_rng(7)
    rows = H.POOL[:H.POOL_WITH_ROW]
    base.apply_batch(SET, rows[::2].copy(), np.zeros(rows[::2].size, np.uint32), rng.integers(1, 401, rows[::2].size).astype(np.uint32), results=False)
    e_now, e_base = now.export("sorted"), base.export("sorted")
    sessions, exclude = [s for s, _ in F.FILL_SESSIONS], [e for _, e in F.FILL_SESSIONS]
    for measure, shrink in (("zscore", 0.0), ("ratio", 10.0)):
        got_t = now.cf_trending(base, 1024, measure, 1, 2, shrink, deny=F.DENY)
        want_t = T.trending(e_now, e_base, 1024, measure, 1, 2, shrink, deny=F.DENY)
        check(got_t, want_t, ("fill list", measure))
        assert 100 < want_t[0].size < 1024
        got = now.cf_recommend_filled(sessions, K, got_t[0], exclude=exclude, deny=F.DENY, sim="jaccard", shrink=10.0)
        want = now.cf_recommend_filled(sessions, K, want_t[0].tolist(), exclude=exclude, deny=F.DENY, sim="jaccard", shrink=10.0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        assert (got[2] == K).all()
        empty = sessions.index([])
        assert got[0][empty].tolist() == want_t[0][:K].tolist() and not got[1][empty].any()
        model = H.SessionModel(e_now)
        for s, sess in enumerate(sessions):
            wi, _, wn = F.filled(model, sess, K, H.SIMS["jaccard"], 10.0, want_t[0].tolist(), None, exclude[s], F.DENY)
            assert got[0][s, :len(wi)].tolist() == wi and int(got[3][s]) == wn
    now.close()
    base.close()
