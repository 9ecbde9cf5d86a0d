"""GPU (-m gpu): the popular call (include/smatrix_batch.h smatrix_cf_popular / _dev; SparseMatrix.cf_popular, cf_popular_dev).

Expected results: tests/cf_fill_helpers.py popular() over the matrix's own export("sorted"): ids and totals must be equal.  The matrix
is cf_fill_helpers.popular_world(): 10 000 rows of scattered 32-bit ids (65 536 directory slots: 256 workgroups of keys, and the
histograms of as many workgroups add up), totals mostly in 1 .. 50; tests/test_cf_fill_model.py shows, without a GPU, that the cuts
at n = 64 and n = 4096 fall inside tie groups."""
import numpy as np
import pytest

from libsmatrix_amd import POPULAR_MAX, SparseMatrix, _lib
from tests import cf_fill_helpers as F

pytestmark = pytest.mark.gpu

SET, DECR = 1, 3
p32 = lambda a: a.ctypes.data_as(_lib.u32p)                               # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


def build(w, chunks=1, reverse=False):
    m = SparseMatrix()
    x, y, v = w["ops"]
    order = np.arange(x.size)[::-1] if reverse else np.arange(x.size)
    for part in np.array_split(order, chunks):                            # (several batches: another insertion and growth history)
        m.apply_batch(SET, x[part], y[part], v[part], results=False)
    for e in (w["empty"][::-1] if reverse else w["empty"]):
        m.set(e, 0, 0)                                                    # an empty row (quirk Q3)
    m.apply_batch(DECR, *w["zeroed"], results=False)                      # heads decremented to 0
    return m


class World:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["full", "small"])
def world(request):
    w = World()
    w.spec = F.popular_world(request.param)
    w.m = build(w.spec)
    w.export = w.m.export("sorted")
    ids, tot = F.heads_of(w.export)
    assert dict(zip(ids.tolist(), tot.tolist())) == w.spec["totals"]      # the matrix holds what the model test looked at
    for e in w.spec["empty"] + w.spec["no_head"] + w.spec["zeroed"][0].tolist() + [0]:
        assert w.m.row_info(e) is not None                                # rows that are no candidates
    w.n_cand = F.popular(w.export, 1 << 20)[0].size
    yield w
    w.m.close()


def check(got, want, tag):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32
    assert got[0].tolist() == want[0].tolist(), (tag, "ids")
    assert got[1].tolist() == want[1].tolist(), (tag, "totals")


def popular_dev(m, n, deny=None, min_total=1):
    """SparseMatrix.cf_popular_dev on torch tensors, on a stream of its own; the outputs start as junk -> (ids, totals, n_found), whole"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        d_bits, deny_n = None, 0
        if deny is not None:
            from libsmatrix_amd.matrix import _deny_bitmap
            bits, deny_n = _deny_bitmap(deny)
            d_bits = torch.from_numpy(bits.view(np.int32)).to(dev)
        d_ids = torch.full((n,), 0x7a7a7a7a, dtype=torch.int32, device=dev)
        d_tot = torch.full((n,), 0x5b5b5b5b, dtype=torch.int32, device=dev)
        d_nf = torch.full((1,), 77, dtype=torch.int32, device=dev)
        m.cf_popular_dev(n, None if d_bits is None else d_bits.data_ptr(), deny_n, min_total, d_ids.data_ptr(), d_tot.data_ptr(), d_nf.data_ptr(),
                         stream=st)
    st.synchronize()
    return d_ids.cpu().numpy().view(np.uint32), d_tot.cpu().numpy().view(np.uint32), int(d_nf.cpu().numpy().view(np.uint32)[0])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_the_n_most_popular_are_the_models(world, n):
    w = world
    want = F.popular(w.export, n)
    assert want[0].size == n
    got = w.m.cf_popular(n)
    check(got, want, n)
    again = w.m.cf_popular(n)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


def test_n_at_and_above_the_candidate_count_and_a_min_total_that_cuts(world):
    w = world
    assert w.n_cand == F.N_ROWS > POPULAR_MAX
    want = F.popular(w.export, POPULAR_MAX, min_total=50)
    c = want[0].size
    assert 100 < c < 4000 and want[1].min() == 50
    for n in (c - 1, c, c + 1, POPULAR_MAX):
        check(w.m.cf_popular(n, min_total=50), F.popular(w.export, n, min_total=50), ("min_total 50", n))
    check(w.m.cf_popular(64, min_total=0), F.popular(w.export, 64), "min_total 0 is 1")
    top = int(want[1].max())
    check(w.m.cf_popular(10, min_total=top), F.popular(w.export, 10, min_total=top), "the best alone")
    if top < 0xFFFFFFFF:
        assert w.m.cf_popular(10, min_total=top + 1)[0].size == 0


def test_a_deny_bitmap_with_deny_n_below_the_largest_id(world):
    w = world
    best = F.popular(w.export, 600)[0]
    low = best[best < (1 << 28)]
    deny = low[::2].tolist() + [int(low.max()) + 1]                       # (an id without a row closes the bitmap)
    assert 10 < len(deny) and max(deny) < (1 << 28) + 1 < int(best.max())
    for n in (64, 4096):
        want = F.popular(w.export, n, deny=deny)
        assert not set(want[0].tolist()) & set(deny) and int(want[0].max()) > max(deny)
        check(w.m.cf_popular(n, deny=deny), want, ("deny", n))
    ids, tot, nf = popular_dev(w.m, 64, deny=deny, min_total=2)
    want = F.popular(w.export, 64, deny=deny, min_total=2)
    assert nf == 64
    check((ids, tot), want, "deny, dev")


def test_the_dev_flavour_on_its_own_stream_leaves_the_unused_entries(world):
    w = world
    for n, min_total in ((4096, 1), (65, 1), (500, 50)):
        want = F.popular(w.export, n, min_total=min_total)
        ids, tot, nf = popular_dev(w.m, n, min_total=min_total)
        assert nf == want[0].size
        check((ids[:nf], tot[:nf]), want, ("dev", n))
        assert (ids[nf:] == 0x7a7a7a7a).all() and (tot[nf:] == 0x5b5b5b5b).all()
    raw = np.full(500, 9, np.uint32), np.full(500, 9, np.uint32), np.full(1, 9, np.uint32)
    assert w.m._lib.smatrix_cf_popular(w.m._h, None, 0, 50, 500, p32(raw[0]), p32(raw[1]), p32(raw[2])) == 0
    nf = int(raw[2][0])
    assert nf == want[0].size and not raw[0][nf:].any() and not raw[1][nf:].any()        # the host flavour zero-fills


def test_the_same_contents_in_another_order_and_a_pruned_copy_give_the_same_bytes(world):
    w = world
    want = w.m.cf_popular(4096)
    other = build(w.spec, chunks=5, reverse=True)
    copy = w.m.pruned()
    for m in (other, copy):
        got = m.cf_popular(4096)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        m.close()


def test_a_total_set_through_the_scalar_call_counts_at_once():
    w = F.popular_world(True)
    m = build(w)
    before = m.cf_popular(64)
    x = int(before[0][40])
    m.set(x, 0, 100000)                                                   # stays in the host mirror until a batch call writes it back
    newcomer = w["no_head"][0]
    m.set(newcomer, 0, 99999)
    after = m.cf_popular(64)
    assert after[0][:2].tolist() == [x, newcomer] and after[1][:2].tolist() == [100000, 99999]
    check(after, F.popular(m.export("sorted"), 64), "after")
    m.close()


@pytest.mark.parametrize("n", [1, 100, 299])
def test_equal_large_totals_take_the_select_down_into_the_id_bytes(n):
    """About 300 rows of ONE total, 0xFF000001, and five of 0xFF000002: the select starts at digit 7 and the totals decide nothing
    below digit 4, so every cut falls among the id bytes.  The two smallest ids of the five differ in their last byte alone: n = 1
    finds two keys in its bin at digits 3, 2 and 1 and ends at digit 0, after all eight passes."""
    rng = np.random.default_rng(97)
    ids = np.unique(rng.integers(1 << 20, 0xFFFFFFFF, 300, dtype=np.uint64).astype(np.uint32))
    five = np.array([0x00012301, 0x00012302, 0x4d000007, 0x9e3779b9, 0xf0000001], np.uint32)
    assert not np.isin(five, ids).any() and ids.size + five.size > 300
    x = np.concatenate([ids, five])
    m = SparseMatrix()
    m.apply_batch(SET, x, np.zeros(x.size, np.uint32), np.where(np.isin(x, five), 0xFF000002, 0xFF000001).astype(np.uint32), results=False)
    want = F.popular(m.export("sorted"), n)
    assert want[0].size == n and want[0][0] == 0x00012301
    check(m.cf_popular(n), want, ("host", n))
    d_ids, d_tot, nf = popular_dev(m, n)
    assert nf == n
    check((d_ids, d_tot), want, ("dev", n))
    m.close()


def test_an_empty_matrix_and_every_id_denied():
    m = SparseMatrix()
    ids, tot = m.cf_popular(64)
    assert ids.size == 0 and tot.size == 0
    assert popular_dev(m, 4096)[2] == 0
    m.apply_batch(SET, np.array([5, 9, 700], np.uint32), np.zeros(3, np.uint32), np.array([3, 3, 8], np.uint32), results=False)
    check(m.cf_popular(10), (np.array([700, 5, 9], np.uint32), np.array([8, 3, 3], np.uint32)), "three")
    assert m.cf_popular(10, deny=[5, 9, 700, 701])[0].size == 0
    assert popular_dev(m, 10, deny=[5, 9, 700])[2] == 0
    check(m.cf_popular(10, deny=[5, 9]), (np.array([700], np.uint32), np.array([8], np.uint32)), "700 is beyond deny_n")
    m.close()


def test_each_refusal_leaves_the_outputs_as_they_were(world):
    import torch
    w = world
    lib, h = w.m._lib, w.m._h
    bits = np.zeros(4, np.uint32)
    sentinel = lambda: (np.full(8, 0xabcdef, np.uint32), np.full(8, 0x123456, np.uint32), np.full(1, 99, np.uint32))       # noqa: E731
    dev = torch.device("cuda", torch.cuda.current_device())
    d = [torch.from_numpy(a.view(np.int32)).to(dev) for a in sentinel()]
    d_bits = torch.from_numpy(bits.view(np.int32)).to(dev)
    bad = [dict(n=0), dict(n=POPULAR_MAX + 1), dict(deny_n=(1 << 32) + 1, deny=True), dict(deny_n=5, deny=False), dict(null=0), dict(null=1), dict(null=2)]
    for case in bad:
        n, deny_n = case.get("n", 8), case.get("deny_n", 0)
        out = sentinel()
        ptrs = [p32(a) for a in out]
        dptrs = [t.data_ptr() for t in d]
        if "null" in case:
            ptrs[case["null"]] = None
            dptrs[case["null"]] = None
        assert lib.smatrix_cf_popular(h, p32(bits) if case.get("deny") else None, deny_n, 1, n, *ptrs) == -1, case
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out, sentinel())), case
        assert lib.smatrix_cf_popular_dev(h, d_bits.data_ptr() if case.get("deny") else None, deny_n, 1, n, *dptrs, None) == -1, case
        torch.cuda.synchronize()
        assert all(t.cpu().numpy().view(np.uint32).tobytes() == b.tobytes() for t, b in zip(d, sentinel())), case
    out = sentinel()                                                      # deny_n == 2^32 itself is allowed (the bitmap is not read below it here)
    assert lib.smatrix_cf_popular(h, None, 0, 1, 8, *[p32(a) for a in out]) == 0 and out[2][0] == 8
