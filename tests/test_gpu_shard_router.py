"""GPU (-m gpu): the shard router's kernels (csrc/kernels/io_router.hpp: k_part_count, k_part_offsets, k_part_scatter,
k_unpack, k_gather, k_displaced_rows, owner_of) against the host model of row ownership in tests/shard_router_helpers.py.

The C entry points are called through ctypes with buffers the test owns: every output array has 64 sentinel words on both
sides of the window the call may write.  Every comparison runs over all n ops, in numpy.  The order of the ops INSIDE a
shard's range comes from atomics and is not promised: nothing here asserts it, and no two runs' perm are compared.

What these tests never do (include/smatrix_shard.h, d_place): hand a kernel a full placement table (the look-up of an absent
id would spin) or a table that names an owner >= world (it would index past the 64 LDS counters).  Every table comes from
shard_router_helpers.place_table, which refuses both, and partition() asserts it once more before the upload."""
import ctypes as C

import numpy as np
import pytest

from tests import shard_router_helpers as H

pytestmark = pytest.mark.gpu

PAD = 64
SENT = 0x5EA7C0DE
SENT64 = 0x5EA7C0DE5EA7C0DE
WORLDS = (1, 2, 3, 7, 8, 63, 64)
N_EDGES = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 524287, 524288, 524289, 2 * 524288 + 65)
N_SMALL = (0, 1, 255, 256, 257, 70001)


@pytest.fixture(scope="module")
def G():
    from tests.gpu_adapter import GpuMatrix
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"
    return GpuMatrix


class Router:
    def __init__(self):
        import torch
        from libsmatrix_amd import _lib
        self.torch, self.lib, self.u64p = torch, _lib.load(), _lib.u64p
        self.dev = torch.device("cuda", 0)

    def up(self, a):
        """a host array of 32-bit words -> device"""
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(self.dev)

    def work(self):
        return self.torch.zeros(128, dtype=self.torch.int64, device=self.dev)             # 1024 bytes of scratch


@pytest.fixture(scope="module")
def R(G):
    return Router()


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


class Window:
    """`words` 32-bit words of device memory that a call may write, PAD sentinel words on both sides (and inside, at first)"""

    def __init__(self, R, words):
        self.words = words
        self.buf = R.torch.full((words + 2 * PAD,), SENT, dtype=R.torch.int32, device=R.dev)
        self.ptr = self.buf.data_ptr() + 4 * PAD

    def read(self):
        a = self.buf.cpu().numpy().view(np.uint32)
        assert (a[:PAD] == SENT).all(), "written in front of the window"
        assert (a[PAD + self.words:] == SENT).all(), "written behind the window"
        return a[PAD:PAD + self.words]

    def untouched(self):
        return bool((self.read() == SENT).all())


class Parted:
    pass


def partition(R, packed, x, y, v, case, work=None):
    """one call of smatrix_partition_dev (packed False) or smatrix_partition_packed_dev -> counts, perm and the reordered
    columns, read back through their padded windows"""
    n, world = x.size, case.world
    tab = case.table()
    if tab is not None:                                                                  # the preconditions, once more
        assert 2 * int((tab[:, 1] == 0).sum()) >= case.slots and int(tab[:, 1].max()) <= world
    dx, dy, dv = R.up(x), R.up(y), R.up(v) if v is not None else None
    dtab = R.up(tab) if tab is not None else None
    dcuts = R.up(np.array(case.cuts, np.uint32)) if case.cuts else None
    work = work if work is not None else R.work()
    counts = (C.c_uint64 * (H.MAX_SHARDS + 2))(*([SENT64] * (H.MAX_SHARDS + 2)))
    perm = Window(R, n)
    w = 3 if v is not None else 2
    if packed:
        out = Window(R, n * w)
        rc = R.lib.smatrix_partition_packed_dev(n, ptr(dx), ptr(dy), ptr(dv), world, C.cast(counts, R.u64p), work.data_ptr(),
                                                perm.ptr, out.ptr, ptr(dtab), case.slots if dtab is not None else 0, ptr(dcuts), None)
    else:
        xo, yo, vo = Window(R, n), Window(R, n), Window(R, n)
        rc = R.lib.smatrix_partition_dev(n, ptr(dx), ptr(dy), ptr(dv), world, C.cast(counts, R.u64p), work.data_ptr(), perm.ptr,
                                         xo.ptr, yo.ptr, vo.ptr, ptr(dtab), case.slots if dtab is not None else 0, ptr(dcuts), None)
    R.torch.cuda.synchronize()
    assert rc == 0
    res = Parted()
    assert all(c == SENT64 for c in counts[world:]), "counts written beyond nshards"
    res.counts = np.array(counts[:world], dtype=np.int64)
    res.perm = perm.read().astype(np.int64)
    if packed:
        rec = out.read().reshape(n, w)
        res.xo, res.yo, res.vo = rec[:, 0], rec[:, 1], rec[:, 2] if w == 3 else None
    else:
        res.xo, res.yo = xo.read(), yo.read()
        if v is None:
            assert vo.untouched(), "d_v == NULL, yet d_vo was written"
        res.vo = vo.read() if v is not None else None
    return res


def check_contract(res, x, y, v, own, world):
    """include/smatrix_shard.h, smatrix_partition_dev: counts, perm and the reordered ops against the model's owners"""
    n = x.size
    assert res.counts.tolist() == np.bincount(own, minlength=world).tolist()
    assert res.perm.size == n
    if n == 0:
        return
    assert res.perm.max() < n and (np.bincount(res.perm, minlength=n) == 1).all(), "perm is no permutation of 0 .. n-1"
    starts = np.concatenate([[0], np.cumsum(res.counts)])
    assert ((starts[own] <= res.perm) & (res.perm < starts[own + 1])).all(), "an op outside its owner's range"
    assert (res.xo[res.perm] == x).all() and (res.yo[res.perm] == y).all()
    if v is not None:
        assert (res.vo[res.perm] == v).all()


def check_case(R, case, x, work=None):
    """both entry points, with and without values, against ONE evaluation of the model; the flavours' counts agree"""
    n = x.size
    y = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(H.M32)).astype(np.uint32)
    v = y ^ np.uint32(0xA5A5A5A5)
    own = case.owner(x)
    assert own.size == n and (n == 0 or (own.min() >= 0 and own.max() < case.world))
    counts = []
    for packed in (False, True):
        for vals in (v, None):
            res = partition(R, packed, x, y, vals, case, work)
            check_contract(res, x, y, vals, own, case.world)
            counts.append(res.counts.tolist())
    assert counts[0] == counts[1] == counts[2] == counts[3]
    return np.array(counts[0]), own


@pytest.mark.parametrize("n", N_EDGES)
def test_partition_sizes(R, n):
    """the edges of a wave (64), a workgroup (256), the scatter tile (2048) and the count kernel's grid-stride loop (2048
    workgroups of 256 = 524288 ops a trip; the last size makes a third trip with a ragged tail), each with cut points and
    placed rows whose range owner is another shard"""
    case = H.placement_cases(7)["both"]
    counts, own = check_case(R, case, case.ids(n, np.random.default_rng(100 + n)))
    if n >= 2049:                                                                        # the batch really exercises both
        keys = np.array(sorted(case.place), np.uint32)
        assert (case.owner(keys) != H.owner_model(keys, 7, case.cuts)).all() and np.isin(keys, case.ids(n, np.random.default_rng(100 + n))).all()


@pytest.mark.parametrize("n", (2049, 524289))
@pytest.mark.parametrize("world", WORLDS)
def test_partition_worlds(R, world, n):
    """1 to MAX_SHARDS shards under every placement of the catalogue (at the larger size: the three that differ in kind)"""
    cases = H.placement_cases(world)
    names = list(cases) if n == 2049 else ["none", "both", "wrap"]
    rng = np.random.default_rng(world * 7 + n)
    for name in names:
        case = cases[name]
        x = case.ids(n, rng)
        counts, own = check_case(R, case, x)
        if name == "cuts_first_zero":
            assert counts[0] == 0 and counts.sum() == n                                  # shard 0 owns nothing
        if name == "cuts_last_max":
            assert counts[world - 1] == int((H.shard_mix_np(x) == H.M32).sum()) >= 1     # the last shard: one hash value
        if name == "cuts_equal_neighbours":
            empty = [r + 1 for r in range(world - 2) if case.cuts[r] == case.cuts[r + 1]]
            assert empty and (counts[empty] == 0).all()
        if name == "wrap":
            # the absent ids probe through the wrapped chain and fall through to their range
            absent = np.array(case.absent, np.uint32)
            assert np.isin(absent, x).all() and (case.owner(absent) == H.owner_model(absent, world, case.cuts)).all()
            keys = np.array(sorted(case.place), np.uint32)
            assert np.isin(keys, x).all() and (world == 1 or (case.owner(keys) != H.owner_model(keys, world, case.cuts)).all())


@pytest.mark.parametrize("world", (1, 8, 64))
def test_one_id_repeated(R, world):
    """every lane of every wave names ONE counter: the ballot path of both kernels with a single group"""
    case = H.placement_cases(world)["both"]
    placed = sorted(case.place)[0]
    for xid in (placed, 0, H.M32, 123456789, int(H.shard_unmix(case.cuts[0] if case.cuts else 5))):
        counts, own = check_case(R, case, np.full(2049, xid, dtype=np.uint32))
        assert sorted(counts.tolist())[-1] == 2049 and len(set(own.tolist())) == 1


@pytest.mark.parametrize("world", (2, 8, 64))
def test_two_owners_per_wave(R, world):
    case = H.placement_cases(world)["both"]
    x = H.two_owner_waves(64 * 40 + 17, case, np.random.default_rng(world))
    own = np.sort(case.owner(x)[:64 * 40].reshape(40, 64), axis=1)
    assert ((np.diff(own, axis=1) != 0).sum(axis=1) == 1).all()
    check_case(R, case, x)


def test_work_buffer_reused(R):
    """one d_work for a 64-shard call and then a 2-shard call: the second call's counts are its own"""
    work = R.work()
    rng = np.random.default_rng(7)
    for world in (64, 2, 64, 1):
        case = H.placement_cases(world)["cuts" if world > 1 else "none"]
        check_case(R, case, case.ids(2049, rng), work)


def test_refusals(R):
    """-1 before any launch"""
    lib = R.lib
    work, tab = R.work(), R.torch.zeros((2048, 2), dtype=R.torch.int32, device=R.dev)   # (an all-empty table)
    counts = (C.c_uint64 * 66)()
    cp = C.cast(counts, R.u64p)

    def both(n, nshards, place, slots, real):
        w, c = (work.data_ptr(), cp) if real else (None, None)
        return (lib.smatrix_partition_dev(n, None, None, None, nshards, c, w, None, None, None, None, place, slots, None, None),
                lib.smatrix_partition_packed_dev(n, None, None, None, nshards, c, w, None, None, place, slots, None, None))

    assert both(0, 0, None, 0, True) == (-1, -1)
    assert both(0, 65, None, 0, True) == (-1, -1)
    assert both(1 << 32, 2, None, 0, False) == (-1, -1)
    assert both(0, 2, tab.data_ptr(), 24, True) == (-1, -1)
    assert both(0, 2, tab.data_ptr(), 2048, True) == (-1, -1)
    assert both(0, 2, None, 16, True) == (-1, -1)
    assert both(0, 2, None, 24, False) == (-1, -1) and both(0, 2, None, 2048, False) == (-1, -1)
    assert both(0, 2, tab.data_ptr(), 16, True) == (0, 0) and both(0, 64, None, 0, True) == (0, 0)     # (the neighbours pass)
    # smatrix_unpack_dev / smatrix_gather_dev count in 32 bits as well
    assert lib.smatrix_unpack_dev(1 << 32, 2, None, None, None, None, None) == -1
    assert lib.smatrix_unpack_dev(1 << 32, 3, None, None, None, None, None) == -1
    assert lib.smatrix_gather_dev(1 << 32, None, None, None, None) == -1
    assert lib.smatrix_gather_dev((1 << 32) + 5, None, None, None, None) == -1


@pytest.mark.parametrize("n", N_SMALL)
@pytest.mark.parametrize("width", (2, 3))
def test_unpack(R, width, n):
    rec = np.random.default_rng(n + width).integers(0, 1 << 32, (n, width), dtype=np.uint64).astype(np.uint32)
    drec = R.up(rec.ravel())
    xw, yw, vw = Window(R, n), Window(R, n), Window(R, n)
    assert R.lib.smatrix_unpack_dev(n, width, ptr(drec), xw.ptr, yw.ptr, vw.ptr, None) == 0
    R.torch.cuda.synchronize()
    assert (xw.read() == rec[:, 0]).all() and (yw.read() == rec[:, 1]).all()
    if width == 3:
        assert (vw.read() == rec[:, 2]).all()
    else:
        assert vw.untouched()


@pytest.mark.parametrize("width", (1, 4))
def test_unpack_refuses_other_widths(R, width):
    n = 257
    drec = R.up(np.arange(n * 4, dtype=np.uint32))
    xw, yw, vw = Window(R, n), Window(R, n), Window(R, n)
    assert R.lib.smatrix_unpack_dev(n, width, ptr(drec), xw.ptr, yw.ptr, vw.ptr, None) == -1
    R.torch.cuda.synchronize()
    assert xw.untouched() and yw.untouched() and vw.untouched()


@pytest.mark.parametrize("n", N_SMALL)
def test_gather(R, n):
    """out[i] = src[perm[i]] -- for a permutation, and for a perm with repeats (a gather, not an un-permute)"""
    rng = np.random.default_rng(n)
    src = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    dsrc = R.up(src)
    for perm in (rng.permutation(n).astype(np.uint32), rng.integers(0, max(n, 1), n, dtype=np.uint64).astype(np.uint32)):
        out = Window(R, n)
        dperm = R.up(perm)
        assert R.lib.smatrix_gather_dev(n, ptr(dsrc), ptr(dperm), out.ptr, None) == 0
        R.torch.cuda.synchronize()
        assert (out.read() == src[perm.astype(np.int64)]).all()


def test_displaced_rows(R, G):
    """k_displaced_rows: the rows of a matrix whose equal-range owner is not `rank`"""
    rng = np.random.default_rng(11)
    rows = np.unique(rng.integers(1, H.M32, 3000, dtype=np.uint64).astype(np.uint32))
    rows = rows[rows != SENT]
    g = G()
    g.apply(2, rows, np.ones(rows.size, np.uint32), np.ones(rows.size, np.uint32))
    lib, h = R.lib, g.m._h
    for rank, world in ((0, 1), (0, 2), (1, 2), (5, 8), (63, 64)):
        want = set(rows[H.owner_model(rows, world) != rank].tolist())
        assert (rank, world) == (0, 1) and not want or 0 < len(want) < rows.size
        assert lib.smatrix_displaced_rows(h, rank, world, None, 0) == len(want)
        for cap in (len(want), len(want) // 3, 1):
            cap = min(cap, len(want))
            buf = np.full(len(want) + 2 * PAD, SENT, np.uint32)
            assert lib.smatrix_displaced_rows(h, rank, world, buf.ctypes.data + 4 * PAD, cap) == len(want)   # the FULL count
            got = buf[PAD:PAD + cap].tolist()
            assert len(set(got)) == cap and set(got) <= want, (rank, world, cap)
            assert (buf[:PAD] == SENT).all() and (buf[PAD + cap:] == SENT).all(), "written outside out_x[0 .. cap)"
            if cap == len(want):
                assert set(got) == want
    g.close()


def test_hip_partitioner_wrapper(R):
    """HipPartitioner: set_placement, partition, partition_packed, and back to equal ranges with set_placement(None)"""
    from libsmatrix_amd.sharded import HipPartitioner, Placement
    world, n = 8, 5000
    case = H.placement_cases(world)["both"]
    part = HipPartitioner(R.dev)
    rng = np.random.default_rng(13)
    x = case.ids(n, rng)
    y = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    v = y ^ np.uint32(0x0F0F0F0F)
    dx, dy, dv = R.up(x), R.up(y), R.up(v)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    for pl, own in ((Placement(world, case.cuts, case.place), case.owner(x)), (None, H.owner_model(x, world))):
        part.set_placement(pl)
        res = Parted()
        counts, perm, xo, yo, vo = part.partition(dx, dy, dv, world)
        R.torch.cuda.synchronize()
        res.counts, res.perm, res.xo, res.yo, res.vo = np.array(counts), u32(perm).astype(np.int64), u32(xo), u32(yo), u32(vo)
        check_contract(res, x, y, v, own, world)
        counts2, perm, rec = part.partition_packed(dx, dy, dv, world)
        R.torch.cuda.synchronize()
        rec = u32(rec)
        res.counts, res.perm, res.xo, res.yo, res.vo = np.array(counts2), u32(perm).astype(np.int64), rec[:, 0], rec[:, 1], rec[:, 2]
        check_contract(res, x, y, v, own, world)
        counts3, perm, rec = part.partition_packed(dx, dy, None, world)
        R.torch.cuda.synchronize()
        rec = u32(rec)
        res.counts, res.perm, res.xo, res.yo, res.vo = np.array(counts3), u32(perm).astype(np.int64), rec[:, 0], rec[:, 1], None
        check_contract(res, x, y, None, own, world)
        assert counts == counts2 == counts3
    assert (case.owner(x) != H.owner_model(x, world)).any()                              # the two halves differed


def test_set_placement_refuses_more_than_512_rows(R):
    """smatrix_shard_set_placement: 513 non-empty pairs are answered with -1 like every other bad argument (they used to end
    the process when the device table was sized); the handle keeps the placement it had and goes on routing"""
    from libsmatrix_amd.sharded import NativeShardedMatrix, Placement
    lib = R.lib
    sh = NativeShardedMatrix(None, rank=0, world=1)
    before = {5: 0, 77: 0, 123456: 0}
    sh.set_placement(Placement(1, None, before))
    tab = np.zeros((1024, 2), np.uint32)
    tab[:513, 0], tab[:513, 1] = np.arange(1000, 1513), 1
    assert lib.smatrix_shard_set_placement(sh._h, None, tab.ctypes.data, 1024) == -1
    assert sh.placement.place == before and sh.placement.cuts is None
    with pytest.raises(ValueError):
        sh.set_placement(Placement(1, None, {1000 + i: 0 for i in range(513)}))
    assert sh.placement.place == before

    rng = np.random.default_rng(17)
    n = 20000
    x, y = rng.integers(0, 2000, n, dtype=np.uint32), rng.integers(1, 50, n, dtype=np.uint32)
    key = x.astype(np.uint64) << np.uint64(32) | y
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)

    def incr_then_get():
        dx, dy, dv = R.up(x), R.up(y), R.up(np.ones(n, np.uint32))
        out, outg = R.torch.empty(n, dtype=R.torch.int32, device=R.dev), R.torch.empty(n, dtype=R.torch.int32, device=R.dev)
        sh.apply_dev(2, dx, dy, dv, out)
        sh.apply_dev(0, dx, dy, None, outg)
        R.torch.cuda.synchronize()
        return outg.cpu().numpy().view(np.uint32)

    assert (incr_then_get() == cnt[inv]).all()                                           # a batch still routes
    tab[512] = 0
    assert lib.smatrix_shard_set_placement(sh._h, None, tab.ctypes.data, 1024) == 0      # 512 pairs are accepted
    assert sh.placement.place == {1000 + i: 0 for i in range(512)}
    assert (incr_then_get() == 2 * cnt[inv]).all()
    sh.close()
