"""CPU: the host model of row ownership (tests/shard_router_helpers.py) against everything else on the host that states
who owns a row -- the library's host entry points, Placement.owner, the numpy partitioner of tests/sharded_worker.py and
the table HipPartitioner.set_placement builds.  tests/test_gpu_shard_router.py then holds the kernels to the same model."""
import os
import subprocess

import numpy as np
import pytest

from tests import shard_router_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = (1, 2, 3, 7, 8, 63, 64)
EDGE_IDS = np.array([0, 1, 1 << 31, H.M32], np.uint32)


@pytest.fixture(scope="module")
def lib():
    from libsmatrix_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", _lib.CSRC], check=True)
    return _lib.load()


def hard_ids(case, rng, n_random=64):
    return np.concatenate([case.special_ids(), EDGE_IDS, rng.integers(0, 1 << 32, n_random, dtype=np.uint64).astype(np.uint32)])


def test_hash_round_trip():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32), EDGE_IDS])
    assert H.shard_unmix(H.shard_mix_np(x)).dtype == np.uint32
    assert (H.shard_unmix(H.shard_mix_np(x)) == x).all()
    assert (H.shard_mix_np(H.shard_unmix(x)) == x).all()
    assert int(H.shard_mix_np(int(H.shard_unmix(12345)))) == 12345                       # scalars too


def test_host_entry_points_agree(lib):
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32), EDGE_IDS])
    assert [lib.smatrix_shard_mix(int(a)) for a in x] == H.shard_mix_np(x).tolist()
    assert [lib.smx_fmix32(int(a)) for a in x] == H.fmix32_np(x).tolist()
    for slots in (1, 2, 16, 64, 1024):
        assert [lib.smatrix_place_slot(int(a), slots) for a in x] == H.place_slot_np(x, slots).tolist()
    for world in range(1, 65):
        # the ids on both sides of every boundary of the equal ranges, and a few hundred others
        ids = np.concatenate([H.boundary_ids(H.equal_range_cuts(world)), x[:300], EDGE_IDS])
        want = H.owner_model(ids, world)
        assert [lib.smatrix_shard_of(int(a), world) for a in ids] == want.tolist(), world
        assert want.min() >= 0 and want.max() < world
        # equal ranges ARE a set of cut points: the two branches of the model agree
        assert (H.owner_model(ids, world, H.equal_range_cuts(world)) == want).all(), world


def test_unmix_stands_on_the_cut(lib):
    """the ids the boundary builder makes hash to c - 1, c, c + 1 -- by the LIBRARY's hash, not only the model's"""
    cuts = [0, 1, 77777, 1 << 31, H.M32 - 1, H.M32]
    ids = H.boundary_ids(cuts)
    got = {lib.smatrix_shard_mix(int(a)) for a in ids[:-2]}
    assert got == {h for c in cuts for h in (c - 1, c, c + 1) if 0 <= h <= H.M32}


@pytest.mark.parametrize("world", WORLDS)
def test_model_against_placement_owner(lib, world):
    from libsmatrix_amd.sharded import Placement
    rng = np.random.default_rng(3)
    cases = H.placement_cases(world)
    want_names = {"none", "place", "both", "wrap", "tab16_one_row", "tab1024_half_full"}
    if world > 1:
        want_names |= {"cuts", "cuts_first_zero", "cuts_last_max"}
    if world > 2:
        want_names |= {"cuts_equal_neighbours"}
    assert set(cases) == want_names
    for name, c in cases.items():
        ids = hard_ids(c, rng)
        pl = Placement(world, c.cuts, c.place)
        assert [pl.owner(int(a), lib) for a in ids] == c.owner(ids).tolist(), name
    if world > 1:
        assert cases["cuts_first_zero"].cuts[0] == 0 and cases["cuts_last_max"].cuts[-1] == H.M32
        ids = hard_ids(cases["cuts_first_zero"], rng, 2000)
        assert (cases["cuts_first_zero"].owner(ids) > 0).all()                         # shard 0 owns nothing
        top = H.shard_unmix(np.array([H.M32 - 1, H.M32], np.uint64))
        assert cases["cuts_last_max"].owner(top).tolist() == [world - 2, world - 1]      # the last shard: one hash
    if world > 2:
        cuts = cases["cuts_equal_neighbours"].cuts
        dup = [r + 1 for r in range(len(cuts) - 1) if cuts[r] == cuts[r + 1]]
        assert dup                                                                       # shard r + 1 has an empty range
        ids = hard_ids(cases["cuts_equal_neighbours"], rng, 5000)
        assert not np.isin(cases["cuts_equal_neighbours"].owner(ids), dup).any()
    if world > 1:                                                                        # "a placed row beats its range"
        c = cases["both"]
        keys = np.array(sorted(c.place), np.uint32)
        assert (c.owner(keys) != H.owner_model(keys, world, c.cuts)).all()


@pytest.mark.parametrize("world", WORLDS)
def test_suite_stand_in_agrees(world):
    """the numpy partitioner the gloo tests route with (tests/sharded_worker.py owner_np)"""
    from libsmatrix_amd.sharded import Placement
    from tests.sharded_worker import owner_np
    rng = np.random.default_rng(4)
    for name, c in H.placement_cases(world).items():
        ids = hard_ids(c, rng, 1000)
        pl = None if name == "none" else Placement(world, c.cuts, c.place)
        assert (owner_np(ids, world, pl) == c.owner(ids)).all(), name


def test_table_construction(lib):
    """place_table lays the rows out as HipPartitioner.set_placement does (built on a CPU device)"""
    import torch
    from libsmatrix_amd.sharded import HipPartitioner, Placement
    part = HipPartitioner(torch.device("cpu"))
    for world in (2, 64):
        for name, c in H.placement_cases(world).items():
            part.set_placement(Placement(world, c.cuts, c.place))
            if not c.place:
                assert part.place is None and part.place_slots == 0
                continue
            assert part.place_slots == c.slots, name
            got = part.place.numpy().view(np.uint32)
            assert (got == H.place_table(c.place, part.place_slots, world)).all(), name
            if c.cuts is not None:
                assert part.cuts.numpy().view(np.uint32).tolist() == c.cuts
    # the chain of the "wrap" case really starts in the last slot and wraps
    c = H.placement_cases(8)["wrap"]
    tab, keys = c.table(), list(c.place)
    assert tab[[15, 0, 1], 0].tolist() == keys and (tab[[15, 0, 1], 1] == np.array([c.place[k] + 1 for k in keys])).all()
    assert tab[2, 1] == 0 and (H.place_slot_np(np.array(keys), 16) == 15).all()
    assert H.place_slot_np(np.array(c.absent), 16).tolist() == [0, 1, 15] and not set(c.absent) & set(keys)


@pytest.mark.parametrize("world", WORLDS)
def test_gpu_inputs_meet_the_preconditions(world):
    """every placement the GPU tests hand to a kernel: at least half of the table's slots empty, owners < world"""
    for name, c in H.placement_cases(world).items():
        tab = c.table()
        if tab is None:
            assert c.slots == 0 and not c.place
            continue
        assert tab.shape == (c.slots, 2) and c.slots <= 1024 and c.slots & (c.slots - 1) == 0
        assert 2 * int((tab[:, 1] == 0).sum()) >= c.slots, name
        assert int(tab[:, 1].max()) <= world, name                                       # (the table holds owner + 1)
        assert int((tab[:, 1] != 0).sum()) == len(c.place)
    assert len(H.placement_cases(world)["tab1024_half_full"].place) == 512


def test_builders_refuse_unsafe_tables():
    """a full table hangs the look-up of an absent id, an owner >= world writes outside the kernels' LDS: never built"""
    with pytest.raises(ValueError):
        H.place_table({i + 1: 0 for i in range(9)}, 16, 2)                               # more than half full
    with pytest.raises(ValueError):
        H.place_table({i + 1: 0 for i in range(16)}, 16, 2)                              # full
    with pytest.raises(ValueError):
        H.place_table({5: 2}, 16, 2)                                                     # owner == world
    with pytest.raises(ValueError):
        H.place_table({5: 64}, 16)                                                       # owner == MAX_SHARDS
    with pytest.raises(ValueError):
        H.place_table({5: 0}, 24, 2)                                                     # not a power of two
    with pytest.raises(ValueError):
        H.place_table({5: 0}, 2048, 2)
    with pytest.raises(ValueError):
        H.Case("bad", 2, None, {5: 2}, 16)
    with pytest.raises(ValueError):
        H.Case("bad", 3, [5, 4])                                                         # descending cut points
    with pytest.raises(ValueError):
        H.owner_model(np.array([1], np.uint32), 65)
    with pytest.raises(ValueError):
        H.owner_model(np.array([1], np.uint32), 3, [1])                                  # world - 1 cut points, no fewer
    assert H.place_table({i + 1: 1 for i in range(8)}, 16, 2).shape == (16, 2)           # exactly half: allowed


def test_two_owner_waves_builder():
    rng = np.random.default_rng(5)
    for world in (2, 8, 64):
        c = H.placement_cases(world)["both"]
        x = H.two_owner_waves(64 * 9 + 17, c, rng)
        own = np.sort(c.owner(x)[:64 * 9].reshape(9, 64), axis=1)
        assert ((np.diff(own, axis=1) != 0).sum(axis=1) == 1).all()                      # exactly two owners per wave
