"""A host model of row ownership for the multi-GPU router (include/smatrix_shard.h, PLACEMENT), numpy only.

Restated from the definitions in libsmatrix_amd/csrc/kernels/io_router.hpp and layout.hpp, not imported from any other
stand-in of the suite: the tests compare the kernels, the host entry points, Placement.owner and the numpy partitioner of
tests/sharded_worker.py against THIS file.

The builders at the end make the inputs at which an owner function goes wrong (ids that stand exactly on a cut point, probe
chains that wrap, waves with two owners).  Every placement they hand out satisfies the two preconditions of a device table
(at least half of the slots empty, owners below `world`); place_table() refuses anything else, because a table that breaks
them must never reach a kernel: a full table makes the look-up of an absent id spin, and an owner >= world indexes past the
kernels' 64 LDS counters.
"""
import numpy as np

M32 = 0xFFFFFFFF
MAX_SHARDS = 64
PLACE_MAX_SLOTS = 1024
C1, C2 = 0x85EBCA6B, 0xC2B2AE35             # murmur3's fmix32 multipliers (layout.hpp fmix32)
SALT = 0x9E3779B9                           # io_router.hpp shard_mix
C1_INV, C2_INV = pow(C1, -1, 1 << 32), pow(C2, -1, 1 << 32)


def _u64(x):
    """any integer array or scalar (int32 views included) -> a fresh uint64 array of its 32-bit patterns"""
    return np.array(x).astype(np.uint64) & np.uint64(M32)


def fmix32_np(x):
    h = _u64(x)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(C1)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(C2)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def shard_mix_np(x):
    """shard_mix(x) = fmix32(x ^ 0x9E3779B9)"""
    return fmix32_np(_u64(x) ^ np.uint64(SALT))


def place_slot_np(x, slots):
    """home slot of x in a placement table of `slots` (a power of two) entries: fmix32(x) & (slots - 1)"""
    return fmix32_np(x) & np.uint32(slots - 1)


def shard_unmix(h):
    """the row id whose shard_mix is exactly h.  x ^= x >> 16 undoes itself; x ^= x >> 13 is undone by
    x ^ (x >> 13) ^ (x >> 26); the multipliers are odd, so they have inverses modulo 2^32."""
    h = _u64(h)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(C2_INV)) & np.uint64(M32)
    h ^= (h >> np.uint64(13)) ^ (h >> np.uint64(26))
    h = (h * np.uint64(C1_INV)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return (h ^ np.uint64(SALT)).astype(np.uint32)


def check_placement(world, cuts=None, place=None, slots=None):
    """raises ValueError unless (world, cuts, place[, slots]) may be handed to a partition kernel"""
    if not 1 <= world <= MAX_SHARDS:
        raise ValueError("world %r is not in 1..%d" % (world, MAX_SHARDS))
    if cuts is not None:
        cuts = [int(c) for c in cuts]
        if len(cuts) != world - 1:
            raise ValueError("%d cut points for %d shards" % (len(cuts), world))
        if any(not 0 <= c <= M32 for c in cuts) or any(a > b for a, b in zip(cuts, cuts[1:])):
            raise ValueError("cut points must ascend within 0 .. 2^32 - 1")
    for x, o in (place or {}).items():
        if not 0 <= int(x) <= M32:
            raise ValueError("row id %r is not a 32-bit id" % (x,))
        if not 0 <= int(o) < world:
            raise ValueError("row %d is placed on shard %r of %d" % (x, o, world))
    if slots is not None and (slots or place):
        if slots < 1 or slots > PLACE_MAX_SLOTS or slots & (slots - 1):
            raise ValueError("%r slots: not a power of two <= %d" % (slots, PLACE_MAX_SLOTS))
        if 2 * len(place or {}) > slots:
            raise ValueError("%d rows leave fewer than half of %d slots empty" % (len(place), slots))


def owner_model(x, world, cuts=None, place=None):
    """owner of every id of x: its entry in `place` ({x: owner}) if it has one; else, with cuts, the number of cut points
    <= shard_mix(x); else floor(shard_mix(x) * world / 2^32)."""
    check_placement(world, cuts, place)
    x = _u64(x)
    h = shard_mix_np(x).astype(np.uint64)
    if cuts is None:
        own = ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)
    else:
        own = np.zeros(x.shape, np.int64)
        for c in cuts:
            own += h >= np.uint64(int(c))
    if place:
        keys = np.array(sorted(place), dtype=np.uint64)
        vals = np.array([place[int(k)] for k in keys], dtype=np.int64)
        at = np.minimum(np.searchsorted(keys, x), keys.size - 1)
        own = np.where(keys[at] == x, vals[at], own)
    return own


def place_table(place, slots, world=MAX_SHARDS):
    """the {x, owner + 1} table of include/smatrix_shard.h: slot of x, linear probing, rows inserted in the dict's order,
    owner + 1 == 0 marks an empty slot.  uint32 [slots, 2]."""
    check_placement(world, None, place, slots)
    tab = np.zeros((slots, 2), np.uint32)
    for x, o in place.items():
        i = int(place_slot_np(int(x), slots))
        while tab[i, 1]:
            i = (i + 1) & (slots - 1)
        tab[i] = (int(x), int(o) + 1)
    return tab


# ---- builders for the hard inputs ---------------------------------------------------------------------------------------
def equal_range_cuts(world):
    """the cut points equal ranges amount to: the smallest hash h with floor(h * world / 2^32) == r, r = 1 .. world - 1"""
    return [-((-r << 32) // world) for r in range(1, world)]


def boundary_ids(cuts):
    """ids whose hash is c - 1, c and c + 1 for every cut point c, ids of hash 0 and 2^32 - 1, and the ids 0 and 2^32 - 1"""
    hs = {0, M32}
    for c in cuts or ():
        hs.update(h for h in (int(c) - 1, int(c), int(c) + 1) if 0 <= h <= M32)
    ids = shard_unmix(np.array(sorted(hs), dtype=np.uint64))
    return np.concatenate([ids, np.array([0, M32], np.uint32)])


def ids_with_home_slot(slot, slots, count, start=1):
    """the first `count` ids >= start whose home slot in a table of `slots` entries is `slot` (found by search)"""
    found, at = [], start
    while len(found) < count:
        ids = np.arange(at, at + 65536, dtype=np.uint64)
        found.extend(ids[place_slot_np(ids, slots) == slot].tolist())
        at += 65536
    return [int(i) for i in found[:count]]


def make_cuts(world, kind, rng):
    """world - 1 ascending cut points.  kind: "random"; "equal_neighbours" (two shards with an empty range, world >= 3);
    "first_zero" (shard 0 owns nothing); "last_max" (the last shard owns the hash 2^32 - 1 alone)"""
    if world < 2:
        raise ValueError("one shard has no cut points")
    cuts = sorted(int(c) for c in rng.integers(1, M32, world - 1))
    if kind == "equal_neighbours":
        if world < 3:
            raise ValueError("equal neighbours need two cut points")
        cuts[(world - 1) // 2] = cuts[(world - 1) // 2 - 1]
        if world >= 5:
            cuts[-1] = cuts[-2]
    elif kind == "first_zero":
        cuts[0] = 0
    elif kind == "last_max":
        cuts[-1] = M32
    elif kind != "random":
        raise ValueError(kind)
    check_placement(world, cuts)
    return cuts


class Case:
    """one placement and the ids that are hard for it"""

    def __init__(self, name, world, cuts=None, place=None, slots=0, absent=()):
        check_placement(world, cuts, place, slots)
        self.name, self.world, self.cuts, self.place, self.slots = name, world, cuts, dict(place or {}), slots
        self.absent = [int(a) for a in absent]             # ids NOT in the table whose probe runs through occupied slots

    def owner(self, x):
        return owner_model(x, self.world, self.cuts, self.place)

    def table(self):
        return place_table(self.place, self.slots, self.world) if self.place else None

    def special_ids(self):
        cuts = self.cuts if self.cuts is not None else equal_range_cuts(self.world)
        return np.concatenate([boundary_ids(cuts), np.array(sorted(self.place), np.uint32), np.array(self.absent, np.uint32)])

    def ids(self, n, rng):
        """n ids: random 32-bit ids, a tenth of them placed rows, every special id once (as many as fit)"""
        x = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if self.place and n:
            keys = np.array(sorted(self.place), np.uint32)
            hot = rng.random(n) < 0.1
            x[hot] = keys[rng.integers(0, keys.size, int(hot.sum()))]
        sp = self.special_ids()
        if sp.size >= n:
            return sp[:n].copy()
        x[rng.choice(n, sp.size, replace=False)] = sp
        return x


def _moved_rows(world, cuts, ids):
    """{x: owner} that places every id on a shard OTHER than the one its range names (world > 1)"""
    own = owner_model(ids, world, cuts)
    step = lambda i: 1 + i % (world - 1) if world > 1 else 0          # 1 .. world - 1: never back to the range owner
    return {int(x): int((o + step(i)) % world) for i, (x, o) in enumerate(zip(ids, own))}


def placement_cases(world, seed=0):
    """the placements the GPU tests use for `world` shards, by name"""
    rng = np.random.default_rng(1000 * seed + world)
    rnd_ids = lambda k: np.unique(rng.integers(1, M32, 2 * k, dtype=np.uint64))[:k].astype(np.uint32)
    cuts = make_cuts(world, "random", rng) if world > 1 else None
    cases = [Case("none", world), Case("place", world, None, _moved_rows(world, None, rnd_ids(8)), 16)]
    if world > 1:
        cases.append(Case("cuts", world, cuts))
        cases.append(Case("cuts_first_zero", world, make_cuts(world, "first_zero", rng)))
        cases.append(Case("cuts_last_max", world, make_cuts(world, "last_max", rng)))
    if world > 2:
        cases.append(Case("cuts_equal_neighbours", world, make_cuts(world, "equal_neighbours", rng)))
    cases.append(Case("both", world, cuts, _moved_rows(world, cuts, rnd_ids(24)), 64))
    cases.append(Case("tab16_one_row", world, cuts, _moved_rows(world, cuts, rnd_ids(1)), 16))
    cases.append(Case("tab1024_half_full", world, cuts, _moved_rows(world, cuts, rnd_ids(512)), 1024))
    # a probe chain that starts in the LAST slot and wraps to slots 0 and 1; absent ids whose home slot lies inside it
    chain = ids_with_home_slot(15, 16, 4)
    inside = ids_with_home_slot(0, 16, 1) + ids_with_home_slot(1, 16, 1) + chain[3:]
    cases.append(Case("wrap", world, cuts, _moved_rows(world, cuts, np.array(chain[:3], np.uint32)), 16, inside))
    return {c.name: c for c in cases}


def two_owner_waves(n, case, rng):
    """n ids in which every full run of 64 (one wave of the kernels) holds exactly two owners, both more than once"""
    pool = np.concatenate([rng.integers(0, 1 << 32, 8192, dtype=np.uint64).astype(np.uint32), case.special_ids()])
    own = case.owner(pool)
    present = np.unique(own)
    if present.size < 2:
        raise ValueError("fewer than two owners to choose from")
    i = np.arange(n)
    w, lane = i // 64, i % 64
    tgt = np.where((lane * 7 + w) % 3 != 0, present[w % present.size], present[(w + 1) % present.size])
    x = np.zeros(n, np.uint32)
    for o in present:
        at = np.nonzero(tgt == o)[0]
        mine = pool[own == o]
        x[at] = mine[rng.integers(0, mine.size, at.size)]
    return x
