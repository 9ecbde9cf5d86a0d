"""The host model of the session tables of kernels/recommend.hpp -- which tier and size k_rec_bound gives a session, which keys
the table will hold, which slots they fill -- and the world and the cases of tests/test_cf_table_model.py and
tests/test_gpu_cf_table_edges.py (a plain module, no tests of its own).

The RESULTS of a session call are cf_sim_helpers.SessionModel's, over a matrix's own export("sorted"); nothing here says what a call
returns.  This module says where a session STANDS in the table machinery, so that a test which claims to stand on an edge of it
proves so before it runs: plan() is k_rec_bound's decision, keys_of() the distinct keys rec_slot will be given, occupied() the slots
a linear-probing table of 2^lg slots ends with (the SET of filled slots does not depend on the order of insertion), and every case
carries the exact need / tier / lg it was built for.  A case whose table could be full -- len(keys) + 1 > 2^lg: rec_slot would not
end, nor rec_rank_table's probe for an absent target -- is refused by check_case() on the host and never reaches a GPU.

`m` is anything with row_info(x) -> (slots, used) or None: a SparseMatrix, or the oracle.  Row sizes are always read from it."""
import functools

import numpy as np

from tests import cf_sim_helpers as H

M32 = 0xFFFFFFFF

# kernels/recommend.hpp (tests/test_cf_table_model.py holds them to the constexpr lines)
REC_LDS_SLOTS = 4096                         # the LDS tier's largest table; need <= this: LDS
REC_LDS_THREADS = 512
REC_SEG = 4096                               # global tier: slots per top-k segment
REC_GL_MIN_LG = 13                           # global tier: at least 8192 slots
REC_CHUNK = 512                              # global tier: cells of a row per wave task
REC_DEDUP_MAX = 8192                         # sessions up to this length: repeated items found exactly
REC_MAX_LG = 32
REC_SCOPE_MAX = 64
REC_LDS_MIN_LG = 6                           # rec_lg(need, 6): the literal in k_rec_bound
# smx_recommend.inc
REC_GROUP_SLOTS = 1 << 25                    # global-tier slots per group of sessions: below it, one buffer serves every session

SOURCE_CONSTANTS = {"REC_LDS_SLOTS": REC_LDS_SLOTS, "REC_LDS_THREADS": REC_LDS_THREADS, "REC_SEG": REC_SEG, "REC_GL_MIN_LG": REC_GL_MIN_LG,
                    "REC_CHUNK": REC_CHUNK, "REC_MAX_LG": REC_MAX_LG, "REC_SCOPE_MAX": REC_SCOPE_MAX}

LDS, GLOBAL, REFUSED = "lds", "global", "refused"


# ---- fmix32 (kernels/layout.hpp), a bijection of the 32-bit words, and its inverse -----------------------------------------------
C1, C2 = 0x85EBCA6B, 0xC2B2AE35
C1_INV, C2_INV = pow(C1, -1, 1 << 32), pow(C2, -1, 1 << 32)


def _u64(x):
    return np.array(x).astype(np.uint64) & np.uint64(M32)


def fmix32(x):
    h = _u64(x)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(C1)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(C2)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def unfmix32(h):
    """the id whose fmix32 is h"""
    x = _u64(h)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(C2_INV)) & np.uint64(M32)
    x ^= (x >> np.uint64(13)) ^ (x >> np.uint64(26))
    x = (x * np.uint64(C1_INV)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def home(ids, lg):
    """the slot rec_slot starts at in a table of 2^lg slots"""
    return fmix32(ids) & np.uint32((1 << lg) - 1)


FLOOR, CEIL = 1 << 20, 1 << 24               # crafted ids: above every other id of the world, below a 2 MB deny bitmap's end


@functools.lru_cache(maxsize=None)
def _homed(slot, lg):
    hs = (np.arange(1 << (32 - lg), dtype=np.uint64) << np.uint64(lg)) | np.uint64(slot)
    ids = unfmix32(hs)
    return np.sort(ids[(ids >= FLOOR) & (ids < CEIL)])


def ids_homed_at(slot, lg, n, skip=0):
    """n ids in [FLOOR, CEIL) whose home slot in a table of 2^lg slots is `slot` (and slot mod 2^l in every smaller table), ascending,
    after the first `skip` of them: the inverse of fmix32 over every word that ends in `slot`"""
    ids = _homed(int(slot), int(lg))[skip:skip + n]
    assert ids.size == n, (slot, lg, n, skip)
    return ids


# ---- the plan: k_rec_bound ------------------------------------------------------------------------------------------------------
def row_slots_of(m, a):
    info = m.row_info(int(a))
    return int(info[0]) if info else 0


def arena_cells(m):
    """all_cells of k_rec_bound: the cells the arena holds (None for the oracle, which has no arena: the bound is not cut)"""
    return int(m.stats()["arena_mapped"]) // 8 if hasattr(m, "stats") else None


def bound_of(m, sess, cells=None):
    sess = [int(a) for a in sess]
    if len(sess) <= REC_DEDUP_MAX:
        return sum(row_slots_of(m, a) for a in set(sess))
    size = {a: row_slots_of(m, a) for a in set(sess)}
    bound = sum(size[a] for a in sess)                                    # a repeated row is counted again ...
    return bound if cells is None else min(bound, cells)                  # ... and the sum is cut to what the arena can hold


def need_of(m, sess, E=0, cells=None):
    """bound + L + E, or 0 for a session without a row (no table: its count is written by k_rec_bound)"""
    bound = bound_of(m, sess, arena_cells(m) if cells is None else cells)
    return 0 if bound == 0 else min(bound + len(sess) + int(E), 1 << REC_MAX_LG)


def rec_lg(need, min_lg):
    lg = min_lg
    while (1 << lg) < need:
        lg += 1
    return lg


def plan(m, sess, E=0, scope=None, cells=None):
    """(tier, lg) as k_rec_bound decides it; None for a session without a table.  k_rec_scope_bound adds nothing to the need -- an id
    out of scope is claimed like a denied one, by a key the bound has counted --; it only refuses a list beyond REC_SCOPE_MAX"""
    if scope is not None and len(scope) > REC_SCOPE_MAX:
        return (REFUSED, None)
    need = need_of(m, sess, E, cells)
    if need == 0:
        return None
    if need <= REC_LDS_SLOTS:
        return (LDS, rec_lg(need, REC_LDS_MIN_LG))
    return (GLOBAL, rec_lg(need, REC_GL_MIN_LG))


def keys_of(model, sess, excl=()):
    """the distinct non-zero keys the session's table will hold: its items, its exclusion ids, every non-zero column of its distinct
    items' rows (denied and out-of-scope ones are claimed too) -> a sorted uint32 array"""
    keys = set(int(a) for a in sess) | set(int(a) for a in excl)
    for a in set(int(a) for a in sess):
        if a in model.row:
            keys.update(int(b) for b in model.row[a][:, 0])
    keys.discard(0)
    return np.array(sorted(keys), np.uint32)


def load(model, sess, excl, lg):
    return keys_of(model, sess, excl).size / float(1 << lg)


def occupied(keys, lg):
    """the table after every key went in by linear probing -> bool[2^lg].  WHICH slots are filled does not depend on the order"""
    size, mask = 1 << lg, (1 << lg) - 1
    assert len(keys) < size, "the table would be full"
    occ = np.zeros(size, bool)
    for h in home(keys, lg).tolist():
        while occ[h]:
            h = (h + 1) & mask
        occ[h] = True
    return occ


def run_end(occ, slot):
    """the first free slot at or behind `slot`, as a distance (0: `slot` is free).  A key with this home lies within that distance of
    it whatever the order of insertion, and a probe for an absent key with this home makes that many steps"""
    size = occ.size
    d = 0
    while occ[(slot + d) % size]:
        d += 1
        assert d < size
    return d


def wrap_run(occ):
    """(slots filled without a gap up to the last slot, slots filled without a gap from slot 0 on): both > 0 is a probe chain
    across the end of the table"""
    size = occ.size
    back = 0
    while back < size and occ[size - 1 - back]:
        back += 1
    return back, run_end(occ, 0)


def longest_run(occ):
    """(first slot, length) of the longest run of filled slots, the table taken as a ring"""
    size = occ.size
    free = np.flatnonzero(~occ)
    assert free.size
    gaps = np.diff(np.concatenate([free, [free[0] + size]])) - 1
    i = int(np.argmax(gaps))
    return int((free[i] + 1) % size), int(gaps[i])


# ---- the world ----------------------------------------------------------------------------------------------------------------------
# Every id below 2^20 but the crafted ones and 0xFFFFFFFF.  Values 1 .. 5 nearly everywhere: ties are the rule.
#   COLS      600 column ids; the first 400 have a row that holds a head total in 1 .. 400 and nothing else
#   ITEM16    400 items with a head and 5 COLS columns: the smallest row table
#   R64, R512, R1024   two items each with 30 / 200 / 400 COLS and FAR columns
#   HUB, HUB2 1500 / 3000 FAR columns: tables of 4096 and 8192 slots
#   C64, C65  exactly 64 and 65 columns, none of them denied
#   (a pair scores 0 when its value is above sqrt(A) * sqrt(B): the heads of TIE, WRAP and SEGROW are large enough for their values)
#   TIE       62 columns that score high, three -- T1 < T2 < 0xFFFFFFFF -- with one value and one total, five that score low
#   ZERO_ROW  item 0: a head and 12 COLS columns
#   WRAP      CHAIN_COLS, 48 crafted ids homed at the last 16 slots of an 8192-slot table (the last 16 of a 4096-slot one as well),
#             and NEAR_COLS, 24 more homed just in front of them with the row's best values: candidates in a segment's last 64 slots
#   SEGROW    70 crafted columns homed at slots 100 .. 169 of an 8192-slot table (segment 0), 5 homed at 5000 .. 5004 (segment 1)
#   ROWLESS   ids the matrix never sees: padding for sessions and exclusion lists, each worth exactly one slot
COLS = np.arange(20000, 20600, dtype=np.uint32)
COLS_WITH_ROW = 400
FAR = np.arange(30000, 34000, dtype=np.uint32)
ITEM16 = np.arange(1000, 1400, dtype=np.uint32)
R64, R512, R1024 = (2000, 2001), (2100, 2101), (2200, 2201)
HUB, HUB2, C64, C65, TIE, WRAP, SEGROW, ZERO_ROW = 2300, 2301, 2500, 2501, 2600, 2700, 2800, 0
T1, T2 = 40100, 40101
TIE_BETTER = np.arange(40000, 40062, dtype=np.uint32)
TIE_WORSE = np.arange(40200, 40205, dtype=np.uint32)
TIE_TOTAL, TIE_VALUE = 9, 5
ROWLESS = np.arange(600000, 640000, dtype=np.uint32)
ABSENT = 987654                                              # in no row, no list
EXPECTED_SLOTS = {int(ITEM16[0]): 16, R64[0]: 64, R512[0]: 512, R1024[0]: 1024, HUB: 4096, HUB2: 8192}
WRAP_LG = 13
LAST16 = range((1 << WRAP_LG) - 16, 1 << WRAP_LG)
CHAIN_COLS = np.concatenate([ids_homed_at(s, WRAP_LG, 3) for s in LAST16])
CHAIN_DENIED = CHAIN_COLS[::4]                               # 12 of them are denied
CHAIN_ITEMS = np.concatenate([ids_homed_at(s, WRAP_LG, 1, skip=3) for s in LAST16])
CHAIN_EXCL = np.concatenate([ids_homed_at(s, WRAP_LG, 2, skip=4) for s in LAST16])
CHAIN_ABSENT = np.concatenate([ids_homed_at(s, WRAP_LG, 1, skip=6) for s in LAST16])
NEAR_COLS = np.concatenate([ids_homed_at(s, WRAP_LG, 1) for s in range((1 << WRAP_LG) - 56, (1 << WRAP_LG) - 32)])
SEG0_COLS = np.concatenate([ids_homed_at(s, 13, 1) for s in range(100, 170)])
SEG1_COLS = np.concatenate([ids_homed_at(s, 13, 1) for s in range(5000, 5005)])
DENY = sorted(CHAIN_DENIED.tolist() + COLS[5::11].tolist() + FAR[3::17].tolist())
GROUP_MOD, GROUP_CAP = 23, 2                                 # the grouped call's map: id % 23 for the ids below FLOOR, at most 2 a group
SCOPE_MOD, SCOPE_LIST = 5, [0, 1, 3]                         # the scoped call's: id % 5, the listed categories


def world_ops():
    """-> (x, y, v) uint32 arrays: SET ops, every (x, y) once; SCALARS go in behind them through set(b, 0, t)"""
    rng = np.random.default_rng(4096)
    xs, ys, vs = [], [], []

    def row(x, cols, vals, head=None):
        cols, vals = list(cols), list(vals)
        if head is not None:
            cols.append(0); vals.append(head)
        xs.append(np.full(len(cols), x, np.uint32)); ys.append(np.asarray(cols, np.uint32)); vs.append(np.asarray(vals, np.uint32))

    with_row = COLS[:COLS_WITH_ROW]
    xs.append(with_row); ys.append(np.zeros(with_row.size, np.uint32)); vs.append(rng.integers(1, 401, with_row.size).astype(np.uint32))
    for a in ITEM16:
        row(int(a), rng.permutation(COLS)[:5], rng.integers(1, 6, 5), head=int(rng.integers(1, 401)))
    both = np.concatenate([COLS, FAR])
    for ids, n in ((R64, 30), (R512, 200), (R1024, 400)):
        for a in ids:
            row(a, rng.permutation(both)[:n], rng.integers(1, 6, n), head=int(rng.integers(50, 401)))
    row(HUB, rng.permutation(FAR)[:1500], rng.integers(1, 6, 1500), head=350)
    row(HUB2, rng.permutation(FAR)[:3000], rng.integers(1, 6, 3000), head=300)
    free = COLS[~np.isin(COLS, DENY)]                                     # (every column a candidate: none is denied)
    row(C64, rng.permutation(free)[:64], rng.integers(1, 6, 64), head=64)
    row(C65, rng.permutation(free)[:65], rng.integers(1, 6, 65), head=65)
    row(TIE, np.concatenate([TIE_BETTER, [T1, T2, M32], TIE_WORSE]),
        np.concatenate([rng.integers(20, 30, TIE_BETTER.size), [TIE_VALUE] * 3, [1] * TIE_WORSE.size]), head=10000)
    row(ZERO_ROW, rng.permutation(COLS)[:12], rng.integers(1, 6, 12), head=50)
    row(WRAP, np.concatenate([CHAIN_COLS, NEAR_COLS]), np.concatenate([rng.integers(1, 6, CHAIN_COLS.size), rng.integers(6, 10, NEAR_COLS.size)]),
        head=400)
    row(SEGROW, np.concatenate([SEG0_COLS, SEG1_COLS]), np.concatenate([6 + np.arange(SEG0_COLS.size) // 2, [1] * SEG1_COLS.size]), head=10000)
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(vs)


SCALARS = [(T1, 0, TIE_TOTAL), (T2, 0, TIE_TOTAL), (M32, 0, TIE_TOTAL)]


def build(m):
    """the world into an EMPTY matrix: a SparseMatrix (apply_batch) or an oracle (apply), then the scalar sets"""
    x, y, v = world_ops()
    if hasattr(m, "apply_batch"):
        m.apply_batch(1, x, y, v, results=False)
    else:
        m.apply(1, x, y, v)
    for b, y0, t in SCALARS:
        m.set(b, y0, t)


def world_contents():
    """the candidate list (x, y, v) of the finished matrix"""
    x, y, v = world_ops()
    s = np.array(SCALARS, np.uint32)
    return np.concatenate([x, s[:, 0]]), np.concatenate([y, s[:, 1]]), np.concatenate([v, s[:, 2]])


def universe():
    """every id a scoped call can meet as a candidate or in the fill list"""
    x, y, _ = world_contents()
    return sorted(set(x.tolist()) | set(y.tolist()) | set(fill_list()))


def fill_list():
    return [0, int(COLS[0]), int(COLS[7]), ABSENT, int(ROWLESS[0])] + COLS[100:180].tolist() + [int(CHAIN_COLS[1]), M32, 777777]


def group_map():
    return np.arange(FLOOR, dtype=np.uint32) % np.uint32(GROUP_MOD)


def scope_map():
    return np.arange(FLOOR, dtype=np.uint32) % np.uint32(SCOPE_MOD)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
class Case:
    """one session of a test: its items, its exclusion list, the targets cf_rank is asked about (None: default_targets), and what the
    case was built for: want = (tier, lg), need = the exact need (None where only the plan is claimed)"""

    def __init__(self, name, sess, excl=(), want=None, need=None, targets=None):
        self.name, self.sess, self.excl = name, [int(a) for a in sess], [int(a) for a in excl]
        self.want, self.need, self.targets = want, need, None if targets is None else [int(t) for t in targets]

    def __repr__(self):
        return "Case(%s)" % self.name


class Pad:
    """hands out ROWLESS ids, never one twice: the padding ids of a section's cases are distinct, so each is worth exactly one slot"""

    def __init__(self):
        self.at = 0

    def take(self, n):
        assert n >= 0 and self.at + n <= ROWLESS.size, n
        out = ROWLESS[self.at:self.at + n].tolist()
        self.at += n
        return out


def padded(m, pad, name, sess, need, excl=(), targets=None, in_session=0):
    """the session brought to exactly `need` by ROWLESS ids: in_session of them as further positions, the rest as exclusion ids"""
    sess = list(sess) + pad.take(in_session)
    have = need_of(m, sess, len(excl))
    assert have and have <= need, (name, have, need)
    excl = list(excl) + pad.take(need - have)
    tier = LDS if need <= REC_LDS_SLOTS else GLOBAL
    return Case(name, sess, excl, (tier, rec_lg(need, REC_LDS_MIN_LG if tier == LDS else REC_GL_MIN_LG)), need, targets)


def check_case(m, model, c):
    """a case's preconditions: the plan it claims, the exact need, and the condition that keeps every probe finite -- the table
    holds one free slot more than it has keys.  -> (lg, keys)"""
    got = plan(m, c.sess, len(c.excl))
    assert got == c.want, (c.name, got, c.want)
    if c.need is not None:
        assert need_of(m, c.sess, len(c.excl)) == c.need, (c.name, need_of(m, c.sess, len(c.excl)), c.need)
    if got is None:
        return None, np.zeros(0, np.uint32)
    keys = keys_of(model, c.sess, c.excl)
    assert keys.size + 1 <= 1 << got[1], (c.name, keys.size, got)
    return got[1], keys


def default_targets(sess, ranking):
    """the candidates at 0, 1, 63, 64, 65 and the last one, the ids 0, 0xFFFFFFFF and ABSENT, a crafted id no table holds, the session's
    first non-zero item"""
    n = len(ranking)
    at = [i for i in (0, 1, 63, 64, 65, n - 1) if 0 <= i < n]
    return [int(ranking[i][0]) for i in dict.fromkeys(at)] + [0, M32, ABSENT, int(CHAIN_ABSENT[0])] + [a for a in sess if a != 0][:1]


def tier_cut_cases(m, pad):
    base = [R1024[0], R1024[0], R512[0], R64[0], int(ITEM16[3]), R512[0]]         # (an adjacent repeat and a later one)
    a = padded(m, pad, "cut 4095", base, 4095)
    b = Case("cut 4096", a.sess, a.excl + pad.take(1), (LDS, 12), 4096)
    c = Case("cut 4097 by an exclusion id", b.sess, b.excl + pad.take(1), (GLOBAL, 13), 4097)
    d = Case("cut 4097 by a position", b.sess + pad.take(1), b.excl, (GLOBAL, 13), 4097)
    return [a, b, c, d]


def size_step_cases(m, pad):
    out = []
    for need, sess in ((64, [int(ITEM16[0])]), (2048, [R1024[1]]), (8192, [HUB]), (16384, [HUB2, HUB])):
        a = padded(m, pad, "step %d" % need, sess, need)
        tier = LDS if need + 1 <= REC_LDS_SLOTS else GLOBAL
        out += [a, Case("step %d" % (need + 1), a.sess, a.excl + pad.take(1), (tier, a.want[1] + 1), need + 1)]
    return out


def load_cases(m, pad):
    return [padded(m, pad, "load 4096", [int(ITEM16[1])], 4096), padded(m, pad, "load 8192", [int(ITEM16[2])], 8192)]


def wrap_cases(m, pad):
    sess = [WRAP] + CHAIN_ITEMS.tolist()
    targets = [int(CHAIN_ABSENT[5]), int(CHAIN_COLS[1]), int(CHAIN_DENIED[0]), int(CHAIN_ITEMS[2]), int(CHAIN_EXCL[3]), int(NEAR_COLS[0]),
               int(CHAIN_ABSENT[15]), int(CHAIN_COLS[46])]
    return [padded(m, pad, "wrap 4096", sess, 2100, CHAIN_EXCL.tolist(), targets),
            padded(m, pad, "wrap 8192", sess, 4200, CHAIN_EXCL.tolist(), targets)]


def dedup_cases(m, pad):
    """L = REC_DEDUP_MAX and one more: the hub first, padding, the hub twice more at the end.  Exact at 8192 (the hub counts once);
    at 8193 its row counts three times"""
    body = pad.take(REC_DEDUP_MAX - 3)
    size = row_slots_of(m, HUB)
    a = Case("L 8192", [HUB] + body + [HUB, HUB], (), (GLOBAL, rec_lg(size + REC_DEDUP_MAX, 13)), size + REC_DEDUP_MAX)
    b = Case("L 8193", [HUB] + body + pad.take(1) + [HUB, HUB], (), (GLOBAL, rec_lg(3 * size + REC_DEDUP_MAX + 1, 13)),
             3 * size + REC_DEDUP_MAX + 1)
    return [a, b]


def global_task_cases(m, pad):
    small = ITEM16[10:310].tolist()
    return [Case("global, 16-slot rows only", small, (), (GLOBAL, 13), 300 * row_slots_of(m, small[0]) + 300),
            padded(m, pad, "global, 512- and 1024-slot rows", [R512[0], R1024[0], R512[1], R1024[1]], 5000),
            padded(m, pad, "one segment holds all 64", [SEGROW], 8000, SEG1_COLS.tolist()),
            padded(m, pad, "a segment with fewer than k", [SEGROW], 8000)]


def ending_cases(m, pad):
    out = []
    for tier, need in ((LDS, 0), (GLOBAL, 4200)):
        def mk(name, sess, excl=(), targets=None):
            if need == 0:
                n = need_of(m, sess, len(excl))
                return Case("%s, %s" % (name, tier), sess, excl, (LDS, rec_lg(n, REC_LDS_MIN_LG)) if n else None, n or None, targets)
            return padded(m, pad, "%s, %s" % (name, tier), sess, need, excl, targets)
        out += [mk("64 candidates", [C64]), mk("65 candidates", [C65]),
                mk("tie at 63 .. 65", [TIE]), mk("tie at 62 .. 64", [TIE], [int(TIE_BETTER[7])]),
                mk("[0, a]", [0, R64[0]]), mk("[a, 0, 0]", [R64[1], 0, 0]), mk("[0]", [0])]
    out.append(padded(m, pad, "64 candidates in a 4096-slot LDS table", [C64], 4000))
    return out


def rank_target_cases(m, model, pad):
    """64 and 65 targets per tier, present and absent ones mixed, the last one present"""
    out = []
    for tier, sess in ((LDS, [R512[1]]), (GLOBAL, [HUB])):
        r = [b for b, _ in model.ranking(sess, H.SIM_COSINE, 0.0, None, (), DENY)]
        for n in (64, 65):
            absent = ROWLESS[-40:-20].tolist() + CHAIN_ABSENT[:8].tolist() + [0, int(DENY[0]), sess[0]]
            present = r[:20] + r[-(n - 20 - len(absent)):]
            t = [present[i // 2] if i % 2 == 0 else absent[i // 2] for i in range(2 * len(absent))] + present[len(absent):]
            assert len(t) == n and t[-1] in r
            nd = need_of(m, sess)
            out.append(Case("%d targets, %s" % (n, tier), sess, (), (tier, rec_lg(nd, 6 if tier == LDS else 13)), nd, t))
    return out


def all_cases(m, model):
    """every case of the GPU file, by section, built over m's row sizes -> {section: [Case]}"""
    return {"cut": tier_cut_cases(m, Pad()), "steps": size_step_cases(m, Pad()), "load": load_cases(m, Pad()), "wrap": wrap_cases(m, Pad()),
            "dedup": dedup_cases(m, Pad()), "tasks": global_task_cases(m, Pad()), "endings": ending_cases(m, Pad()),
            "targets": rank_target_cases(m, model, Pad())}


def load_targets(model, c, lg, n=12, seed=7):
    """what cf_rank is asked in a load case: the candidates, absent ids crafted to home inside the longest run of filled slots (their
    probe walks the rest of the run), absent ids drawn at random, and ids of the exclusion list"""
    keys = keys_of(model, c.sess, c.excl)
    start, length = longest_run(occupied(keys, lg))
    have = set(keys.tolist())
    inside = []
    for d in range(0, length, max(1, length // n)):
        slot = (start + d) & ((1 << lg) - 1)
        inside += [int(b) for b in ids_homed_at(slot, lg, 4) if int(b) not in have][:1]
    rng = np.random.default_rng(seed)
    rand = [int(b) for b in rng.integers(FLOOR, CEIL, n) if int(b) not in have]
    cand = [int(b) for b in model.row[c.sess[0]][:, 0] if b != 0]
    return cand + inside + rand + c.excl[:3] + c.excl[-3:], inside, (start, length)


# ---- the oracle as a matrix -------------------------------------------------------------------------------------------------------
def oracle_sorted_export(o):
    """the export("sorted") the oracle's contents call for"""
    xs = np.sort(o.list_rows().astype(np.uint32))
    ptr = np.zeros(xs.size + 1, np.uint64)
    parts = [np.zeros((0, 2), np.uint32)]
    for i, x in enumerate(xs.tolist()):
        s = o.row_slots(x)
        ne = s[(s[:, 0] != 0) | (s[:, 1] != 0)]
        parts.append(ne[np.argsort(ne[:, 0], kind="stable")].astype(np.uint32))
        ptr[i + 1] = ptr[i] + np.uint64(ne.shape[0])
    return xs, ptr, np.concatenate(parts)
