"""The model of a LONG probe -- an op whose key does not sit at its home cell -- at the constants of kernels/ops.hpp (the lane's budget,
k_get_clu, the hint table, coop_probe's window and bitmap phases) and of kernels/layout.hpp (HOME_LG, BIG_LG), shared by
tests/test_probe_model.py (no GPU: every constant against its source line, every case's claims on the oracle's own slot dump) and
tests/test_gpu_probe_edges.py (the kernels).

A probe is the reference's (src/smatrix.c:363-380): from y % size, cell by cell, to the first cell that holds y or is empty.  The
kernels examine the same cells in the same order but in PHASES, and each phase has an exact first and last distance from home:

    hinted (a clustered matrix: k_get_clu, k_apply<OP, true>, the retry kernels)
        the lane        d = 0 .. HINT_BUDGET                         hand-over at home + HINT_BUDGET + 1
        the window      d = HINT_BUDGET + 1 .. HINT_BUDGET + WINDOW  4 x 64 cells in one step
        the bitmap      d > HINT_BUDGET + WINDOW   rows of >= 2^HOME_LG cells: 64 words (4096 cells) per group, the cells whose bit is
                        clear numbered in probe order and examined 64 (writers) or 256 (k_get_clu) at a time
    hint-less (k_apply<OP>)
        the lane        d = 0 .. PROBE_BUDGET, then windows of WINDOW cells to the end of the turn

A case is a ROW: a run of dense keys at home, a pile of keys h + j * size behind it -- key i of the pile is inserted i-th and lands on
the first free cell behind the run, so its distance is chosen by choosing h --, optionally a second run the pile flows around, in the
middle of the table or ending at its last slot (the pile then lies on slots 0, 1, ...).  The pile is built ONE key per row and call:
such a table is the same bytes on the oracle and on the GPU, whatever order a batch takes.  Nothing here is believed: the model test
reads every distance back from the oracle's slot dump."""
import functools

import numpy as np

from tests.write_batch_helpers import OP_GET, OP_SET, OP_INCR, OP_DECR, u32     # noqa: F401  (re-exported)

# ---- the constants, each stated once (tests/test_probe_model.py holds them to the source) --------------------------------------------
HINT_BUDGET = 8            # ops.hpp SMX_HINT_BUDGET: cells BEHIND home a lane examines when the matrix has a hint table
PROBE_BUDGET = 48          # ops.hpp SMX_PROBE_BUDGET: the same without one
WINDOW = 256               # coop_probe: `done += 256`, four 64-lane loads per step; the bitmap phase starts at pb + 256
HOME_LG = 12               # layout.hpp SMX_HOME_LG: rows of >= 2^12 cells carry an at-home bitmap
BIG_LG = 15                # layout.hpp SMX_BIG_LG: rows of >= 2^15 cells keep sub-counter lines between cells and bitmap
WORD = 64                  # cells per bitmap word
GROUP_WORDS = 64           # coop_probe: `wd += 64` -- 64 words (4096 cells) per group
CAND_U1 = 64               # candidates per trip, U = 1 (writers, k_apply<GET, true>)
CAND_U4 = 256              # ... U = SMX_GET_WALK_U = 4 (k_get_clu)
HINT_WAYS = 2              # entries per hint slot
FAR_JOIN_MIN = 1 << 16     # smx_runtime.hip: the pass in front of prep runs for batches of n >= (1u << 16)
FAR_ROW_LG = 13            # ops.hpp SMX_FAR_ROW_LG: the far join indexes rows of >= 2^13 cells
AGG_MIN = 1024             # Matrix::agg_min: the lane-per-op kernel below it

SIZES = (2048, 4096, 16384, 32768)     # no bitmap; HOME_LG itself (one group); several groups; BIG_LG
PILE = 400                 # keys in a row's pile


def first_bitmap_distance(hinted=True):
    return (HINT_BUDGET if hinted else PROBE_BUDGET) + WINDOW + 1


def classes(hinted, size):
    """name -> distance from home of the classes a kernel family has on a row of `size` cells"""
    b = HINT_BUDGET if hinted else PROBE_BUDGET
    c = {"home": 0, "lane last": b, "window first": b + 1, "window last": b + WINDOW, "behind the window": b + WINDOW + 1}
    if hinted:
        c["lane first"] = 1
        # the word the bitmap walk starts in (coop_probe masks it from bit start & 63): the key on the bit just before `start` is the
        # window's last cell, the key on bit `start & 63` the walk's first -- one word holds both as long as start & 63 != 0
        c["start word, bit before"] = b + WINDOW
        c["start word, first bit"] = b + WINDOW + 1
        if size >= 4 << HOME_LG:
            # the bitmap walk starts in the word of home + b + 1 + WINDOW and takes GROUP_WORDS words per group: from this distance
            # on a key lies in the second group whatever bit the walk started at
            c["second group"] = b + 1 + WINDOW + GROUP_WORDS * WORD
    else:
        c["second window last"] = b + 2 * WINDOW
        c["third window first"] = b + 2 * WINDOW + 1
    return c


# exact distances the pile holds (pile index -> distance): both families' classes, and four keys at the very front of the pile whose
# walk -- when the run ends at the last slot -- crosses slot size-1 -> 0 inside the lane's cells (1, 8, 9) and inside the window (100)
SPECIAL = {0: 1, 1: 8, 2: 9, 5: 100}
SPECIAL.update({270 + i: d for i, d in enumerate((1, 8, 9, 48, 49, 264, 265, 304, 305, 560, 561))})
# every other pile key has the run's FIRST cell as its home: key i is reached after exactly i cells that are not at home
GROUP_EDGES = (CAND_U1 - 1, CAND_U1, CAND_U1 + 1, CAND_U4 - 1, CAND_U4, CAND_U4 + 1)
ABSENT_D = (0, 1, 8, 9, 48, 49, 264, 265, 304, 305, 560, 561)      # ... and the whole stretch (home = the run's first cell)


# ---- reading a slot dump --------------------------------------------------------------------------------------------------------------
def distances(slots):
    """row_slots -> (key, slot, distance) of every non-empty cell, distance = (slot - key) & mask"""
    s = np.asarray(slots, np.uint32)
    at = np.flatnonzero((s[:, 0] != 0) | (s[:, 1] != 0)).astype(np.uint32)
    key = s[at, 0]
    return key, at, (at - key) & np.uint32(s.shape[0] - 1)


def probe_end(slots, y):
    """where the reference's probe for y ends: the first cell from home that holds y or is empty (y == 0: whose key field is 0,
    quirk Q1) -> (slot, distance, found)"""
    s = np.asarray(slots, np.uint32)
    size = s.shape[0]
    home = int(y) & (size - 1)
    order = (home + np.arange(size)) & (size - 1)
    k, v = s[order, 0], s[order, 1]
    stop = (k == 0) if y == 0 else (k == y) | ((k == 0) & (v == 0))
    d = int(np.argmax(stop))
    assert stop[d], "neither the key nor a free cell"
    return int(order[d]), d, bool(k[d] == y and (y != 0 or v[d] != 0))


def start_bit(size, y, hinted=True):
    """bit `start & 63` of the word the bitmap walk for y starts in"""
    return ((int(y) & (size - 1)) + first_bitmap_distance(hinted)) & (WORD - 1)


def not_home_before(slots, y, hinted=True):
    """how many cells that are not at home (empty, or holding a displaced key: the cells the bitmap walk examines) lie between the
    start of the bitmap phase and the end of y's probe; None when the probe ends before that phase"""
    s = np.asarray(slots, np.uint32)
    size = s.shape[0]
    _, d, _ = probe_end(s, y)
    d0 = first_bitmap_distance(hinted)
    if d < d0 or size < 1 << HOME_LG:
        return None
    home = int(y) & (size - 1)
    cells = (home + np.arange(d0, d)) & (size - 1)
    at_home = ((s[cells, 0] & np.uint32(size - 1)) == cells) & ((s[cells, 0] != 0) | (s[cells, 1] != 0))
    return int((~at_home).sum())


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def value_of(key):
    return ((np.asarray(key, np.uint64) * np.uint64(2654435761) >> np.uint64(7)) & np.uint64(0x7FFFFFFF)).astype(np.uint32) | np.uint32(1)


class Case:
    """one row.  run: dense keys at home on [a, a + r); second: another such run 300 cells behind the first (the pile fills the gap
    and goes on behind it); wrap: the run ends at slot size - 1.  r = size/4 + 2 keys bring the row to `size` cells on their own; with
    the pile it holds fewer than size/2 + 1, and the difference is the room for the absent-key inserts of the GPU tests."""
    GAP, RUN2 = 300, 100

    def __init__(self, row, size, wrap=False, second=False):
        self.row, self.size, self.wrap, self.second = row, size, wrap, second
        S, r = size, size // 4 + 2
        self.a = a = S - r if wrap else S // 4 + 37            # (middle: a & 63 == 37 -- the walk never starts on a word's first bit)
        self.r = r
        occ = np.zeros(S, bool)
        occ[(a + np.arange(r)) % S] = True
        run = (a + np.arange(r)) % S
        if second:
            run2 = (a + r + self.GAP + np.arange(self.RUN2)) % S
            occ[run2] = True
            run = np.concatenate([run, run2])
        assert (run != 0).all()
        self.run = run.astype(np.uint32)                       # key == slot: at home at this size, and the only keys when it is reached
        pile, want = [], {}
        t = (a + r) % S
        for i in range(PILE):
            while occ[t]:
                t = (t + 1) % S
            stretch = (t - a) % S
            d = SPECIAL.get(i, stretch)
            assert 0 < d <= stretch
            home = (t - d) % S
            key = home + (i + 1) * S
            occ[t] = True
            pile.append(key); want[key] = (t, d)
        self.pile = np.asarray(pile, np.uint32)
        self.pile_at = want                                    # key -> (slot, distance) as planned; the model test reads it back
        while occ[t]:
            t = (t + 1) % S
        self.end = t                                           # the first free cell behind everything
        stretch = (t - a) % S
        self.absent_d = tuple(d for d in ABSENT_D if d <= stretch) + (stretch,)
        self.absent = np.asarray([(t - d) % S + (PILE + 50 + k) * S for k, d in enumerate(self.absent_d)], np.uint32)
        self.n_keys = self.run.size + PILE
        self.room = S // 2 + 1 - self.n_keys                   # new keys the row takes before it doubles

    @property
    def name(self):
        return "%d%s%s" % (self.size, " wrap" if self.wrap else "", " two runs" if self.second else "")

    def claims(self, hinted):
        """the distances this row must hold present keys at, for one kernel family"""
        c = dict(classes(hinted, self.size))
        return {n: d for n, d in c.items() if d <= self.r + PILE - 1}


@functools.lru_cache(maxsize=None)
def cases():
    out, row = [], 1
    for size in SIZES:
        for wrap in (False, True):
            out.append(Case(row, size, wrap)); row += 1
    out.append(Case(row, 16384, False, second=True))
    return tuple(out)


MISSING_ROWS = (901, 902, 0x7FFFFFFF)


def steps(cs=None, how="steps"):
    """the calls that build the rows -> [(op, x, y, v)]: the runs of all rows in one batch (every key at home: one layout in any
    order), then pile key i of every row in call i.  how == "one batch": everything in ONE call (the layout is then the batch's own)"""
    cs = cases() if cs is None else cs
    x = np.concatenate([np.full(c.run.size, c.row, np.uint32) for c in cs])
    y = np.concatenate([c.run for c in cs])
    out = [(OP_INCR, x, y, value_of(y))]
    rows = np.asarray([c.row for c in cs], np.uint32)
    for i in range(PILE):
        k = np.asarray([c.pile[i] for c in cs], np.uint32)
        out.append((OP_INCR, rows, k, value_of(k)))
    if how == "one batch":
        p = np.random.default_rng(7).permutation(sum(s[1].size for s in out))
        return [(OP_INCR,) + tuple(np.concatenate([s[j] for s in out])[p] for j in (1, 2, 3))]
    return out


def queries(cs=None, every=97):
    """every pile key, every absent key, the runs' first and last keys and one in `every`, (row, 0), and rows that do not exist"""
    cs = cases() if cs is None else cs
    xs, ys = [], []
    for c in cs:
        run1 = c.run[:c.r]
        keys = np.concatenate([c.pile, c.absent, run1[:2], run1[-2:], c.run[::every], c.run[-2:], [0]]).astype(np.uint32)
        xs.append(np.full(keys.size, c.row, np.uint32)); ys.append(keys)
    for r in MISSING_ROWS:
        ys.append(np.asarray([0, 1, cs[0].pile[3]], np.uint32)); xs.append(np.full(3, r, np.uint32))
    return np.concatenate(xs), np.concatenate(ys)


def far_keys(cs=None, hinted=True):
    """(x, y) of the pile keys whose planned distance lies behind the first window: what walks with the wave and is remembered"""
    cs = cases() if cs is None else cs
    d0 = first_bitmap_distance(hinted)
    xy = [(c.row, k) for c in cs for k in c.pile.tolist() if c.pile_at[k][1] >= d0]
    return np.asarray([p[0] for p in xy], np.uint32), np.asarray([p[1] for p in xy], np.uint32)


def grow_batch(o, cs=None):
    """one batch that doubles every row once: as many new keys as bring it to size/2 + 2, each at home in a free cell of the OLD
    table (read from the oracle's dump) -> (x, y, v)"""
    cs = cases() if cs is None else cs
    xs, ys = [], []
    for c in cs:
        size, used = o.row_info(c.row)
        s = np.asarray(o.row_slots(c.row))
        free = np.flatnonzero((s[:, 0] == 0) & (s[:, 1] == 0))
        free = free[free != 0][-(size // 2 + 2 - used):]                    # (from the far end: away from the pile)
        assert free.size == size // 2 + 2 - used
        xs.append(np.full(free.size, c.row, np.uint32)); ys.append(free.astype(np.uint32))
    x, y = np.concatenate(xs), np.concatenate(ys)
    return x, y, value_of(y)


N_ABSENT = len(ABSENT_D) + 1
ABSENT_PICK = (N_ABSENT - 1, ABSENT_D.index(265), ABSENT_D.index(264), ABSENT_D.index(9), ABSENT_D.index(8), 0)     # where a short run of inserts starts


def absent_batch(o, k, cs=None):
    """class k of ABSENT_D (k == len(ABSENT_D): the whole stretch) as ONE new key per row -- no order to take --, at that distance
    from the first free cell behind the row's stretch AS IT STANDS in the oracle's dump -> (x, y, [probe_end of each key]); the key's
    multiplier is the row's used counter: no key is made twice"""
    cs = cases() if cs is None else cs
    x, y, ends = [], [], []
    for c in cs:
        size, used = o.row_info(c.row)
        assert used <= size // 2, "the row would double"
        s = np.asarray(o.row_slots(c.row))
        end, stretch, found = probe_end(s, c.a + (PILE + 20) * size)
        assert not found
        d = ABSENT_D[k] if k < len(ABSENT_D) else stretch
        key = (end - d) % size + (PILE + 100 + used) * size
        e = probe_end(s, key)
        assert e == (end, d, False)
        x.append(c.row); y.append(key); ends.append(e)
    return np.asarray(x, np.uint32), np.asarray(y, np.uint32), ends
