"""GPU (-m gpu): state that the clustered write path carries from one round or batch to the next, in the orders of rounds that
make it stale -- checked against the oracle through the C ABI after every batch: per-key return multisets (one amount per key
and batch: the multisets are then the same in every serialisation), the gets, and every row's size, used counter, cells (as a
set), probe invariant and rowlen (tests/cold_soak.check_rows).

* The waiting-key records of a clustered prep ({directory slot, key} of every op whose key was absent) belong to the growth round
  right behind that prep.  A round that defers ops without growing a row leaves them behind; a cold start in the next round
  (insert_pending_keys) inserts those keys itself and then grows rows -- its growth must not take the old records in again (a
  duplicate cell and an over-counted `used`), nor, after the directory grew in between, into whatever row a record's slot names
  now.  The trace (SMATRIX_TRACE_ROUNDS=1) proves that the sequence really ran.
* Clustered mode switched off by quiet scrambled-id batches, rows that double while it is off (nobody keeps the hint table and the
  at-home bitmaps), and the mode on again by dense ids: every key the oracle holds reads back."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OP_GET, OP_INCR, OP_DECR = 0, 2, 3


@pytest.fixture
def G():
    from tests.gpu_adapter import GpuMatrix
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"
    return GpuMatrix


@pytest.fixture
def check_rows(monkeypatch):
    # (tests/cold_soak.py sets a default SMATRIX_COLD_MIN when it is first imported: here that lands in monkeypatch's keeping)
    monkeypatch.setenv("SMATRIX_COLD_MIN", "0")
    from tests.cold_soak import check_rows
    monkeypatch.delenv("SMATRIX_COLD_MIN")
    return check_rows


def write_checked(g, o, check_rows, op, x, y, amount, tag):
    """one write batch on both sides, then its returns, its gets and every row"""
    x = np.asarray(x, np.uint32); y = np.asarray(y, np.uint32)
    v = np.full(x.size, amount, np.uint32)
    a, b = g.apply(op, x, y, v), o.apply(op, x, y, v)
    kk = x.astype(np.uint64) << np.uint64(32) | y
    check_rows(g, o, tag)
    assert (a[np.lexsort((a, kk))] == b[np.lexsort((b, kk))]).all(), (tag, "returns")
    assert (g.apply(OP_GET, x, y) == o.apply(OP_GET, x, y)).all(), (tag, "gets")


# ---- the trace ------------------------------------------------------------------------------------------------------------------
_N = r"deferred=(\d+) grow=(\d+)"
_COLD_ROUND = re.compile(r"\[smatrix\] batch (\d+) cold round \d+ .*?: keys=\d+ " + _N)
_CHAIN = re.compile(r"\[smatrix\] batch (\d+) chain: .*\| after the retry: " + _N)
_ROUND = re.compile(r"\[smatrix\] batch (\d+) round \d+ .*?: ops=\d+ " + _N)
_COLD = re.compile(r"\[smatrix\] batch (\d+) cold start: ")
_DIR = re.compile(r"\[smatrix\] batch (\d+) directory grown: ")


def trace_events(err):
    """the write rounds of a trace, in order: (kind, batch, deferred, grow) with kind round / cold / cold_round / dir"""
    ev = []
    for line in err.splitlines():
        for kind, rx in (("cold_round", _COLD_ROUND), ("round", _CHAIN), ("round", _ROUND), ("cold", _COLD), ("dir", _DIR)):
            mt = rx.search(line)
            if mt:
                g = mt.groups()
                ev.append((kind, int(g[0]), int(g[1]) if len(g) > 1 else 0, int(g[2]) if len(g) > 2 else 0))
                break
    return ev


def stale_record_sequences(err):
    """every cold start whose batch's last round in front of it deferred ops and grew no row, and one of whose cold rounds grew
    rows: [(batch, the directory grew between that round and the cold start)]"""
    ev, out = trace_events(err), []
    for i, (kind, batch, _, _) in enumerate(ev):
        if kind != "cold":
            continue
        j = i - 1
        while j >= 0 and ev[j][0] == "dir":
            j -= 1
        if j < 0 or ev[j][0] != "round" or ev[j][1] != batch or not (ev[j][2] > 0 and ev[j][3] == 0):
            continue
        dir_between = any(e[0] == "dir" for e in ev[j + 1:i])
        k = i + 1
        grew = False
        while k < len(ev) and ev[k][0] in ("cold_round", "dir") and ev[k][1] == batch:
            grew |= ev[k][0] == "cold_round" and ev[k][3] > 0
            k += 1
        if grew:
            out.append((batch, dir_between))
    return out


# ---- the recipes ----------------------------------------------------------------------------------------------------------------
ROWS = (3, 5)          # the clustered rows
K_HOME = 12000         # keys 1..K_HOME at home in each: 2^15 cells, 4385 keys of room below the threshold (src/smatrix.c:346)
N_WRAP = 6000          # new keys per row in the batch of the cold start, more than the room: the row doubles in a cold round
WARM_ROWS = 1 << 20    # the one-key rows of the warm-up batch start here


def setup_cold(monkeypatch, spec):
    monkeypatch.setenv("SMATRIX_CLUSTERED", "1")
    monkeypatch.setenv("SMATRIX_COLD_MIN", "1024")
    monkeypatch.setenv("SMATRIX_COLD_SHARE", "1024")
    monkeypatch.setenv("SMATRIX_TRACE_ROUNDS", "1")
    if spec is None:
        monkeypatch.delenv("SMATRIX_SPEC", raising=False)
    else:
        monkeypatch.setenv("SMATRIX_SPEC", spec)


def fill_and_warm(g, o, check_rows, rng, rows=ROWS, k_home=K_HOME):
    """batch 1: keys 1..k_home at home in every row; batch 2 (warm-up): hits on those keys plus a few hundred one-key rows -- a
    short round-0 remainder, so that the next batch is neither taken for a bulk load nor kept from the chain"""
    x = np.repeat(np.asarray(rows, np.uint32), k_home)
    y = np.tile(np.arange(1, k_home + 1, dtype=np.uint32), len(rows))
    write_checked(g, o, check_rows, OP_INCR, x, y, 1, "fill")
    hx = rng.choice(x, 16384); hy = rng.integers(1, k_home + 1, 16384).astype(np.uint32)
    wx = np.arange(WARM_ROWS, WARM_ROWS + 300, dtype=np.uint32); wy = np.ones(300, np.uint32)
    write_checked(g, o, check_rows, OP_INCR, np.concatenate([hx, wx]), np.concatenate([hy, wy]), 1, "warm-up")


def wrap_batch(rng, rows=ROWS, k_home=K_HOME, n_wrap=N_WRAP, times=2.5):
    """n_wrap new keys per row whose homes lie in the run 1..k_home (small ids plus multiples of the table sizes in play), each
    named `times` times on average (the cold start wants >= 25 % duplicates among the pending ops)"""
    xs, ys = [], []
    for r in rows:
        y = np.unique((rng.integers(1, k_home, 3 * n_wrap) + (np.uint64(1) << rng.integers(15, 21, 3 * n_wrap).astype(np.uint64))).astype(np.uint32))
        y = rng.permutation(y)[:n_wrap]
        y = np.concatenate([y] * int(times) + [y[: int(n_wrap * (times - int(times)))]])
        xs.append(np.full(y.size, r, np.uint32)); ys.append(y)
    x, y = np.concatenate(xs), np.concatenate(ys)
    p = rng.permutation(x.size)
    return x[p], y[p]


# ---- a. ---------------------------------------------------------------------------------------------------------------------------
def test_cold_start_after_a_round_without_growth(G, oracle_mod, check_rows, monkeypatch, capfd):
    """Clustered rows with keys 1..12000 at home and room left; then a batch of new keys that wrap onto the runs, each named two or
    three times.  A round defers them without growing a row (long probes, quotas) and leaves waiting-key records; the next round
    is a cold start (insert_pending_keys, SMATRIX_COLD_MIN 1024) that inserts some of the keys itself and then doubles the rows.
    Its growth must not take the stale records in: each would be a second cell of a key the cold round has just inserted, and an
    over-counted `used`.
    Host-driven rounds (SMATRIX_SPEC=0).  The chained shape cannot be brought to this order at test sizes: its pass in front of
    prep takes nearly all of the batch, the chain's growth round doubles the rows behind its first prep, and the retry leaves
    nothing deferred -- no round without growth and no cold start follow (a cold start would also keep the next batch from the
    chain)."""
    setup_cold(monkeypatch, "0")
    rng = np.random.default_rng(61)
    g, o = G(), oracle_mod.Oracle()
    fill_and_warm(g, o, check_rows, rng)
    capfd.readouterr()
    cold0 = g.stats()["cold_starts"]
    x, y = wrap_batch(rng)
    write_checked(g, o, check_rows, OP_INCR, x, y, 2, "wrap")
    err = capfd.readouterr().err
    assert g.stats()["cold_starts"] > cold0, err[-3000:]
    assert stale_record_sequences(err), ("no round without growth in front of a cold start that grew rows", err[-3000:])
    # the next batch on top (decr: the rows as the cold start left them)
    x, y = wrap_batch(rng, n_wrap=2000)
    write_checked(g, o, check_rows, OP_DECR, x, y, 1, "after")
    g.close(); o.close()


# ---- b. ---------------------------------------------------------------------------------------------------------------------------
def test_cold_start_after_the_directory_grew(G, oracle_mod, check_rows, monkeypatch, capfd):
    """As (a), host-driven, and the batch of the cold start also creates 33 000 one-key rows: the directory (65 536 slots at
    open) grows after the round that left the waiting-key records and before the cold start.  A record's slot may then name
    another row -- a key of row 3 must not land in a row it does not belong to."""
    setup_cold(monkeypatch, "0")
    rng = np.random.default_rng(62)
    g, o = G(), oracle_mod.Oracle()
    fill_and_warm(g, o, check_rows, rng, rows=(3,))
    capfd.readouterr()
    cold0, dir0 = g.stats()["cold_starts"], g.stats()["dir_grown"]
    x, y = wrap_batch(rng, rows=(3,), n_wrap=5000, times=4)      # (53 000 ops: below 2^16, no pass in front of round 0's prep)
    nx = np.arange(2 << 20, (2 << 20) + 33000, dtype=np.uint32)
    ny = rng.integers(1, 1 << 30, nx.size).astype(np.uint32)
    p = rng.permutation(x.size + nx.size)
    x, y = np.concatenate([x, nx])[p], np.concatenate([y, ny])[p]
    write_checked(g, o, check_rows, OP_INCR, x, y, 3, "wrap + rows")
    err = capfd.readouterr().err
    st = g.stats()
    assert st["cold_starts"] > cold0 and st["dir_grown"] > dir0, err[-3000:]
    seq = stale_record_sequences(err)
    assert any(d for _, d in seq), ("the directory did not grow between the round without growth and the cold start", seq, err[-3000:])
    x, y = wrap_batch(rng, rows=(3,), n_wrap=2000)
    write_checked(g, o, check_rows, OP_INCR, x, y, 1, "after")
    g.close(); o.close()


# ---- c. ---------------------------------------------------------------------------------------------------------------------------
DENSE_ROWS = np.arange(1, 9, dtype=np.uint32)     # 8 rows of dense keys
SCRAMBLED_ROWS = 2000                              # rows 1000.. of the scrambled batches


def dense_batch(rng, k_home, n_wrap, lg, fresh_row):
    """keys that wrap onto the runs 1..k_home of the dense rows (tables of 2^lg cells and more), twice each; and keys 1..300 of a
    row the batch creates -- it doubles round after round, so that the rounds behind round 0, in which the lane-per-op kernel
    finishes the long probes, still defer ops and the host sees their count (the rule that switches the mode on)"""
    xs, ys = [np.full(300, fresh_row, np.uint32)], [np.arange(1, 301, dtype=np.uint32)]
    for r in DENSE_ROWS:
        y = np.unique((rng.integers(1, k_home, n_wrap) + (np.uint64(1) << rng.integers(lg, lg + 6, n_wrap).astype(np.uint64))).astype(np.uint32))
        xs.append(np.full(2 * y.size, r, np.uint32)); ys.append(np.concatenate([y, y]))
    x, y = np.concatenate(xs), np.concatenate(ys)
    p = rng.permutation(x.size)
    return x[p], y[p]


def scrambled_batch(rng, n, dense_share=0):
    """n ops of scrambled ids on rows of Zipf-like sizes (some row reaches its threshold in every batch); dense_share of them
    new scrambled keys of the dense rows"""
    nd = int(n * dense_share)
    x = (1000 + (rng.zipf(1.2, n - nd) - 1) % SCRAMBLED_ROWS).astype(np.uint32)
    x = np.concatenate([x, rng.choice(DENSE_ROWS, nd)])
    y = (rng.integers(1, 1 << 31, n, dtype=np.uint64) * 2 + 1).astype(np.uint32)
    p = rng.permutation(n)
    return x[p], y[p]


def all_keys_read_back(g, o, tag, rows=None):
    """a get of every key the oracle holds in these rows (all rows by default): its value"""
    xs, cells = [], []
    for r in (o.list_rows() if rows is None else np.asarray(rows)).tolist():
        s = np.asarray(o.row_slots(r))
        s = s[(s[:, 0] != 0) | (s[:, 1] != 0)]
        xs.append(np.full(s.shape[0], r, np.uint32)); cells.append(s)
    x, s = np.concatenate(xs), np.concatenate(cells)
    got = g.apply(OP_GET, x, s[:, 0])
    bad = np.flatnonzero(got != s[:, 1])
    assert bad.size == 0, (tag, bad.size, [(int(x[i]), int(s[i, 0]), int(got[i]), int(s[i, 1])) for i in bad[:8]])


def test_clustered_mode_off_and_on_again(G, oracle_mod, check_rows, monkeypatch):
    """The data decides the mode (SMATRIX_CLUSTERED unset; a hint table of 2^10 entries, so that its entries collide): dense keys
    switch it on; eight chained batches of scrambled ids in a row with hardly a long probe switch it off; scrambled keys then
    double the dense rows while nobody keeps their hints and at-home bitmaps; dense keys switch it on again (the bitmaps are
    rebuilt, the hint table is the one of before).  After every batch the rows are the oracle's; after every phase every key
    the oracle holds reads back -- the dense rows' keys through hints that point into tables that have since doubled."""
    monkeypatch.delenv("SMATRIX_CLUSTERED", raising=False)
    monkeypatch.delenv("SMATRIX_SPEC", raising=False)
    monkeypatch.setenv("SMATRIX_HINT_LG", "10")
    monkeypatch.setenv("SMATRIX_TRACE_ROUNDS", "1")
    rng = np.random.default_rng(63)
    g, o = G(), oracle_mod.Oracle()
    mode = lambda: g.stats()["clustered_mode"]
    k_home = 3000                                   # 2^13 cells, 1098 keys of room
    x = np.repeat(DENSE_ROWS, k_home); y = np.tile(np.arange(1, k_home + 1, dtype=np.uint32), DENSE_ROWS.size)
    write_checked(g, o, check_rows, OP_INCR, x, y, 1, "dense fill")
    seen = [mode()]
    for b in range(4):                              # on
        if mode():
            break
        write_checked(g, o, check_rows, OP_INCR, *dense_batch(rng, k_home, 300, 13, 100 + b), 1, ("dense", b))
    assert mode() == 1, "dense keys did not switch the mode on"
    seen.append(1)
    all_keys_read_back(g, o, "on")
    sizes_on = {int(r): o.row_info(int(r))[0] for r in DENSE_ROWS}
    for b in range(24):                             # off: at least 8 chained batches of scrambled ids
        write_checked(g, o, check_rows, OP_INCR, *scrambled_batch(rng, 1 << 16), 1, ("scrambled", b))
        if mode() == 0:
            break
    assert b >= 7 and mode() == 0, "scrambled batches did not switch the mode off"
    seen.append(0)
    for b in range(8):                              # the dense rows double while the mode is off
        write_checked(g, o, check_rows, OP_INCR, *scrambled_batch(rng, 1 << 16, 0.02), 3, ("scrambled into dense rows", b))
        assert mode() == 0
        if all(o.row_info(int(r))[0] > sizes_on[int(r)] for r in DENSE_ROWS):
            break
    doubled = [int(r) for r in DENSE_ROWS if o.row_info(int(r))[0] > sizes_on[int(r)]]
    assert len(doubled) == DENSE_ROWS.size, (sizes_on, doubled)
    all_keys_read_back(g, o, "off", DENSE_ROWS)
    for b in range(4):                              # on again
        write_checked(g, o, check_rows, OP_INCR, *dense_batch(rng, k_home, 300, 14, 200 + b), 2, ("dense again", b))
        if mode():
            break
    assert mode() == 1, "dense keys did not switch the mode on again"
    seen.append(1)
    assert seen[1:] == [1, 0, 1]
    all_keys_read_back(g, o, "on again")
    write_checked(g, o, check_rows, OP_DECR, *dense_batch(rng, k_home, 300, 14, 300), 1, "dense decr")
    all_keys_read_back(g, o, "end", DENSE_ROWS)
    g.close(); o.close()
