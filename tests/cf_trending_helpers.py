"""The model of smatrix_cf_trending (include/smatrix_batch.h) and the data its tests run on, for tests/test_cf_trending_model.py and
tests/test_gpu_cf_trending.py (a plain module, no tests of its own).

trending()  over the export("sorted") of two matrices: the head pairs (column 0) of `now` with x != 0, T >= max(min_total, 1) and an id
            that is not denied; B the head of the same id in `base` (0 without one); E = floor(B * num / den) in unsigned 64-bit
            integers; T > E and G = T - E >= max(min_gain, 1); D = float64(E) + shrink with 0 counted as 1; the score G, G / D or
            G / sqrt(D) in float64, one rounding per operation; (score descending, id ascending), cut at n.
The matrices are trending_world()'s: two of about 10 000 rows of scattered 32-bit ids, in the manner of cf_fill_helpers.popular_world."""
import numpy as np

from tests import cf_fill_helpers as F

MEASURES = ("gain", "ratio", "zscore")
# (num, den, shrink): the floor matters in 1/7 and 3/7 (base totals 1 .. 9 are no multiples of 7); with shrink 0 an id that base
# does not hold has D == 0, counted as 1
PARAMS = [(1, 1, 0.0), (1, 7, 0.0), (3, 7, 0.0), (1, 1, 10.0), (3, 7, 0.1)]


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def trending(export_now, export_base, n, measure="zscore", num=1, den=1, shrink=0.0, deny=(), min_total=1, min_gain=1):
    """-> (ids uint32, scores float64, totals uint32, expected uint32), each [n_found], best first"""
    ids, T = F.heads_of(export_now)
    b_ids, b_tot = F.heads_of(export_base)
    order = np.argsort(b_ids, kind="stable")
    b_ids, b_tot = b_ids[order], b_tot[order]
    at = np.minimum(np.searchsorted(b_ids, ids), max(b_ids.size - 1, 0))
    B = np.where(b_ids[at] == ids, b_tot[at], 0).astype(np.uint64) if b_ids.size else np.zeros(ids.size, np.uint64)
    E = B * np.uint64(num) // np.uint64(den)                            # (B < 2^32, num < 2^32: the product fits 64 bits)
    T64 = T.astype(np.uint64)
    keep = (ids != 0) & (T >= max(int(min_total), 1)) & ~np.isin(ids, np.asarray(list(deny), np.uint32)) & (T64 > E)
    ids, T, T64, E = ids[keep], T[keep], T64[keep], E[keep]
    G = T64 - E
    keep = G >= np.uint64(max(int(min_gain), 1))
    ids, T, E, G = ids[keep], T[keep], E[keep], G[keep].astype(np.float64)
    D = E.astype(np.float64) + np.float64(shrink)
    D[D == 0.0] = 1.0
    score = {"gain": lambda: G, "ratio": lambda: G / D, "zscore": lambda: G / np.sqrt(D)}[measure]()
    assert np.isfinite(score).all() and (score > 0).all()
    order = np.lexsort((ids, -score))[:n]
    return ids[order], score[order], T[order], E[order].astype(np.uint32)


# ---- the two matrices ------------------------------------------------------------------------------------------------------------------
N_ROWS = 10000
N_TWINS = 300                      # ids with one T and one B: a tie group under every measure, only the id bytes tell them apart
TWIN_T, TWIN_B = 5000, 70
N_CLOSE = 8                        # ids whose RATIO scores at 1/1, shrink 0 differ in the lowest mantissa byte alone
CLOSE_K = (1 << 24) + 1            # G = k + 1 + i over E = k + i: neighbours are 1 / (k (k + 1)) apart, about 16 units of the last place


def close_totals():
    """-> (T, B) of the N_CLOSE ids: T = 2 k + 1 + 2 i >= 2^25, B = k + i"""
    i = np.arange(N_CLOSE, dtype=np.uint64)
    return (2 * CLOSE_K + 1 + 2 * i).astype(np.uint32), (CLOSE_K + i).astype(np.uint32)


def trending_world():
    """-> dict of two matrices' recipes, `now` and `base`: each {ops: (x, y, v) SET ops, every (x, y) once; empty: ids made by the
    scalar set(x, 0, 0); zeroed: (x, y, v) DECR ops that bring a head to 0; totals: {id: total} of every head pair that ends
    non-zero}, and the id groups by name.
    now   totals 1 .. 12 nearly everywhere; six totals >= 2^24, one of them 0xFFFFFFFF (id 0xFFFFFFFF's); the twins; the close
          group; rows without a head pair, empty rows, zeroed heads, row 0
    base  most of now's ids with totals 0 < B <= 9 (tie groups of scores; E == T and E > T happen by themselves); a tenth of
          now's ids absent; now's ids with a row but no head pair, with a head decremented to 0, with an empty row (quirk Q3);
          200 ids that only base holds, with large totals; totals >= 2^24 and one 0xFFFFFFFF under now's large ones"""
    rng = np.random.default_rng(4242)
    ids = np.unique(rng.integers(1, 0xFFFFFFFF, N_ROWS + 600, dtype=np.uint64).astype(np.uint32))
    ids = rng.permutation(ids[ids != 0xFFFFFFFF])
    main = np.concatenate([np.array([0xFFFFFFFF], np.uint32), ids[:N_ROWS - 1]])
    rest = ids[N_ROWS:]
    no_head, empty, zeroed, only_base = rest[:40], rest[40:43], rest[43:48], rest[48:248]
    tot = rng.integers(1, 13, main.size).astype(np.uint32)
    big = slice(0, 6)
    tot[big] = [0xFFFFFFFF, 1 << 24, (1 << 24) + 5, 1 << 30, (1 << 31) + 7, 1 << 24]
    twins = slice(6, 6 + N_TWINS)
    tot[twins] = TWIN_T
    close = slice(6 + N_TWINS, 6 + N_TWINS + N_CLOSE)
    tot[close] = close_totals()[0]
    pairs = main[::7]

    def recipe(xs, ys, vs, empty, zeroed, totals):
        return {"ops": tuple(np.concatenate(a).astype(np.uint32) for a in (xs, ys, vs)), "empty": [int(e) for e in empty],
                "zeroed": (np.asarray(zeroed, np.uint32), np.zeros(len(zeroed), np.uint32), np.full(len(zeroed), 7, np.uint32)),
                "totals": totals}

    u32 = lambda a: np.asarray(a, np.uint32)                              # noqa: E731
    now_totals = dict(zip(main.tolist(), tot.tolist()))
    now_totals[0] = 1000
    now = recipe([main, pairs, u32([0, 0]), no_head, zeroed, zeroed],
                 [np.zeros(main.size, np.uint32), np.full(pairs.size, 5), u32([0, 9]), np.full(no_head.size, 5), np.zeros(zeroed.size), np.full(zeroed.size, 6)],
                 [tot, np.full(pairs.size, 3), u32([1000, 1]), np.full(no_head.size, 2), np.full(zeroed.size, 7), np.ones(zeroed.size)],
                 empty, zeroed, now_totals)

    # base: the mass is main[6 + N_TWINS + N_CLOSE:]; of it a tenth absent, 30 without a head pair, 5 zeroed, 3 empty rows
    mass = main[6 + N_TWINS + N_CLOSE:]
    role = rng.permutation(mass.size)
    n_abs = mass.size // 10
    absent, b_no_head, b_zeroed, b_empty = (mass[role[:n_abs]], mass[role[n_abs:n_abs + 30]], mass[role[n_abs + 30:n_abs + 35]],
                                            mass[role[n_abs + 35:n_abs + 38]])
    held = mass[role[n_abs + 38:]]
    held_tot = rng.integers(1, 10, held.size).astype(np.uint32)
    # under now's six large totals, in order: absent from base; E == T at 1/1; a small B; a small B; 0xFFFFFFFF (E > T at 1/1, E < T at 3/7, and
    # B * 3 needs 64 bits); one less than T
    big_ids, big_b = main[1:6], u32([1 << 24, 5, 7, 0xFFFFFFFF, (1 << 24) - 1])
    only_tot = rng.integers(1 << 20, 1 << 26, only_base.size).astype(np.uint32)
    b_x = [held, big_ids, main[twins], main[close], only_base, u32([0])]
    b_v = [held_tot, big_b, np.full(N_TWINS, TWIN_B), close_totals()[1], only_tot, u32([50])]
    base_totals = dict(zip(np.concatenate(b_x).tolist(), np.concatenate(b_v).astype(np.uint32).tolist()))
    b_pairs = held[::5]
    base = recipe(b_x + [b_pairs, b_no_head, b_zeroed, b_zeroed],
                  [np.zeros(sum(a.size for a in b_x)), np.full(b_pairs.size, 5), np.full(b_no_head.size, 5), np.zeros(b_zeroed.size), np.full(b_zeroed.size, 6)],
                  b_v + [np.full(b_pairs.size, 3), np.full(b_no_head.size, 2), np.full(b_zeroed.size, 7), np.ones(b_zeroed.size)],
                  b_empty, b_zeroed, base_totals)
    return {"now": now, "base": base, "twins": main[twins].copy(), "close": main[close].copy(), "big": main[big].copy(),
            "absent": absent, "only_base": only_base, "base_no_head": b_no_head, "base_zeroed": b_zeroed, "base_empty": b_empty,
            "now_no_candidates": np.concatenate([no_head, empty, zeroed])}


def export_of(recipe):
    """what export("sorted") returns of a matrix built from the recipe, as far as trending() reads it: the head pairs that end non-zero"""
    return F.export_of_totals(recipe["totals"])


def three_row_world():
    """-> (now ops, base ops): three candidates and an id that only base holds"""
    u32 = lambda a: np.asarray(a, np.uint32)                              # noqa: E731
    return (u32([5, 9, 700]), u32([0, 0, 0]), u32([30, 30, 8])), (u32([5, 9, 12]), u32([0, 0, 0]), u32([10, 10, 99]))
