#!/usr/bin/env python3
"""The grouped call (smatrix_cf_recommend_grouped_dev) next to the recommend call it extends (smatrix_cf_recommend_sim_dev, k = 10); same
process, same matrix, one GPU.

  python3 tools/probe/cf_grouped_time.py [--ops 4e8] [--reps 5] [--inner 20] [--sessions 4096] [--out profiles/cf_grouped_time.txt]

The matrix is tools/probe/cf_fill_time.py's serving copy: the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches of
2^24, every row's head pair set to the sum of the row's values, then truncated(64, rank="cosine").  After one warm-up rep, `reps` reps,
the variants alternated rep by rep, the best rep reported; a rep is `inner` calls back to back between two device synchronisations,
its time the mean per call; every array on the device:
  rec, rec_again   cf_recommend_sim_dev("cosine", 0, k = 10) on `sessions` sessions of 8 ids drawn from the stream's own row ids, timed
                   TWICE: the difference of the two bests is the run's own spread
  no_map           cf_recommend_grouped_dev with no map: the sim call's launches, expected within the spread
  cap2, cap1       cf_recommend_grouped_dev with the map id -> id % 1000 and cap = 2, cap = 1.  The stream's ids are scrambled over all of
                   uint32, so the map has 2^32 entries (16 GiB): a gather from it is as expensive as a gather gets
  skew1            the same with cap = 1 and a map that puts 19 ids of 20 into ONE group and the others into 1000: a dominant brand, so the
                   quota binds in every session and the ending needs a second round
  *_host_only_us   the two Python methods called on NO sessions: the host's own part of a call (argument checks, ctypes), which a call
                   that reads its tier counts back cannot hide behind the kernels of the call before
and, as checks, that no_map has rec's bytes, that no group occurs more than cap times in a result, and that the results are the
closed form's on a sample of sessions whose whole rankings are rebuilt on the host (the rows of the session's items through
getrow_batch, the order through cf_rank) -- which also gives the ROUNDS the kernel makes on them: a round looks at the 64 best
candidates still alive and strikes out those and every candidate of a group that is full.  Writes one JSON line under a header to
--out and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libsmatrix_amd import OP_INCR, SparseMatrix, Stream  # noqa: E402
from tools.probe.merge_time import B  # noqa: E402

L, K, M, N_GROUPS, SAMPLE = 8, 10, 64, 1000, 256
OP_SET = 1


def rounds_and_result(order, groups, cap, k):
    """the ranking `order` (ids, best first) and their groups -> (the rounds of kernels/recommend.hpp rec_group_table, its result)"""
    alive = np.ones(order.size, bool)
    used, res, rounds = {}, [], 0
    while True:
        rounds += 1
        at = np.flatnonzero(alive)[:64]
        full = set()
        for i in at:
            g = int(groups[i])
            if used.get(g, 0) < cap:
                if len(res) < k:
                    res.append(int(order[i]))
                used[g] = used.get(g, 0) + 1
                if used[g] == cap:
                    full.add(g)
        if len(res) >= k or at.size < 64:
            return rounds, res
        alive[at] = False
        alive &= ~np.isin(groups, list(full))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_grouped_time.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    src = SparseMatrix()
    gen = Stream("zipf", bench.SEED, bench.N_IDS, bench.ZIPF_S, 1)
    x = torch.empty(B, dtype=torch.int32, device=dev); y = torch.empty_like(x); ones = torch.ones_like(x)
    nb = max(1, int(a.ops) // B)
    for s in range(nb):
        gen.fill_device(s * B, B, x.data_ptr(), y.data_ptr(), stream)
        src.apply_batch_dev(OP_INCR, B, x.data_ptr(), y.data_ptr(), ones.data_ptr(), None, stream)
    torch.cuda.synchronize()
    n = a.sessions
    sx, _ = gen.fill(0, L * n)
    gen.close()
    del x, y, ones
    rows, row_ptr, pairs = src.export_dev("table")                       # the totals: (x, 0, sum of row x)
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(pairs[:, 1].to(torch.int64) & 0xFFFFFFFF, 0)])
    totals = (csum[row_ptr[1:]] - csum[row_ptr[:-1]]).clamp(max=0x7FFFFFFF).to(torch.int32)
    zeros = torch.zeros_like(rows)
    torch.cuda.synchronize()
    for s in range(0, rows.numel(), B):
        c = min(B, rows.numel() - s)
        src.apply_batch_dev(OP_SET, c, rows[s:].data_ptr(), zeros[s:].data_ptr(), totals[s:].data_ptr(), None, stream)
    torch.cuda.synchronize()
    del rows, row_ptr, pairs, csum, totals, zeros
    torch.cuda.empty_cache()
    st = src.stats()
    res = {"ops_in_stream": nb * B, "src_rows": st["rows"], "totals": "row sums", "copy": "truncated(64, rank='cosine')", "reps": a.reps,
           "inner": a.inner, "sessions": n, "session_len": L, "k": K, "m": M, "groups": "id %% %d" % N_GROUPS, "sim": "cosine", "shrink": 0.0}
    m = src.truncated(M, rank="cosine")
    src.close()
    torch.cuda.empty_cache()

    ids = np.ascontiguousarray(sx.astype(np.uint32)).reshape(n, L)
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * L
    d_items = torch.from_numpy(ids.view(np.int32).reshape(-1)).to(dev)
    group_n = 1 << 32                                                     # the stream's ids are fmix32(rank): the map covers every uint32
    d_grp = torch.empty(group_n, dtype=torch.int32, device=dev)           # 16 GiB: every gather is a miss in a table of this size
    for c in range(0, group_n, 1 << 28):
        d_grp[c:c + (1 << 28)] = (torch.arange(c, c + (1 << 28), dtype=torch.int64, device=dev) % N_GROUPS).to(torch.int32)
    res["group_n"] = group_n
    d_skew = torch.empty(group_n, dtype=torch.int32, device=dev)          # one dominant brand: 19 ids of 20 in group 0
    for c in range(0, group_n, 1 << 28):
        i = torch.arange(c, c + (1 << 28), dtype=torch.int64, device=dev)
        d_skew[c:c + (1 << 28)] = torch.where(i % 20 != 0, torch.zeros_like(i), 1 + i % N_GROUPS).to(torch.int32)
    del i
    names = ("rec", "no_map", "cap2", "cap1", "skew1", "rec_again")
    out = {v: (torch.zeros(n * K, dtype=torch.int32, device=dev), torch.zeros(n * K, dtype=torch.float64, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev)) for v in names}

    def recommend(v):
        o = [u.data_ptr() for u in out[v]]
        return lambda: m.cf_recommend_sim_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, K, o[0], o[1],
                                              o[2], stream)

    def grouped(v, cap, gmap=None):
        o = [u.data_ptr() for u in out[v]]
        return lambda: m.cf_recommend_grouped_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0,
                                                  None if gmap is None else gmap.data_ptr(), 0 if gmap is None else group_n, cap, "cosine",
                                                  0.0, K, o[0], o[1], o[2], stream)

    variants = [("rec", recommend("rec")), ("no_map", grouped("no_map", 1)), ("cap2", grouped("cap2", 2, d_grp)), ("cap1", grouped("cap1", 1, d_grp)),
                ("skew1", grouped("skew1", 1, d_skew)), ("rec_again", recommend("rec_again"))]
    # what a call costs on the host before the library touches the device: the two methods on NO sessions (both return at once).  Every
    # call reads its tier counts back, so this time is not hidden behind the kernels of the call before
    host = {}
    for name, fn in (("rec", lambda: m.cf_recommend_sim_dev(0, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, K,
                                                            0, 0, 0, stream)),
                     ("no_map", lambda: m.cf_recommend_grouped_dev(0, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, None, 0, 1,
                                                                   "cosine", 0.0, K, 0, 0, 0, stream))):
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(20000):
                fn()
            best = min(best, (time.perf_counter() - t0) / 20000)
        host[name] = best
    res["rec_host_only_us"] = round(host["rec"] * 1e6, 3)
    res["no_map_host_only_us"] = round(host["no_map"] * 1e6, 3)
    t = {name: [] for name, _ in variants}
    for rep in range(a.reps + 1):                      # rep 0 is the warm-up
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.inner):
                fn()
            torch.cuda.synchronize()
            if rep:
                t[name].append((time.perf_counter() - t0) * 1e3 / a.inner)
        print("# rep %d of %d done" % (rep, a.reps), flush=True)
    for name, _ in variants:
        res["%s_ms_best" % name] = round(min(t[name]), 4)
        res["%s_ms_all" % name] = [round(u, 4) for u in t[name]]
    yard = min(res["rec_ms_best"], res["rec_again_ms_best"])
    res["rec_spread_ms"] = round(abs(res["rec_ms_best"] - res["rec_again_ms_best"]), 4)
    res["no_map_minus_rec_ms"] = round(res["no_map_ms_best"] - yard, 4)
    res["no_map_beyond_spread_ms"] = round(max(0.0, res["no_map_ms_best"] - yard - res["rec_spread_ms"]), 4)
    # the same launches: what is left of the difference once the host's own part of a call is taken off
    res["no_map_host_extra_ms"] = round((res["no_map_host_only_us"] - res["rec_host_only_us"]) * 1e-3, 4)
    res["no_map_minus_rec_minus_host_ms"] = round(res["no_map_minus_rec_ms"] - res["no_map_host_extra_ms"], 4)
    res["no_map_reps_overlap_recs"] = bool(min(t["no_map"]) <= max(t["rec"] + t["rec_again"]))
    plain = lambda i: i % N_GROUPS                                        # noqa: E731  (the maps, on numpy ids)
    skew = lambda i: np.where(i % 20 != 0, 0, 1 + i % N_GROUPS)           # noqa: E731
    capped = (("cap2", 2, plain), ("cap1", 1, plain), ("skew1", 1, skew))
    for v, _, _ in capped:
        res["%s_over_rec" % v] = round(res["%s_ms_best" % v] / yard, 3)
    # the calls agree
    got = {v: [u.cpu().numpy() for u in out[v]] for v in names}
    res["no_map_is_recs_bytes"] = bool(all(p.tobytes() == q.tobytes() for p, q in zip(got["no_map"], got["rec"])))
    for v, cap, gmap in capped:
        r_ids, cnt = got[v][0].view(np.uint32).reshape(n, K), got[v][2].view(np.uint32)
        worst = 0
        for s in range(n):
            g = gmap(r_ids[s, :cnt[s]].astype(np.int64))
            worst = max(worst, int(np.bincount(g, minlength=1).max()) if cnt[s] else 0)
        res["%s_most_of_one_group" % v] = worst
        res["%s_results_mean" % v] = round(float(cnt.mean()), 3)
        res["%s_sessions_that_differ_from_rec" % v] = int((r_ids != got["rec"][0].view(np.uint32).reshape(n, K)).any(axis=1).sum())
    # the whole rankings of a sample, on the host: the closed form's result, and the rounds
    sample = list(range(0, n, max(1, n // SAMPLE)))[:SAMPLE]
    uniq = np.unique(ids[sample].reshape(-1))
    r_off, r_pairs, r_cnt = m.getrow_batch(uniq)
    row = {int(u): r_pairs[int(r_off[i]):int(r_off[i]) + int(r_cnt[i]), 0] for i, u in enumerate(uniq)}
    sessions = [ids[s].tolist() for s in sample]
    cands = [np.setdiff1d(np.unique(np.concatenate([row[int(v)] for v in sess])), np.array([0] + sess, np.uint32)) for sess in sessions]
    ranks, _, ncand = m.cf_rank(sessions, [c.tolist() for c in cands])
    rounds = {v: [] for v, _, _ in capped}
    same = True
    j = 0
    for i, c in enumerate(cands):
        r = ranks[j:j + c.size]
        j += c.size
        order = np.empty(c.size, np.uint32)
        order[r] = c                                                      # every candidate has a rank of its own
        for v, cap, gmap in capped:
            nr, want = rounds_and_result(order, gmap(order.astype(np.int64)), cap, K)
            rounds[v].append(nr)
            s = sample[i]
            have = got[v][0].view(np.uint32).reshape(n, K)[s, :got[v][2].view(np.uint32)[s]].tolist()
            same = same and have == want and int(ncand[i]) == c.size
    res.update(sample=len(sample), sample_candidates_mean=round(float(np.mean([c.size for c in cands])), 1), sample_is_the_closed_forms=bool(same),
               rounds_are="a host restatement of the kernel's rounds on the sample, not a device counter")
    for v, _, _ in capped:
        res["%s_rounds_mean" % v] = round(float(np.mean(rounds[v])), 3)
        res["%s_rounds_max" % v] = int(max(rounds[v]))
    m.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write("# python3 tools/probe/cf_grouped_time.py   (1x MI355X; --ops %g --reps %d --inner %d --sessions %d)\n" % (a.ops, a.reps, a.inner, n))
        f.write("# ms, mean of `inner` calls, best rep.  rec / rec_again = cf_recommend_sim_dev(k = 10) on src.truncated(64, rank=\"cosine\"), the same\n")
        f.write("# call timed twice: rec_spread_ms; no_map = cf_recommend_grouped_dev without a map (the same launches); cap2 / cap1 = the same with\n")
        f.write("# the map id -> id %% %d and that cap; skew1 = cap 1 with 19 ids of 20 in ONE group (a dominant brand: the quota binds in every\n" % N_GROUPS)
        f.write("# session).  *_host_only_us = the Python call on no sessions: the host's part of a call.  *_rounds_* = the rounds of the grouped\n")
        f.write("# ending on a sample of sessions, restated on the host from rankings rebuilt there -- not counted by the kernel.\n")
        f.write("# The global tier's cost (a workgroup per session over its whole table, as on pruned(1)) is NOT measured here.\n")
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
