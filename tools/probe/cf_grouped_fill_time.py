#!/usr/bin/env python3
"""The grouped fill call (smatrix_cf_recommend_grouped_fill_dev) next to the two calls it joins (smatrix_cf_recommend_grouped_dev and
smatrix_cf_recommend_fill_dev, k = 10); same process, same matrix, one GPU.

  python3 tools/probe/cf_grouped_fill_time.py [--ops 4e8] [--reps 5] [--inner 20] [--sessions 4096] [--out profiles/cf_grouped_fill_time.txt]

The matrix is tools/probe/cf_grouped_time.py's serving copy: the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches of
2^24, every row's head pair set to the sum of the row's values, then truncated(64, rank="cosine").  The map is that probe's dominant
brand -- 19 ids of 20 in ONE group, the others in 1000 --, over all of uint32 (16 GiB: a gather from it is as expensive as a gather
gets), cap = 1; the list is the 1024 most popular ids of the source (cf_popular_dev).  After one warm-up rep, `reps` reps, the variants
alternated rep by rep, the best rep reported; a rep is `inner` calls back to back between two device synchronisations, its time the mean
per call; every array on the device:
  grouped, grouped_again   cf_recommend_grouped_dev with that map and cap on `sessions` sessions of 8 ids drawn from the stream's own row
                           ids, timed TWICE: the difference of the two bests is the run's own spread
  fill, fill_again         cf_recommend_fill_dev on the same sessions with the list, timed twice likewise
  both_warm                cf_recommend_grouped_fill_dev on the same sessions, with the map, the cap and the list
  fill_cold                cf_recommend_fill_dev on `sessions` sessions of 8 ids without rows: every place filled, no quotas
  both_cold                cf_recommend_grouped_fill_dev on those sessions: every place filled under the quotas
and, as checks, that both_warm's scored part has grouped's bytes and its n_scored grouped's counts, that no group occurs more than cap
times in any result, and that every cold session holds the serial walk of the list under the quota, made on the host.  Writes one JSON
line under a header to --out and prints it."""
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

L, K, M, N_GROUPS, N_FILL, CAP = 8, 10, 64, 1000, 1024, 1
OP_SET = 1


def skew(i):
    """the map, on numpy ids: 19 of 20 in group 0"""
    return np.where(i % 20 != 0, 0, 1 + i % N_GROUPS)


def walk(fill, cap, k):
    """the serial walk of the list for a session with no result, no items in the list and no filters -> (ids, the entries walked)"""
    out, used = [], {}
    for at, f in enumerate(int(v) for v in fill):
        g = int(skew(np.int64(f)))
        if f == 0 or f in out or used.get(g, 0) >= cap:
            continue
        out.append(f)
        used[g] = used.get(g, 0) + 1
        if len(out) == k:
            return out, at + 1
    return out, len(fill)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_grouped_fill_time.txt"))
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
    h_rows = rows.cpu().numpy().view(np.uint32)
    del rows, row_ptr, pairs, csum, totals, zeros
    torch.cuda.empty_cache()
    st = src.stats()
    res = {"ops_in_stream": nb * B, "src_rows": st["rows"], "totals": "row sums", "copy": "truncated(64, rank='cosine')", "reps": a.reps,
           "inner": a.inner, "sessions": n, "session_len": L, "k": K, "m": M, "cap": CAP, "n_fill": N_FILL,
           "groups": "19 ids of 20 in group 0, the others in 1 + id %% %d" % N_GROUPS, "sim": "cosine", "shrink": 0.0}
    d_fill = torch.zeros(N_FILL, dtype=torch.int32, device=dev); d_ptot = torch.zeros_like(d_fill)
    d_pn = torch.zeros(1, dtype=torch.int32, device=dev)
    src.cf_popular_dev(N_FILL, None, 0, 1, d_fill.data_ptr(), d_ptot.data_ptr(), d_pn.data_ptr(), stream)
    torch.cuda.synchronize()
    assert int(d_pn.cpu().numpy()[0]) == N_FILL
    m = src.truncated(M, rank="cosine")
    src.close()
    torch.cuda.empty_cache()

    ids = np.ascontiguousarray(sx.astype(np.uint32)).reshape(n, L)
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * L
    d_items = torch.from_numpy(ids.view(np.int32).reshape(-1)).to(dev)
    cold = np.arange(1, 2 * n * L + h_rows.size + 1, dtype=np.uint32)                       # the first n * L ids that have no row
    cold = cold[~np.isin(cold, h_rows)][:n * L].reshape(n, L)
    d_cold = torch.from_numpy(cold.view(np.int32).reshape(-1)).to(dev)
    group_n = 1 << 32                                                     # the stream's ids are fmix32(rank): the map covers every uint32
    d_grp = torch.empty(group_n, dtype=torch.int32, device=dev)
    for c in range(0, group_n, 1 << 28):
        i = torch.arange(c, c + (1 << 28), dtype=torch.int64, device=dev)
        d_grp[c:c + (1 << 28)] = torch.where(i % 20 != 0, torch.zeros_like(i), 1 + i % N_GROUPS).to(torch.int32)
    del i
    res["group_n"] = group_n
    names = ("grouped", "fill", "both_warm", "fill_cold", "both_cold", "grouped_again", "fill_again")
    out = {v: (torch.zeros(n * K, dtype=torch.int32, device=dev), torch.zeros(n * K, dtype=torch.float64, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for v in names}

    def grouped(v):
        o = [u.data_ptr() for u in out[v]]
        return lambda: m.cf_recommend_grouped_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, d_grp.data_ptr(), group_n,
                                                  CAP, "cosine", 0.0, K, o[0], o[1], o[2], stream)

    def fill(v, items):
        o = [u.data_ptr() for u in out[v]]
        return lambda: m.cf_recommend_fill_dev(n, d_off.data_ptr(), items.data_ptr(), None, None, None, None, 0, d_fill.data_ptr(), N_FILL,
                                               "cosine", 0.0, K, o[0], o[1], o[2], o[3], stream)

    def both(v, items):
        o = [u.data_ptr() for u in out[v]]
        return lambda: m.cf_recommend_grouped_fill_dev(n, d_off.data_ptr(), items.data_ptr(), None, None, None, None, 0, d_grp.data_ptr(),
                                                       group_n, CAP, d_fill.data_ptr(), N_FILL, "cosine", 0.0, K, o[0], o[1], o[2], o[3], stream)

    variants = [("grouped", grouped("grouped")), ("fill", fill("fill", d_items)), ("both_warm", both("both_warm", d_items)),
                ("fill_cold", fill("fill_cold", d_cold)), ("both_cold", both("both_cold", d_cold)), ("grouped_again", grouped("grouped_again")),
                ("fill_again", fill("fill_again", d_items))]
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
    g_yard, f_yard = min(res["grouped_ms_best"], res["grouped_again_ms_best"]), min(res["fill_ms_best"], res["fill_again_ms_best"])
    res["grouped_spread_ms"] = round(abs(res["grouped_ms_best"] - res["grouped_again_ms_best"]), 4)
    res["fill_spread_ms"] = round(abs(res["fill_ms_best"] - res["fill_again_ms_best"]), 4)
    res["both_warm_minus_grouped_ms"] = round(res["both_warm_ms_best"] - g_yard, 4)
    res["both_warm_beyond_spread_ms"] = round(max(0.0, res["both_warm_ms_best"] - g_yard - max(res["grouped_spread_ms"], res["fill_spread_ms"])), 4)
    res["both_cold_minus_fill_cold_ms"] = round(res["both_cold_ms_best"] - res["fill_cold_ms_best"], 4)
    res["fill_minus_grouped_ms"] = round(f_yard - g_yard, 4)              # other launches in front of the fill: not the fill's extra
    # the calls agree
    got = {v: [u.cpu().numpy() for u in out[v]] for v in names}
    g, bw, bc = got["grouped"], got["both_warm"], got["both_cold"]
    used = np.arange(K)[None, :] < g[2][:, None]
    res["warm_sessions_that_fill"] = int((bw[3] < K).sum())
    res["warm_results_mean"] = round(float(bw[2].mean()), 3)
    res["grouped_results_mean"] = round(float(g[2].mean()), 3)
    res["warm_scored_part_is_groupeds"] = bool((bw[3] == g[2]).all() and (bw[0].reshape(n, K)[used] == g[0].reshape(n, K)[used]).all() and
                                               (bw[1].reshape(n, K).view(np.uint64)[used] == g[1].reshape(n, K).view(np.uint64)[used]).all())
    worst = 0
    for v in (bw, bc):
        r_ids, cnt = v[0].view(np.uint32).reshape(n, K), v[2].view(np.uint32)
        for s in range(n):
            grp = skew(r_ids[s, :cnt[s]].astype(np.int64))
            worst = max(worst, int(np.bincount(grp, minlength=1).max()) if cnt[s] else 0)
    res["most_of_one_group"] = worst
    want, walked = walk(d_fill.cpu().numpy().view(np.uint32), CAP, K)
    res["cold_list_entries_walked"] = walked
    res["cold_all_filled_with_the_walks_ids"] = bool((bc[3] == 0).all() and (bc[2] == len(want)).all() and len(want) == K and
                                                     (bc[0].view(np.uint32).reshape(n, K) == np.array(want, np.uint32)[None, :]).all() and not bc[1].any())
    m.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write("# python3 tools/probe/cf_grouped_fill_time.py   (1x MI355X; --ops %g --reps %d --inner %d --sessions %d)\n" % (a.ops, a.reps, a.inner, n))
        f.write("# ms, mean of `inner` calls, best rep.  On src.truncated(64, rank=\"cosine\"), k = 10, cap = 1, the map 19 ids of 20 in ONE group, the\n")
        f.write("# list the 1024 most popular ids.  grouped / grouped_again = cf_recommend_grouped_dev, fill / fill_again = cf_recommend_fill_dev, each\n")
        f.write("# timed twice: *_spread_ms; both_warm = cf_recommend_grouped_fill_dev on the same sessions; fill_cold / both_cold = the fill call and\n")
        f.write("# the grouped fill call on sessions of ids without rows (every place filled; both_cold under the quotas).\n")
        f.write("# The global tier's cost is NOT measured here, and neither is a list longer than 1024 ids.\n")
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
