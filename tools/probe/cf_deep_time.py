#!/usr/bin/env python3
"""The deep call (smatrix_cf_recommend_deep_dev, up to 1024 results per session) next to the recommend call it extends
(smatrix_cf_recommend_sim_dev); same process, same matrix, one GPU.

  python3 tools/probe/cf_deep_time.py [--ops 4e8] [--reps 5] [--inner 20] [--sessions 4096] [--out profiles/cf_deep_time.txt]

The matrix is tools/probe/cf_grouped_time.py's: the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches of 2^24, every
row's head pair set to the sum of the row's values; the serving copy is truncated(64, rank="cosine").  After one warm-up rep, `reps`
reps, the variants alternated rep by rep, the best rep reported; a rep is `inner` calls back to back between two device
synchronisations, its time the mean per call; every array on the device:
  rec, rec_again   cf_recommend_sim_dev("cosine", 0, k = 10) on `sessions` sessions of 8 ids drawn from the stream's own row ids, timed
                   TWICE: the difference of the two bests is the run's own spread
  rec64            the same with k = 64: the yardstick of the deep ending's ratios
  deep10, deep64   cf_recommend_deep_dev with k = 10 and k = 64: the sim call's launches, expected within the spread
  deep100, deep256, deep1024   the deep ending on the truncated copy, where a session has at most 8 x 64 candidates
and, before the copy is made, on the UNTRUNCATED table (`--global-sessions` single-item sessions of its hottest rows; `--global-inner`
calls a rep):
  gl_deep1024      cf_recommend_deep_dev(k = 1024): a session of the global tier is ended by ONE workgroup over its whole table
  gl_rank1         cf_rank_dev with one target per session (the best id): the same tables, the rank ending, one workgroup each as well
  gl_rec64         cf_recommend_sim_dev(k = 64): the top-k ending, a wave per 4096-slot segment
and, as checks, that deep10 / deep64 have rec's / rec64's bytes, that the first 64 entries of deep1024 are rec64's, and that cf_rank
answers a sample of deep1024's ids with their places.  Writes one JSON line under a header to --out and prints it."""
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
from libsmatrix_amd import DEEP_MAX, OP_INCR, SparseMatrix, Stream  # noqa: E402
from tools.probe.merge_time import B  # noqa: E402

L, M = 8, 64
OP_SET = 1
LDS_SLOTS = 4096


def timed(variants, reps, inner):
    """{name: the per-call ms of every rep but the warm-up}, the variants alternated rep by rep"""
    t = {name: [] for name, _ in variants}
    for rep in range(reps + 1):                        # rep 0 is the warm-up
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if rep:
                t[name].append((time.perf_counter() - t0) * 1e3 / inner)
        print("# rep %d of %d done" % (rep, reps), flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--global-sessions", type=int, default=256)
    ap.add_argument("--global-inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_deep_time.txt"))
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
    sx, _ = gen.fill(0, max(L * n, 1 << 20))
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
           "inner": a.inner, "sessions": n, "session_len": L, "m": M, "sim": "cosine", "shrink": 0.0}

    def outputs(count, k):
        return (torch.zeros(count * k, dtype=torch.int32, device=dev), torch.zeros(count * k, dtype=torch.float64, device=dev),
                torch.zeros(count, dtype=torch.int32, device=dev))

    def call(m, method, count, off, items, k, o):
        p = [u.data_ptr() for u in o]
        return lambda: getattr(m, method)(count, off.data_ptr(), items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, k, p[0], p[1], p[2], stream)

    # ---- the global tier: single-item sessions of the hottest rows of the untruncated table ----
    ng = a.global_sessions
    uniq, freq = np.unique(sx, return_counts=True)
    hot = np.ascontiguousarray(uniq[np.argsort(-freq, kind="stable")][:ng].astype(np.uint32))
    slots = np.array([(src.row_info(int(r)) or (0, 0))[0] for r in hot], np.int64)
    res.update(gl_sessions=int(hot.size), gl_sessions_in_the_global_tier=int((slots + 1 > LDS_SLOTS).sum()), gl_row_slots_min=int(slots.min()),
               gl_row_slots_max=int(slots.max()), gl_inner=a.global_inner)
    g_off = torch.arange(0, hot.size + 1, dtype=torch.int64, device=dev)
    g_items = torch.from_numpy(hot.view(np.int32)).to(dev)
    g_deep, g_rec = outputs(hot.size, DEEP_MAX), outputs(hot.size, 64)
    call(src, "cf_recommend_deep_dev", hot.size, g_off, g_items, DEEP_MAX, g_deep)()
    torch.cuda.synchronize()
    g_tg = g_deep[0].view(hot.size, DEEP_MAX)[:, 0].contiguous()          # one target per session: its best id
    g_ranks = torch.zeros(hot.size, dtype=torch.int32, device=dev)
    g_sc = torch.zeros(hot.size, dtype=torch.float64, device=dev)
    g_nc = torch.zeros(hot.size, dtype=torch.int32, device=dev)
    rank1 = lambda: src.cf_rank_dev(hot.size, g_off.data_ptr(), g_items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, g_off.data_ptr(),   # noqa: E731
                                    g_tg.data_ptr(), g_ranks.data_ptr(), g_sc.data_ptr(), g_nc.data_ptr(), stream)
    t = timed([("gl_rec64", call(src, "cf_recommend_sim_dev", hot.size, g_off, g_items, 64, g_rec)), ("gl_rank1", rank1),
               ("gl_deep1024", call(src, "cf_recommend_deep_dev", hot.size, g_off, g_items, DEEP_MAX, g_deep))], a.reps, a.global_inner)
    for name in t:
        res["%s_ms_best" % name] = round(min(t[name]), 4)
        res["%s_ms_all" % name] = [round(u, 4) for u in t[name]]
    res["gl_deep1024_over_rank1"] = round(res["gl_deep1024_ms_best"] / res["gl_rank1_ms_best"], 3)
    res["gl_deep1024_over_rec64"] = round(res["gl_deep1024_ms_best"] / res["gl_rec64_ms_best"], 3)
    nc = g_nc.cpu().numpy().view(np.uint32)
    res.update(gl_candidates_mean=round(float(nc.mean()), 1), gl_candidates_max=int(nc.max()),
               gl_rank_of_the_best_is_0=bool((g_ranks.cpu().numpy() == 0).all()),
               gl_first_64_are_rec64s=bool(g_deep[0].view(hot.size, DEEP_MAX)[:, :64].cpu().numpy().tobytes() == g_rec[0].cpu().numpy().tobytes()))
    del g_deep, g_rec

    m = src.truncated(M, rank="cosine")
    src.close()
    torch.cuda.empty_cache()

    # ---- the serving copy ----
    ids = np.ascontiguousarray(sx[:L * n].astype(np.uint32)).reshape(n, L)
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * L
    d_items = torch.from_numpy(ids.view(np.int32).reshape(-1)).to(dev)
    spec = [("rec", "cf_recommend_sim_dev", 10), ("deep10", "cf_recommend_deep_dev", 10), ("rec64", "cf_recommend_sim_dev", 64),
            ("deep64", "cf_recommend_deep_dev", 64), ("deep100", "cf_recommend_deep_dev", 100), ("deep256", "cf_recommend_deep_dev", 256),
            ("deep1024", "cf_recommend_deep_dev", DEEP_MAX), ("rec_again", "cf_recommend_sim_dev", 10)]
    out = {name: outputs(n, k) for name, _, k in spec}
    t = timed([(name, call(m, method, n, d_off, d_items, k, out[name])) for name, method, k in spec], a.reps, a.inner)
    for name in t:
        res["%s_ms_best" % name] = round(min(t[name]), 4)
        res["%s_ms_all" % name] = [round(u, 4) for u in t[name]]
    yard = min(res["rec_ms_best"], res["rec_again_ms_best"])
    res["rec_spread_ms"] = round(abs(res["rec_ms_best"] - res["rec_again_ms_best"]), 4)
    res["deep10_minus_rec_ms"] = round(res["deep10_ms_best"] - yard, 4)
    res["deep10_beyond_spread_ms"] = round(max(0.0, res["deep10_ms_best"] - yard - res["rec_spread_ms"]), 4)
    res["deep64_minus_rec64_ms"] = round(res["deep64_ms_best"] - res["rec64_ms_best"], 4)
    res["deep64_beyond_spread_ms"] = round(max(0.0, res["deep64_ms_best"] - res["rec64_ms_best"] - res["rec_spread_ms"]), 4)
    for name in ("deep100", "deep256", "deep1024"):
        res["%s_over_rec64" % name] = round(res["%s_ms_best" % name] / res["rec64_ms_best"], 3)
    # the calls agree
    got = {name: [u.cpu().numpy() for u in out[name]] for name in out}
    res["deep10_is_recs_bytes"] = bool(all(p.tobytes() == q.tobytes() for p, q in zip(got["deep10"], got["rec"])))
    res["deep64_is_rec64s_bytes"] = bool(all(p.tobytes() == q.tobytes() for p, q in zip(got["deep64"], got["rec64"])))
    d_ids, d_sc, d_cnt = got["deep1024"][0].view(np.uint32).reshape(n, DEEP_MAX), got["deep1024"][1].reshape(n, DEEP_MAX), got["deep1024"][2].view(np.uint32)
    res["deep1024_first_64_are_rec64s"] = bool(d_ids[:, :64].tobytes() == got["rec64"][0].tobytes() and d_sc[:, :64].tobytes() == got["rec64"][1].tobytes())
    res.update(candidates_mean=round(float(d_cnt.mean()), 1), candidates_max=int(d_cnt.max()))
    sample = list(range(0, n, max(1, n // 64)))[:64]
    targets = [d_ids[s, :d_cnt[s]].tolist() for s in sample]
    ranks, scores, _ = m.cf_rank([ids[s].tolist() for s in sample], targets)
    res["sample_ranks_are_the_places"] = bool(ranks.tolist() == [r for tg in targets for r in range(len(tg))] and
                                              scores.tobytes() == np.concatenate([d_sc[s, :d_cnt[s]] for s in sample]).tobytes())
    m.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write("# python3 tools/probe/cf_deep_time.py   (1x MI355X; --ops %g --reps %d --inner %d --sessions %d --global-sessions %d --global-inner %d)\n"
                % (a.ops, a.reps, a.inner, n, ng, a.global_inner))
        f.write("# ms, mean of `inner` calls, best rep.  rec / rec_again = cf_recommend_sim_dev(k = 10) on src.truncated(64, rank=\"cosine\"), the same\n")
        f.write("# call timed twice: rec_spread_ms; rec64 = the same with k = 64; deepK = cf_recommend_deep_dev(k = K) on the same sessions: deep10 and\n")
        f.write("# deep64 are the sim call's launches, deep100 / deep256 / deep1024 the deep ending (a session has at most 8 x 64 candidates there).\n")
        f.write("# gl_* = single-item sessions of the hottest rows of the UNTRUNCATED table (global tier; `gl_inner` calls a rep): the deep call at\n")
        f.write("# k = 1024, cf_rank_dev with one target per session, cf_recommend_sim_dev(k = 64).\n")
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
