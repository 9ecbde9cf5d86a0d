#!/usr/bin/env python3
"""The fill call (smatrix_cf_recommend_fill_dev) next to the recommend call it extends (smatrix_cf_recommend_sim_dev, k = 10), and the
popular call (smatrix_cf_popular_dev) next to the bytes it must move; same process, same matrix, one GPU.

  python3 tools/probe/cf_fill_time.py [--ops 4e8] [--reps 5] [--inner 20] [--sessions 4096] [--out profiles/cf_fill_time.txt]

src = the source of tools/probe/cf_explain_time.py: the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches of 2^24, and
every row's head pair set to the sum of the row's values.  The recommend and fill calls read the serving copy,
src.truncated(64, rank="cosine"); the popular call reads src itself, the table of a million rows.  After one warm-up rep, `reps` reps,
the variants alternated rep by rep, the best rep reported; a rep is `inner` calls back to back between two device synchronisations,
its time the mean per call; every array on the device:
  rec, rec_again   cf_recommend_sim_dev("cosine", 0, k = 10) on `sessions` sessions of 8 ids drawn from the stream's own row ids, timed
                   TWICE: the difference of the two bests is the run's own spread
  fill_warm        cf_recommend_fill_dev on the same sessions with the 1024 most popular ids as its list: nearly no session fills, the
                   call is the yardstick plus one small launch
  fill_cold        cf_recommend_fill_dev on `sessions` sessions of 8 ids without rows: every session fills all 10 places
  popular          cf_popular_dev(4096) on src, against a model of the bytes it moves: the directory once (16 bytes a slot), one
                   64-byte line per row for its head cell, the keys written once (8 bytes a slot) and read once per pass and once by
                   the collection -- at STREAM_TBS, what profiles/experiments_r1_r3.md records for a streaming read
and, as checks, that fill_warm's scored part has rec's bytes, that every cold session is filled with the list's first ids, and that
the popular ids are the numpy model's.  Writes one JSON line under a header to --out and prints it."""
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
from libsmatrix_amd import OP_INCR, POPULAR_MAX, SparseMatrix, Stream  # noqa: E402
from tools.probe.merge_time import B  # noqa: E402

L, K, M, N_FILL = 8, 10, 64, 1024
OP_SET = 1
STREAM_TBS = 5.9                                          # profiles/experiments_r1_r3.md: plain streaming reads, 5.9 - 6.4 TB/s


def passes_of(keys, n):
    """the histogram passes of the device's MSB radix select for the n largest of `keys` (uint64, unique, non-zero)"""
    if keys.size <= n:
        return 0
    dg = (int(np.bitwise_or.reduce(keys)).bit_length() - 1) >> 3
    need, live, passes = n, keys, 0
    while True:
        passes += 1
        d = (live >> np.uint64(8 * dg)) & np.uint64(255)
        hist = np.bincount(d.astype(np.int64), minlength=256)
        above = 0
        for b in range(255, -1, -1):
            if above + hist[b] >= need:
                break
            above += hist[b]
        need -= above
        if dg == 0 or hist[b] == need:
            return passes
        live, dg = live[d == np.uint64(b)], dg - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_fill_time.txt"))
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
    h_rows, h_tot = rows.cpu().numpy().view(np.uint32), totals.cpu().numpy().view(np.uint32)
    del rows, row_ptr, pairs, csum, totals, zeros
    torch.cuda.empty_cache()
    st = src.stats()
    res = {"ops_in_stream": nb * B, "src_rows": st["rows"], "src_dir_slots": st["dir_slots"], "totals": "row sums",
           "copy": "truncated(64, rank='cosine')", "reps": a.reps, "inner": a.inner, "sessions": n, "session_len": L, "k": K, "m": M,
           "n_fill": N_FILL, "n_popular": POPULAR_MAX, "sim": "cosine", "shrink": 0.0}

    # ---- the popular call, on src -----------------------------------------------------------------------------------------------------
    d_pid = torch.zeros(POPULAR_MAX, dtype=torch.int32, device=dev); d_ptot = torch.zeros_like(d_pid)
    d_pn = torch.zeros(1, dtype=torch.int32, device=dev)

    def popular():
        src.cf_popular_dev(POPULAR_MAX, None, 0, 1, d_pid.data_ptr(), d_ptot.data_ptr(), d_pn.data_ptr(), stream)

    t_pop = []
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            popular()
        torch.cuda.synchronize()
        if rep:
            t_pop.append((time.perf_counter() - t0) * 1e3 / a.inner)
    keep = (h_rows != 0) & (h_tot != 0)
    keys = (h_tot[keep].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - h_rows[keep].astype(np.uint64))
    best = np.sort(keys)[::-1][:POPULAR_MAX]
    pop_ids = d_pid.cpu().numpy().view(np.uint32)
    res["popular_found"] = int(d_pn.cpu().numpy()[0])
    res["popular_is_the_models"] = bool(res["popular_found"] == best.size and
                                        (pop_ids[:best.size] == (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.uint32)).all() and
                                        (d_ptot.cpu().numpy().view(np.uint32)[:best.size] == (best >> np.uint64(32)).astype(np.uint32)).all())
    passes = passes_of(keys, POPULAR_MAX)
    slots = st["dir_slots"]
    moved = slots * 16 + int(keep.sum()) * 64 + slots * 8 + (passes + 1) * slots * 8
    res.update(popular_ms_best=round(min(t_pop), 4), popular_ms_all=[round(u, 4) for u in t_pop], popular_passes=passes, popular_bytes_model=moved,
               popular_stream_ms=round(moved / (STREAM_TBS * 1e9), 4), popular_launches=4 + 2 * 8)
    res["popular_share_of_stream"] = round(res["popular_stream_ms"] / res["popular_ms_best"], 4)

    # ---- the recommend and fill calls, on the serving copy ---------------------------------------------------------------------------
    ids = np.ascontiguousarray(sx.astype(np.uint32)).reshape(n, L)
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * L
    d_items = torch.from_numpy(ids.view(np.int32).reshape(-1)).to(dev)
    cold = np.arange(1, 2 * n * L + h_rows.size + 1, dtype=np.uint32)                       # the first n * L ids that have no row
    cold = cold[~np.isin(cold, h_rows)][:n * L].reshape(n, L)
    d_cold = torch.from_numpy(cold.view(np.int32).reshape(-1)).to(dev)
    d_fill = d_pid[:N_FILL].clone()
    m = src.truncated(M, rank="cosine")
    src.close()
    torch.cuda.empty_cache()
    out = {v: (torch.zeros(n * K, dtype=torch.int32, device=dev), torch.zeros(n * K, dtype=torch.float64, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
           for v in ("rec", "rec_again", "fill_warm", "fill_cold")}

    def recommend(v):
        o = [u.data_ptr() for u in out[v]]
        return lambda: m.cf_recommend_sim_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, K, o[0], o[1],
                                              o[2], stream)

    def fill(v, items):
        o = [u.data_ptr() for u in out[v]]
        return lambda: m.cf_recommend_fill_dev(n, d_off.data_ptr(), items.data_ptr(), None, None, None, None, 0, d_fill.data_ptr(), N_FILL,
                                               "cosine", 0.0, K, o[0], o[1], o[2], o[3], stream)

    variants = [("rec", recommend("rec")), ("fill_warm", fill("fill_warm", d_items)), ("fill_cold", fill("fill_cold", d_cold)),
                ("rec_again", recommend("rec_again"))]
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
    res["fill_warm_minus_rec_ms"] = round(res["fill_warm_ms_best"] - yard, 4)
    res["fill_warm_beyond_spread_ms"] = round(max(0.0, res["fill_warm_ms_best"] - yard - res["rec_spread_ms"]), 4)
    # the calls agree
    r, fw, fc = ([u.cpu().numpy() for u in out[v]] for v in ("rec", "fill_warm", "fill_cold"))
    used = np.arange(K)[None, :] < r[2][:, None]
    res["warm_sessions_that_fill"] = int((fw[3] < K).sum())
    res["warm_scored_part_is_recs"] = bool((fw[3] == r[2]).all() and (fw[0].reshape(n, K)[used] == r[0].reshape(n, K)[used]).all() and
                                           (fw[1].reshape(n, K).view(np.uint64)[used] == r[1].reshape(n, K).view(np.uint64)[used]).all())
    res["cold_all_filled_with_the_lists_first"] = bool((fc[3] == 0).all() and (fc[2] == K).all() and
                                                      (fc[0].reshape(n, K) == d_fill.cpu().numpy()[:K][None, :]).all() and not fc[1].any())
    m.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write("# python3 tools/probe/cf_fill_time.py   (1x MI355X; --ops %g --reps %d --inner %d --sessions %d)\n" % (a.ops, a.reps, a.inner, n))
        f.write("# ms, mean of `inner` calls, best rep.  rec / rec_again = cf_recommend_sim_dev(k = 10) on src.truncated(64, rank=\"cosine\"), the same\n")
        f.write("# call timed twice: rec_spread_ms; fill_warm = cf_recommend_fill_dev, same sessions, a 1024-id list; fill_cold = the same on sessions\n")
        f.write("# of ids without rows (every place filled); popular = cf_popular_dev(4096) on src, popular_stream_ms = its bytes model at %.1f TB/s.\n" % STREAM_TBS)
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
