#!/usr/bin/env python3
"""The rank call (smatrix_cf_rank_dev) next to the recommend call it shares everything but the ending with
(smatrix_cf_recommend_sim_dev, k = 10), same process, same matrix, same sessions, one GPU -- and the numbers the call exists for.

  python3 tools/probe/cf_rank_time.py [--ops 4e8] [--reps 5] [--inner 20] [--inner-pruned 1] [--sessions 4096]
                                      [--out profiles/cf_rank_time.txt]

src = the source of tools/probe/cf_sim_time.py: the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches of 2^24, and
every row's head pair set to the sum of the row's values.  `sessions` sessions of 8 ids drawn from the stream's own row ids: the
first 7 are the session, the 8th is its one target.  On each of two copies, src.pruned(1) (every pair) and
src.truncated(64, rank="cosine"), after one warm-up rep, `reps` reps, the variants alternated rep by rep, the best rep reported; a
rep is `inner` calls back to back between two device synchronisations, its time the mean per call (on the pruned copy
`inner-pruned` calls: there the hot rows make every session a global-tier one and a call takes seconds, which needs no averaging
and at 20 calls a rep would take minutes); every array on the device:
  rec, rec_again   cf_recommend_sim_dev("cosine", 0, k = 10), timed TWICE: the difference of the two bests is the run's own spread
  rank             cf_rank_dev("cosine", 0) with the one target per session
and rank_metrics of the ranks (hit rate at 10 and 100, MRR) on both copies: what the truncation costs in accuracy is the difference
(this table's rows are Zipf draws without item-to-item structure, so the figures are small; the difference is what to look at).
Writes one JSON line under a header to --out and prints it."""
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
from libsmatrix_amd import OP_INCR, SparseMatrix, Stream, rank_metrics  # noqa: E402
from tools.probe.merge_time import B  # noqa: E402

L, K, M = 7, 10, 64
OP_SET = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--inner-pruned", type=int, default=1)
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_rank_time.txt"))
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
    sx, _ = gen.fill(0, (L + 1) * n)
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
    res = {"ops_in_stream": nb * B, "src_rows": src.stats()["rows"], "totals": "row sums", "reps": a.reps, "inner": a.inner,
           "inner_pruned": a.inner_pruned, "sessions": n,
           "session_len": L, "targets_per_session": 1, "k": K, "m": M, "sim": "cosine", "shrink": 0.0}
    ids = np.ascontiguousarray(sx.astype(np.uint32)).reshape(n, L + 1)
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * L
    d_items = torch.from_numpy(np.ascontiguousarray(ids[:, :L]).view(np.int32).reshape(-1)).to(dev)
    d_toff = torch.arange(0, n + 1, dtype=torch.int64, device=dev)
    d_tg = torch.from_numpy(np.ascontiguousarray(ids[:, L]).view(np.int32)).to(dev)
    copies = [("pruned", src.pruned(1)), ("trunc", src.truncated(M, rank="cosine"))]
    src.close()
    torch.cuda.empty_cache()
    for tag, m in copies:
        rec = {v: (torch.zeros(n * K, dtype=torch.int32, device=dev), torch.zeros(n * K, dtype=torch.float64, device=dev),
                   torch.zeros(n, dtype=torch.int32, device=dev)) for v in ("rec", "rec_again")}
        d_ranks = torch.zeros(n, dtype=torch.int32, device=dev)
        d_sc = torch.zeros(n, dtype=torch.float64, device=dev)
        d_nc = torch.zeros(n, dtype=torch.int32, device=dev)

        def recommend(v):
            o = [u.data_ptr() for u in rec[v]]
            return lambda: m.cf_recommend_sim_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, K, o[0], o[1],
                                                  o[2], stream)

        def rank():
            m.cf_rank_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, d_toff.data_ptr(), d_tg.data_ptr(),
                          d_ranks.data_ptr(), d_sc.data_ptr(), d_nc.data_ptr(), stream)

        variants = [("rec", recommend("rec")), ("rank", rank), ("rec_again", recommend("rec_again"))]
        t = {name: [] for name, _ in variants}
        inner = a.inner_pruned if tag == "pruned" else a.inner
        for rep in range(a.reps + 1):                  # rep 0 is the warm-up
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                if rep:
                    t[name].append((time.perf_counter() - t0) * 1e3 / inner)
            print("# %s rep %d of %d done" % (tag, rep, a.reps), flush=True)
        for name, _ in variants:
            res["%s_%s_ms_best" % (tag, name)] = round(min(t[name]), 4)
            res["%s_%s_ms_all" % (tag, name)] = [round(u, 4) for u in t[name]]
        res[tag + "_rec_spread_ms"] = round(abs(res[tag + "_rec_ms_best"] - res[tag + "_rec_again_ms_best"]), 4)
        res[tag + "_rank_over_rec"] = round(res[tag + "_rank_ms_best"] / min(res[tag + "_rec_ms_best"], res[tag + "_rec_again_ms_best"]), 4)
        ranks = d_ranks.cpu().numpy().view(np.uint32)
        got = rank_metrics(ranks, (10, 100))
        res[tag + "_targets_found"] = got["found"]
        res[tag + "_hit_rate_10"], res[tag + "_hit_rate_100"], res[tag + "_mrr"] = round(got["hit_rate"][10], 5), round(got["hit_rate"][100], 5), round(got["mrr"], 6)
        res[tag + "_candidates_mean"] = round(float(d_nc.cpu().numpy().view(np.uint32).mean()), 1)
        # the two calls agree: a target the recommend call returned at r has the rank r
        r_ids, r_cnt = rec["rec"][0].cpu().numpy().view(np.uint32).reshape(n, K), rec["rec"][2].cpu().numpy()
        at = [np.flatnonzero(r_ids[s, :r_cnt[s]] == ids[s, L]) for s in range(n)]
        res[tag + "_ranks_agree_with_rec"] = all((a_.size == 0 and not ranks[s] < K) or (a_.size == 1 and ranks[s] == a_[0]) for s, a_ in enumerate(at))
        m.close()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write("# python3 tools/probe/cf_rank_time.py   (1x MI355X; --ops %g --reps %d --inner %d --inner-pruned %d --sessions %d)\n"
                % (a.ops, a.reps, a.inner, a.inner_pruned, n))
        f.write("# ms, mean of `inner` calls (pruned: `inner_pruned`), best rep.  rec / rec_again = cf_recommend_sim_dev(k = 10), the same call timed twice: *_rec_spread_ms;\n")
        f.write("# rank = cf_rank_dev, one target per session.  pruned = src.pruned(1), trunc = src.truncated(64, rank=\"cosine\").\n")
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
