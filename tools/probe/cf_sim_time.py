#!/usr/bin/env python3
"""The similarity measures (smatrix_cf_recommend_sim_dev, smatrix_merge_topk_sim) next to the cosine calls they extend
(smatrix_cf_recommend_filtered_dev, smatrix_merge_topk_by), same process, same matrix, one GPU.

  python3 tools/probe/cf_sim_time.py [--ops 4e8] [--reps 5] [--inner 20] [--sessions 4096] [--out profiles/cf_sim_time.txt]

src = the source of tools/probe/merge_topk_by_time.py: the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches of
2^24, and every row's head pair set to the sum of the row's values (the stream writes no column 0, and without totals every score
is 0).  Two tables, each after one warm-up rep, `reps` reps, the variants alternated rep by rep, the best rep reported:
  recommend  on src.truncated(64, rank="cosine"), `sessions` sessions of 8 ids drawn from the stream's own row ids, k = 10, every
             array on the device; a rep is `inner` calls back to back between two device synchronisations, its time the mean per
             call.  The yardstick is cf_recommend_filtered_dev with nothing given, timed TWICE (old, old_again): the difference of
             their bests is the run-to-run spread.  Then cf_recommend_sim_dev for each measure with shrink 0 and 10 -- ("cosine",
             0) is the yardstick's own code path.
  truncate   src.truncated(64, rank=R, shrink=h) into a new matrix, wall time around the whole call with the device idle before
             and synchronised after.  The yardstick is rank="cosine", timed twice; then cosine with shrink 10, jaccard and lift
             with shrink 0 and 10.
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
from libsmatrix_amd import OP_INCR, SparseMatrix, Stream  # noqa: E402
from tools.probe.merge_time import B, wall  # noqa: E402

L, K, M = 8, 10, 64
OP_SET = 1
NEW = [("cosine", 10.0), ("jaccard", 0.0), ("jaccard", 10.0), ("lift", 0.0), ("lift", 10.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_sim_time.txt"))
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
    res = {"ops_in_stream": nb * B, "src_rows": st["rows"], "totals": "row sums", "reps": a.reps, "inner": a.inner, "sessions": n,
           "session_len": L, "k": K, "m": M}

    # ---- truncate ----
    makers = [("trunc_old", lambda: src.truncated(M, rank="cosine")), ("trunc_old_again", lambda: src.truncated(M, rank="cosine"))]
    makers += [("trunc_%s_%g" % (r, h), (lambda r=r, h=h: src.truncated(M, rank=r, shrink=h))) for r, h in NEW]
    t = {name: [] for name, _ in makers}
    for rep in range(a.reps + 1):                      # rep 0 is the warm-up
        for name, make in makers:
            out = []
            ms = wall(lambda: out.append(make()))
            if rep == a.reps:
                res[name + "_pairs"] = int(out[0].export_dev("table")[2].shape[0])
            out[0].close()
            if rep:
                t[name].append(ms)
    for name, _ in makers:
        res[name + "_ms_best"] = round(min(t[name]), 3)
        res[name + "_ms_all"] = [round(u, 2) for u in t[name]]
    res["trunc_spread_ms"] = round(abs(res["trunc_old_ms_best"] - res["trunc_old_again_ms_best"]), 3)
    for r, h in NEW:
        res["trunc_%s_%g_over_old" % (r, h)] = round(res["trunc_%s_%g_ms_best" % (r, h)] / res["trunc_old_ms_best"], 4)

    # ---- recommend ----
    m = src.truncated(M, rank="cosine")
    src.close()
    torch.cuda.empty_cache()
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * L
    d_items = torch.from_numpy(np.ascontiguousarray(sx.astype(np.uint32)).view(np.int32)).to(dev)
    out = {}

    def outputs(name):
        out[name] = (torch.zeros(n * K, dtype=torch.int32, device=dev), torch.zeros(n * K, dtype=torch.float64, device=dev),
                     torch.zeros(n, dtype=torch.int32, device=dev))
        return [u.data_ptr() for u in out[name]]

    def old(name):
        o = outputs(name)
        return lambda: m.cf_recommend_filtered_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, K, o[0], o[1], o[2], stream)

    def new(name, sim, shrink):
        o = outputs(name)
        return lambda: m.cf_recommend_sim_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, sim, shrink, K, o[0], o[1],
                                              o[2], stream)

    variants = [("rec_old", old("rec_old")), ("rec_old_again", old("rec_old_again")), ("rec_cosine_0", new("rec_cosine_0", "cosine", 0.0))]
    variants += [("rec_%s_%g" % (r, h), new("rec_%s_%g" % (r, h), r, h)) for r, h in NEW]
    t = {name: [] for name, _ in variants}
    for rep in range(a.reps + 1):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.inner):
                fn()
            torch.cuda.synchronize()
            if rep:
                t[name].append((time.perf_counter() - t0) * 1e3 / a.inner)
    for name, _ in variants:
        res[name + "_ms_best"] = round(min(t[name]), 4)
        res[name + "_ms_all"] = [round(u, 4) for u in t[name]]
        res[name + "_results"] = int(out[name][2].sum().item())
    res["rec_spread_ms"] = round(abs(res["rec_old_ms_best"] - res["rec_old_again_ms_best"]), 4)
    for name, _ in variants[2:]:
        res[name + "_over_old"] = round(res[name + "_ms_best"] / res["rec_old_ms_best"], 4)
    res["rec_cosine_0_same_bytes_as_old"] = all(torch.equal(p, q) for p, q in zip(out["rec_old"], out["rec_cosine_0"]))
    m.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write("# python3 tools/probe/cf_sim_time.py   (1x MI355X; --ops %g --reps %d --inner %d --sessions %d)\n" % (a.ops, a.reps, a.inner, n))
        f.write("# ms.  trunc_*: SparseMatrix.truncated(64, rank, shrink), wall time of the call; rec_*: cf_recommend_*_dev, mean of `inner` calls.\n")
        f.write("# old = the cosine call that was there before (rank=\"cosine\" / cf_recommend_filtered_dev), timed twice: *_spread_ms.\n")
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
