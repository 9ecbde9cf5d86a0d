#!/usr/bin/env python3
"""The explain call (smatrix_cf_explain_dev) next to the recommend call whose results it explains (smatrix_cf_recommend_sim_dev,
k = 10), same process, same matrix, same sessions, one GPU.

  python3 tools/probe/cf_explain_time.py [--ops 4e8] [--reps 5] [--inner 20] [--sessions 4096] [--out profiles/cf_explain_time.txt]

src = the source of tools/probe/cf_rank_time.py: the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches of 2^24, and
every row's head pair set to the sum of the row's values.  `sessions` sessions of 8 ids drawn from the stream's own row ids.  The
matrix read is the serving copy, src.truncated(64, rank="cosine"); the untruncated table, where a recommend call takes over a
second, is NOT measured here.  After one warm-up rep, `reps` reps, the variants alternated rep by rep, the best rep reported; a rep
is `inner` calls back to back between two device synchronisations, its time the mean per call; every array on the device:
  rec, rec_again   cf_recommend_sim_dev("cosine", 0, k = 10), timed TWICE: the difference of the two bests is the run's own spread
  explain          cf_explain_dev("cosine", 0) with the 10 ids rec returned for every session as its targets (unused slots hold the
                   id 0): 10 * 8 entries a session
and, as a check, that the left fold of every returned id's terms has the bytes of its score.
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
from tools.probe.merge_time import B  # noqa: E402

L, K, M = 8, 10, 64
OP_SET = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_explain_time.txt"))
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
    res = {"ops_in_stream": nb * B, "src_rows": src.stats()["rows"], "totals": "row sums", "copy": "truncated(64, rank='cosine')", "reps": a.reps,
           "inner": a.inner, "sessions": n, "session_len": L, "targets_per_session": K, "entries": n * K * L, "k": K, "m": M, "sim": "cosine",
           "shrink": 0.0}
    ids = np.ascontiguousarray(sx.astype(np.uint32)).reshape(n, L)
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * L
    d_items = torch.from_numpy(ids.view(np.int32).reshape(-1)).to(dev)
    d_toff = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * K
    d_eoff = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * (K * L)
    m = src.truncated(M, rank="cosine")
    src.close()
    torch.cuda.empty_cache()
    rec = {v: (torch.zeros(n * K, dtype=torch.int32, device=dev), torch.zeros(n * K, dtype=torch.float64, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev)) for v in ("rec", "rec_again")}
    d_terms = torch.zeros(n * K * L, dtype=torch.float64, device=dev)
    d_cc = torch.zeros(n * K * L, dtype=torch.int32, device=dev)

    def recommend(v):
        o = [u.data_ptr() for u in rec[v]]
        return lambda: m.cf_recommend_sim_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, K, o[0], o[1],
                                              o[2], stream)

    def explain():
        m.cf_explain_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, "cosine", 0.0, d_toff.data_ptr(), rec["rec"][0].data_ptr(),
                         d_eoff.data_ptr(), n * K * L, d_terms.data_ptr(), d_cc.data_ptr(), stream)

    variants = [("rec", recommend("rec")), ("explain", explain), ("rec_again", recommend("rec_again"))]
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
    res["rec_spread_ms"] = round(abs(res["rec_ms_best"] - res["rec_again_ms_best"]), 4)
    res["explain_over_rec"] = round(res["explain_ms_best"] / min(res["rec_ms_best"], res["rec_again_ms_best"]), 4)
    # the two calls agree: the terms of a returned id add up, left to right, to the bytes of its score
    terms = d_terms.cpu().numpy().reshape(n, K, L)
    sc, cnt = rec["rec"][1].cpu().numpy().reshape(n, K), rec["rec"][2].cpu().numpy()
    acc = np.zeros((n, K), np.float64)
    for i in range(L):
        acc = acc + terms[:, :, i]
    used = np.arange(K)[None, :] < cnt[:, None]
    res["returned_ids"] = int(used.sum())
    res["terms_add_up_to_the_scores"] = bool((acc.view(np.uint64)[used] == sc.view(np.uint64)[used]).all() and not acc[~used].any())
    res["entries_with_a_cell"] = int(np.count_nonzero(d_cc.cpu().numpy()))
    m.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write("# python3 tools/probe/cf_explain_time.py   (1x MI355X; --ops %g --reps %d --inner %d --sessions %d)\n" % (a.ops, a.reps, a.inner, n))
        f.write("# ms, mean of `inner` calls, best rep, on src.truncated(64, rank=\"cosine\").  rec / rec_again = cf_recommend_sim_dev(k = 10), the same\n")
        f.write("# call timed twice: rec_spread_ms; explain = cf_explain_dev for the 10 ids rec returned per session (10 * 8 entries a session).\n")
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
