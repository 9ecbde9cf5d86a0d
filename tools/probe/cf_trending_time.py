#!/usr/bin/env python3
"""The trending call (smatrix_cf_trending_dev, n = 4096) for each measure next to the popular call (smatrix_cf_popular_dev, n = 4096) on
the same matrix; same process, one GPU.

  python3 tools/probe/cf_trending_time.py [--ops 4e8] [--reps 5] [--inner 20] [--out profiles/cf_trending_time.txt]

now = the source of tools/probe/cf_fill_time.py: the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches of 2^24, and
every row's head pair set to the sum of the row's values.  base = an empty matrix after merge_scaled(now, "set", num = 1, den = 2): the
same ids, every total halved.  After one warm-up rep, `reps` reps, the variants alternated rep by rep, the best rep reported; a rep is
`inner` calls back to back between two device synchronisations, its time the mean per call; every array on the device:
  popular, popular_again   cf_popular_dev(4096) on now, timed TWICE: the difference of the two bests is the run's own spread
  gain, ratio, zscore      cf_trending_dev(base, 4096, measure, num = 1, den = 1, shrink = 0)
and, as checks, that each measure's ids, score bytes, totals and expected values are the numpy model's over the exported heads.
What the code leads one to expect of the ratio to popular: up to 12 digit passes against 8, 12-byte keys against 8, and one more
dependent look-up per row in the key pass.  Not measured here: the host flavour, file-backed matrices, a base much larger than now.
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
from libsmatrix_amd import OP_INCR, POPULAR_MAX, SparseMatrix, Stream  # noqa: E402
from tools.probe.merge_time import B  # noqa: E402

OP_SET = 1
MEASURES = ("gain", "ratio", "zscore")


def model(ids, T, Bt, measure, n):
    """the header's contract over the heads (num = den = 1, shrink = 0) -> (ids, scores, totals, expected)"""
    keep = (ids != 0) & (T >= 1) & (T > Bt)
    ids, T, E = ids[keep], T[keep], Bt[keep]
    G = (T.astype(np.uint64) - E.astype(np.uint64)).astype(np.float64)
    D = E.astype(np.float64)
    D[D == 0.0] = 1.0
    score = G if measure == "gain" else G / D if measure == "ratio" else G / np.sqrt(D)
    order = np.lexsort((ids, -score))[:n]
    return ids[order], score[order], T[order], E[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_trending_time.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    now = SparseMatrix()
    gen = Stream("zipf", bench.SEED, bench.N_IDS, bench.ZIPF_S, 1)
    x = torch.empty(B, dtype=torch.int32, device=dev); y = torch.empty_like(x); ones = torch.ones_like(x)
    nb = max(1, int(a.ops) // B)
    for s in range(nb):
        gen.fill_device(s * B, B, x.data_ptr(), y.data_ptr(), stream)
        now.apply_batch_dev(OP_INCR, B, x.data_ptr(), y.data_ptr(), ones.data_ptr(), None, stream)
    torch.cuda.synchronize()
    gen.close()
    del x, y, ones
    rows, row_ptr, pairs = now.export_dev("table")                       # the totals: (x, 0, sum of row x)
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(pairs[:, 1].to(torch.int64) & 0xFFFFFFFF, 0)])
    totals = (csum[row_ptr[1:]] - csum[row_ptr[:-1]]).clamp(max=0x7FFFFFFF).to(torch.int32)
    zeros = torch.zeros_like(rows)
    torch.cuda.synchronize()
    for s in range(0, rows.numel(), B):
        c = min(B, rows.numel() - s)
        now.apply_batch_dev(OP_SET, c, rows[s:].data_ptr(), zeros[s:].data_ptr(), totals[s:].data_ptr(), None, stream)
    torch.cuda.synchronize()
    h_rows, h_tot = rows.cpu().numpy().view(np.uint32), totals.cpu().numpy().view(np.uint32)
    del rows, row_ptr, pairs, csum, totals, zeros
    torch.cuda.empty_cache()
    base = SparseMatrix()
    base.merge_scaled(now, "set", num=1, den=2)
    print("# matrices built", flush=True)
    st, sb = now.stats(), base.stats()
    n = POPULAR_MAX
    res = {"ops_in_stream": nb * B, "now_rows": st["rows"], "now_dir_slots": st["dir_slots"], "base_rows": sb["rows"],
           "base_dir_slots": sb["dir_slots"], "totals": "row sums", "base": "merge_scaled(now, 'set', 1, 2)", "reps": a.reps, "inner": a.inner,
           "n": n, "num": 1, "den": 1, "shrink": 0.0}

    d_pid = torch.zeros(n, dtype=torch.int32, device=dev); d_ptot = torch.zeros_like(d_pid); d_pn = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {m: (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.float64, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
               torch.zeros(1, dtype=torch.int32, device=dev)) for m in MEASURES}

    def popular():
        now.cf_popular_dev(n, None, 0, 1, d_pid.data_ptr(), d_ptot.data_ptr(), d_pn.data_ptr(), stream)

    def trending(m):
        o = [u.data_ptr() for u in out[m]]
        return lambda: now.cf_trending_dev(base, n, m, 1, 1, 0.0, None, 0, 1, 1, o[0], o[1], o[2], o[3], o[4], stream)

    variants = [("popular", popular)] + [(m, trending(m)) for m in MEASURES] + [("popular_again", popular)]
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
    yard = min(res["popular_ms_best"], res["popular_again_ms_best"])
    res["popular_spread_ms"] = round(abs(res["popular_ms_best"] - res["popular_again_ms_best"]), 4)
    for m in MEASURES:
        res["%s_over_popular" % m] = round(res["%s_ms_best" % m] / yard, 3)

    # the calls agree with the model
    h_base = np.asarray(base.get_batch(h_rows, np.zeros(h_rows.size, np.uint32)), np.uint32)
    res["base_totals_are_half"] = bool((h_base == h_tot // 2).all())
    for m in MEASURES:
        ids, sc, tot, exp, nf = (u.cpu().numpy() for u in out[m])
        want = model(h_rows, h_tot, h_base, m, n)
        res["%s_found" % m] = int(nf[0])
        res["%s_is_the_models" % m] = bool(int(nf[0]) == want[0].size and (ids.view(np.uint32)[:want[0].size] == want[0]).all() and
                                           sc[:want[0].size].tobytes() == want[1].tobytes() and
                                           (tot.view(np.uint32)[:want[0].size] == want[2]).all() and
                                           (exp.view(np.uint32)[:want[0].size] == want[3]).all())
    now.close()
    base.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write("# python3 tools/probe/cf_trending_time.py   (1x MI355X; --ops %g --reps %d --inner %d)\n" % (a.ops, a.reps, a.inner))
        f.write("# ms, mean of `inner` calls, best rep, variants alternated.  popular / popular_again = cf_popular_dev(4096) on now, the same call\n")
        f.write("# timed twice: popular_spread_ms; gain / ratio / zscore = cf_trending_dev(base, 4096, measure, 1, 1, 0.0) with base = now's\n")
        f.write("# merge_scaled(1, 2) copy; *_over_popular = the ratio to the better popular time.  Not measured: the host flavour, file-backed\n")
        f.write("# matrices, a base much larger than now.  No profile was taken: where the time goes inside a call is not measured.\n")
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
