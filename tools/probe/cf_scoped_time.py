#!/usr/bin/env python3
"""The scoped call (smatrix_cf_recommend_scoped_dev) next to the sim call (smatrix_cf_recommend_sim_dev, k = 10); same process, same
matrix, one GPU.

  python3 tools/probe/cf_scoped_time.py [--ops 4e8] [--reps 5] [--inner 20] [--sessions 4096] [--out profiles/cf_scoped_time.txt]

The matrix is tools/probe/cf_grouped_fill_time.py's serving copy: the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches
of 2^24, every row's head pair set to the sum of the row's values, then truncated(64, rank="cosine").  The scope map is id % 1000 over all
of uint32 (16 GiB: a gather from it is as expensive as a gather gets).  After one warm-up rep, `reps` reps, the variants alternated rep
by rep, the best rep reported; a rep is `inner` calls back to back between two device synchronisations, its time the mean per call;
every array on the device; `sessions` sessions of 8 ids drawn from the stream's own row ids:
  sim, sim_again   cf_recommend_sim_dev, timed TWICE: the yardstick, and the difference of the two bests the run's own spread
  no_scope         cf_recommend_scoped_dev with no lists, no quotas, no fill list: the sim call's launches and the fill's one
  only_1, only_8, only_64   ONLY with that many listed groups per session (session s lists s % 1000, s + 1 % 1000, ...: distinct groups)
  except_8         EXCEPT with the lists of only_8
  only_8_fill      only_8 with the 1024 most popular ids of the source as fill list (cf_popular_dev)
and, as checks, that no_scope has the sim call's bytes, that every result id of the ONLY variants is in a listed group and none of
except_8 is, and that only_8_fill's scored part is only_8's.  Writes one JSON line under a header to --out and prints it."""
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

L, K, M, N_GROUPS, N_FILL = 8, 10, 64, 1000, 1024
OP_SET = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_scoped_time.txt"))
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
           "inner": a.inner, "sessions": n, "session_len": L, "k": K, "m": M, "n_fill": N_FILL, "scope_of": "id %% %d" % N_GROUPS,
           "sim": "cosine", "shrink": 0.0}
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
    scope_n = 1 << 32                                                     # the stream's ids are fmix32(rank): the map covers every uint32
    d_scp = torch.empty(scope_n, dtype=torch.int32, device=dev)
    for c in range(0, scope_n, 1 << 28):
        i = torch.arange(c, c + (1 << 28), dtype=torch.int64, device=dev)
        d_scp[c:c + (1 << 28)] = (i % N_GROUPS).to(torch.int32)
    del i
    res["scope_n"] = scope_n
    lists = {w: (np.arange(n)[:, None] + np.arange(w)[None, :]) % N_GROUPS for w in (1, 8, 64)}      # session s: s, s + 1, ... mod 1000
    d_lists = {w: (torch.arange(0, n + 1, dtype=torch.int64, device=dev) * w, torch.from_numpy(v.astype(np.int32).reshape(-1)).to(dev))
               for w, v in lists.items()}
    names = ("sim", "no_scope", "only_1", "only_8", "only_64", "except_8", "only_8_fill", "sim_again")
    out = {v: (torch.zeros(n * K, dtype=torch.int32, device=dev), torch.zeros(n * K, dtype=torch.float64, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for v in names}

    def sim(v):
        o = [u.data_ptr() for u in out[v]]
        return lambda: m.cf_recommend_sim_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, "cosine", 0.0, K, o[0], o[1], o[2],
                                              stream)

    def scoped(v, width, mode, fill):
        o = [u.data_ptr() for u in out[v]]
        sc = (None, 0, None, None) if width is None else (d_scp.data_ptr(), scope_n, d_lists[width][0].data_ptr(), d_lists[width][1].data_ptr())
        fl = (d_fill.data_ptr(), N_FILL) if fill else (None, 0)
        return lambda: m.cf_recommend_scoped_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, None, None, None, 0, *sc, mode, None, 0, 64, *fl,
                                                 "cosine", 0.0, K, o[0], o[1], o[2], o[3], stream)

    variants = [("sim", sim("sim")), ("no_scope", scoped("no_scope", None, "only", False)), ("only_1", scoped("only_1", 1, "only", False)),
                ("only_8", scoped("only_8", 8, "only", False)), ("only_64", scoped("only_64", 64, "only", False)),
                ("except_8", scoped("except_8", 8, "except", False)), ("only_8_fill", scoped("only_8_fill", 8, "only", True)),
                ("sim_again", sim("sim_again"))]
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
    yard = min(res["sim_ms_best"], res["sim_again_ms_best"])
    res["sim_spread_ms"] = round(abs(res["sim_ms_best"] - res["sim_again_ms_best"]), 4)
    for name in names[1:-1]:
        res["%s_over_sim" % name] = round(res["%s_ms_best" % name] / yard, 3)
    # the calls agree
    got = {v: [u.cpu().numpy() for u in out[v]] for v in names}
    shaped = lambda v: (got[v][0].view(np.uint32).reshape(n, K), got[v][1].reshape(n, K).view(np.uint64), got[v][2].view(np.uint32))   # noqa: E731
    s_ids, s_sc, s_cnt = shaped("sim")
    u_ids, u_sc, u_cnt = shaped("no_scope")
    used = np.arange(K)[None, :] < s_cnt[:, None]
    res["no_scope_is_the_sim_call"] = bool((u_cnt == s_cnt).all() and (u_ids[used] == s_ids[used]).all() and (u_sc[used] == s_sc[used]).all())
    res["sim_results_mean"] = round(float(s_cnt.mean()), 3)
    for v, w, inside in (("only_1", 1, True), ("only_8", 8, True), ("only_64", 64, True), ("except_8", 8, False), ("only_8_fill", 8, True)):
        r_ids, _, cnt = shaped(v)
        live = np.arange(K)[None, :] < cnt[:, None]
        hit = ((r_ids.astype(np.int64) % N_GROUPS)[:, :, None] == lists[w][:, None, :]).any(axis=2)
        res["%s_results_mean" % v] = round(float(cnt.mean()), 3)
        res["%s_scope_holds" % v] = bool((hit[live] == inside).all())
    o_ids, o_sc, o_cnt = shaped("only_8")
    f_ids, f_sc, _ = shaped("only_8_fill")
    f_nsc = got["only_8_fill"][3].view(np.uint32)
    used = np.arange(K)[None, :] < o_cnt[:, None]
    res["fill_scored_part_is_only_8s"] = bool((f_nsc == o_cnt).all() and (f_ids[used] == o_ids[used]).all() and (f_sc[used] == o_sc[used]).all())
    m.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write("# python3 tools/probe/cf_scoped_time.py   (1x MI355X; --ops %g --reps %d --inner %d --sessions %d)\n" % (a.ops, a.reps, a.inner, n))
        f.write("# ms, mean of `inner` calls, best rep.  On src.truncated(64, rank=\"cosine\"), k = 10, the scope map id % 1000 over all of uint32.\n")
        f.write("# sim / sim_again = cf_recommend_sim_dev timed twice: sim_spread_ms; no_scope = cf_recommend_scoped_dev without lists; only_W =\n")
        f.write("# ONLY with W listed groups per session; except_8 = EXCEPT with 8; only_8_fill = only_8 with the 1024 most popular ids as fill\n")
        f.write("# list.  *_over_sim = the variant's best over the better of the two sim bests.\n")
        f.write("# NOT measured: the global tier (these sessions are the LDS tier's), quotas together with a scope, a list longer than 1024 ids,\n")
        f.write("# a small map that stays in cache, and the host flavour's staging of map and lists.\n")
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
