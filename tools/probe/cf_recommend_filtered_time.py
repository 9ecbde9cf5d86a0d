#!/usr/bin/env python3
"""Filtered session recommendations (smatrix_cf_recommend_filtered_dev) next to smatrix_cf_recommend_batch_dev, same process, same
matrix, one GPU.

  python3 tools/probe/cf_recommend_filtered_time.py [--ops 4e8] [--reps 5] [--inner 20] [--sessions 4096] [--only-batch]

The matrix is the serving copy of tools/probe/merge_topk_time.py: truncated(64) of the table that the first `ops` ops of bench.py's
config-2 Zipf stream build.  The query is that probe's too: `sessions` sessions of 8 ids drawn from the stream's own row ids,
k = 10.  Every array is on the device before the clock starts (the _dev flavours: what is timed is the call, not the packing of
Python lists).  The variants:
  a  cf_recommend_batch_dev
  b  cf_recommend_filtered_dev with nothing given (it runs a's kernels)
  c  ... with weights (position i of 8 weighs (i + 1) / 8)
  d  ... with an exclusion list of 256 stream-drawn ids per session
  e  ... with a deny bitmap over 1 M ids, one id in 16 set
After one warm-up rep, `reps` reps, the variants alternated rep by rep; a rep of a variant is `inner` calls back to back between
two device synchronisations, its time the mean per call (one call is about a millisecond: too short a window on its own).
Prints one JSON line: per variant the best rep and all reps, a's spread (its worst rep - its best), and every variant's best
over a's.  --only-batch times a alone and uses nothing newer than cf_recommend_batch_dev, so the same file runs on an older
tree: a on two trees, on one machine in one visit, is how a change to the shared kernels is judged."""
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

B = 1 << 24
L, K, E = 8, 10, 256
DENY_N, DENY_ONE_IN = 1000000, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--only-batch", action="store_true")
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
    ex, _ = gen.fill(L * n, E * n)
    gen.close()
    del x, y, ones
    m = src.truncated(64)
    src.close()
    torch.cuda.empty_cache()

    def up(arr, view):
        return torch.from_numpy(np.ascontiguousarray(arr).view(view)).to(dev)
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * L
    d_items = up(sx.astype(np.uint32), np.int32)
    d_w = torch.from_numpy(np.tile((np.arange(L) + 1.0) / L, n)).to(dev)
    d_exoff = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * E
    d_ex = up(ex.astype(np.uint32), np.int32)
    bits = np.packbits(np.random.default_rng(2026).random(((DENY_N + 31) // 32) * 32) < 1.0 / DENY_ONE_IN, bitorder="little")
    d_deny = up(bits, np.int32)
    out = {}

    def outputs(name):
        out[name] = (torch.zeros(n * K, dtype=torch.int32, device=dev), torch.zeros(n * K, dtype=torch.float64, device=dev),
                     torch.zeros(n, dtype=torch.int32, device=dev))
        return [t.data_ptr() for t in out[name]]

    def batch():
        o = outputs("a")
        return lambda: m.cf_recommend_batch_dev(n, d_off.data_ptr(), d_items.data_ptr(), K, o[0], o[1], o[2], stream)

    def filtered(name, w=None, exoff=None, exi=None, deny=None, deny_n=0):
        o = outputs(name)
        p = lambda t: None if t is None else t.data_ptr()
        return lambda: m.cf_recommend_filtered_dev(n, d_off.data_ptr(), d_items.data_ptr(), p(w), p(exoff), p(exi), p(deny), deny_n, K,
                                                   o[0], o[1], o[2], stream)

    variants = [("a", batch())]
    if not a.only_batch:
        variants += [("b", filtered("b")), ("c", filtered("c", w=d_w)), ("d", filtered("d", exoff=d_exoff, exi=d_ex)),
                     ("e", filtered("e", deny=d_deny, deny_n=DENY_N))]
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
    res = {"ops_in_stream": nb * B, "matrix": "truncated(64)", "sessions": n, "session_len": L, "k": K, "reps": a.reps, "inner": a.inner,
           "exclusion_ids_per_session": E, "deny_n": DENY_N, "deny_set": int(np.unpackbits(bits[:DENY_N // 8]).sum())}
    for name, _ in variants:
        res[name + "_ms_best"] = round(min(t[name]), 4)
        res[name + "_ms_all"] = [round(u, 4) for u in t[name]]
        res[name + "_results"] = int(out[name][2].sum().item())
        if name != "a":
            res[name + "_over_a"] = round(min(t[name]) / min(t["a"]), 4)
    res["a_spread_ms"] = round(max(t["a"]) - min(t["a"]), 4)
    if not a.only_batch:
        res["b_same_bytes_as_a"] = all(torch.equal(p, q) for p, q in zip(out["a"], out["b"]))
    print(json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    main()
