#!/usr/bin/env python3
"""SparseMatrix.truncated(m, rank="cosine") (smatrix_merge_topk_by) next to truncated(64) by value (smatrix_merge_topk, the
yardstick) of the same source, same process, one GPU.

  python3 tools/probe/merge_topk_by_time.py [--ops 4e8] [--reps 5] [--sessions 4096]

src = the source of tools/probe/merge_topk_time.py (the first `ops` ops of bench.py's config-2 Zipf stream, incr in batches of
2^24) with ONE addition: the stream writes no column 0, and without totals every cosine is 0, so every row gets the head pair
(x, 0, sum of the row's values) -- what the CF import leaves there up to the factor of the session length.  Timed, after one
warm-up rep, `reps` times, alternated rep by rep, every call into a new matrix: truncated(64) by value, then
truncated(m, rank="cosine") for m = 16, 64, 256; wall time around the whole call with the device idle before and synchronised
after.  The selection kernels alone: one more call per flavour with smatrix_profile on, the library's own HIP-event line.  For
every copy: its pair count, and the overlap of its cf_recommend_batch(k = 10) ids with those of the untruncated matrix on one
fixed set of sessions of 8 ids each, drawn from the stream's own row ids.  (Passes per row are not counted: the kernels keep no
counters.)  Prints one JSON line."""
import argparse
import json
import os
import re
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libsmatrix_amd import OP_INCR, SparseMatrix, Stream  # noqa: E402
from tools.probe.merge_time import B, wall  # noqa: E402

MS = (16, 64, 256)
OP_SET = 1


def profiled(src, m, rank):
    """the library's stderr lines of a profiled merge_topk(m, rank=rank): (selection ms, count scan ms, emission ms)"""
    d = SparseMatrix()
    d.profile(True)
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            d.merge_topk(src, m, "set", 1, rank=rank)
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    d.close()
    out = []
    for pat in (r"selection ([0-9.]+) ms", r"count scan ([0-9.]+) ms", r"record emission ([0-9.]+) ms"):
        g = re.search(pat, text)
        out.append(float(g.group(1)) if g else None)
    return out


def overlap(ids, counts, ref_ids, ref_counts):
    """the share of the reference's recommended ids that the copy recommends too, over all sessions"""
    hit = tot = 0
    for i in range(ids.shape[0]):
        want = set(ref_ids[i, :int(ref_counts[i])].tolist())
        hit += len(want & set(ids[i, :int(counts[i])].tolist()))
        tot += len(want)
    return hit / max(tot, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sessions", type=int, default=4096)
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
    sx, _ = gen.fill(0, 8 * a.sessions)
    sessions = [sx[8 * i:8 * i + 8] for i in range(a.sessions)]
    gen.close()
    del x, y, ones
    # the totals: (x, 0, sum of row x)
    rows, row_ptr, pairs = src.export_dev("table")
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(pairs[:, 1].to(torch.int64) & 0xFFFFFFFF, 0)])
    totals = (csum[row_ptr[1:]] - csum[row_ptr[:-1]]).clamp(max=0x7FFFFFFF).to(torch.int32)
    zeros = torch.zeros_like(rows)
    torch.cuda.synchronize()
    for s in range(0, rows.numel(), B):
        n = min(B, rows.numel() - s)
        src.apply_batch_dev(OP_SET, n, rows[s:].data_ptr(), zeros[s:].data_ptr(), totals[s:].data_ptr(), None, stream)
    torch.cuda.synchronize()
    del rows, row_ptr, pairs, csum, totals, zeros
    torch.cuda.empty_cache()

    makers = [("value_64", lambda: src.truncated(64))] + [("cosine_%d" % m, (lambda m=m: src.truncated(m, rank="cosine"))) for m in MS]
    t = {name: [] for name, _ in makers}
    for rep in range(a.reps + 1):                      # rep 0 is the warm-up
        for name, make in makers:
            out = []
            ms = wall(lambda: out.append(make()))
            out[0].close()
            if rep:
                t[name].append(ms)
    st = src.stats()
    res = {"ops_in_stream": nb * B, "src_rows": st["rows"], "src_table_bytes": (st["arena_units"] - st["arena_free_units"]) * 128,
           "totals": "row sums", "reps": a.reps, "sessions": a.sessions, "session_len": 8, "k": 10}
    ref_ids, _, ref_counts = src.cf_recommend_batch(sessions, 10)
    for name, make in makers:
        res[name + "_ms_best"] = min(t[name])
        res[name + "_ms_all"] = [round(u, 2) for u in t[name]]
        c = make()
        res[name + "_pairs"] = int(c.export_dev("table")[2].shape[0])
        ids, _, counts = c.cf_recommend_batch(sessions, 10)
        res[name + "_recommend_overlap"] = round(overlap(ids, counts, ref_ids, ref_counts), 4)
        c.close()
        torch.cuda.empty_cache()
    for name, m, rank in [("value_64", 64, "value")] + [("cosine_%d" % m, m, "cosine") for m in MS]:
        sel, scan, emit = profiled(src, m, rank)
        res[name + "_selection_ms"], res[name + "_count_scan_ms"], res[name + "_emit_ms"] = sel, scan, emit
    for m in MS:
        res["cosine_%d_selection_over_value_64" % m] = res["cosine_%d_selection_ms" % m] / res["value_64_selection_ms"]
        res["cosine_%d_over_value_64" % m] = res["cosine_%d_ms_best" % m] / res["value_64_ms_best"]
    print(json.dumps(res), flush=True)
    src.close()


if __name__ == "__main__":
    main()
