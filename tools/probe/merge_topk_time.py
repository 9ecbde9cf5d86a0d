#!/usr/bin/env python3
"""SparseMatrix.truncated(m) (smatrix_merge_topk) next to SparseMatrix.pruned(1) (smatrix_merge_scaled) of the same source, same
process, one GPU.

  python3 tools/probe/merge_topk_time.py [--ops 4e8] [--reps 5] [--sessions 4096]

src = the source of tools/probe/merge_scaled_time.py: the first `ops` ops of bench.py's config-2 Zipf stream, in batches of 2^24
incr (4e8: 1 M rows / 100 M pairs).  Timed, after one warm-up rep, `reps` times, alternated rep by rep, every call into a new
matrix: pruned(1), truncated(16), truncated(64), truncated(256); wall time around the whole call with the device idle before and
synchronised after.  The selection kernels alone: one more truncated(m) per m with smatrix_profile on, the library's own
HIP-event line.  For every copy: its pair count, its `mem`, and the time of cf_recommend_batch(k = 10) on one fixed set of
sessions of 8 ids each, drawn from the stream's own row ids (so hot rows are in them as often as the stream writes them), best
of 3 after a warm-up.  Prints one JSON line."""
import argparse
import json
import os
import re
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libsmatrix_amd import OP_INCR, SparseMatrix, Stream  # noqa: E402
from tools.probe.merge_time import B, wall  # noqa: E402

MS = (16, 64, 256)


def profiled(src, m):
    """the library's stderr line of a profiled truncated(m): (selection ms, count scan ms, emission ms)"""
    d = SparseMatrix()
    d.profile(True)
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            d.merge_topk(src, m, "set", 1)
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
    torch.cuda.empty_cache()

    makers = [("pruned_1", lambda: src.pruned(1))] + [("truncated_%d" % m, (lambda m=m: src.truncated(m))) for m in MS]
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
           "reps": a.reps, "sessions": a.sessions, "session_len": 8, "k": 10}
    for name, make in makers:
        res[name + "_ms_best"] = min(t[name])
        res[name + "_ms_all"] = [round(u, 2) for u in t[name]]
        c = make()
        res[name + "_pairs"] = int(c.export_dev("table")[2].shape[0])
        res[name + "_mem"] = int(c.mem)
        c.cf_recommend_batch(sessions, 10)
        res[name + "_recommend_ms_best"] = min(wall(lambda: c.cf_recommend_batch(sessions, 10)) for _ in range(3))
        c.close()
        torch.cuda.empty_cache()
    for m in MS:
        sel, scan, emit = profiled(src, m)
        res["truncated_%d_selection_ms" % m], res["truncated_%d_count_scan_ms" % m], res["truncated_%d_emit_ms" % m] = sel, scan, emit
        res["truncated_%d_over_pruned_1" % m] = res["truncated_%d_ms_best" % m] / res["pruned_1_ms_best"]
    print(json.dumps(res), flush=True)
    src.close()


if __name__ == "__main__":
    main()
