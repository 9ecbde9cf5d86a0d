#!/usr/bin/env python3
"""Whole-matrix export (smatrix_export_dev, TABLE and SORTED) against getrow_batch_dev over the same rows, same process.

  python3 tools/probe/export_time.py [config3_rows] [config2_batches]

config 3: the CF matrix of bench.py --config 3 (default 13 M rows x 115 ops); config 2: the first N batches of 2^24 ops of
bench.py's Zipf stream (default 24 = 4e8 ops).  Export times are wall time of the call (it reads the sizes back and returns
when the export has finished), best of 3; getrow is HIP events around getrow_batch_dev over the TABLE export's rows, with
the export's row_ptr as its offsets (exactly room enough), best of 3.  Prints one JSON line per matrix."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libsmatrix_amd import OP_INCR, SparseMatrix, Stream  # noqa: E402


def measure(m, dev, tag, reps=3):
    stream = torch.cuda.current_stream().cuda_stream
    res = {"matrix": tag}
    for order in ("table", "sorted"):
        best = 1e9
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.export_dev(order)
            best = min(best, time.perf_counter() - t0)
            if order == "table":
                rows, ptr, pairs = out
            del out
        res[order + "_ms"] = best * 1e3
    n, nnz = rows.numel(), pairs.shape[0]
    ret = torch.empty_like(pairs)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    best = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.getrow_batch_dev(n, rows.data_ptr(), ptr.data_ptr(), ret.data_ptr(), cnt.data_ptr(), stream)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    res.update({"rows": n, "nnz": nnz, "getrow_ms": best, "table_over_getrow": res["table_ms"] / best,
                "sorted_over_getrow": res["sorted_ms"] / best, "getrow_bytes_equal_table": bool(torch.equal(ret, pairs))})
    print(json.dumps(res), flush=True)
    del rows, ptr, pairs, ret, cnt
    torch.cuda.empty_cache()


def main():
    rows3 = int(sys.argv[1]) if len(sys.argv) > 1 else 13000000
    batches2 = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    if rows3:
        m = SparseMatrix()
        m.reserve(int(rows3 * 256 * 8 * 1.15) + (1 << 30))
        bench.build_cf(torch, dev, m, rows3)
        measure(m, dev, "config3 %d rows" % rows3)
        m.close()
    if batches2:
        m = SparseMatrix()
        stream = torch.cuda.current_stream().cuda_stream
        B = 1 << bench.BATCH_LG
        gen = Stream("zipf", bench.SEED, bench.N_IDS, bench.ZIPF_S, 1)
        x = torch.empty(B, dtype=torch.int32, device=dev); y = torch.empty_like(x); ones = torch.ones_like(x)
        for s in range(batches2):
            gen.fill_device(s * B, B, x.data_ptr(), y.data_ptr(), stream)
            m.apply_batch_dev(OP_INCR, B, x.data_ptr(), y.data_ptr(), ones.data_ptr(), None, stream)
        torch.cuda.synchronize()
        gen.close()
        measure(m, dev, "config2 %d ops" % (batches2 * B))
        m.close()


if __name__ == "__main__":
    main()
