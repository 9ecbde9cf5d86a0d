#!/usr/bin/env python3
"""smatrix_merge against the composition the public API offered before it, same process, one GPU.

  python3 tools/probe/merge_time.py [--ops 4e8] [--reps 5]

src = the table of bench.py's config 2: the first `ops` ops of its Zipf stream, in batches of 2^24 incr (4e8: 1 M rows /
100 M pairs).  Timed, each after one warm-up, best of `reps`, merge and composition alternated rep by rep, every rep on a fresh
destination:
  (a) dst.merge(src) into an empty dst              (b) the same into a dst that already holds src's keys
  (c) the composition: src.export_dev("table"), torch.repeat_interleave of the row ids, the pairs de-interleaved,
      dst.apply_batch_dev(INCR, no results) in slices of 2^24 ops -- into an empty dst and into one that holds the keys
Times are wall time around the whole call with the device idle before and synchronised after (merge runs on the matrix's own
stream and returns when it has finished; HIP events on another stream would not see it).  Extra device memory: for the
composition torch.cuda.max_memory_allocated of its tensors; for the merge the largest drop of hipMemGetInfo's free memory
during the call, sampled every millisecond by a thread, less what the destination's arena grew by.  The emit kernels alone:
one more merge with smatrix_profile on, the library's own HIP-event line, over the bytes of src's row tables.
Prints one JSON line."""
import argparse
import json
import os
import re
import sys
import tempfile
import threading
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libsmatrix_amd import OP_INCR, SparseMatrix, Stream  # noqa: E402

B = 1 << 24


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def composition(src, dst):
    stream = torch.cuda.current_stream().cuda_stream
    rows, ptr, pairs = src.export_dev("table")
    x = torch.repeat_interleave(rows, ptr[1:] - ptr[:-1])
    y, v = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    n = x.numel()
    for a in range(0, n, B):
        k = min(B, n - a)
        dst.apply_batch_dev(OP_INCR, k, x.data_ptr() + 4 * a, y.data_ptr() + 4 * a, v.data_ptr() + 4 * a, None, stream)


class FreeWatch(threading.Thread):
    """the smallest free device memory seen while it runs"""
    def __init__(self):
        super().__init__(daemon=True)
        self.stop = False
        self.low = torch.cuda.mem_get_info(0)[0]

    def run(self):
        while not self.stop:
            self.low = min(self.low, torch.cuda.mem_get_info(0)[0])
            time.sleep(0.001)


def merge_extra_bytes(src, dst):
    torch.cuda.synchronize()
    mapped0, free0 = dst.stats()["arena_mapped"], torch.cuda.mem_get_info(0)[0]
    w = FreeWatch(); w.start()
    dst.merge(src)
    w.stop = True; w.join()
    return max(0, free0 - w.low - (dst.stats()["arena_mapped"] - mapped0))


def emit_ms(src, dst):
    """the library's stderr line of a profiled merge"""
    dst.profile(True)
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            dst.merge(src)
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    dst.profile(False)
    m = re.search(r"record emission ([0-9.]+) ms", text)
    return float(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
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
    gen.close()
    del x, y, ones
    torch.cuda.empty_cache()

    n_ops = [0]

    def holding_the_keys():
        d = SparseMatrix()
        n_ops[0] = d.merge(src)
        return d

    t = {"merge_empty": [], "merge_same": [], "comp_empty": [], "comp_same": []}
    for rep in range(a.reps + 1):                      # rep 0 is the warm-up
        for name, fresh, fn in (("merge_empty", SparseMatrix, lambda d: d.merge(src)),
                                ("comp_empty", SparseMatrix, lambda d: composition(src, d)),
                                ("merge_same", holding_the_keys, lambda d: d.merge(src)),
                                ("comp_same", holding_the_keys, lambda d: composition(src, d))):
            d = fresh()
            ms = wall(lambda: fn(d))
            d.close()
            torch.cuda.empty_cache()
            if rep:
                t[name].append(ms)
    # memory
    d = holding_the_keys()
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    composition(src, d)
    torch.cuda.synchronize()
    comp_extra = torch.cuda.max_memory_allocated() - base
    torch.cuda.empty_cache()
    merge_extra = merge_extra_bytes(src, d)
    e_ms = emit_ms(src, d)
    d.close()
    st = src.stats()
    table_bytes = (st["arena_units"] - st["arena_free_units"]) * 128
    res = {"ops_in_stream": nb * B, "src_rows": st["rows"], "src_pairs": n_ops[0], "src_table_bytes": table_bytes, "reps": a.reps}
    for k, v in t.items():
        res[k + "_ms_best"] = min(v)
        res[k + "_ms_all"] = [round(u, 2) for u in v]
    res["merge_over_comp_empty"] = res["merge_empty_ms_best"] / res["comp_empty_ms_best"]
    res["merge_over_comp_same"] = res["merge_same_ms_best"] / res["comp_same_ms_best"]
    res["comp_extra_bytes"] = comp_extra
    res["merge_extra_bytes"] = merge_extra
    res["emit_ms"] = e_ms
    res["emit_GBps_of_table_bytes"] = table_bytes / (e_ms * 1e-3) / 1e9 if e_ms else None
    print(json.dumps(res), flush=True)
    src.close()


if __name__ == "__main__":
    main()
