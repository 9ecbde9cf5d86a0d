#!/usr/bin/env python3
"""smatrix_merge_scaled against the composition the public API offers without it, same process, one GPU.

  python3 tools/probe/merge_scaled_time.py [--ops 4e8] [--reps 5] [--num 1] [--den 2] [--min-value 1]

src = the table of bench.py's config 2: the first `ops` ops of its Zipf stream, in batches of 2^24 incr (4e8: 1 M rows /
100 M pairs).  Timed, each after one warm-up, `reps` times, the two sides alternated rep by rep, every rep on a fresh
destination:
  (a) dst.merge_scaled(src, "incr", num, den, min_value) into an empty dst      (b) the same into a dst that holds the surviving keys
  (c) the composition: src.export_dev("table"), torch: v' = v * num // den in int64, the mask of the two drop rules,
      repeat_interleave of the row ids, the three masked selections, dst.apply_batch_dev(INCR, no results) in slices of 2^24 ops
      -- into an empty dst and into one that holds the keys
Times are wall time around the whole call with the device idle before and synchronised after (merge_scaled runs on the matrix's
own stream and returns when it has finished).  Extra device memory: for the composition torch.cuda.max_memory_allocated of its
tensors; for merge_scaled the largest drop of hipMemGetInfo's free memory during the call, sampled every millisecond by a
thread, less what the destination's arena grew by.  The kernels alone: one more call with smatrix_profile on, the library's own
HIP-event lines (the filtered count on the matrix's stream; the emission on the helper stream, beside the write path), over the
bytes of src's row tables.  Prints one JSON line."""
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
from tools.probe.merge_time import B, FreeWatch, wall  # noqa: E402


def composition(src, dst, num, den, min_value):
    stream = torch.cuda.current_stream().cuda_stream
    rows, ptr, pairs = src.export_dev("table")
    w = (pairs[:, 1].to(torch.int64) & 0xFFFFFFFF) * num // den          # (v * num < 2^63 for the fractions probed here)
    keep = (w >= min_value) & ((pairs[:, 0] != 0) | (w != 0))
    x = torch.repeat_interleave(rows, ptr[1:] - ptr[:-1])[keep]
    y = pairs[:, 0][keep].contiguous()
    v = w[keep].to(torch.int32)
    n = x.numel()
    for a in range(0, n, B):
        k = min(B, n - a)
        dst.apply_batch_dev(OP_INCR, k, x.data_ptr() + 4 * a, y.data_ptr() + 4 * a, v.data_ptr() + 4 * a, None, stream)
    return n


def extra_bytes(fn, dst):
    torch.cuda.synchronize()
    mapped0, free0 = dst.stats()["arena_mapped"], torch.cuda.mem_get_info(0)[0]
    w = FreeWatch(); w.start()
    fn()
    w.stop = True; w.join()
    return max(0, free0 - w.low - (dst.stats()["arena_mapped"] - mapped0))


def kernel_ms(fn, dst):
    """the library's stderr lines of a profiled call: (filtered count ms, record emission ms)"""
    dst.profile(True)
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    dst.profile(False)
    c, e = re.search(r"filtered count ([0-9.]+) ms", text), re.search(r"record emission ([0-9.]+) ms", text)
    return (float(c.group(1)) if c else None), (float(e.group(1)) if e else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=float, default=4e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--num", type=int, default=1)
    ap.add_argument("--den", type=int, default=2)
    ap.add_argument("--min-value", type=int, default=1)
    a = ap.parse_args()
    num, den, mv = a.num, a.den, a.min_value
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

    counts = [0, 0]
    scaled = lambda d: d.merge_scaled(src, "incr", num, den, mv)

    def holding_the_keys():
        d = SparseMatrix()
        counts[0], counts[1] = scaled(d)
        return d

    t = {"scaled_empty": [], "scaled_same": [], "comp_empty": [], "comp_same": []}
    comp_ops = 0
    for rep in range(a.reps + 1):                      # rep 0 is the warm-up
        for name, fresh, fn in (("scaled_empty", SparseMatrix, scaled),
                                ("comp_empty", SparseMatrix, lambda d: composition(src, d, num, den, mv)),
                                ("scaled_same", holding_the_keys, scaled),
                                ("comp_same", holding_the_keys, lambda d: composition(src, d, num, den, mv))):
            d = fresh()
            out = []
            ms = wall(lambda: out.append(fn(d)))
            if name == "comp_empty":
                comp_ops = out[0]
            d.close()
            torch.cuda.empty_cache()
            if rep:
                t[name].append(ms)
    # memory
    d = holding_the_keys()
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    composition(src, d, num, den, mv)
    torch.cuda.synchronize()
    comp_extra = torch.cuda.max_memory_allocated() - base
    torch.cuda.empty_cache()
    scaled_extra = extra_bytes(lambda: scaled(d), d)
    c_ms, e_ms = kernel_ms(lambda: scaled(d), d)
    d.close()
    st = src.stats()
    table_bytes = (st["arena_units"] - st["arena_free_units"]) * 128
    res = {"ops_in_stream": nb * B, "fraction": [num, den], "min_value": mv, "src_rows": st["rows"], "src_pairs": counts[0] + counts[1],
           "applied": counts[0], "dropped": counts[1], "comp_applied": comp_ops, "src_table_bytes": table_bytes, "reps": a.reps}
    for k, v in t.items():
        res[k + "_ms_best"] = min(v)
        res[k + "_ms_all"] = [round(u, 2) for u in v]
    res["scaled_over_comp_empty"] = res["scaled_empty_ms_best"] / res["comp_empty_ms_best"]
    res["scaled_over_comp_same"] = res["scaled_same_ms_best"] / res["comp_same_ms_best"]
    res["comp_extra_bytes"] = comp_extra
    res["scaled_extra_bytes"] = scaled_extra
    res["count_ms"], res["emit_ms"] = c_ms, e_ms
    res["count_GBps_of_table_bytes"] = table_bytes / (c_ms * 1e-3) / 1e9 if c_ms else None
    res["emit_GBps_of_table_bytes"] = table_bytes / (e_ms * 1e-3) / 1e9 if e_ms else None
    print(json.dumps(res), flush=True)
    src.close()


if __name__ == "__main__":
    main()
