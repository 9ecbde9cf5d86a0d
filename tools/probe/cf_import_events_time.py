#!/usr/bin/env python3
"""The event import (smatrix_cf_import_events_dev) next to what it is measured by, one process, _dev flavours, every import into a
fresh matrix (rows are created and grown on the way, as in bench.py's CF import leg), wall time around the call and a device
synchronisation, best of `reps` with the spread (worst - best) given.

  python3 tools/probe/cf_import_events_time.py [sessions_lg] [reps]

(a) old against new at the defaults: the sessions bench.py's CF import leg builds (2^20 of 12 ids, Zipf(1.1) over 1 M scrambled
    ids); cf_import_sessions_dev, cf_import_events_dev with default arguments, cf_import_sessions_dev again, alternated rep by rep.
    The yardstick is the old call in the same run, the margin the difference of its two timings.
(b) a windowed import: the same ids regrouped into sessions of 64, window 5, both directions and FORWARD; and apply_batch_dev(INCR)
    on the very same ops expanded beforehand (torch, on the device), in batches of 2^25 as the import applies them: the generator's
    and the compaction's share is the difference of the two.
(c) forget: the DECR of (b), both directions, on the matrix its INCR filled, next to that INCR.
Prints one JSON line per part."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libsmatrix_amd import IMPORT_FORWARD, OP_DECR, OP_INCR, SparseMatrix, Stream  # noqa: E402

CHUNK = 1 << 25


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fresh(fns, reps):
    """each of fns(m) on a fresh matrix, alternated rep by rep -> per fn (best ms, spread ms, the last result)"""
    times, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(reps):
        for i, fn in enumerate(fns):
            m = SparseMatrix()
            t, outs[i] = wall(lambda: fn(m))
            times[i].append(t)
            m.close()
    return [(min(t), max(t) - min(t), o) for t, o in zip(times, outs)]


def expand(ids, L, window, forward):
    """the ops of sessions of L ids each, every amount 1, window >= 1: (x, y) int32 on the device, position-major"""
    n = ids.numel() // L
    p = torch.arange(L, device=ids.device)
    d = torch.arange(0 if forward else -window, window + 1, device=ids.device)
    q = p[:, None] + d[None, :]
    ok = ((q >= 0) & (q < L)).flatten()
    pp, qq = p[:, None].expand_as(q).flatten()[ok], q.flatten()[ok]
    s = ids.view(n, L)
    x, y = s[:, pp], s[:, qq].clone()
    y[:, pp == qq] = 0
    return x.reshape(-1).contiguous(), y.reshape(-1).contiguous()


def main():
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    n, L = 1 << lg, 12
    gen = Stream("zipf", bench.SEED + 7, bench.N_IDS, bench.ZIPF_S, 1)
    ids = torch.empty(n * L, dtype=torch.int32, device=dev); scratch = torch.empty_like(ids)
    gen.fill_device(0, n * L, ids.data_ptr(), scratch.data_ptr(), stream)
    torch.cuda.synchronize()
    gen.close()
    del scratch
    off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * L
    op_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * (L * L)
    bench.touch_hbm(torch, dev, 8 << 30)

    old = lambda m: m.cf_import_sessions_dev(n, off.data_ptr(), ids.data_ptr(), op_off.data_ptr(), n * L * L, stream)          # noqa: E731
    new = lambda m: m.cf_import_events_dev(OP_INCR, n, off.data_ptr(), ids.data_ptr(), None, 0, 0, stream=stream)               # noqa: E731
    fresh([old], 1)                                                                                                             # warm-up
    (o1, s1, _), (nw, sn, n_ops), (o2, s2, _) = fresh([old, new, old], reps)
    print(json.dumps({"part": "a", "sessions": n, "ids_per_session": L, "ops": n_ops, "old_ms": [o1, o2], "old_spread_ms": [s1, s2],
                      "new_ms": nw, "new_spread_ms": sn, "margin_ms": abs(o1 - o2), "new_minus_old_ms": nw - min(o1, o2),
                      "chunks": -(-n * L * L // CHUNK), "new_Gops_per_s": n_ops / nw / 1e6, "old_Gops_per_s": n_ops / min(o1, o2) / 1e6}), flush=True)

    L2, W = 64, 5
    n2 = ids.numel() // L2
    ids2 = ids[:n2 * L2]
    off2 = torch.arange(0, n2 + 1, dtype=torch.int64, device=dev) * L2
    for forward in (False, True):
        flags = IMPORT_FORWARD if forward else 0
        x, y = expand(ids2, L2, W, forward)
        ones = torch.ones(min(CHUNK, x.numel()), dtype=torch.int32, device=dev)

        def applied(m):
            for t0 in range(0, x.numel(), CHUNK):
                k = min(CHUNK, x.numel() - t0)
                m.apply_batch_dev(OP_INCR, k, x.data_ptr() + 4 * t0, y.data_ptr() + 4 * t0, ones.data_ptr(), None, stream)
            return x.numel()

        imp = lambda m: m.cf_import_events_dev(OP_INCR, n2, off2.data_ptr(), ids2.data_ptr(), None, W, flags, stream=stream)    # noqa: E731
        (ti, si, n_ops), (ta, sa, n_exp) = fresh([imp, applied], reps)
        assert n_ops == n_exp, (n_ops, n_exp)
        slots = n2 * L2 * ((W + 1) if forward else (2 * W + 1))
        print(json.dumps({"part": "b", "forward": forward, "sessions": n2, "ids_per_session": L2, "window": W, "ops": n_ops, "slots": slots,
                          "import_ms": ti, "import_spread_ms": si, "import_Gops_per_s": n_ops / ti / 1e6,
                          "apply_expanded_ms": ta, "apply_expanded_spread_ms": sa, "generator_and_compaction_ms": ti - ta}), flush=True)
        del x, y, ones

    # (c) the DECR next to its INCR, on one matrix per rep
    t_in, t_out = [], []
    for _ in range(reps):
        m = SparseMatrix()
        t, n_in = wall(lambda: m.cf_import_events_dev(OP_INCR, n2, off2.data_ptr(), ids2.data_ptr(), None, W, 0, stream=stream))
        t_in.append(t)
        t, n_out = wall(lambda: m.cf_import_events_dev(OP_DECR, n2, off2.data_ptr(), ids2.data_ptr(), None, W, 0, stream=stream))
        t_out.append(t)
        assert n_in == n_out
        m.close()
    print(json.dumps({"part": "c", "sessions": n2, "ids_per_session": L2, "window": W, "ops": n_in, "incr_ms": min(t_in),
                      "incr_spread_ms": max(t_in) - min(t_in), "decr_ms": min(t_out), "decr_spread_ms": max(t_out) - min(t_out),
                      "decr_Gops_per_s": n_out / min(t_out) / 1e6}), flush=True)


if __name__ == "__main__":
    main()
