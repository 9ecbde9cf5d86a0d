#!/usr/bin/env python3
"""The host flavours of the item-neighbour calls and of the session import, per call: smatrix_cf_neighbors_batch,
smatrix_cf_topk_batch (k = 10) and smatrix_cf_import_sessions at n = 1024 items or sessions, through ctypes on numpy arrays made once.

  python3 tools/probe/cf_host_calls_time.py [--calls 300] [--lib path/to/smatrix.so] [--out file]

The matrix: 4096 sessions of 8 distinct ids out of 1 .. 20000 (seed 7), imported once.  The items are 1024 ids of those sessions, the
neighbours' caps rowlen + 1; the import call's sessions are the first 1024 of the matrix's own, so from its second call on every op
hits a cell that exists.  After 20 warm-up calls of a kind, `calls` calls of it back to back, each timed on its own (a host flavour
returns with its results on the host): median, fastest, 10th and 90th percentile in microseconds.  --lib times another build's
library (the parent commit's) with this tree's Python.  Prints one JSON line and, with --out, appends it to that file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libsmatrix_amd import _lib  # noqa: E402

N, K, L, WARM = 1024, 10, 8, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from libsmatrix_amd import SparseMatrix
    p32, p64 = (lambda v: v.ctypes.data_as(_lib.u32p)), (lambda v: v.ctypes.data_as(_lib.u64p))
    pd = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rng = np.random.default_rng(7)
    sessions = [rng.choice(np.arange(1, 20001), size=L, replace=False).astype(np.uint32) for _ in range(4096)]
    m = SparseMatrix()
    m.cf_import_sessions(sessions)
    lib, h = m._lib, m._h
    items = np.ascontiguousarray(np.unique(np.concatenate(sessions))[:N])
    assert items.size == N
    off = np.zeros(N + 1, np.uint64)
    np.cumsum(m.rowlen_batch(items).astype(np.uint64) + 1, out=off[1:])
    total = int(off[-1])
    nb = np.zeros(total, np.uint32), np.zeros(total, np.float64), np.zeros(N, np.uint32)
    tk = np.zeros(N * K, np.uint32), np.zeros(N * K, np.float64), np.zeros(N, np.uint32)
    s_off = np.arange(0, N + 1, dtype=np.uint64) * L
    s_ids = np.ascontiguousarray(np.concatenate(sessions[:N]))
    kinds = (
        ("neighbors", lambda: lib.smatrix_cf_neighbors_batch(h, N, p32(items), p64(off), p32(nb[0]), pd(nb[1]), p32(nb[2]))),
        ("topk", lambda: lib.smatrix_cf_topk_batch(h, N, p32(items), K, p32(tk[0]), pd(tk[1]), p32(tk[2]))),
        ("import", lambda: lib.smatrix_cf_import_sessions(h, N, p64(s_off), p32(s_ids))),
    )
    res = {"label": a.label, "n": N, "k": K, "session_len": L, "calls": a.calls, "neighbours_out": total}
    for name, call in kinds:
        t = []
        for i in range(WARM + a.calls):
            t0 = time.perf_counter()
            rc = call()
            t1 = time.perf_counter()
            assert rc == 0, (name, rc)
            if i >= WARM:
                t.append((t1 - t0) * 1e6)
        q = np.percentile(t, [50, 10, 90])
        res["%s_us" % name] = {"median": round(float(q[0]), 2), "min": round(min(t), 2), "p10": round(float(q[1]), 2), "p90": round(float(q[2]), 2)}
    res["checks"] = {"neighbours_found": int(nb[2].sum()), "topk_found": int(tk[2].sum()), "rows": int(m.stats()["rows"])}
    m.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
