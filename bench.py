#!/usr/bin/env python3
"""bench.py -- mixed incr+get throughput of the HIP path on BASELINE.json's config 2.

Workload (N=1): the 1M-row x 1M-col Zipf(1.1) stream with scrambled ids, seed 12345
(SURVEY.md 8d), cut into batches of 2^24 ops.  One STEP = one pass of the hot path
over one batch: smatrix_incr on the batch, then smatrix_get on the same keys (the
order of the reference benchmark: incr test, then get test,
src/smatrix_benchmark.c:226-230) = 2 * 2^24 ops.  Batches are generated on the GPU
before the timed region, so inputs are resident in HBM when timing starts.
warmup + steps = 24 batches cover the whole 4e8-op stream (100.4M nnz in 1M rows).

N>1 = BASELINE.json's config 4: the row-hash-sharded Zipf(1.1) stream over 8M x 8M scrambled ids
(SURVEY.md 8d), seed 12345 + rank, generated on the device.  `python bench.py --gpus N` launches
its own N ranks (child processes, spawned before this process touches any GPU) when it was not
started by torch.distributed.run; `--steps 75` at N=8 is the full 10^10-incr-op stream.
One process per GPU (torch.distributed, backend nccl = RCCL); every rank draws its
own slice of the stream, ops are routed to the row's owner shard with all_to_all
(libsmatrix_amd/sharded.py) and results routed back; the exchange of get(s) overlaps the
incr kernels of step s and the exchange of incr(s+1) overlaps get(s) (split-phase API on a
separate communication stream).  scaling = weak.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the steps and prints the line (`value`,
`ms_per_step`); `--full` adds the rest (kernel timers and roofline, cold start, table figures, the all-hits replay, the
extra legs, random-access ceilings, cpu_baseline).  `--dump-outputs DIR` writes what the last timed step returned.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BATCH_LG = 24
N_IDS = 1000000
N_IDS_CONFIG4 = 8000000   # config 4 (N > 1): 8M x 8M ids, SURVEY.md 8(d)
RING_MAX = 96             # pre-generated batches kept in HBM (12 GB of ids at 2^24 ops per batch)
ZIPF_S = 1.1
SEED = 12345
# algorithmic bytes per op, SURVEY.md 8(d): get = 8 in + 12 cell + 4 out; incr (with return) = 12 + 12 + 4 + 4
BYTES_GET, BYTES_INCR = 24, 32
HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8 TB/s


LINE_MAX = 4096           # the ONE stdout line stays below this (the driver scans a bounded window: r03's 20 KB line went unparsed)
DUMP_SAMPLE = 1 << 21     # --dump-outputs: positions of the last batch written per output (2 x 16 MB of float64)


def _r(v, sig=5):
    """floats to `sig` significant digits; containers recursively"""
    if isinstance(v, float):
        return float("%.*g" % (sig, v)) if v == v and abs(v) != float("inf") else None
    if isinstance(v, dict):
        return {k: _r(x, sig) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_r(x, sig) for x in v]
    return v


def _pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def short_line(full, detail_path=None):
    """The ONE stdout JSON line: the contract's keys, `roofline`, `cpu_baseline` and one-number summaries of the other
    legs -- the shape of the reference's own harness, one short line per measurement (src/smatrix_benchmark.c:134-138).
    Everything else (per-group arrays, notes, checksum replays, config-1 tables) lives in the detail file."""
    g = lambda d, *path: (g(d.get(path[0]), *path[1:]) if len(path) > 1 else d.get(path[0])) if isinstance(d, dict) else None
    line = _pick(full, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data")
    cfg = full.get("config", {})
    c = _pick(cfg, "ids_per_axis", "batch_ops", "parallelism", "router", "rccl")
    c["workload"] = cfg.get("workload_short") or cfg.get("workload", "")[:200]
    if isinstance(cfg.get("placement"), dict):
        c["placement"] = _pick(cfg["placement"], "rows_placed_by_load", "ops_applied_over_mean")
    line["config"] = c
    for k in ("roofline", "roofline_get"):
        if isinstance(full.get(k), dict):
            line[k] = _pick(full[k], "bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "memory_side_atomics",
                            "avg_launch_ms", "gops_per_s")
    cb = full.get("cpu_baseline")
    if isinstance(cb, dict):
        s = _pick(cb, "value", "unit", "cores", "kind")
        s["sample"] = str(cb.get("sample", ""))[:160]
        for k in ("threads_8", "threads_all_physical"):
            if isinstance(cb.get(k), dict):
                s[k] = _pick(cb[k], "value", "cores")
        s["host_cores"] = os.cpu_count()
        line["cpu_baseline"] = s
    ra = full.get("random_access")
    if isinstance(ra, dict):
        line["random_access"] = {"read8": ra.get("read8_gtouch_per_s"), "atomic_ret": ra.get("atomic_ret_gtouch_per_s"),
                                 "read8_32gib": g(ra, "table_sized_buffer_32gib", "read8_gtouch_per_s"),
                                 "unit": "Gtouch/s", "mixed_frac_of_read8": ra.get("mixed_frac_of_read8"),
                                 "mixed_frac_of_mixed_ceiling": ra.get("mixed_frac_of_mixed_ceiling"),
                                 "all_hits_frac_of_read8": ra.get("all_hits_frac_of_read8")}
    if isinstance(full.get("steady_state_all_hits"), dict):
        line["steady_state_all_hits"] = _pick(full["steady_state_all_hits"], "steps", "ms_per_step", "Mops_per_s")
    if isinstance(full.get("cold_start"), dict):
        line["cold_start"] = _pick(full["cold_start"], "first_step_ms", "over_timed_step")
    if isinstance(full.get("table"), dict):
        line["table"] = _pick(full["table"], "rows", "batches", "rounds", "rows_grown", "spec_chains", "spec_refused")
    if "sanity_all_gets_positive" in full:
        line["sanity_all_gets_positive"] = full["sanity_all_gets_positive"]
    summ = {"sustained_ms_per_step_median_group": g(full, "sustained", "ms_per_step_median_group"),
            "matches_reference_checksums": g(full, "reference_checksums", "matches_reference"),
            "dense_ids_Mops_per_s": g(full, "dense_ids", "Mops_per_s"),
            "dense_ids_first_step_ms": g(full, "dense_ids", "first_step_ms"),
            # (the incr call of the first step / of a mean late step: wall, waiting for the device, device allocations, the rest)
            "dense_ids_first_step_split": g(full, "dense_ids", "first_step_incr_split"),
            "dense_ids_mean_step_split": g(full, "dense_ids", "mean_step_incr_split"),
            "dense_ids_matches_reference": g(full, "dense_ids", "matches_reference"),
            "roofline_dense": _pick(g(full, "dense_ids", "roofline_dense") or {}, "kernel", "avg_launch_ms", "traffic", "r04_fetch_bytes", "achieved", "frac"),
            "op_kinds_Gops_per_s": g(full, "op_kinds", "Gops_per_s"),
            "host_api_Gops": {"incr": g(full, "host_api", "incr_Gops_per_s"), "get": g(full, "host_api", "get_Gops_per_s")},
            "config3": {"getrow_ms": g(full, "config3_getrow", "getrow_ms"), "frac": g(full, "config3_getrow", "roofline", "frac"),
                        "traffic": g(full, "config3_getrow", "roofline", "traffic"),
                        "verified": g(full, "config3_getrow", "verified_sum_of_values_eq_ops")},
            "config5": _pick(full.get("config5_file_1gpu") or {}, "close_s", "open_s", "verified", "file_bytes")}
    for k, v in list(summ.items()):
        if v is None or v == {} or (isinstance(v, dict) and all(x is None for x in v.values())):
            del summ[k]
    for k in ("sustained", "dense_ids", "op_kinds", "host_api", "config3_getrow", "config5_file_1gpu", "reference_checksums"):
        if isinstance(full.get(k), dict) and "error" in full[k]:
            summ[k + "_error"] = str(full[k]["error"])[:120]
    if summ:
        line["legs"] = summ
    if detail_path:
        line["detail"] = detail_path
    line = _r(line)
    text = json.dumps(line, separators=(",", ":"))
    # never let an unexpected field push the line out of the driver's window: shed the optional parts, largest first
    for k in ("legs", "table", "steady_state_all_hits", "cold_start", "roofline_get", "random_access"):
        if len(text) < LINE_MAX:
            break
        line.pop(k, None)
        text = json.dumps(line, separators=(",", ":"))
    assert len(text) < LINE_MAX, len(text)
    return text


def emit(full, json_out, name="bench_detail.json"):
    """full result -> detail file (repo root, and gpurun_out/ when present) + stderr; short line -> stdout"""
    rel = None
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        try:
            if os.path.isdir(d):
                with open(os.path.join(d, name), "w") as f:
                    json.dump(full, f, indent=1, default=str)
                rel = rel or name
        except OSError:
            pass
    print("bench detail: " + json.dumps(full, default=str), file=sys.stderr, flush=True)
    print(short_line(full, rel), file=json_out, flush=True)


def dump_outputs(torch, d, x, y, out_i, out_g):
    """--dump-outputs: what the last timed step returned (incr batch, then get batch on the same keys), at a fixed seeded
    sample of positions, as float64 (exact for uint32).  The get values are final values and do not depend on the order
    the ops were applied in.  For a key that occurs k times in one incr batch, the batch contract (include/smatrix_batch.h)
    fixes its k returns as a set but not which position gets which, so incr_returns holds them in canonical form: the
    returns of each key in ascending order over its positions in index order."""
    import numpy as np
    u = lambda t: t.to(torch.int64) & 0xFFFFFFFF
    key = (u(x) << 32) | u(y)
    ret = u(out_i)
    by_pos = torch.sort(key, stable=True).indices                  # grouped by key, index order inside a key
    q = torch.sort(ret, stable=True).indices
    by_ret = q[torch.sort(key[q], stable=True).indices]             # grouped by key, ascending return inside a key
    canon = torch.empty_like(ret)
    canon[by_pos] = ret[by_ret]
    n = key.numel()
    idx = np.sort(np.random.default_rng(SEED).choice(n, min(n, DUMP_SAMPLE), replace=False))
    at = torch.from_numpy(idx).to(key.device)
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "incr_returns.npy"), canon[at].cpu().numpy().astype(np.float64))
    np.save(os.path.join(d, "get_values.npy"), u(out_g)[at].cpu().numpy().astype(np.float64))


def cpu_baseline(sample_ops, torch, dev):
    """The reference's CPU path timed on this host, one thread, on the first `sample_ops` ops of the
    same stream (generated on the GPU, copied to the host): incr batch then get batch, in chunks of
    2^24 like the GPU run.  Uses the real reference (oracle/_ref, kind 'reference') when the prebuilt
    library is present, else the port.  ~10-30 s of CPU work."""
    import numpy as np
    from libsmatrix_amd import Stream
    from oracle import oracle as O
    gen = Stream("zipf", SEED, N_IDS, ZIPF_S, 1)
    xd = torch.empty(sample_ops, dtype=torch.int32, device=dev)
    yd = torch.empty_like(xd)
    gen.fill_device(0, sample_ops, xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x, y = xd.cpu().numpy().view(np.uint32), yd.cpu().numpy().view(np.uint32)
    del xd, yd
    kind = "reference" if O.have_reference() else "port"
    m = O.Reference() if kind == "reference" else O.Oracle()
    chunk = 1 << 24
    t_incr = t_get = 0.0
    for a in range(0, sample_ops, chunk):
        xs, ys = x[a:a + chunk], y[a:a + chunk]
        ones = np.ones(xs.size, np.uint32)
        t0 = time.perf_counter()
        m.apply(O.OP_INCR, xs, ys, ones)
        t1 = time.perf_counter()
        m.apply(O.OP_GET, xs, ys)
        t2 = time.perf_counter()
        t_incr += t1 - t0
        t_get += t2 - t1
    rows = m.num_rows()
    m.close()
    res = {
        "value": round(2 * sample_ops / (t_incr + t_get) / 1e6, 3), "unit": "Mops/s", "cores": 1, "kind": kind,
        "sample": "first %d ops of the same stream, batches of 2^24, incr batch then get batch: incr %.2fs + get %.2fs, "
                  "1 thread, %d rows; host has %d cores" % (sample_ops, t_incr, t_get, rows, os.cpu_count()),
    }
    if kind == "reference":
        # the reference is thread-safe (per-row spin RW locks, src/smatrix.c:843-889): the same ops split in
        # contiguous slices over 8 threads, thread start inside the timed region as in smatrix_benchmark.c:109-122
        import threading
        T, n8 = 8, min(sample_ops, 1 << 25)
        m = O.Reference()
        t8 = 0.0
        for a in range(0, n8, chunk):
            xs, ys = x[a:a + chunk], y[a:a + chunk]
            ones = np.ones(xs.size, np.uint32)
            per = (xs.size + T - 1) // T
            for op in (O.OP_INCR, O.OP_GET):
                th = [threading.Thread(target=m.apply, args=(op, xs[i * per:(i + 1) * per], ys[i * per:(i + 1) * per],
                                                             ones[i * per:(i + 1) * per])) for i in range(T)]
                t0 = time.perf_counter()
                for t in th:
                    t.start()
                for t in th:
                    t.join()
                t8 += time.perf_counter() - t0
        m.close()
        res["threads_8"] = {"value": round(2 * n8 / t8 / 1e6, 3), "unit": "Mops/s", "cores": T,
                            "sample": "first %d ops, each batch split over 8 threads: %.2fs" % (n8, t8)}
        # T = all physical cores.  The reference's spin locks scale NEGATIVELY under Zipf (one global
        # reader count + per-row mutexes, src/smatrix.c:843-889), so the sample is kept small: 2^20 ops (round 3; 2^21 took
        # 18.5 s and pushed the whole CPU leg to 44 s)
        try:
            import psutil
            T = psutil.cpu_count(logical=False) or os.cpu_count()
        except Exception:
            T = os.cpu_count()
        nall = min(sample_ops, 1 << 20)
        m = O.Reference()
        xs, ys = x[:nall], y[:nall]
        ones = np.ones(nall, np.uint32)
        per = (nall + T - 1) // T
        tall = 0.0
        for op in (O.OP_INCR, O.OP_GET):
            th = [threading.Thread(target=m.apply, args=(op, xs[i * per:(i + 1) * per], ys[i * per:(i + 1) * per],
                                                         ones[i * per:(i + 1) * per])) for i in range(T)]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            tall += time.perf_counter() - t0
        m.close()
        res["threads_all_physical"] = {"value": round(2 * nall / tall / 1e6, 3), "unit": "Mops/s", "cores": T,
                                       "sample": "first %d ops split over %d threads (thread start inside the timed region, "
                                                 "src/smatrix_benchmark.c:109-122): %.2fs" % (nall, T, tall)}
    # BASELINE config 1 (CPU-only configuration): (a) the stock benchmark pattern, 1 036 288 incr then get, T = 1
    # (src/smatrix_benchmark.c:29-65); (b) 1 M uniform-random ops over 2^20 x 2^20 ids, incr batch then get batch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from smatrix_benchmark import pattern
    c1 = {}
    px, py = pattern(0, 1024)
    m = O.Reference() if kind == "reference" else O.Oracle()
    ones = np.ones(px.size, np.uint32)
    t0 = time.perf_counter(); m.apply(O.OP_INCR, px, py, ones); t1 = time.perf_counter(); m.apply(O.OP_GET, px, py); t2 = time.perf_counter()
    m.close()
    c1["stock_pattern_T1"] = {"ops": int(px.size), "incr_ms": (t1 - t0) * 1e3, "get_ms": (t2 - t1) * 1e3,
                              "incr_Mops": px.size / (t1 - t0) / 1e6, "get_Mops": px.size / (t2 - t1) / 1e6}
    ug = Stream("uniform", SEED, 1 << 20, 1.1, 0)
    ux, uy = ug.fill(0, 1000000)
    ug.close()
    m = O.Reference() if kind == "reference" else O.Oracle()
    ones = np.ones(ux.size, np.uint32)
    t0 = time.perf_counter(); m.apply(O.OP_INCR, ux, uy, ones); t1 = time.perf_counter(); want = m.apply(O.OP_GET, ux, uy); t2 = time.perf_counter()
    rows_u = m.num_rows()
    m.close()
    c1["uniform_1m_T1"] = {"ops": 1000000, "incr_Mops": 1.0 / (t1 - t0), "get_Mops": 1.0 / (t2 - t1), "rows": rows_u,
                           "sum_get": int(want.astype(np.uint64).sum())}
    # the same two workloads through the HIP library's host-pointer batch API (PCIe copies included), checked against the CPU
    from libsmatrix_amd import SparseMatrix
    g = SparseMatrix()
    ones = np.ones(ux.size, np.uint32)
    g.incr_batch(ux[:1000], uy[:1000] + (1 << 21), ones[:1000])                     # first-call set-up outside the timing
    t0 = time.perf_counter(); g.incr_batch(ux, uy, ones); t1 = time.perf_counter(); got = g.get_batch(ux, uy); t2 = time.perf_counter()
    g.close()
    c1["uniform_1m_hip_host_api"] = {"incr_Mops": 1.0 / (t1 - t0), "get_Mops": 1.0 / (t2 - t1), "equals_cpu": bool((got == want).all())}
    res["config1"] = c1
    return res


def random_access_roofline(torch, dev, gib=4, touches=1 << 27):
    """R_rand of this chip, measured now (not a datasheet number): pseudo-random
    8-byte touches over a table-sized buffer, one kernel per mode, torch events on the stream
    the probe kernel is launched on."""
    from libsmatrix_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(gib << 27, dtype=torch.int64, device=dev)       # gib GiB
    sink = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"buffer_gib": gib, "touches": touches}
    for mode, name in ((0, "read8"), (3, "chain2"), (1, "atomic_ret"), (2, "atomic_noret")):
        best = None
        for rep in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lib.smx_probe_random_dev(buf.data_ptr(), buf.numel() * 8, touches, mode, 99 + rep, sink.data_ptr(), stream)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        out[name + "_gtouch_per_s"] = touches / (best * 1e-3) / 1e9
    del buf
    return out


CF_COLS, CF_PER_ROW = 13000000, 115          # config 3 / 5 shape, SURVEY.md 8(d)
BYTES_NNZ, BYTES_ROW = 16, 24                # getrow: 8 B cell read + 8 B pair written per nnz; 4 B id + 16 B directory slot + 4 B count per row


def kernel_source_sha16():
    """identifies the kernels a PMC profile was taken with (profiles/*_pmc.json carries the same hash)"""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "libsmatrix_amd", "csrc")
    for f in ["smx_kernels.hpp"] + sorted(os.path.join("kernels", k) for k in os.listdir(os.path.join(csrc, "kernels")) if k.endswith(".hpp")) + ["smx_runtime.hip"]:
        h.update(open(os.path.join(csrc, f), "rb").read())
    return h.hexdigest()[:16]


def verify_config2(torch, dev, xs_ring, ys_ring, B, n_ring):
    """Parity inside the bench, against numbers the REFERENCE produced (compiled reference, 263 s on
    one CPU thread): a fresh matrix takes exactly the first 4e8 ops of the stream; after 10^7 ops the sum over the
    stream of get(x_i,y_i) must be 52 480 898 544 with 561 596 rows / 4 463 637 nnz, after 4e8 ops the matrix must
    hold exactly 1 000 000 rows, 100 401 767 nnz and a hottest row of 935 410 columns."""
    from libsmatrix_amd import SparseMatrix, Stream, OP_GET, OP_INCR
    stream = torch.cuda.current_stream().cuda_stream
    m = SparseMatrix()
    gen = Stream("zipf", SEED, N_IDS, ZIPF_S, 1)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    out = torch.empty(B, dtype=torch.int32, device=dev)
    xt = torch.empty(B, dtype=torch.int32, device=dev); yt = torch.empty_like(xt)

    def batch(s):
        if s < n_ring:
            return xs_ring[s], ys_ring[s]
        gen.fill_device(s * B, B, xt.data_ptr(), yt.data_ptr(), stream)
        return xt, yt

    def incr(x, y, a, b):
        if b > a:
            m.apply_batch_dev(OP_INCR, b - a, x[a:b].data_ptr(), y[a:b].data_ptr(), ones.data_ptr(), out.data_ptr(), stream)

    def census():
        ids = torch.arange(1, N_IDS + 1, dtype=torch.int64, device=dev)
        h = ids ^ (ids >> 16); h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h = h ^ (h >> 13); h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h = h ^ (h >> 16)                                                    # fmix32(rank): the scrambled row ids
        rows = torch.where(h >= 2 ** 31, h - 2 ** 32, h).to(torch.int32)
        lens = torch.empty(N_IDS, dtype=torch.int32, device=dev)
        m.rowlen_batch_dev(N_IDS, rows.data_ptr(), lens.data_ptr(), stream)
        torch.cuda.synchronize()
        return int(m.stats()["rows"]), int(lens.sum(dtype=torch.int64).item()), int(lens.max().item())

    res = {}
    P1, P2 = 10000000, 400000000
    assert P1 <= B
    pos = 0
    for s in range((P2 + B - 1) // B):
        x, y = batch(s)
        lo, hi = s * B, min(s * B + B, P2)
        for cut in [c for c in (P1,) if lo < c < hi] + [hi]:
            incr(x, y, pos - lo, cut - lo)
            pos = cut
            if cut == P1:                               # get over the first 10^7 ops of the stream (all inside batch 0)
                m.apply_batch_dev(OP_GET, P1, x.data_ptr(), y.data_ptr(), None, out.data_ptr(), stream)
                torch.cuda.synchronize()
                sum_get = int(out[:P1].sum(dtype=torch.int64).item())
                res["at_1e7_ops"] = dict(zip(("rows", "nnz", "max_rowlen"), census()), sum_get=sum_get)
    res["at_4e8_ops"] = dict(zip(("rows", "nnz", "max_rowlen"), census()))
    res["clustered_mode"] = int(m.stats()["clustered_mode"])      # (scrambled ids: must stay 0)
    res["getrow_all_rows_at_4e8"] = scan_config2(torch, dev, m, stream)
    m.close(); gen.close()
    want = {"at_1e7_ops": {"rows": 561596, "nnz": 4463637, "max_rowlen": 159472, "sum_get": 52480898544},
            "at_4e8_ops": {"rows": 1000000, "nnz": 100401767, "max_rowlen": 935410}}
    res["matches_reference"] = res["at_1e7_ops"] == want["at_1e7_ops"] and res["at_4e8_ops"] == want["at_4e8_ops"]
    g = res["getrow_all_rows_at_4e8"]
    # getrow over every row: as many pairs as nnz, the values sum to the number of incr ops (every op added 1, y >= 1),
    # and the hottest row -- 2 M slots, read by one workgroup per 32768-cell segment -- returns all its 935 410 pairs
    res["matches_reference"] = res["matches_reference"] and g["pairs"] == want["at_4e8_ops"]["nnz"] and g["sum_of_values"] == P2 \
        and g["max_row_pairs"] == want["at_4e8_ops"]["max_rowlen"]
    res["reference_figures"] = "SURVEY.md A.4 (compiled reference, this stream)"
    assert res["matches_reference"], (res, want)
    return res


def scan_config2(torch, dev, m, stream, reps=3):
    """smatrix_rowlen + smatrix_getrow over all 1 M rows of the config-2 table in one device call each (HIP events)"""
    ids = torch.arange(1, N_IDS + 1, dtype=torch.int64, device=dev)
    h = ids ^ (ids >> 16); h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h = h ^ (h >> 13); h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    rows = torch.where(h >= 2 ** 31, h - 2 ** 32, h).to(torch.int32)
    lens = torch.empty(N_IDS, dtype=torch.int32, device=dev)
    m.rowlen_batch_dev(N_IDS, rows.data_ptr(), lens.data_ptr(), stream)
    l64 = lens.to(torch.int64) & 0xFFFFFFFF
    off = torch.zeros(N_IDS + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(l64 + 1, 0)                                       # rowlen + 1 pairs of room per row (quirk Q5)
    total = int(off[-1].item())
    ret = torch.empty((total, 2), dtype=torch.int32, device=dev)
    cnt = torch.empty(N_IDS, dtype=torch.int32, device=dev)
    best = 1e9
    for _ in range(reps):
        ret.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.getrow_batch_dev(N_IDS, rows.data_ptr(), off.data_ptr(), ret.data_ptr(), cnt.data_ptr(), stream)
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    c64 = cnt.to(torch.int64) & 0xFFFFFFFF
    pairs = int(c64.sum().item())
    # rows are packed back to back only up to their count: everything past it inside a row's room stayed zero
    vals = (ret[:, 1].to(torch.int64) & 0xFFFFFFFF).sum().item()
    return {"rows": N_IDS, "pairs": pairs, "sum_of_values": int(vals), "max_row_pairs": int(c64.max().item()),
            "counts_equal_rowlen": bool((c64 == l64).all().item()), "getrow_ms": best, "Gnnz_per_s": pairs / best / 1e6}


def build_cf(torch, dev, m, rows, chunk_rows=1 << 17):
    """config 3 / 5 table: `rows` rows x 115 ops, uniform columns over 13 M, scrambled ids (SMX_DIST_CF), generated on the device"""
    from libsmatrix_amd import Stream, OP_INCR
    stream = torch.cuda.current_stream().cuda_stream
    gen = Stream("cf", SEED, CF_COLS, float(CF_PER_ROW), 1)
    n_max = chunk_rows * CF_PER_ROW
    x = torch.empty(n_max, dtype=torch.int32, device=dev); y = torch.empty_like(x)
    ones = torch.ones_like(x); out = torch.empty_like(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r0 in range(0, rows, chunk_rows):
        n = (min(rows, r0 + chunk_rows) - r0) * CF_PER_ROW
        gen.fill_device(r0 * CF_PER_ROW, n, x.data_ptr(), y.data_ptr(), stream)
        m.apply_batch_dev(OP_INCR, n, x.data_ptr(), y.data_ptr(), ones.data_ptr(), out.data_ptr(), stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gen.close()
    return dt


def cf_row_ids(torch, dev, rows, shuffle=True):
    ids = torch.arange(1, rows + 1, dtype=torch.int64, device=dev)
    h = ids ^ (ids >> 16); h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h = h ^ (h >> 13); h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    xs = torch.where(h >= 2 ** 31, h - 2 ** 32, h).to(torch.int32)
    if shuffle:                                        # scan order != creation order
        g = torch.Generator(device=dev); g.manual_seed(SEED)
        xs = xs[torch.randperm(rows, device=dev, generator=g)]
    return xs.contiguous()


def scan_cf(torch, dev, m, rows, reps=5):
    """rowlen_batch + getrow_batch over ALL rows (the reference's caller idiom: rowlen, buffer, getrow --
    src/smatrix_jni.c:130-139); HIP events on the stream the kernels are launched on"""
    stream = torch.cuda.current_stream().cuda_stream
    xs = cf_row_ids(torch, dev, rows)
    lens = torch.empty(rows, dtype=torch.int32, device=dev)
    best = None
    for rep in range(reps):
        e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        e0.record()
        m.rowlen_batch_dev(rows, xs.data_ptr(), lens.data_ptr(), stream)
        e1.record()
        if rep == 0:
            off = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
            torch.cumsum(lens.long() + 1, 0, out=off[1:])
            ret = torch.zeros((int(off[-1].item()), 2), dtype=torch.int32, device=dev)
            cnt = torch.empty(rows, dtype=torch.int32, device=dev)
        e2.record()
        m.getrow_batch_dev(rows, xs.data_ptr(), off.data_ptr(), ret.data_ptr(), cnt.data_ptr(), stream)
        e3.record()
        torch.cuda.synchronize()
        t = (e0.elapsed_time(e1), e2.elapsed_time(e3))
        if best is None or t[1] < best[1]:
            best = t
    nnz = int(cnt.sum(dtype=torch.int64).item())
    ok = bool((cnt == lens).all().item()) and int(ret[:, 1].sum(dtype=torch.int64).item()) == rows * CF_PER_ROW
    ksum = int(ret[:, 0].sum(dtype=torch.int64).item())
    st = m.stats()
    table_bytes = (int(st["arena_units"]) - int(st["arena_free_units"])) * 128
    alg = nnz * BYTES_NNZ + rows * BYTES_ROW
    sec = best[1] * 1e-3
    traffic = None
    try:                                   # committed PMC passes of `bench.py --config 3`, valid for these kernel sources only
        pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc.json")))
        if pmc.get("kernel_source_sha16") == kernel_source_sha16() and pmc["k_getrow"]["rows"] == rows:
            traffic = pmc["k_getrow"]["bytes_per_launch"]
    except Exception:
        pass
    return {"rows": rows, "nnz": nnz, "verified_sum_of_values_eq_ops": ok, "key_checksum": ksum,
            "rowlen_ms": best[0], "getrow_ms": best[1], "Gnnz_per_s": nnz / sec / 1e9, "Mrows_per_s": rows / sec / 1e6,
            "roofline": {"bound": "hbm", "kernel": "k_getrow", "achieved": alg / sec / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": alg / sec / 1e9 / HBM_PEAK_GBS, "traffic": traffic, "avg_launch_ms": best[1],
                         "bytes_per_nnz": BYTES_NNZ, "bytes_per_row": BYTES_ROW,
                         "bytes_moved_model": table_bytes + 8 * nnz + 24 * rows,
                         "moved_GBps_model": (table_bytes + 8 * nnz + 24 * rows) / sec / 1e9,
                         "note": "achieved = algorithmic 16 B/nnz + 24 B/row; the tables are <= 50 % full by the reference's growth "
                                 "rule (src/smatrix.c:346), so the kernel has to MOVE table bytes + 8 B/nnz: moved_GBps_model"}}


def cf_read_path(torch, dev, m, rows, reps=3):
    """The reference's documented use of a matrix of this shape (examples/cf_recommender.c:50-86): column 0 of every row holds
    the item's total; neighbors_for_item(a) = getrow(a) and, per neighbour b, get(b,0) and cc / (sqrt(total_a) sqrt(total_b)).
    Here: the totals are added (one incr(x, 0, 115) per row), then smatrix_cf_neighbors_batch_dev scores ALL items in one call."""
    from libsmatrix_amd import OP_INCR, OP_GET
    stream = torch.cuda.current_stream().cuda_stream
    xs = cf_row_ids(torch, dev, rows)
    zeros = torch.zeros(rows, dtype=torch.int32, device=dev)
    per = torch.full((rows,), CF_PER_ROW, dtype=torch.int32, device=dev)
    m.apply_batch_dev(OP_INCR, rows, xs.data_ptr(), zeros.data_ptr(), per.data_ptr(), None, stream)
    lens = torch.empty(rows, dtype=torch.int32, device=dev)
    m.rowlen_batch_dev(rows, xs.data_ptr(), lens.data_ptr(), stream)
    off = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens.long() + 2, 0, out=off[1:])              # the (0,total) cell is not in rowlen (quirk Q1): +1, and +1 spare
    total = int(off[-1].item())
    ids = torch.zeros(total, dtype=torch.int32, device=dev)
    scores = torch.zeros(total, dtype=torch.float64, device=dev)
    cnt = torch.empty(rows, dtype=torch.int32, device=dev)
    best = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.cf_neighbors_batch_dev(rows, xs.data_ptr(), off.data_ptr(), ids.data_ptr(), scores.data_ptr(), cnt.data_ptr(), stream)
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    nb = int(cnt.sum(dtype=torch.int64).item())
    # check a sample of items against the same arithmetic in torch (float64, IEEE sqrt / multiply / divide: exact)
    g = torch.Generator(device=dev); g.manual_seed(SEED + 1)
    pick = torch.randint(0, rows, (20000,), device=dev, generator=g)
    ok = True
    a0 = off[pick]; c = cnt[pick].long()
    idx = (a0.repeat_interleave(c) + (torch.arange(int(c.sum().item()), device=dev) - (torch.cumsum(c, 0) - c).repeat_interleave(c)))
    nb_ids = ids[idx].contiguous(); nb_sc = scores[idx]
    owner = xs[pick].repeat_interleave(c).contiguous()
    n_s = nb_ids.numel()
    cc = torch.empty(n_s, dtype=torch.int32, device=dev); tb = torch.empty_like(cc); ta = torch.empty_like(cc)
    z = torch.zeros(n_s, dtype=torch.int32, device=dev)
    m.apply_batch_dev(OP_GET, n_s, owner.data_ptr(), nb_ids.data_ptr(), None, cc.data_ptr(), stream)
    m.apply_batch_dev(OP_GET, n_s, nb_ids.data_ptr(), z.data_ptr(), None, tb.data_ptr(), stream)
    m.apply_batch_dev(OP_GET, n_s, owner.data_ptr(), z.data_ptr(), None, ta.data_ptr(), stream)
    torch.cuda.synchronize()
    u = lambda t: (t.long() & 0xFFFFFFFF).double()
    tbf = torch.where(tb == 0, torch.ones_like(tb), tb)
    den = torch.sqrt(u(ta)) * torch.sqrt(u(tbf)); num = u(cc)
    want = torch.where((den == 0) | (num > den), torch.zeros_like(den), num / den)
    ok = bool((want == nb_sc).all().item()) and nb == int(lens.sum(dtype=torch.int64).item()) + rows
    # the k best per item only (smatrix_cf_topk_batch_dev, k = 10): same candidates, 120 B out per item instead of ~1.4 KB
    K = 10
    tid = torch.zeros((rows, K), dtype=torch.int32, device=dev); tsc = torch.zeros((rows, K), dtype=torch.float64, device=dev)
    tcnt = torch.empty(rows, dtype=torch.int32, device=dev)
    best_k = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.cf_topk_batch_dev(rows, xs.data_ptr(), K, tid.data_ptr(), tsc.data_ptr(), tcnt.data_ptr(), stream)
        e1.record(); torch.cuda.synchronize()
        best_k = min(best_k, e0.elapsed_time(e1))
    # against the full lists of the sampled items: the K largest scores, in order
    seg = torch.arange(pick.numel(), device=dev).repeat_interleave(c)
    dense = torch.full((pick.numel(), int(c.max().item())), -1.0, dtype=torch.float64, device=dev)
    col = torch.arange(int(c.sum().item()), device=dev) - (torch.cumsum(c, 0) - c).repeat_interleave(c)
    dense[seg, col] = nb_sc
    want_k = torch.topk(dense, K, dim=1).values
    got_k = torch.where(torch.arange(K, device=dev)[None, :] < tcnt[pick].long()[:, None], tsc[pick], torch.full_like(want_k, -1.0))
    ok_k = bool((want_k == got_k).all().item()) and bool((tcnt.long() == torch.clamp(cnt.long(), max=K)).all().item())
    sec = best * 1e-3
    return {"items": rows, "neighbours": nb, "ms": best, "Gneighbours_per_s": nb / sec / 1e9, "Mitems_per_s": rows / sec / 1e6,
            "verified_sample_items": int(pick.numel()), "verified": ok,
            "top10": {"ms": best_k, "Mitems_per_s": rows / best_k / 1e3, "Gneighbours_scored_per_s": nb / best_k / 1e6, "verified": ok_k},
            "random_touches_per_neighbour": 2,
            "note": "per neighbour: its cell in the item's row (streamed), then get(b,0) = one directory slot + one cell at random; "
                    "12 B out (id + double).  The per-item totals were added first with %d incr(x,0,115) ops (y = 0: quirk path)" % rows}


def cf_write_path(torch, dev, sessions=1 << 20, L=12):
    """examples/cf_recommender.c:36-47 on the device: `sessions` sessions of L item ids (Zipf(1.1) over 1 M scrambled ids, the
    config-2 marginal) -> L*L incr ops each, generated and applied by smatrix_cf_import_sessions_dev"""
    from libsmatrix_amd import SparseMatrix, Stream, OP_GET
    stream = torch.cuda.current_stream().cuda_stream
    n_ids = sessions * L
    gen = Stream("zipf", SEED + 7, N_IDS, ZIPF_S, 1)
    ids = torch.empty(n_ids, dtype=torch.int32, device=dev); scratch = torch.empty_like(ids)
    gen.fill_device(0, n_ids, ids.data_ptr(), scratch.data_ptr(), stream)
    off = torch.arange(0, sessions + 1, dtype=torch.int64, device=dev) * L
    op_off = torch.arange(0, sessions + 1, dtype=torch.int64, device=dev) * (L * L)
    total = sessions * L * L
    m = SparseMatrix()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.cf_import_sessions_dev(sessions, off.data_ptr(), ids.data_ptr(), op_off.data_ptr(), total, stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # every position of every session added 1 to its item's total in column 0
    items = torch.unique(ids)
    z = torch.zeros_like(items); tot = torch.empty_like(items)
    m.apply_batch_dev(OP_GET, items.numel(), items.data_ptr(), z.data_ptr(), None, tot.data_ptr(), stream)
    torch.cuda.synchronize()
    st = m.stats()
    ok = int((tot.long() & 0xFFFFFFFF).sum().item()) == n_ids and int(st["rows"]) == items.numel()
    m.close(); gen.close()
    return {"sessions": sessions, "ids_per_session": L, "incr_ops": total, "seconds": dt, "Gops_per_s": total / dt / 1e9,
            "items": int(items.numel()), "verified_totals": ok,
            "note": "first import into an empty matrix (rows are created and grown on the way)"}


def touch_hbm(torch, dev, nbytes):
    """First use of fresh HBM on a newly booted box is slow (the first 27 GB build of a process on a fresh box took 1.2 s,
    every later one 0.24 s -- driver-side first-touch work, not kernels): touch the amount once, outside any timing."""
    try:
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        t.zero_()
        torch.cuda.synchronize()
        del t
        torch.cuda.empty_cache()
    except Exception:                                          # noqa: BLE001
        pass


def run_config3(torch, dev, rows=13000000, reps=5):
    from libsmatrix_amd import SparseMatrix
    touch_hbm(torch, dev, rows * 256 * 8 * 1.6)
    # built twice: the first 27 GB build of the first process on a freshly leased box has been seen at 1.2-1.6 s against
    # 0.24 s for every later one, same kernels and round counts (driver-side first use of that much HBM, which the
    # touch above does not always absorb) -- both are reported, `build_s` is the second
    # (round 3: the slow build was seen on the SECOND matrix as well -- 1.39 s against 0.25 s -- i.e. it is the arena's growth
    #  steps, calls into the driver that can block while freed memory is wiped, not the first use of the HBM.  Both builds
    #  now map their arena up front, like config 2: smatrix_reserve, outside the timed build.)
    arena_hint = int(rows * 256 * 8 * 1.15) + (1 << 30)
    m = SparseMatrix()
    m.reserve(arena_hint)
    build_first_s = build_cf(torch, dev, m, rows)
    m.close()
    m = SparseMatrix()
    m.reserve(arena_hint)
    build_s = build_cf(torch, dev, m, rows)
    res = scan_cf(torch, dev, m, rows, reps)
    res["build_s"] = build_s
    res["build_first_s"] = build_first_s
    res["build_Gops_per_s"] = rows * CF_PER_ROW / build_s / 1e9
    res["workload"] = "config-3: smatrix_rowlen + smatrix_getrow over all %d rows / %d nnz (CF shape), table built on the device" % (rows, res["nnz"])
    res["cf_read_path"] = guarded(cf_read_path, torch, dev, m, rows)
    m.close()
    res["cf_write_path"] = guarded(cf_write_path, torch, dev)
    return res


def run_config5(torch, dev, rows=None, path=None):
    """config 5 on ONE GPU: persist the config-3 matrix (smatrix_close), reopen (bulk load), verify, re-bench get/getrow"""
    import shutil, tempfile
    from libsmatrix_amd import SparseMatrix, Stream, OP_GET
    stream = torch.cuda.current_stream().cuda_stream
    d = os.path.dirname(path) if path else tempfile.gettempdir()
    free = shutil.disk_usage(d).free
    if rows is None:
        rows = 13000000 if free > 40e9 else max(int(free * 0.5 / 2100) // 100000 * 100000, 100000)
    path = path or os.path.join(d, "smx_bench_config5_%d.smx" % os.getpid())
    if os.path.exists(path):
        os.remove(path)
    touch_hbm(torch, dev, rows * 256 * 8 * 1.6)
    # the background flusher (SMATRIX_FLUSH_MS, default 100 ms) would write most rows while the table is still being built
    # and scanned; it is switched off here so that close_s is the cost of persisting the WHOLE matrix, as in rounds 1-2
    keep = os.environ.get("SMATRIX_FLUSH_MS")
    os.environ["SMATRIX_FLUSH_MS"] = "0"
    try:
        m = SparseMatrix(path)
    finally:
        if keep is None:
            os.environ.pop("SMATRIX_FLUSH_MS", None)
        else:
            os.environ["SMATRIX_FLUSH_MS"] = keep
    m.reserve(int(rows * 256 * 8 * 1.15) + (1 << 30))         # (like run_config3: no arena growth steps inside the build)
    build_cf(torch, dev, m, rows)
    before = scan_cf(torch, dev, m, rows, 1)
    gen = Stream("cf", SEED, CF_COLS, float(CF_PER_ROW), 1)
    n = 1 << 24
    x = torch.empty(n, dtype=torch.int32, device=dev); y = torch.empty_like(x)
    want = torch.empty_like(x); got = torch.empty_like(x)
    gen.fill_device((rows // 2) * CF_PER_ROW, n, x.data_ptr(), y.data_ptr(), stream)
    m.apply_batch_dev(OP_GET, n, x.data_ptr(), y.data_ptr(), None, want.data_ptr(), stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); m.close(); t_close = time.perf_counter() - t0
    fbytes = os.path.getsize(path)
    t0 = time.perf_counter(); m = SparseMatrix(path); t_open = time.perf_counter() - t0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    m.apply_batch_dev(OP_GET, n, x.data_ptr(), y.data_ptr(), None, got.data_ptr(), stream)
    e1.record(); torch.cuda.synchronize()
    after = scan_cf(torch, dev, m, rows, 3)
    ok = bool(torch.equal(got, want)) and all(after[k] == before[k] for k in ("rows", "nnz", "key_checksum")) \
        and after["verified_sum_of_values_eq_ops"] and int(m.stats()["rows"]) == rows
    res = {"workload": "config-5 on one GPU: %d-row CF matrix persisted in the reference's file format, reopened, verified" % rows,
           "rows": rows, "nnz": after["nnz"], "file_bytes": fbytes, "close_s": t_close, "write_GBps": fbytes / t_close / 1e9,
           "open_s": t_open, "load_GBps": fbytes / t_open / 1e9, "verified": ok,
           "get_after_reopen_Gops": n / (e0.elapsed_time(e1) * 1e-3) / 1e9, "getrow_after_reopen": after,
           "scratch_free_bytes": free}
    gen.close()
    m.close()                       # nothing was written since the reload: close has nothing to persist
    try:
        os.remove(path)
    except OSError:
        pass
    return res



def guarded(fn, *a):
    """extra legs must never take the metric line down with them"""
    try:
        return fn(*a)
    except Exception as e:                                    # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, e)}


def op_kinds_leg(torch, dev, m, x, y, B, stream):
    """all four op kinds of the path on the finished config-2 table, one 2^24-op batch of present keys each (wall clock
    around the call, best of 3): get / incr / decr / set, write kinds also without a result array"""
    from libsmatrix_amd import OP_GET, OP_SET, OP_INCR, OP_DECR
    ones = torch.ones(B, dtype=torch.int32, device=dev); out = torch.empty_like(ones)

    def timed(op, v, o):
        best = 1e9
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            m.apply_batch_dev(op, B, x.data_ptr(), y.data_ptr(), v, o, stream)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best * 1e3
    r = {}
    for name, op in (("get", OP_GET), ("incr", OP_INCR), ("decr", OP_DECR)):
        r[name + "_ms"] = timed(op, ones.data_ptr(), out.data_ptr())
        if op != OP_GET:
            r[name + "_no_results_ms"] = timed(op, ones.data_ptr(), None)
    # set LAST, with the values the cells hold now (a get of the same keys): the table is left as it was
    m.apply_batch_dev(OP_GET, B, x.data_ptr(), y.data_ptr(), None, out.data_ptr(), stream)
    vals = out.clone(); o2 = torch.empty_like(out)
    r["set_ms"] = timed(OP_SET, vals.data_ptr(), o2.data_ptr())
    r["Gops_per_s"] = {k[:-3]: B / v / 1e6 for k, v in r.items() if k.endswith("_ms")}
    r["note"] = "present keys (no inserts); set resolves duplicates highest-index-wins (k_set_fold + the entry passes)"
    return r


def sustained_leg(torch, dev, m, gen, first_step, B, seconds, stream, group=16):
    """the SAME step on the continuing stream in back-to-back timed groups of `group` steps (inputs generated between
    the groups).  Per group: ms per step and what the table did meanwhile (rounds, rows grown, arena mapped) -- VERDICT r2
    asked where a 3.0 ms group comes from when the headline step is 2.4 ms."""
    from libsmatrix_amd import OP_GET, OP_INCR
    xs = torch.empty((group, B), dtype=torch.int32, device=dev); ys = torch.empty_like(xs)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    o1 = torch.empty(B, dtype=torch.int32, device=dev); o2 = torch.empty_like(o1)
    busy, steps, s = 0.0, 0, first_step
    groups = []
    keys = ("rounds", "rows_grown", "deferred_ops", "arena_mapped", "spec_chains", "spec_refused", "dir_grown")
    reserves = []
    while busy < seconds and steps < 4096:
        for k in range(group):
            gen.fill_device((s + k) * B, B, xs[k].data_ptr(), ys[k].data_ptr(), stream)
        st0 = m.stats()
        # capacity is managed BETWEEN the timed groups, the way a latency-sensitive caller would (smatrix_reserve, like
        # vector::reserve): an arena growth step inside a group maps GBs of fresh device memory, which costs from 2 ms to
        # 0.4 s depending on the box (round 3, profiles/r03_sustained_arena_growth.txt: groups of 9.8 / 13.5 / 19.2 / 26.7 ms
        # per step beside 2.1-2.2 -- VERDICT r2's unexplained 3.0 ms group)
        used_b, mapped_b = int(st0["arena_units"]) * 128, int(st0["arena_mapped"])
        if used_b > 0.6 * mapped_b:
            t_r = time.perf_counter()
            m.reserve(int(mapped_b * 1.6))
            torch.cuda.synchronize()
            reserves.append({"before_step": s, "mapped_bytes": int(mapped_b * 1.6), "seconds": round(time.perf_counter() - t_r, 4)})
            st0 = m.stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(group):
            m.apply_batch_dev(OP_INCR, B, xs[k].data_ptr(), ys[k].data_ptr(), ones.data_ptr(), o1.data_ptr(), stream)
            m.apply_batch_dev(OP_GET, B, xs[k].data_ptr(), ys[k].data_ptr(), None, o2.data_ptr(), stream)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st1 = m.stats()
        busy += dt
        groups.append(dict({k: int(st1[k]) - int(st0[k]) for k in keys}, first_step=s, ms_per_step=round(dt / group * 1e3, 4)))
        steps += group; s += group
    st = m.stats()
    per = sorted(g["ms_per_step"] for g in groups)
    return {"steps": steps, "timed_s": busy, "ms_per_step": busy / steps * 1e3, "Mops_per_s": 2 * B * steps / busy / 1e6,
            "ms_per_step_median_group": per[len(per) // 2], "ms_per_step_best_group": per[0], "ms_per_step_worst_group": per[-1],
            "groups": groups, "reserves_between_groups": reserves, "stream_ops_at_end": s * B, "rows": int(st["rows"]), "next_step": s,
            "note": "continues the config-2 stream past 4e8 ops in timed groups of %d steps (inputs generated between groups); a group in "
                    "which one of the giant rows doubles (rows_grown, rounds) carries that row's whole rehash" % group}


def batch_size_leg(torch, dev, lg, stream):
    """the config-2 stream in batches of 2^lg ops (batches of 2^24 - 2^26), fresh matrix, same 4e8-op stream:
    the per-batch fixed cost (the rounds after round 0: ~0.3 ms of small launches) is shared by four times the ops"""
    from libsmatrix_amd import SparseMatrix, Stream, OP_GET, OP_INCR
    B = 1 << lg
    nb = max((400000000 + B - 1) // B, 3)
    gen = Stream("zipf", SEED, N_IDS, ZIPF_S, 1)
    m = SparseMatrix()
    m.reserve(8 << 30)
    xs = torch.empty((nb, B), dtype=torch.int32, device=dev); ys = torch.empty_like(xs)
    for k in range(nb):
        gen.fill_device(k * B, B, xs[k].data_ptr(), ys[k].data_ptr(), stream)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    o1 = torch.empty(B, dtype=torch.int32, device=dev); o2 = torch.empty_like(o1)
    warm = 1
    for k in range(nb):
        if k == warm:
            torch.cuda.synchronize(); t0 = time.perf_counter()
        m.apply_batch_dev(OP_INCR, B, xs[k].data_ptr(), ys[k].data_ptr(), ones.data_ptr(), o1.data_ptr(), stream)
        m.apply_batch_dev(OP_GET, B, xs[k].data_ptr(), ys[k].data_ptr(), None, o2.data_ptr(), stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = m.stats()
    ok = bool((o2 >= 1).all().item()) and int(st["rows"]) <= N_IDS
    m.close(); gen.close()
    n = nb - warm
    return {"batch_lg": lg, "steps": n, "ms_per_step": dt / n * 1e3, "ms_per_2^24_ops_step": dt / n * 1e3 / (B >> 24),
            "Mops_per_s": 2 * B * n / dt / 1e6, "rounds": int(st["rounds"]), "sanity": ok,
            "note": "NOT `value` (that stays at 2^24-op batches, comparable across rounds): the same stream in %d batches of 2^%d ops" % (nb, lg)}


def rccl_library_in_use():
    """{path, version} of the RCCL the C router binds in this process (include/smatrix_shard.h smatrix_shard_rccl_library: the copy
    the process already holds -- torch's -- comes first, so that a torch process never ends up with two RCCLs on two HIP runtimes)"""
    import ctypes as C
    from libsmatrix_amd import _lib
    lib = _lib.load()
    lib.smatrix_shard_rccl_library.restype = C.c_char_p
    lib.smatrix_shard_rccl_library.argtypes = [C.POINTER(C.c_int)]
    v = C.c_int(0)
    p = lib.smatrix_shard_rccl_library(C.byref(v))
    return {"path": p.decode() if p else None, "version": v.value}


def host_api_leg(B, calls=5):
    """The host-pointer batch API -- what a JNI / Ruby batch binding calls with the caller's own arrays (the
    reference's glue passes host values, src/smatrix_jni.c:95-111): 2^24-op incr and get calls from numpy arrays on the
    config-2 stream, PCIe copies included (never `value`).  Calls of this size run as a three-stage pipeline over
    2^21-op chunks (csrc/smx_runtime.hip host_pipeline)."""
    import numpy as np
    from libsmatrix_amd import SparseMatrix, Stream
    gen = Stream("zipf", SEED, N_IDS, ZIPF_S, 1)
    m = SparseMatrix()
    ones = np.ones(B, np.uint32)
    r = np.zeros(B, np.uint32); g = np.zeros(B, np.uint32)       # the caller's own result arrays, reused (what a binding passes)
    ti, tg = [], []
    ok = True
    for k in range(calls + 1):
        x, y = gen.fill(k * B, B)
        t0 = time.perf_counter(); m.incr_batch(x, y, ones, out=r); t1 = time.perf_counter(); m.get_batch(x, y, out=g); t2 = time.perf_counter()
        ok = ok and bool((g >= r).all()) and bool((r >= 1).all())
        if k:                                                    # (call 0 creates the rows and the staging buffers)
            ti.append(t1 - t0); tg.append(t2 - t1)
    m.close(); gen.close()
    return {"ops_per_call": B, "calls": calls, "incr_Gops_per_s": B / (sum(ti) / len(ti)) / 1e9, "get_Gops_per_s": B / (sum(tg) / len(tg)) / 1e9,
            "incr_Gops_best_call": B / min(ti) / 1e9, "get_Gops_best_call": B / min(tg) / 1e9,
            "incr_ms": [t * 1e3 for t in ti], "get_ms": [t * 1e3 for t in tg], "sanity": ok,
            "note": "numpy arrays in pageable host memory; PCIe-inclusive, bounded by 16 B/op (incr) and 12 B/op (get) over the link"}


def dense_ids_leg(torch, dev, B, stream, steps=24):
    from libsmatrix_amd import SparseMatrix, Stream, OP_GET, OP_INCR
    gen = Stream("zipf", SEED, N_IDS, ZIPF_S, 0)
    m = SparseMatrix()
    m.reserve(8 << 30)                  # (the capacity hint of include/smatrix_batch.h: the row arena's first 8 GB are mapped before the clock starts)
    xs = torch.empty((steps, B), dtype=torch.int32, device=dev); ys = torch.empty_like(xs)
    for k in range(steps):
        gen.fill_device(k * B, B, xs[k].data_ptr(), ys[k].data_ptr(), stream)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    o1 = torch.empty(B, dtype=torch.int32, device=dev); o2 = torch.empty_like(o1)
    warm = 2
    m.profile(True)
    first_ms = None
    # where a write batch's wall time goes (smatrix_stats_t::write_*_ms, round 6): waiting for the device in the read-backs between
    # rounds (kernels running), device allocations / frees / maps, and the rest -- host work between launches
    split = lambda s: {"call_ms": s["last_write_call_ms"], "device_wait_ms": s["last_write_wait_ms"], "alloc_ms": s["last_write_alloc_ms"],
                       "host_ms": s["last_write_call_ms"] - s["last_write_wait_ms"] - s["last_write_alloc_ms"]}
    first_split = None
    for k in range(steps):
        if k == warm:
            m.profile(True)
            st_w = m.stats()
            torch.cuda.synchronize(); t0 = time.perf_counter()
        if k == 0:
            torch.cuda.synchronize(); tf = time.perf_counter()
        m.apply_batch_dev(OP_INCR, B, xs[k].data_ptr(), ys[k].data_ptr(), ones.data_ptr(), o1.data_ptr(), stream)
        m.apply_batch_dev(OP_GET, B, xs[k].data_ptr(), ys[k].data_ptr(), None, o2.data_ptr(), stream)
        if k == 0:
            torch.cuda.synchronize(); first_ms = (time.perf_counter() - tf) * 1e3      # (the cold start of a dense-id matrix: every row created, the keys of the hot rows in their best order)
            first_split = split(m.stats())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = m.stats()
    nn = max(steps - warm, 1)
    late_split = {"call_ms": (st["write_call_ms"] - st_w["write_call_ms"]) / nn, "device_wait_ms": (st["write_wait_ms"] - st_w["write_wait_ms"]) / nn,
                  "alloc_ms": (st["write_alloc_ms"] - st_w["write_alloc_ms"]) / nn}
    late_split["host_ms"] = late_split["call_ms"] - late_split["device_wait_ms"] - late_split["alloc_ms"]
    ok = bool((o2 >= 1).all().item()) and int(st["rows"]) <= N_IDS
    m.close()
    # Parity at full size, untimed: relabelling the ids does not change what the stream builds, so a second matrix fed exactly
    # 4e8 ops of the dense stream must hold the figures the reference's own run of the scrambled stream holds (reference_checksums:
    # 1 000 000 rows / 100 401 767 nnz / hottest row 935 410 columns) -- through the clustered path: far join, claimed inserts, the
    # in-LDS move of doubling rows.
    ref = {"rows": 1000000, "nnz": 100401767, "max_rowlen": 935410}
    got = None
    if steps * B >= 400000000:
        m2 = SparseMatrix()
        left = 400000000
        for k in range(steps):
            c = min(B, left)
            if c <= 0:
                break
            m2.apply_batch_dev(OP_INCR, c, xs[k].data_ptr(), ys[k].data_ptr(), ones.data_ptr(), o1.data_ptr(), stream)
            left -= c
        ids = torch.arange(1, N_IDS + 1, dtype=torch.int32, device=dev)
        lens = torch.empty(N_IDS, dtype=torch.int32, device=dev)
        m2.rowlen_batch_dev(N_IDS, ids.data_ptr(), lens.data_ptr(), stream)
        torch.cuda.synchronize()
        got = {"rows": int(m2.stats()["rows"]), "nnz": int(lens.sum(dtype=torch.int64).item()), "max_rowlen": int(lens.max().item()),
               "clustered_mode": int(m2.stats()["clustered_mode"])}
        m2.close()
        ok = ok and all(got[k] == ref[k] for k in ref)
    gen.close()
    n = steps - warm
    # the pass in front of prep (the dense stream's own kernel): time and HBM bytes per launch from the committed rocprofv3 passes of
    # this same stream (tools/refresh_dense_profile.sh), only while they were taken with the kernels that are running
    rd = None
    try:
        pd = json.load(open(os.path.join(ROOT, "profiles", "pmc_dense.json")))
        if pd.get("kernel_source_sha16") == kernel_source_sha16():
            rd = {"bound": "hbm", "kernel": pd["kernel"], "avg_launch_ms": pd["avg_launch_ms_last8"], "traffic": pd["fetch_bytes_per_launch"] + pd["write_bytes_per_launch"],
                  "fetch_bytes": pd["fetch_bytes_per_launch"], "r04_fetch_bytes": pd["r04_walking_pass_fetch_bytes_per_launch"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                  "achieved": (pd["fetch_bytes_per_launch"] + pd["write_bytes_per_launch"]) / max(pd["avg_launch_ms_last8"], 1e-9) / 1e6,
                  "source": pd["summary"]}
            rd["frac"] = rd["achieved"] / HBM_PEAK_GBS
    except Exception:
        rd = None
    return {"steps": n, "ms_per_step": dt / n * 1e3, "Mops_per_s": 2 * B * n / dt / 1e6, "first_step_ms": first_ms, "rows": int(st["rows"]), "roofline_dense": rd,
            "first_step_incr_split": first_split, "mean_step_incr_split": late_split,
            "incr_kernel_ms": st["kernel_ms_incr"] / max(st["kernel_launches_incr"], 1),
            "get_kernel_ms": st["kernel_ms_get"] / max(st["kernel_launches_get"], 1), "sanity": ok,
            "at_4e8_ops": got, "matches_reference": None if got is None else all(got[k] == ref[k] for k in ref),
            "note": "same stream with id = rank (dense): row tables use the reference's identity hash y % size, so hot columns cluster"}



def fail_rank(rank, why, code=3):
    """one line, then out -- never re-exec, never hang (os._exit: no atexit handler may wait for a peer that is gone)"""
    print("bench.py rank %d: %s" % (rank, why), file=sys.stderr, flush=True)
    os._exit(code)


class Watchdog:
    """a timer thread that ends THIS process with a one-line reason when `seconds` pass before cancel()"""

    def __init__(self, seconds, rank, what):
        import threading
        self._t = threading.Timer(seconds, fail_rank, args=(rank, "%s within %.0f s -- giving up" % (what, seconds), 4))
        self._t.daemon = True
        self._t.start()

    def cancel(self):
        self._t.cancel()


def preflight_router(torch, dev, m, stream):
    """the first collective calls of the C router on a matrix that stays empty: a get batch (reads of an empty matrix decide
    nothing about the placement) through the blocking call and through the split phases -- count exchange, grouped
    send/recv of records and results, gather"""
    from libsmatrix_amd import OP_GET
    n = 4096
    x = torch.arange(1, n + 1, dtype=torch.int32, device=dev) * 7919
    y = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    out = torch.full((n,), -1, dtype=torch.int32, device=dev)
    m.apply_dev(OP_GET, x, y, None, out, stream)
    torch.cuda.synchronize()
    if int(out.abs().sum().item()) != 0:
        raise RuntimeError("preflight: gets on an empty sharded matrix returned non-zero values")
    h = m.route(OP_GET, x, y, None, False, stream)
    m.apply_routed(h, False, stream)
    m.finish(h, out)
    m.wait(h, stream)
    torch.cuda.synchronize()
    if int(out.abs().sum().item()) != 0:
        raise RuntimeError("preflight: split-phase gets on an empty sharded matrix returned non-zero values")


def self_launch(n):
    """N ranks of this very command line as child processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their
    environment, rendezvous on 127.0.0.1); rank 0 inherits stdout (its ONE JSON line), the others' stdout goes to
    stderr.  Returns the worst exit code; if a rank dies the others are killed by PID."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else sys.stderr))
    worst = 0
    alive = set(range(n))
    while alive:
        for r in sorted(alive):
            rc = procs[r].poll()
            if rc is None:
                continue
            alive.discard(r)
            if rc != 0:
                worst = worst or rc
                for q in alive:
                    procs[q].kill()                        # (exact PIDs of our own children)
        time.sleep(0.05)
    return worst if worst >= 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=22)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch-lg", type=int, default=BATCH_LG)
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--cpu-sample-lg", type=int, default=26)
    ap.add_argument("--no-profile", action="store_true", help="do not time kernels with HIP events (A/B of the overhead)")
    ap.add_argument("--default-stream", action="store_true", help="N=1: issue the batches on the NULL stream (the library then waits for every call; A/B)")
    ap.add_argument("--no-overlap", action="store_true", help="sharded path: one blocking apply_dev per op batch")
    ap.add_argument("--no-comm-thread", action="store_true", help="sharded path: issue the exchange from the main thread")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo for test rigs)")
    ap.add_argument("--single-device", action="store_true",
                    help="test rig: every rank uses cuda:0 and the exchange is staged through the host (gloo)")
    ap.add_argument("--force-sharded", action="store_true",
                    help="route through ShardedMatrix even with one rank (exercises the exchange path)")
    ap.add_argument("--split-get", action="store_true",
                    help="sharded path: route the get batch on its own (two partitions and record exchanges per step, round 1's form)")
    ap.add_argument("--c-router", action="store_true",
                    help="(the default since round 4) sharded path through the C library's own router (include/smatrix_shard.h: RCCL "
                         "send/recv issued by the library, one partition + one record exchange per incr+get step)")
    ap.add_argument("--py-router", action="store_true",
                    help="sharded path through the torch.distributed router (libsmatrix_amd/sharded.py) instead of the C library's")
    ap.add_argument("--preflight-s", type=float, default=float(os.environ.get("SMATRIX_PREFLIGHT_S", "180")),
                    help="N > 1: seconds the first contact with the other ranks may take (process group, RCCL communicator, one "
                         "tiny routed batch) before this rank gives up with a one-line reason and a non-zero exit code")
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 5),
                    help="2 (default): the metric's workload; 3: getrow scan of the 13M-row CF matrix; 5: file round trip of it (one GPU)")
    ap.add_argument("--rows", type=int, default=None, help="--config 3/5: rows of the CF matrix (default 13M)")
    ap.add_argument("--no-extras", action="store_true",
                    help="config 2 only: skip the legs that are not `value` (reference-checksum replay, sustained run, dense ids, configs 3/5)")
    ap.add_argument("--no-reserve", action="store_true", help="do not map the row arena up front (A/B of smatrix_reserve)")
    ap.add_argument("--sustain-s", type=float, default=1.5, help="seconds of the sustained (continuing-stream) leg")
    ap.add_argument("--batch-leg", type=int, default=0, help="extra leg: the same stream in batches of 2^N ops (e.g. 26), not part of the default run")
    ap.add_argument("--full", action="store_true",
                    help="config 2 / 4: everything beyond the headline figure -- kernel timers and roofline, cold start, table figures, "
                         "the all-hits replay, the extra legs, random-access ceilings, cpu_baseline (a plain run only sets up, warms "
                         "up, times the steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="config 2 / 4: after the timed steps, write what the last timed step returned as DIR/<name>.npy (float64; "
                         "a fixed seeded sample of %d positions of the batch, rank 0's batch at N > 1)" % DUMP_SAMPLE)
    args = ap.parse_args()
    if args.dump_outputs and args.config != 2:
        ap.error("--dump-outputs applies to config 2 / 4 only")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as given: this process becomes a launcher.  It spawns N CHILD interpreters, one
        # rank each, BEFORE anything here has touched a GPU (torch is not even imported yet) and only relays rank 0's
        # JSON line and the exit codes -- it never execs, and never initialises HIP itself.
        sys.exit(self_launch(args.gpus))

    # ONE JSON line on stdout: everything else that libraries print there (RCCL's version banner at communicator
    # creation, for one) is sent to stderr for the whole run
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.single_device:
        local = 0
        os.environ["SMATRIX_SHARD_HOST_STAGED"] = "1"        # the Python router: payload staged through the host (gloo)
        os.environ["SMATRIX_SHARD_TRANSPORT"] = "shm"        # the C router: its shared-memory test transport
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if args.config in (3, 5):
        # the other single-GPU configurations of BASELINE.json, one JSON line each with their own roofline
        if args.config == 3:
            r = run_config3(torch, dev, args.rows or 13000000)
            line = {"metric": "getrow full-row scan", "value": r["Gnnz_per_s"] * 1e3, "unit": "Mnnz/s", "ms_per_step": r["getrow_ms"]}
        else:
            r = run_config5(torch, dev, args.rows)
            line = {"metric": "file-backed persist + reopen", "value": r["load_GBps"], "unit": "GB/s (bulk load)", "ms_per_step": r["open_s"] * 1e3}
        line.update({"n_gpus": 1, "steps": 1, "warmup": 0, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                     "dtype": "u32", "data": "synthetic", "config": {"workload": r["workload"]},
                     "roofline": r.get("roofline") or r["getrow_after_reopen"]["roofline"], "result": r})
        emit(line, json_out, "bench_detail_config%d.json" % args.config)
        return
    sharded = world > 1 or args.force_sharded
    # N > 1 goes through the C library's router (north_star: "host C calling HIP ... RCCL alltoallv") unless --py-router
    args.c_router = sharded and not args.py_router
    watchdog = None
    if sharded:
        import torch.distributed as dist
        if "MASTER_ADDR" not in os.environ:          # single process, --force-sharded
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29544", RANK="0", WORLD_SIZE="1")
        # First contact with the other ranks (rendezvous, RCCL communicator creation, the first grouped send/recv) is where a
        # multi-GPU run hangs if it hangs.  A rank that has not come through after --preflight-s seconds says why in ONE line
        # and leaves with a non-zero code -- it never re-execs and never waits for ever; a parent started as `bench.py --gpus N`
        # then ends the siblings (self_launch), torch.distributed.run does the same for its workers.
        watchdog = Watchdog(args.preflight_s, rank, "first contact with the other ranks (process group / RCCL communicator / first "
                                                     "routed batch) did not complete")
        try:
            if args.backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
            else:
                dist.init_process_group(args.backend)
        except Exception as e:                                  # noqa: BLE001
            fail_rank(rank, "process group (%s) could not be created: %s: %s" % (args.backend, type(e).__name__, e))

    from libsmatrix_amd import SparseMatrix, Stream, OP_GET, OP_INCR
    B = 1 << args.batch_lg
    total_steps = args.warmup + args.steps
    # N > 1 is config 4: 8M x 8M ids, every rank its own stream (seed 12345 + rank), generated on the device
    n_ids = N_IDS_CONFIG4 if world > 1 else N_IDS
    gen = Stream("zipf", SEED + (rank if world > 1 else 0), n_ids, ZIPF_S, 1)

    # inputs live in HBM before the timed region; beyond 32 batches (4 GB) the pre-generated batches are
    # reused cyclically (the stream then repeats: later passes over a batch are all hits)
    ring = min(total_steps, RING_MAX if world > 1 else 32)
    xs_all = torch.empty((ring, B), dtype=torch.int32, device=dev)
    ys_all = torch.empty((ring, B), dtype=torch.int32, device=dev)

    class _Ring:
        def __init__(self, t):
            self.t = t

        def __getitem__(self, s):
            return self.t[s % ring]
    xs, ys = _Ring(xs_all), _Ring(ys_all)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    out_i = torch.empty(B, dtype=torch.int32, device=dev)
    out_g = torch.empty(B, dtype=torch.int32, device=dev)
    if not sharded and not args.default_stream:
        # The batch calls are asynchronous on a caller's stream (include/smatrix_batch.h); on the NULL stream the library waits for
        # each call to finish, and the host's time between a get batch and the next incr batch (26 us of a 2.4 ms step on the
        # builder's boxes, more on slower hosts) is then idle time on the GPU.  The timed region is fenced with
        # torch.cuda.synchronize() either way.
        torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    stream = torch.cuda.current_stream().cuda_stream
    for s in range(ring):
        gen.fill_device(s * B, B, xs[s].data_ptr(), ys[s].data_ptr(), stream)
    torch.cuda.synchronize()

    router_note = None
    if sharded and args.c_router:
        from libsmatrix_amd.sharded import NativeShardedMatrix
        m, why = None, None

        def any_rank_failed(reason):
            # every rank must take the same router: agree on the worst outcome (one small all-reduce)
            flag = torch.tensor([0 if reason is None else 1], dtype=torch.int32, device=dev if args.backend == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            return bool(int(flag.item()))
        try:
            m = NativeShardedMatrix()                           # (RCCL loaded, the id travelled, ncclCommInitRank done)
        except Exception as e:                                  # noqa: BLE001
            why = "%s: %s" % (type(e).__name__, e)
        failed = any_rank_failed(why)                           # BEFORE the first collective of the router: a rank without a handle cannot take part in it
        if not failed:
            try:
                preflight_router(torch, dev, m, stream)
            except Exception as e:                              # noqa: BLE001
                why = "%s: %s" % (type(e).__name__, e)
            failed = any_rank_failed(why)
        if failed:
            # the library's own RCCL path is not usable here (RCCL missing, communicator refused): say so once and take the
            # torch.distributed router -- same partition kernels, same shards, the exchange issued by torch
            print("bench.py rank %d: C router unavailable (%s) -- falling back to the torch.distributed router" % (rank, why or "a peer failed"),
                  file=sys.stderr, flush=True)
            if m is not None:
                try:
                    m.close()
                except Exception:                                # noqa: BLE001
                    pass
            args.c_router = False
            router_note = "fallback from the C router: %s" % (why or "a peer failed")
    if sharded and not args.c_router:
        from libsmatrix_amd.sharded import ShardedMatrix
        try:
            m = ShardedMatrix()
        except Exception as e:                                  # noqa: BLE001
            fail_rank(rank, "torch.distributed router could not be created: %s: %s" % (type(e).__name__, e))
    elif not sharded:
        m = SparseMatrix()
    if watchdog:
        dist.barrier()
        watchdog.cancel()
    # capacity hint (smatrix_reserve, like vector::reserve): the row arena of this workload ends at ~3.1 GB (6 GB after the
    # sustained leg); mapped up front, no growth step -- a call into the driver, which can block for seconds while it still
    # has a previous process's freed memory to wipe -- falls into the timed region.  The tables themselves still grow
    # row by row inside it.
    ARENA_RESERVE = 8 << 30
    if args.no_reserve:
        ARENA_RESERVE = 0
    else:
        (m.local if sharded else m).reserve(ARENA_RESERVE)

    pending = {}       # sharded: batches whose incr records are already travelling (routed ahead)

    # Sharded + overlap: everything that talks to the other ranks (partition, the collectives, gather) runs on
    # ONE helper thread, in a fixed order, so that the host-side waits of the exchange (split sizes must reach
    # the host before a collective can be issued) run under the host-driven rounds of the op kernels instead of
    # in front of them.  The library calls release the GIL; the op kernels stay on the main thread.
    comm = None
    if sharded and not args.no_overlap and not args.no_comm_thread and not args.c_router:
        from concurrent.futures import ThreadPoolExecutor
        comm = ThreadPoolExecutor(max_workers=1, initializer=lambda: torch.cuda.set_device(local))

    READY = True       # the batches were generated before the timed region: route() need not wait for the compute stream
    lagging = []       # handles whose results the compute stream has not been told to wait for yet

    def step_fused(s):
        # ONE partition + ONE record exchange per step: the owner applies incr, then get on the records it holds
        # (ShardedMatrix.apply_routed_get); the records of step s+1 travel under the kernels of step s
        f_i = pending.pop(s, None) or comm.submit(m.route, OP_INCR, xs[s], ys[s], ones, READY)
        h = f_i.result()
        m.apply_routed(h)
        if s + 1 < total_steps and s + 1 != args.warmup:           # never across the timing fence
            pending[s + 1] = comm.submit(m.route, OP_INCR, xs[s + 1], ys[s + 1], ones, READY)
        m.apply_routed_get(h)
        comm.submit(m.finish, h, out_i, out_g).result()
        for hh in lagging:
            m.wait(hh)
        lagging[:] = [h]

    def step_threaded(s):
        if not args.split_get:
            return step_fused(s)
        f_i = pending.pop(s, None) or comm.submit(m.route, OP_INCR, xs[s], ys[s], ones, READY)
        f_g = comm.submit(m.route, OP_GET, xs[s], ys[s], None, READY)           # travels under the incr kernels of s
        h_i = f_i.result()
        m.apply_routed(h_i)
        f_fi = comm.submit(m.finish, h_i, out_i)
        h_g = f_g.result()
        m.apply_routed(h_g)
        if s + 1 < total_steps and s + 1 != args.warmup:           # never across the timing fence
            pending[s + 1] = comm.submit(m.route, OP_INCR, xs[s + 1], ys[s + 1], ones, READY)
        f_fg = comm.submit(m.finish, h_g, out_g)
        f_fi.result(); f_fg.result()
        # results are consumed after the timed region only: the compute stream is made to wait for the result
        # exchange of the PREVIOUS step (long finished), not of this one (same box: 3.93 -> 3.88 ms, one rank)
        for h in lagging:
            m.wait(h)
        lagging[:] = [h_i, h_g]

    def step_c_router(s):
        # the C library's router, split phases (include/smatrix_shard.h): the records of step s+1 are partitioned and
        # exchanged by the library's communication thread while this thread drives the op kernels of step s
        if args.no_overlap:
            return m.apply_then_get_dev(OP_INCR, xs[s], ys[s], ones, out_i, out_g, stream)
        h = pending.pop(s, None) or m.route(OP_INCR, xs[s], ys[s], ones, True, stream)
        if s + 1 < total_steps and s + 1 != args.warmup:           # never across the timing fence
            pending[s + 1] = m.route(OP_INCR, xs[s + 1], ys[s + 1], ones, True, stream)
        m.apply_routed(h, True, stream)
        m.finish(h, out_i, out_g)
        m.wait(h, stream)

    def step(s):
        if args.c_router and sharded:
            return step_c_router(s)
        if comm is not None:
            return step_threaded(s)
        if sharded and not args.no_overlap:
            # exchange of get(s) overlaps the incr kernels of s; exchange of incr(s+1) overlaps get(s)
            h_i = pending.pop(s, None) or m.route(OP_INCR, xs[s], ys[s], ones, READY)
            h_g = m.route(OP_GET, xs[s], ys[s], None, READY)
            m.apply_routed(h_i)                                   # host-driven rounds; get(s) records travel meanwhile
            m.finish(h_i, out_i)
            m.apply_routed(h_g)                                   # one async launch: runs while the host sits in the next route()
            if s + 1 < total_steps and s + 1 != args.warmup:      # never across the timing fence
                pending[s + 1] = m.route(OP_INCR, xs[s + 1], ys[s + 1], ones, READY)
            m.finish(h_g, out_g)
            m.wait(h_i); m.wait(h_g)
        elif sharded:
            m.apply_dev(OP_INCR, xs[s], ys[s], ones, out_i)
            m.apply_dev(OP_GET, xs[s], ys[s], None, out_g)
        else:
            m.apply_batch_dev(OP_INCR, B, xs[s].data_ptr(), ys[s].data_ptr(), ones.data_ptr(),
                              out_i.data_ptr(), stream)
            m.apply_batch_dev(OP_GET, B, xs[s].data_ptr(), ys[s].data_ptr(), None, out_g.data_ptr(), stream)

    def fence():
        for h in lagging:
            m.wait(h)
        del lagging[:]
        if sharded:
            dist.barrier()
        torch.cuda.synchronize()

    first_step_ms = None
    for s in range(args.warmup):
        if s == 0 and not sharded and args.full:
            # the cold start: step 0 creates the rows and doubles the hot ones up to 2^19 cells (untimed warmup; reported as an extra)
            torch.cuda.synchronize(); tc = time.perf_counter()
            step(s)
            torch.cuda.synchronize(); first_step_ms = (time.perf_counter() - tc) * 1e3
        else:
            step(s)
    local_m = m.local if sharded else m
    if args.full:
        local_m.profile(not args.no_profile)      # HIP events around the op kernels, on the stream they run on
    fence()
    t0 = time.perf_counter()
    for s in range(args.warmup, total_steps):
        step(s)
    fence()
    dt = time.perf_counter() - t0
    if args.full:
        st = local_m.stats()
        local_m.profile(False)
    if args.dump_outputs and rank == 0:
        dump_outputs(torch, args.dump_outputs, xs[total_steps - 1], ys[total_steps - 1], out_i, out_g)
    shard_info = None
    if sharded:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        # how evenly the placement spread the ops (ops each shard applied over the whole run / mean)
        loads = [None] * world
        dist.all_gather_object(loads, int(m.exchanged_ops))
        mean = max(sum(loads) / world, 1)
        shard_info = {"router": "C library (transport: %s; split phases on its communication thread; placement planned by the library)" % m.transport,
                      "rows_placed_by_load": len(m.placement.place),
                      "hash_range_widths": ([round((b - a) / 2.0 ** 32, 4) for a, b in zip([0] + m.placement.cuts, m.placement.cuts + [1 << 32])]
                                            if m.placement.cuts is not None else "equal"),
                      "ops_applied_over_mean": [round(v / mean, 3) for v in loads]} if args.c_router else {"rows_placed_by_load": len(m.placement.place),
                      "hash_range_widths": ([round((b - a) / 2.0 ** 32, 4) for a, b in
                                             zip([0] + m.placement.cuts, m.placement.cuts + [1 << 32])]
                                            if m.placement.cuts is not None else "equal"),
                      "ops_applied_over_mean": [round(v / mean, 3) for v in loads]}

    # informative extra (not `value`): the same step on the finished table -- every incr is a hit
    steady = None
    if not sharded and args.full:
        fence()
        t1 = time.perf_counter()
        for s in range(total_steps - 4, total_steps):
            step(s)
        fence()
        steady = {"steps": 4, "ms_per_step": (time.perf_counter() - t1) / 4 * 1e3,
                  "Mops_per_s": 2 * B * 4 / (time.perf_counter() - t1) / 1e6,
                  "note": "last 4 batches replayed on the 100.4M-nnz table: no inserts, no growth"}

    # parity spot-check inside the bench: the last get batch must equal the last incr returns' per-key max
    ok = bool((out_g >= 1).all().item()) if args.full else None

    extras = {}
    if not sharded and args.batch_leg:
        extras["batch_2_%d" % args.batch_leg] = guarded(batch_size_leg, torch, dev, args.batch_leg, stream)
    if not sharded and args.full and not args.no_extras and args.batch_lg == BATCH_LG:
        # (1) the reference-held checksums of this very stream, on a fresh matrix (outside the timed region)
        # (2) sustained leg: the SAME step on the continuing stream (fresh batches, table keeps growing) for >= 1 s of
        #     back-to-back steps, so that the run holds a timed region far longer than any sampling period -- once right
        #     behind the timed steps, once more after the checksum replay has opened, filled and closed a second matrix
        extras["sustained"] = guarded(sustained_leg, torch, dev, m, gen, total_steps, B, args.sustain_s, stream)
        extras["reference_checksums"] = verify_config2(torch, dev, xs_all, ys_all, B, ring)
        nxt = extras["sustained"].get("next_step", total_steps) if isinstance(extras["sustained"], dict) else total_steps
        extras["sustained_after_checksum_replay"] = guarded(sustained_leg, torch, dev, m, gen, nxt, B, 0.5, stream)
        # (3) dense ids (id = Zipf rank, no scramble): the reference's identity-hash tables cluster here
        #     (displacement 10^3-10^4); secondary metric
        extras["dense_ids"] = guarded(dense_ids_leg, torch, dev, B, stream)
        # (4) the four op kinds on the finished table
        extras["op_kinds"] = guarded(op_kinds_leg, torch, dev, m, xs[total_steps - 1], ys[total_steps - 1], B, stream)
        # (5) the host-pointer batch API (numpy arrays, PCIe included): never `value`
        extras["host_api"] = guarded(host_api_leg, B)

    total_ops = 2 * B * args.steps * world
    res = {
        "metric": "mixed incr+get ops/s", "value": total_ops / dt / 1e6, "unit": "Mops/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u32", "data": "synthetic",
        "config": {"workload": ("config-2: Zipf(1.1) x Zipf(1.1) over 1M x 1M scrambled ids, seed 12345, "
                                "batches of 2^%d ops, step = incr batch + get batch on the same keys; "
                                "table grows from %d to %d batches of the 4e8-op stream during the timed steps"
                                % (args.batch_lg, args.warmup, total_steps)) if world == 1 else
                               ("config-4: row-hash-sharded Zipf(1.1) x Zipf(1.1) stream over 8M x 8M scrambled ids, one stream per "
                                "rank (seed 12345 + rank) generated on the device, owner = planned hash ranges of the row id, "
                                "RCCL exchange over xGMI; step = every rank routes and applies an incr batch of 2^%d ops and a get "
                                "batch on the same keys; %d ranks x %d steps = %.3g incr ops (+ as many gets) in the timed "
                                "region (the full 10^10-op stream is --steps 75 at 8 ranks)"
                                % (args.batch_lg, world, args.steps, float(world) * args.steps * B)),
                   "workload_short": ("config-2: 1xMI355X, 100M-nnz / 1M-row Zipf(1.1) stream (scrambled ids, seed 12345), batched incr+get, "
                                      "2^%d ops per batch, step = incr batch + get batch" % args.batch_lg) if world == 1 else
                                     ("config-4: %dxMI355X, row-hash-sharded Zipf(1.1) incr(+get) stream over 8M x 8M ids, 2^%d ops per rank "
                                      "and step, exchange over RCCL/xGMI" % (world, args.batch_lg)),
                   "ids_per_axis": n_ids,
                   "batch_ops": B, "arena_reserved_bytes": ARENA_RESERVE, "distinct_batches": ring, "parallelism": "row-hash shards x%d" % world if sharded else "single GPU"},
    }
    if args.full:
        res["sanity_all_gets_positive"] = ok
    if sharded:
        res["config"]["router"] = ("c-library/%s" % m.transport) if args.c_router else "torch.distributed/%s" % args.backend
        res["config"]["rccl"] = rccl_library_in_use()            # which RCCL served the exchange: path and ncclGetVersion()
        if router_note:
            res["config"]["router_note"] = router_note
    if shard_info:
        res["config"]["placement"] = shard_info
    res.update(extras)
    if rank == 0 and args.full:
        ki = st["kernel_ms_incr"] / max(st["kernel_launches_incr"], 1)
        kg = st["kernel_ms_get"] / max(st["kernel_launches_get"], 1)
        # per-launch units: rank 0's local launches (N=1: exactly B ops per launch)
        ops_i = st["kernel_ops_incr"] / max(st["kernel_launches_incr"], 1)
        ops_g = st["kernel_ops_get"] / max(st["kernel_launches_get"], 1)
        ach_i = ops_i * BYTES_INCR / (ki * 1e-3) / 1e9 if ki else 0.0
        ach_g = ops_g * BYTES_GET / (kg * 1e-3) / 1e9 if kg else 0.0
        res["roofline"] = {"bound": "hbm", "kernel": "k_apply_agg<INCR> (round 0)", "achieved": ach_i,
                           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach_i / HBM_PEAK_GBS, "traffic": None,
                           "avg_launch_ms": ki, "ops_per_launch": ops_i, "bytes_per_op": BYTES_INCR,
                           "gops_per_s": ops_i / (ki * 1e-3) / 1e9 if ki else 0.0}
        res["roofline_get"] = {"bound": "hbm", "kernel": "k_apply<GET>", "achieved": ach_g, "peak": HBM_PEAK_GBS,
                               "unit": "GB/s", "frac": ach_g / HBM_PEAK_GBS, "traffic": None,
                               "avg_launch_ms": kg, "ops_per_launch": ops_g, "bytes_per_op": BYTES_GET,
                               "gops_per_s": ops_g / (kg * 1e-3) / 1e9 if kg else 0.0}
        # HBM-side bytes per launch: PMC counters cannot be read from inside the measured process, so they come from
        # the committed rocprofv3 --pmc passes of this same command -- but ONLY while that profile was taken with the
        # kernels that are running now (source hash); otherwise null, never a stale number next to fresh timings
        try:
            pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc.json")))
            if world == 1 and args.batch_lg == BATCH_LG and pmc.get("kernel_source_sha16") == kernel_source_sha16():
                res["roofline"]["traffic"] = pmc["k_apply_agg_incr"]["bytes_per_launch"]
                res["roofline_get"]["traffic"] = pmc["k_apply_get"]["bytes_per_launch"]
                res["roofline"]["memory_side_atomics"] = pmc["k_apply_agg_incr"].get("memory_side_atomics")
                res["roofline"]["traffic_source"] = res["roofline_get"]["traffic_source"] = pmc.get("summary", "profiles/")
            else:
                res["roofline"]["traffic_note"] = "profiles/pmc.json was taken with other kernel sources (%s): traffic left null" % pmc.get("kernel_source_sha16")
        except Exception:
            pass
        if steady:
            res["steady_state_all_hits"] = steady
        if first_step_ms is not None:
            res["cold_start"] = {"first_step_ms": first_step_ms, "over_timed_step": first_step_ms / (dt / args.steps * 1e3),
                                 "note": "step 0 of the stream on an empty matrix (incr batch + get batch): every row is created, the hot rows double up to fifteen times"}
        res["table"] = {k: st[k] for k in ("rows", "dir_slots", "arena_units", "arena_mapped", "batches",
                                           "rounds", "deferred_ops", "rows_grown", "dir_grown", "spec_chains", "spec_refused", "bulk_rounds")}
        if world == 1 and not sharded and not args.no_extras:
            del xs_all, ys_all
            res["config3_getrow"] = guarded(run_config3, torch, dev)
            res["config5_file_1gpu"] = guarded(run_config5, torch, dev)
        if world == 1:
            ra = random_access_roofline(torch, dev)
            big = random_access_roofline(torch, dev, gib=32)
            ra["table_sized_buffer_32gib"] = {k: v for k, v in big.items() if k.endswith("_per_s")}
            g_get = res["roofline_get"]["gops_per_s"]; g_inc = res["roofline"]["gops_per_s"]
            ra.update({
                "get_gops_per_s": g_get, "incr_gops_per_s": g_inc,
                # a get is a directory touch + a dependent cell touch; an incr adds one returning atomic
                "get_frac_of_chain2": g_get / ra["chain2_gtouch_per_s"],
                "get_frac_of_read8": g_get / ra["read8_gtouch_per_s"],
                "incr_frac_of_atomic_ret": g_inc / ra["atomic_ret_gtouch_per_s"],
                # the composite ceiling of the MIXED step: one random read per get, one returning atomic per incr --
                # 2 ops in 1/read8 + 1/atomic_ret seconds -- next to the north star's plain read8 fraction
                "mixed_ceiling_gops_per_s": 2.0 / (1.0 / ra["read8_gtouch_per_s"] + 1.0 / ra["atomic_ret_gtouch_per_s"]),
                "mixed_frac_of_read8": res["value"] / 1e3 / ra["read8_gtouch_per_s"],
                "all_hits_frac_of_read8": (steady["Mops_per_s"] / 1e3 / ra["read8_gtouch_per_s"]) if steady else None,
                "mixed_frac_of_mixed_ceiling": res["value"] / 1e3 * (1.0 / ra["read8_gtouch_per_s"] + 1.0 / ra["atomic_ret_gtouch_per_s"]) / 2.0,
                "note": "ceilings are uniform-random over the buffer; the Zipf stream re-touches hot lines "
                        "in L2/Infinity Cache, so fractions above 1 are cache assistance, not an error",
            })
            res["random_access"] = ra
        if world == 1 and not args.no_cpu:
            res["cpu_baseline"] = cpu_baseline(1 << args.cpu_sample_lg, torch, dev)
    if rank == 0:
        emit(res, json_out)
    if comm is not None:
        comm.shutdown()
    m.close()
    if sharded:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
