#!/usr/bin/env python3
"""Session recommendations (smatrix_cf_recommend_batch_dev) against the composition a caller could build without it:
cf_neighbors_batch_dev over every distinct item of every session, then torch on the device (exclusion of id 0 and of the
session's items, scatter-add per (session, id), a sort, the k best per session).  Same process, same matrix, alternated.

  python3 tools/probe/cf_recommend_time.py [import_sessions_lg] [query_sessions_lg] [reps]

The matrix: 2^20 sessions (default) of 12 ids drawn from bench.py's Zipf(1.1) stream over 1 M scrambled ids, imported by
cf_import_sessions_dev.  The query: 2^16 sessions (default) of 8..32 items; 7/8 of them from the items of rank >= 20 000 (small
rows: the LDS tier), 1/8 with one to three items of rank 200..5 000 (rows of thousands of cells: the global tier).  The tier of a
session is estimated from rowlen (table size = the power of two the growth rule gives).  Times: HIP events, best of `reps`
after one warm-up.  The fused call on all sessions and the composition are ALTERNATED rep by rep (fused, composition, fused,
...); then the fused call on each tier's sessions alone.  Prints one JSON line per k."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libsmatrix_amd import SparseMatrix, Stream  # noqa: E402

LDS_SLOTS = 4096                       # kernels/recommend.hpp REC_LDS_SLOTS


def timed(fns, reps):
    """best time of each of fns, the calls alternated: fns[0], fns[1], .. fns[0], fns[1], .."""
    for fn in fns:
        fn()
    best = [1e9] * len(fns)
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            best[i] = min(best[i], e0.elapsed_time(e1))
    return best


def main():
    imp_lg = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    q_lg = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    L = 12
    n_imp = 1 << imp_lg
    gen = Stream("zipf", bench.SEED + 7, bench.N_IDS, bench.ZIPF_S, 1)
    ids = torch.empty(n_imp * L, dtype=torch.int32, device=dev); scratch = torch.empty_like(ids)
    gen.fill_device(0, n_imp * L, ids.data_ptr(), scratch.data_ptr(), stream)
    off = torch.arange(0, n_imp + 1, dtype=torch.int64, device=dev) * L
    op_off = torch.arange(0, n_imp + 1, dtype=torch.int64, device=dev) * (L * L)
    m = SparseMatrix()
    m.cf_import_sessions_dev(n_imp, off.data_ptr(), ids.data_ptr(), op_off.data_ptr(), n_imp * L * L, stream)
    torch.cuda.synchronize()
    gen.close()
    items, counts = torch.unique(ids, return_counts=True)
    by_rank = items[torch.argsort(counts, descending=True, stable=True)].cpu().numpy().astype(np.uint32)
    del ids, scratch, off, op_off, items, counts
    rl = {}

    # the query
    rng = np.random.default_rng(2026)
    nq = 1 << q_lg
    lens = rng.integers(8, 33, nq)
    tail = by_rank[20000:]
    mid = by_rank[200:5000]
    sess = []
    for i in range(nq):
        s = rng.choice(tail, int(lens[i]))
        if i % 8 == 7:
            j = int(rng.integers(1, 4))
            s[:j] = rng.choice(mid, j)
            rng.shuffle(s)
        sess.append(s.astype(np.uint32))
    flat = np.concatenate(sess)
    uq = np.unique(flat)
    rlen = m.rowlen_batch(uq).astype(np.int64)
    size = np.maximum(16, 1 << np.ceil(np.log2(np.maximum(2 * (rlen - 1), 1))).astype(np.int64))
    size[rlen == 0] = 0
    for a, z in zip(uq.tolist(), size.tolist()):
        rl[a] = z
    bound = np.array([sum(rl[int(a)] for a in np.unique(s)) + s.size for s in sess])
    lds = bound <= LDS_SLOTS

    def dev_set(sel):
        ss = [s for s, keep in zip(sess, sel) if keep]
        o = np.zeros(len(ss) + 1, np.int64)
        np.cumsum([s.size for s in ss], out=o[1:])
        return (len(ss), torch.from_numpy(o).to(dev), torch.from_numpy(np.concatenate(ss).view(np.int32)).to(dev),
                int(sum(rl[int(a)] for s in ss for a in np.unique(s))))

    sets = {"all": dev_set(np.ones(nq, bool)), "lds": dev_set(lds), "global": dev_set(~lds)}
    n_all, d_off, d_items, _ = sets["all"]

    # the composition's fixed inputs: distinct (session, item) pairs at their first position, neighbour offsets
    seg = torch.repeat_interleave(torch.arange(n_all, device=dev), torch.diff(d_off))
    key = (seg << 32) | (d_items.long() & 0xFFFFFFFF)
    ukey = torch.unique(key)                                           # the session's item set, sorted (session, item)
    c_seg, c_items = (ukey >> 32), (ukey & 0xFFFFFFFF).to(torch.int32)
    c_len = torch.empty(c_items.numel(), dtype=torch.int32, device=dev)
    m.rowlen_batch_dev(c_items.numel(), c_items.data_ptr(), c_len.data_ptr(), stream)
    c_off = torch.zeros(c_items.numel() + 1, dtype=torch.int64, device=dev)
    c_off[1:] = torch.cumsum(c_len.long() + 1, 0)
    total_nb = int(c_off[-1].item())
    nb_ids = torch.empty(total_nb, dtype=torch.int32, device=dev)
    nb_sc = torch.empty(total_nb, dtype=torch.float64, device=dev)
    nb_cnt = torch.empty(c_items.numel(), dtype=torch.int32, device=dev)
    rows = []
    for k in (10, 64):
        outs = {}
        res = {"k": k, "query_sessions": nq, "items_per_session": "8..32", "import_sessions": n_imp, "import_ids_per_session": L,
               "sessions_lds_tier_est": int(lds.sum()), "sessions_global_tier_est": int((~lds).sum())}
        for name, (n, o, it, cells) in sets.items():
            if n == 0:
                continue
            r_ids = torch.zeros(n * k, dtype=torch.int32, device=dev)
            r_sc = torch.zeros(n * k, dtype=torch.float64, device=dev)
            r_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
            outs[name] = (n, o, it, cells, r_ids, r_sc, r_cnt,
                          lambda n=n, o=o, it=it, r_ids=r_ids, r_sc=r_sc, r_cnt=r_cnt: m.cf_recommend_batch_dev(
                              n, o.data_ptr(), it.data_ptr(), k, r_ids.data_ptr(), r_sc.data_ptr(), r_cnt.data_ptr(), stream))

        def compose():
            m.cf_neighbors_batch_dev(c_items.numel(), c_items.data_ptr(), c_off.data_ptr(), nb_ids.data_ptr(), nb_sc.data_ptr(),
                                     nb_cnt.data_ptr(), stream)
            pos = torch.arange(total_nb, device=dev)
            owner = torch.searchsorted(c_off, pos, right=True) - 1
            valid = (pos - c_off[owner]) < nb_cnt[owner].long()
            b = nb_ids.long() & 0xFFFFFFFF
            s_of = c_seg[owner]
            kk = (s_of << 32) | b
            idx = torch.searchsorted(ukey, kk).clamp(max=ukey.numel() - 1)
            keep = valid & (b != 0) & (ukey[idx] != kk)
            kk, sc = kk[keep], nb_sc[keep]
            uk, inv = torch.unique(kk, return_inverse=True)
            tot = torch.zeros(uk.numel(), dtype=torch.float64, device=dev).index_add_(0, inv, sc)
            us, ub = uk >> 32, uk & 0xFFFFFFFF
            o1 = torch.argsort(ub, stable=True)                          # (session asc, score desc, id asc)
            o2 = o1[torch.argsort(-tot[o1], stable=True)]
            o3 = o2[torch.argsort(us[o2], stable=True)]
            ss = us[o3]
            first = torch.searchsorted(ss, torch.arange(n_all, device=dev))
            rank = torch.arange(ss.numel(), device=dev) - first[ss]
            top = rank < k
            c_ids = torch.zeros(n_all * k, dtype=torch.int64, device=dev)
            c_ids[ss[top] * k + rank[top]] = ub[o3][top]
            return c_ids
        for name in outs:
            n, o, it, cells = outs[name][:4]
            if name == "all":
                t, res["composition_ms"] = timed([outs[name][7], compose], reps)
            else:
                t = timed([outs[name][7]], reps)[0]
            res["fused_%s_ms" % name] = t
            res["fused_%s_sessions_per_s" % name] = n / t * 1e3
            res["fused_%s_row_slots_scanned_per_s" % name] = cells / t * 1e3
        res["composition_neighbours"] = total_nb
        c_ids = compose()
        f_ids = outs["all"][4].long() & 0xFFFFFFFF
        same = (c_ids.view(n_all, k) == f_ids.view(n_all, k)).all(1)
        res["composition_same_ids_sessions"] = int(same.sum().item())
        res["fused_over_composition_speedup"] = res["composition_ms"] / res["fused_all_ms"]
        print(json.dumps(res), flush=True)
        rows.append(res)
    m.close()


if __name__ == "__main__":
    main()
