// smx_recommend.inc -- session recommendations (include/smatrix_batch.h smatrix_cf_recommend_batch / _dev,
// smatrix_cf_recommend_filtered / _dev, smatrix_cf_recommend_sim / _dev and smatrix_cf_rank / _dev), host side.
// Included by smx_runtime.hip inside the translation unit, after smx_export.inc (uses Matrix, DevBuf, HIP_OK, and the export's
// u32 -> u64 scan kernels); the device code is kernels/recommend.hpp.
//
// Under the matrix lock, after the scalar mirror has been written back (cache_sync):
//   1. k_rec_bound sorts the sessions into the LDS tier and the global tier; ONE read-back of RecCtl (counts, global-tier sizes)
//   2. k_rec_lds: every LDS-tier session, one workgroup each
//   3. the global tier, per group of sessions whose tables fit REC_GROUP_SLOTS (normally one group): zeroed tables, k_rec_gl_init,
//      per block of item positions the chunk counts (k_rec_gl_plan) and their scan, a k_rec_gl_scan launch per position (the
//      kernel boundary keeps the items in session order), k_rec_gl_topk, k_rec_gl_merge
// The filtered call is the same driver with a RecFilt (weights, exclusion lists, deny bitmap) and the kernels' <true> instances;
// with nothing given it runs the <false> ones, the code of smatrix_cf_recommend_batch.
// The sim call is the filtered call with a measure and a shrinkage in the RecFilt and, for the two kernels that make a score,
// their _sim instances; with SMATRIX_SIM_COSINE and shrink 0 it IS the filtered call.
// The rank call is the sim call with another ending (rec_run<.., .., true>): the answers are filled with "no answer", k_rec_lds_rank
// stands for k_rec_lds, and k_rec_gl_rank for k_rec_gl_topk + k_rec_gl_merge; everything before the ending is shared.

namespace {

constexpr uint64_t REC_GROUP_SLOTS = 1ull << 25;      // global-tier tables per group: 640 MB (20 bytes a slot), plus the largest table
constexpr uint64_t REC_PLAN_MAX = 1ull << 24;         // (position, session) counts per plan

struct RecScratch {
  DevBuf<RecCtl> ctl;
  DevBuf<uint32_t> lds_list, big_list, gk, owner, zpos, cnt, li;
  DevBuf<unsigned long long> big_off;
  DevBuf<uint8_t> tlg;
  DevBuf<double> gq, gs;
  DevBuf<long long> lk;
  DevBuf<uint64_t> scan, part;
  DevBuf<uint32_t> h_items, h_ids, h_counts;         // the host flavour's device copies of the caller's arrays
  DevBuf<uint64_t> h_off;
  DevBuf<double> h_scores, h_w;                      // ... and the filtered call's: weights, exclusion lists, deny bitmap
  DevBuf<uint64_t> h_exoff;
  DevBuf<uint32_t> h_ex, h_deny;
  DevBuf<uint64_t> h_toff;                           // ... and the rank call's: target lists, ranks (scores: h_scores, counts: h_counts)
  DevBuf<uint32_t> h_tg, h_ranks;
  DevBuf<uint64_t> h_eoff;                           // ... and the explain call's (smx_explain.inc): entry offsets (terms: h_scores, cc: h_ids),
  DevBuf<double> e_ra, e_cb;                         // and both its flavours' doubles per session entry and per target
  hipEvent_t done = nullptr;                         // recorded behind the last call's work (its stream may be any)
};

RecScratch& rec_of(Matrix* m) {
  if (!m->rec) m->rec = new RecScratch();
  return *static_cast<RecScratch*>(m->rec);
}

template <typename T>
bool rec_big(const DevBuf<T>& b) { return b.cap * sizeof(T) > ((size_t)64 << 20); }
template <typename T>
void rec_trim(DevBuf<T>& b, bool all) {
  if (all || rec_big(b)) b.release();                                 // (as the export: no HBM pinned for good)
}
void rec_trim_all(RecScratch& x, bool all) {
  rec_trim(x.ctl, all); rec_trim(x.lds_list, all); rec_trim(x.big_list, all); rec_trim(x.gk, all); rec_trim(x.owner, all);
  rec_trim(x.zpos, all); rec_trim(x.cnt, all); rec_trim(x.li, all); rec_trim(x.big_off, all); rec_trim(x.tlg, all); rec_trim(x.gq, all);
  rec_trim(x.gs, all); rec_trim(x.lk, all); rec_trim(x.scan, all); rec_trim(x.part, all); rec_trim(x.h_items, all); rec_trim(x.h_ids, all);
  rec_trim(x.h_counts, all); rec_trim(x.h_off, all); rec_trim(x.h_scores, all); rec_trim(x.h_w, all); rec_trim(x.h_exoff, all);
  rec_trim(x.h_ex, all); rec_trim(x.h_deny, all); rec_trim(x.h_toff, all); rec_trim(x.h_tg, all); rec_trim(x.h_ranks, all);
  rec_trim(x.h_eoff, all); rec_trim(x.e_ra, all); rec_trim(x.e_cb, all);
}

bool rec_any_big(const RecScratch& x) {
  return rec_big(x.lds_list) || rec_big(x.big_list) || rec_big(x.gk) || rec_big(x.owner) || rec_big(x.zpos) || rec_big(x.cnt) ||
         rec_big(x.li) || rec_big(x.big_off) || rec_big(x.tlg) || rec_big(x.gq) || rec_big(x.gs) || rec_big(x.lk) || rec_big(x.scan) ||
         rec_big(x.part);
}

// The scratch is the matrix's, the stream the caller's: a call on another stream than the one before it (or the host flavour,
// on the matrix's stream) must not touch the scratch while kernels of the earlier call may still read it.
void rec_begin(RecScratch& x, hipStream_t s) {
  if (x.done) HIP_OK(hipStreamWaitEvent(s, x.done, 0));
}
void rec_end(RecScratch& x, hipStream_t s) {
  if (!x.done) HIP_OK(hipEventCreateWithFlags(&x.done, hipEventDisableTiming));
  HIP_OK(hipEventRecord(x.done, s));
}

// out[0 .. n] = exclusive prefix of n u32 counts (the export's scan kernels)
void rec_scan(RecScratch& x, hipStream_t s, const uint32_t* in, uint64_t n, uint64_t* out) {
  const uint32_t nt = (uint32_t)((n + EX_TILE - 1) / EX_TILE);
  x.part.need((size_t)nt + 1);
  if (nt) hipLaunchKernelGGL(k_ex_scan_reduce, dim3(nt), dim3(EX_THREADS), 0, s, in, n, x.part.p);
  hipLaunchKernelGGL(k_ex_scan_part, dim3(1), dim3(EX_THREADS), 0, s, x.part.p, nt);
  hipLaunchKernelGGL(k_ex_scan_apply, dim3(std::max<uint32_t>(nt, 1)), dim3(EX_THREADS), 0, s, in, n, x.part.p, nt, out);
  HIP_OK(hipGetLastError());
}

// the whole call on stream s, every array on the device; returns with the work enqueued (after one synchronising read-back).
// F: the filtered call with something given in f; S: the sim call, the score is f.m's.  -1 (nothing but k_rec_bound has run) for
// a bad weight, 0 otherwise.
// R: the ending is the rank call's, not the top-k: rk's answers are filled and written, d_counts receives the candidate counts,
// k / d_ids / d_scores are not used
template <bool F, bool S, bool R>
int rec_run(Matrix* m, RecScratch& x, hipStream_t s, uint32_t n, const uint64_t* d_off, const uint32_t* d_items, uint32_t k,
            uint32_t* d_ids, double* d_scores, uint32_t* d_counts, const RecFilt& f, const RecRank& rk) {
  DirSlot* dir = m->d_dir;
  const uint32_t dmask = m->dir_size - 1;
  if (R) hipLaunchKernelGGL(k_rec_rank_fill, dim3(1024), dim3(256), 0, s, n, rk);
  x.ctl.need(1); x.lds_list.need(n); x.big_list.need(n); x.big_off.need(n); x.tlg.need(n);
  HIP_OK(hipMemsetAsync(x.ctl.p, 0, sizeof(RecCtl), s));
  hipLaunchKernelGGL(k_rec_bound<F>, dim3(std::min<uint32_t>(blocks_for((uint64_t)n * 64), 16384)), dim3(256), 0, s, dir, dmask, n, d_off,
                     d_items, (uint64_t)(m->arena.mapped / 8), x.ctl.p, x.lds_list.p, x.tlg.p, x.big_list.p, x.big_off.p, d_counts, f);
  HIP_OK(hipGetLastError());
  RecCtl c;
  HIP_OK(hipMemcpyAsync(&c, x.ctl.p, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (F && c.bad) return -1;
  if (c.n_lds && R)
    hipLaunchKernelGGL(S ? k_rec_lds_rank_sim<F> : k_rec_lds_rank<F>, dim3(std::min<uint32_t>(c.n_lds, 1u << 16)), dim3(REC_LDS_THREADS), 0, s, dir,
                       dmask, m->arena.base, x.ctl.p, x.lds_list.p, x.tlg.p, d_off, d_items, rk, d_counts, f);
  else if (c.n_lds)
    hipLaunchKernelGGL(S ? k_rec_lds_sim<F> : k_rec_lds<F>, dim3(std::min<uint32_t>(c.n_lds, 1u << 16)), dim3(REC_LDS_THREADS), 0, s, dir, dmask, m->arena.base,
                       x.ctl.p, x.lds_list.p, x.tlg.p, d_off, d_items, k, d_ids, d_scores, d_counts, f);
  HIP_OK(hipGetLastError());
  if (!c.n_big) return 0;
  const uint64_t ngroups = (c.total_slots + REC_GROUP_SLOTS - 1) / REC_GROUP_SLOTS;
  const uint64_t cap = ngroups == 1 ? c.total_slots : REC_GROUP_SLOTS + c.max_slots;
  const uint64_t nseg = cap / REC_SEG;
  const uint32_t np = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(c.max_len, REC_PLAN_MAX / c.n_big));
  x.gk.need(cap); x.gq.need(cap); x.gs.need(cap); x.owner.need(nseg); x.zpos.need(c.n_big);
  if (!R) { x.lk.need(nseg * 64); x.li.need(nseg * 64); }
  x.cnt.need((uint64_t)np * c.n_big); x.scan.need((uint64_t)np * c.n_big + 1);
  RecGl G{x.gk.p, x.gq.p, x.gs.p, x.owner.p, x.zpos.p, x.big_list.p, x.big_off.p, x.tlg.p, c.n_big, 0u, REC_GROUP_SLOTS};
  for (uint64_t g = 0; g < ngroups; g++) {
    G.g = (uint32_t)g;
    const uint64_t ext = ngroups == 1 ? cap : std::min<uint64_t>(cap, c.total_slots - g * REC_GROUP_SLOTS + c.max_slots);
    HIP_OK(hipMemsetAsync(x.gk.p, 0, ext * 4, s));
    HIP_OK(hipMemsetAsync(x.gq.p, 0, ext * 8, s));
    HIP_OK(hipMemsetAsync(x.gs.p, 0, ext * 8, s));
    HIP_OK(hipMemsetAsync(x.owner.p, 0xff, nseg * 4, s));
    HIP_OK(hipMemsetAsync(x.zpos.p, 0, (size_t)c.n_big * 4, s));
    hipLaunchKernelGGL(k_rec_gl_init<F>, dim3(std::min<uint32_t>(c.n_big, 1u << 16)), dim3(256), 0, s, G, d_off, d_items, f);
    HIP_OK(hipGetLastError());
    for (uint32_t p0 = 0; p0 < c.max_len; p0 += np) {
      const uint32_t nj = std::min<uint32_t>(np, c.max_len - p0);
      const uint64_t nt = (uint64_t)nj * c.n_big;
      hipLaunchKernelGGL(k_rec_gl_plan, dim3(blocks_for(nt)), dim3(256), 0, s, G, dir, dmask, d_off, d_items, p0, nj, x.cnt.p);
      HIP_OK(hipGetLastError());
      rec_scan(x, s, x.cnt.p, nt, x.scan.p);
      for (uint32_t j = 0; j < nj; j++)
        hipLaunchKernelGGL(S ? k_rec_gl_scan_sim<F> : k_rec_gl_scan<F>, dim3(2048), dim3(256), 0, s, G, dir, dmask, m->arena.base, d_off,
                           d_items, p0, j, x.scan.p, f);
      HIP_OK(hipGetLastError());
    }
    if (R) {
      hipLaunchKernelGGL(k_rec_gl_rank, dim3(std::min<uint32_t>(c.n_big, 1u << 16)), dim3(REC_MERGE_THREADS), 0, s, G, rk, d_counts);
    } else {
      hipLaunchKernelGGL(k_rec_gl_topk, dim3((uint32_t)std::min<uint64_t>((nseg + 3) / 4, 16384)), dim3(256), 0, s, G, nseg, k, x.lk.p,
                         x.li.p);
      hipLaunchKernelGGL(k_rec_gl_merge, dim3(std::min<uint32_t>(c.n_big, 1u << 16)), dim3(REC_MERGE_THREADS), 0, s, G, k, x.lk.p, x.li.p,
                         d_ids, d_scores, d_counts);
    }
    HIP_OK(hipGetLastError());
  }
  return 0;
}

// what both flavours of the filtered call refuse before anything else
bool rec_filt_args_ok(size_t n_sessions, const void* ex_offsets, const void* ex_items, const void* deny_bits, uint64_t deny_n,
                      uint32_t k) {
  if (k == 0 || k > 64 || n_sessions > 0xffffffffull) return false;
  if (deny_n > (1ull << 32) || (!deny_bits && deny_n)) return false;
  return (ex_offsets == nullptr) == (ex_items == nullptr);
}
bool rec_filt_any(const RecFilt& f) { return f.w || f.ex_off || f.deny_n; }
// (the sim call refuses on top of them what sim_args_ok of smx_merge.inc refuses: shrink is a host scalar in both flavours)

// the kernels' instances for what the call was given: <false, .> with no filter, <., true> with a measure; R: the rank ending
template <bool R>
int rec_dispatch(Matrix* m, RecScratch& x, hipStream_t s, uint32_t n, const uint64_t* d_off, const uint32_t* d_items, uint32_t k,
                 uint32_t* d_ids, double* d_scores, uint32_t* d_counts, const RecFilt& f, bool sim, const RecRank& rk) {
  if (sim) return rec_filt_any(f) ? rec_run<true, true, R>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk)
                                  : rec_run<false, true, R>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk);
  return rec_filt_any(f) ? rec_run<true, false, R>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk)
                         : rec_run<false, false, R>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk);
}

// smatrix_cf_recommend_filtered_dev and smatrix_cf_recommend_sim_dev behind their refusals; sim: score by f_m, not by the cosine
int rec_filtered_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items, const double* d_weights,
                     const uint64_t* d_ex_offsets, const uint32_t* d_ex_items, const uint32_t* d_deny_bits, uint64_t deny_n, uint32_t k,
                     uint32_t* d_ids, double* d_scores, uint32_t* d_counts, void* hip_stream, bool sim, SimArgs f_m) {
  if (n_sessions == 0) return 0;
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
  RecScratch& x = rec_of(m);
  rec_begin(x, s);
  const RecFilt f{d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, f_m};
  const int rc = rec_dispatch<false>(m, x, s, (uint32_t)n_sessions, d_offsets, d_items, k, d_ids, d_scores, d_counts, f, sim, RecRank{});
  rec_end(x, s);
  if (!hip_stream || rec_any_big(x)) HIP_OK(hipStreamSynchronize(s));   // (the kernels use the buffers rec_trim_all releases)
  rec_trim_all(x, false);
  return rc;
}

// the host flavours of the same two
int rec_filtered_host(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                      const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, uint32_t k,
                      uint32_t* ids, double* scores, uint32_t* counts, bool sim, SimArgs f_m) {
  if (n_sessions == 0) return 0;
  const uint64_t n = n_sessions, n_items = offsets[n] - offsets[0];
  if (weights)
    for (uint64_t i = 0; i < n_items; i++)
      if (!(weights[offsets[0] + i] >= 0.0) || !std::isfinite(weights[offsets[0] + i])) return -1;   // (before the device is touched)
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = m->stream;
  RecScratch& x = rec_of(m);
  rec_begin(x, s);
  const uint64_t n_ex = ex_offsets ? ex_offsets[n] - ex_offsets[0] : 0, n_deny = (deny_n + 31) / 32;
  std::vector<uint64_t> rel(n + 1), ex_rel(ex_offsets ? n + 1 : 0);
  for (uint64_t i = 0; i <= n; i++) rel[i] = offsets[i] - offsets[0];
  for (uint64_t i = 0; i < ex_rel.size(); i++) ex_rel[i] = ex_offsets[i] - ex_offsets[0];
  x.h_off.need(n + 1); x.h_items.need(std::max<uint64_t>(n_items, 1)); x.h_ids.need(n * k); x.h_scores.need(n * k); x.h_counts.need(n);
  HIP_OK(hipMemcpyAsync(x.h_off.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_items) HIP_OK(hipMemcpyAsync(x.h_items.p, items + offsets[0], n_items * 4, hipMemcpyHostToDevice, s));
  RecFilt f{};
  f.m = f_m;
  if (weights) {
    x.h_w.need(std::max<uint64_t>(n_items, 1));
    if (n_items) HIP_OK(hipMemcpyAsync(x.h_w.p, weights + offsets[0], n_items * 8, hipMemcpyHostToDevice, s));
    f.w = x.h_w.p;
  }
  if (ex_offsets) {
    x.h_exoff.need(n + 1); x.h_ex.need(std::max<uint64_t>(n_ex, 1));
    HIP_OK(hipMemcpyAsync(x.h_exoff.p, ex_rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_ex) HIP_OK(hipMemcpyAsync(x.h_ex.p, ex_items + ex_offsets[0], n_ex * 4, hipMemcpyHostToDevice, s));
    f.ex_off = x.h_exoff.p; f.ex = x.h_ex.p;
  }
  if (deny_n) {
    x.h_deny.need(n_deny);
    HIP_OK(hipMemcpyAsync(x.h_deny.p, deny_bits, n_deny * 4, hipMemcpyHostToDevice, s));
    f.deny = x.h_deny.p; f.deny_n = deny_n;
  }
  HIP_OK(hipMemsetAsync(x.h_ids.p, 0, n * k * 4, s));                // unused entries read 0, as smatrix_cf_recommend_batch's
  HIP_OK(hipMemsetAsync(x.h_scores.p, 0, n * k * 8, s));
  rec_dispatch<false>(m, x, s, (uint32_t)n, x.h_off.p, x.h_items.p, k, x.h_ids.p, x.h_scores.p, x.h_counts.p, f, sim, RecRank{});
  HIP_OK(hipMemcpyAsync(counts, x.h_counts.p, n * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(ids, x.h_ids.p, n * k * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(scores, x.h_scores.p, n * k * 8, hipMemcpyDeviceToHost, s));
  rec_end(x, s);
  HIP_OK(hipStreamSynchronize(s));
  rec_trim_all(x, false);
  return 0;
}

// smatrix_cf_rank_dev behind its refusals: rec_filtered_dev with the rank ending
int rec_rank_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items, const double* d_weights,
                 const uint64_t* d_ex_offsets, const uint32_t* d_ex_items, const uint32_t* d_deny_bits, uint64_t deny_n, bool sim,
                 SimArgs f_m, const RecRank& rk, uint32_t* d_n_candidates, void* hip_stream) {
  if (n_sessions == 0) return 0;
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
  RecScratch& x = rec_of(m);
  rec_begin(x, s);
  const RecFilt f{d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, f_m};
  const int rc = rec_dispatch<true>(m, x, s, (uint32_t)n_sessions, d_offsets, d_items, 0u, nullptr, nullptr, d_n_candidates, f, sim, rk);
  rec_end(x, s);
  if (!hip_stream || rec_any_big(x)) HIP_OK(hipStreamSynchronize(s));   // (the kernels use the buffers rec_trim_all releases)
  rec_trim_all(x, false);
  return rc;
}

// the host flavour: rec_filtered_host's copies, and the target lists and the answers' [t_offsets[0], t_offsets[n]) beside them
int rec_rank_host(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                  const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, bool sim, SimArgs f_m,
                  const uint64_t* t_offsets, const uint32_t* targets, uint32_t* ranks, double* scores, uint32_t* n_candidates) {
  if (n_sessions == 0) return 0;
  const uint64_t n = n_sessions, n_items = offsets[n] - offsets[0], n_t = t_offsets[n] - t_offsets[0];
  if (weights)
    for (uint64_t i = 0; i < n_items; i++)
      if (!(weights[offsets[0] + i] >= 0.0) || !std::isfinite(weights[offsets[0] + i])) return -1;   // (before the device is touched)
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = m->stream;
  RecScratch& x = rec_of(m);
  rec_begin(x, s);
  const uint64_t n_ex = ex_offsets ? ex_offsets[n] - ex_offsets[0] : 0, n_deny = (deny_n + 31) / 32;
  std::vector<uint64_t> rel(n + 1), t_rel(n + 1), ex_rel(ex_offsets ? n + 1 : 0);
  for (uint64_t i = 0; i <= n; i++) { rel[i] = offsets[i] - offsets[0]; t_rel[i] = t_offsets[i] - t_offsets[0]; }
  for (uint64_t i = 0; i < ex_rel.size(); i++) ex_rel[i] = ex_offsets[i] - ex_offsets[0];
  x.h_off.need(n + 1); x.h_items.need(std::max<uint64_t>(n_items, 1)); x.h_counts.need(n);
  x.h_toff.need(n + 1); x.h_tg.need(std::max<uint64_t>(n_t, 1)); x.h_ranks.need(std::max<uint64_t>(n_t, 1)); x.h_scores.need(std::max<uint64_t>(n_t, 1));
  HIP_OK(hipMemcpyAsync(x.h_off.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_items) HIP_OK(hipMemcpyAsync(x.h_items.p, items + offsets[0], n_items * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(x.h_toff.p, t_rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_t) HIP_OK(hipMemcpyAsync(x.h_tg.p, targets + t_offsets[0], n_t * 4, hipMemcpyHostToDevice, s));
  RecFilt f{};
  f.m = f_m;
  if (weights) {
    x.h_w.need(std::max<uint64_t>(n_items, 1));
    if (n_items) HIP_OK(hipMemcpyAsync(x.h_w.p, weights + offsets[0], n_items * 8, hipMemcpyHostToDevice, s));
    f.w = x.h_w.p;
  }
  if (ex_offsets) {
    x.h_exoff.need(n + 1); x.h_ex.need(std::max<uint64_t>(n_ex, 1));
    HIP_OK(hipMemcpyAsync(x.h_exoff.p, ex_rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_ex) HIP_OK(hipMemcpyAsync(x.h_ex.p, ex_items + ex_offsets[0], n_ex * 4, hipMemcpyHostToDevice, s));
    f.ex_off = x.h_exoff.p; f.ex = x.h_ex.p;
  }
  if (deny_n) {
    x.h_deny.need(n_deny);
    HIP_OK(hipMemcpyAsync(x.h_deny.p, deny_bits, n_deny * 4, hipMemcpyHostToDevice, s));
    f.deny = x.h_deny.p; f.deny_n = deny_n;
  }
  const RecRank rk{x.h_toff.p, x.h_tg.p, x.h_ranks.p, x.h_scores.p};
  rec_dispatch<true>(m, x, s, (uint32_t)n, x.h_off.p, x.h_items.p, 0u, nullptr, nullptr, x.h_counts.p, f, sim, rk);
  HIP_OK(hipMemcpyAsync(n_candidates, x.h_counts.p, n * 4, hipMemcpyDeviceToHost, s));
  if (n_t) HIP_OK(hipMemcpyAsync(ranks + t_offsets[0], x.h_ranks.p, n_t * 4, hipMemcpyDeviceToHost, s));
  if (n_t) HIP_OK(hipMemcpyAsync(scores + t_offsets[0], x.h_scores.p, n_t * 8, hipMemcpyDeviceToHost, s));
  rec_end(x, s);
  HIP_OK(hipStreamSynchronize(s));
  rec_trim_all(x, false);
  return 0;
}

// what both flavours of the rank call refuse before anything else (k: there is none)
bool rec_rank_args_ok(size_t n_sessions, const void* ex_offsets, const void* ex_items, const void* deny_bits, uint64_t deny_n, int sim,
                      double shrink, const void* t_offsets, const void* targets) {
  return sim_args_ok(sim, shrink) && rec_filt_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, 1u) && t_offsets && targets;
}

void recommend_release(Matrix* m) {
  if (!m->rec) return;
  RecScratch* x = static_cast<RecScratch*>(m->rec);
  if (x->done) { HIP_OK(hipEventSynchronize(x->done)); (void)hipEventDestroy(x->done); }
  rec_trim_all(*x, true);
  delete static_cast<RecScratch*>(m->rec);
  m->rec = nullptr;
}

}  // namespace

extern "C" {

int smatrix_cf_recommend_batch_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items, uint32_t k,
                                   uint32_t* d_ids, double* d_scores, uint32_t* d_counts, void* hip_stream) {
  if (k == 0 || k > 64 || n_sessions > 0xffffffffull) return -1;
  if (n_sessions == 0) return 0;
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
  RecScratch& x = rec_of(m);
  rec_begin(x, s);
  rec_run<false, false, false>(m, x, s, (uint32_t)n_sessions, d_offsets, d_items, k, d_ids, d_scores, d_counts, RecFilt{}, RecRank{});
  rec_end(x, s);
  if (!hip_stream || rec_any_big(x)) HIP_OK(hipStreamSynchronize(s));   // (the kernels use the buffers rec_trim_all releases)
  rec_trim_all(x, false);
  return 0;
}

int smatrix_cf_recommend_batch(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, uint32_t k,
                               uint32_t* ids, double* scores, uint32_t* counts) {
  if (k == 0 || k > 64 || n_sessions > 0xffffffffull) return -1;
  if (n_sessions == 0) return 0;
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = m->stream;
  RecScratch& x = rec_of(m);
  rec_begin(x, s);
  const uint64_t n = n_sessions, n_items = offsets[n] - offsets[0];
  std::vector<uint64_t> rel(n + 1);
  for (uint64_t i = 0; i <= n; i++) rel[i] = offsets[i] - offsets[0];
  x.h_off.need(n + 1); x.h_items.need(std::max<uint64_t>(n_items, 1)); x.h_ids.need(n * k); x.h_scores.need(n * k); x.h_counts.need(n);
  HIP_OK(hipMemcpyAsync(x.h_off.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_items) HIP_OK(hipMemcpyAsync(x.h_items.p, items + offsets[0], n_items * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemsetAsync(x.h_ids.p, 0, n * k * 4, s));                // unused entries read 0, as cf_topk_batch's
  HIP_OK(hipMemsetAsync(x.h_scores.p, 0, n * k * 8, s));
  rec_run<false, false, false>(m, x, s, (uint32_t)n, x.h_off.p, x.h_items.p, k, x.h_ids.p, x.h_scores.p, x.h_counts.p, RecFilt{}, RecRank{});
  HIP_OK(hipMemcpyAsync(counts, x.h_counts.p, n * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(ids, x.h_ids.p, n * k * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(scores, x.h_scores.p, n * k * 8, hipMemcpyDeviceToHost, s));
  rec_end(x, s);
  HIP_OK(hipStreamSynchronize(s));
  rec_trim_all(x, false);
  return 0;
}

int smatrix_cf_recommend_filtered_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                      const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                      const uint32_t* d_deny_bits, uint64_t deny_n, uint32_t k, uint32_t* d_ids, double* d_scores,
                                      uint32_t* d_counts, void* hip_stream) {
  if (!rec_filt_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, k)) return -1;
  return rec_filtered_dev(self, n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, k, d_ids,
                          d_scores, d_counts, hip_stream, false, SimArgs{});
}

int smatrix_cf_recommend_filtered(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                                  const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                                  const uint32_t* deny_bits, uint64_t deny_n, uint32_t k, uint32_t* ids, double* scores,
                                  uint32_t* counts) {
  if (!rec_filt_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, k)) return -1;
  return rec_filtered_host(self, n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, k, ids, scores, counts,
                           false, SimArgs{});
}

int smatrix_cf_recommend_sim_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                 const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                 const uint32_t* d_deny_bits, uint64_t deny_n, int sim, double shrink, uint32_t k, uint32_t* d_ids,
                                 double* d_scores, uint32_t* d_counts, void* hip_stream) {
  if (!sim_args_ok(sim, shrink) || !rec_filt_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, k)) return -1;
  return rec_filtered_dev(self, n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, k, d_ids,
                          d_scores, d_counts, hip_stream, !sim_is_plain_cosine(sim, shrink), SimArgs{sim, shrink});
}

int smatrix_cf_recommend_sim(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                             const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, int sim,
                             double shrink, uint32_t k, uint32_t* ids, double* scores, uint32_t* counts) {
  if (!sim_args_ok(sim, shrink) || !rec_filt_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, k)) return -1;
  return rec_filtered_host(self, n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, k, ids, scores, counts,
                           !sim_is_plain_cosine(sim, shrink), SimArgs{sim, shrink});
}

int smatrix_cf_rank_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items, const double* d_weights,
                        const uint64_t* d_ex_offsets, const uint32_t* d_ex_items, const uint32_t* d_deny_bits, uint64_t deny_n, int sim,
                        double shrink, const uint64_t* d_t_offsets, const uint32_t* d_targets, uint32_t* d_ranks, double* d_scores,
                        uint32_t* d_n_candidates, void* hip_stream) {
  if (!rec_rank_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink, d_t_offsets, d_targets)) return -1;
  return rec_rank_dev(self, n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n,
                      !sim_is_plain_cosine(sim, shrink), SimArgs{sim, shrink}, RecRank{d_t_offsets, d_targets, d_ranks, d_scores},
                      d_n_candidates, hip_stream);
}

int smatrix_cf_rank(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                    const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, int sim,
                    double shrink, const uint64_t* t_offsets, const uint32_t* targets, uint32_t* ranks, double* scores,
                    uint32_t* n_candidates) {
  if (!rec_rank_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink, t_offsets, targets)) return -1;
  return rec_rank_host(self, n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n,
                       !sim_is_plain_cosine(sim, shrink), SimArgs{sim, shrink}, t_offsets, targets, ranks, scores, n_candidates);
}

}  // extern "C"
