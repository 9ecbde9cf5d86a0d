// smx_explain.inc -- each session item's share of a candidate's score (include/smatrix_batch.h smatrix_cf_explain / _dev), host
// side.  Included by smx_runtime.hip inside the translation unit, after smx_recommend.inc (uses its RecScratch, rec_begin /
// rec_end, rec_trim_all, and sim_args_ok of smx_merge.inc); the device code is kernels/explain.hpp.
//
// Under the matrix lock, after the scalar mirror has been written back (cache_sync), behind the previous read-path call's work:
//   1. k_exp_prep_items (first positions, the rows' doubles, the weights' check) and k_exp_prep_targets (the targets' doubles)
//   2. ONE 4-byte read-back: a bad weight ends the call here
//   3. k_exp_terms, a lane per output entry
// The _dev flavour does not know how long items and targets are: it reads d_offsets[n] and d_t_offsets[n] back first (16 bytes)
// to size the two scratch arrays.  No session table and no tier: nothing of rec_run is used.

namespace {

bool exp_big(const RecScratch& x) { return rec_big(x.e_ra) || rec_big(x.e_cb); }

// the whole call on stream s, every array on the device; n >= 1, n_items / n_t = off[n] / t_off[n] (the entries of items and of
// targets the offsets can name).  Returns with k_exp_terms enqueued; -1 (the outputs are not written) for a bad weight.
int exp_run(Matrix* m, RecScratch& x, hipStream_t s, uint32_t n, const uint64_t* d_off, const uint32_t* d_items, const double* d_w,
            SimArgs f_m, const uint64_t* d_toff, const uint32_t* d_tg, const uint64_t* d_eoff, uint64_t total, uint64_t n_items,
            uint64_t n_t, double* d_terms, uint32_t* d_cc) {
  DirSlot* dir = m->d_dir;
  const uint32_t dmask = m->dir_size - 1;
  x.ctl.need(1); x.e_ra.need(std::max<uint64_t>(n_items, 1)); x.e_cb.need(std::max<uint64_t>(n_t, 1));
  HIP_OK(hipMemsetAsync(x.ctl.p, 0, sizeof(RecCtl), s));
  hipLaunchKernelGGL(k_exp_prep_items, dim3(std::min<uint32_t>(blocks_for((uint64_t)n * 64), 16384)), dim3(256), 0, s, dir, dmask,
                     m->arena.base, n, d_off, d_items, d_w, f_m.sim, x.e_ra.p, &x.ctl.p->bad);
  if (n_t && total)
    hipLaunchKernelGGL(k_exp_prep_targets, dim3((uint32_t)std::min<uint64_t>((n_t + 255) / 256, 16384)), dim3(256), 0, s, dir, dmask,
                       m->arena.base, n_t, d_tg, f_m.sim, x.e_cb.p);
  HIP_OK(hipGetLastError());
  uint32_t bad = 0;
  if (d_w) {
    HIP_OK(hipMemcpyAsync(&bad, &x.ctl.p->bad, 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
  }
  if (bad) return -1;
  if (!total) return 0;
  const ExpArgs a{d_off, d_items, d_w, d_toff, d_tg, d_eoff, x.e_ra.p, x.e_cb.p, n, f_m};
  hipLaunchKernelGGL(k_exp_terms, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 1u << 20)), dim3(256), 0, s, dir, dmask,
                     m->arena.base, a, total, d_terms, d_cc);
  HIP_OK(hipGetLastError());
  return 0;
}

// what both flavours refuse before anything else
bool exp_args_ok(size_t n_sessions, int sim, double shrink, const void* t_offsets, const void* targets, const void* terms,
                 const void* cc) {
  return n_sessions <= 0xffffffffull && sim_args_ok(sim, shrink) && t_offsets && targets && terms && cc;
}

}  // namespace

extern "C" {

int smatrix_cf_explain_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                           const double* d_weights, int sim, double shrink, const uint64_t* d_t_offsets, const uint32_t* d_targets,
                           const uint64_t* d_e_offsets, uint64_t total, double* d_terms, uint32_t* d_cc, void* hip_stream) {
  if (!exp_args_ok(n_sessions, sim, shrink, d_t_offsets, d_targets, d_terms, d_cc) || !d_e_offsets) return -1;
  if (n_sessions == 0) return 0;
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
  RecScratch& x = rec_of(m);
  rec_begin(x, s);
  uint64_t n_items = 0, n_t = 0;                          // what the scratch must hold: the offsets' last entries
  HIP_OK(hipMemcpyAsync(&n_items, d_offsets + n_sessions, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&n_t, d_t_offsets + n_sessions, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  const int rc = exp_run(m, x, s, (uint32_t)n_sessions, d_offsets, d_items, d_weights, SimArgs{sim, shrink}, d_t_offsets, d_targets,
                         d_e_offsets, total, n_items, n_t, d_terms, d_cc);
  rec_end(x, s);
  if (!hip_stream || exp_big(x)) HIP_OK(hipStreamSynchronize(s));   // (the kernels use the buffers rec_trim_all releases)
  rec_trim_all(x, false);
  return rc;
}

int smatrix_cf_explain(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                       int sim, double shrink, const uint64_t* t_offsets, const uint32_t* targets, double* terms, uint32_t* cc) {
  if (!exp_args_ok(n_sessions, sim, shrink, t_offsets, targets, terms, cc)) return -1;
  if (n_sessions == 0) return 0;
  const uint64_t n = n_sessions, n_items = offsets[n] - offsets[0], n_t = t_offsets[n] - t_offsets[0];
  if (weights)
    for (uint64_t i = 0; i < n_items; i++)
      if (!(weights[offsets[0] + i] >= 0.0) || !std::isfinite(weights[offsets[0] + i])) return -1;   // (before the device is touched)
  std::vector<uint64_t> rel(n + 1), t_rel(n + 1), e_rel(n + 1);
  e_rel[0] = 0;
  for (uint64_t i = 0; i <= n; i++) { rel[i] = offsets[i] - offsets[0]; t_rel[i] = t_offsets[i] - t_offsets[0]; }
  for (uint64_t i = 0; i < n; i++) e_rel[i + 1] = e_rel[i] + (t_rel[i + 1] - t_rel[i]) * (rel[i + 1] - rel[i]);
  const uint64_t total = e_rel[n];
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = m->stream;
  RecScratch& x = rec_of(m);
  rec_begin(x, s);
  x.h_off.need(n + 1); x.h_toff.need(n + 1); x.h_eoff.need(n + 1);
  x.h_items.need(std::max<uint64_t>(n_items, 1)); x.h_tg.need(std::max<uint64_t>(n_t, 1));
  x.h_scores.need(std::max<uint64_t>(total, 1)); x.h_ids.need(std::max<uint64_t>(total, 1));
  HIP_OK(hipMemcpyAsync(x.h_off.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(x.h_toff.p, t_rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(x.h_eoff.p, e_rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_items) HIP_OK(hipMemcpyAsync(x.h_items.p, items + offsets[0], n_items * 4, hipMemcpyHostToDevice, s));
  if (n_t) HIP_OK(hipMemcpyAsync(x.h_tg.p, targets + t_offsets[0], n_t * 4, hipMemcpyHostToDevice, s));
  const double* d_w = nullptr;
  if (weights) {
    x.h_w.need(std::max<uint64_t>(n_items, 1));
    if (n_items) HIP_OK(hipMemcpyAsync(x.h_w.p, weights + offsets[0], n_items * 8, hipMemcpyHostToDevice, s));
    d_w = x.h_w.p;
  }
  exp_run(m, x, s, (uint32_t)n, x.h_off.p, x.h_items.p, d_w, SimArgs{sim, shrink}, x.h_toff.p, x.h_tg.p, x.h_eoff.p, total, n_items, n_t,
          x.h_scores.p, x.h_ids.p);
  if (total) HIP_OK(hipMemcpyAsync(terms, x.h_scores.p, total * 8, hipMemcpyDeviceToHost, s));
  if (total) HIP_OK(hipMemcpyAsync(cc, x.h_ids.p, total * 4, hipMemcpyDeviceToHost, s));
  rec_end(x, s);
  HIP_OK(hipStreamSynchronize(s));
  rec_trim_all(x, false);
  return 0;
}

}  // extern "C"
