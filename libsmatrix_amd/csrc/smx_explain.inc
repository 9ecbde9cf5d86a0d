// smx_explain.inc -- each session item's share of a candidate's score (include/smatrix_batch.h smatrix_cf_explain / _dev), host
// side.  Included by smx_runtime.hip inside the translation unit, after smx_recommend.inc (uses its RecScratch, its call scope
// RecCall with the stagers and the host weight check, and sim_args_ok of smx_merge.inc); the device code is kernels/explain.hpp.
//
// Inside a RecCall (the matrix lock, the scalar mirror written back, behind the previous read-path call's work; its finish
// applies the same synchronisation rule and trim as the recommend calls'), exp_run:
//   1. k_exp_prep_items (first positions, the rows' doubles, the weights' check) and k_exp_prep_targets (the targets' doubles)
//   2. ONE 4-byte read-back: a bad weight ends the call here
//   3. k_exp_terms, a lane per output entry
// The host flavour stages sessions, targets and weights with the scope's stagers and the entry offsets it computes itself.
// The _dev flavour does not know how long items and targets are: it reads d_offsets[n] and d_t_offsets[n] back first (16 bytes),
// inside the scope, to size the two scratch arrays.  No session table and no tier: nothing of rec_run is used.

namespace {

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
  RecCall c(self, hip_stream);
  uint64_t n_items = 0, n_t = 0;                          // what the scratch must hold: the offsets' last entries
  HIP_OK(hipMemcpyAsync(&n_items, d_offsets + n_sessions, 8, hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipMemcpyAsync(&n_t, d_t_offsets + n_sessions, 8, hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipStreamSynchronize(c.s));
  return c.finish(exp_run(c.m, c.x(), c.s, (uint32_t)n_sessions, d_offsets, d_items, d_weights, SimArgs{sim, shrink}, d_t_offsets,
                          d_targets, d_e_offsets, total, n_items, n_t, d_terms, d_cc));
}

int smatrix_cf_explain(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                       int sim, double shrink, const uint64_t* t_offsets, const uint32_t* targets, double* terms, uint32_t* cc) {
  if (!exp_args_ok(n_sessions, sim, shrink, t_offsets, targets, terms, cc)) return -1;
  if (n_sessions == 0) return 0;
  const uint64_t n = n_sessions;
  if (!rec_host_weights_ok(weights, offsets, n)) return -1;
  std::vector<uint64_t> e_rel(n + 1);                     // session s's entries start at the sum of targets * length before it
  e_rel[0] = 0;
  for (uint64_t i = 0; i < n; i++) e_rel[i + 1] = e_rel[i] + (t_offsets[i + 1] - t_offsets[i]) * (offsets[i + 1] - offsets[i]);
  const uint64_t total = e_rel[n];
  RecCall c(self);
  RecScratch& x = c.x();
  const RecList q = c.stage(n, offsets, items, x.h_off, x.h_items), t = c.stage(n, t_offsets, targets, x.h_toff, x.h_tg);
  const double* d_w = c.stage_weights(weights, offsets[0], q.count);
  x.h_eoff.need(n + 1); x.h_scores.need(std::max<uint64_t>(total, 1)); x.h_ids.need(std::max<uint64_t>(total, 1));
  HIP_OK(hipMemcpyAsync(x.h_eoff.p, e_rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, c.s));
  exp_run(c.m, x, c.s, (uint32_t)n, q.off, q.val, d_w, SimArgs{sim, shrink}, t.off, t.val, x.h_eoff.p, total, q.count, t.count,
          x.h_scores.p, x.h_ids.p);                       // (the weights were checked here: its result says nothing)
  if (total) HIP_OK(hipMemcpyAsync(terms, x.h_scores.p, total * 8, hipMemcpyDeviceToHost, c.s));
  if (total) HIP_OK(hipMemcpyAsync(cc, x.h_ids.p, total * 4, hipMemcpyDeviceToHost, c.s));
  return c.finish(0);
}

}  // extern "C"
