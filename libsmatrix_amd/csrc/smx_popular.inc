// smx_popular.inc -- the most popular items (include/smatrix_batch.h smatrix_cf_popular / _dev), host side.  Included by
// smx_runtime.hip inside the translation unit, after smx_recommend.inc (uses its RecScratch and its call scope RecCall with
// stage_filter: the deny bitmap is the filtered call's); the device code is kernels/popular.hpp.
//
// Inside a RecCall (the matrix lock, the scalar mirror written back, behind the previous read-path call's work; its finish applies
// the recommend calls' synchronisation rule and trim), pop_run enqueues, with no read-back anywhere, k_pop_keys, the dense select
// of kernels/select.hpp (sel_run, here because the trending call enqueues the same) and k_pop_sort.  Scratch: RecScratch's sel_*,
// 8 bytes per directory slot (the keys), 8 n bytes (the keys collected), SelCtl.  The host flavour stages the bitmap and copies
// the answers back.

namespace {

template <typename P>
SelCtl<P>* sel_ctl(RecScratch& x) { return reinterpret_cast<SelCtl<P>*>(x.sel_ctl.p); }

// The select over a key of type P per directory slot, from the key kernel to the collection: sizes the scratch, zeroes SelCtl<P>,
// launch_keys(grid, keys, ctl), then k_sel_start, P::DIGITS times (k_sel_hist, k_sel_pick) -- a pass behind the one that finished
// the select returns at its first load -- and k_sel_collect.  -> the min(n, candidates) keys collected (their number: SelCtl::n_out).
template <typename P, typename Keys>
const uint32_t* sel_run(RecScratch& x, hipStream_t s, uint32_t slots, uint32_t n, Keys launch_keys) {
  const uint32_t grid = std::min<uint32_t>(blocks_for(slots), POP_GRID_MAX);
  x.sel_ctl.need(sizeof(SelCtl<P>) / 4); x.sel_keys.need((size_t)slots * P::W); x.sel_out.need((size_t)n * P::W);
  SelCtl<P>* ctl = sel_ctl<P>(x);
  HIP_OK(hipMemsetAsync(ctl, 0, sizeof(SelCtl<P>), s));
  launch_keys(grid, x.sel_keys.p, ctl);
  hipLaunchKernelGGL(k_sel_start<P>, dim3(1), dim3(64), 0, s, ctl, n);
  for (uint32_t pass = 0; pass < P::DIGITS; pass++) {
    hipLaunchKernelGGL(k_sel_hist<P>, dim3(grid), dim3(256), 0, s, x.sel_keys.p, slots, ctl, pass);
    hipLaunchKernelGGL(k_sel_pick<P>, dim3(1), dim3(64), 0, s, ctl, pass);
  }
  hipLaunchKernelGGL(k_sel_collect<P>, dim3(grid), dim3(256), 0, s, x.sel_keys.p, slots, ctl, n, x.sel_out.p);
  return x.sel_out.p;
}

void pop_run(Matrix* m, RecScratch& x, hipStream_t s, const RecFilt& f, uint32_t min_total, uint32_t n, uint32_t* d_ids, uint32_t* d_totals,
             uint32_t* d_n_found) {
  const uint32_t* out = sel_run<RkValue>(x, s, m->dir_size, n, [&](uint32_t grid, uint32_t* keys, SelCtl<RkValue>* ctl) {
    hipLaunchKernelGGL(k_pop_keys, dim3(grid), dim3(256), 0, s, m->d_dir, m->dir_size, m->arena.base, f, min_total, keys, ctl);
  });
  hipLaunchKernelGGL(k_pop_sort, dim3(1), dim3(POP_SORT_THREADS), 0, s, sel_ctl<RkValue>(x), n, out, d_ids, d_totals, d_n_found);
  HIP_OK(hipGetLastError());
}

// what both flavours refuse before anything else
bool pop_args_ok(const void* deny_bits, uint64_t deny_n, uint32_t n, const void* ids, const void* totals, const void* n_found) {
  return n != 0 && n <= POP_MAX && deny_n <= (1ull << 32) && (deny_bits || deny_n == 0) && ids && totals && n_found;
}

}  // namespace

extern "C" {

int smatrix_cf_popular_dev(smatrix_t* self, const uint32_t* d_deny_bits, uint64_t deny_n, uint32_t min_total, uint32_t n, uint32_t* d_ids,
                           uint32_t* d_totals, uint32_t* d_n_found, void* hip_stream) {
  if (!pop_args_ok(d_deny_bits, deny_n, n, d_ids, d_totals, d_n_found)) return -1;
  RecCall c(self, hip_stream);
  RecFilt f{};
  f.deny = d_deny_bits; f.deny_n = deny_n;
  pop_run(c.m, c.x(), c.s, f, min_total, n, d_ids, d_totals, d_n_found);
  return c.finish(0);
}

int smatrix_cf_popular(smatrix_t* self, const uint32_t* deny_bits, uint64_t deny_n, uint32_t min_total, uint32_t n, uint32_t* ids,
                       uint32_t* totals, uint32_t* n_found) {
  if (!pop_args_ok(deny_bits, deny_n, n, ids, totals, n_found)) return -1;
  RecCall c(self);
  RecScratch& x = c.x();
  const uint64_t none[1] = {0};                           // (no sessions: the stager carries the bitmap alone)
  const RecFilt f = c.stage_filter(0, none, nullptr, nullptr, nullptr, deny_bits, deny_n, SimArgs{});
  x.h_ids.need(n); x.h_counts.need(n); x.h_nsc.need(1);
  HIP_OK(hipMemsetAsync(x.h_ids.p, 0, (size_t)n * 4, c.s));           // unused entries read 0
  HIP_OK(hipMemsetAsync(x.h_counts.p, 0, (size_t)n * 4, c.s));
  pop_run(c.m, x, c.s, f, min_total, n, x.h_ids.p, x.h_counts.p, x.h_nsc.p);
  HIP_OK(hipMemcpyAsync(ids, x.h_ids.p, (size_t)n * 4, hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipMemcpyAsync(totals, x.h_counts.p, (size_t)n * 4, hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipMemcpyAsync(n_found, x.h_nsc.p, 4, hipMemcpyDeviceToHost, c.s));
  return c.finish(0);
}

}  // extern "C"
