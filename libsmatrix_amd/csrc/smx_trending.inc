// smx_trending.inc -- the trending items (include/smatrix_batch.h smatrix_cf_trending / _dev), host side.  Included by
// smx_runtime.hip inside the translation unit, after smx_popular.inc (sel_run, pop_args_ok and its RecCall with stage_filter; the
// scratch is RecScratch's sel_*); the device code is kernels/trending.hpp.
//
// trend_call is both flavours: a RecCall on `now` (its lock, its mirror written back, the scratch behind the previous read-path
// call's work, the synchronisation rule and the trim at finish) with base's lock taken in address order around it -- mg_merge's
// rule -- and base's mirror written back.  Inside it trend_run enqueues, with no read-back anywhere, k_trend_keys, the dense select
// (sel_run) and k_trend_sort.
// Scratch: 12 bytes per slot of now's directory (the keys, three planes of words), 12 n bytes (the keys collected), SelCtl.
// The host flavour stages the bitmap and copies the answers back.

namespace {

typedef RkCosine TrendKey;

struct TrendOut {
  uint32_t* ids;
  double* scores;
  uint32_t *totals, *expected, *n_found;
};

void trend_run(Matrix* m, RecScratch& x, hipStream_t s, const RecFilt& f, const TrendArgs& t, uint32_t n, const TrendOut& o) {
  const uint32_t slots = m->dir_size;
  const uint32_t* out = sel_run<TrendKey>(x, s, slots, n, [&](uint32_t grid, uint32_t* keys, SelCtl<TrendKey>* ctl) {
    hipLaunchKernelGGL(k_trend_keys, dim3(grid), dim3(256), 0, s, m->d_dir, slots, m->arena.base, f, t, keys, ctl);
  });
  hipLaunchKernelGGL(k_trend_sort, dim3(1), dim3(POP_SORT_THREADS), 0, s, sel_ctl<TrendKey>(x), n, out, m->d_dir, slots - 1, m->arena.base, t,
                     o.ids, o.scores, o.totals, o.expected, o.n_found);
  HIP_OK(hipGetLastError());
}

// what both flavours refuse before any lock or device call
bool trend_args_ok(smatrix_t* now, smatrix_t* base, int measure, uint32_t num, uint32_t den, double shrink, const void* deny_bits,
                   uint64_t deny_n, uint32_t n, const TrendOut& o) {
  if (!pop_args_ok(deny_bits, deny_n, n, o.ids, o.totals, o.n_found) || !o.scores || !o.expected) return false;
  if (!now || !base || base == now || M(base) == M(now) || M(base)->device != M(now)->device) return false;
  if (num == 0 || den == 0 || num > den) return false;
  if (measure != TREND_GAIN && measure != TREND_RATIO && measure != TREND_ZSCORE) return false;
  return shrink >= 0.0 && std::isfinite(shrink);                      // (-0.0 passes, NaN fails)
}

// The call, for both flavours.  `stage(c)` -> the RecFilt and the outputs on the device; `back(c, o)` enqueues what follows the kernels.
template <typename Stage, typename Back>
int trend_call(smatrix_t* now, smatrix_t* base, bool host, void* hip_stream, int measure, uint32_t num, uint32_t den, double shrink,
               uint32_t min_total, uint32_t min_gain, uint32_t n, Stage stage, Back back) {
  Matrix *a = M(now), *b = M(base);
  // both matrix locks, lower address first, as mg_merge takes them: this call and a merge of the same two matrices cannot wait for
  // each other.  The RecCall takes now's; base's goes in front of it or behind it.
  std::unique_lock<std::mutex> lb(b->mu, std::defer_lock);
  if (b < a) lb.lock();
  RecCall c(now, host, hip_stream);
  if (!lb.owns_lock()) lb.lock();
  cache_sync(b, false);
  RecFilt f{};
  TrendOut o{};
  stage(c, f, o);
  const TrendArgs t{b->d_dir, b->dir_size - 1, b->arena.base, measure, num, den, shrink, min_total, min_gain};
  trend_run(c.m, c.x(), c.s, f, t, n, o);
  back(c, o);
  return c.finish(0);
}

}  // namespace

extern "C" {

int smatrix_cf_trending_dev(smatrix_t* now, smatrix_t* base, int measure, uint32_t num, uint32_t den, double shrink,
                            const uint32_t* d_deny_bits, uint64_t deny_n, uint32_t min_total, uint32_t min_gain, uint32_t n,
                            uint32_t* d_ids, double* d_scores, uint32_t* d_totals, uint32_t* d_expected, uint32_t* d_n_found,
                            void* hip_stream) {
  const TrendOut out{d_ids, d_scores, d_totals, d_expected, d_n_found};
  if (!trend_args_ok(now, base, measure, num, den, shrink, d_deny_bits, deny_n, n, out)) return -1;
  return trend_call(now, base, false, hip_stream, measure, num, den, shrink, min_total, min_gain, n,
                    [&](RecCall&, RecFilt& f, TrendOut& o) { f.deny = d_deny_bits; f.deny_n = deny_n; o = out; },
                    [](RecCall&, const TrendOut&) {});
}

int smatrix_cf_trending(smatrix_t* now, smatrix_t* base, int measure, uint32_t num, uint32_t den, double shrink,
                        const uint32_t* deny_bits, uint64_t deny_n, uint32_t min_total, uint32_t min_gain, uint32_t n,
                        uint32_t* ids, double* scores, uint32_t* totals, uint32_t* expected, uint32_t* n_found) {
  const TrendOut out{ids, scores, totals, expected, n_found};
  if (!trend_args_ok(now, base, measure, num, den, shrink, deny_bits, deny_n, n, out)) return -1;
  return trend_call(now, base, true, nullptr, measure, num, den, shrink, min_total, min_gain, n,
                    [&](RecCall& c, RecFilt& f, TrendOut& o) {
                      RecScratch& x = c.x();
                      const uint64_t none[1] = {0};                   // (no sessions: the stager carries the bitmap alone)
                      f = c.stage_filter(0, none, nullptr, nullptr, nullptr, deny_bits, deny_n, SimArgs{});
                      x.h_ids.need(n); x.h_scores.need(n); x.h_counts.need(n); x.h_ranks.need(n); x.h_nsc.need(1);
                      o = TrendOut{x.h_ids.p, x.h_scores.p, x.h_counts.p, x.h_ranks.p, x.h_nsc.p};   // (expected: the rank call's u32 buffer)
                      HIP_OK(hipMemsetAsync(o.ids, 0, (size_t)n * 4, c.s));                          // unused entries read 0
                      HIP_OK(hipMemsetAsync(o.scores, 0, (size_t)n * 8, c.s));
                      HIP_OK(hipMemsetAsync(o.totals, 0, (size_t)n * 4, c.s));
                      HIP_OK(hipMemsetAsync(o.expected, 0, (size_t)n * 4, c.s));
                    },
                    [&](RecCall& c, const TrendOut& o) {
                      HIP_OK(hipMemcpyAsync(ids, o.ids, (size_t)n * 4, hipMemcpyDeviceToHost, c.s));
                      HIP_OK(hipMemcpyAsync(scores, o.scores, (size_t)n * 8, hipMemcpyDeviceToHost, c.s));
                      HIP_OK(hipMemcpyAsync(totals, o.totals, (size_t)n * 4, hipMemcpyDeviceToHost, c.s));
                      HIP_OK(hipMemcpyAsync(expected, o.expected, (size_t)n * 4, hipMemcpyDeviceToHost, c.s));
                      HIP_OK(hipMemcpyAsync(n_found, o.n_found, 4, hipMemcpyDeviceToHost, c.s));
                    });
}

}  // extern "C"
