// smx_recommend.inc -- session recommendations (include/smatrix_batch.h smatrix_cf_recommend_batch / _dev,
// smatrix_cf_recommend_filtered / _dev, smatrix_cf_recommend_sim / _dev, smatrix_cf_recommend_grouped / _dev,
// smatrix_cf_recommend_deep / _dev and smatrix_cf_rank / _dev), host side.
// Included by smx_runtime.hip inside the translation unit, after smx_export.inc (uses Matrix, DevBuf, HIP_OK, and the export's
// u32 -> u64 scan kernels); the device code is kernels/recommend.hpp.
//
// Three layers, top down:
//   the extern "C" symbols   refuse bad arguments, then name what the call was given: a RecFilt, a measure, a RecRank
//   RecCall                  ONE scope for every call on the read path's scratch (the files included behind this one as well: the
//                            item-neighbour calls' host flavours, the explain call, both imports, the popular call): the matrix lock,
//                            the scalar mirror written back (cache_sync), the stream, the wait for the call before, and at finish
//                            the event, the synchronisation rule and the trim.  Its stagers carry a host flavour's arrays to the
//                            device: stage (a window of a list of lists: sessions, exclusion lists, targets), stage_weights,
//                            stage_filter.  A _dev flavour is the scope around the driver; a host flavour stages, runs, copies back
//   rec_run<F, S, R>         the driver, every array on the device:
//     1. k_rec_bound sorts the sessions into the LDS tier and the global tier; ONE read-back of RecCtl (counts, global-tier sizes)
//     2. k_rec_lds: every LDS-tier session, one workgroup each
//     3. the global tier, per group of sessions whose tables fit REC_GROUP_SLOTS (normally one group): zeroed tables, k_rec_gl_init,
//        per block of item positions the chunk counts (k_rec_gl_plan) and their scan, a k_rec_gl_scan launch per position (the
//        kernel boundary keeps the items in session order), k_rec_gl_topk, k_rec_gl_merge
// The filtered call runs the kernels' <true> instances for its RecFilt (weights, exclusion lists, deny bitmap); with nothing given
// it runs the <false> ones, and that is what smatrix_cf_recommend_batch is: the filtered call with nothing given.
// The sim call is the filtered call with a measure and a shrinkage in the RecFilt and, for the two kernels that make a score,
// their _sim instances; with SMATRIX_SIM_COSINE and shrink 0 it IS the filtered call.
// The rank call is the sim call with another ending (rec_run<.., .., true>): the answers are filled with "no answer", k_rec_lds_rank
// stands for k_rec_lds, and k_rec_gl_rank for k_rec_gl_topk + k_rec_gl_merge; everything before the ending is shared.
// The fill call (smatrix_cf_recommend_fill / _dev) is the sim call with ONE launch behind the driver's, rec_fill: k_rec_fill reads
// the ids and counts both tiers wrote, notes them as n_scored and fills the free places from the caller's list (RecFill).
// The grouped call (smatrix_cf_recommend_grouped / _dev) is the sim call with a third ending (rec_run<.., .., false, true>, RecGroup):
// k_rec_lds_grouped stands for k_rec_lds, and k_rec_gl_grouped for k_rec_gl_topk + k_rec_gl_merge.  With no map, or a quota that
// cannot bind (cap >= k), it IS the sim call.
// The deep call (smatrix_cf_recommend_deep / _dev) is the sim call with k up to SMATRIX_DEEP_MAX and, above 64, a fourth ending
// (rec_run<.., .., false, false, true>): k_rec_lds_deep stands for k_rec_lds, and k_rec_gl_deep for k_rec_gl_topk + k_rec_gl_merge (lk / li
// are not allocated).  With k <= 64 it IS the sim call.

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
  DevBuf<uint32_t> h_amt, i_cnt;                     // ... and the event import's (smx_import.inc): amounts, the chunk's op counter,
  DevBuf<uint64_t> i_soff, i_part;                   // the slots before every session and before every tile of sessions
  DevBuf<uint64_t> h_opoff;                          // ... and the old import's: the ops before every session
  DevBuf<uint64_t> h_foff;                           // ... and the fill call's: the staged list (one list: two offsets), n_scored
  DevBuf<uint32_t> h_fill, h_nsc;
  DevBuf<uint32_t> h_grp;                            // ... and the grouped call's: the group of every id
  DevBuf<PopCtl> p_ctl;                              // ... and the popular call's (smx_popular.inc): the select's state, a key per
  DevBuf<unsigned long long> p_keys, p_out;          // directory slot, the n keys collected (ids: h_ids, totals: h_counts, n: h_nsc)
  hipEvent_t done = nullptr;                         // recorded behind the last call's work (its stream may be any)
  // EVERY buffer above, and the only list of them: the trim, the "any buffer big" test and the release are this visitor's
  template <typename Fn>
  void for_each_buf(Fn f) {
    f(ctl); f(lds_list); f(big_list); f(gk); f(owner); f(zpos); f(cnt); f(li); f(big_off); f(tlg); f(gq); f(gs); f(lk); f(scan); f(part);
    f(h_items); f(h_ids); f(h_counts); f(h_off); f(h_scores); f(h_w); f(h_exoff); f(h_ex); f(h_deny); f(h_toff); f(h_tg); f(h_ranks);
    f(h_eoff); f(e_ra); f(e_cb); f(h_amt); f(i_cnt); f(i_soff); f(i_part); f(h_opoff); f(h_foff); f(h_fill); f(h_nsc); f(h_grp); f(p_ctl); f(p_keys); f(p_out);
  }
};

RecScratch& rec_of(Matrix* m) {
  if (!m->rec) m->rec = new RecScratch();
  return *static_cast<RecScratch*>(m->rec);
}

template <typename T>
bool rec_big(const DevBuf<T>& b) { return b.cap * sizeof(T) > ((size_t)64 << 20); }
void rec_trim_all(RecScratch& x, bool all) {
  x.for_each_buf([all](auto& b) { if (all || rec_big(b)) b.release(); });   // (as the export: no HBM pinned for good)
}
bool rec_any_big(RecScratch& x) {
  bool big = false;
  x.for_each_buf([&big](auto& b) { big = big || rec_big(b); });
  return big;
}

// a window of a caller's list of lists on the device: offsets that start at 0, the values they name, and how many those are
struct RecList {
  const uint64_t* off;
  const uint32_t* val;
  uint64_t count;
};

// One call on the read path's scratch, from the lock to the trim; every entry point opens one behind its refusals.
// The scratch is the matrix's, the stream the caller's: a call on another stream than the one before it (or a host flavour, on
// the matrix's stream) must not touch the scratch while kernels of the earlier call may still read it -- hence `done`.
struct RecCall {
  Matrix* const m;
  std::unique_lock<std::mutex> lock;
  hipStream_t s;
  RecScratch* scratch;
  const bool host;                                        // a host flavour: finish always synchronises
  std::vector<std::vector<uint64_t>> rel;                 // the offsets the copies in flight read: alive until finish

  explicit RecCall(smatrix_t* self) : RecCall(self, true, nullptr) {}                      // a host flavour: the matrix's stream
  RecCall(smatrix_t* self, void* hip_stream) : RecCall(self, false, hip_stream) {}         // a _dev flavour: NULL = the legacy default stream
  RecCall(smatrix_t* self, bool host_flavour, void* hip_stream) : m(M(self)), host(host_flavour) {
    set_device(m);
    lock = std::unique_lock<std::mutex>(m->mu);
    cache_sync(m, false);
    s = host ? m->stream : static_cast<hipStream_t>(hip_stream);
    scratch = &rec_of(m);
    if (scratch->done) HIP_OK(hipStreamWaitEvent(s, scratch->done, 0));
  }
  RecScratch& x() { return *scratch; }

  // The end of the call, whatever it returns.  The kernels use the buffers the trim releases, so a _dev call whose stream is the
  // caller's returns with its work in flight only when no buffer is above the threshold.  The test runs over ALL buffers: one
  // that is big now was grown by this call, because the call that made a buffer big before synchronised and released it here.
  int finish(int rc) {
    RecScratch& x = *scratch;
    if (!x.done) HIP_OK(hipEventCreateWithFlags(&x.done, hipEventDisableTiming));
    HIP_OK(hipEventRecord(x.done, s));
    if (host || !s || rec_any_big(x)) HIP_OK(hipStreamSynchronize(s));
    rec_trim_all(x, false);
    return rc;
  }

  // offsets[0 .. n] and values[offsets[0] .. offsets[n]) of the caller: zero-based offsets to d_off, the values to d_val (sized to
  // one element when there is none: no NULL goes to a kernel)
  RecList stage(uint64_t n, const uint64_t* offsets, const uint32_t* values, DevBuf<uint64_t>& d_off, DevBuf<uint32_t>& d_val) {
    rel.emplace_back(n + 1);
    std::vector<uint64_t>& r = rel.back();
    for (uint64_t i = 0; i <= n; i++) r[i] = offsets[i] - offsets[0];
    d_off.need(n + 1); d_val.need(std::max<uint64_t>(r[n], 1));
    HIP_OK(hipMemcpyAsync(d_off.p, r.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (r[n]) HIP_OK(hipMemcpyAsync(d_val.p, values + offsets[0], r[n] * 4, hipMemcpyHostToDevice, s));
    return RecList{d_off.p, d_val.p, r[n]};
  }
  // the weights of the staged sessions (they lie at the sessions' offsets), or NULL for none
  const double* stage_weights(const double* weights, uint64_t first, uint64_t n_items) {
    if (!weights) return nullptr;
    RecScratch& x = *scratch;
    x.h_w.need(std::max<uint64_t>(n_items, 1));
    if (n_items) HIP_OK(hipMemcpyAsync(x.h_w.p, weights + first, n_items * 8, hipMemcpyHostToDevice, s));
    return x.h_w.p;
  }
  // a host flavour's RecFilt: the weights, the exclusion lists and the deny bitmap, whichever were given
  RecFilt stage_filter(uint64_t n, const uint64_t* offsets, const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                       const uint32_t* deny_bits, uint64_t deny_n, SimArgs f_m) {
    RecScratch& x = *scratch;
    RecFilt f{};
    f.m = f_m;
    f.w = stage_weights(weights, offsets[0], offsets[n] - offsets[0]);
    if (ex_offsets) {
      const RecList ex = stage(n, ex_offsets, ex_items, x.h_exoff, x.h_ex);
      f.ex_off = ex.off; f.ex = ex.val;
    }
    if (deny_n) {
      const uint64_t n_deny = (deny_n + 31) / 32;
      x.h_deny.need(n_deny);
      HIP_OK(hipMemcpyAsync(x.h_deny.p, deny_bits, n_deny * 4, hipMemcpyHostToDevice, s));
      f.deny = x.h_deny.p; f.deny_n = deny_n;
    }
    return f;
  }
};

// a host flavour's weights, before the device is touched: the sessions' entries finite and >= 0 (the _dev flavours find a bad
// one on the device)
bool rec_host_weights_ok(const double* weights, const uint64_t* offsets, uint64_t n) {
  if (weights)
    for (uint64_t i = offsets[0]; i < offsets[n]; i++)
      if (!(weights[i] >= 0.0) || !std::isfinite(weights[i])) return false;
  return true;
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
// Q: the ending is the grouped call's (R is false): k_rec_lds_grouped stands for k_rec_lds, and k_rec_gl_grouped for k_rec_gl_topk +
// k_rec_gl_merge, over the map and the quota in gr
// D: the ending is the deep call's (R and Q are false; k may be up to SMATRIX_DEEP_MAX): k_rec_lds_deep stands for k_rec_lds, and
// k_rec_gl_deep for k_rec_gl_topk + k_rec_gl_merge
template <bool F, bool S, bool R, bool Q = false, bool D = false>
int rec_run(Matrix* m, RecScratch& x, hipStream_t s, uint32_t n, const uint64_t* d_off, const uint32_t* d_items, uint32_t k,
            uint32_t* d_ids, double* d_scores, uint32_t* d_counts, const RecFilt& f, const RecRank& rk, const RecGroup& gr = RecGroup{}) {
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
  else if (c.n_lds && Q)
    hipLaunchKernelGGL(S ? k_rec_lds_grouped_sim<F> : k_rec_lds_grouped<F>, dim3(std::min<uint32_t>(c.n_lds, 1u << 16)), dim3(REC_LDS_THREADS), 0, s, dir,
                       dmask, m->arena.base, x.ctl.p, x.lds_list.p, x.tlg.p, d_off, d_items, k, d_ids, d_scores, d_counts, f, gr);
  else if (c.n_lds && D)
    hipLaunchKernelGGL(S ? k_rec_lds_deep_sim<F> : k_rec_lds_deep<F>, dim3(std::min<uint32_t>(c.n_lds, 1u << 16)), dim3(REC_LDS_THREADS), 0, s, dir,
                       dmask, m->arena.base, x.ctl.p, x.lds_list.p, x.tlg.p, d_off, d_items, k, d_ids, d_scores, d_counts, f);
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
  if (!R && !Q && !D) { x.lk.need(nseg * 64); x.li.need(nseg * 64); }
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
    } else if (Q) {
      hipLaunchKernelGGL(k_rec_gl_grouped, dim3(std::min<uint32_t>(c.n_big, 1u << 16)), dim3(REC_MERGE_THREADS), 0, s, G, gr, k, d_ids, d_scores,
                         d_counts);
    } else if (D) {
      hipLaunchKernelGGL(k_rec_gl_deep, dim3(std::min<uint32_t>(c.n_big, 1u << 16)), dim3(REC_MERGE_THREADS), 0, s, G, k, d_ids, d_scores, d_counts);
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

// what both flavours of the plain call refuse, and of the filtered call before anything else
bool rec_k_ok(size_t n_sessions, uint32_t k) { return k != 0 && k <= 64 && n_sessions <= 0xffffffffull; }
bool rec_filt_args_ok(size_t n_sessions, const void* ex_offsets, const void* ex_items, const void* deny_bits, uint64_t deny_n,
                      uint32_t k) {
  if (!rec_k_ok(n_sessions, k)) return false;
  if (deny_n > (1ull << 32) || (!deny_bits && deny_n)) return false;
  return (ex_offsets == nullptr) == (ex_items == nullptr);
}
bool rec_filt_any(const RecFilt& f) { return f.w || f.ex_off || f.deny_n; }
// ... and the fill call on top of the sim call's
bool rec_fill_args_ok(const void* fill_ids, uint64_t n_fill, const void* n_scored) {
  return n_scored && n_fill < (1ull << 32) && (fill_ids || n_fill == 0);
}
// ... and the grouped call on top of the sim call's
bool rec_group_args_ok(const void* group_of, uint64_t group_n, uint32_t cap) {
  return cap != 0 && cap <= 64 && group_n <= (1ull << 32) && (group_of || group_n == 0);
}
// does the map change anything?  Without ids in it nobody is grouped, and a quota of k or more refuses nobody before the cut at k:
// both are the sim call, through its own launches
bool rec_group_binds(const RecGroup& gr, uint32_t k) { return gr.n != 0 && gr.cap < k; }
// what the deep call refuses in place of the sim call's k <= 64, and when its own ending runs: up to 64 results it IS the sim call
bool rec_deep_k_ok(uint32_t k) { return k != 0 && k <= SMATRIX_DEEP_MAX; }
bool rec_deep_binds(uint32_t k) { return k > 64; }
static_assert(SMATRIX_DEEP_MAX == REC_DEEP_MAX, "the list of kernels/recommend.hpp holds SMATRIX_DEEP_MAX entries");
// (the sim call refuses on top of them what sim_args_ok of smx_merge.inc refuses: shrink is a host scalar in both flavours)

// the kernels' instances for what the call was given: <false, .> with no filter, <., true> with a measure; R: the rank ending;
// gr: the grouped ending (never with R); deep: the deep ending (never with R or gr)
template <bool R>
int rec_dispatch(Matrix* m, RecScratch& x, hipStream_t s, uint32_t n, const uint64_t* d_off, const uint32_t* d_items, uint32_t k,
                 uint32_t* d_ids, double* d_scores, uint32_t* d_counts, const RecFilt& f, bool sim, const RecRank& rk,
                 const RecGroup* gr = nullptr, bool deep = false) {
  if constexpr (!R) {
    if (deep && sim) return rec_filt_any(f) ? rec_run<true, true, false, false, true>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk)
                                            : rec_run<false, true, false, false, true>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk);
    if (deep) return rec_filt_any(f) ? rec_run<true, false, false, false, true>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk)
                                     : rec_run<false, false, false, false, true>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk);
    if (gr && sim) return rec_filt_any(f) ? rec_run<true, true, false, true>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk, *gr)
                                          : rec_run<false, true, false, true>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk, *gr);
    if (gr) return rec_filt_any(f) ? rec_run<true, false, false, true>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk, *gr)
                                   : rec_run<false, false, false, true>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk, *gr);
  }
  if (sim) return rec_filt_any(f) ? rec_run<true, true, R>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk)
                                  : rec_run<false, true, R>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk);
  return rec_filt_any(f) ? rec_run<true, false, R>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk)
                         : rec_run<false, false, R>(m, x, s, n, d_off, d_items, k, d_ids, d_scores, d_counts, f, rk);
}

// what smatrix_cf_recommend_fill adds to the sim call: the caller's list and where the scored counts go, all on the device
struct RecFill {
  const uint32_t* ids;
  uint64_t n;
  uint32_t* n_scored;
};
// behind the recommend launches of both tiers, whatever they were: k_rec_fill, a wave per session
void rec_fill(hipStream_t s, uint32_t n, const uint64_t* d_off, const uint32_t* d_items, uint32_t k, const RecFill& fl, uint32_t* d_ids,
              double* d_scores, uint32_t* d_counts, const RecFilt& f) {
  hipLaunchKernelGGL(k_rec_fill, dim3(std::min<uint32_t>(blocks_for((uint64_t)n * 64), 16384)), dim3(256), 0, s, n, d_off, d_items, k, fl.ids,
                     (uint32_t)fl.n, d_ids, d_scores, d_counts, fl.n_scored, f);
  HIP_OK(hipGetLastError());
}

// every _dev flavour behind its refusals: the scope around the driver.  R: the rank call (k, d_ids, d_scores: none); sim: score by
// f.m, not by the cosine.  A bad weight is found on the device: -1 through the same finish.  fl: the fill call, its kernel behind
// the driver's; gr: the grouped call, its ending in place of the top-k; deep: the deep call with k > 64, its ending in that place
template <bool R>
int rec_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items, const RecFilt& f, bool sim, uint32_t k,
            uint32_t* d_ids, double* d_scores, uint32_t* d_counts, const RecRank& rk, void* hip_stream, const RecFill* fl = nullptr,
            const RecGroup* gr = nullptr, bool deep = false) {
  if (n_sessions == 0) return 0;
  RecCall c(self, hip_stream);
  const int rc = rec_dispatch<R>(c.m, c.x(), c.s, (uint32_t)n_sessions, d_offsets, d_items, k, d_ids, d_scores, d_counts, f, sim, rk, gr, deep);
  if (fl && rc == 0) rec_fill(c.s, (uint32_t)n_sessions, d_offsets, d_items, k, *fl, d_ids, d_scores, d_counts, f);
  return c.finish(rc);
}

// the host flavours of the plain, the filtered and the sim call (the weights were checked here: the driver's result says nothing);
// fl: the fill call, with the HOST's list and n_scored -- the list goes through the stager as a list of lists that holds one list;
// gr: the grouped call, with the HOST's map, staged once; deep: the deep call with k > 64 (n * k: 64-bit throughout)
int rec_filtered_host(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                      const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, uint32_t k,
                      uint32_t* ids, double* scores, uint32_t* counts, bool sim, SimArgs f_m, const RecFill* fl = nullptr,
                      const RecGroup* gr = nullptr, bool deep = false) {
  if (n_sessions == 0) return 0;
  const uint64_t n = n_sessions;
  if (!rec_host_weights_ok(weights, offsets, n)) return -1;
  RecCall c(self);
  RecScratch& x = c.x();
  const RecList q = c.stage(n, offsets, items, x.h_off, x.h_items);
  const RecFilt f = c.stage_filter(n, offsets, weights, ex_offsets, ex_items, deny_bits, deny_n, f_m);
  x.h_ids.need(n * k); x.h_scores.need(n * k); x.h_counts.need(n);
  HIP_OK(hipMemsetAsync(x.h_ids.p, 0, n * k * 4, c.s));              // unused entries read 0, as cf_topk_batch's
  HIP_OK(hipMemsetAsync(x.h_scores.p, 0, n * k * 8, c.s));
  RecGroup d_gr{};
  if (gr) {
    x.h_grp.need(gr->n);
    HIP_OK(hipMemcpyAsync(x.h_grp.p, gr->of, gr->n * 4, hipMemcpyHostToDevice, c.s));
    d_gr = RecGroup{x.h_grp.p, gr->n, gr->cap};
  }
  rec_dispatch<false>(c.m, x, c.s, (uint32_t)n, q.off, q.val, k, x.h_ids.p, x.h_scores.p, x.h_counts.p, f, sim, RecRank{}, gr ? &d_gr : nullptr, deep);
  if (fl) {
    const uint64_t one_list[2] = {0, fl->n};
    const RecList l = c.stage(1, one_list, fl->ids, x.h_foff, x.h_fill);
    x.h_nsc.need(n);
    rec_fill(c.s, (uint32_t)n, q.off, q.val, k, RecFill{l.val, l.count, x.h_nsc.p}, x.h_ids.p, x.h_scores.p, x.h_counts.p, f);
    HIP_OK(hipMemcpyAsync(fl->n_scored, x.h_nsc.p, n * 4, hipMemcpyDeviceToHost, c.s));
  }
  HIP_OK(hipMemcpyAsync(counts, x.h_counts.p, n * 4, hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipMemcpyAsync(ids, x.h_ids.p, n * k * 4, hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipMemcpyAsync(scores, x.h_scores.p, n * k * 8, hipMemcpyDeviceToHost, c.s));
  return c.finish(0);
}

// the rank call's: the same staging, and the target lists and the answers' [t_offsets[0], t_offsets[n]) beside it
int rec_rank_host(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                  const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, bool sim, SimArgs f_m,
                  const uint64_t* t_offsets, const uint32_t* targets, uint32_t* ranks, double* scores, uint32_t* n_candidates) {
  if (n_sessions == 0) return 0;
  const uint64_t n = n_sessions;
  if (!rec_host_weights_ok(weights, offsets, n)) return -1;
  RecCall c(self);
  RecScratch& x = c.x();
  const RecList q = c.stage(n, offsets, items, x.h_off, x.h_items), t = c.stage(n, t_offsets, targets, x.h_toff, x.h_tg);
  const RecFilt f = c.stage_filter(n, offsets, weights, ex_offsets, ex_items, deny_bits, deny_n, f_m);
  x.h_counts.need(n); x.h_ranks.need(std::max<uint64_t>(t.count, 1)); x.h_scores.need(std::max<uint64_t>(t.count, 1));
  rec_dispatch<true>(c.m, x, c.s, (uint32_t)n, q.off, q.val, 0u, nullptr, nullptr, x.h_counts.p, f, sim,
                     RecRank{t.off, t.val, x.h_ranks.p, x.h_scores.p});
  HIP_OK(hipMemcpyAsync(n_candidates, x.h_counts.p, n * 4, hipMemcpyDeviceToHost, c.s));
  if (t.count) HIP_OK(hipMemcpyAsync(ranks + t_offsets[0], x.h_ranks.p, t.count * 4, hipMemcpyDeviceToHost, c.s));
  if (t.count) HIP_OK(hipMemcpyAsync(scores + t_offsets[0], x.h_scores.p, t.count * 8, hipMemcpyDeviceToHost, c.s));
  return c.finish(0);
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
  if (!rec_k_ok(n_sessions, k)) return -1;
  return rec_dev<false>(self, n_sessions, d_offsets, d_items, RecFilt{}, false, k, d_ids, d_scores, d_counts, RecRank{}, hip_stream);
}

int smatrix_cf_recommend_batch(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, uint32_t k,
                               uint32_t* ids, double* scores, uint32_t* counts) {
  if (!rec_k_ok(n_sessions, k)) return -1;
  return rec_filtered_host(self, n_sessions, offsets, items, nullptr, nullptr, nullptr, nullptr, 0, k, ids, scores, counts, false, SimArgs{});
}

int smatrix_cf_recommend_filtered_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                      const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                      const uint32_t* d_deny_bits, uint64_t deny_n, uint32_t k, uint32_t* d_ids, double* d_scores,
                                      uint32_t* d_counts, void* hip_stream) {
  if (!rec_filt_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, k)) return -1;
  return rec_dev<false>(self, n_sessions, d_offsets, d_items, RecFilt{d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, SimArgs{}}, false,
                        k, d_ids, d_scores, d_counts, RecRank{}, hip_stream);
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
  return rec_dev<false>(self, n_sessions, d_offsets, d_items,
                        RecFilt{d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, SimArgs{sim, shrink}},
                        !sim_is_plain_cosine(sim, shrink), k, d_ids, d_scores, d_counts, RecRank{}, hip_stream);
}

int smatrix_cf_recommend_sim(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                             const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, int sim,
                             double shrink, uint32_t k, uint32_t* ids, double* scores, uint32_t* counts) {
  if (!sim_args_ok(sim, shrink) || !rec_filt_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, k)) return -1;
  return rec_filtered_host(self, n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, k, ids, scores, counts,
                           !sim_is_plain_cosine(sim, shrink), SimArgs{sim, shrink});
}

int smatrix_cf_recommend_fill_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                  const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                  const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_fill_ids, uint64_t n_fill, int sim,
                                  double shrink, uint32_t k, uint32_t* d_ids, double* d_scores, uint32_t* d_counts, uint32_t* d_n_scored,
                                  void* hip_stream) {
  if (!sim_args_ok(sim, shrink) || !rec_filt_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, k)) return -1;
  if (!rec_fill_args_ok(d_fill_ids, n_fill, d_n_scored)) return -1;
  const RecFill fl{d_fill_ids, n_fill, d_n_scored};
  return rec_dev<false>(self, n_sessions, d_offsets, d_items,
                        RecFilt{d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, SimArgs{sim, shrink}},
                        !sim_is_plain_cosine(sim, shrink), k, d_ids, d_scores, d_counts, RecRank{}, hip_stream, &fl);
}

int smatrix_cf_recommend_fill(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                              const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n,
                              const uint32_t* fill_ids, uint64_t n_fill, int sim, double shrink, uint32_t k, uint32_t* ids, double* scores,
                              uint32_t* counts, uint32_t* n_scored) {
  if (!sim_args_ok(sim, shrink) || !rec_filt_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, k)) return -1;
  if (!rec_fill_args_ok(fill_ids, n_fill, n_scored)) return -1;
  const RecFill fl{fill_ids, n_fill, n_scored};
  return rec_filtered_host(self, n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, k, ids, scores, counts,
                           !sim_is_plain_cosine(sim, shrink), SimArgs{sim, shrink}, &fl);
}

int smatrix_cf_recommend_grouped_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                     const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                     const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_group_of, uint64_t group_n, uint32_t cap,
                                     int sim, double shrink, uint32_t k, uint32_t* d_ids, double* d_scores, uint32_t* d_counts,
                                     void* hip_stream) {
  if (!sim_args_ok(sim, shrink) || !rec_filt_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, k)) return -1;
  if (!rec_group_args_ok(d_group_of, group_n, cap)) return -1;
  const RecGroup gr{d_group_of, group_n, cap};
  return rec_dev<false>(self, n_sessions, d_offsets, d_items,
                        RecFilt{d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, SimArgs{sim, shrink}},
                        !sim_is_plain_cosine(sim, shrink), k, d_ids, d_scores, d_counts, RecRank{}, hip_stream, nullptr,
                        rec_group_binds(gr, k) ? &gr : nullptr);
}

int smatrix_cf_recommend_grouped(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                                 const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n,
                                 const uint32_t* group_of, uint64_t group_n, uint32_t cap, int sim, double shrink, uint32_t k, uint32_t* ids,
                                 double* scores, uint32_t* counts) {
  if (!sim_args_ok(sim, shrink) || !rec_filt_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, k)) return -1;
  if (!rec_group_args_ok(group_of, group_n, cap)) return -1;
  const RecGroup gr{group_of, group_n, cap};
  return rec_filtered_host(self, n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, k, ids, scores, counts,
                           !sim_is_plain_cosine(sim, shrink), SimArgs{sim, shrink}, nullptr, rec_group_binds(gr, k) ? &gr : nullptr);
}

int smatrix_cf_recommend_deep_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                  const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                  const uint32_t* d_deny_bits, uint64_t deny_n, int sim, double shrink, uint32_t k, uint32_t* d_ids,
                                  double* d_scores, uint32_t* d_counts, void* hip_stream) {
  if (!sim_args_ok(sim, shrink) || !rec_deep_k_ok(k) || !rec_filt_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, 1u)) return -1;
  return rec_dev<false>(self, n_sessions, d_offsets, d_items,
                        RecFilt{d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, SimArgs{sim, shrink}},
                        !sim_is_plain_cosine(sim, shrink), k, d_ids, d_scores, d_counts, RecRank{}, hip_stream, nullptr, nullptr,
                        rec_deep_binds(k));
}

int smatrix_cf_recommend_deep(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                              const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, int sim,
                              double shrink, uint32_t k, uint32_t* ids, double* scores, uint32_t* counts) {
  if (!sim_args_ok(sim, shrink) || !rec_deep_k_ok(k) || !rec_filt_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, 1u)) return -1;
  return rec_filtered_host(self, n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, k, ids, scores, counts,
                           !sim_is_plain_cosine(sim, shrink), SimArgs{sim, shrink}, nullptr, nullptr, rec_deep_binds(k));
}

int smatrix_cf_rank_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items, const double* d_weights,
                        const uint64_t* d_ex_offsets, const uint32_t* d_ex_items, const uint32_t* d_deny_bits, uint64_t deny_n, int sim,
                        double shrink, const uint64_t* d_t_offsets, const uint32_t* d_targets, uint32_t* d_ranks, double* d_scores,
                        uint32_t* d_n_candidates, void* hip_stream) {
  if (!rec_rank_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink, d_t_offsets, d_targets)) return -1;
  return rec_dev<true>(self, n_sessions, d_offsets, d_items,
                       RecFilt{d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, SimArgs{sim, shrink}},
                       !sim_is_plain_cosine(sim, shrink), 0u, nullptr, nullptr, d_n_candidates,
                       RecRank{d_t_offsets, d_targets, d_ranks, d_scores}, hip_stream);
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
