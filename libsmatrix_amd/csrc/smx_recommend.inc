// smx_recommend.inc -- session recommendations (include/smatrix_batch.h smatrix_cf_recommend_batch / _dev,
// smatrix_cf_recommend_filtered / _dev, smatrix_cf_recommend_sim / _dev, smatrix_cf_recommend_fill / _dev,
// smatrix_cf_recommend_grouped / _dev, smatrix_cf_recommend_grouped_fill / _dev, smatrix_cf_recommend_scoped / _dev,
// smatrix_cf_recommend_deep / _dev and smatrix_cf_rank / _dev), host side.
// Included by smx_runtime.hip inside the translation unit, after smx_export.inc (uses Matrix, DevBuf, HIP_OK, and the export's
// u32 -> u64 scan kernels); the device code is kernels/recommend.hpp.
//
// Four layers, top down:
//   the extern "C" symbols   each is its refusals, its request, the call.  rec_args_ok refuses what every call refuses; a call adds
//                            its own (rec_k_ok, rec_deep_k_ok, rec_fill_args_ok, rec_group_args_ok, the targets)
//   RecReq (rec_req)         ONE request: everything a session call is given -- the sessions, the RecFilt, the ending (RecEnd), k and
//                            the outputs, the RecRank, the RecGroup, the RecFill -- with the arrays where the caller has them.  rec_req
//                            writes the one RecFilt literal and is the one place that normalises: which ending really runs, and
//                            which kernel instances
//   rec_call                 ONE call function for both flavours: scope, (host) rec_stage, rec_run, rec_fill, (host) rec_copy_back,
//                            finish.  The scope is RecCall, the one for every call on the read path's scratch (the files included
//                            behind this one as well: the item-neighbour calls' host flavours, the explain call, both imports, the
//                            popular call): the matrix lock, the scalar mirror written back (cache_sync), the stream, the wait for the
//                            call before, and at finish the event, the synchronisation rule and the trim.  Its stagers carry a host
//                            flavour's arrays to the device: stage (a window of a list of lists: sessions, exclusion lists, targets),
//                            stage_weights, stage_filter
//   rec_run                  the driver, ONE host function, given a request whose arrays are on the device:
//     1. k_rec_bound sorts the sessions into the LDS tier and the global tier; ONE read-back of RecCtl (counts, global-tier sizes)
//     2. rec_launch_lds: every LDS-tier session, one workgroup each, by the kernel of the request's ending
//     3. the global tier, per group of sessions whose tables fit REC_GROUP_SLOTS (normally one group): zeroed tables, k_rec_gl_init,
//        per block of item positions the chunk counts (k_rec_gl_plan) and their scan, a k_rec_gl_scan launch per position (the
//        kernel boundary keeps the items in session order), then rec_launch_tail: the kernels of the request's ending
// The endings (RecEnd), each a case of the two launch switches:
//   TopK     k_rec_lds; k_rec_gl_topk + k_rec_gl_merge (the only ending that uses lk / li)
//   Rank     the rank call: the answers are filled with "no answer" first (k_rec_rank_fill), k_rec_lds_rank, k_rec_gl_rank; counts
//            receives the candidate counts, k / ids / scores are not used
//   Grouped  the grouped call, over the map and the quota of its RecGroup: k_rec_lds_grouped, k_rec_gl_grouped
//   Deep     the deep call, k up to SMATRIX_DEEP_MAX: k_rec_lds_deep, k_rec_gl_deep
// Everything before the ending is shared.  A request with something in its RecFilt (weights, exclusion lists, deny bitmap) runs the
// kernels' <true> instances and with nothing given the <false> ones; with a measure in it the two kernels that make a score run as
// their _sim instances.  What rec_req makes of the calls, and the header promises: smatrix_cf_recommend_batch is the filtered call
// with nothing given; the sim call with SMATRIX_SIM_COSINE and shrink 0 IS the filtered call; the grouped call with no map, or with a
// quota that cannot bind (cap >= k), and the deep call with k <= 64 ARE the sim call, through the same launches.
// The fill call (smatrix_cf_recommend_fill / _dev) is the sim call with ONE launch behind the driver's, rec_fill: k_rec_fill reads
// the ids and counts both tiers wrote, notes them as n_scored and fills the free places from the caller's list (RecFill).// The grouped fill call (smatrix_cf_recommend_grouped_fill / _dev) is the grouped call with that launch behind it: a request with a
// RecGroup AND a RecFill.  Where the map binds, rec_fill launches k_rec_fill_grouped, the fill under the same quotas; where it cannot,
// rec_req has made the request the fill call's, k_rec_fill included.
// The scoped call (smatrix_cf_recommend_scoped / _dev) is the grouped fill call with a RecScope.  With lists given, the kernels that
// decide what a candidate is -- the LDS tier's, k_rec_gl_scan and the fill's -- run as their _scoped instances (REC_SC), which exist
// over the filtered _sim bodies alone, and k_rec_scope_bound measures the lists beside k_rec_bound, before the read-back; every other
// launch is the grouped fill call's.  Without lists rec_req leaves the request unscoped: the grouped fill call, launch for launch.

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
  DevBuf<uint32_t> h_scp, h_scgr;                    // ... and the scoped call's: its own map, the sessions' scope lists
  DevBuf<uint64_t> h_scoff;
  // ... and the dense select's (sel_run in smx_popular.inc; kernels/select.hpp): the words of the SelCtl<P> asked for, P::W words per
  // directory slot and per key collected.  One set for the popular and the trending call: a call holds the matrix lock and queues
  // behind `done` of the call before it, so no two selects are in flight on one matrix
  DevBuf<uint32_t> sel_ctl, sel_keys, sel_out;
  hipEvent_t done = nullptr;                         // recorded behind the last call's work (its stream may be any)
  // EVERY buffer above, and the only list of them: the trim, the "any buffer big" test and the release are this visitor's
  template <typename Fn>
  void for_each_buf(Fn f) {
    f(ctl); f(lds_list); f(big_list); f(gk); f(owner); f(zpos); f(cnt); f(li); f(big_off); f(tlg); f(gq); f(gs); f(lk); f(scan); f(part);
    f(h_items); f(h_ids); f(h_counts); f(h_off); f(h_scores); f(h_w); f(h_exoff); f(h_ex); f(h_deny); f(h_toff); f(h_tg); f(h_ranks);
    f(h_eoff); f(e_ra); f(e_cb); f(h_amt); f(i_cnt); f(i_soff); f(i_part); f(h_opoff); f(h_foff); f(h_fill); f(h_nsc); f(h_grp); f(h_scp); f(h_scgr); f(h_scoff);
    f(sel_ctl); f(sel_keys); f(sel_out);
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

// what ends a session's table: the top-k, or the rank call's, the grouped call's or the deep call's ending in its place
enum class RecEnd { TopK, Rank, Grouped, Deep };

// what smatrix_cf_recommend_fill adds to the sim call: the caller's list and where the scored counts go (NULL: not the fill call)
struct RecFill {
  const uint32_t* ids;
  uint64_t n;
  uint32_t* n_scored;
};

// Everything a session call is given, once.  The arrays are the caller's, host or device: an entry point writes down what it was
// handed, rec_stage makes a host flavour's request into one on the device, and the driver only ever sees the latter.
struct RecReq {
  uint32_t n;                                 // the sessions: off[0 .. n], items
  const uint64_t* off;
  const uint32_t* items;
  RecFilt f;
  bool filt, sim;                             // the kernels' instances: <true> for something given in f; _sim: the score is f.m's
  RecEnd end;
  uint32_t k;                                 // TopK, Grouped, Deep: ids / scores [n * k]; Rank: 0 and NULL
  uint32_t* ids;
  double* scores;
  uint32_t* counts;                           // [n]; Rank: the candidate counts
  RecRank rk;                                 // Rank: the target lists and their answers
  RecGroup gr;                                // Grouped: the map and the quota
  RecFill fl;                                 // the fill calls (fl.n_scored is given): k_rec_fill behind the driver's launches, behind the
                                              // Grouped ending k_rec_fill_grouped
  RecScope sc;                                // the scoped call: the map, the sessions' lists and the mode
  bool scoped;                                // lists were given: the _scoped instances (and then filt and sim are set)
};

// does the map change anything?  Without ids in it nobody is grouped, and a quota of k or more refuses nobody before the cut at k
bool rec_group_binds(const RecGroup& gr, uint32_t k) { return gr.n != 0 && gr.cap < k; }

// The request of a call behind its refusals, normalised HERE and nowhere else.  These are contracts of the header, not shortcuts: a
// grouped call that cannot bind and a deep call with k <= 64 ARE the sim call, (COSINE, 0) IS the filtered call, and a filtered
// call with nothing given IS the plain call -- through the same launches, the <false> and the not-_sim instances they always ran.
// The one RecFilt literal is here too: NULL / 0 for what was not given; the calls without a measure pass SMATRIX_SIM_COSINE and 0.0.
RecReq rec_req(size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights, const uint64_t* ex_offsets,
               const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, int sim, double shrink, RecEnd end, uint32_t k, uint32_t* ids,
               double* scores, uint32_t* counts, const RecRank& rk = RecRank{}, const RecGroup& gr = RecGroup{}, const RecFill& fl = RecFill{},
               const RecScope& sc = RecScope{}) {
  const RecFilt f{weights, ex_offsets, ex_items, deny_bits, deny_n, SimArgs{sim, shrink}};
  if (end == RecEnd::Grouped && !rec_group_binds(gr, k)) end = RecEnd::TopK;
  if (end == RecEnd::Deep && k <= 64) end = RecEnd::TopK;                 // up to 64 results the top-k ending holds them
  const bool scoped = sc.off != nullptr;                                  // no lists: not scoped (the entry point has refused a map without)
  return RecReq{(uint32_t)n_sessions, offsets, items, f, scoped || f.w || f.ex_off || f.deny_n, scoped || !sim_is_plain_cosine(sim, shrink), end, k,
                ids, scores, counts, rk, end == RecEnd::Grouped ? gr : RecGroup{}, fl, scoped ? sc : RecScope{}, scoped};
}

// a kernel template's instance for request q: k<true> with a filter, k<false> without; and of k / k_sim the second for a measure
#define REC_F(q, k) ((q).filt ? k<true> : k<false>)
#define REC_FS(q, k) ((q).sim ? REC_F(q, k##_sim) : REC_F(q, k))
// launch(kernel, args...) for request q, or launch(kernel_scoped, args..., q.sc) for a scoped one
#define REC_SC(q, launch, kernel, scoped_kernel, ...) \
  do { if ((q).scoped) launch(scoped_kernel, __VA_ARGS__, (q).sc); else launch(kernel, __VA_ARGS__); } while (0)

// the LDS tier, one workgroup per session of lds_list: the ending's kernel stands for k_rec_lds, behind the arguments all four share
void rec_launch_lds(Matrix* m, RecScratch& x, hipStream_t s, const RecReq& q, uint32_t n_lds) {
  auto launch = [&](auto kernel, auto... ending) {
    hipLaunchKernelGGL(kernel, dim3(std::min<uint32_t>(n_lds, 1u << 16)), dim3(REC_LDS_THREADS), 0, s, m->d_dir, m->dir_size - 1, m->arena.base,
                       x.ctl.p, x.lds_list.p, x.tlg.p, q.off, q.items, ending...);
  };
  switch (q.end) {
    case RecEnd::TopK:    REC_SC(q, launch, REC_FS(q, k_rec_lds), k_rec_lds_scoped, q.k, q.ids, q.scores, q.counts, q.f); break;
    case RecEnd::Rank:    launch(REC_FS(q, k_rec_lds_rank), q.rk, q.counts, q.f); break;
    case RecEnd::Grouped: REC_SC(q, launch, REC_FS(q, k_rec_lds_grouped), k_rec_lds_grouped_scoped, q.k, q.ids, q.scores, q.counts, q.f, q.gr); break;
    case RecEnd::Deep:    launch(REC_FS(q, k_rec_lds_deep), q.k, q.ids, q.scores, q.counts, q.f); break;
  }
}

// the global tier's ending over a group's finished tables G: one workgroup per session -- for the top-k behind a wave per segment
void rec_launch_tail(RecScratch& x, hipStream_t s, const RecReq& q, const RecGl& G, uint64_t nseg) {
  auto launch = [&](auto kernel, auto... ending) {
    hipLaunchKernelGGL(kernel, dim3(std::min<uint32_t>(G.n_big, 1u << 16)), dim3(REC_MERGE_THREADS), 0, s, G, ending...);
  };
  switch (q.end) {
    case RecEnd::TopK:
      hipLaunchKernelGGL(k_rec_gl_topk, dim3((uint32_t)std::min<uint64_t>((nseg + 3) / 4, 16384)), dim3(256), 0, s, G, nseg, q.k, x.lk.p,
                         x.li.p);
      launch(k_rec_gl_merge, q.k, x.lk.p, x.li.p, q.ids, q.scores, q.counts);
      break;
    case RecEnd::Rank:    launch(k_rec_gl_rank, q.rk, q.counts); break;
    case RecEnd::Grouped: launch(k_rec_gl_grouped, q.gr, q.k, q.ids, q.scores, q.counts); break;
    case RecEnd::Deep:    launch(k_rec_gl_deep, q.k, q.ids, q.scores, q.counts); break;
  }
}

// the whole call on stream s, every array of q on the device; returns with the work enqueued (after one synchronising read-back).
// -1 (nothing but k_rec_bound and k_rec_scope_bound has run) for a bad weight or an over-long scope list, which only a request with a filter can have; 0
// otherwise.
int rec_run(Matrix* m, RecScratch& x, hipStream_t s, const RecReq& q) {
  DirSlot* dir = m->d_dir;
  const uint32_t dmask = m->dir_size - 1, n = q.n;
  if (q.end == RecEnd::Rank) hipLaunchKernelGGL(k_rec_rank_fill, dim3(1024), dim3(256), 0, s, n, q.rk);
  x.ctl.need(1); x.lds_list.need(n); x.big_list.need(n); x.big_off.need(n); x.tlg.need(n);
  HIP_OK(hipMemsetAsync(x.ctl.p, 0, sizeof(RecCtl), s));
  hipLaunchKernelGGL(REC_F(q, k_rec_bound), dim3(std::min<uint32_t>(blocks_for((uint64_t)n * 64), 16384)), dim3(256), 0, s, dir, dmask, n, q.off,
                     q.items, (uint64_t)(m->arena.mapped / 8), x.ctl.p, x.lds_list.p, x.tlg.p, x.big_list.p, x.big_off.p, q.counts, q.f);
  if (q.scoped) hipLaunchKernelGGL(k_rec_scope_bound, dim3(std::min<uint32_t>(blocks_for(n), 16384)), dim3(256), 0, s, n, q.sc, x.ctl.p);
  HIP_OK(hipGetLastError());
  RecCtl c;
  HIP_OK(hipMemcpyAsync(&c, x.ctl.p, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (q.filt && c.bad) return -1;
  if (c.n_lds) rec_launch_lds(m, x, s, q, c.n_lds);
  HIP_OK(hipGetLastError());
  if (!c.n_big) return 0;
  const uint64_t ngroups = (c.total_slots + REC_GROUP_SLOTS - 1) / REC_GROUP_SLOTS;
  const uint64_t cap = ngroups == 1 ? c.total_slots : REC_GROUP_SLOTS + c.max_slots;
  const uint64_t nseg = cap / REC_SEG;
  const uint32_t np = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(c.max_len, REC_PLAN_MAX / c.n_big));
  x.gk.need(cap); x.gq.need(cap); x.gs.need(cap); x.owner.need(nseg); x.zpos.need(c.n_big);
  if (q.end == RecEnd::TopK) { x.lk.need(nseg * 64); x.li.need(nseg * 64); }
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
    hipLaunchKernelGGL(REC_F(q, k_rec_gl_init), dim3(std::min<uint32_t>(c.n_big, 1u << 16)), dim3(256), 0, s, G, q.off, q.items, q.f);
    HIP_OK(hipGetLastError());
    for (uint32_t p0 = 0; p0 < c.max_len; p0 += np) {
      const uint32_t nj = std::min<uint32_t>(np, c.max_len - p0);
      const uint64_t nt = (uint64_t)nj * c.n_big;
      hipLaunchKernelGGL(k_rec_gl_plan, dim3(blocks_for(nt)), dim3(256), 0, s, G, dir, dmask, q.off, q.items, p0, nj, x.cnt.p);
      HIP_OK(hipGetLastError());
      rec_scan(x, s, x.cnt.p, nt, x.scan.p);
      auto scan = [&](auto kernel, auto... args) {
        hipLaunchKernelGGL(kernel, dim3(2048), dim3(256), 0, s, G, dir, dmask, m->arena.base, q.off, q.items, p0, args...);
      };
      for (uint32_t j = 0; j < nj; j++) REC_SC(q, scan, REC_FS(q, k_rec_gl_scan), k_rec_gl_scan_scoped, j, x.scan.p, q.f);
      HIP_OK(hipGetLastError());
    }
    rec_launch_tail(x, s, q, G, nseg);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

// behind the recommend launches of both tiers, whatever they were: k_rec_fill, a wave per session -- behind the grouped ending
// k_rec_fill_grouped, the same under the request's quotas; for a scoped request k_rec_fill_scoped, which is both (the two are
// instances of one device body, rec_fill_walk<scope>)
void rec_fill(hipStream_t s, const RecReq& q) {
  auto launch = [&](auto kernel, auto... quotas) {
    hipLaunchKernelGGL(kernel, dim3(std::min<uint32_t>(blocks_for((uint64_t)q.n * 64), 16384)), dim3(256), 0, s, q.n, q.off, q.items, q.k,
                       q.fl.ids, (uint32_t)q.fl.n, q.ids, q.scores, q.counts, q.fl.n_scored, q.f, quotas...);
  };
  if (q.scoped) launch(k_rec_fill_scoped, q.gr, q.sc);                   // (without quotas q.gr holds no id: k_rec_fill's walk)
  else if (q.end == RecEnd::Grouped) launch(k_rec_fill_grouped, q.gr);
  else launch(k_rec_fill);
  HIP_OK(hipGetLastError());
}

#undef REC_SC
#undef REC_FS
#undef REC_F

// A host flavour's request on the device: what the request names is staged, and nothing else.  The rank call's answers are the
// targets' [t_offsets[0], t_offsets[n]); the other endings' unused entries read 0, as cf_topk_batch's (n * k: 64-bit throughout);
// the fill list goes through the stager as a list of lists that holds one list.
RecReq rec_stage(RecCall& c, const RecReq& q) {
  RecScratch& x = c.x();
  const uint64_t n = q.n;
  RecReq d = q;
  const RecList ses = c.stage(n, q.off, q.items, x.h_off, x.h_items);
  d.off = ses.off; d.items = ses.val;
  d.f = c.stage_filter(n, q.off, q.f.w, q.f.ex_off, q.f.ex, q.f.deny, q.f.deny_n, q.f.m);
  x.h_counts.need(n);
  d.counts = x.h_counts.p;
  if (q.end == RecEnd::Rank) {
    const RecList t = c.stage(n, q.rk.t_off, q.rk.targets, x.h_toff, x.h_tg);
    x.h_ranks.need(std::max<uint64_t>(t.count, 1)); x.h_scores.need(std::max<uint64_t>(t.count, 1));
    d.rk = RecRank{t.off, t.val, x.h_ranks.p, x.h_scores.p};
  } else {
    x.h_ids.need(n * q.k); x.h_scores.need(n * q.k);
    HIP_OK(hipMemsetAsync(x.h_ids.p, 0, n * q.k * 4, c.s));
    HIP_OK(hipMemsetAsync(x.h_scores.p, 0, n * q.k * 8, c.s));
    d.ids = x.h_ids.p; d.scores = x.h_scores.p;
  }
  if (q.end == RecEnd::Grouped) {
    x.h_grp.need(q.gr.n);
    HIP_OK(hipMemcpyAsync(x.h_grp.p, q.gr.of, q.gr.n * 4, hipMemcpyHostToDevice, c.s));
    d.gr.of = x.h_grp.p;
  }
  if (q.scoped) {
    x.h_scp.need(std::max<uint64_t>(q.sc.n, 1));
    if (q.sc.n) HIP_OK(hipMemcpyAsync(x.h_scp.p, q.sc.of, q.sc.n * 4, hipMemcpyHostToDevice, c.s));
    const RecList l = c.stage(n, q.sc.off, q.sc.gr, x.h_scoff, x.h_scgr);
    d.sc = RecScope{x.h_scp.p, q.sc.n, l.off, l.val, q.sc.except};
  }
  if (q.fl.n_scored) {
    const uint64_t one_list[2] = {0, q.fl.n};
    const RecList l = c.stage(1, one_list, q.fl.ids, x.h_foff, x.h_fill);
    x.h_nsc.need(n);
    d.fl = RecFill{l.val, l.count, x.h_nsc.p};
  }
  return d;
}

// ... and its answers, from the staged request d back to the caller's q
void rec_copy_back(RecCall& c, const RecReq& q, const RecReq& d) {
  const uint64_t n = q.n;
  HIP_OK(hipMemcpyAsync(q.counts, d.counts, n * 4, hipMemcpyDeviceToHost, c.s));
  if (q.end == RecEnd::Rank) {
    const uint64_t t0 = q.rk.t_off[0], count = q.rk.t_off[n] - t0;
    if (count) HIP_OK(hipMemcpyAsync(q.rk.ranks + t0, d.rk.ranks, count * 4, hipMemcpyDeviceToHost, c.s));
    if (count) HIP_OK(hipMemcpyAsync(q.rk.scores + t0, d.rk.scores, count * 8, hipMemcpyDeviceToHost, c.s));
  } else {
    HIP_OK(hipMemcpyAsync(q.ids, d.ids, n * q.k * 4, hipMemcpyDeviceToHost, c.s));
    HIP_OK(hipMemcpyAsync(q.scores, d.scores, n * q.k * 8, hipMemcpyDeviceToHost, c.s));
  }
  if (q.fl.n_scored) HIP_OK(hipMemcpyAsync(q.fl.n_scored, d.fl.n_scored, n * 4, hipMemcpyDeviceToHost, c.s));
}

// ... and its scope lists: none longer than SMATRIX_SCOPE_MAX
bool rec_host_scope_ok(const RecReq& q) {
  if (q.scoped)
    for (uint64_t s = 0; s < q.n; s++)
      if (q.sc.off[s + 1] - q.sc.off[s] > REC_SCOPE_MAX) return false;
  return true;
}

// Every session call behind its refusals.  No sessions: 0, and no scope.  A host flavour checks its weights and the lengths of its
// scope lists before the device is touched, so its driver result is 0; a _dev flavour's bad weight or over-long list is found on the
// device: -1 through the same finish, and no fill.
int rec_call(smatrix_t* self, const RecReq& q, bool host, void* hip_stream = nullptr) {
  if (q.n == 0) return 0;
  if (host && (!rec_host_weights_ok(q.f.w, q.off, q.n) || !rec_host_scope_ok(q))) return -1;
  RecCall c(self, host, hip_stream);
  const RecReq d = host ? rec_stage(c, q) : q;
  const int rc = rec_run(c.m, c.x(), c.s, d);
  if (d.fl.n_scored && rc == 0) rec_fill(c.s, d);
  if (host) rec_copy_back(c, q, d);
  return c.finish(rc);
}

// what every session call refuses, both flavours alike: a measure or a shrinkage that is none (sim_args_ok of smx_merge.inc: shrink is
// a host scalar in both flavours), too many sessions, a deny bitmap or exclusion lists given by half
bool rec_args_ok(size_t n_sessions, const void* ex_offsets, const void* ex_items, const void* deny_bits, uint64_t deny_n, int sim,
                 double shrink) {
  if (!sim_args_ok(sim, shrink) || n_sessions > 0xffffffffull) return false;
  if (deny_n > (1ull << 32) || (!deny_bits && deny_n)) return false;
  return (ex_offsets == nullptr) == (ex_items == nullptr);
}
// ... and what a call adds: the k of the top-k ending's 64 lanes, or the deep call's in its place
bool rec_k_ok(uint32_t k) { return k != 0 && k <= 64; }
bool rec_deep_k_ok(uint32_t k) { return k != 0 && k <= SMATRIX_DEEP_MAX; }
static_assert(SMATRIX_DEEP_MAX == REC_DEEP_MAX, "the list of kernels/recommend.hpp holds SMATRIX_DEEP_MAX entries");
// ... the fill call's list and n_scored
bool rec_fill_args_ok(const void* fill_ids, uint64_t n_fill, const void* n_scored) {
  return n_scored && n_fill < (1ull << 32) && (fill_ids || n_fill == 0);
}
// ... the grouped call's map and quota
bool rec_group_args_ok(const void* group_of, uint64_t group_n, uint32_t cap) {
  return cap != 0 && cap <= 64 && group_n <= (1ull << 32) && (group_of || group_n == 0);
}

// ... the scoped call's map, lists and mode: a map needs lists, lists come as a pair, and without lists nothing else is given
static_assert(SMATRIX_SCOPE_MAX == REC_SCOPE_MAX, "the fill kernels of kernels/recommend.hpp hold a scope list one entry per lane");
bool rec_scope_args_ok(const void* scope_of, uint64_t scope_n, const void* sc_offsets, const void* sc_groups, int scope_mode) {
  if (scope_mode != SMATRIX_SCOPE_ONLY && scope_mode != SMATRIX_SCOPE_EXCEPT) return false;
  if (scope_n > (1ull << 32) || (!scope_of && scope_n)) return false;
  if ((sc_offsets == nullptr) != (sc_groups == nullptr)) return false;
  return sc_offsets || (!scope_of && scope_n == 0);
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
  if (!rec_args_ok(n_sessions, nullptr, nullptr, nullptr, 0, SMATRIX_SIM_COSINE, 0.0) || !rec_k_ok(k)) return -1;
  return rec_call(self, rec_req(n_sessions, d_offsets, d_items, nullptr, nullptr, nullptr, nullptr, 0, SMATRIX_SIM_COSINE, 0.0,
                                RecEnd::TopK, k, d_ids, d_scores, d_counts), false, hip_stream);
}

int smatrix_cf_recommend_batch(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, uint32_t k,
                               uint32_t* ids, double* scores, uint32_t* counts) {
  if (!rec_args_ok(n_sessions, nullptr, nullptr, nullptr, 0, SMATRIX_SIM_COSINE, 0.0) || !rec_k_ok(k)) return -1;
  return rec_call(self, rec_req(n_sessions, offsets, items, nullptr, nullptr, nullptr, nullptr, 0, SMATRIX_SIM_COSINE, 0.0,
                                RecEnd::TopK, k, ids, scores, counts), true);
}

int smatrix_cf_recommend_filtered_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                      const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                      const uint32_t* d_deny_bits, uint64_t deny_n, uint32_t k, uint32_t* d_ids, double* d_scores,
                                      uint32_t* d_counts, void* hip_stream) {
  if (!rec_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, SMATRIX_SIM_COSINE, 0.0) || !rec_k_ok(k)) return -1;
  return rec_call(self, rec_req(n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, SMATRIX_SIM_COSINE, 0.0,
                                RecEnd::TopK, k, d_ids, d_scores, d_counts), false, hip_stream);
}

int smatrix_cf_recommend_filtered(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                                  const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                                  const uint32_t* deny_bits, uint64_t deny_n, uint32_t k, uint32_t* ids, double* scores,
                                  uint32_t* counts) {
  if (!rec_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, SMATRIX_SIM_COSINE, 0.0) || !rec_k_ok(k)) return -1;
  return rec_call(self, rec_req(n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, SMATRIX_SIM_COSINE, 0.0,
                                RecEnd::TopK, k, ids, scores, counts), true);
}

int smatrix_cf_recommend_sim_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                 const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                 const uint32_t* d_deny_bits, uint64_t deny_n, int sim, double shrink, uint32_t k, uint32_t* d_ids,
                                 double* d_scores, uint32_t* d_counts, void* hip_stream) {
  if (!rec_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink) || !rec_k_ok(k)) return -1;
  return rec_call(self, rec_req(n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink,
                                RecEnd::TopK, k, d_ids, d_scores, d_counts), false, hip_stream);
}

int smatrix_cf_recommend_sim(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                             const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, int sim,
                             double shrink, uint32_t k, uint32_t* ids, double* scores, uint32_t* counts) {
  if (!rec_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink) || !rec_k_ok(k)) return -1;
  return rec_call(self, rec_req(n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink,
                                RecEnd::TopK, k, ids, scores, counts), true);
}

int smatrix_cf_recommend_fill_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                  const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                  const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_fill_ids, uint64_t n_fill, int sim,
                                  double shrink, uint32_t k, uint32_t* d_ids, double* d_scores, uint32_t* d_counts, uint32_t* d_n_scored,
                                  void* hip_stream) {
  if (!rec_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink) || !rec_k_ok(k) || !rec_fill_args_ok(d_fill_ids, n_fill, d_n_scored)) return -1;
  return rec_call(self, rec_req(n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink,
                                RecEnd::TopK, k, d_ids, d_scores, d_counts, RecRank{}, RecGroup{}, RecFill{d_fill_ids, n_fill, d_n_scored}), false, hip_stream);
}

int smatrix_cf_recommend_fill(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                              const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n,
                              const uint32_t* fill_ids, uint64_t n_fill, int sim, double shrink, uint32_t k, uint32_t* ids, double* scores,
                              uint32_t* counts, uint32_t* n_scored) {
  if (!rec_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink) || !rec_k_ok(k) || !rec_fill_args_ok(fill_ids, n_fill, n_scored)) return -1;
  return rec_call(self, rec_req(n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink,
                                RecEnd::TopK, k, ids, scores, counts, RecRank{}, RecGroup{}, RecFill{fill_ids, n_fill, n_scored}), true);
}

int smatrix_cf_recommend_grouped_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                     const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                     const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_group_of, uint64_t group_n, uint32_t cap,
                                     int sim, double shrink, uint32_t k, uint32_t* d_ids, double* d_scores, uint32_t* d_counts,
                                     void* hip_stream) {
  if (!rec_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink) || !rec_k_ok(k) || !rec_group_args_ok(d_group_of, group_n, cap)) return -1;
  return rec_call(self, rec_req(n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink,
                                RecEnd::Grouped, k, d_ids, d_scores, d_counts, RecRank{}, RecGroup{d_group_of, group_n, cap}), false, hip_stream);
}

int smatrix_cf_recommend_grouped(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                                 const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n,
                                 const uint32_t* group_of, uint64_t group_n, uint32_t cap, int sim, double shrink, uint32_t k, uint32_t* ids,
                                 double* scores, uint32_t* counts) {
  if (!rec_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink) || !rec_k_ok(k) || !rec_group_args_ok(group_of, group_n, cap)) return -1;
  return rec_call(self, rec_req(n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink,
                                RecEnd::Grouped, k, ids, scores, counts, RecRank{}, RecGroup{group_of, group_n, cap}), true);
}

int smatrix_cf_recommend_grouped_fill_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                          const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                          const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_group_of, uint64_t group_n,
                                          uint32_t cap, const uint32_t* d_fill_ids, uint64_t n_fill, int sim, double shrink, uint32_t k,
                                          uint32_t* d_ids, double* d_scores, uint32_t* d_counts, uint32_t* d_n_scored, void* hip_stream) {
  if (!rec_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink) || !rec_k_ok(k) || !rec_group_args_ok(d_group_of, group_n, cap) ||
      !rec_fill_args_ok(d_fill_ids, n_fill, d_n_scored)) return -1;
  return rec_call(self, rec_req(n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink,
                                RecEnd::Grouped, k, d_ids, d_scores, d_counts, RecRank{}, RecGroup{d_group_of, group_n, cap},
                                RecFill{d_fill_ids, n_fill, d_n_scored}), false, hip_stream);
}

int smatrix_cf_recommend_grouped_fill(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                                      const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits,
                                      uint64_t deny_n, const uint32_t* group_of, uint64_t group_n, uint32_t cap, const uint32_t* fill_ids,
                                      uint64_t n_fill, int sim, double shrink, uint32_t k, uint32_t* ids, double* scores, uint32_t* counts,
                                      uint32_t* n_scored) {
  if (!rec_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink) || !rec_k_ok(k) || !rec_group_args_ok(group_of, group_n, cap) ||
      !rec_fill_args_ok(fill_ids, n_fill, n_scored)) return -1;
  return rec_call(self, rec_req(n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink,
                                RecEnd::Grouped, k, ids, scores, counts, RecRank{}, RecGroup{group_of, group_n, cap},
                                RecFill{fill_ids, n_fill, n_scored}), true);
}

int smatrix_cf_recommend_scoped_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                    const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                    const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_scope_of, uint64_t scope_n,
                                    const uint64_t* d_sc_offsets, const uint32_t* d_sc_groups, int scope_mode, const uint32_t* d_group_of,
                                    uint64_t group_n, uint32_t cap, const uint32_t* d_fill_ids, uint64_t n_fill, int sim, double shrink,
                                    uint32_t k, uint32_t* d_ids, double* d_scores, uint32_t* d_counts, uint32_t* d_n_scored, void* hip_stream) {
  if (!rec_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink) || !rec_k_ok(k) || !rec_group_args_ok(d_group_of, group_n, cap) ||
      !rec_fill_args_ok(d_fill_ids, n_fill, d_n_scored) || !rec_scope_args_ok(d_scope_of, scope_n, d_sc_offsets, d_sc_groups, scope_mode)) return -1;
  return rec_call(self, rec_req(n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink,
                                RecEnd::Grouped, k, d_ids, d_scores, d_counts, RecRank{}, RecGroup{d_group_of, group_n, cap},
                                RecFill{d_fill_ids, n_fill, d_n_scored},
                                RecScope{d_scope_of, scope_n, d_sc_offsets, d_sc_groups, scope_mode == SMATRIX_SCOPE_EXCEPT ? 1u : 0u}), false, hip_stream);
}

int smatrix_cf_recommend_scoped(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                                const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n,
                                const uint32_t* scope_of, uint64_t scope_n, const uint64_t* sc_offsets, const uint32_t* sc_groups, int scope_mode,
                                const uint32_t* group_of, uint64_t group_n, uint32_t cap, const uint32_t* fill_ids, uint64_t n_fill, int sim,
                                double shrink, uint32_t k, uint32_t* ids, double* scores, uint32_t* counts, uint32_t* n_scored) {
  if (!rec_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink) || !rec_k_ok(k) || !rec_group_args_ok(group_of, group_n, cap) ||
      !rec_fill_args_ok(fill_ids, n_fill, n_scored) || !rec_scope_args_ok(scope_of, scope_n, sc_offsets, sc_groups, scope_mode)) return -1;
  return rec_call(self, rec_req(n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink,
                                RecEnd::Grouped, k, ids, scores, counts, RecRank{}, RecGroup{group_of, group_n, cap},
                                RecFill{fill_ids, n_fill, n_scored},
                                RecScope{scope_of, scope_n, sc_offsets, sc_groups, scope_mode == SMATRIX_SCOPE_EXCEPT ? 1u : 0u}), true);
}

int smatrix_cf_recommend_deep_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                  const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                  const uint32_t* d_deny_bits, uint64_t deny_n, int sim, double shrink, uint32_t k, uint32_t* d_ids,
                                  double* d_scores, uint32_t* d_counts, void* hip_stream) {
  if (!rec_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink) || !rec_deep_k_ok(k)) return -1;
  return rec_call(self, rec_req(n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink,
                                RecEnd::Deep, k, d_ids, d_scores, d_counts), false, hip_stream);
}

int smatrix_cf_recommend_deep(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                              const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, int sim,
                              double shrink, uint32_t k, uint32_t* ids, double* scores, uint32_t* counts) {
  if (!rec_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink) || !rec_deep_k_ok(k)) return -1;
  return rec_call(self, rec_req(n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink,
                                RecEnd::Deep, k, ids, scores, counts), true);
}

int smatrix_cf_rank_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items, const double* d_weights,
                        const uint64_t* d_ex_offsets, const uint32_t* d_ex_items, const uint32_t* d_deny_bits, uint64_t deny_n, int sim,
                        double shrink, const uint64_t* d_t_offsets, const uint32_t* d_targets, uint32_t* d_ranks, double* d_scores,
                        uint32_t* d_n_candidates, void* hip_stream) {
  if (!rec_args_ok(n_sessions, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink) || !d_t_offsets || !d_targets) return -1;
  return rec_call(self, rec_req(n_sessions, d_offsets, d_items, d_weights, d_ex_offsets, d_ex_items, d_deny_bits, deny_n, sim, shrink,
                                RecEnd::Rank, 0u, nullptr, nullptr, d_n_candidates, RecRank{d_t_offsets, d_targets, d_ranks, d_scores}), false, hip_stream);
}

int smatrix_cf_rank(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                    const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, int sim,
                    double shrink, const uint64_t* t_offsets, const uint32_t* targets, uint32_t* ranks, double* scores,
                    uint32_t* n_candidates) {
  if (!rec_args_ok(n_sessions, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink) || !t_offsets || !targets) return -1;
  return rec_call(self, rec_req(n_sessions, offsets, items, weights, ex_offsets, ex_items, deny_bits, deny_n, sim, shrink,
                                RecEnd::Rank, 0u, nullptr, nullptr, n_candidates, RecRank{t_offsets, targets, ranks, scores}), true);
}

}  // extern "C"
