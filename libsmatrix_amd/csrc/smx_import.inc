// smx_import.inc -- the session imports, host side: the windowed, weighted, reversible one (include/smatrix_batch.h
// smatrix_cf_import_events / _dev) and the reference example's loop (smatrix_cf_import_sessions / _dev).  Included by smx_runtime.hip
// inside the translation unit, after smx_explain.inc (uses smx_recommend.inc's call scope RecCall with its stager and its
// RecScratch, and the write path's apply_dev_locked, CkptAfter and cache_sync); the device code is kernels/import_events.hpp and,
// for the old call, k_cf_expand of kernels/rows.hpp.
//
// Inside a RecCall (the matrix lock, the stream, behind the previous call on the scratch; its finish applies the synchronisation
// rule and the trim), with a CkptAfter declared in front of it, imp_run:
//   1. k_imp_scan_reduce / _part / _apply: the slots before every session (8 bytes a session), every add saturating
//   2. ONE 8-byte read-back of the last entry: offsets that decrease or a total of 2^63 slots or more end the call here,
//      before the first write (DECR reads the offsets' first and last entry in the same wait: the positions of its head pass)
//   3. the scalar mirror dropped (cache_sync(m, true): the ops may touch mirrored cells)
//   4. per chunk of at most max_batch SLOTS: the chunk's counter zeroed, k_imp_emit (generation and compaction into the write
//      path's own sx / sy / sv), a 4-byte read-back of the counter, apply_dev_locked for that many ops with no result array.
//      A chunk holds at most as many ops as slots, so an internal batch never exceeds max_batch ops; one that compacts to
//      nothing applies nothing and is no batch.
// DECR runs step 4 with the head ops left out and then applies those, a lane per position (k_imp_heads), in batches of their
// own: a head cell (x, 0) that reaches 0 IS the empty slot (SURVEY.md quirk Q3) and cuts the probe chains that pass it, so a
// pair op of row x applied after it would miss its cell and make a second one.  A head cell reaches 0 only when every position
// that holds x is forgotten, and then every pair cell of the row is forgotten too: with the head ops last the row ends with all
// its cells at 0 and in place, in every order the two groups of batches run in.  INCR is one pass.
// The host flavour checks the offsets and the total before it touches the device, then stages offsets, ids and amounts with the
// scope's stager.
// The old call, smatrix_cf_import_sessions, shares the host side and not the generator: its host flavour is the same scope, CkptAfter
// and stager (and one buffer more, the op offsets the host worked out), but its ops come from ses_run -- k_cf_expand over those op
// offsets, L * L ops a session, no scan, no compaction, no read-back.  Its _dev flavour has no scratch and opens no scope.

namespace {

constexpr uint64_t IMP_DEFAULT_BATCH = 1ull << 25;     // (= CF_IMPORT_CHUNK, the old call's)
constexpr uint64_t IMP_MAX_BATCH = 1ull << 31;         // (a write batch holds fewer than 2^32 ops)
static_assert(IMP_FORWARD == SMATRIX_IMPORT_FORWARD && IMP_NO_SELF == SMATRIX_IMPORT_NO_SELF, "kernels/import_events.hpp");

// what both flavours refuse before anything else
bool imp_args_ok(int op, uint32_t flags, size_t n_sessions) {
  return (op == OP_INCR || op == OP_DECR) && !(flags & ~(IMP_FORWARD | IMP_NO_SELF)) && n_sessions <= 0xffffffffull;
}

// the whole call on the scope's stream, every array on the device; n >= 1.  -1 with nothing written for offsets that decrease
// or too many slots, else 0 with every batch applied (the write path returns after its last round) and *n_ops set.
int imp_run(smatrix_t* self, RecCall& c, int op, uint32_t n, const uint64_t* d_off, const uint32_t* d_ids, const uint32_t* d_amt,
            uint32_t window, uint32_t flags, uint64_t max_batch, uint64_t* n_ops) {
  Matrix* m = c.m;
  RecScratch& x = c.x();
  hipStream_t s = c.s;
  const uint32_t nt = (uint32_t)(((uint64_t)n + IMP_TILE - 1) / IMP_TILE);
  x.i_soff.need((size_t)n + 1); x.i_part.need((size_t)nt + 1); x.i_cnt.need(1);
  hipLaunchKernelGGL(k_imp_scan_reduce, dim3(nt), dim3(IMP_THREADS), 0, s, n, d_off, window, flags, x.i_part.p);
  hipLaunchKernelGGL(k_imp_scan_part, dim3(1), dim3(IMP_THREADS), 0, s, x.i_part.p, nt);
  hipLaunchKernelGGL(k_imp_scan_apply, dim3(nt), dim3(IMP_THREADS), 0, s, n, d_off, window, flags, x.i_part.p, nt, x.i_soff.p);
  HIP_OK(hipGetLastError());
  const bool heads_last = op == OP_DECR;
  uint64_t total = 0, pos[2] = {0, 0};                     // pos: the positions of ids the offsets name, [pos[0], pos[1])
  HIP_OK(hipMemcpyAsync(&total, x.i_soff.p + n, 8, hipMemcpyDeviceToHost, s));
  if (heads_last) {
    HIP_OK(hipMemcpyAsync(&pos[0], d_off, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(&pos[1], d_off + n, 8, hipMemcpyDeviceToHost, s));
  }
  HIP_OK(hipStreamSynchronize(s));
  if (total >= IMP_SAT) return -1;
  uint64_t applied = 0;
  if (total) {
    cache_sync(m, true);
    const uint64_t B = std::min(max_batch == 0 ? IMP_DEFAULT_BATCH : std::min(max_batch, IMP_MAX_BATCH), total);
    m->sx.need(B); m->sy.need(B); m->sv.need(B); m->so.need(B);
    const ImpArgs a{d_off, d_ids, d_amt, x.i_soff.p, n, window, flags, !heads_last};
    // one chunk of `cnt` slots (pairs) or positions (!pairs) from t0 on: generated, compacted, counted, applied
    auto chunk = [&](bool pairs, uint64_t t0, uint32_t cnt) {
      HIP_OK(hipMemsetAsync(x.i_cnt.p, 0, 4, s));
      if (pairs) hipLaunchKernelGGL(k_imp_emit, dim3(blocks_for(cnt)), dim3(256), 0, s, a, t0, cnt, x.i_cnt.p, m->sx.p, m->sy.p, m->sv.p);
      else hipLaunchKernelGGL(k_imp_heads, dim3(blocks_for(cnt)), dim3(256), 0, s, d_ids, d_amt, t0, cnt, x.i_cnt.p, m->sx.p, m->sy.p, m->sv.p);
      HIP_OK(hipGetLastError());
      uint32_t k = 0;
      HIP_OK(hipMemcpyAsync(&k, x.i_cnt.p, 4, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      if (!k) return;
      m->no_ret = true;                                   // no result array: a column-0 cell takes one 64-bit add
      apply_dev_locked(self, op, k, m->sx.p, m->sy.p, m->sv.p, m->so.p, s);
      m->no_ret = false;
      applied += k;
    };
    for (uint64_t t0 = 0; t0 < total; t0 += B) chunk(true, t0, (uint32_t)std::min<uint64_t>(B, total - t0));
    if (heads_last)
      for (uint64_t i0 = pos[0]; i0 < pos[1]; i0 += B) chunk(false, i0, (uint32_t)std::min<uint64_t>(B, pos[1] - i0));
  }
  if (n_ops) *n_ops = applied;
  return 0;
}

// the old call on stream s, under the matrix lock with the mirror dropped: the L * L incr ops of every session (d_op_offsets[s] = the
// ops before session s, the last entry = total_ops) generated in chunks of CF_IMPORT_CHUNK ops and applied as ordinary incr batches
constexpr uint64_t CF_IMPORT_CHUNK = 1ull << 25;
void ses_run(smatrix_t* self, Matrix* m, hipStream_t s, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_ids,
             const uint64_t* d_op_offsets, uint64_t total_ops) {
  const size_t chunk = (size_t)std::min<uint64_t>(total_ops, CF_IMPORT_CHUNK);
  m->sx.need(chunk); m->sy.need(chunk); m->sv.need(chunk); m->so.need(chunk);
  for (uint64_t t0 = 0; t0 < total_ops; t0 += CF_IMPORT_CHUNK) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(CF_IMPORT_CHUNK, total_ops - t0);
    hipLaunchKernelGGL(k_cf_expand, dim3(blocks_for(n)), dim3(256), 0, s, t0, n, (uint32_t)n_sessions, d_offsets, d_ids,
                       d_op_offsets, m->sx.p, m->sy.p, m->sv.p);
    HIP_OK(hipGetLastError());
    m->no_ret = true;
    apply_dev_locked(self, OP_INCR, n, m->sx.p, m->sy.p, m->sv.p, m->so.p, s);
    m->no_ret = false;
  }
}

}  // namespace

extern "C" {

// ---- CF-recommender write path (examples/cf_recommender.c:36-47) ------------------------------------------------
int smatrix_cf_import_sessions_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_ids,
                                   const uint64_t* d_op_offsets, uint64_t total_ops, void* hip_stream) {
  if (n_sessions == 0 || total_ops == 0) return 0;
  if (n_sessions > 0xffffffffull) return -1;
  Matrix* m = M(self);
  set_device(m);
  CkptAfter ckpt(self);                                  // (a checkpoint that falls due is taken after m->mu is released)
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, true);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
  ses_run(self, m, s, n_sessions, d_offsets, d_ids, d_op_offsets, total_ops);
  if (!hip_stream) HIP_OK(hipStreamSynchronize(s));
  return 0;
}

int smatrix_cf_import_sessions(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* ids) {
  if (n_sessions == 0) return 0;
  std::vector<uint64_t> op_off(n_sessions + 1, 0);
  for (size_t i = 0; i < n_sessions; i++) {
    if (offsets[i + 1] < offsets[i]) return -1;
    const uint64_t L = offsets[i + 1] - offsets[i];
    op_off[i + 1] = op_off[i] + L * L;
  }
  const uint64_t total = op_off[n_sessions];
  if (total == 0) return 0;
  if (n_sessions > 0xffffffffull) return -1;
  CkptAfter ckpt(self);
  RecCall c(self);
  RecScratch& x = c.x();
  const RecList q = c.stage(n_sessions, offsets, ids, x.h_off, x.h_items);
  c.rel.push_back(std::move(op_off));                     // (read by the copy in flight: alive until finish)
  x.h_opoff.need(n_sessions + 1);
  HIP_OK(hipMemcpyAsync(x.h_opoff.p, c.rel.back().data(), (n_sessions + 1) * 8, hipMemcpyHostToDevice, c.s));
  cache_sync(c.m, true);
  ses_run(self, c.m, c.s, n_sessions, q.off, q.val, x.h_opoff.p, total);
  return c.finish(0);
}

// ---- the same with a window, amounts and a way back ---------------------------------------------------------------

int smatrix_cf_import_events_dev(smatrix_t* self, int op, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_ids,
                                 const uint32_t* d_amounts, uint32_t window, uint32_t flags, uint64_t max_batch,
                                 uint64_t* n_ops, void* hip_stream) {
  if (!imp_args_ok(op, flags, n_sessions)) return -1;
  if (n_sessions == 0) { if (n_ops) *n_ops = 0; return 0; }
  CkptAfter ckpt(self);                                  // (a checkpoint that falls due is taken after m->mu is released)
  RecCall c(self, hip_stream);
  return c.finish(imp_run(self, c, op, (uint32_t)n_sessions, d_offsets, d_ids, d_amounts, window, flags, max_batch, n_ops));
}

int smatrix_cf_import_events(smatrix_t* self, int op, size_t n_sessions, const uint64_t* offsets, const uint32_t* ids,
                             const uint32_t* amounts, uint32_t window, uint32_t flags, uint64_t max_batch, uint64_t* n_ops) {
  if (!imp_args_ok(op, flags, n_sessions)) return -1;
  if (n_sessions == 0) { if (n_ops) *n_ops = 0; return 0; }
  const uint64_t n = n_sessions;
  uint64_t total = 0;                                     // the device's check, before the device is touched
  for (uint64_t i = 0; i < n; i++) total = imp_sat_add(total, imp_slots(offsets[i], offsets[i + 1], window, flags));
  if (total >= IMP_SAT) return -1;
  if (total == 0) { if (n_ops) *n_ops = 0; return 0; }
  CkptAfter ckpt(self);
  RecCall c(self);
  RecScratch& x = c.x();
  const RecList q = c.stage(n, offsets, ids, x.h_off, x.h_items);
  const uint32_t* d_amt = nullptr;
  if (amounts) {
    x.h_amt.need(std::max<uint64_t>(q.count, 1));
    if (q.count) HIP_OK(hipMemcpyAsync(x.h_amt.p, amounts + offsets[0], q.count * 4, hipMemcpyHostToDevice, c.s));
    d_amt = x.h_amt.p;
  }
  return c.finish(imp_run(self, c, op, (uint32_t)n, q.off, q.val, d_amt, window, flags, max_batch, n_ops));
}

}  // extern "C"
