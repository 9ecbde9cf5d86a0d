// smx_merge.inc -- smatrix_merge / smatrix_merge_scaled / smatrix_merge_topk / smatrix_merge_topk_by / _sim / smatrix_import_csr /
// smatrix_import_csr_dev (include/smatrix_batch.h), host side.
// Included by smx_runtime.hip inside the translation unit, after smx_export.inc (uses its ExportScratch, ex_row_list, ex_measure
// and scan); the device code is kernels/merge.hpp.
//
// The three merges are one driver, mg_merge (validation, both locks, the mirrors, the scratch, the end of the call), around two
// stages that the entry point hands it: a count stage that leaves every row's count in x.cnt (ex_measure; for the filtered
// flavours mg_count_filtered around their own kernels) and an emit stage that mg_run_rows calls batch by batch.
//
// Every call is one loop over INTERNAL BATCHES of at most `bound` ops: a kernel writes batch b's packed {x, y, v} records into
// one of two record buffers, the ordinary write path applies them (run_write with in_stride == 3 and no result array, as
// smatrix_apply_packed_dev does), batches in order.  Batch b + 1 is emitted on a helper stream while the rounds of batch b run:
//   helper:  emit(0)  emit(1)         emit(2)          ...        (emit(b) waits for the write of batch b - 2: same buffer)
//   stream:           write(0)        write(1)         ...        (write(b) waits for emit(b))
// merge: the batches are runs of rows of the source's row list (ex_measure: directory-slot order, exact pair counts, u64 scan),
//        cut on the host from the scan; a row is never split, so bound = max(max_batch, longest row)
// CSR:   the batches are runs of max_batch pairs, wherever the rows' borders fall
// Device memory: two record buffers of 12 * bound bytes, the write path's own scratch for a batch of `bound` ops, and per ROW of
// the source 8 (row list) + 4 (counts) + 8 (scan) bytes -- nothing per pair.
// merge_scaled: merge with the counts of the SURVIVORS of its transform (k_mgx_count*, instead of the export's k_ex_count*) under
//        the same scan, so the cuts and the rows' record offsets are those of what k_mgx_emit* will write; same memory.
// merge_topk, merge_topk_by: the same with the counts and a threshold per row from the selection (mg_count_selected); the emission
//        filters by that threshold and counts a cut row's segments batch by batch, as merge does.  By value (k_mgt_*) the threshold
//        is 8 bytes, 28 bytes per row; by cosine (k_mgc_*) 12, its score half in thr and its column half in thr_col, 32 bytes per
//        row and no score per pair.  merge_topk_sim (k_mgs_*) is the cosine flavour with the measure and its shrinkage as two
//        more kernel arguments: the same 32 bytes per row.

namespace {

constexpr uint64_t MG_DEFAULT_BATCH = 1ull << 24;      // the batch size the write path is tuned for
constexpr uint64_t MG_MAX_BATCH = 1ull << 31;          // (a write batch holds fewer than 2^32 ops)

struct MergeScratch {
  DevBuf<uint32_t> rec[2], big, seg_cnt, flag, h_rows, h_pairs[2], thr_col;   // thr_col: the column half of a cosine threshold
  DevBuf<uint64_t> ptr, h_ptr, thr;                      // thr: merge_topk's per-row rank-key thresholds
  DevBuf<unsigned long long> tot;                        // merge_scaled: the candidates the count kernels saw
  hipStream_t e = nullptr;                               // the helper stream: emission
  hipEvent_t ev_start = nullptr, ev_rec[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
};

MergeScratch& mg_of(Matrix* m) {
  if (!m->mg) {
    MergeScratch* g = new MergeScratch();
    HIP_OK(hipStreamCreateWithFlags(&g->e, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&g->ev_start, hipEventDisableTiming));
    for (int i = 0; i < 2; i++) {
      HIP_OK(hipEventCreateWithFlags(&g->ev_rec[i], hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&g->ev_done[i], hipEventDisableTiming));
    }
    m->mg = g;
  }
  return *static_cast<MergeScratch*>(m->mg);
}

void mg_trim_all(MergeScratch& g, bool all) {
  ex_trim(g.rec[0], all); ex_trim(g.rec[1], all); ex_trim(g.big, all); ex_trim(g.seg_cnt, all); ex_trim(g.flag, all);
  ex_trim(g.h_rows, all); ex_trim(g.h_pairs[0], all); ex_trim(g.h_pairs[1], all); ex_trim(g.ptr, all); ex_trim(g.h_ptr, all);
  ex_trim(g.tot, all); ex_trim(g.thr, all); ex_trim(g.thr_col, all);
}

void merge_release(Matrix* m) {
  if (!m->mg) return;
  MergeScratch* g = static_cast<MergeScratch*>(m->mg);
  mg_trim_all(*g, true);
  (void)hipEventDestroy(g->ev_start);
  for (int i = 0; i < 2; i++) { (void)hipEventDestroy(g->ev_rec[i]); (void)hipEventDestroy(g->ev_done[i]); }
  (void)hipStreamDestroy(g->e);
  delete g;
  m->mg = nullptr;
}

// the measure and the shrinkage of smatrix_merge_topk_sim and smatrix_cf_recommend_sim (smx_recommend.inc): a known measure, a
// finite shrink >= 0 (-0.0 passes, NaN fails); the plain cosine is the existing code path of both
static_assert(SIM_COSINE == SMATRIX_SIM_COSINE && SIM_JACCARD == SMATRIX_SIM_JACCARD && SIM_LIFT == SMATRIX_SIM_LIFT, "kernels/sim.hpp");
bool sim_args_ok(int sim, double shrink) {
  return (sim == SMATRIX_SIM_COSINE || sim == SMATRIX_SIM_JACCARD || sim == SMATRIX_SIM_LIFT) && shrink >= 0.0 && std::isfinite(shrink);
}
bool sim_is_plain_cosine(int sim, double shrink) { return sim == SMATRIX_SIM_COSINE && shrink == 0.0; }

bool mg_op_ok(int op) { return op == OP_SET || op == OP_INCR || op == OP_DECR; }
uint64_t mg_batch(uint64_t max_batch) { return max_batch == 0 ? MG_DEFAULT_BATCH : std::min(max_batch, MG_MAX_BATCH); }

// The loop above.  count(b) = ops of batch b (> 0); emit(b, rec, e) enqueues the kernels that write them on stream e.
// Caller holds d->mu and has dropped d's scalar mirror; `bound` >= every count(b).
template <typename Count, typename Emit>
void mg_run(smatrix_t* dst, MergeScratch& g, int op, hipStream_t s, size_t nb, uint64_t bound, Count count, Emit emit) {
  if (!nb) return;
  Matrix* d = M(dst);
  g.rec[0].need(3 * bound);
  if (nb > 1) g.rec[1].need(3 * bound);
  HIP_OK(hipEventRecord(g.ev_start, s));                  // (the caller's arrays may be the work of earlier kernels on s)
  HIP_OK(hipStreamWaitEvent(g.e, g.ev_start, 0));
  // smatrix_profile(dst, 1): the emission of every batch is timed with HIP events on the helper stream; one stderr line per call
  const bool timed = d->profile;
  std::vector<hipEvent_t> tev;
  auto enqueue = [&](size_t b) {
    if (b >= 2) HIP_OK(hipStreamWaitEvent(g.e, g.ev_done[b & 1], 0));
    if (timed) { tev.emplace_back(); HIP_OK(hipEventCreate(&tev.back())); HIP_OK(hipEventRecord(tev.back(), g.e)); }
    emit(b, g.rec[b & 1].p, g.e);
    HIP_OK(hipGetLastError());
    if (timed) { tev.emplace_back(); HIP_OK(hipEventCreate(&tev.back())); HIP_OK(hipEventRecord(tev.back(), g.e)); }
    HIP_OK(hipEventRecord(g.ev_rec[b & 1], g.e));
  };
  enqueue(0);
  for (size_t b = 0; b < nb; b++) {
    if (b + 1 < nb) enqueue(b + 1);
    HIP_OK(hipStreamWaitEvent(s, g.ev_rec[b & 1], 0));
    const uint32_t n = count(b);
    const uint32_t* rec = g.rec[b & 1].p;
    d->in_stride = 3;
    d->so.need(n);
    d->no_ret = true;                                     // no result array: a column-0 cell takes one 64-bit add
    apply_dev_locked(dst, op, n, rec, rec + 1, rec + 2, d->so.p, s);
    d->no_ret = false;
    d->in_stride = 1;
    HIP_OK(hipEventRecord(g.ev_done[b & 1], s));
  }
  // (smatrix_stats_t::batches counts the internal batches -- each is a write batch the device executed; SMATRIX_FLUSH_EVERY: the
  //  call owes ONE checkpoint when any of them was an N-th, apply_dev_locked's ckpt_due, taken by the caller's CkptAfter)
  HIP_OK(hipStreamSynchronize(g.e));
  if (timed) {
    double ms = 0;
    for (size_t i = 0; i + 1 < tev.size(); i += 2) { float t = 0; HIP_OK(hipEventElapsedTime(&t, tev[i], tev[i + 1])); ms += t; }
    for (hipEvent_t ev : tev) (void)hipEventDestroy(ev);
    fprintf(stderr, "[smatrix] merge: %zu internal batches of at most %llu ops, record emission %.3f ms in all (helper stream, beside the write path)\n",
            nb, (unsigned long long)bound, ms);
  }
}

// the CSR flavours' common part: arrays on the device, except the pairs when h_pairs is given (uploaded batch by batch)
int mg_import(smatrix_t* self, int op, uint64_t n_rows, const uint32_t* d_rows, const uint64_t* d_row_ptr, const uint32_t* d_pairs,
              const uint32_t* h_pairs, uint64_t max_batch, uint64_t* n_ops, hipStream_t s) {
  Matrix* m = M(self);
  MergeScratch& g = mg_of(m);
  g.flag.need(1);
  HIP_OK(hipMemsetAsync(g.flag.p, 0, 4, s));
  hipLaunchKernelGGL(k_mg_csr_check, dim3(std::min<uint32_t>(blocks_for(n_rows), 4096)), dim3(256), 0, s, n_rows, d_row_ptr, g.flag.p);
  HIP_OK(hipGetLastError());
  uint64_t nnz = 0;
  uint32_t bad = 0;
  HIP_OK(hipMemcpyAsync(&bad, g.flag.p, 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&nnz, d_row_ptr + n_rows, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (bad) return -1;
  const uint64_t B = std::min(mg_batch(max_batch), std::max<uint64_t>(nnz, 1));
  const size_t nb = (size_t)((nnz + B - 1) / B);
  if (h_pairs && nb) { g.h_pairs[0].need(2 * B); if (nb > 1) g.h_pairs[1].need(2 * B); }
  cache_sync(m, true);
  mg_run(self, g, op, s, nb, B,
         [&](size_t b) { return (uint32_t)std::min<uint64_t>(B, nnz - b * B); },
         [&](size_t b, uint32_t* rec, hipStream_t e) {
           const uint64_t t0 = b * B;
           const uint32_t cnt = (uint32_t)std::min<uint64_t>(B, nnz - t0);
           const uint32_t* pairs = d_pairs ? d_pairs + 2 * t0 : g.h_pairs[b & 1].p;
           if (!d_pairs) HIP_OK(hipMemcpyAsync(g.h_pairs[b & 1].p, h_pairs + 2 * t0, (size_t)cnt * 8, hipMemcpyHostToDevice, e));
           hipLaunchKernelGGL(k_mg_emit_csr, dim3(blocks_for(cnt)), dim3(256), 0, e, n_rows, d_rows, d_row_ptr, pairs, t0, cnt, rec);
         });
  if (n_ops) *n_ops = nnz;
  mg_trim_all(g, false);
  return 0;
}

// the merges once the counts of the source's n rows are in x.cnt and the first half of their scan is done (x.cnt_tiles): the
// second half, the batches cut on the host, the loop.  emit(r0, r1, rec, e) enqueues the kernels that write the records of the
// rows [r0, r1) of the row list on stream e.  The caller holds both locks.
template <typename EmitRows>
void mg_run_rows(smatrix_t* dst, ExportScratch& x, MergeScratch& g, int op, hipStream_t s, uint64_t n, uint64_t max_batch, EmitRows emit) {
  g.ptr.need(n + 1);
  ex_scan_apply(x, s, x.cnt.p, n, x.cnt_tiles, g.ptr.p);
  std::vector<uint64_t> ptr(n + 1);
  HIP_OK(hipMemcpyAsync(ptr.data(), g.ptr.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  // the batches: rows [cut[b], cut[b + 1]), as many whole rows as fit into B ops -- at least one
  const uint64_t B = mg_batch(max_batch);
  std::vector<uint32_t> cut{0};
  uint64_t bound = 0;
  for (uint64_t r0 = 0; r0 < n;) {
    uint64_t r1 = std::upper_bound(ptr.begin() + r0 + 1, ptr.end(), ptr[r0] + B) - ptr.begin() - 1;   // the last r1 with ptr[r1] - ptr[r0] <= B
    if (r1 == r0) r1 = r0 + 1;
    if (ptr[r1] > ptr[r0]) {                              // (a run of rows without pairs at the end emits nothing)
      cut.push_back((uint32_t)r1);
      bound = std::max(bound, ptr[r1] - ptr[r0]);
    } else if (cut.size() > 1) cut.back() = (uint32_t)r1;
    else cut[0] = (uint32_t)r1;
    r0 = r1;
  }
  if (bound >= (1ull << 32)) smx_die("merge: a source row of 2^32 pairs");
  mg_run(dst, g, op, s, cut.size() - 1, bound,
         [&](size_t b) { return (uint32_t)(ptr[cut[b + 1]] - ptr[cut[b]]); },
         [&](size_t b, uint32_t* rec, hipStream_t e) { emit(cut[b], cut[b + 1], rec, e); });
}

// rows of more than GETROW_WAVE_MAX cells: noted per batch; a cut row's segment counts by arena position (kernels/merge.hpp)
// (segments of uncut rows: 128 KiB of cells and up each; of cut rows: 256 KiB each -- two words per entry)
void mg_need_big(MergeScratch& g, Matrix* sm) {
  g.big.need(2 * ((sm->arena.mapped >> 17) + (sm->arena.mapped >> MG_SEG_SHIFT) + 2) + 1);
  g.seg_cnt.need((sm->arena.mapped >> MG_SEG_SHIFT) + 2);
}
uint32_t mg_row_grid(uint64_t rows) { return std::min<uint32_t>(blocks_for(rows * 64), 16384); }   // the wave-per-row kernels

// One call of the merge family, between its stages: both matrices (locked), the destination's stream, the source's export
// scratch, the destination's merge scratch; from the count stage on, the rows of the source's row list (x.items), the pairs the
// call applies and, in the filtered flavours, the pairs it looked at.
struct MergeCall {
  Matrix *d, *sm;
  hipStream_t s;
  ExportScratch& x;
  MergeScratch& g;
  uint32_t big_grid;                                       // of the 1024-lane kernels that walk `big`
  uint64_t n = 0, kept = 0;
  unsigned long long seen = 0;
};

// the wave-per-row / per-segment launch of an emission: the kernel's common arguments, then the flavour's functor (if any)
template <typename K, typename... F>
void mg_emit(const MergeCall& c, K kernel, uint32_t r0, uint32_t r1, uint32_t* rec, hipStream_t e, F... f) {
  hipLaunchKernelGGL(kernel, dim3(mg_row_grid(r1 - r0)), dim3(256), 0, e, c.sm->d_dir, c.sm->arena.base, c.x.items.p, c.g.ptr.p,
                     r0, r1, rec, c.g.big.p, f...);
}
template <typename K, typename... F>
void mg_emit_big(const MergeCall& c, K kernel, uint32_t r0, uint32_t* rec, hipStream_t e, F... f) {
  hipLaunchKernelGGL(kernel, dim3(c.big_grid), dim3(1024), 0, e, c.sm->d_dir, c.sm->arena.base, c.x.items.p, c.g.ptr.p,
                     r0, rec, c.g.big.p, c.g.seg_cnt.p, f...);
}

// The driver of smatrix_merge / _scaled / _topk, behind the flavour's own validation clause.
//   count(c)                  leaves c.n, every row's count in c.x.cnt, c.x.cnt_tiles (ex_scan_prep), c.kept and c.seen; when
//                             c.kept != 0 also `big` and seg_cnt sized (mg_need_big)
//   emit(c, r0, r1, rec, e)   enqueues the kernels that write the records of the rows [r0, r1) on stream e; big[0] is 0
// Refusals come before any lock or device call; n_dropped is NULL where the flavour drops nothing.
template <typename Count, typename Emit>
int mg_merge(smatrix_t* dst, smatrix_t* src, int op, uint64_t max_batch, uint64_t* n_ops, uint64_t* n_dropped, Count count, Emit emit) {
  if (!mg_op_ok(op) || !dst || !src || dst == src) return -1;
  Matrix *d = M(dst), *sm = M(src);
  if (d == sm || d->device != sm->device) return -1;
  set_device(d);
  CkptAfter ckpt(dst);                                    // (a checkpoint that falls due is taken after the locks are released)
  // both matrix locks, lower address first: merge(a, b) and merge(b, a) on two threads cannot wait for each other.  Neither
  // file lock is needed (nothing here writes a file), so the file-then-matrix order holds trivially.
  std::unique_lock<std::mutex> l0(d < sm ? d->mu : sm->mu);
  std::unique_lock<std::mutex> l1(d < sm ? sm->mu : d->mu);
  cache_sync(sm, false);
  cache_sync(d, true);
  MergeCall c{d, sm, d->stream, ex_of(sm), mg_of(d), (uint32_t)std::min<uint64_t>(sm->arena.mapped / 8 / GETROW_SEG + 1, 2048)};
  count(c);
  if (c.kept)
    mg_run_rows(dst, c.x, c.g, op, c.s, c.n, max_batch, [&](uint32_t r0, uint32_t r1, uint32_t* rec, hipStream_t e) {
      HIP_OK(hipMemsetAsync(c.g.big.p, 0, 4, e));
      emit(c, r0, r1, rec, e);
    });
  HIP_OK(hipStreamSynchronize(c.s));
  if (n_ops) *n_ops = c.kept;
  if (n_dropped) *n_dropped = c.seen - c.kept;
  ex_trim_all(c.x, false);
  mg_trim_all(c.g, false);
  return 0;
}

// The count stage of the filtered flavours (what ex_measure is to smatrix_merge): the row list; `launch` enqueues the kernels
// that leave every row's survivors in x.cnt and the non-empty cells they saw in *g.tot (with `big` started at 0 entries); the
// first half of the scan; both totals read back.  A profiled matrix times the kernels, and the scan when scan_timed, with HIP
// events: report(kernels_ms, scan_ms) prints the flavour's stderr line.
template <typename Launch, typename Report>
void mg_count_filtered(MergeCall& c, bool scan_timed, Launch launch, Report report) {
  ExportScratch& x = c.x;
  MergeScratch& g = c.g;
  hipStream_t s = c.s;
  c.n = ex_row_list(c.sm, x, SMATRIX_EXPORT_TABLE, s);
  if (!c.n) return;
  x.cnt.need(c.n);
  mg_need_big(g, c.sm);
  g.tot.need(1);
  HIP_OK(hipMemsetAsync(g.big.p, 0, 4, s));
  HIP_OK(hipMemsetAsync(g.tot.p, 0, 8, s));
  const bool timed = c.d->profile;
  hipEvent_t tev[3] = {nullptr, nullptr, nullptr};
  if (timed) { for (hipEvent_t& ev : tev) HIP_OK(hipEventCreate(&ev)); HIP_OK(hipEventRecord(tev[0], s)); }
  launch();
  HIP_OK(hipGetLastError());
  if (timed) HIP_OK(hipEventRecord(tev[1], s));
  x.cnt_tiles = ex_scan_prep(x, s, x.cnt.p, c.n);
  if (timed && scan_timed) HIP_OK(hipEventRecord(tev[2], s));
  HIP_OK(hipMemcpyAsync(&c.seen, g.tot.p, 8, hipMemcpyDeviceToHost, s));
  c.kept = ex_read(x.part.p + x.cnt_tiles, s);
  if (timed) {
    float kernels = 0, scan = 0;
    HIP_OK(hipEventElapsedTime(&kernels, tev[0], tev[1]));
    if (scan_timed) HIP_OK(hipEventElapsedTime(&scan, tev[1], tev[2]));
    for (hipEvent_t ev : tev) (void)hipEventDestroy(ev);
    report(kernels, scan);
  }
}

// The count stage of the top-k flavours: the selection, which leaves every row's threshold and, with it, the number of pairs the
// row keeps -- the count of an uncut row needs no pass of its own.  `big` lists the rows of more than GETROW_WAVE_MAX cells here
// (one word each: it has room for two per 128 KiB of row tables, and such a row is 128 KiB at least); the emission of every batch
// starts it afresh.  launch(c, kernel, grid, lanes, n...) is the flavour's argument list, for the wave-per-row kernel (n = the
// rows) and for the workgroup-per-row kernel (no n); col_half: the thresholds have a column half, in thr_col.
template <typename KW, typename KB, typename Launch>
auto mg_count_selected(const char* flavour, bool col_half, KW k_wave, KB k_big, Launch launch) {
  return [=](MergeCall& c) {
    mg_count_filtered(c, true,
      [&] {
        c.g.thr.need(c.n);
        if (col_half) c.g.thr_col.need(c.n);
        launch(c, k_wave, dim3(mg_row_grid(c.n)), dim3(256), (uint32_t)c.n);
        launch(c, k_big, dim3(c.big_grid), dim3(1024));
      },
      [&](float sel, float cnt) {
        fprintf(stderr, "[smatrix] %s: selection %.3f ms (the kept count of every row with it), count scan %.3f ms, %llu of %llu pairs survive\n",
                flavour, sel, cnt, (unsigned long long)c.kept, c.seen);
      });
  };
}

// their emit stage: the rows, then the segments of the cut rows counted and written, all with the flavour's filter
template <typename K, typename KC, typename KB, typename F>
void mg_emit_topk(const MergeCall& c, K k_rows, KC k_big_count, KB k_big, uint32_t r0, uint32_t r1, uint32_t* rec, hipStream_t e, const F f) {
  mg_emit(c, k_rows, r0, r1, rec, e, f);
  mg_emit_big(c, k_big_count, r0, rec, e, f);
  mg_emit_big(c, k_big, r0, rec, e, f);
}

}  // namespace

extern "C" {

int smatrix_merge(smatrix_t* dst, smatrix_t* src, int op, uint64_t max_batch, uint64_t* n_ops) {
  return mg_merge(dst, src, op, max_batch, n_ops, nullptr,
    [](MergeCall& c) {                                    // the row list, the counts, the first half of their scan
      ex_measure(c.sm, c.x, SMATRIX_EXPORT_TABLE, c.s, &c.n, &c.kept);
      if (c.kept) mg_need_big(c.g, c.sm);
    },
    [](const MergeCall& c, uint32_t r0, uint32_t r1, uint32_t* rec, hipStream_t e) {
      mg_emit(c, k_mg_emit, r0, r1, rec, e);
      mg_emit_big(c, k_mg_emit_big<true>, r0, rec, e);
      mg_emit_big(c, k_mg_emit_big<false>, r0, rec, e);
    });
}

int smatrix_merge_scaled(smatrix_t* dst, smatrix_t* src, int op, uint32_t num, uint32_t den, uint32_t min_value, uint64_t max_batch,
                         uint64_t* n_ops, uint64_t* n_dropped) {
  if (num == 0 || num > den) return -1;                   // (num >= 1, so den == 0 is num > den)
  const MgScale f{num, den, min_value, 1.0 / (double)den};
  return mg_merge(dst, src, op, max_batch, n_ops, n_dropped,
    [&](MergeCall& c) {
      // the survivors of every row (and of every segment of a cut row) and the candidates in all: the one counting pass
      mg_count_filtered(c, false,
        [&] {
          hipLaunchKernelGGL(k_mgx_count, dim3(mg_row_grid(c.n)), dim3(256), 0, c.s, c.sm->d_dir, c.sm->arena.base, (uint32_t)c.n,
                             c.x.items.p, c.x.cnt.p, c.g.big.p, c.g.tot.p, f);
          hipLaunchKernelGGL(k_mgx_count_big, dim3(c.big_grid), dim3(1024), 0, c.s, c.sm->d_dir, c.sm->arena.base, c.x.items.p,
                             c.x.cnt.p, c.g.big.p, c.g.seg_cnt.p, c.g.tot.p, f);
        },
        [&](float ms, float) {
          fprintf(stderr, "[smatrix] merge_scaled: filtered count %.3f ms, %llu of %llu pairs survive\n", ms, (unsigned long long)c.kept, c.seen);
        });
    },
    [&](const MergeCall& c, uint32_t r0, uint32_t r1, uint32_t* rec, hipStream_t e) {
      mg_emit(c, k_mgx_emit, r0, r1, rec, e, f);
      mg_emit_big(c, k_mgx_emit_big, r0, rec, e, f);
    });
}

int smatrix_merge_topk(smatrix_t* dst, smatrix_t* src, int op, uint32_t m, uint32_t min_value, uint64_t max_batch, uint64_t* n_ops,
                       uint64_t* n_dropped) {
  if (m == 0) return -1;
  return mg_merge(dst, src, op, max_batch, n_ops, n_dropped,
    mg_count_selected("merge_topk", false, k_mgt_select, k_mgt_select_big, [=](MergeCall& c, auto kernel, dim3 grid, dim3 lanes, auto... n) {
      hipLaunchKernelGGL(kernel, grid, lanes, 0, c.s, c.sm->d_dir, c.sm->arena.base, n..., c.x.items.p, m, min_value, c.g.thr.p,
                         c.x.cnt.p, c.g.big.p, c.g.tot.p);
    }),
    [&](const MergeCall& c, uint32_t r0, uint32_t r1, uint32_t* rec, hipStream_t e) {
      mg_emit_topk(c, k_mgt_emit, k_mgt_emit_big<true>, k_mgt_emit_big<false>, r0, r1, rec, e, MgTopk{{c.g.thr.p}, {}, min_value});
    });
}

int smatrix_merge_topk_by(smatrix_t* dst, smatrix_t* src, int op, int rank, uint32_t m, uint32_t min_value, uint64_t max_batch,
                          uint64_t* n_ops, uint64_t* n_dropped) {
  if (rank == SMATRIX_RANK_VALUE) return smatrix_merge_topk(dst, src, op, m, min_value, max_batch, n_ops, n_dropped);
  if (rank != SMATRIX_RANK_COSINE || m == 0) return -1;
  return mg_merge(dst, src, op, max_batch, n_ops, n_dropped,
    mg_count_selected("merge_topk_by cosine", true, k_mgc_select, k_mgc_select_big, [=](MergeCall& c, auto kernel, dim3 grid, dim3 lanes, auto... n) {
      hipLaunchKernelGGL(kernel, grid, lanes, 0, c.s, c.sm->d_dir, c.sm->dir_size - 1, c.sm->arena.base, n..., c.x.items.p, m, min_value,
                         c.g.thr.p, c.g.thr_col.p, c.x.cnt.p, c.g.big.p, c.g.tot.p);
    }),
    [&](const MergeCall& c, uint32_t r0, uint32_t r1, uint32_t* rec, hipStream_t e) {
      mg_emit_topk(c, k_mgc_emit, k_mgc_emit_big<true>, k_mgc_emit_big<false>, r0, r1, rec, e,
                   MgCos{{c.g.thr.p, c.g.thr_col.p}, {c.sm->d_dir, c.sm->arena.base, c.x.items.p, c.sm->dir_size - 1}, min_value});
    });
}

int smatrix_merge_topk_sim(smatrix_t* dst, smatrix_t* src, int op, int sim, double shrink, uint32_t m, uint32_t min_value,
                           uint64_t max_batch, uint64_t* n_ops, uint64_t* n_dropped) {
  if (!sim_args_ok(sim, shrink)) return -1;
  if (sim_is_plain_cosine(sim, shrink))
    return smatrix_merge_topk_by(dst, src, op, SMATRIX_RANK_COSINE, m, min_value, max_batch, n_ops, n_dropped);
  if (m == 0) return -1;
  const SimArgs f{sim, shrink};
  return mg_merge(dst, src, op, max_batch, n_ops, n_dropped,
    mg_count_selected("merge_topk_sim", true, k_mgs_select, k_mgs_select_big, [=](MergeCall& c, auto kernel, dim3 grid, dim3 lanes, auto... n) {
      hipLaunchKernelGGL(kernel, grid, lanes, 0, c.s, c.sm->d_dir, c.sm->dir_size - 1, c.sm->arena.base, n..., c.x.items.p, m, min_value, f,
                         c.g.thr.p, c.g.thr_col.p, c.x.cnt.p, c.g.big.p, c.g.tot.p);
    }),
    [&](const MergeCall& c, uint32_t r0, uint32_t r1, uint32_t* rec, hipStream_t e) {
      mg_emit_topk(c, k_mgs_emit, k_mgs_emit_big<true>, k_mgs_emit_big<false>, r0, r1, rec, e,
                   MgSimArgs{c.g.thr.p, c.g.thr_col.p, c.sm->dir_size - 1, min_value, f});
    });
}

int smatrix_import_csr_dev(smatrix_t* self, int op, uint64_t n_rows, const uint32_t* d_rows, const uint64_t* d_row_ptr,
                           const uint32_t* d_pairs, uint64_t max_batch, uint64_t* n_ops, void* hip_stream) {
  if (!mg_op_ok(op) || !self) return -1;
  if (n_ops) *n_ops = 0;
  if (n_rows == 0) return 0;
  Matrix* m = M(self);
  set_device(m);
  CkptAfter ckpt(self);
  std::lock_guard<std::mutex> lk(m->mu);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
  const int rc = mg_import(self, op, n_rows, d_rows, d_row_ptr, d_pairs, nullptr, max_batch, n_ops, s);
  if (rc == 0 && !hip_stream) HIP_OK(hipStreamSynchronize(s));
  return rc;
}

int smatrix_import_csr(smatrix_t* self, int op, uint64_t n_rows, const uint32_t* rows, const uint64_t* row_ptr, const uint32_t* pairs,
                       uint64_t max_batch, uint64_t* n_ops) {
  if (!mg_op_ok(op) || !self) return -1;
  if (n_ops) *n_ops = 0;
  if (n_rows == 0) return 0;
  Matrix* m = M(self);
  set_device(m);
  CkptAfter ckpt(self);
  std::lock_guard<std::mutex> lk(m->mu);
  hipStream_t s = m->stream;
  MergeScratch& g = mg_of(m);
  g.h_rows.need(n_rows); g.h_ptr.need(n_rows + 1);         // per row; the pairs travel batch by batch (mg_import)
  HIP_OK(hipMemcpyAsync(g.h_rows.p, rows, n_rows * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(g.h_ptr.p, row_ptr, (n_rows + 1) * 8, hipMemcpyHostToDevice, s));
  const int rc = mg_import(self, op, n_rows, g.h_rows.p, g.h_ptr.p, nullptr, pairs, max_batch, n_ops, s);
  HIP_OK(hipStreamSynchronize(s));
  return rc;
}

}  // extern "C"
