// smx_export.inc -- whole-matrix export (include/smatrix_batch.h smatrix_export / smatrix_export_dev), host side.
// Included by smx_runtime.hip inside the translation unit (uses Matrix, DevBuf, HIP_OK, smx_die, launch_getrow); the device
// code is kernels/export.hpp.
//
// Under the matrix lock, after the scalar mirror has been written back (cache_sync):
//   1. the row list: per-tile counts of the USED directory slots, a scan, an ordered write -> {row id, slot}, slot order;
//      SORTED: a stable LSD radix sort of that list by id
//   2. every row's exact pair count (k_ex_count / k_ex_count_big), its scan -> nnz; both sizes are read back
//   3. (room enough) row_ptr = the scan, rows = the ids, the pairs by launch_getrow with row_ptr as its offsets: TABLE order is
//      getrow's bytes by construction; the counts getrow reports are compared with step 2's on the device
//   4. SORTED: every row's pairs by column -- in LDS for rows of up to EX_LDS_MID pairs, by the segmented radix sort above that

namespace {

struct ExportScratch {
  DevBuf<uint32_t> tcnt, cnt, got, ctl, l0, l1, l2, hist, tstart;
  DevBuf<uint64_t> part, toff, items, hscan, info, seg, tmp;
  DevBuf<uint32_t> h_rows;                 // the host flavour's device copies of the caller's arrays
  DevBuf<uint64_t> h_ptr, h_pairs;
  uint32_t cnt_tiles = 0;                  // tiles of the count scan whose partial sums `part` holds (step 2 -> step 3)
};

ExportScratch& ex_of(Matrix* m) {
  if (!m->ex) m->ex = new ExportScratch();
  return *static_cast<ExportScratch*>(m->ex);
}

template <typename T>
void ex_trim(DevBuf<T>& b, bool all) {
  if (all || b.cap * sizeof(T) > ((size_t)64 << 20)) b.release();   // (as smatrix_getrow_batch's row_ret: no HBM pinned for good)
}
void ex_trim_all(ExportScratch& x, bool all) {
  ex_trim(x.tcnt, all); ex_trim(x.cnt, all); ex_trim(x.got, all); ex_trim(x.ctl, all); ex_trim(x.l0, all); ex_trim(x.l1, all);
  ex_trim(x.l2, all); ex_trim(x.hist, all); ex_trim(x.tstart, all); ex_trim(x.part, all); ex_trim(x.toff, all); ex_trim(x.items, all);
  ex_trim(x.hscan, all); ex_trim(x.info, all); ex_trim(x.seg, all); ex_trim(x.tmp, all);
  ex_trim(x.h_rows, all); ex_trim(x.h_ptr, all); ex_trim(x.h_pairs, all);
}

void export_release(Matrix* m) {
  if (!m->ex) return;
  ex_trim_all(*static_cast<ExportScratch*>(m->ex), true);
  delete static_cast<ExportScratch*>(m->ex);
  m->ex = nullptr;
}

template <typename T>
T ex_read(const T* d, hipStream_t s) {
  T v;
  HIP_OK(hipMemcpyAsync(&v, d, sizeof(T), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return v;
}

// first half of an exclusive scan of n u32 counts: the tiles' sums and their prefix in x.part (x.part[nt] = the total)
uint32_t ex_scan_prep(ExportScratch& x, hipStream_t s, const uint32_t* in, uint64_t n) {
  const uint32_t nt = (uint32_t)((n + EX_TILE - 1) / EX_TILE);
  x.part.need((size_t)nt + 1);
  if (nt) hipLaunchKernelGGL(k_ex_scan_reduce, dim3(nt), dim3(EX_THREADS), 0, s, in, n, x.part.p);
  hipLaunchKernelGGL(k_ex_scan_part, dim3(1), dim3(EX_THREADS), 0, s, x.part.p, nt);
  HIP_OK(hipGetLastError());
  return nt;
}
// second half: out[0 .. n] (n + 1 entries)
void ex_scan_apply(ExportScratch& x, hipStream_t s, const uint32_t* in, uint64_t n, uint32_t nt, uint64_t* out) {
  hipLaunchKernelGGL(k_ex_scan_apply, dim3(std::max<uint32_t>(nt, 1)), dim3(EX_THREADS), 0, s, in, n, x.part.p, nt, out);
  HIP_OK(hipGetLastError());
}

// Stable LSD radix sort of nseg segments of 64-bit entries by their low word, in place in `data`, through x.tmp.  Segment b:
// cnt[b] entries at data + off[b], staged at x.tmp + toffs[b]; tiles tstart[b] .. tstart[b+1].  Host arrays: copied here.
void ex_radix(ExportScratch& x, hipStream_t s, uint64_t* data, const std::vector<uint64_t>& off, const std::vector<uint64_t>& cnt) {
  const uint32_t nseg = (uint32_t)off.size();
  if (!nseg) return;
  std::vector<uint64_t> seg(3 * (size_t)nseg);
  std::vector<uint32_t> tstart((size_t)nseg + 1);
  uint64_t staged = 0, tiles = 0;
  for (uint32_t b = 0; b < nseg; b++) {
    seg[b] = off[b]; seg[nseg + b] = staged; seg[2 * (size_t)nseg + b] = cnt[b];
    tstart[b] = (uint32_t)tiles;
    staged += cnt[b];
    tiles += (cnt[b] + EX_TILE - 1) / EX_TILE;
  }
  tstart[nseg] = (uint32_t)tiles;
  if (tiles >= (1ull << 32) / 256) smx_die("export: too many entries to sort");
  const uint32_t nt = (uint32_t)tiles;
  x.seg.need(seg.size()); x.tstart.need(tstart.size()); x.tmp.need(std::max<uint64_t>(staged, 1));
  x.hist.need(256ull * nt); x.hscan.need(256ull * nt + 1);
  HIP_OK(hipMemcpyAsync(x.seg.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(x.tstart.p, tstart.data(), tstart.size() * 4, hipMemcpyHostToDevice, s));
  const uint64_t *doff = x.seg.p, *toff = x.seg.p + nseg, *dcnt = x.seg.p + 2 * (size_t)nseg;
  for (uint32_t pass = 0; pass < 4; pass++) {                     // data -> tmp -> data -> tmp -> data
    const bool fwd = (pass & 1u) == 0;
    const uint64_t* from = fwd ? data : x.tmp.p;
    uint64_t* to = fwd ? x.tmp.p : data;
    const uint64_t *foff = fwd ? doff : toff, *tofs = fwd ? toff : doff;
    hipLaunchKernelGGL(k_ex_rs_hist, dim3(nt), dim3(EX_THREADS), 0, s, from, foff, dcnt, x.tstart.p, nseg, 8 * pass, x.hist.p);
    HIP_OK(hipGetLastError());
    const uint32_t ht = ex_scan_prep(x, s, x.hist.p, 256ull * nt);
    ex_scan_apply(x, s, x.hist.p, 256ull * nt, ht, x.hscan.p);
    hipLaunchKernelGGL(k_ex_rs_scatter, dim3(nt), dim3(EX_THREADS), 0, s, from, foff, to, tofs, dcnt, x.tstart.p, nseg, 8 * pass,
                       x.hscan.p);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipStreamSynchronize(s));                                // (the host arrays above are the sources of the copies)
}

// step 1: the row list in x.items; returns the number of rows
uint64_t ex_row_list(Matrix* m, ExportScratch& x, int order, hipStream_t s) {
  const uint32_t dsz = m->dir_size;
  const uint32_t ntd = (dsz + EX_TILE - 1) / EX_TILE;
  x.tcnt.need(ntd); x.toff.need((size_t)ntd + 1);
  hipLaunchKernelGGL(k_ex_dir_count, dim3(ntd), dim3(EX_THREADS), 0, s, m->d_dir, dsz, x.tcnt.p);
  HIP_OK(hipGetLastError());
  const uint32_t nt = ex_scan_prep(x, s, x.tcnt.p, ntd);
  ex_scan_apply(x, s, x.tcnt.p, ntd, nt, x.toff.p);
  const uint64_t n = ex_read(x.toff.p + ntd, s);
  x.cnt_tiles = 0;
  if (n) {
    x.items.need(n);
    hipLaunchKernelGGL(k_ex_dir_write, dim3(ntd), dim3(EX_THREADS), 0, s, m->d_dir, dsz, x.toff.p, x.items.p);
    HIP_OK(hipGetLastError());
    if (order == SMATRIX_EXPORT_SORTED && n > 1) ex_radix(x, s, x.items.p, {0}, {n});
  }
  return n;
}

// steps 1 and 2: the row list and the counts in scratch; *n_out / *nnz_out = rows / pairs
void ex_measure(Matrix* m, ExportScratch& x, int order, hipStream_t s, uint64_t* n_out, uint64_t* nnz_out) {
  const uint64_t n = ex_row_list(m, x, order, s);
  uint64_t nnz = 0;
  if (n) {
    x.cnt.need(n); x.l0.need(n + 1);                              // l0: the rows of more than GETROW_WAVE_MAX cells
    HIP_OK(hipMemsetAsync(x.l0.p, 0, 4, s));
    hipLaunchKernelGGL(k_ex_count, dim3(std::min<uint32_t>(blocks_for(n * 64), 16384)), dim3(EX_THREADS), 0, s, m->d_dir,
                       m->arena.base, (uint32_t)n, x.items.p, x.cnt.p, x.l0.p);
    hipLaunchKernelGGL(k_ex_count_big, dim3(512), dim3(1024), 0, s, m->d_dir, m->arena.base, x.items.p, x.cnt.p, x.l0.p);
    HIP_OK(hipGetLastError());
    x.cnt_tiles = ex_scan_prep(x, s, x.cnt.p, n);
    nnz = ex_read(x.part.p + x.cnt_tiles, s);
  }
  *n_out = n;
  *nnz_out = nnz;
}

// steps 3 and 4 into the caller's device arrays (room checked by the caller); returns after the stream has finished
void ex_write(Matrix* m, ExportScratch& x, int order, hipStream_t s, uint64_t n, uint64_t nnz, uint32_t* d_rows, uint64_t* d_row_ptr,
              uint32_t* d_pairs) {
  if (!n) {
    HIP_OK(hipMemsetAsync(d_row_ptr, 0, 8, s));
    HIP_OK(hipStreamSynchronize(s));
    return;
  }
  ex_scan_apply(x, s, x.cnt.p, n, x.cnt_tiles, d_row_ptr);
  hipLaunchKernelGGL(k_ex_rows, dim3(blocks_for(n)), dim3(256), 0, s, (uint32_t)n, x.items.p, d_rows);
  HIP_OK(hipGetLastError());
  x.got.need(n); x.ctl.need(4);
  HIP_OK(hipMemsetAsync(x.ctl.p, 0, 16, s));
  uint64_t* pairs = reinterpret_cast<uint64_t*>(d_pairs);
  launch_getrow(m, s, (uint32_t)n, d_rows, d_row_ptr, pairs, x.got.p);
  hipLaunchKernelGGL(k_ex_check, dim3(blocks_for(n)), dim3(256), 0, s, (uint32_t)n, x.cnt.p, x.got.p, x.ctl.p + 3);
  HIP_OK(hipGetLastError());
  if (order == SMATRIX_EXPORT_SORTED && nnz) {
    const uint64_t cap1 = std::min<uint64_t>(n, nnz / (EX_LDS_SMALL + 1) + 1), cap2 = std::min<uint64_t>(n, nnz / (EX_LDS_MID + 1) + 1);
    x.l0.need(n); x.l1.need(cap1); x.l2.need(cap2);
    hipLaunchKernelGGL(k_ex_classify, dim3(blocks_for(n)), dim3(256), 0, s, (uint32_t)n, d_row_ptr, x.ctl.p, x.l0.p, x.l1.p, x.l2.p);
    HIP_OK(hipGetLastError());
    uint32_t c[4];
    HIP_OK(hipMemcpyAsync(c, x.ctl.p, 16, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (c[0]) hipLaunchKernelGGL((k_ex_sort_lds<64, EX_LDS_SMALL>), dim3(std::min<uint32_t>(c[0], 65536)), dim3(64), 0, s, x.l0.p, x.ctl.p, 0u,
                                 d_row_ptr, pairs);
    if (c[1]) hipLaunchKernelGGL((k_ex_sort_lds<256, EX_LDS_MID>), dim3(std::min<uint32_t>(c[1], 8192)), dim3(256), 0, s, x.l1.p, x.ctl.p, 1u,
                                 d_row_ptr, pairs);
    HIP_OK(hipGetLastError());
    if (c[2]) {                                                   // the long rows: (offset, count) each, in row order
      x.info.need(2 * (size_t)c[2]);
      hipLaunchKernelGGL(k_ex_big_info, dim3(blocks_for(c[2])), dim3(256), 0, s, c[2], x.l2.p, d_row_ptr, x.info.p);
      HIP_OK(hipGetLastError());
      std::vector<uint64_t> info(2 * (size_t)c[2]);
      HIP_OK(hipMemcpyAsync(info.data(), x.info.p, info.size() * 8, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      std::vector<std::pair<uint64_t, uint64_t>> rows(c[2]);
      for (uint32_t i = 0; i < c[2]; i++) rows[i] = {info[2 * i], info[2 * i + 1]};
      std::sort(rows.begin(), rows.end());                      // (the list's order came from atomics; the layout of tmp does not)
      std::vector<uint64_t> off(c[2]), cnt(c[2]);
      for (uint32_t i = 0; i < c[2]; i++) { off[i] = rows[i].first; cnt[i] = rows[i].second; }
      ex_radix(x, s, pairs, off, cnt);
    }
  }
  const uint32_t bad = ex_read(x.ctl.p + 3, s);                   // (synchronises the stream)
  if (bad) smx_die("export: getrow wrote a different number of pairs than the export counted");
}

}  // namespace

extern "C" {

int smatrix_export_dev(smatrix_t* self, int order, uint64_t cap_rows, uint64_t cap_nnz, uint32_t* d_rows, uint64_t* d_row_ptr,
                       uint32_t* d_pairs, uint64_t* n_rows, uint64_t* nnz, void* hip_stream) {
  if (order != SMATRIX_EXPORT_TABLE && order != SMATRIX_EXPORT_SORTED) return -1;
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
  ExportScratch& x = ex_of(m);
  uint64_t n = 0, z = 0;
  ex_measure(m, x, order, s, &n, &z);
  if (n_rows) *n_rows = n;
  if (nnz) *nnz = z;
  int rc = 0;
  if (d_row_ptr && (n > cap_rows || z > cap_nnz)) rc = 1;
  else if (d_row_ptr) ex_write(m, x, order, s, n, z, d_rows, d_row_ptr, d_pairs);
  ex_trim_all(x, false);
  return rc;
}

int smatrix_export(smatrix_t* self, int order, uint64_t cap_rows, uint64_t cap_nnz, uint32_t* rows, uint64_t* row_ptr, uint32_t* pairs,
                   uint64_t* n_rows, uint64_t* nnz) {
  if (order != SMATRIX_EXPORT_TABLE && order != SMATRIX_EXPORT_SORTED) return -1;
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = m->stream;
  ExportScratch& x = ex_of(m);
  uint64_t n = 0, z = 0;
  ex_measure(m, x, order, s, &n, &z);
  if (n_rows) *n_rows = n;
  if (nnz) *nnz = z;
  int rc = 0;
  if (row_ptr && (n > cap_rows || z > cap_nnz)) rc = 1;
  else if (row_ptr) {
    x.h_rows.need(std::max<uint64_t>(n, 1)); x.h_ptr.need(n + 1); x.h_pairs.need(std::max<uint64_t>(z, 1));
    ex_write(m, x, order, s, n, z, x.h_rows.p, x.h_ptr.p, reinterpret_cast<uint32_t*>(x.h_pairs.p));
    if (n) HIP_OK(hipMemcpyAsync(rows, x.h_rows.p, n * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(row_ptr, x.h_ptr.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (z) HIP_OK(hipMemcpyAsync(pairs, x.h_pairs.p, z * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
  }
  ex_trim_all(x, false);
  return rc;
}

}  // extern "C"
