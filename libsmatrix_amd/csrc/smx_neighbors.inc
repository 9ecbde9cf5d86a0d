// smx_neighbors.inc -- an item's neighbours and their cosines, all or the k best (include/smatrix_batch.h smatrix_cf_neighbors_batch /
// _dev, smatrix_cf_topk_batch / _dev), host side.  Included by smx_runtime.hip inside the translation unit, after smx_recommend.inc
// (uses its call scope RecCall and its RecScratch); the device code is in kernels/rows.hpp: one launch, a wave per item.
// A _dev flavour has no scratch and opens no scope: the lock, the mirror written back, the launch on the caller's stream.  A host
// flavour is a RecCall: the items and zeroed answers in the scope's h_* buffers, the launch, the answers back, finish.  The
// neighbours' offsets are OUTPUT offsets, not a window of a list of lists: they are copied as they are, and ids / scores
// [0, offsets[n]) are the call's whole -- zeros wherever no neighbour was written, [0, offsets[0]) included.

namespace {

void nb_launch(Matrix* m, hipStream_t s, size_t n, const uint32_t* d_items, const uint64_t* d_offsets, uint32_t* d_ids, double* d_scores,
               uint32_t* d_counts) {
  uint32_t grid = std::min<uint32_t>(blocks_for((uint64_t)n * 64), 16384);
  hipLaunchKernelGGL(k_cf_neighbors, dim3(grid), dim3(256), 0, s, m->d_dir, m->dir_size - 1, m->arena.base,
                     (uint32_t)n, d_items, d_offsets, d_ids, d_scores, d_counts);
  HIP_OK(hipGetLastError());
}
void nb_launch_topk(Matrix* m, hipStream_t s, size_t n, const uint32_t* d_items, uint32_t k, uint32_t* d_ids, double* d_scores,
                    uint32_t* d_counts) {
  uint32_t grid = std::min<uint32_t>(blocks_for((uint64_t)n * 64), 16384);
  hipLaunchKernelGGL(k_cf_topk, dim3(grid), dim3(256), 0, s, m->d_dir, m->dir_size - 1, m->arena.base, (uint32_t)n, d_items, k,
                     d_ids, d_scores, d_counts);
  HIP_OK(hipGetLastError());
}

// a host flavour's items and its n_out zeroed answers in the scope's buffers (entries that no neighbour is written to read 0) ...
void nb_stage(RecCall& c, size_t n, const uint32_t* items, uint64_t n_out) {
  RecScratch& x = c.x();
  const uint64_t room = std::max<uint64_t>(n_out, 1);
  x.h_items.need(n); x.h_counts.need(n); x.h_ids.need(room); x.h_scores.need(room);
  HIP_OK(hipMemcpyAsync(x.h_items.p, items, n * 4, hipMemcpyHostToDevice, c.s));
  HIP_OK(hipMemsetAsync(x.h_ids.p, 0, room * 4, c.s));
  HIP_OK(hipMemsetAsync(x.h_scores.p, 0, room * 8, c.s));
}
// ... and the way back: counts[0 .. n), ids / scores [0 .. n_out)
int nb_finish(RecCall& c, size_t n, uint64_t n_out, uint32_t* ids, double* scores, uint32_t* counts) {
  RecScratch& x = c.x();
  HIP_OK(hipMemcpyAsync(counts, x.h_counts.p, n * 4, hipMemcpyDeviceToHost, c.s));
  if (n_out) HIP_OK(hipMemcpyAsync(ids, x.h_ids.p, n_out * 4, hipMemcpyDeviceToHost, c.s));
  if (n_out) HIP_OK(hipMemcpyAsync(scores, x.h_scores.p, n_out * 8, hipMemcpyDeviceToHost, c.s));
  return c.finish(0);
}

}  // namespace

extern "C" {

int smatrix_cf_neighbors_batch_dev(smatrix_t* self, size_t n, const uint32_t* d_items, const uint64_t* d_offsets, uint32_t* d_ids,
                                   double* d_scores, uint32_t* d_counts, void* hip_stream) {
  if (n == 0) return 0;
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
  nb_launch(m, s, n, d_items, d_offsets, d_ids, d_scores, d_counts);
  if (!hip_stream) HIP_OK(hipStreamSynchronize(s));
  return 0;
}

int smatrix_cf_neighbors_batch(smatrix_t* self, size_t n, const uint32_t* items, const uint64_t* offsets, uint32_t* ids, double* scores,
                               uint32_t* counts) {
  if (n == 0) return 0;
  RecCall c(self);
  RecScratch& x = c.x();
  nb_stage(c, n, items, offsets[n]);
  x.h_off.need(n + 1);
  HIP_OK(hipMemcpyAsync(x.h_off.p, offsets, (n + 1) * 8, hipMemcpyHostToDevice, c.s));
  nb_launch(c.m, c.s, n, x.h_items.p, x.h_off.p, x.h_ids.p, x.h_scores.p, x.h_counts.p);
  return nb_finish(c, n, offsets[n], ids, scores, counts);
}

// the k best neighbours per item (k <= 64); ids / scores hold n * k entries, item i's at [i*k, i*k + counts[i])
int smatrix_cf_topk_batch_dev(smatrix_t* self, size_t n, const uint32_t* d_items, uint32_t k, uint32_t* d_ids,
                              double* d_scores, uint32_t* d_counts, void* hip_stream) {
  if (k == 0 || k > 64) return -1;
  if (n == 0) return 0;
  Matrix* m = M(self);
  set_device(m);
  std::lock_guard<std::mutex> g(m->mu);
  cache_sync(m, false);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
  nb_launch_topk(m, s, n, d_items, k, d_ids, d_scores, d_counts);
  if (!hip_stream) HIP_OK(hipStreamSynchronize(s));
  return 0;
}

int smatrix_cf_topk_batch(smatrix_t* self, size_t n, const uint32_t* items, uint32_t k, uint32_t* ids, double* scores,
                          uint32_t* counts) {
  if (k == 0 || k > 64) return -1;
  if (n == 0) return 0;
  RecCall c(self);
  RecScratch& x = c.x();
  nb_stage(c, n, items, (uint64_t)n * k);
  nb_launch_topk(c.m, c.s, n, x.h_items.p, k, x.h_ids.p, x.h_scores.p, x.h_counts.p);
  return nb_finish(c, n, (uint64_t)n * k, ids, scores, counts);
}

}  // extern "C"
