// kernels/popular.hpp -- the most popular items (include/smatrix_batch.h smatrix_cf_popular): the n ids with the largest column-0
// totals over the WHOLE directory, chosen on the device with no read-back.  Host side: smx_popular.inc.
// A fragment of smx_kernels.hpp: included there after select.hpp (the dense select and its limits) and recommend.hpp (RecFilt,
// rec_denied: the deny bitmap is the filtered call's), INSIDE namespace smx.
//
// A candidate's key is RkValue::make(x, total) of kernels/rank_key.hpp -- total descending, equal totals by ascending id, unique --
// and the selection is select.hpp's over 64-bit keys stored whole:
//   k_pop_keys               a lane per directory slot: the key of a present row x != 0 whose head cell passes min_total and the
//                            deny bitmap, 0 for anything else; the OR of the keys and their number through sel_publish
//   k_sel_start<RkValue>, RkValue::DIGITS times (k_sel_hist<RkValue>, k_sel_pick<RkValue>), k_sel_collect<RkValue>
//   k_pop_sort               one workgroup: the buffer (<= 4096 keys, 32 KiB of LDS) sorted by sel_bitonic, best first -> ids, totals, n

__global__ __launch_bounds__(256) void k_pop_keys(DirSlot* dir, uint32_t dir_size, uint8_t* arena, RecFilt f, uint32_t min_total,
                                                  uint32_t* __restrict__ keys, SelCtl<RkValue>* ctl) {
  typedef RkValue P;
  P::Acc a = P::acc0();
  uint32_t cnt = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < dir_size; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[i]);       // {meta, x, base, used}
    P::Key key = P::zero();
    if ((s.x & META_USED) && s.y != 0 && s.z != 0 && !rec_denied(f, s.y)) {
      bool dummy = false;
      const uint32_t t = apply_row<OP_GET>(&dir[i], s, arena, 0u, 0u, 0u, &dummy, nullptr);   // smatrix_get(x, 0)
      if (t != 0 && t >= min_total) key = P::make(s.y, t);
    }
    sel_store<P>(keys, dir_size, i, key);
    if (!P::is_zero(key)) { P::acc_add(a, key); cnt++; }
  }
  sel_publish<P>(ctl, a, cnt);
}

__global__ __launch_bounds__(POP_SORT_THREADS) void k_pop_sort(const SelCtl<RkValue>* ctl, uint32_t n, const uint32_t* __restrict__ out,
                                                               uint32_t* __restrict__ ids, uint32_t* __restrict__ totals,
                                                               uint32_t* __restrict__ n_found) {
  typedef RkValue P;
  __shared__ P::Key s_key[POP_MAX];
  const uint32_t cnt = ctl->n_out < n ? ctl->n_out : n;
  uint32_t Q = 64;
  while (Q < cnt) Q <<= 1;                                            // (n <= POP_MAX: Q <= POP_MAX)
  for (uint32_t i = threadIdx.x; i < Q; i += POP_SORT_THREADS) s_key[i] = i < cnt ? sel_load<P>(out, n, i) : P::zero();
  __syncthreads();
  sel_bitonic<P>(Q, [&](uint32_t i) { return s_key[i]; }, [&](uint32_t i, P::Key key) { s_key[i] = key; });
  for (uint32_t i = threadIdx.x; i < cnt; i += POP_SORT_THREADS) {
    const P::Key key = s_key[i];
    ids[i] = 0xFFFFFFFFu - (uint32_t)key;
    totals[i] = (uint32_t)(key >> 32);
  }
  if (threadIdx.x == 0) *n_found = cnt;
}
