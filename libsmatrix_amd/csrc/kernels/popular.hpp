// kernels/popular.hpp -- the most popular items (include/smatrix_batch.h smatrix_cf_popular): the n ids with the largest column-0
// totals over the WHOLE directory, chosen on the device with no read-back.  Host side: smx_popular.inc.
// A fragment of smx_kernels.hpp: included there, after merge.hpp (mgt_hist_add, mgt_pick, mg_wave_or, mg_wave_sum) and recommend.hpp
// (RecFilt, rec_denied: the deny bitmap is the filtered call's), INSIDE namespace smx.
//
// A candidate's key is RkValue::make(x, total) of kernels/rank_key.hpp -- total descending, equal totals by ascending id, unique --
// and the selection is merge.hpp's per-row MSB radix select with the row replaced by one dense array of a key per directory slot:
//   k_pop_keys      a lane per directory slot: the key of a present row x != 0 whose head cell passes min_total and the deny
//                   bitmap, 0 for anything else; the OR of the keys and their number, one atomic each per workgroup
//   k_pop_start     one lane: fewer than n + 1 candidates -> the threshold is "every non-zero key", done; else RkValue::start
//   k_pop_hist      per pass, streaming: a 256-bin LDS histogram of the digit of the keys that agree with the prefix, added to the
//                   pass's global histogram with one add per non-empty bin per workgroup
//   k_pop_pick      per pass, one wave: mgt_pick on the global histogram; prefix, digit and the keys still needed stay in PopCtl.
//                   The select ends at digit 0 or as soon as the chosen bin holds exactly the keys still needed: the prefix with
//                   zeros below it is then a threshold that no key undercuts (a bin of one key is that case)
//   k_pop_collect   keys >= threshold -> an n-entry buffer: a ballot per wave, ONE atomic add per workgroup that takes any
//   k_pop_sort      one workgroup: the buffer (<= 4096 keys, 32 KiB of LDS) sorted by a bitonic network, best first -> ids, totals, n
// Every pass kernel of a finished select returns at once (PopCtl::done): the host enqueues RkValue::DIGITS passes and reads nothing.

constexpr uint32_t POP_MAX = 4096;            // SMATRIX_POPULAR_MAX: what k_pop_sort holds in LDS
constexpr uint32_t POP_SORT_THREADS = 1024;
constexpr uint32_t POP_GRID_MAX = 2048;       // workgroups of the streaming kernels (grid-stride beyond)

struct PopCtl {                               // zeroed by the host before k_pop_keys
  uint32_t acc[2];                            // RkValue::Acc: the OR of the keys
  uint32_t n_cand;                            // the non-zero keys
  uint32_t n_out;                             // keys collected (k_pop_collect's counter)
  uint32_t dg, need, done, pad;               // the next pass's digit; keys still to take among those that agree with the prefix
  unsigned long long prefix, pad2;            // done: the threshold
  uint32_t hist[RkValue::DIGITS][256];        // a histogram per pass: none is zeroed between passes
};
static_assert(offsetof(PopCtl, hist) % 16 == 0, "mgt_pick reads four bins per lane");

__global__ __launch_bounds__(256) void k_pop_keys(DirSlot* dir, uint32_t dir_size, uint8_t* arena, RecFilt f, uint32_t min_total,
                                                  unsigned long long* __restrict__ keys, PopCtl* ctl) {
  __shared__ uint32_t w_acc[3][4];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  RkValue::Acc a = RkValue::acc0();
  uint32_t cnt = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < dir_size; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[i]);       // {meta, x, base, used}
    RkValue::Key key = RkValue::zero();
    if ((s.x & META_USED) && s.y != 0 && s.z != 0 && !rec_denied(f, s.y)) {
      bool dummy = false;
      const uint32_t t = apply_row<OP_GET>(&dir[i], s, arena, 0u, 0u, 0u, &dummy, nullptr);   // smatrix_get(x, 0)
      if (t != 0 && t >= min_total) key = RkValue::make(s.y, t);
    }
    keys[i] = key;
    RkValue::acc_add(a, key);
    cnt += !RkValue::is_zero(key);
  }
  a.w[0] = mg_wave_or(a.w[0]); a.w[1] = mg_wave_or(a.w[1]); cnt = mg_wave_sum(cnt);
  if (lane == 0) { w_acc[0][w] = a.w[0]; w_acc[1][w] = a.w[1]; w_acc[2][w] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t hi = w_acc[0][0] | w_acc[0][1] | w_acc[0][2] | w_acc[0][3], lo = w_acc[1][0] | w_acc[1][1] | w_acc[1][2] | w_acc[1][3];
    const uint32_t c = w_acc[2][0] + w_acc[2][1] + w_acc[2][2] + w_acc[2][3];
    if (c) { atomicOr(&ctl->acc[0], hi); atomicOr(&ctl->acc[1], lo); atomicAdd(&ctl->n_cand, c); }
  }
}

__global__ __launch_bounds__(64) void k_pop_start(PopCtl* ctl, uint32_t n) {
  if (threadIdx.x != 0) return;
  if (ctl->n_cand <= n) { ctl->prefix = RkValue::zero(); ctl->done = 1u; return; }   // every non-zero key
  const RkValue::Acc a{{ctl->acc[0], ctl->acc[1]}};
  RkValue::Key prefix;
  ctl->dg = RkValue::start(a, prefix);                                // (n + 1 keys and more: their OR is not 0)
  ctl->prefix = prefix;
  ctl->need = n;
}

__global__ __launch_bounds__(256) void k_pop_hist(const unsigned long long* __restrict__ keys, uint32_t n_keys, PopCtl* ctl, uint32_t pass) {
  __shared__ uint32_t s_hist[256];
  if (aload(&ctl->done)) return;
  const uint32_t dg = aload(&ctl->dg), lane = threadIdx.x & 63;
  const RkValue::Key prefix = ctl->prefix;
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n_keys; i0 += (uint64_t)gridDim.x * blockDim.x) {   // block-uniform: the steps hold ballots
    const uint64_t i = i0 + threadIdx.x;
    const RkValue::Key key = i < n_keys ? keys[i] : RkValue::zero();
    mgt_hist_add(s_hist, !RkValue::is_zero(key) && RkValue::agrees_above(key, prefix, dg), RkValue::digit(key, dg), lane);
  }
  __syncthreads();
  const uint32_t c = s_hist[threadIdx.x];
  if (c) atomicAdd(&ctl->hist[pass][threadIdx.x], c);
}

__global__ __launch_bounds__(64) void k_pop_pick(PopCtl* ctl, uint32_t pass) {
  if (aload(&ctl->done)) return;
  uint32_t d, above, bucket;
  mgt_pick<false>(ctl->hist[pass], ctl->need, threadIdx.x, d, above, bucket);
  if (threadIdx.x != 0) return;
  const uint32_t dg = ctl->dg, need = ctl->need - above;
  RkValue::Key prefix = ctl->prefix;
  RkValue::take_digit(prefix, dg, d);
  ctl->prefix = prefix;
  ctl->need = need;
  if (dg == 0 || bucket == need) ctl->done = 1u;                      // every key of the bin is wanted: nothing below decides
  else ctl->dg = dg - 1;
}

__global__ __launch_bounds__(256) void k_pop_collect(const unsigned long long* __restrict__ keys, uint32_t n_keys, PopCtl* ctl, uint32_t n,
                                                     unsigned long long* __restrict__ out) {
  __shared__ uint32_t w_cnt[4], s_base;
  const RkValue::Key thr = ctl->prefix;
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n_keys; i0 += (uint64_t)gridDim.x * blockDim.x) {   // block-uniform
    const uint64_t i = i0 + threadIdx.x;
    const RkValue::Key key = i < n_keys ? keys[i] : RkValue::zero();
    const bool take = !RkValue::is_zero(key) && RkValue::ge(key, thr);
    const uint32_t total = (uint32_t)__syncthreads_count(take);
    if (total == 0) continue;                                         // (nearly every step: n of all the keys are taken)
    const uint64_t m = __ballot(take);
    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) w_cnt[w] = (uint32_t)__popcll(m);
    if (threadIdx.x == 0) s_base = atomicAdd(&ctl->n_out, total);
    __syncthreads();
    uint32_t at = s_base + before;
    for (uint32_t v = 0; v < w; v++) at += w_cnt[v];
    if (take && at < n) out[at] = key;                                // (the select leaves min(n, candidates) keys: never beyond)
    __syncthreads();                                                  // before the next step's counts
  }
}

__global__ __launch_bounds__(POP_SORT_THREADS) void k_pop_sort(const PopCtl* ctl, uint32_t n, const unsigned long long* __restrict__ out,
                                                               uint32_t* __restrict__ ids, uint32_t* __restrict__ totals,
                                                               uint32_t* __restrict__ n_found) {
  __shared__ unsigned long long s_key[POP_MAX];
  const uint32_t cnt = ctl->n_out < n ? ctl->n_out : n;
  uint32_t P = 64;
  while (P < cnt) P <<= 1;                                            // (n <= POP_MAX: P <= POP_MAX)
  for (uint32_t i = threadIdx.x; i < P; i += POP_SORT_THREADS) s_key[i] = i < cnt ? out[i] : 0ull;
  __syncthreads();
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < P; i += POP_SORT_THREADS) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const unsigned long long a = s_key[i], b = s_key[l];
          if ((i & k) == 0 ? a < b : a > b) { s_key[i] = b; s_key[l] = a; }   // the last stage (k == P) is descending throughout
        }
      }
      __syncthreads();
    }
  for (uint32_t i = threadIdx.x; i < cnt; i += POP_SORT_THREADS) {
    const unsigned long long key = s_key[i];
    ids[i] = 0xFFFFFFFFu - (uint32_t)key;
    totals[i] = (uint32_t)(key >> 32);
  }
  if (threadIdx.x == 0) *n_found = cnt;
}
