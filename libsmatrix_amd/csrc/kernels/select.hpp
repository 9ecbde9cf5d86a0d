// kernels/select.hpp -- the n largest of one dense array of rank keys, a key per directory slot, chosen on the device with no
// read-back: the selection of smatrix_cf_popular (kernels/popular.hpp) and smatrix_cf_trending (kernels/trending.hpp), written once
// over the key policy P of kernels/rank_key.hpp.  Host side: sel_run in smx_popular.inc.
// A fragment of smx_kernels.hpp: included there after merge.hpp (mgt_hist_add, mgt_pick, mg_wave_or, mg_wave_sum) and recommend.hpp,
// before the list-makers, INSIDE namespace smx.
//
// It is merge.hpp's per-row MSB radix select with the row replaced by the array.  A list-maker writes a key kernel -- a lane per
// slot, P::zero() for a slot that holds no candidate, sel_store, and sel_publish as its tail -- and a sort kernel with its own LDS
// layout and emission around sel_bitonic; between the two the host enqueues
//   k_sel_start<P>    one lane: fewer than n + 1 candidates -> the threshold is "every non-zero key", done; else P::start -- the
//                     first digit that can decide, the digits above it as the prefix
//   k_sel_hist<P>     per pass, streaming: a 256-bin LDS histogram of the digit of the keys that agree with the prefix, added to the
//                     pass's global histogram with one add per non-empty bin per workgroup
//   k_sel_pick<P>     per pass, one wave: mgt_pick on the global histogram; prefix, digit and the keys still needed stay in SelCtl.
//                     The select ends at digit 0 or as soon as the chosen bin holds exactly the keys still needed: the prefix with
//                     zeros below it is then a threshold that no key undercuts (a bin of one key is that case)
//   k_sel_collect<P>  keys >= threshold -> an n-entry buffer: a ballot per wave, ONE atomic add per workgroup that takes any
// Every pass kernel of a finished select returns at its first load (SelCtl::done): the host enqueues P::DIGITS passes and reads nothing.
//
// Keys in memory, two layouts in one uint32_t array of P::W * n_keys words (sel_load / sel_store are the only code that knows):
//   a Key that is a plain uint64_t (RkValue) is stored whole, key i at byte 8 i (hipMalloc's alignment covers the access): one
//     address pair and one 8-byte load per lane -- k_sel_hist<RkValue> sits exactly on its bound of 16 VGPRs, and a second plane
//     would cost a second address pair there and change the popular call's memory traffic
//   any other Key (RkCosine) as P::W planes of 32-bit words, word w of key i at [w * n_keys + i] (P::or_words / P::from_words name
//     the words): a wave's load of one plane is 256 contiguous bytes whatever P::W is; a 12-byte array of structures would straddle.

constexpr uint32_t POP_MAX = 4096;            // SMATRIX_POPULAR_MAX: what a sort kernel holds in LDS
constexpr uint32_t POP_SORT_THREADS = 1024;
constexpr uint32_t POP_GRID_MAX = 2048;       // workgroups of the streaming kernels (grid-stride beyond)

template <typename P>
struct SelCtl {                               // zeroed by the host before the key kernel
  static constexpr uint32_t AW = sizeof(typename P::Acc) / 4;
  uint32_t acc[8];                            // P::Acc, word for word
  uint32_t n_cand;                            // the non-zero keys
  uint32_t n_out;                             // keys collected (k_sel_collect's counter)
  uint32_t dg, need, done, pad[3];            // the next pass's digit; keys still to take among those that agree with the prefix
  uint32_t prefix[4];                         // P::W words; done: the threshold
  uint32_t hist[P::DIGITS][256];              // a histogram per pass: none is zeroed between passes
  static_assert(AW <= 8 && P::W <= 4, "the control block holds 8 words of Acc and 4 of a key");
};
static_assert(offsetof(SelCtl<RkCosine>, hist) % 16 == 0 && offsetof(SelCtl<RkValue>, hist) % 16 == 0, "mgt_pick reads four bins per lane");

template <typename P>
constexpr bool sel_whole = std::is_same<typename P::Key, uint64_t>::value;

template <typename P>
__device__ __forceinline__ typename P::Key sel_load(const uint32_t* __restrict__ keys, uint64_t n_keys, uint64_t i) {
  if constexpr (sel_whole<P>) return reinterpret_cast<const uint64_t*>(keys)[i];
  else {
    uint32_t w[P::W];
#pragma unroll
    for (uint32_t k = 0; k < P::W; k++) w[k] = keys[k * n_keys + i];
    return P::from_words(w);
  }
}
template <typename P>
__device__ __forceinline__ void sel_store(uint32_t* __restrict__ keys, uint64_t n_keys, uint64_t i, typename P::Key key) {
  if constexpr (sel_whole<P>) reinterpret_cast<uint64_t*>(keys)[i] = key;
  else {
    uint32_t w[P::W] = {};
    P::or_words(w, key);
#pragma unroll
    for (uint32_t k = 0; k < P::W; k++) keys[k * n_keys + i] = w[k];
  }
}
template <typename P>
__device__ __forceinline__ typename P::Key sel_prefix(const SelCtl<P>* ctl) {
  uint32_t w[P::W];
#pragma unroll
  for (uint32_t k = 0; k < P::W; k++) w[k] = ctl->prefix[k];
  return P::from_words(w);
}
template <typename P>
__device__ __forceinline__ void sel_set_prefix(SelCtl<P>* ctl, typename P::Key prefix) {
  uint32_t w[P::W] = {};
  P::or_words(w, prefix);
#pragma unroll
  for (uint32_t k = 0; k < P::W; k++) ctl->prefix[k] = w[k];
}

// The tail of a key kernel (256 lanes, every lane arrives): `a` = the lane's P::Acc over its NON-ZERO keys (a zero key would empty
// RkCosine's AND of the keys), `cnt` their number -> SelCtl, one atomic per word and per workgroup that holds a candidate.
template <typename P>
__device__ __forceinline__ void sel_publish(SelCtl<P>* ctl, typename P::Acc a, uint32_t cnt) {
  constexpr uint32_t AW = SelCtl<P>::AW;
  __shared__ uint32_t w_acc[AW + 1][4];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t k = 0; k < AW; k++) a.w[k] = mg_wave_or(a.w[k]);
  cnt = mg_wave_sum(cnt);
  if (lane == 0) {
    for (uint32_t k = 0; k < AW; k++) w_acc[k][w] = a.w[k];
    w_acc[AW][w] = cnt;
  }
  __syncthreads();
  if (threadIdx.x <= AW && (w_acc[AW][0] | w_acc[AW][1] | w_acc[AW][2] | w_acc[AW][3])) {   // lane k: word k; lane AW: the count
    const uint32_t* v = w_acc[threadIdx.x];
    if (threadIdx.x < AW) atomicOr(&ctl->acc[threadIdx.x], v[0] | v[1] | v[2] | v[3]);
    else atomicAdd(&ctl->n_cand, v[0] + v[1] + v[2] + v[3]);
  }
}

template <typename P>
__global__ __launch_bounds__(64) void k_sel_start(SelCtl<P>* ctl, uint32_t n) {
  if (threadIdx.x != 0) return;
  if (ctl->n_cand <= n) { sel_set_prefix<P>(ctl, P::zero()); ctl->done = 1u; return; }   // every non-zero key
  typename P::Acc a;
  for (uint32_t k = 0; k < SelCtl<P>::AW; k++) a.w[k] = ctl->acc[k];
  typename P::Key prefix;
  ctl->dg = P::start(a, prefix);                                      // (n + 1 keys and more, all different)
  sel_set_prefix<P>(ctl, prefix);
  ctl->need = n;
}

template <typename P>
__global__ __launch_bounds__(256) void k_sel_hist(const uint32_t* __restrict__ keys, uint32_t n_keys, SelCtl<P>* ctl, uint32_t pass) {
  __shared__ uint32_t s_hist[256];
  if (aload(&ctl->done)) return;
  const uint32_t dg = aload(&ctl->dg), lane = threadIdx.x & 63;
  const typename P::Key prefix = sel_prefix<P>(ctl);
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n_keys; i0 += (uint64_t)gridDim.x * blockDim.x) {   // block-uniform: the steps hold ballots
    const uint64_t i = i0 + threadIdx.x;
    const typename P::Key key = i < n_keys ? sel_load<P>(keys, n_keys, i) : P::zero();
    mgt_hist_add(s_hist, !P::is_zero(key) && P::agrees_above(key, prefix, dg), P::digit(key, dg), lane);
  }
  __syncthreads();
  const uint32_t c = s_hist[threadIdx.x];
  if (c) atomicAdd(&ctl->hist[pass][threadIdx.x], c);
}

template <typename P>
__global__ __launch_bounds__(64) void k_sel_pick(SelCtl<P>* ctl, uint32_t pass) {
  if (aload(&ctl->done)) return;
  uint32_t d, above, bucket;
  mgt_pick<false>(ctl->hist[pass], ctl->need, threadIdx.x, d, above, bucket);
  if (threadIdx.x != 0) return;
  const uint32_t dg = ctl->dg, need = ctl->need - above;
  typename P::Key prefix = sel_prefix<P>(ctl);
  P::take_digit(prefix, dg, d);
  sel_set_prefix<P>(ctl, prefix);
  ctl->need = need;
  if (dg == 0 || bucket == need) ctl->done = 1u;                      // every key of the bin is wanted: nothing below decides
  else ctl->dg = dg - 1;
}

template <typename P>
__global__ __launch_bounds__(256) void k_sel_collect(const uint32_t* __restrict__ keys, uint32_t n_keys, SelCtl<P>* ctl, uint32_t n,
                                                     uint32_t* __restrict__ out) {
  __shared__ uint32_t w_cnt[4], s_base;
  const typename P::Key thr = sel_prefix<P>(ctl);
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n_keys; i0 += (uint64_t)gridDim.x * blockDim.x) {   // block-uniform
    const uint64_t i = i0 + threadIdx.x;
    const typename P::Key key = i < n_keys ? sel_load<P>(keys, n_keys, i) : P::zero();
    const bool take = !P::is_zero(key) && P::ge(key, thr);
    const uint32_t total = (uint32_t)__syncthreads_count(take);
    if (total == 0) continue;                                         // (nearly every step: n of all the keys are taken)
    const uint64_t m = __ballot(take);
    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) w_cnt[w] = (uint32_t)__popcll(m);
    if (threadIdx.x == 0) s_base = atomicAdd(&ctl->n_out, total);
    __syncthreads();
    uint32_t at = s_base + before;
    for (uint32_t v = 0; v < w; v++) at += w_cnt[v];
    if (take && at < n) sel_store<P>(out, n, at, key);                // (the select leaves min(n, candidates) keys: never beyond)
    __syncthreads();                                                  // before the next step's counts
  }
}

// The network of a sort kernel: one workgroup of POP_SORT_THREADS lanes sorts Q keys (a power of two >= 64, the buffer padded with
// P::zero()) descending by P::ge, in the caller's LDS through get(i) -> Key and put(i, Key); the caller synchronises before it.
template <typename P, typename Get, typename Put>
__device__ __forceinline__ void sel_bitonic(uint32_t Q, Get get, Put put) {
  for (uint32_t k = 2; k <= Q; k <<= 1)
    for (uint32_t j = k >> 1; j; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < Q; i += POP_SORT_THREADS) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const typename P::Key a = get(i), b = get(l);
          if ((i & k) == 0 ? !P::ge(a, b) : !P::ge(b, a)) { put(i, b); put(l, a); }   // the last stage (k == Q) is descending throughout
        }
      }
      __syncthreads();
    }
}
