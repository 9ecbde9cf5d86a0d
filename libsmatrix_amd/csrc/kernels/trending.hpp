// kernels/trending.hpp -- the trending items (include/smatrix_batch.h smatrix_cf_trending): the n ids whose column-0 totals in one
// matrix (`now`) grew most against a scaled baseline from a second one (`base`), chosen on the device with no read-back.  Host side:
// smx_trending.inc.
// A fragment of smx_kernels.hpp: included there after popular.hpp (POP_MAX, POP_SORT_THREADS, POP_GRID_MAX: the limits are the
// popular call's), merge.hpp (mgt_hist_add, mgt_pick, mg_wave_or, mg_wave_sum) and recommend.hpp (RecFilt, rec_denied), INSIDE
// namespace smx.
//
// A candidate x has T = get(now, x, 0), B = get(base, x, 0), E = floor(B * num / den) and the gain G = T - E > 0; its score is G,
// G / D or G / sqrt(D) with D = E + shrink (0 counted as 1), an IEEE double > 0, and its key RkCosine::make(x, the score's bits) of
// kernels/rank_key.hpp: score descending, equal scores by ascending id, unique.  The selection is popular.hpp's, step for step,
// over 96-bit keys -- written over the key policy P (the interface in rank_key.hpp) and instantiated for RkCosine alone:
//   k_trend_keys      a lane per slot of now's directory: the head-cell total, ONE look-up of x in base's directory, the score, the
//                     key; P::zero() for anything that is no candidate.  The keys' P::Acc (the OR of the keys and of their
//                     complements) and their number, one atomic per word and per workgroup that holds a candidate
//   k_sel_start<P>    one lane: fewer than n + 1 candidates -> the threshold is "every non-zero key", done; else P::start -- the
//                     highest digit in which the keys differ, the digits above it as the prefix
//   k_sel_hist<P>     per pass, streaming: a 256-bin LDS histogram of the digit of the keys that agree with the prefix
//   k_sel_pick<P>     per pass, one wave: mgt_pick; ends the select at digit 0 or when the chosen bin holds exactly the keys needed
//   k_sel_collect<P>  keys >= threshold -> an n-entry buffer, ONE atomic add per workgroup that takes any
//   k_trend_sort      one workgroup: the buffer (<= 4096 keys, 48 KiB of LDS) sorted by a bitonic network on P::ge, best first; ids
//                     and scores decoded, T and E looked up again per result entry (no payload rides through the sort)
// Every pass kernel of a finished select returns at its first load (SelCtl::done): the host enqueues P::DIGITS passes and reads nothing.
//
// Keys in memory: P::W planes of 32-bit words in one array, word w of key i at [w * n_keys + i] (P::or_words / P::from_words name
// the words).  A wave's load of one plane is 256 contiguous bytes whatever P::W is; a 12-byte array of structures would straddle.

constexpr int TREND_GAIN = 0, TREND_RATIO = 1, TREND_ZSCORE = 2;   // SMATRIX_TREND_*

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
static_assert(offsetof(SelCtl<RkCosine>, hist) % 16 == 0, "mgt_pick reads four bins per lane");

template <typename P>
__device__ __forceinline__ typename P::Key sel_load(const uint32_t* __restrict__ keys, uint64_t n_keys, uint64_t i) {
  uint32_t w[P::W];
#pragma unroll
  for (uint32_t k = 0; k < P::W; k++) w[k] = keys[k * n_keys + i];
  return P::from_words(w);
}
template <typename P>
__device__ __forceinline__ void sel_store(uint32_t* __restrict__ keys, uint64_t n_keys, uint64_t i, typename P::Key key) {
  uint32_t w[P::W] = {};
  P::or_words(w, key);
#pragma unroll
  for (uint32_t k = 0; k < P::W; k++) keys[k * n_keys + i] = w[k];
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

// what smatrix_cf_trending adds to the popular call's arguments
struct TrendArgs {
  DirSlot* b_dir;                             // base's directory and arena
  uint32_t b_mask;
  uint8_t* b_arena;
  int measure;                                // TREND_*
  uint32_t num, den;                          // 1 <= num <= den: E = floor(B * num / den), smatrix_merge_scaled's transform
  double shrink;                              // finite, >= 0 (-0.0 acts as 0.0: E + -0.0 is never -0.0)
  uint32_t min_total, min_gain;
};

__device__ __forceinline__ uint32_t trend_expected(const TrendArgs& t, uint32_t x) {
  bool dummy = false;
  const uint32_t b = apply_one<OP_GET>(t.b_dir, t.b_mask, t.b_arena, x, 0u, 0u, &dummy);     // smatrix_get(base, x, 0): 0 without a row
  return (uint32_t)((uint64_t)b * t.num / t.den);                                            // (num <= den: fits)
}
// the score of a gain g >= 1 over e expected: each operation rounded on its own, finite and > 0
__device__ __forceinline__ uint64_t trend_score_bits(int measure, double shrink, uint32_t g, uint32_t e) {
#pragma clang fp contract(off)
  double d = (double)e + shrink;
  if (d == 0.0) d = 1.0;                                              // (a new item with shrink 0: the read path's tb == 0 -> 1)
  const double G = (double)g;
  const double score = measure == TREND_GAIN ? G : measure == TREND_RATIO ? G / d : G / sqrt(d);
  return (uint64_t)__double_as_longlong(score);
}

__global__ __launch_bounds__(256) void k_trend_keys(DirSlot* dir, uint32_t dir_size, uint8_t* arena, RecFilt f, TrendArgs t,
                                                    uint32_t* __restrict__ keys, SelCtl<RkCosine>* ctl) {
  typedef RkCosine P;
  constexpr uint32_t AW = SelCtl<P>::AW;
  __shared__ uint32_t w_acc[AW + 1][4];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  P::Acc a = P::acc0();
  uint32_t cnt = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < dir_size; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[i]);       // {meta, x, base, used}
    P::Key key = P::zero();
    if ((s.x & META_USED) && s.y != 0 && s.z != 0 && !rec_denied(f, s.y)) {
      bool dummy = false;
      const uint32_t T = apply_row<OP_GET>(&dir[i], s, arena, 0u, 0u, 0u, &dummy, nullptr);   // smatrix_get(now, x, 0)
      if (T != 0 && T >= t.min_total) {
        const uint32_t E = trend_expected(t, s.y);
        if (T > E && T - E >= t.min_gain) key = P::make(s.y, trend_score_bits(t.measure, t.shrink, T - E, E));
      }
    }
    sel_store<P>(keys, dir_size, i, key);
    if (!P::is_zero(key)) { P::acc_add(a, key); cnt++; }              // (a zero key would empty the AND of the keys)
  }
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

__global__ __launch_bounds__(POP_SORT_THREADS) void k_trend_sort(const SelCtl<RkCosine>* ctl, uint32_t n, const uint32_t* __restrict__ out,
                                                                 DirSlot* dir, uint32_t dmask, uint8_t* arena, TrendArgs t,
                                                                 uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                                 uint32_t* __restrict__ totals, uint32_t* __restrict__ expected,
                                                                 uint32_t* __restrict__ n_found) {
  typedef RkCosine P;
  __shared__ uint64_t s_s[POP_MAX];                                   // the score bits and the column words apart: 32 + 16 KiB,
  __shared__ uint32_t s_c[POP_MAX];                                   // neighbouring lanes on neighbouring banks in both
  const uint32_t cnt = ctl->n_out < n ? ctl->n_out : n;
  uint32_t Q = 64;
  while (Q < cnt) Q <<= 1;                                            // (n <= POP_MAX: Q <= POP_MAX)
  for (uint32_t i = threadIdx.x; i < Q; i += POP_SORT_THREADS) {
    const P::Key key = i < cnt ? sel_load<P>(out, n, i) : P::zero();
    s_s[i] = key.s; s_c[i] = key.c;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= Q; k <<= 1)
    for (uint32_t j = k >> 1; j; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < Q; i += POP_SORT_THREADS) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const P::Key a{s_s[i], s_c[i]}, b{s_s[l], s_c[l]};
          if ((i & k) == 0 ? !P::ge(a, b) : !P::ge(b, a)) {           // the last stage (k == Q) is descending throughout
            s_s[i] = b.s; s_c[i] = b.c; s_s[l] = a.s; s_c[l] = a.c;
          }
        }
      }
      __syncthreads();
    }
  for (uint32_t i = threadIdx.x; i < cnt; i += POP_SORT_THREADS) {
    const uint32_t x = 0xFFFFFFFFu - s_c[i];
    bool dummy = false;
    ids[i] = x;
    scores[i] = __longlong_as_double((long long)s_s[i]);
    totals[i] = apply_one<OP_GET>(dir, dmask, arena, x, 0u, 0u, &dummy);
    expected[i] = trend_expected(t, x);
  }
  if (threadIdx.x == 0) *n_found = cnt;
}
