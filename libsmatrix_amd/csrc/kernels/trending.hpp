// kernels/trending.hpp -- the trending items (include/smatrix_batch.h smatrix_cf_trending): the n ids whose column-0 totals in one
// matrix (`now`) grew most against a scaled baseline from a second one (`base`), chosen on the device with no read-back.  Host side:
// smx_trending.inc.
// A fragment of smx_kernels.hpp: included there after select.hpp (the dense select and its limits) and recommend.hpp (RecFilt,
// rec_denied), INSIDE namespace smx.
//
// A candidate x has T = get(now, x, 0), B = get(base, x, 0), E = floor(B * num / den) and the gain G = T - E > 0; its score is G,
// G / D or G / sqrt(D) with D = E + shrink (0 counted as 1), an IEEE double > 0, and its key RkCosine::make(x, the score's bits) of
// kernels/rank_key.hpp: score descending, equal scores by ascending id, unique.  The selection is select.hpp's over 96-bit keys in
// three planes of words (the select starts at the highest digit in which the keys differ: positive doubles share their top bytes):
//   k_trend_keys      a lane per slot of now's directory: the head-cell total, ONE look-up of x in base's directory, the score, the
//                     key; P::zero() for anything that is no candidate.  The keys' P::Acc (the OR of the keys and of their
//                     complements) and their number through sel_publish
//   k_sel_start<RkCosine>, RkCosine::DIGITS times (k_sel_hist<RkCosine>, k_sel_pick<RkCosine>), k_sel_collect<RkCosine>
//   k_trend_sort      one workgroup: the buffer (<= 4096 keys, 48 KiB of LDS) sorted by sel_bitonic, best first; ids and scores
//                     decoded, T and E looked up again per result entry (no payload rides through the sort)

constexpr int TREND_GAIN = 0, TREND_RATIO = 1, TREND_ZSCORE = 2;   // SMATRIX_TREND_*

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
  sel_publish<P>(ctl, a, cnt);
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
  sel_bitonic<P>(Q, [&](uint32_t i) { return P::Key{s_s[i], s_c[i]}; }, [&](uint32_t i, P::Key key) { s_s[i] = key.s; s_c[i] = key.c; });
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
