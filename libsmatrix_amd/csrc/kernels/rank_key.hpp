// kernels/rank_key.hpp -- the rank keys of smatrix_merge_topk / smatrix_merge_topk_by, as bit arithmetic and nothing else: what a
// key is, its digits for the MSB radix select of kernels/merge.hpp, where that select starts, and the comparison the emission
// makes with the finished threshold.  A fragment of smx_kernels.hpp (included there before merge.hpp, inside namespace smx) that
// needs <stdint.h> alone: host C++ includes it with __host__ and __device__ defined away (tests/c/rank_key_select.cpp).
//
// A key orders the eligible pairs of ONE row, larger is better, and is unique within the row.  Both policies have one interface:
//   Key, zero(), is_zero(k), ge(k, thr)           the key; the threshold "every eligible pair"; what the emission keeps
//   DIGITS, digit(k, dg)                          its bytes, most significant = DIGITS - 1
//   agrees_above / agrees_down(k, prefix, dg)     k has the prefix's digits above dg / down to dg
//   take_digit(prefix, dg, d)                     the prefix with digit dg chosen
//   W, or_words(w, k), from_words(w)              the key as W 32-bit words, for OR reductions (keys are unique: the OR of the
//                                                 keys that agree with a prefix no other key has is that key)
//   Acc, acc0(), acc_add(a, k), start(a, prefix)  what the select needs of ALL keys before its first pass, every word of it
//                                                 combined by OR; start() -> the first digit, and the digits above it in prefix
// A shift is by 56 + 8 at most, in two steps: never a shift by 64.
#include <stdint.h>

#define RK_FN __host__ __device__ inline __attribute__((always_inline))

// rank VALUE: 64 bits {v, 0xFFFFFFFF - y} -- by value, equal values by ascending column.
// The select starts at the highest byte that is not 0 in every key (small values: 3 passes less), from the OR of the keys alone.
struct RkValue {
  typedef uint64_t Key;
  struct Acc { uint32_t w[2]; };                           // the OR of the keys
  static constexpr uint32_t DIGITS = 8, W = 2;
  static RK_FN Key make(uint32_t y, uint32_t v) { return ((uint64_t)v << 32) | (0xFFFFFFFFu - y); }
  static RK_FN Key zero() { return 0; }
  static RK_FN bool is_zero(Key k) { return k == 0; }
  static RK_FN bool ge(Key k, Key thr) { return k >= thr; }
  static RK_FN uint32_t digit(Key k, uint32_t dg) { return (uint32_t)(k >> (8 * dg)) & 255u; }
  static RK_FN bool agrees_above(Key k, Key p, uint32_t dg) { return (((k ^ p) >> (8 * dg)) >> 8) == 0; }
  static RK_FN bool agrees_down(Key k, Key p, uint32_t dg) { return ((k ^ p) >> (8 * dg)) == 0; }
  static RK_FN void take_digit(Key& p, uint32_t dg, uint32_t d) { p |= (uint64_t)d << (8 * dg); }
  static RK_FN void or_words(uint32_t* w, Key k) { w[0] |= (uint32_t)(k >> 32); w[1] |= (uint32_t)k; }
  static RK_FN Key from_words(const uint32_t* w) { return ((uint64_t)w[0] << 32) | w[1]; }
  static RK_FN Acc acc0() { return Acc{{0, 0}}; }
  static RK_FN void acc_add(Acc& a, Key k) { or_words(a.w, k); }
  static RK_FN uint32_t start(const Acc& a, Key& prefix) {   // (two keys and more: their OR is not 0)
    prefix = 0;
    return (63u - (uint32_t)__builtin_clzll(from_words(a.w))) >> 3;
  }
};

// rank COSINE: 96 bits {the bit pattern of the score, an IEEE double >= 0, 0xFFFFFFFF - y} -- by score (patterns of doubles >= 0
// order as the doubles do), equal scores by ascending column.  Digits 11 .. 4 are the score's bytes 7 .. 0, 3 .. 0 the column's.
// Positive doubles share their top bytes, so the select starts at the highest digit in which the row's keys DIFFER (two keys and
// more: there is one), with the digits above it -- common to all keys -- as the prefix: from the OR and the AND of the keys.
struct RkCosine {
  struct Key { uint64_t s; uint32_t c; };
  struct Acc { uint32_t w[6]; };                           // the OR of the keys, the OR of their complements (the AND, inverted)
  static constexpr uint32_t DIGITS = 12, W = 3;
  static RK_FN Key make(uint32_t y, uint64_t score_bits) { return Key{score_bits, 0xFFFFFFFFu - y}; }
  static RK_FN Key zero() { return Key{0, 0}; }
  static RK_FN bool is_zero(Key k) { return (k.s | k.c) == 0; }
  static RK_FN bool ge(Key k, Key thr) { return k.s > thr.s || (k.s == thr.s && k.c >= thr.c); }
  static RK_FN uint32_t digit(Key k, uint32_t dg) {
    return dg >= 4 ? (uint32_t)(k.s >> (8 * (dg - 4))) & 255u : (k.c >> (8 * dg)) & 255u;
  }
  static RK_FN bool agrees_above(Key k, Key p, uint32_t dg) {
    return dg >= 4 ? (((k.s ^ p.s) >> (8 * (dg - 4))) >> 8) == 0 : k.s == p.s && (((k.c ^ p.c) >> (8 * dg)) >> 8) == 0;
  }
  static RK_FN bool agrees_down(Key k, Key p, uint32_t dg) {
    return dg >= 4 ? ((k.s ^ p.s) >> (8 * (dg - 4))) == 0 : k.s == p.s && ((k.c ^ p.c) >> (8 * dg)) == 0;
  }
  static RK_FN void take_digit(Key& p, uint32_t dg, uint32_t d) {
    if (dg >= 4) p.s |= (uint64_t)d << (8 * (dg - 4));
    else p.c |= d << (8 * dg);
  }
  static RK_FN void or_words(uint32_t* w, Key k) { w[0] |= (uint32_t)(k.s >> 32); w[1] |= (uint32_t)k.s; w[2] |= k.c; }
  static RK_FN Key from_words(const uint32_t* w) { return Key{((uint64_t)w[0] << 32) | w[1], w[2]}; }
  static RK_FN Acc acc0() { return Acc{{0, 0, 0, 0, 0, 0}}; }
  static RK_FN void acc_add(Acc& a, Key k) { or_words(a.w, k); or_words(a.w + 3, Key{~k.s, ~k.c}); }
  static RK_FN uint32_t start(const Acc& a, Key& prefix) {
    const Key o = from_words(a.w), n = from_words(a.w + 3);
    const uint64_t and_s = ~n.s, ds = o.s ^ and_s;
    const uint32_t and_c = ~n.c, dc = o.c ^ and_c;
    if (ds) {
      const uint32_t sh = (63u - (uint32_t)__builtin_clzll(ds)) & ~7u;
      prefix = Key{((and_s >> sh) >> 8) << 8 << sh, 0};
      return 4 + (sh >> 3);
    }
    const uint32_t sh = dc ? (31u - (uint32_t)__builtin_clz(dc)) & ~7u : 0u;
    prefix = Key{and_s, ((and_c >> sh) >> 8) << 8 << sh};
    return sh >> 3;
  }
};
#undef RK_FN
