// The rank keys of smatrix_merge_topk / smatrix_merge_topk_by (libsmatrix_amd/csrc/kernels/rank_key.hpp) as host code: the digit
// loop the selection kernels run (kernels/merge.hpp, mgt_select_row), here with a plain 256-bin histogram over a vector of keys,
// must end at the m-th largest key by std::sort, for every m from 1 to n - 1, and the emission's comparison with that threshold
// must keep exactly m keys.  Built with -fsanitize=undefined,address by tests/test_rank_key_select.py: a shift by 64 fails here.
#define __host__
#define __device__
#include "rank_key.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

// an order of its own, not the policy's ge()
static bool less(uint64_t a, uint64_t b) { return a < b; }
static bool less(RkCosine::Key a, RkCosine::Key b) { return a.s != b.s ? a.s < b.s : a.c < b.c; }
static bool same(uint64_t a, uint64_t b) { return a == b; }
static bool same(RkCosine::Key a, RkCosine::Key b) { return a.s == b.s && a.c == b.c; }

template <typename P>
static typename P::Key select(const std::vector<typename P::Key>& keys, uint32_t m) {
  typename P::Acc a = P::acc0();
  for (auto k : keys) P::acc_add(a, k);
  typename P::Key prefix;
  uint32_t dg = P::start(a, prefix), need = m;
  CHECK(dg < P::DIGITS, "start digit %u", dg);
  for (;;) {
    uint32_t hist[256] = {0};
    for (auto k : keys)
      if (P::agrees_above(k, prefix, dg)) {
        const uint32_t d = P::digit(k, dg);
        CHECK(d < 256, "digit %u", d);
        hist[d]++;
      }
    uint32_t d = 255, above = 0;
    while (above + hist[d] < need) { above += hist[d]; CHECK(d > 0, "the bins hold fewer than %u keys", need); d--; }
    const uint32_t bucket = hist[d];
    need -= above;
    P::take_digit(prefix, dg, d);
    if (dg == 0) return prefix;
    if (bucket == 1) {                                     // as the kernels: the OR of the keys that agree down to this digit
      uint32_t w[P::W] = {0};
      uint32_t found = 0;
      for (auto k : keys)
        if (P::agrees_down(k, prefix, dg)) { P::or_words(w, k); found++; }
      CHECK(found == 1, "a bin of one key holds %u", found);
      return P::from_words(w);
    }
    dg--;
  }
}

template <typename P>
static void run(const char* name, const std::vector<typename P::Key>& keys) {
  std::vector<typename P::Key> sorted(keys);
  std::sort(sorted.begin(), sorted.end(), [](auto a, auto b) { return less(b, a); });   // best first
  for (size_t i = 1; i < sorted.size(); i++) CHECK(less(sorted[i], sorted[i - 1]), "%s: key %zu twice", name, i);
  for (uint32_t m = 1; m < keys.size(); m++) {
    const typename P::Key t = select<P>(keys, m);
    CHECK(same(t, sorted[m - 1]), "%s: m %u of %zu", name, m, keys.size());
    CHECK(!P::is_zero(t), "%s: m %u: the threshold of a cut row is zero", name, m);
    uint32_t kept = 0;
    for (auto k : keys) kept += P::ge(k, t);
    CHECK(kept == m, "%s: m %u: the comparison keeps %u", name, m, kept);
  }
  std::printf("%s: %zu keys ok\n", name, keys.size());
}

int main() {
  std::mt19937_64 rng(20240607);
  const uint32_t ONES = 0xFFFFFFFFu;
  std::vector<uint64_t> v;
  std::vector<RkCosine::Key> c;
  auto both = [&](const char* name) { run<RkValue>(name, v); run<RkCosine>(name, c); v.clear(); c.clear(); };

  for (uint32_t j = 1; j <= 300; j++) {                    // any bits; columns 1 .. 300, so the keys are unique
    v.push_back(RkValue::make(j, (uint32_t)rng()));
    c.push_back(RkCosine::make(j, rng()));
  }
  both("random bits");
  for (uint32_t j = 1; j <= 300; j++) {                    // values 1 .. 5, a handful of scores: ties everywhere
    v.push_back(RkValue::make(j * 977, 1 + (uint32_t)(rng() % 5)));
    c.push_back(RkCosine::make(j * 977, 0x3FB0000000000000ull + ((rng() % 7) << 44)));
  }
  both("ties");
  for (uint32_t j = 1; j <= 200; j++) {                    // all keys equal except the last byte
    v.push_back(RkValue::make(j, 7));
    c.push_back(RkCosine::make(j, 0x3FD5555555555555ull));
  }
  both("the last byte of the column");
  for (uint32_t j = 1; j <= 200; j++) c.push_back(RkCosine::make(5, 0x3FD5555555555500ull + j));
  run<RkCosine>("the last byte of the score", c);
  c.clear();
  for (uint32_t j = 1; j <= 200; j++) {                    // keys that differ in the top byte only
    v.push_back(RkValue::make(5, j << 24));
    c.push_back(RkCosine::make(5, (uint64_t)j << 56));
  }
  both("the top byte");
  for (uint32_t j = 1; j <= 200; j++) {                    // all scores 0: the column decides
    v.push_back(RkValue::make(j * 977, 0));
    c.push_back(RkCosine::make(j * 977, 0));
  }
  both("all scores 0");
  for (uint32_t hi : {0u, ONES})                           // the extremes of both halves
    for (uint32_t lo : {0u, ONES}) {
      v.push_back(RkValue::make(lo, hi));
      for (uint32_t col : {0u, ONES}) c.push_back(RkCosine::make(col, ((uint64_t)hi << 32) | lo));
    }
  both("extremes");
  v = {RkValue::make(1, 5), RkValue::make(2, 5)};          // two keys: one bit apart, and every bit apart
  c = {RkCosine::make(1, 0x3FF0000000000000ull), RkCosine::make(2, 0x3FF0000000000000ull)};
  both("two keys");
  v = {RkValue::make(ONES, 0), RkValue::make(0, ONES)};
  c = {RkCosine::make(ONES, 0), RkCosine::make(0, ~0ull)};
  both("two keys, all bits");
  std::printf("RANK_KEY_OK\n");
  return 0;
}
