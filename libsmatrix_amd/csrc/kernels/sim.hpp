// kernels/sim.hpp -- the similarity measures of smatrix_cf_recommend_sim and smatrix_merge_topk_sim (include/smatrix_batch.h
// SMATRIX_SIM_*): one score, made in one place, for the recommend kernels (recommend.hpp) and the truncation's rank key (merge.hpp).
// A fragment of smx_kernels.hpp: included there before merge.hpp, INSIDE namespace smx.
//
// For a pair (b, cc) of row a, with A = total(a), B = total(b) (0 counted as 1) and c = cc as doubles (all three exact):
//     A == 0                     score = 0           (a row without a head pair scores 0 everywhere)
//     base = COSINE  sqrt(A) * sqrt(B)
//            JACCARD (A + B) - c
//            LIFT    A * B
//     den   = base + shrink
//     score = den != 0 && !(c > den) ? c / den : 0
// Split the way the recommend kernels cache it: sim_row (per row: sqrt(A) or A; 0 iff A == 0), sim_col (per candidate: sqrt(B) or
// B; always >= 1) and sim_score over the two.
// base is rounded to double ON ITS OWN before shrink is added.  hipcc contracts a * b + c into one fused multiply-add by default,
// across statements and through inlined helpers: __dadd_rn(__dmul_rn(a, b), c) is a plain `a * b + c` in this toolchain's headers and
// comes out as ONE v_fmac_f64.  What keeps the two roundings apart is the pragma in sim_den: the multiply and the add written under
// it carry no contract flag, wherever they are inlined.

constexpr int SIM_COSINE = 0, SIM_JACCARD = 1, SIM_LIFT = 2;

struct SimArgs {
  int sim;                                                 // SIM_*
  double shrink;                                           // finite, >= 0 (-0.0 acts as 0.0: base is never -0.0)
};

__device__ __forceinline__ double sim_row(int sim, uint32_t ta) {
  const double A = (double)ta;
  return sim == SIM_COSINE ? sqrt(A) : A;
}
__device__ __forceinline__ double sim_col(int sim, uint32_t tb) {
  const double B = (double)(tb == 0 ? 1u : tb);
  return sim == SIM_COSINE ? sqrt(B) : B;
}
__device__ __forceinline__ double sim_den(int sim, double shrink, double c, double ra, double cb) {
#pragma clang fp contract(off)
  const double base = sim == SIM_JACCARD ? (ra + cb) - c : ra * cb;
  return base + shrink;
}
__device__ __forceinline__ double sim_score(const SimArgs& m, uint32_t cc, double ra, double cb) {
  if (ra == 0.0) return 0.0;
  const double c = (double)cc;
  const double den = sim_den(m.sim, m.shrink, c, ra, cb);  // (a negative Jaccard denominator fails c > den: scores lie in [0, 1])
  return (den != 0.0 && !(c > den)) ? c / den : 0.0;
}
