// kernels/explain.hpp -- why an item was recommended (include/smatrix_batch.h smatrix_cf_explain): for every (target t, session
// position i) the term w_i * score(a_i, t) that smatrix_cf_recommend_sim adds to t's sum for the item a_i at that position, and
// the pair's count cc = get(a_i, t).  Host side: smx_explain.inc.
// A fragment of smx_kernels.hpp: included there after recommend.hpp (rec_weight_ok), INSIDE namespace smx.
//
// No session table is built: a term is a function of three cells -- get(a, t), get(a, 0), get(t, 0) -- and of whether position i
// is the FIRST one that holds a.  The two totals and the first positions are made once per session entry and once per target:
//   k_exp_prep_items    a wave per session: ra[off[s] + i] = -1.0 for a later occurrence of an id, else sim_row(sim, get(a, 0)),
//                       which is >= 0.  Every position is compared with all earlier ones, 64 at a time through the wave
//                       (k_rec_bound's compare, here without its REC_DEDUP_MAX cut): L * (L + 1) / 2 compares for a session of L
//                       ids, exact at every L.  Every weight is checked (*bad).
//   k_exp_prep_targets  a lane per target: cb[j] = sim_col(sim, get(t, 0)), always >= 1
//   k_exp_terms         a lane per output entry e < total: the session by binary search in e_off, then ONE look-up get(a, t) --
//                       64 independent look-ups in flight per wave --, the term by sim_score over the two cached doubles (the
//                       denominator is sim_den's, two roundings, as everywhere) and the weight product by __dmul_rn.  The entry
//                       is stored, nothing is accumulated: the sum is the caller's left fold.
// Every lane of k_exp_terms writes entry e of terms and cc and no other, e < total: whatever e_off holds, nothing outside
// [0, total) is written.  What it READS is bounded by off and t_off alone: i < L_s and j < T_s are checked before items, targets,
// ra and cb are indexed.

__global__ __launch_bounds__(256) void k_exp_prep_items(DirSlot* dir, uint32_t dmask, uint8_t* arena, uint32_t n,
                                                        const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                        const double* __restrict__ w, int sim, double* __restrict__ ra,
                                                        uint32_t* bad) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t s = wave; s < n; s += nwaves) {
    const uint64_t b0 = off[s], L = off[s + 1] - b0;
    for (uint64_t c0 = 0; c0 < L; c0 += 64) {                       // (wave-uniform loops: the shuffles need every lane)
      const uint64_t i = c0 + lane;
      const uint32_t a = i < L ? items[b0 + i] : 0u;
      if (w && i < L && !rec_weight_ok(w[b0 + i])) *bad = 1u;
      bool dup = false;
      for (uint64_t e0 = 0; e0 <= c0; e0 += 64) {                   // the positions before mine, 64 at a time
        const uint32_t e = e0 + lane < L ? items[b0 + e0 + lane] : 0u;
        const uint32_t lim = e0 == c0 ? lane : 64u;
        for (uint32_t j = 0; j < 64; j++) {
          const uint32_t o = (uint32_t)__shfl((int)e, (int)j);
          dup |= j < lim && o == a;
        }
      }
      if (i >= L) continue;
      bool dummy = false;
      ra[b0 + i] = dup ? -1.0 : sim_row(sim, apply_one<OP_GET>(dir, dmask, arena, a, 0u, 0u, &dummy));
    }
  }
}

__global__ __launch_bounds__(256) void k_exp_prep_targets(DirSlot* dir, uint32_t dmask, uint8_t* arena, uint64_t n_targets,
                                                          const uint32_t* __restrict__ targets, int sim, double* __restrict__ cb) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_targets; j += (uint64_t)gridDim.x * blockDim.x) {
    bool dummy = false;
    cb[j] = sim_col(sim, apply_one<OP_GET>(dir, dmask, arena, targets[j], 0u, 0u, &dummy));
  }
}

struct ExpArgs {
  const uint64_t* off;                        // n + 1: session s is items[off[s] .. off[s+1])
  const uint32_t* items;
  const double* w;                            // per entry of items, or NULL: every weight 1.0
  const uint64_t* t_off;                      // n + 1: its targets are targets[t_off[s] .. t_off[s+1])
  const uint32_t* targets;
  const uint64_t* e_off;                      // n + 1: its entries start at e_off[s]
  const double* ra;                           // k_exp_prep_items', parallel to items
  const double* cb;                           // k_exp_prep_targets', parallel to targets
  uint32_t n;
  SimArgs m;
};

__global__ __launch_bounds__(256) void k_exp_terms(DirSlot* dir, uint32_t dmask, uint8_t* arena, ExpArgs x, uint64_t total,
                                                   double* __restrict__ terms, uint32_t* __restrict__ cc) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    // the LAST s < n with e_off[s] <= e: sessions without targets or without items make runs of equal offsets
    uint32_t lo = 0, hi = x.n;
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (x.e_off[mid] <= e) lo = mid; else hi = mid;
    }
    const uint32_t s = lo;
    double term = 0.0;
    uint32_t c = 0;
    const uint64_t E = x.e_off[s], b0 = x.off[s], L = x.off[s + 1] - b0, t0 = x.t_off[s], T = x.t_off[s + 1] - t0;
    if (E <= e && L != 0) {
      const uint64_t r = e - E, j = r / L, i = r - j * L;
      if (j < T) {
        const uint32_t t = x.targets[t0 + j];
        const double ra = x.ra[b0 + i];
        if (t != 0 && ra >= 0.0) {                                  // (ra < 0: a later occurrence of the id)
          bool dummy = false;
          c = apply_one<OP_GET>(dir, dmask, arena, x.items[b0 + i], t, 0u, &dummy);
          if (c != 0) {                                             // (an absent cell and a dead one: +0.0, 0)
            double wa = x.w ? x.w[b0 + i] : 1.0;
            if (wa == 0.0) wa = 0.0;                                // -0.0 acts as 0.0: no entry is ever -0.0
            term = __dmul_rn(wa, sim_score(x.m, c, ra, x.cb[t0 + j]));   // (rounded on its own; wa == 1.0 changes no bit)
          }
        }
      }
    }
    terms[e] = term;
    cc[e] = c;
  }
}
