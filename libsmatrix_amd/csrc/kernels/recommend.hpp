// kernels/recommend.hpp -- session recommendations (include/smatrix_batch.h smatrix_cf_recommend_batch): per session, the k best
// items over the union of its items' rows, a candidate b scored by the sum, in session order, of cf_cosine(a, b) over the session's
// distinct items a whose row holds b.  Host side: smx_recommend.inc.
// A fragment of smx_kernels.hpp: included there, after rows.hpp (CfCand, cf_sort64, cf_merge_stages), INSIDE namespace smx.
//
// Every session is summed in a hash of its own.  A slot holds {key, sqrt(get(b,0)) or -1 for an item of the session, running sum}:
// the session's items go in first (excluded keys; an item's FIRST position is kept in the low word of its sum as 2^32-1 - pos, by
// atomicMax), then the items' rows are scanned one item at a time in session order, with a barrier (LDS tier) or a kernel boundary
// (global tier) between items.  A key appears once in a row, so a slot receives at most one term per item: the sum is a
// left-to-right sum in session order, whatever the order of lanes.  The terms are added with atomics only so that a row holding
// a key twice (the reference's reload can leave one) still adds both terms.
//   k_rec_bound     a wave per session: bound = sum of its distinct items' row sizes (slots: every quirk row is covered); tiers
//   k_rec_lds       a workgroup per session of bound + length <= REC_LDS_SLOTS: the hash in LDS, the top-k at the end
//   k_rec_gl_*      the other sessions: hashes in a pooled device buffer, a launch per item position, a wave per 512-cell chunk
//                   of a row; then a wave per 4096-slot segment (its top-64) and a workgroup per session (the merge)
// smatrix_cf_recommend_filtered (RecFilt, the kernels' <true> instances; <false> is smatrix_cf_recommend_batch's code):
//   exclusion list  more excluded keys, entered with the session's items (sqrt = -1; the low word of the sum is left alone: it is
//                   an ITEM's first position, and an id may be both); the table has room for them (k_rec_bound)
//   deny bitmap     tested where a key is claimed: a denied key gets sqrt = -1 like an item
//   weights         the term of the item at position i is multiplied by w[i] (__dmul_rn: rounded on its own) before it is added
// smatrix_cf_recommend_sim (RecFilt::m; k_rec_lds_sim<F>, k_rec_gl_scan_sim<F>: the two kernels that make a score, over the same
// bodies): the term is kernels/sim.hpp's, the per-row double sqrt(A) or A, the slot's double sqrt(B) or B.  The tiers, the
// tables and the top-k know nothing of the measure: k_rec_bound, k_rec_gl_init and the rest are the filtered call's.
// smatrix_cf_rank (RecRank; k_rec_lds_rank<F>, k_rec_lds_rank_sim<F>, k_rec_gl_rank): the same tables with another ending.  Instead
// of the k best slots, the session's targets are looked up in the finished table (they are never entered: tiers and table sizes
// are the recommend call's) and the candidates that beat each are counted, rec_rank_table: one pass over the table per 64 targets.
// smatrix_cf_recommend_grouped (RecGroup; k_rec_lds_grouped<F>, k_rec_lds_grouped_sim<F>, k_rec_gl_grouped): the same tables with a
// third ending, rec_group_table: at most cap results of one group, decided in rounds over the 64 best slots still alive.
// smatrix_cf_recommend_deep with k > 64 (k_rec_lds_deep<F>, k_rec_lds_deep_sim<F>, k_rec_gl_deep): the same tables with a fourth ending,
// rec_deep_table: up to REC_DEEP_MAX results, by a radix select of the k-th best key and a workgroup sort of what is at or above it.
// smatrix_cf_recommend_fill (k_rec_fill, at the end of this file): the sim call's launches as they are, and one more behind them that
// fills the free places of a short result from the caller's list under the session's own filters.
// smatrix_cf_recommend_grouped_fill (k_rec_fill_grouped, behind k_rec_fill): the grouped call's launches as they are, and the fill
// under the same quotas: the groups of the results live in lanes beside the ids, and a step's quota is decided by counts.  It is
// rec_fill_walk<false>, ONE body for the fill under quotas with and without a scope.
// smatrix_cf_recommend_scoped (RecScope; k_rec_lds_scoped, k_rec_lds_grouped_scoped and k_rec_gl_scan_scoped, over the same bodies
// with C set; k_rec_scope_bound and k_rec_fill_scoped = rec_fill_walk<true> at the end of this file): the grouped fill call
// with a per-session deny decided by the id's group in a second map.  The test stands where rec_denied stands, on a claimed key of
// either tier -- once per distinct key of a session --, and an out-of-scope key gets sqrt = -1 like a denied one, so the endings and
// the tables know nothing of it; the walk tests the list's ids the same way.  The tiers' other instances have C == false.

constexpr uint32_t REC_LDS_SLOTS = 4096;      // 4 + 8 + 8 bytes a slot: 80 KiB, two workgroups per CU (160 KiB)
constexpr uint32_t REC_LDS_THREADS = 512;
constexpr uint32_t REC_SEG = 4096;            // global tier: slots per top-k segment; global tables are multiples of it
constexpr uint32_t REC_GL_MIN_LG = 13;        // ... and at least 8192 slots (the bound of such a session is above 4096)
constexpr uint32_t REC_CHUNK = 512;           // global tier: cells of a row per wave task
constexpr uint32_t REC_MERGE_THREADS = 1024;

struct RecCtl {
  uint32_t n_lds, n_big, max_len, bad;        // bad: a weight that is negative, NaN or infinite (k_rec_bound<true>)
  unsigned long long total_slots, max_slots;  // global tier: table slots of all its sessions, of the largest one
};

// what smatrix_cf_recommend_filtered adds; every pointer may be NULL (not given), deny == NULL goes with deny_n == 0
struct RecFilt {
  const double* w;                            // per entry of items
  const uint64_t* ex_off;                     // session s must not be given ex[ex_off[s] .. ex_off[s+1])
  const uint32_t* ex;
  const uint32_t* deny;                       // bit b & 31 of word b >> 5: id b < deny_n is never given
  uint64_t deny_n;
  SimArgs m;                                  // smatrix_cf_recommend_sim: the measure and its shrinkage (read by the <.., true> bodies alone)
};
__device__ __forceinline__ bool rec_denied(const RecFilt& f, uint32_t b) {
  return b < f.deny_n && ((f.deny[b >> 5] >> (b & 31)) & 1u) != 0;
}
__device__ __forceinline__ bool rec_weight_ok(double w) { return w >= 0.0 && w <= 1.7976931348623157e308; }   // (-0.0 passes, NaN fails)

// (score desc, id asc): the result order of smatrix_cf_recommend_batch
struct CfById {
  __device__ __forceinline__ bool operator()(const CfCand& a, const CfCand& b) const {
    return a.key > b.key || (a.key == b.key && a.id < b.id);
  }
};

// one term.  <false>: exactly as k_cf_neighbors computes it (sa = sqrt of get(a,0); sqb = sqrt of get(b,0), 0 counted as 1).
// <true>: the measure m (kernels/sim.hpp) over the same two cached doubles, sa = sim_row of get(a,0), sqb = sim_col of get(b,0)
template <bool S>
__device__ __forceinline__ double rec_term(uint32_t cc, double sa, double sqb, const SimArgs& m) {
  if (S) return sim_score(m, cc, sa, sqb);
  const double num = (double)cc;
  const double den = sa * sqb;
  return (den != 0.0 && !(num > den)) ? num / den : 0.0;
}
// the row's double of item a, and the candidate's of key b: what a slot caches (always >= 1, so 0.0 = not yet filled and
// -1 = an excluded key keep their meaning under every measure)
template <bool S>
__device__ __forceinline__ double rec_row_total(DirSlot* dir, uint32_t dmask, uint8_t* arena, uint32_t a, const SimArgs& m) {
  bool dummy = false;
  const uint32_t t = apply_one<OP_GET>(dir, dmask, arena, a, 0u, 0u, &dummy);
  return S ? sim_row(m.sim, t) : sqrt((double)t);
}
template <bool S>
__device__ __forceinline__ double rec_col_total(DirSlot* dir, uint32_t dmask, uint8_t* arena, uint32_t b, const SimArgs& m) {
  bool dummy = false;
  uint32_t t = apply_one<OP_GET>(dir, dmask, arena, b, 0u, 0u, &dummy);
  if (S) return sim_col(m.sim, t);
  if (t == 0) t = 1;
  return sqrt((double)t);
}
__device__ __forceinline__ uint32_t rec_lg(uint64_t need, uint32_t min_lg) {
  uint32_t lg = min_lg;
  while ((1ull << lg) < need) lg++;
  return lg;
}
__device__ __forceinline__ uint32_t rec_first_word(uint64_t pos) { return 0xffffffffu - (uint32_t)pos; }

// find or claim key b (!= 0) in a hash of mask + 1 slots (never full: it has room for every key it can be given)
template <bool LDS>
__device__ __forceinline__ uint32_t rec_slot(uint32_t* keys, uint32_t mask, uint32_t b, bool* claimed) {
  uint32_t h = fmix32(b) & mask;
  for (;;) {
    const uint32_t c = LDS ? __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                           : __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c == b) { *claimed = false; return h; }
    if (c == 0) {
      const uint32_t old = atomicCAS(&keys[h], 0u, b);
      if (old == 0) { *claimed = true; return h; }
      if (old == b) { *claimed = false; return h; }
    }
    h = (h + 1) & mask;
  }
}
// the slot of a key that is there (an item of the session)
__device__ __forceinline__ uint32_t rec_find(const uint32_t* keys, uint32_t mask, uint32_t b) {
  uint32_t h = fmix32(b) & mask;
  while (keys[h] != b) h = (h + 1) & mask;
  return h;
}
__device__ __forceinline__ uint32_t rec_low_word(const double* p) { return *reinterpret_cast<const uint32_t*>(p); }

// what smatrix_cf_rank asks and answers: session s asks about targets[t_off[s] .. t_off[s+1]); ranks / scores run parallel to
// targets and were filled with SMATRIX_RANK_NONE / 0.0 before the kernels run, so only a target that is found is written
struct RecRank {
  const uint64_t* t_off;
  const uint32_t* targets;
  uint32_t* ranks;
  double* scores;
};

__device__ __forceinline__ long long rec_readlane(long long v, uint32_t j) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), (int)j);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// The rank ending of both tiers, run by a workgroup of NW waves over the finished table {keys, sq, sum} of tsize slots (a power of
// two >= 64) of session s.  A candidate is a slot with key != 0 && sq > 0, the test of the top-k endings; a target is found by
// probing from its hash until its key or an empty slot (the table is never full), and a found slot that is no candidate is no
// answer.  Per batch of up to 64 targets: lane j of EVERY wave holds target j's (sum bits, id) and a counter; a wave walks its share
// of the slots 64 at a time and, for each target of the batch, adds the popcount of the ballot "candidate and better than target
// j" (CfById's order: the sums are >= +0.0, their bit patterns order as the doubles do) to lane j's counter; the waves' counters
// are added up through part (NW * 64 + NW words of LDS).  counts[s] = the candidates, counted by the first batch's pass (a session
// without targets makes that pass alone).
// FOLDED (the LDS tier, whose 80 KiB leave no LDS for part): the caller has folded the candidate test into the sums -- the sum of
// a key that is no candidate is -1.0, a sign bit no candidate's sum has -- and sq is not read: part may lie in it.
template <bool FOLDED, uint32_t NW, typename I>
__device__ __forceinline__ void rec_rank_table(const uint32_t* keys, const double* sq, const double* sum, I tsize, const RecRank& rk,
                                               uint32_t s, uint32_t* __restrict__ counts, uint32_t* part) {
  constexpr long long NONE = (long long)0x8000000000000000ull;
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t mask = (uint32_t)(tsize - 1);                      // (a table of 2^32 slots: mask 2^32 - 1)
  const uint64_t t0 = rk.t_off[s], T = rk.t_off[s + 1] - t0;
  for (uint64_t j0 = 0; j0 == 0 || j0 < T; j0 += 64) {
    const uint32_t nt = (uint32_t)(T - j0 < 64 ? T - j0 : 64);
    const uint32_t b = lane < nt ? rk.targets[t0 + j0 + lane] : 0u;
    long long tk = NONE;                                            // NONE: no answer (id 0, not in the table, not a candidate)
    if (b != 0) {
      uint32_t h = fmix32(b) & mask, c;
      while ((c = keys[h]) != b && c != 0) h = (h + 1) & mask;
      if (c == b && (FOLDED || sq[h] > 0.0)) tk = __double_as_longlong(sum[h]);
      if (tk < 0) tk = NONE;
    }
    uint32_t cnt = 0, nc = 0;
    for (I p0 = w * 64; p0 < tsize; p0 += NW * 64) {
      const I p = p0 + lane;
      const uint32_t key = keys[p];
      long long sk = NONE;
      if (key != 0 && (FOLDED || sq[p] > 0.0)) sk = __double_as_longlong(sum[p]);
      const uint64_t cm = __ballot(sk >= 0);                        // the candidates of this step
      if (cm == 0) continue;
      nc += (uint32_t)__popcll(cm);
      for (uint32_t j = 0; j < nt; j++) {                           // (wave-uniform: target j's pair comes as scalars)
        const long long tj = rec_readlane(tk, j);
        const uint32_t bj = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)j);
        const uint64_t m = __ballot(sk > tj || (sk == tj && key < bj)) & cm;
        if (lane == j) cnt += (uint32_t)__popcll(m);
      }
    }
    part[w * 64 + lane] = cnt;
    if (lane == 0) part[NW * 64 + w] = nc;
    __syncthreads();
    if (w == 0) {
      uint32_t r = 0;
      for (uint32_t v = 0; v < NW; v++) r += part[v * 64 + lane];
      if (lane < nt && tk != NONE) {
        rk.ranks[t0 + j0 + lane] = r;
        rk.scores[t0 + j0 + lane] = __longlong_as_double(tk);
      }
      if (j0 == 0 && lane == 0) {
        uint32_t c = 0;
        for (uint32_t v = 0; v < NW; v++) c += part[NW * 64 + v];
        counts[s] = c;
      }
    }
    __syncthreads();                                                // before part is written again (or the table cleared)
  }
}

// what smatrix_cf_recommend_grouped adds: candidate b belongs to group of[b]; an id >= n, or one whose entry is REC_GROUP_NONE, is
// ungrouped.  At most cap results of a session share a group
constexpr uint32_t REC_GROUP_NONE = 0xffffffffu;
struct RecGroup {
  const uint32_t* of;
  uint64_t n;
  uint32_t cap;
};
// what smatrix_cf_recommend_scoped adds: a per-session deny decided by the id's group in a map of its own, of[b] for b < n, else
// REC_GROUP_NONE.  Session s lists gr[off[s] .. off[s+1]), at most REC_SCOPE_MAX groups; with an empty list it is unscoped.  An id is
// LISTED when its group is not REC_GROUP_NONE and occurs in the list; a scoped session is given the listed ids alone (except == 0)
// or every id but the listed ones (except != 0).
constexpr uint32_t REC_SCOPE_MAX = 64;        // SMATRIX_SCOPE_MAX: the fill kernels hold a list one entry per lane
struct RecScope {
  const uint32_t* of;
  uint64_t n;
  const uint64_t* off;
  const uint32_t* gr;
  uint32_t except;
};
// session s's list as {first entry, length}.  A longer list than REC_SCOPE_MAX is a refusal (k_rec_scope_bound sets RecCtl::bad
// and nothing runs behind it); the cut only keeps every reader inside 64 entries
__device__ __forceinline__ uint32_t rec_scope_len(const RecScope& sc, uint32_t s, uint64_t* l0) {
  *l0 = sc.off[s];
  const uint64_t nl = sc.off[s + 1] - *l0;
  return (uint32_t)(nl < REC_SCOPE_MAX ? nl : REC_SCOPE_MAX);
}
// is key b kept from a session whose list is gr[l0 .. l0 + nl)?  One gather from the map, then nl compares against words at
// addresses the whole wave shares (the list lies in global memory: the LDS tier has no word to spare)
__device__ __forceinline__ bool rec_out_of_scope(const RecScope& sc, uint64_t l0, uint32_t nl, uint32_t b) {
  if (nl == 0) return false;
  const uint32_t g = b < sc.n ? sc.of[b] : REC_GROUP_NONE;
  bool listed = false;
  if (g != REC_GROUP_NONE)
    for (uint32_t j = 0; j < nl; j++) listed |= sc.gr[l0 + j] == g;
  return listed == (sc.except != 0);
}

// the LDS words the grouped ending needs beside the table: NW lists of 64 {key, id, group}, the <= 64 groups a round fills, and
// {the round's verdict, the key and the id of the last candidate it looked at}
constexpr uint32_t REC_GRP_DONE = 0xffffffffu;
constexpr uint32_t rec_group_words(uint32_t NW) { return NW * 64 * 4 + 64 + 4; }

// cf_sort64 / cf_merge_stages in CfById's order with their stage loops kept ROLLED.  Unrolled, every stage's lane masks are loop
// invariants that are kept in scalar registers across the rounds -- more of them than there are, beside the grouped ending's own state
// --; rolled, a stage's mask lives for that stage, and the distance of the shuffle is a register, not a constant.
__device__ __forceinline__ void rec_merge_rolled(CfCand& v, uint32_t lane) {
  const CfById better;
#pragma nounroll
  for (uint32_t j = 32; j; j >>= 1) {
    const CfCand o = cf_shfl_xor(v, (int)j);
    if (better(o, v) == ((lane & j) == 0)) v = o;                   // the lower lane of a pair keeps the better one
  }
}
__device__ __forceinline__ void rec_sort64_rolled(CfCand& v, uint32_t lane) {
  const CfById better;
#pragma nounroll
  for (uint32_t k2 = 2; k2 <= 64; k2 <<= 1) {
#pragma nounroll
    for (uint32_t j = k2 >> 1; j; j >>= 1) {
      const CfCand o = cf_shfl_xor(v, (int)j);
      const bool down = (lane & k2) == 0 || k2 == 64;               // blocks alternate direction; the last pass is best-first
      if (better(o, v) == (((lane & j) == 0) == down)) v = o;
    }
  }
}

// The grouped ending of both tiers, run by a workgroup of NW waves over the finished table {keys, sq, sum} of tsize slots (a power of
// two >= 64) of session s: the first k candidates, in CfById's order, that fewer than cap candidates of their own group precede.
// The candidate test is folded into the sums first (a slot that is no candidate, an empty one included, gets the sum -1.0: "dead"),
// then sq is free and its first 4 * tsize bytes hold the group of every slot alive -- one gather from gr.of per candidate.
// A ROUND: the 64 best slots alive (every wave over its share, k_cf_topk's loop; wave 0 merges the waves' lists through ws) stand in
// wave 0's lanes in order, the group in CfCand::slot.  Lane i is a survivor iff it is ungrouped or (the results taken so far + the
// lanes below i) hold fewer than cap of its group: every candidate of a group that came before lane i and is not in one of those two
// places was a survivor itself while the group was below cap, and dead since.  The survivors are numbered by mbcnt behind the results
// taken, cut at k, stored, and their groups handed to the lanes that own the new places (the results live in lanes, as in
// k_rec_fill).  Then everything that can no longer be taken dies in one pass: the slots not worse than the round's last (the 64
// looked at), and the slots of a group that reached cap in this round.  The call ends at k results or after a round that found
// fewer than 64 alive.  A round's first candidate is always a survivor (its group would be dead otherwise): at most k rounds.
// A thread meets the same slots in every pass (p = threadIdx.x + i * NW * 64), so the table needs no barrier of its own; the two
// barriers of a round order ws.  Nothing depends on slot order: the order is CfById's, and ids are distinct.
template <uint32_t NW, typename I>
__device__ __forceinline__ void rec_group_table(const uint32_t* keys, double* sq, double* sum, I tsize, const RecGroup& gr, uint32_t k,
                                                uint32_t s, uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                uint32_t* __restrict__ counts, uint32_t* ws) {
  constexpr long long NONE = (long long)0x8000000000000000ull;
  constexpr uint32_t NT = NW * 64;
  const CfById better;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t* grp = reinterpret_cast<uint32_t*>(sq);
  long long* l_key = reinterpret_cast<long long*>(ws);              // (ws is 8-byte aligned)
  uint32_t* l_id = ws + NT * 2;
  uint32_t* l_grp = l_id + NT;
  uint32_t* full = l_grp + NT;
  uint32_t* ctl = full + 64;
  for (I p = tid; p < tsize; p += NT)
    if (!(keys[p] != 0 && sq[p] > 0.0)) sum[p] = -1.0;
  __syncthreads();                                                  // sq is read: the groups go over it
  for (I p = tid; p < tsize; p += NT)
    if (__double_as_longlong(sum[p]) >= 0) grp[p] = keys[p] < gr.n ? gr.of[keys[p]] : REC_GROUP_NONE;
  uint32_t taken = 0, res_grp = REC_GROUP_NONE;                     // wave 0: the results so far, lane r the group of result r
  for (;;) {
    CfCand top{NONE, REC_GROUP_NONE, 0xffffffffu};
    for (I p = tid; p < tsize; p += NT) {                           // (uniform per wave: tsize is a multiple of 64)
      const long long sk = __double_as_longlong(sum[p]);
      CfCand cand{NONE, REC_GROUP_NONE, 0xffffffffu};               // (a dead slot carries no id: nothing orders the dead)
      if (sk >= 0) { cand.key = sk; cand.slot = grp[p]; cand.id = keys[p]; }
      const CfCand last = cf_shfl(top, 63);
      if (!__any(cand.key != NONE && better(cand, last))) continue;
      rec_sort64_rolled(cand, lane);
      const CfCand rev = cf_shfl(cand, 63 - (int)lane);
      if (better(rev, top)) top = rev;
      rec_merge_rolled(top, lane);
    }
    l_key[tid] = top.key;
    l_id[tid] = top.id;
    l_grp[tid] = top.slot;
    __syncthreads();
    if (w == 0) {
      for (uint32_t v = 1; v < NW; v++) {
        const CfCand o{l_key[v * 64 + 63 - lane], l_grp[v * 64 + 63 - lane], l_id[v * 64 + 63 - lane]};
        if (better(o, top)) top = o;
        rec_merge_rolled(top, lane);
      }
      const bool valid = top.key != NONE;                           // (the valid lanes are the first ones)
      const uint32_t g = top.slot;                                  // REC_GROUP_NONE in a lane that is not valid
      uint32_t same = 0;
#pragma nounroll                                                    // (unrolled, the shuffles become 128 scalar registers)
      for (uint32_t j = 0; j < 64; j++) {                           // (every lane shuffles)
        const uint32_t r = (uint32_t)__shfl((int)res_grp, (int)j), o = (uint32_t)__shfl((int)g, (int)j);
        same += (r == g ? 1u : 0u) + (j < lane && o == g ? 1u : 0u);
      }
      const bool grouped = g != REC_GROUP_NONE;
      const bool ok = valid && (!grouped || same < gr.cap);
      const uint64_t m = __ballot(ok);
      const uint32_t place = taken + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      const bool take = ok && place < k;
      if (take) {
        ids[(uint64_t)s * k + place] = top.id;
        scores[(uint64_t)s * k + place] = __longlong_as_double(top.key);
      }
      const uint32_t to = take ? place : 0xffffffffu;
#pragma nounroll
      for (uint32_t j = 0; j < 64; j++) {
        const uint32_t o = (uint32_t)__shfl((int)g, (int)j);
        if ((uint32_t)__shfl((int)to, (int)j) == lane) res_grp = o;
      }
      const uint64_t mf = __ballot(take && grouped && same + 1 == gr.cap);   // one lane per group that is full now
      if ((mf >> lane) & 1) full[__builtin_amdgcn_mbcnt_hi((uint32_t)(mf >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mf, 0u))] = g;
      const uint32_t room = k - taken, found = (uint32_t)__popcll(m);
      taken += found < room ? found : room;
      const bool done = taken >= k || __popcll(__ballot(valid)) < 64;
      if (lane == 63) {
        ctl[0] = done ? REC_GRP_DONE : (uint32_t)__popcll(mf);
        ctl[1] = (uint32_t)top.key;
        ctl[2] = (uint32_t)((unsigned long long)top.key >> 32);
        ctl[3] = top.id;
      }
    }
    __syncthreads();
    const uint32_t nf = ctl[0];
    if (nf == REC_GRP_DONE) break;
    const long long lk = (long long)(((unsigned long long)ctl[2] << 32) | ctl[1]);
    const uint32_t li = ctl[3];
    for (I p = tid; p < tsize; p += NT) {
      const long long sk = __double_as_longlong(sum[p]);
      if (sk < 0) continue;
      bool dead = sk > lk || (sk == lk && keys[p] <= li);           // not worse than the round's last: looked at
      const uint32_t g = grp[p];
      for (uint32_t c = 0; c < nf; c++) dead |= full[c] == g;       // (an ungrouped slot's REC_GROUP_NONE is never in the list)
      if (dead) sum[p] = -1.0;
    }
  }
  if (tid == 0) counts[s] = taken;
  __syncthreads();                                                  // before ws or the table is written again
}

// the LDS words the deep ending needs beside the table: the list of REC_DEEP_MAX {8-byte key, 4-byte id}, the select's 256 bins,
// and {candidates, collected, the pass's digit, what is still wanted of its bin, the bin's count, -, the OR of the keys (3 words),
// the OR of their complements (3 words)}
constexpr uint32_t REC_DEEP_MAX = 1024;       // SMATRIX_DEEP_MAX
constexpr uint32_t REC_DEEP_CTL = 12;
constexpr uint32_t rec_deep_words() { return REC_DEEP_MAX * 3 + 256 + REC_DEEP_CTL; }

// The deep ending of both tiers (smatrix_cf_recommend_deep with k > 64), run by a workgroup of NW waves over the finished table
// {keys, sq, sum} of tsize slots (a power of two >= 64) of session s: the first k <= REC_DEEP_MAX candidates in CfById's order.
//   1. The candidate test is folded into the sums (a slot that is no candidate, an empty one included, gets the sum -1.0); sq is not
//      read again, so ws may lie in it.  The candidates are counted and their keys' OR and AND taken: a key is RkCosine's (kernels/
//      rank_key.hpp), {the sum's bit pattern, 0xFFFFFFFF - id} -- larger is better, which is CfById's order, and unique in a table.
//   2. With more than k candidates: an MSB radix select of the k-th best key.  It starts at the highest digit in which the keys
//      differ (RkCosine::start).  A pass counts, in 256 bins, the digit of every key that agrees with the prefix chosen so far; wave
//      0 walks the bins from the top to the one that holds the `need`-th key, which becomes the next digit of the prefix.  When
//      that bin is wanted WHOLE (need == its count; at the last digit a bin holds one key) the select ends: the threshold is the
//      prefix with zeros below, and exactly k keys are at or above it.  At most 12 passes; a table without ties across the cut ends
//      within the score's digits.  With at most k candidates the threshold is RkCosine::zero(): everything.
//   3. The slots at or above the threshold go into the list in any order (a wave's share behind one atomic), the list is padded to
//      a power of two with the worst key, sorted by a bitonic network over LDS (a pair per thread and step) and stored, a thread
//      per place.  Keys are unique, so the sorted list does not depend on the order of collection.
// A thread meets the same slots in every pass (p = threadIdx.x + i * NW * 64), so the folded sums need no barrier of their own.
template <uint32_t NW, typename I>
__device__ __forceinline__ void rec_deep_table(const uint32_t* keys, const double* sq, double* sum, I tsize, uint32_t k, uint32_t s,
                                               uint32_t* __restrict__ ids, double* __restrict__ scores, uint32_t* __restrict__ counts,
                                               uint32_t* ws) {
  constexpr long long NONE = (long long)0x8000000000000000ull;
  constexpr uint32_t NT = NW * 64;
  typedef RkCosine RK;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long* l_key = reinterpret_cast<long long*>(ws);              // (ws is 8-byte aligned)
  uint32_t* l_id = ws + REC_DEEP_MAX * 2;
  uint32_t* hist = l_id + REC_DEEP_MAX;
  uint32_t* ctl = hist + 256;
  uint32_t mine = 0;
  RK::Acc acc = RK::acc0();
  for (I p = tid; p < tsize; p += NT) {
    const uint32_t b = keys[p];
    if (b != 0 && sq[p] > 0.0) {
      mine++;
      RK::acc_add(acc, RK::make(b, (uint64_t)__double_as_longlong(sum[p])));
    } else {
      sum[p] = -1.0;
    }
  }
  __syncthreads();                                                  // sq is read: ws may lie in it
  if (tid < REC_DEEP_CTL) ctl[tid] = 0;
  __syncthreads();
  for (uint32_t d = 32; d; d >>= 1) {
    mine += (uint32_t)__shfl_xor((int)mine, (int)d);
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) acc.w[j] |= (uint32_t)__shfl_xor((int)acc.w[j], (int)d);
  }
  if (lane == 0) {
    atomicAdd(&ctl[0], mine);
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) atomicOr(&ctl[6 + j], acc.w[j]);
  }
  __syncthreads();
  const uint32_t ncand = ctl[0];
  const uint32_t want = ncand < k ? ncand : k;
  RK::Key thr = RK::zero();
  if (ncand > k) {                                                  // (uniform: two keys and more, and they differ)
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) acc.w[j] = ctl[6 + j];
    uint32_t dg = RK::start(acc, thr), need = k;
    for (;;) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (I p = tid; p < tsize; p += NT) {
        const long long sk = __double_as_longlong(sum[p]);
        if (sk < 0) continue;
        const RK::Key key = RK::make(keys[p], (uint64_t)sk);
        if (RK::agrees_above(key, thr, dg)) atomicAdd(&hist[RK::digit(key, dg)], 1u);
      }
      __syncthreads();
      if (w == 0) {                                                 // lane l: the bins 255 - 4l .. 252 - 4l, from the top
        const uint32_t top = 255 - 4 * lane;
        const uint32_t c0 = hist[top], c1 = hist[top - 1], c2 = hist[top - 2], c3 = hist[top - 3];
        const uint32_t tot = c0 + c1 + c2 + c3;
        uint32_t incl = tot;
        for (uint32_t d = 1; d < 64; d <<= 1) {                     // (every lane shuffles)
          const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
          if (lane >= d) incl += o;
        }
        uint32_t above = incl - tot;                                // the keys in the bins above this lane's
        if (above < need && need <= incl) {                         // one lane: the pass counted `need` keys and more
          uint32_t dd = top, c = c0;
          if (above + c < need) {
            above += c; dd--; c = c1;
            if (above + c < need) {
              above += c; dd--; c = c2;
              if (above + c < need) { above += c; dd--; c = c3; }
            }
          }
          ctl[2] = dd;
          ctl[3] = need - above;
          ctl[4] = c;
        }
      }
      __syncthreads();
      RK::take_digit(thr, dg, ctl[2]);
      need = ctl[3];
      if (need == ctl[4] || dg == 0) break;                         // the bin is wanted whole: every key at or above the prefix
      dg--;
    }
  }
  for (I p0 = w * 64; p0 < tsize; p0 += NT) {                       // (uniform per wave: tsize is a multiple of 64)
    const I p = p0 + lane;
    const long long sk = __double_as_longlong(sum[p]);
    const uint32_t b = keys[p];
    const bool take = sk >= 0 && RK::ge(RK::make(b, (uint64_t)sk), thr);
    const uint64_t m = __ballot(take);
    if (m == 0) continue;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctl[1], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, 0);
    const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (take && at < REC_DEEP_MAX) {                                // (at < want <= REC_DEEP_MAX: exactly `want` slots are taken)
      l_key[at] = sk;
      l_id[at] = b;
    }
  }
  uint32_t P = 64;
  while (P < want) P <<= 1;
  for (uint32_t i = want + tid; i < P; i += NT) { l_key[i] = NONE; l_id[i] = 0xffffffffu; }
  __syncthreads();
  const CfById better;
#pragma nounroll
  for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
#pragma nounroll
    for (uint32_t j = k2 >> 1; j; j >>= 1) {
      for (uint32_t t = tid; t < P / 2; t += NT) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;   // the pair (i, i + j) of step j
        const CfCand a{l_key[i], 0u, l_id[i]}, c{l_key[o], 0u, l_id[o]};
        const bool down = (i & k2) == 0;                            // blocks alternate direction; the last pass (k2 == P) is best-first
        if (better(c, a) == down) {
          l_key[i] = c.key; l_id[i] = c.id;
          l_key[o] = a.key; l_id[o] = a.id;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t r = tid; r < want; r += NT) {
    ids[(uint64_t)s * k + r] = l_id[r];
    scores[(uint64_t)s * k + r] = __longlong_as_double(l_key[r]);
  }
  if (tid == 0) counts[s] = want;
  __syncthreads();                                                  // before ws or the table is written again
}

// ---- tiers ----------------------------------------------------------------------------------------------------------------
// bound = the sum of the row sizes (slots) of the session's DISTINCT items: every candidate is a non-empty cell of one of
// those rows, whatever quirk the row carries.  Duplicates are found exactly for sessions of up to REC_DEDUP_MAX items
// (a wave compares every position with all earlier ones); a longer session counts a repeated row again, and its bound is
// cut to all_cells, the cells the arena can hold (no session has more candidates than the matrix has cells).  A table never
// needs more than 2^32 slots: its keys are distinct non-zero 32-bit ids.
// A session with no row at all has no candidate: its count is written here.  tlg[s] = log2 of the session's table size.
// <true>: the table also holds the E ids of the session's exclusion list (a repeated id only wastes a slot), so the tier is chosen
// on bound + L + E; every weight of the session is checked (ctl->bad).
constexpr uint64_t REC_DEDUP_MAX = 8192;
constexpr uint32_t REC_MAX_LG = 32;

template <bool F>
__global__ __launch_bounds__(256) void k_rec_bound(DirSlot* dir, uint32_t dmask, uint32_t n, const uint64_t* __restrict__ off,
                                                   const uint32_t* __restrict__ items, uint64_t all_cells, RecCtl* ctl,
                                                   uint32_t* lds_list, uint8_t* tlg, uint32_t* big_list, unsigned long long* big_off,
                                                   uint32_t* __restrict__ counts, RecFilt f) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t s = wave; s < n; s += nwaves) {
    const uint64_t b0 = off[s], L = off[s + 1] - b0;
    const bool exact = L <= REC_DEDUP_MAX;
    uint64_t bound = 0;
    for (uint64_t c0 = 0; c0 < L; c0 += 64) {                       // (wave-uniform loops: the shuffles need every lane)
      const uint64_t i = c0 + lane;
      const uint32_t a = i < L ? items[b0 + i] : 0u;
      if (F && f.w && i < L && !rec_weight_ok(f.w[b0 + i])) ctl->bad = 1u;
      uint64_t sz = 0;
      uint4 sn;
      if (i < L && dir_find(dir, dmask, a, &sn) && sn.z != 0) sz = 1ull << meta_lg(sn.x);
      if (exact && __any(sz != 0)) {
        bool dup = false;
        for (uint64_t e0 = 0; e0 <= c0; e0 += 64) {                 // the positions before mine, 64 at a time
          const uint32_t e = e0 + lane < L ? items[b0 + e0 + lane] : 0u;
          const uint32_t lim = e0 == c0 ? lane : 64u;
          for (uint32_t j = 0; j < 64; j++) {
            const uint32_t o = (uint32_t)__shfl((int)e, (int)j);
            dup |= j < lim && o == a;
          }
        }
        if (dup) sz = 0;
      }
      bound += sz;
    }
    for (uint32_t d = 32; d; d >>= 1) bound += __shfl_xor(bound, d);
    if (lane != 0) continue;
    if (bound == 0) { counts[s] = 0; continue; }
    if (bound > all_cells) bound = all_cells;
    uint64_t need = bound + L;
    if (F && f.ex_off) need += f.ex_off[s + 1] - f.ex_off[s];
    if (need > (1ull << REC_MAX_LG)) need = 1ull << REC_MAX_LG;
    if (need <= REC_LDS_SLOTS) {
      tlg[s] = (uint8_t)rec_lg(need, 6);
      lds_list[atomicAdd(&ctl->n_lds, 1u)] = s;
    } else {
      const uint32_t lg = rec_lg(need, REC_GL_MIN_LG);
      tlg[s] = (uint8_t)lg;
      const uint32_t idx = atomicAdd(&ctl->n_big, 1u);
      big_list[idx] = s;
      big_off[idx] = atomicAdd(&ctl->total_slots, 1ull << lg);
      atomicMax(&ctl->max_slots, 1ull << lg);
      atomicMax(&ctl->max_len, (uint32_t)L);
    }
  }
}

// ---- LDS tier: a workgroup per session ---------------------------------------------------------------------------------------
// (the body of k_rec_lds<F> and of k_rec_lds_sim<F>; S: the score is f.m's, not the cosine's; R: smatrix_cf_rank's ending in place
// of the top-k, k_rec_lds_rank<F> and k_rec_lds_rank_sim<F>: scores and counts are then the targets' and the candidate counts;
// G: smatrix_cf_recommend_grouped's ending, rec_group_table, k_rec_lds_grouped<F> and k_rec_lds_grouped_sim<F>;
// D: smatrix_cf_recommend_deep's ending, rec_deep_table, k_rec_lds_deep<F> and k_rec_lds_deep_sim<F>;
// C: smatrix_cf_recommend_scoped's test on a claimed key, k_rec_lds_scoped and k_rec_lds_grouped_scoped)
template <bool F, bool S, bool R, bool G = false, bool D = false, bool C = false>
__device__ __forceinline__ void rec_lds(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                        const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                        const uint64_t* __restrict__ off, const uint32_t* __restrict__ items, uint32_t k,
                                        uint32_t* __restrict__ ids, double* __restrict__ scores, uint32_t* __restrict__ counts,
                                        const RecFilt& f, const RecRank& rk, const RecGroup& gr = RecGroup{},
                                        const RecScope& sc = RecScope{}) {
  __shared__ uint32_t s_key[REC_LDS_SLOTS];
  __shared__ double s_sq[REC_LDS_SLOTS];
  __shared__ double s_sum[REC_LDS_SLOTS];
  constexpr long long NONE = (long long)0x8000000000000000ull;
  constexpr uint32_t NW = REC_LDS_THREADS / 64;
  const CfById better;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t n = ctl->n_lds;
  for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
    const uint32_t s = lds_list[q];
    const uint32_t tsize = 1u << tlg[s], mask = tsize - 1;    // (<= REC_LDS_SLOTS here)
    const uint64_t b0 = off[s], L = off[s + 1] - b0;
    uint64_t l0 = 0;                                                // the session's scope list (uniform; read where a key is claimed)
    const uint32_t nl = C ? rec_scope_len(sc, s, &l0) : 0u;
    for (uint32_t i = tid; i < tsize; i += REC_LDS_THREADS) { s_key[i] = 0; s_sq[i] = 0.0; s_sum[i] = 0.0; }
    __syncthreads();
    for (uint32_t i = tid; i < L; i += REC_LDS_THREADS) {          // the session's items: excluded, first positions
      const uint32_t a = items[b0 + i];
      if (a == 0) continue;
      bool claimed;
      const uint32_t h = rec_slot<true>(s_key, mask, a, &claimed);
      s_sq[h] = -1.0;
      atomicMax(reinterpret_cast<uint32_t*>(&s_sum[h]), rec_first_word(i));
    }
    if (F && f.ex_off) {                                            // the exclusion list: excluded, and no more
      const uint64_t e0 = f.ex_off[s], E = f.ex_off[s + 1] - e0;
      for (uint64_t i = tid; i < E; i += REC_LDS_THREADS) {
        const uint32_t a = f.ex[e0 + i];
        if (a == 0) continue;
        bool claimed;
        s_sq[rec_slot<true>(s_key, mask, a, &claimed)] = -1.0;
      }
    }
    __syncthreads();
    bool seen0 = false;                                             // (item 0 is never a key: its duplicates are told here)
    for (uint32_t i = 0; i < L; i++) {                              // session order; everything up to the scan is uniform
      const uint32_t a = items[b0 + i];
      if (a == 0) {
        if (seen0) continue;
        seen0 = true;
      } else if (rec_low_word(&s_sum[rec_find(s_key, mask, a)]) != rec_first_word(i)) {
        continue;                                                   // a later occurrence
      }
      uint4 sn;
      if (!dir_find(dir, dmask, a, &sn) || sn.z == 0) continue;
      const double sa = rec_row_total<S>(dir, dmask, arena, a, f.m);
      const double wa = F && f.w ? f.w[b0 + i] : 1.0;
      const uint32_t size = 1u << meta_lg(sn.x);
      const uint64_t* cells = row_cells(arena, sn.z);
      for (uint32_t p = tid; p < size; p += REC_LDS_THREADS) {
        const uint64_t c = cells[p];
        const uint32_t b = cell_key(c);
        if (b == 0) continue;                                       // an empty cell, or column 0 (the totals)
        bool claimed;
        const uint32_t h = rec_slot<true>(s_key, mask, b, &claimed);
        double sqb;
        if (claimed) {
          if (F && rec_denied(f, b)) { s_sq[h] = -1.0; continue; }  // a denied key: excluded from here on
          if (C && rec_out_of_scope(sc, l0, nl, b)) { s_sq[h] = -1.0; continue; }   // ... and a key out of the session's scope
          sqb = rec_col_total<S>(dir, dmask, arena, b, f.m);
          s_sq[h] = sqb;
        } else {
          sqb = s_sq[h];
          if (sqb < 0.0) continue;                                  // an item of the session, an excluded, a denied or an out-of-scope key
          // claimed by another lane of this row (a twice-held key).  If that lane is about to deny the key, or to find it out of
          // scope, this term is added to a sum nobody reads: the selection below takes s_sq > 0 after the barrier
          if (sqb == 0.0) sqb = rec_col_total<S>(dir, dmask, arena, b, f.m);
        }
        double term = rec_term<S>(cell_val(c), sa, sqb, f.m);
        if (F) term = __dmul_rn(wa, term);                          // (rounded before the add; wa == 1.0 changes no bit)
        __hip_atomic_fetch_add(&s_sum[h], term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      __syncthreads();
    }
    __syncthreads();
    if (R) {
      // the table fills the LDS two workgroups of a CU share: the candidate test goes into the sums, and s_sq holds the counters
      for (uint32_t i = tid; i < tsize; i += REC_LDS_THREADS)
        if (s_key[i] != 0 && !(s_sq[i] > 0.0)) s_sum[i] = -1.0;
      __syncthreads();
      rec_rank_table<true, NW>(s_key, s_sq, s_sum, tsize, rk, s, counts, reinterpret_cast<uint32_t*>(s_sq));
      continue;                                                     // (its last barrier stands before the next session's clearing)
    }
    if (G) {
      // the table must outlive the rounds: the groups take the first 16 KiB of s_sq, the waves' lists lie in the rest of it
      rec_group_table<NW>(s_key, s_sq, s_sum, tsize, gr, k, s, ids, scores, counts, reinterpret_cast<uint32_t*>(s_sq) + REC_LDS_SLOTS);
      continue;
    }
    if (D) {
      // the table must outlive the select's passes: the list, the bins and the control words lie in s_sq, free once it is folded
      rec_deep_table<NW>(s_key, s_sq, s_sum, tsize, k, s, ids, scores, counts, reinterpret_cast<uint32_t*>(s_sq));
      continue;
    }
    // the k best: every wave over its 64-slot steps (k_cf_topk's loop), then wave 0 merges the waves' lists
    CfCand top{NONE, 0xffffffffu, 0xffffffffu};
    for (uint32_t p0 = w * 64; p0 < tsize; p0 += REC_LDS_THREADS) {
      const uint32_t p = p0 + lane;
      const uint32_t b = s_key[p];
      CfCand cand{NONE, 0xffffffffu, b};
      if (b != 0 && s_sq[p] > 0.0) cand.key = __double_as_longlong(s_sum[p]);
      const CfCand kth = cf_shfl(top, (int)k - 1);
      if (!__any(cand.key != NONE && better(cand, kth))) continue;
      cf_sort64<CfById>(cand, lane);
      const CfCand rev = cf_shfl(cand, 63 - (int)lane);
      if (better(rev, top)) top = rev;
      cf_merge_stages<CfById>(top, lane, 32);
    }
    __syncthreads();                                                // the table is read: its first words hold the lists
    long long* l_key = reinterpret_cast<long long*>(s_sq);
    l_key[w * 64 + lane] = top.key;
    s_key[w * 64 + lane] = top.id;
    __syncthreads();
    if (w == 0) {
      for (uint32_t v = 1; v < NW; v++) {
        const CfCand o{l_key[v * 64 + 63 - lane], 0xffffffffu, s_key[v * 64 + 63 - lane]};
        if (better(o, top)) top = o;
        cf_merge_stages<CfById>(top, lane, 32);
      }
      const bool have = lane < k && top.key != NONE;
      if (have) {
        ids[(uint64_t)s * k + lane] = top.id;
        scores[(uint64_t)s * k + lane] = __longlong_as_double(top.key);
      }
      const uint64_t m = __ballot(have);
      if (lane == 0) counts[s] = (uint32_t)__popcll(m);
    }
    __syncthreads();                                                // before the next session clears the table
  }
}

template <bool F>
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                             const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                                             const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                             uint32_t k, uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                             uint32_t* __restrict__ counts, RecFilt f) {
  rec_lds<F, false, false>(dir, dmask, arena, ctl, lds_list, tlg, off, items, k, ids, scores, counts, f, RecRank{});
}
template <bool F>
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds_sim(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                                 const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                                                 const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                                 uint32_t k, uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                                 uint32_t* __restrict__ counts, RecFilt f) {
  rec_lds<F, true, false>(dir, dmask, arena, ctl, lds_list, tlg, off, items, k, ids, scores, counts, f, RecRank{});
}
// smatrix_cf_rank's instances: the same fill, rec_rank_table at the end; ncand[s] = the session's candidates
template <bool F>
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds_rank(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                                  const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                                                  const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                                  RecRank rk, uint32_t* __restrict__ ncand, RecFilt f) {
  rec_lds<F, false, true>(dir, dmask, arena, ctl, lds_list, tlg, off, items, 0u, nullptr, nullptr, ncand, f, rk);
}
template <bool F>
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds_rank_sim(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                                      const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                                                      const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                                      RecRank rk, uint32_t* __restrict__ ncand, RecFilt f) {
  rec_lds<F, true, true>(dir, dmask, arena, ctl, lds_list, tlg, off, items, 0u, nullptr, nullptr, ncand, f, rk);
}

// smatrix_cf_recommend_grouped's instances: the same fill, rec_group_table at the end
static_assert(REC_LDS_SLOTS * 4 + rec_group_words(REC_LDS_THREADS / 64) * 4 <= REC_LDS_SLOTS * 8, "the groups and the lists share s_sq");
template <bool F>
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds_grouped(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                                     const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                                                     const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                                     uint32_t k, uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                                     uint32_t* __restrict__ counts, RecFilt f, RecGroup gr) {
  rec_lds<F, false, false, true>(dir, dmask, arena, ctl, lds_list, tlg, off, items, k, ids, scores, counts, f, RecRank{}, gr);
}
template <bool F>
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds_grouped_sim(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                                         const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                                                         const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                                         uint32_t k, uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                                         uint32_t* __restrict__ counts, RecFilt f, RecGroup gr) {
  rec_lds<F, true, false, true>(dir, dmask, arena, ctl, lds_list, tlg, off, items, k, ids, scores, counts, f, RecRank{}, gr);
}

// smatrix_cf_recommend_scoped's instances: the filtered _sim bodies of the top-k and of the grouped ending with the scope test where a
// key is claimed (plain cosine goes through sim_score too: sqrt(A) * sqrt(B) + 0.0 is the plain term's denominator, bit for bit)
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds_scoped(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                                    const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                                                    const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                                    uint32_t k, uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                                    uint32_t* __restrict__ counts, RecFilt f, RecScope sc) {
  rec_lds<true, true, false, false, false, true>(dir, dmask, arena, ctl, lds_list, tlg, off, items, k, ids, scores, counts, f, RecRank{},
                                                 RecGroup{}, sc);
}
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds_grouped_scoped(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                                            const uint32_t* __restrict__ lds_list,
                                                                            const uint8_t* __restrict__ tlg, const uint64_t* __restrict__ off,
                                                                            const uint32_t* __restrict__ items, uint32_t k,
                                                                            uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                                            uint32_t* __restrict__ counts, RecFilt f, RecGroup gr, RecScope sc) {
  rec_lds<true, true, false, true, false, true>(dir, dmask, arena, ctl, lds_list, tlg, off, items, k, ids, scores, counts, f, RecRank{}, gr,
                                                sc);
}

// smatrix_cf_recommend_deep's instances (k > 64): the same fill, rec_deep_table at the end
static_assert(rec_deep_words() * 4 <= REC_LDS_SLOTS * 8, "the list, the bins and the control words share s_sq");
template <bool F>
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds_deep(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                                  const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                                                  const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                                  uint32_t k, uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                                  uint32_t* __restrict__ counts, RecFilt f) {
  rec_lds<F, false, false, false, true>(dir, dmask, arena, ctl, lds_list, tlg, off, items, k, ids, scores, counts, f, RecRank{});
}
template <bool F>
__global__ __launch_bounds__(REC_LDS_THREADS) void k_rec_lds_deep_sim(DirSlot* dir, uint32_t dmask, uint8_t* arena, const RecCtl* ctl,
                                                                      const uint32_t* __restrict__ lds_list, const uint8_t* __restrict__ tlg,
                                                                      const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                                      uint32_t k, uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                                      uint32_t* __restrict__ counts, RecFilt f) {
  rec_lds<F, true, false, false, true>(dir, dmask, arena, ctl, lds_list, tlg, off, items, k, ids, scores, counts, f, RecRank{});
}

// ---- global tier -----------------------------------------------------------------------------------------------------------
// Sessions are processed in GROUPS by their table offset (big_off / G): group g's tables live at big_off - g * G in the
// buffers gk (keys), gq (sqrt of the totals, -1: an item), gs (sums), which the host has zeroed.  owner[segment] = the session
// index (in big_list) whose table holds the segment; zpos[idx] = 2^32-1 - the first position of item 0 in the session.
struct RecGl {
  uint32_t* gk;
  double* gq;
  double* gs;
  uint32_t* owner;
  uint32_t* zpos;
  const uint32_t* big_list;
  const unsigned long long* big_off;
  const uint8_t* tlg;
  uint32_t n_big;
  uint32_t g;
  unsigned long long G;
};

__device__ __forceinline__ bool rec_in_group(const RecGl& R, uint32_t idx, uint64_t* loc) {
  const uint64_t o = R.big_off[idx];
  if (o / R.G != R.g) return false;
  *loc = o - (uint64_t)R.g * R.G;
  return true;
}

// a workgroup per session: the items as excluded keys, item 0's first position, the owners of the table's segments;
// <true>: the exclusion list as excluded keys
template <bool F>
__global__ __launch_bounds__(256) void k_rec_gl_init(RecGl R, const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                     RecFilt f) {
  for (uint32_t idx = blockIdx.x; idx < R.n_big; idx += gridDim.x) {
    uint64_t loc;
    if (!rec_in_group(R, idx, &loc)) continue;
    const uint32_t s = R.big_list[idx];
    const uint64_t tsize = 1ull << R.tlg[s], b0 = off[s], L = off[s + 1] - b0;
    for (uint64_t j = threadIdx.x; j < tsize / REC_SEG; j += blockDim.x) R.owner[loc / REC_SEG + j] = idx;
    uint32_t* keys = R.gk + loc;
    for (uint64_t i = threadIdx.x; i < L; i += blockDim.x) {
      const uint32_t a = items[b0 + i];
      if (a == 0) { atomicMax(&R.zpos[idx], rec_first_word(i)); continue; }
      bool claimed;
      const uint32_t h = rec_slot<false>(keys, (uint32_t)(tsize - 1), a, &claimed);
      R.gq[loc + h] = -1.0;
      atomicMax(reinterpret_cast<uint32_t*>(&R.gs[loc + h]), rec_first_word(i));
    }
    if (F && f.ex_off) {
      const uint64_t e0 = f.ex_off[s], E = f.ex_off[s + 1] - e0;
      for (uint64_t i = threadIdx.x; i < E; i += blockDim.x) {
        const uint32_t a = f.ex[e0 + i];
        if (a == 0) continue;
        bool claimed;
        R.gq[loc + rec_slot<false>(keys, (uint32_t)(tsize - 1), a, &claimed)] = -1.0;
      }
    }
  }
}

// per (position p0 + j, session idx) with j < np: the 512-cell chunks of the row of the session's item there, 0 for a later
// occurrence, an item without a row, a session of this length or less, a session of another group
__global__ __launch_bounds__(256) void k_rec_gl_plan(RecGl R, DirSlot* dir, uint32_t dmask, const uint64_t* __restrict__ off,
                                                     const uint32_t* __restrict__ items, uint32_t p0, uint32_t np, uint32_t* cnt) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)np * R.n_big) return;
  const uint32_t idx = (uint32_t)(t % R.n_big), p = p0 + (uint32_t)(t / R.n_big);
  uint32_t c = 0;
  uint64_t loc;
  if (rec_in_group(R, idx, &loc)) {
    const uint32_t s = R.big_list[idx];
    const uint64_t b0 = off[s], L = off[s + 1] - b0;
    if (p < L) {
      const uint32_t a = items[b0 + p];
      const uint32_t mask = (uint32_t)((1ull << R.tlg[s]) - 1u);   // (tables of 2^32 slots: mask 2^32 - 1)
      const bool first = a == 0 ? R.zpos[idx] == rec_first_word(p)
                                : rec_low_word(&R.gs[loc + rec_find(R.gk + loc, mask, a)]) == rec_first_word(p);
      uint4 sn;
      if (first && dir_find(dir, dmask, a, &sn) && sn.z != 0) c = ((1u << meta_lg(sn.x)) + REC_CHUNK - 1) / REC_CHUNK;
    }
  }
  cnt[t] = c;
}

// position p = p0 + j: a wave per chunk task; scan[j * n_big + idx] = the first task of session idx (scan of k_rec_gl_plan's counts)
// (the body of k_rec_gl_scan<F>, of k_rec_gl_scan_sim<F> and, with C, of k_rec_gl_scan_scoped, as rec_lds)
template <bool F, bool S, bool C = false>
__device__ __forceinline__ void rec_gl_scan(const RecGl& R, DirSlot* dir, uint32_t dmask, uint8_t* arena,
                                            const uint64_t* __restrict__ off, const uint32_t* __restrict__ items, uint32_t p0,
                                            uint32_t j, const uint64_t* __restrict__ scan, const RecFilt& f,
                                            const RecScope& scope = RecScope{}) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint64_t* sc = scan + (uint64_t)j * R.n_big;
  const uint64_t t0 = sc[0], t1 = sc[R.n_big];
  for (uint64_t t = t0 + wave; t < t1; t += nwaves) {
    uint32_t lo = 0, hi = R.n_big;                                  // the last session whose first task is <= t
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (sc[mid] <= t) lo = mid; else hi = mid; }
    const uint32_t idx = lo;
    const uint64_t chunk = t - sc[idx];
    const uint64_t loc = R.big_off[idx] - (uint64_t)R.g * R.G;
    const uint32_t s = R.big_list[idx];
    const uint32_t mask = (uint32_t)((1ull << R.tlg[s]) - 1u);   // (tables of 2^32 slots: mask 2^32 - 1)
    const uint32_t a = items[off[s] + p0 + j];
    uint64_t l0 = 0;                                                // the session's scope list (uniform per wave)
    const uint32_t nl = C ? rec_scope_len(scope, s, &l0) : 0u;
    uint4 sn;
    dir_find(dir, dmask, a, &sn);                                   // (there: the plan gave it chunks)
    const double sa = rec_row_total<S>(dir, dmask, arena, a, f.m);
    const double wa = F && f.w ? f.w[off[s] + p0 + j] : 1.0;
    const uint32_t size = 1u << meta_lg(sn.x);
    const uint64_t* cells = row_cells(arena, sn.z);
    uint32_t* keys = R.gk + loc;
    double* sq = R.gq + loc;
    double* sum = R.gs + loc;
    uint64_t cv[REC_CHUNK / 64];
#pragma unroll
    for (uint32_t u = 0; u < REC_CHUNK / 64; u++) {                 // the chunk's loads all in flight
      const uint64_t p = chunk * REC_CHUNK + u * 64 + lane;
      cv[u] = p < size ? cells[p] : 0ull;
    }
#pragma unroll
    for (uint32_t u = 0; u < REC_CHUNK / 64; u++) {
      const uint32_t b = cell_key(cv[u]);
      if (b == 0) continue;
      bool claimed;
      const uint32_t h = rec_slot<false>(keys, mask, b, &claimed);
      double sqb;
      if (claimed) {
        if (F && rec_denied(f, b)) { sq[h] = -1.0; continue; }
        if (C && rec_out_of_scope(scope, l0, nl, b)) { sq[h] = -1.0; continue; }
        sqb = rec_col_total<S>(dir, dmask, arena, b, f.m);
        sq[h] = sqb;
      } else {
        sqb = __hip_atomic_load(&sq[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sqb < 0.0) continue;
        if (sqb == 0.0) sqb = rec_col_total<S>(dir, dmask, arena, b, f.m);   // (the claimer of a denied or out-of-scope key may be between
      }                                                               // its claim and its store: as in k_rec_lds, the endings read gq > 0 later)
      double term = rec_term<S>(cell_val(cv[u]), sa, sqb, f.m);
      if (F) term = __dmul_rn(wa, term);
      unsafeAtomicAdd(&sum[h], term);
    }
  }
}

template <bool F>
__global__ __launch_bounds__(256) void k_rec_gl_scan(RecGl R, DirSlot* dir, uint32_t dmask, uint8_t* arena,
                                                     const uint64_t* __restrict__ off, const uint32_t* __restrict__ items, uint32_t p0,
                                                     uint32_t j, const uint64_t* __restrict__ scan, RecFilt f) {
  rec_gl_scan<F, false>(R, dir, dmask, arena, off, items, p0, j, scan, f);
}
template <bool F>
__global__ __launch_bounds__(256) void k_rec_gl_scan_sim(RecGl R, DirSlot* dir, uint32_t dmask, uint8_t* arena,
                                                         const uint64_t* __restrict__ off, const uint32_t* __restrict__ items, uint32_t p0,
                                                         uint32_t j, const uint64_t* __restrict__ scan, RecFilt f) {
  rec_gl_scan<F, true>(R, dir, dmask, arena, off, items, p0, j, scan, f);
}
__global__ __launch_bounds__(256) void k_rec_gl_scan_scoped(RecGl R, DirSlot* dir, uint32_t dmask, uint8_t* arena,
                                                            const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                            uint32_t p0, uint32_t j, const uint64_t* __restrict__ scan, RecFilt f,
                                                            RecScope sc) {
  rec_gl_scan<true, true, true>(R, dir, dmask, arena, off, items, p0, j, scan, f, sc);
}

// a wave per REC_SEG-slot segment of the group's tables: its 64 best -> lk / li (64 entries per segment, best first)
__global__ __launch_bounds__(256) void k_rec_gl_topk(RecGl R, uint64_t nseg, uint32_t k, long long* __restrict__ lk,
                                                     uint32_t* __restrict__ li) {
  constexpr long long NONE = (long long)0x8000000000000000ull;
  const CfById better;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t g = wave; g < nseg; g += nwaves) {
    if (R.owner[g] == 0xffffffffu) continue;
    CfCand top{NONE, 0xffffffffu, 0xffffffffu};
    for (uint64_t p0 = g * REC_SEG; p0 < (g + 1) * REC_SEG; p0 += 64) {
      const uint64_t p = p0 + lane;
      const uint32_t b = R.gk[p];
      CfCand cand{NONE, 0xffffffffu, b};
      if (b != 0 && R.gq[p] > 0.0) cand.key = __double_as_longlong(R.gs[p]);
      const CfCand kth = cf_shfl(top, (int)k - 1);
      if (!__any(cand.key != NONE && better(cand, kth))) continue;
      cf_sort64<CfById>(cand, lane);
      const CfCand rev = cf_shfl(cand, 63 - (int)lane);
      if (better(rev, top)) top = rev;
      cf_merge_stages<CfById>(top, lane, 32);
    }
    lk[g * 64 + lane] = top.key;
    li[g * 64 + lane] = top.id;
  }
}

// a workgroup per session of the group: its segments' lists merged (each wave a share, then wave 0 over the waves), the k best out
__global__ __launch_bounds__(REC_MERGE_THREADS) void k_rec_gl_merge(RecGl R, uint32_t k, const long long* __restrict__ lk,
                                                                    const uint32_t* __restrict__ li, uint32_t* __restrict__ ids,
                                                                    double* __restrict__ scores, uint32_t* __restrict__ counts) {
  constexpr long long NONE = (long long)0x8000000000000000ull;
  constexpr uint32_t NW = REC_MERGE_THREADS / 64;
  __shared__ long long m_key[NW * 64];
  __shared__ uint32_t m_id[NW * 64];
  const CfById better;
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t idx = blockIdx.x; idx < R.n_big; idx += gridDim.x) {
    uint64_t loc;
    if (!rec_in_group(R, idx, &loc)) continue;
    const uint32_t s = R.big_list[idx];
    const uint64_t g0 = loc / REC_SEG, ns = (1ull << R.tlg[s]) / REC_SEG;
    CfCand top{NONE, 0xffffffffu, 0xffffffffu};
    for (uint64_t g = g0 + w; g < g0 + ns; g += NW) {
      const CfCand o{lk[g * 64 + 63 - lane], 0xffffffffu, li[g * 64 + 63 - lane]};
      if (better(o, top)) top = o;
      cf_merge_stages<CfById>(top, lane, 32);
    }
    m_key[w * 64 + lane] = top.key;
    m_id[w * 64 + lane] = top.id;
    __syncthreads();
    if (w == 0) {
      for (uint32_t v = 1; v < NW; v++) {
        const CfCand o{m_key[v * 64 + 63 - lane], 0xffffffffu, m_id[v * 64 + 63 - lane]};
        if (better(o, top)) top = o;
        cf_merge_stages<CfById>(top, lane, 32);
      }
      const bool have = lane < k && top.key != NONE;
      if (have) {
        ids[(uint64_t)s * k + lane] = top.id;
        scores[(uint64_t)s * k + lane] = __longlong_as_double(top.key);
      }
      const uint64_t m = __ballot(have);
      if (lane == 0) counts[s] = (uint32_t)__popcll(m);
    }
    __syncthreads();
  }
}

// smatrix_cf_rank's ending of the global tier, in place of k_rec_gl_topk + k_rec_gl_merge: a workgroup per session of the group
__global__ __launch_bounds__(REC_MERGE_THREADS) void k_rec_gl_rank(RecGl R, RecRank rk, uint32_t* __restrict__ ncand) {
  constexpr uint32_t NW = REC_MERGE_THREADS / 64;
  __shared__ uint32_t part[NW * 64 + NW];
  for (uint32_t idx = blockIdx.x; idx < R.n_big; idx += gridDim.x) {
    uint64_t loc;
    if (!rec_in_group(R, idx, &loc)) continue;
    const uint32_t s = R.big_list[idx];
    rec_rank_table<false, NW>(R.gk + loc, R.gq + loc, R.gs + loc, 1ull << R.tlg[s], rk, s, ncand, part);
  }
}

// smatrix_cf_recommend_grouped's ending of the global tier, in place of k_rec_gl_topk + k_rec_gl_merge (a segment's 64 best may all be
// of one group): a workgroup per session of the group over its whole table, gq reused for the groups -- k_rec_gl_rank's shape
__global__ __launch_bounds__(REC_MERGE_THREADS) void k_rec_gl_grouped(RecGl R, RecGroup gr, uint32_t k, uint32_t* __restrict__ ids,
                                                                      double* __restrict__ scores, uint32_t* __restrict__ counts) {
  constexpr uint32_t NW = REC_MERGE_THREADS / 64;
  __shared__ __attribute__((aligned(8))) uint32_t ws[rec_group_words(NW)];
  for (uint32_t idx = blockIdx.x; idx < R.n_big; idx += gridDim.x) {
    uint64_t loc;
    if (!rec_in_group(R, idx, &loc)) continue;
    const uint32_t s = R.big_list[idx];
    rec_group_table<NW>(R.gk + loc, R.gq + loc, R.gs + loc, 1ull << R.tlg[s], gr, k, s, ids, scores, counts, ws);
  }
}

// smatrix_cf_recommend_deep's ending of the global tier (k > 64), in place of k_rec_gl_topk + k_rec_gl_merge (a segment's list holds 64
// entries): a workgroup per session of the group over its whole table, gq folded into gs first -- k_rec_gl_rank's shape
__global__ __launch_bounds__(REC_MERGE_THREADS) void k_rec_gl_deep(RecGl R, uint32_t k, uint32_t* __restrict__ ids, double* __restrict__ scores,
                                                                   uint32_t* __restrict__ counts) {
  constexpr uint32_t NW = REC_MERGE_THREADS / 64;
  __shared__ __attribute__((aligned(8))) uint32_t ws[rec_deep_words()];
  for (uint32_t idx = blockIdx.x; idx < R.n_big; idx += gridDim.x) {
    uint64_t loc;
    if (!rec_in_group(R, idx, &loc)) continue;
    const uint32_t s = R.big_list[idx];
    rec_deep_table<NW>(R.gk + loc, R.gq + loc, R.gs + loc, 1ull << R.tlg[s], k, s, ids, scores, counts, ws);
  }
}

// before the kernels above: every answer the call owns reads "no answer" (SMATRIX_RANK_NONE, 0.0)
__global__ __launch_bounds__(256) void k_rec_rank_fill(uint32_t n, RecRank rk) {
  const uint64_t j0 = rk.t_off[0], j1 = rk.t_off[n];
  for (uint64_t j = j0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < j1; j += (uint64_t)gridDim.x * blockDim.x) {
    rk.ranks[j] = 0xffffffffu;
    rk.scores[j] = 0.0;
  }
}

// ---- smatrix_cf_recommend_fill: the free places of a short result, from the caller's list ---------------------------------
// Enqueued behind the recommend launches of both tiers: it reads ids / counts as they wrote them and knows no tier.  A wave per
// session: n_scored[s] = counts[s]; a full session ends there.  Otherwise the list is walked 64 ids a step, a lane each.  An id is
// taken unless it is 0, denied, an item of the session or on its exclusion list (both 64 at a time through the wave), in the
// result already -- the <= 64 ids of the result live in lanes, `mine`, 0 for a free place -- or the id of a lane below in the same
// step.  Every test is a function of the id alone, so of the lanes of a step that hold one id the lowest decides for all.  The
// lanes taken are numbered by mbcnt, cut at the room left, and handed to the lanes that own the new places: list order is kept.
__global__ __launch_bounds__(256) void k_rec_fill(uint32_t n, const uint64_t* __restrict__ off, const uint32_t* __restrict__ items, uint32_t k,
                                                  const uint32_t* __restrict__ fill, uint32_t n_fill, uint32_t* ids, double* scores,
                                                  uint32_t* counts, uint32_t* __restrict__ n_scored, RecFilt f) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t s = wave; s < n; s += nwaves) {                     // (wave-uniform throughout: the shuffles need every lane)
    uint32_t have = counts[s];
    if (lane == 0) n_scored[s] = have;
    if (have >= k || n_fill == 0) continue;
    const uint64_t b0 = off[s], L = off[s + 1] - b0;
    const uint64_t e0 = f.ex_off ? f.ex_off[s] : 0ull, E = f.ex_off ? f.ex_off[s + 1] - e0 : 0ull;
    uint32_t mine = lane < have ? ids[(uint64_t)s * k + lane] : 0u;
    for (uint32_t j0 = 0; j0 < n_fill && have < k; j0 += 64) {
      const uint32_t fid = j0 + lane < n_fill ? fill[j0 + lane] : 0u;
      bool ok = fid != 0 && !rec_denied(f, fid);
      if (!__any(ok)) continue;
      for (uint64_t c0 = 0; c0 < L; c0 += 64) {
        const uint32_t e = c0 + lane < L ? items[b0 + c0 + lane] : 0u;   // (a 0 beyond the end meets no id that is still ok)
        for (uint32_t j = 0; j < 64; j++) ok &= (uint32_t)__shfl((int)e, (int)j) != fid;
      }
      for (uint64_t c0 = 0; c0 < E; c0 += 64) {
        const uint32_t e = c0 + lane < E ? f.ex[e0 + c0 + lane] : 0u;
        for (uint32_t j = 0; j < 64; j++) ok &= (uint32_t)__shfl((int)e, (int)j) != fid;
      }
      for (uint32_t j = 0; j < 64; j++) {
        const uint32_t r = (uint32_t)__shfl((int)mine, (int)j), o = (uint32_t)__shfl((int)fid, (int)j);   // (every lane shuffles)
        ok &= r != fid;                                             // in the result, scored or filled by an earlier step
        ok &= !(j < lane && o == fid);                              // a lane below holds the same id
      }
      const uint64_t m = __ballot(ok);
      if (m == 0) continue;
      const uint32_t place = have + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      const bool take = ok && place < k;                            // the room left is the cut
      if (take) {
        ids[(uint64_t)s * k + place] = fid;
        scores[(uint64_t)s * k + place] = 0.0;
      }
      const uint32_t to = take ? place : 0xffffffffu;               // ... and the lane that owns the place holds the id from here on
      for (uint32_t j = 0; j < 64; j++) {
        const uint32_t o = (uint32_t)__shfl((int)fid, (int)j);
        if ((uint32_t)__shfl((int)to, (int)j) == lane) mine = o;
      }
      const uint32_t room = k - have, found = (uint32_t)__popcll(m);
      have += found < room ? found : room;
    }
    if (lane == 0) counts[s] = have;
  }
}

// ---- the fill under quotas, and under a scope: ONE walk, rec_fill_walk<C>, and two kernels over it ---------------------------------
// k_rec_fill_grouped (smatrix_cf_recommend_grouped_fill, <false>) and k_rec_fill_scoped (smatrix_cf_recommend_scoped, <true>); C is
// the session's scope list in lanes and the scope test in front, every other line is shared.  k_rec_fill above is the same walk without
// the groups, and stays written out: as an instance of this body it was measured slower ("One walk, two instances").
// EVERY __shfl IS EXECUTED BY ALL 64 LANES, here and in k_rec_fill.  No shuffle stands on the right-hand side of && or ||, none in a
// branch that is not wave-uniform: the only branches around shuffles are the template parameter, `nl != 0` (the session's, so the
// wave's) and the __any / ballot exits.  A lane-dependent condition is applied to what the shuffle returned (`j < lane && o == fid`,
// never `j < lane && __shfl(..)`): a shuffle reads garbage from a lane that does not execute it.
// The step rule.  k_rec_fill's with the groups beside the ids: `mg` is the group of the result in `mine` (REC_GROUP_NONE in a free
// place), one gather from gr.of per scored result at the start.  A step first finishes `ok` exactly as k_rec_fill does -- so of the
// lanes that hold one id only the lowest is still ok, and a repeated id counts once --, then gathers the group of every lane still ok, g.
// The survivors.  Lane i is a SURVIVOR iff it is ungrouped or (the lanes j < have with mg_j == g) + (the ok lanes j < i with g_j == g)
// < cap: rec_group_table's argument.  An ok lane of group g below i that is no survivor found the group full, and a full group stays
// full, so lane i finds it full as well; and when every ok lane of group g below i survived, the sum IS the count of the serial walk.
// Both counts come from one more 64-step shuffle loop, over mg and g.  The survivors are numbered by mbcnt behind `have` and cut at the
// room left (the session is full behind a cut: the lanes it drops decide nothing any more), and the id AND its group go to the lane
// that owns the new place.  A step whose lanes are all refused -- 64 ids of full groups -- takes nothing and the walk goes on.
// The scope (C).  An id out of the session's scope is an excluded id.  The wave holds the session's scope list one entry per lane,
// `sl` -- hence REC_SCOPE_MAX = 64 --, REC_GROUP_NONE in the lanes beyond its end, and tests a step's 64 ids with one more 64-step
// shuffle loop: lane i's id is LISTED iff its group in sc.of is not REC_GROUP_NONE and some lane's `sl` equals it.  The test is a
// function of the id alone, like every test before the quotas, and stands first, so a step whose ids are all out of scope ends at the
// first __any.  An unscoped session (an empty list) skips it: nl is the wave's.
template <bool C>
__device__ __forceinline__ void rec_fill_walk(uint32_t n, const uint64_t* __restrict__ off, const uint32_t* __restrict__ items, uint32_t k,
                                              const uint32_t* __restrict__ fill, uint32_t n_fill, uint32_t* ids, double* scores,
                                              uint32_t* counts, uint32_t* __restrict__ n_scored, const RecFilt& f, const RecGroup& gr,
                                              const RecScope& sc) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t s = wave; s < n; s += nwaves) {                     // (wave-uniform throughout: the shuffles need every lane)
    uint32_t have = counts[s];
    if (lane == 0) n_scored[s] = have;
    if (have >= k || n_fill == 0) continue;
    const uint64_t b0 = off[s], L = off[s + 1] - b0;
    const uint64_t e0 = f.ex_off ? f.ex_off[s] : 0ull, E = f.ex_off ? f.ex_off[s + 1] - e0 : 0ull;
    uint32_t mine = lane < have ? ids[(uint64_t)s * k + lane] : 0u;
    uint32_t mg = lane < have && mine < gr.n ? gr.of[mine] : REC_GROUP_NONE, nl = 0, sl = REC_GROUP_NONE;
    if constexpr (C) {
      uint64_t l0;
      nl = rec_scope_len(sc, s, &l0);
      sl = lane < nl ? sc.gr[l0 + lane] : REC_GROUP_NONE;
    }
    for (uint32_t j0 = 0; j0 < n_fill && have < k; j0 += 64) {
      const uint32_t fid = j0 + lane < n_fill ? fill[j0 + lane] : 0u;
      bool ok = fid != 0 && !rec_denied(f, fid);
      if constexpr (C) {
        if (nl != 0) {
          const uint32_t sg = ok && fid < sc.n ? sc.of[fid] : REC_GROUP_NONE;
          bool listed = false;
          for (uint32_t j = 0; j < 64; j++) listed |= (uint32_t)__shfl((int)sl, (int)j) == sg;
          listed &= sg != REC_GROUP_NONE;                           // (an ungrouped id is listed nowhere: REC_GROUP_NONE matches nothing)
          ok &= listed == (sc.except == 0);
        }
      }
      if (!__any(ok)) continue;
      for (uint64_t c0 = 0; c0 < L; c0 += 64) {
        const uint32_t e = c0 + lane < L ? items[b0 + c0 + lane] : 0u;   // (a 0 beyond the end meets no id that is still ok)
        for (uint32_t j = 0; j < 64; j++) ok &= (uint32_t)__shfl((int)e, (int)j) != fid;
      }
      for (uint64_t c0 = 0; c0 < E; c0 += 64) {
        const uint32_t e = c0 + lane < E ? f.ex[e0 + c0 + lane] : 0u;
        for (uint32_t j = 0; j < 64; j++) ok &= (uint32_t)__shfl((int)e, (int)j) != fid;
      }
      for (uint32_t j = 0; j < 64; j++) {
        const uint32_t r = (uint32_t)__shfl((int)mine, (int)j), o = (uint32_t)__shfl((int)fid, (int)j);
        ok &= r != fid;                                             // in the result, scored or filled by an earlier step
        ok &= !(j < lane && o == fid);                              // a lane below holds the same id
      }
      if (!__any(ok)) continue;
      const uint32_t g = ok && fid < gr.n ? gr.of[fid] : REC_GROUP_NONE;   // (a lane that is not ok is in no group: it counts for nobody)
      uint32_t same = 0;
      for (uint32_t j = 0; j < 64; j++) {
        const uint32_t r = (uint32_t)__shfl((int)mg, (int)j), o = (uint32_t)__shfl((int)g, (int)j);
        same += (r == g ? 1u : 0u) + (j < lane && o == g ? 1u : 0u);
      }
      const bool sv = ok && (g == REC_GROUP_NONE || same < gr.cap);
      const uint64_t m = __ballot(sv);
      if (m == 0) continue;
      const uint32_t place = have + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      const bool take = sv && place < k;                            // the room left is the cut
      if (take) {
        ids[(uint64_t)s * k + place] = fid;
        scores[(uint64_t)s * k + place] = 0.0;
      }
      const uint32_t to = take ? place : 0xffffffffu;               // ... and the lane that owns the place holds id and group from here on
      for (uint32_t j = 0; j < 64; j++) {
        const uint32_t o = (uint32_t)__shfl((int)fid, (int)j), t = (uint32_t)__shfl((int)to, (int)j), og = (uint32_t)__shfl((int)g, (int)j);
        if (t == lane) { mg = og; mine = o; }
      }
      const uint32_t room = k - have, found = (uint32_t)__popcll(m);
      have += found < room ? found : room;
    }
    if (lane == 0) counts[s] = have;
  }
}

// smatrix_cf_recommend_grouped_fill: the walk behind the grouped ending
__global__ __launch_bounds__(256) void k_rec_fill_grouped(uint32_t n, const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                          uint32_t k, const uint32_t* __restrict__ fill, uint32_t n_fill, uint32_t* ids,
                                                          double* scores, uint32_t* counts, uint32_t* __restrict__ n_scored, RecFilt f,
                                                          RecGroup gr) {
  rec_fill_walk<false>(n, off, items, k, fill, n_fill, ids, scores, counts, n_scored, f, gr, RecScope{});
}

// ---- smatrix_cf_recommend_scoped: the lists measured, and the fill under a scope -----------------------------------------------
// beside k_rec_bound, before the driver's one read-back: a scope list longer than REC_SCOPE_MAX is RecCtl::bad, as a bad weight is
__global__ __launch_bounds__(256) void k_rec_scope_bound(uint32_t n, RecScope sc, RecCtl* ctl) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (uint64_t)gridDim.x * blockDim.x)
    if (sc.off[s + 1] - sc.off[s] > REC_SCOPE_MAX) ctl->bad = 1u;
}
// the walk under a scope; WITHOUT quotas too: under a RecGroup of no ids every ok lane survives, and it writes k_rec_fill's bytes
__global__ __launch_bounds__(256) void k_rec_fill_scoped(uint32_t n, const uint64_t* __restrict__ off, const uint32_t* __restrict__ items,
                                                         uint32_t k, const uint32_t* __restrict__ fill, uint32_t n_fill, uint32_t* ids,
                                                         double* scores, uint32_t* counts, uint32_t* __restrict__ n_scored, RecFilt f,
                                                         RecGroup gr, RecScope sc) {
  rec_fill_walk<true>(n, off, items, k, fill, n_fill, ids, scores, counts, n_scored, f, gr, sc);
}
