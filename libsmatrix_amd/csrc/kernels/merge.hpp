// kernels/merge.hpp -- record emission for smatrix_merge / smatrix_import_csr (include/smatrix_batch.h): row tables, or a CSR,
// straight into a bounded batch of packed {x, key, value} records -- the form the write path takes with in_stride == 3
// (smatrix_apply_packed_dev).  No whole-matrix CSR and no triples of nnz words in between.
// A fragment of smx_kernels.hpp: included there, after export.hpp and rank_key.hpp, INSIDE namespace smx; not a header of its own.
//
// From row tables (one internal batch = the rows [r0, r1) of the export's row list, `items`, whose exact pair counts were scanned
// into ptr[] by k_ex_count / k_ex_scan_*): the record of a row's j-th non-empty cell, in slot order, is number
// ptr[r] - ptr[r0] + j of the batch.
//   k_mg_emit          a wave per row of up to GETROW_WAVE_MAX cells, 128 cells (1 KiB) per step with 16-byte loads, the
//                      non-empty ones compacted with ballots + prefix popcounts; a longer row is only noted down in `big`, one
//                      entry {row, segment} per segment of GETROW_SEG cells (big[0] = entries)
//   k_mg_emit_big<C>   the noted segments, a 1024-lane workgroup each (as k_getrow_big; a workgroup touches its own entries only):
//                      <true> counts a cut row's segments, <false> writes every segment's records behind those of the segments
//                      before it
// Each source cell is read once (twice in a row of >= 2 segments) and 12 bytes leave per pair.
//
// smatrix_merge_scaled runs the same row walkers with a TRANSFORM between the cell and the record: the bodies below are
// templated on a functor  bool f(key, value&)  that rewrites the value of a non-empty cell and says whether the pair survives.
// MgIdent (smatrix_merge: every pair as it is) folds away; MgScale is v' = floor(v * num / den) with the two drop rules.
//   k_mgx_count        the SURVIVORS of every row of the row list -> cnt[] (what k_ex_count is to the export), a wave per row up to
//                      GETROW_WAVE_MAX cells; longer rows get cnt 0 and one {row, segment} entry per segment in `big`
//   k_mgx_count_big    those segments, a 1024-lane workgroup each: adds the segment's survivors to cnt[row] and, in a cut row,
//                      leaves them in seg_cnt[] -- for the whole matrix at once, so the emission has no counting pass of its own
//   k_mgx_emit, k_mgx_emit_big   k_mg_emit / k_mg_emit_big<false> with the transform
// Both count kernels also sum the non-empty cells they saw into *tot: dropped = *tot - survivors.  A source cell is read twice
// in all: once counted, once emitted.
//
// A cut row's segment counts live in seg_cnt[] at (byte offset of the segment in the arena) >> 18: a segment is 256 KiB of
// cells and rows do not overlap, so no two segments of any two rows share an index, and the array is arena / 65536 bytes -- no
// plan pass that numbers the segments.

constexpr uint32_t MG_SEG_SHIFT = 18;                       // log2(GETROW_SEG cells * 8 bytes)
static_assert((1u << MG_SEG_SHIFT) == GETROW_SEG * 8, "a segment of the merge is a segment of getrow");

__device__ __forceinline__ void mg_put(uint32_t* __restrict__ rec, uint64_t at, uint32_t x, uint32_t key, uint32_t val) {
  uint32_t* p = rec + 3 * at;
  p[0] = x; p[1] = key; p[2] = val;
}

__device__ __forceinline__ uint32_t mg_wave_or(uint32_t v) {
  for (uint32_t d = 32; d; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d);
  return v;
}
__device__ __forceinline__ uint32_t mg_wave_sum(uint32_t v) {
  for (uint32_t d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}

// the cells [p_begin, p_end) of segment g of a row of nseg segments (an uncut row of any size is its one segment)
__device__ __forceinline__ void mg_seg_range(uint32_t size, uint32_t nseg, uint32_t g, uint32_t& p_begin, uint32_t& p_end) {
  p_begin = nseg == 1 ? 0u : g * GETROW_SEG;
  p_end = nseg == 1 ? size : p_begin + GETROW_SEG;
}

// (the walkers ask the functor for the predicate of row r of the row list, f.at(r): these two are the same for every row)
struct MgIdent {
  __device__ __forceinline__ bool operator()(uint32_t, uint32_t&) const { return true; }
  __device__ __forceinline__ const MgIdent& at(uint32_t) const { return *this; }
};

// floor(v * num / den) for 1 <= num <= den, exactly, without a 64-bit division.  n = v * num < 2^64 and the quotient is <= v.
// The estimate: n as a double (hi * 2^32 + lo: both parts exact, the fma rounds once), times the rounded 1 / den, rounded again
// -- three roundings of 2^-53 relative each on a quotient below 2^32, so it is off by less than 2^-19 from n / den and its
// integer part is the quotient, or one beside it.  The remainder (64-bit, wrapping; it lies in [-den, 2 * den)) says which.
__host__ __device__ __forceinline__ uint32_t mg_scale_value(uint32_t v, uint32_t num, uint32_t den, double rden) {
  const uint64_t n = (uint64_t)v * num;
  const double d = fma((double)(uint32_t)(n >> 32), 4294967296.0, (double)(uint32_t)n);
  uint32_t q = (uint32_t)fmin(d * rden, 4294967295.0);
  const int64_t r = (int64_t)(n - (uint64_t)q * den);
  if (r < 0) q--;
  else if (r >= (int64_t)den) q++;
  return q;
}

// smatrix_merge_scaled's transform and filter: the pair survives unless v' < min_value or it would be the empty slot (0, 0)
struct MgScale {
  uint32_t num, den, min_value;
  double rden;                                             // 1.0 / den
  __device__ __forceinline__ bool operator()(uint32_t key, uint32_t& val) const {
    if (num != den) val = mg_scale_value(val, num, den, rden);
    return val >= min_value && (key | val) != 0;
  }
  __device__ __forceinline__ const MgScale& at(uint32_t) const { return *this; }
};

template <typename F>
__device__ __forceinline__ void mg_emit_rows(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                             const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t r1,
                                             uint32_t* __restrict__ rec, uint32_t* big, const uint32_t wave, const uint32_t nwaves,
                                             const F fn) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t lt = (1ull << lane) - 1;
  const uint64_t base = ptr[r0];
  for (uint32_t r = r0 + wave; r < r1; r += nwaves) {
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    if (s.z == 0) continue;                                            // no block yet (quirk Q3): no pairs
    const uint32_t size = 1u << meta_lg(s.x);
    if (size > GETROW_WAVE_MAX) {                                      // one entry {row, segment} per segment, in any order
      const uint32_t nseg = getrow_nseg(size);
      uint32_t e0 = 0;
      if (lane == 0) e0 = atomicAdd(&big[0], nseg);
      e0 = (uint32_t)__shfl((int)e0, 0);
      for (uint32_t g = lane; g < nseg; g += 64) { big[1 + 2 * (e0 + g)] = r; big[2 + 2 * (e0 + g)] = g; }
      continue;
    }
    const uint4* cells = reinterpret_cast<const uint4*>(row_cells(arena, s.z));
    const uint32_t x = s.y;
    const auto f = fn.at(r);
    uint64_t at = ptr[r] - base;
    auto fetch = [&](uint32_t p0) -> uint4 {
      const uint32_t p = p0 + 2 * lane;
      return p < size ? cells[p >> 1] : make_uint4(0, 0, 0, 0);
    };
    auto step = [&](const uint4 c) {                                   // compacts the 128 cells held in c (slot order)
      uint32_t v0 = c.y, v1 = c.w;
      const bool ne0 = (c.x | c.y) != 0 && f(c.x, v0), ne1 = (c.z | c.w) != 0 && f(c.z, v1);
      const uint64_t m0 = __ballot(ne0), m1 = __ballot(ne1);
      uint64_t o = at + (uint32_t)__popcll(m0 & lt) + (uint32_t)__popcll(m1 & lt);
      if (ne0) mg_put(rec, o, x, c.x, v0);
      o += ne0;
      if (ne1) mg_put(rec, o, x, c.z, v1);
      at += (uint32_t)__popcll(m0) + (uint32_t)__popcll(m1);
    };
    // every load of a row of up to 512 cells (the CF shape and four times that) is in flight before the first is consumed
    const uint4 a0 = fetch(0), a1 = fetch(128), a2 = fetch(256), a3 = fetch(384);
    step(a0);
    if (size > 128) step(a1);
    if (size > 256) { step(a2); step(a3); }
    for (uint32_t p0 = 512; p0 < size; p0 += 512) {                    // (sizes are powers of two: 1024 and up here)
      const uint4 b0 = fetch(p0), b1 = fetch(p0 + 128), b2 = fetch(p0 + 256), b3 = fetch(p0 + 384);
      step(b0); step(b1); step(b2); step(b3);
    }
  }
}

__global__ __launch_bounds__(256) void k_mg_emit(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                 const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t r1,
                                                 uint32_t* __restrict__ rec, uint32_t* big) {
  // (the wave's number and the number of waves are taken here: blockDim is a constant of the launch to a kernel only)
  mg_emit_rows(dir, arena, items, ptr, r0, r1, rec, big, (blockIdx.x * blockDim.x + threadIdx.x) >> 6, (gridDim.x * blockDim.x) >> 6, MgIdent());
}

__global__ __launch_bounds__(256) void k_mgx_emit(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                  const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t r1,
                                                  uint32_t* __restrict__ rec, uint32_t* big, const MgScale f) {
  mg_emit_rows(dir, arena, items, ptr, r0, r1, rec, big, (blockIdx.x * blockDim.x + threadIdx.x) >> 6, (gridDim.x * blockDim.x) >> 6, f);
}

template <bool COUNT, typename F>
__device__ __forceinline__ void mg_emit_segs(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                             const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t* __restrict__ rec,
                                             const uint32_t* big, uint32_t* seg_cnt, const F fn) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t s_written;
  const uint32_t nent = big[0];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1;
  const uint64_t base = ptr[r0];
  auto block_sum = [&](uint32_t v) -> uint32_t {          // sum over the workgroup, to every lane
    v = mg_wave_sum(v);
    __syncthreads();
    if (lane == 0) wsum[w] = v;
    __syncthreads();
    uint32_t t = 0;
    for (uint32_t i = 0; i < 16; i++) t += wsum[i];
    __syncthreads();
    return t;
  };
  for (uint32_t t = blockIdx.x; t < nent; t += gridDim.x) {
    const uint32_t r = big[1 + 2 * t], g = big[2 + 2 * t];
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    const uint32_t size = 1u << meta_lg(s.x);                          // > GETROW_WAVE_MAX: a multiple of 2048
    const uint32_t nseg = getrow_nseg(size);
    if (COUNT && nseg == 1) continue;
    const uint8_t* cell_bytes = reinterpret_cast<const uint8_t*>(row_cells(arena, s.z));
    const uint4* cells = reinterpret_cast<const uint4*>(cell_bytes);
    const uint64_t first = (uint64_t)(cell_bytes - arena) >> MG_SEG_SHIFT;   // the row's first entry of seg_cnt
    const auto f = fn.at(r);
    {
      uint32_t p_begin, p_end;
      mg_seg_range(size, nseg, g, p_begin, p_end);
      if (COUNT) {
        uint32_t c = 0;
        for (uint32_t p0 = p_begin; p0 < p_end; p0 += 2048) {
          const uint4 q = cells[(p0 >> 1) + threadIdx.x];
          uint32_t v0 = q.y, v1 = q.w;
          c += ((q.x | q.y) != 0 && f(q.x, v0)) + ((q.z | q.w) != 0 && f(q.z, v1));
        }
        c = block_sum(c);
        if (threadIdx.x == 0) seg_cnt[first + g] = c;
        continue;
      }
      uint32_t before_me = 0;
      if (nseg > 1) {
        uint32_t mine = 0;
        for (uint32_t i = threadIdx.x; i < g; i += 1024) mine += seg_cnt[first + i];
        before_me = block_sum(mine);
      }
      if (threadIdx.x == 0) s_written = before_me;
      __syncthreads();
      const uint64_t off = ptr[r] - base;
      for (uint32_t p0 = p_begin; p0 < p_end; p0 += 2048) {
        const uint32_t written = s_written;
        const uint4 c = cells[(p0 >> 1) + threadIdx.x];
        uint32_t v0 = c.y, v1 = c.w;
        const bool ne0 = (c.x | c.y) != 0 && f(c.x, v0), ne1 = (c.z | c.w) != 0 && f(c.z, v1);
        const uint64_t m0 = __ballot(ne0), m1 = __ballot(ne1);
        if (lane == 0) wsum[w] = (uint32_t)__popcll(m0) + (uint32_t)__popcll(m1);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t i = 0; i < 16; i++) { const uint32_t v = wsum[i]; if (i < w) before += v; total += v; }
        uint64_t o = off + written + before + (uint32_t)__popcll(m0 & lt) + (uint32_t)__popcll(m1 & lt);
        if (ne0) mg_put(rec, o, s.y, c.x, v0);
        o += ne0;
        if (ne1) mg_put(rec, o, s.y, c.z, v1);
        __syncthreads();
        if (threadIdx.x == 0) s_written = written + total;
        __syncthreads();
      }
    }
  }
}

template <bool COUNT>
__global__ __launch_bounds__(1024) void k_mg_emit_big(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                      const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t* __restrict__ rec,
                                                      const uint32_t* big, uint32_t* seg_cnt) {
  mg_emit_segs<COUNT>(dir, arena, items, ptr, r0, rec, big, seg_cnt, MgIdent());
}

// (the cut rows' seg_cnt entries are k_mgx_count_big's, of this very transform)
__global__ __launch_bounds__(1024) void k_mgx_emit_big(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                       const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t* __restrict__ rec,
                                                       const uint32_t* big, uint32_t* seg_cnt, const MgScale f) {
  mg_emit_segs<false>(dir, arena, items, ptr, r0, rec, big, seg_cnt, f);
}

// ---- the filtered counts of smatrix_merge_scaled ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mgx_count(const DirSlot* __restrict__ dir, uint8_t* arena, uint32_t n,
                                                   const uint64_t* __restrict__ items, uint32_t* __restrict__ cnt, uint32_t* big,
                                                   unsigned long long* tot, const MgScale f) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  uint32_t seen = 0;                                                   // this lane's non-empty cells, over all the wave's rows
  for (uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n; r += nwaves) {
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    const uint32_t size = s.z ? 1u << meta_lg(s.x) : 0u;
    if (size > GETROW_WAVE_MAX) {                                      // as k_mg_emit: one entry {row, segment} per segment
      const uint32_t nseg = getrow_nseg(size);
      uint32_t e0 = 0;
      if (lane == 0) { cnt[r] = 0; e0 = atomicAdd(&big[0], nseg); }
      e0 = (uint32_t)__shfl((int)e0, 0);
      for (uint32_t g = lane; g < nseg; g += 64) { big[1 + 2 * (e0 + g)] = r; big[2 + 2 * (e0 + g)] = g; }
      continue;
    }
    const uint4* cells = s.z ? reinterpret_cast<const uint4*>(row_cells(arena, s.z)) : nullptr;
    uint32_t c = 0;
    for (uint32_t p = 2 * lane; p < size; p += 128) {
      uint4 q = cells[p >> 1];
      const bool ne0 = (q.x | q.y) != 0, ne1 = (q.z | q.w) != 0;
      seen += ne0 + ne1;
      c += (ne0 && f(q.x, q.y)) + (ne1 && f(q.z, q.w));
    }
    for (uint32_t d = 32; d; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d);
    if (lane == 0) cnt[r] = c;
  }
  seen = mg_wave_sum(seen);                                            // (a wave's rows hold < 2^32 cells: rows * 8192 / waves)
  if (lane == 0 && seen) atomicAdd(tot, (unsigned long long)seen);
}

__global__ __launch_bounds__(1024) void k_mgx_count_big(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                        uint32_t* cnt, const uint32_t* big, uint32_t* seg_cnt, unsigned long long* tot,
                                                        const MgScale f) {
  __shared__ uint32_t wsum[2][16];
  const uint32_t nent = big[0];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t t = blockIdx.x; t < nent; t += gridDim.x) {
    const uint32_t r = big[1 + 2 * t], g = big[2 + 2 * t];
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    const uint32_t size = 1u << meta_lg(s.x);                          // > GETROW_WAVE_MAX: a multiple of 2048
    const uint32_t nseg = getrow_nseg(size);
    const uint8_t* cell_bytes = reinterpret_cast<const uint8_t*>(row_cells(arena, s.z));
    const uint4* cells = reinterpret_cast<const uint4*>(cell_bytes);
    uint32_t p_begin, p_end;
    mg_seg_range(size, nseg, g, p_begin, p_end);
    uint32_t c = 0, seen = 0;
    for (uint32_t p0 = p_begin; p0 < p_end; p0 += 2048) {
      uint4 q = cells[(p0 >> 1) + threadIdx.x];
      const bool ne0 = (q.x | q.y) != 0, ne1 = (q.z | q.w) != 0;
      seen += ne0 + ne1;
      c += (ne0 && f(q.x, q.y)) + (ne1 && f(q.z, q.w));
    }
    // (spelled out here and in k_mgx_count's loop: through mg_wave_sum these two kernels come out scheduled differently)
    for (uint32_t d = 32; d; d >>= 1) { c += (uint32_t)__shfl_xor((int)c, d); seen += (uint32_t)__shfl_xor((int)seen, d); }
    if (lane == 0) { wsum[0][w] = c; wsum[1][w] = seen; }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tc = 0, ts = 0;
      for (uint32_t i = 0; i < 16; i++) { tc += wsum[0][i]; ts += wsum[1][i]; }
      // (an uncut row's table may share its 256 KiB with another row's: only cut rows own their seg_cnt entries)
      if (nseg > 1) seg_cnt[((uint64_t)(cell_bytes - arena) >> MG_SEG_SHIFT) + g] = tc;
      if (tc) atomicAdd(&cnt[r], tc);
      if (ts) atomicAdd(tot, (unsigned long long)ts);
    }
    __syncthreads();
  }
}

// ---- smatrix_merge_topk / smatrix_merge_topk_by: the m best pairs of every row ------------------------------------------------------
// thr[r] = the rank key of the m-th best ELIGIBLE pair of row r (y != 0, v >= min_value), or zero when the row has at most m of
// them; cnt[r] = the pairs the row keeps: min(m, eligible) + its head pair (y == 0) when v >= min_value.  What a key is, is a
// policy (kernels/rank_key.hpp for the bits, below for what a key is made from):
//   MgtValueKey    {v, ~y}.  Free to make: the counting pass ORs the keys as it goes.
//   MgtSimKey      MgtCosineKey with the score of kernels/sim.hpp (smatrix_merge_topk_sim: Jaccard, lift, shrinkage); all that is
//                  said of the cosine key below holds for it.
//   MgtCosineKey   {the score's bits, ~y}.  The score of the pair (y, v) of row x is k_cf_neighbors' (kernels/rows.hpp), expression
//                  for expression, in IEEE double:
//                    tb = get(y, 0), 0 counted as 1;  den = sqrt(get(x, 0)) * sqrt(tb);  score = den != 0 && !(v > den) ? v / den : 0
//                  A row without a head pair scores 0 everywhere and keeps its m lowest eligible columns; a dead cell scores 0.
//                  The score is never stored per pair: every pass that needs it makes it again, each lane with its own
//                  neighbour's get(y, 0) (apply_one<OP_GET>, as k_cf_neighbors: many independent look-ups in flight per wave).
//                  So the counting pass makes no key, the row's own total is read only in a row that has more than m eligible
//                  pairs, a pass of its own ORs the keys of such a row, and a row of at most 128 cells (a lane holds two) keeps
//                  its two keys in registers: ONE gather per pair for the whole selection.
// The selection of one row is an MSB radix select, 8 bits per pass, the 256 bins in LDS:
//   the count   one read counts the eligible pairs: a row of at most m is done
//   the start   from the OR of the keys (rank_key.hpp): the first digit worth a pass, the digits above it as the prefix
//   a pass      re-reads the row (a wave-path row is at most 64 KiB and stays in L2) and counts, by their next digit, the keys
//               that agree with the digits chosen so far; the bins are walked from 255 down to the one that holds the key wanted
//   the end     the last digit, or earlier when that bin holds ONE key: one more read of the row fetches it
//   k_mgt_select, k_mgc_select          mgt_select_row<P>, written once over the key policy: a wave per row of up to
//                      GETROW_WAVE_MAX cells, a histogram per wave, fenced for the wave alone: no workgroup barrier.  Longer
//                      rows are noted in `big` (big[0] = entries, one row index each).
//   k_mgt_select_big, k_mgc_select_big  those rows, ONE 1024-lane workgroup per row over all its segments -- they are few, and a
//                      histogram across workgroups is not worth its launches.  These two are still written out per key, with the
//                      key arithmetic beside them (mgt_key, mgc_*): one body over the key policy, with or without a scope policy
//                      under mgt_select_row, measured 4 to 9 % slower in k_mgt_select_big, the longest kernel of the value
//                      selection, for a reason that was not found (profiles/merge_select_fold_time.txt).  What decides a branch
//                      or a barrier in them comes out of LDS through readfirstlane: the same scalar in all 16 waves.
// Both sum the non-empty cells they saw into *tot, as the k_mgx_count kernels do.  The emission is the walkers above with
// MgRank<P>: the pair's key is made once more and compared with the row's threshold; zero = every eligible pair, and then
// nothing is gathered.  A cut row's seg_cnt entries are counted with the finished threshold by k_*_emit_big<true>, batch by
// batch, as smatrix_merge does.
// Gathers per eligible pair of a row that the cosine rank cuts to m: 1 (the start) + the passes + 1 (a bin of one key) + 1
// (emission; 2 in a row of two segments and more), or 1 + 1 in a row of at most 128 cells.
__device__ __forceinline__ void mgt_wave_sync() {          // the LDS traffic of one wave, in program order for all its lanes
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// one wave-wide step of a pass: hist[digit]++ for every lane with `match`.  Ties are the rule (equal values share the value
// bytes), so the lanes that share the first matching lane's digit go in as one add.
__device__ __forceinline__ void mgt_hist_add(uint32_t* hist, bool match, uint32_t digit, uint32_t lane) {
  const uint64_t mm = __ballot(match);
  if (mm == 0) return;
  const uint32_t first = (uint32_t)__ffsll((unsigned long long)mm) - 1;
  const uint32_t d0 = (uint32_t)__shfl((int)digit, (int)first);
  const uint64_t same = __ballot(match && digit == d0);
  if (lane == first) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
  if (match && digit != d0) atomicAdd(&hist[digit], 1u);
}

// one wave: the bin d that holds the need-th key counted from bin 255 down (1 <= need <= the sum of the bins), the keys in the
// bins above d, and the keys in d -- to every lane.  Lane l holds bins 4 l .. 4 l + 3.
// SERIAL: the bins of the lanes above come from 63 broadcast reads of LDS instead of a scan with shuffles -- the 1024-lane kernel
// picks once per pass over a row of 128 KiB and more, and the scan's six lane tests, hoisted, are six SGPR pairs it has not got.
template <bool SERIAL>
__device__ __forceinline__ void mgt_pick(const uint32_t* hist, uint32_t need, uint32_t lane, uint32_t& d, uint32_t& above, uint32_t& bucket) {
  const uint4 b = *reinterpret_cast<const uint4*>(hist + 4 * lane);
  const uint32_t s = b.x + b.y + b.z + b.w;
  uint32_t S = s;                                          // the bins of this lane and of the lanes above it
  if (SERIAL) {
#pragma unroll 1
    for (uint32_t j = 1; j < 64; j++) {
      const uint4 o = *reinterpret_cast<const uint4*>(hist + 4 * j);
      if (j > lane) S += o.x + o.y + o.z + o.w;
    }
  } else {
    for (uint32_t k = 1; k < 64; k <<= 1) { const uint32_t t = (uint32_t)__shfl_down((int)S, k); if (lane + k < 64) S += t; }
  }
  uint32_t a = S - s, dd = 3, bk = b.w;
  const bool hit = a < need && need <= S;
  if (need > a + b.w) {
    a += b.w; dd = 2; bk = b.z;
    if (need > a + b.z) {
      a += b.z; dd = 1; bk = b.y;
      if (need > a + b.y) { a += b.y; dd = 0; bk = b.x; }
    }
  }
  const uint64_t hm = __ballot(hit);
  const int src = hm ? __ffsll((unsigned long long)hm) - 1 : 0;
  d = (uint32_t)__shfl((int)(4 * lane + dd), src);
  above = (uint32_t)__shfl((int)a, src);
  bucket = (uint32_t)__shfl((int)bk, src);
}

__device__ __forceinline__ uint64_t mgc_score_bits(DirSlot* dir, uint32_t dmask, uint8_t* arena, double sa, uint32_t y, uint32_t v) {
  bool dummy = false;
  uint32_t b_total = apply_one<OP_GET>(dir, dmask, arena, y, 0u, 0u, &dummy);
  if (b_total == 0) b_total = 1;
  const double num = (double)v;
  const double den = sa * sqrt((double)b_total);
  double score = 0.0;
  if (den != 0.0 && !(num > den)) score = num / den;
  return (uint64_t)__double_as_longlong(score);
}

// The key policies.  Beside the bits: FREE, a key costs no memory access; HOLD, a row that one step of a wave covers keeps its
// keys in registers; Thr, the per-row thresholds in device memory; Src, what keys are made from, and Row, that for one row --
// Src::row(x) for row id x, Src::at(r) for row r of the row list, Src::blank() before either: it makes no key yet.
struct MgtValueKey : RkValue {
  static constexpr bool FREE = true, HOLD = false;
  struct Thr {
    uint64_t* thr;
    __device__ __forceinline__ Key load(uint32_t r) const { return thr[r]; }
    __device__ __forceinline__ void store(uint32_t r, Key k) const { thr[r] = k; }
  };
  struct Row { __device__ __forceinline__ Key key(uint32_t y, uint32_t v) const { return make(y, v); } };
  struct Src {
    __device__ __forceinline__ Row blank() const { return Row{}; }
    __device__ __forceinline__ Row row(uint32_t) const { return Row{}; }
    __device__ __forceinline__ Row at(uint32_t) const { return Row{}; }
  };
};

struct MgtCosineKey : RkCosine {
  static constexpr bool FREE = false, HOLD = true;
  struct Thr {
    uint64_t* thr;                                         // the score half,
    uint32_t* thr_col;                                     // the column half
    __device__ __forceinline__ Key load(uint32_t r) const { return Key{thr[r], thr_col[r]}; }
    __device__ __forceinline__ void store(uint32_t r, Key k) const { thr[r] = k.s; thr_col[r] = k.c; }
  };
  struct Row {
    DirSlot* dir;
    uint8_t* arena;
    uint32_t dmask;
    double sa;                                             // sqrt of the row's own total
    __device__ __forceinline__ Key key(uint32_t y, uint32_t v) const { return make(y, mgc_score_bits(dir, dmask, arena, sa, y, v)); }
  };
  struct Src {
    DirSlot* dir;
    uint8_t* arena;
    const uint64_t* items;                                 // the row list (the row's directory slot in the high word)
    uint32_t dmask;
    __device__ __forceinline__ Row blank() const { return Row{dir, arena, dmask, 0.0}; }
    __device__ __forceinline__ Row row(uint32_t x) const {
      bool dummy = false;
      return Row{dir, arena, dmask, sqrt((double)apply_one<OP_GET>(dir, dmask, arena, x, 0u, 0u, &dummy))};
    }
    __device__ __forceinline__ Row at(uint32_t r) const { return row(dir[(uint32_t)(items[r] >> 32)].x); }
  };
};

// smatrix_merge_topk_sim: MgtCosineKey's key with the score of kernels/sim.hpp -- the measure and its shrinkage travel with the
// row's own double (sim_row: sqrt of the total for COSINE, the total otherwise)
struct MgtSimKey : RkCosine {
  static constexpr bool FREE = false, HOLD = true;
  typedef MgtCosineKey::Thr Thr;
  struct Row {
    DirSlot* dir;
    uint8_t* arena;
    uint32_t dmask;
    double ra;                                             // sim_row of the row's own total
    SimArgs m;
    __device__ __forceinline__ Key key(uint32_t y, uint32_t v) const {
      bool dummy = false;
      const double cb = sim_col(m.sim, apply_one<OP_GET>(dir, dmask, arena, y, 0u, 0u, &dummy));
      return make(y, (uint64_t)__double_as_longlong(sim_score(m, v, ra, cb)));
    }
  };
  struct Src {
    DirSlot* dir;
    uint8_t* arena;
    const uint64_t* items;
    uint32_t dmask;
    SimArgs m;
    __device__ __forceinline__ Row blank() const { return Row{dir, arena, dmask, 0.0, m}; }
    __device__ __forceinline__ Row row(uint32_t x) const {
      bool dummy = false;
      return Row{dir, arena, dmask, sim_row(m.sim, apply_one<OP_GET>(dir, dmask, arena, x, 0u, 0u, &dummy)), m};
    }
    __device__ __forceinline__ Row at(uint32_t r) const { return row(dir[(uint32_t)(items[r] >> 32)].x); }
  };
};

// the emission's filter: the pairs of row r whose rank key is at least the row's threshold, and the head pair
template <typename P>
struct MgRankRow {
  typename P::Key thr;
  typename P::Row row;
  uint32_t min_value;
  __device__ __forceinline__ bool operator()(uint32_t key, uint32_t& val) const {
    if (val < min_value) return false;
    if (key == 0) return val != 0;
    if (!P::FREE && P::is_zero(thr)) return true;
    return P::ge(row.key(key, val), thr);
  }
};
template <typename P>
struct MgRank {
  typename P::Thr thr;                                     // per row of the row list; zero = every eligible pair
  typename P::Src src;
  uint32_t min_value;
  __device__ __forceinline__ MgRankRow<P> at(uint32_t r) const {
    MgRankRow<P> f{thr.load(r), src.blank(), min_value};
    if (P::FREE || !P::is_zero(f.thr)) f.row = src.at(r);   // (a row that keeps all its eligible pairs scores nothing)
    return f;
  }
};
using MgTopk = MgRank<MgtValueKey>;
using MgCos = MgRank<MgtCosineKey>;
using MgSim = MgRank<MgtSimKey>;

__device__ __forceinline__ bool mgt_eligible(uint32_t key, uint32_t val, uint32_t min_value) { return key != 0 && val >= min_value; }

template <typename K>
struct MgtPair {                                           // the two cells a lane holds at one step, as rank keys
  K k0, k1;
  bool e0, e1;                                             // eligible
};
template <typename P>
__device__ __forceinline__ MgtPair<typename P::Key> mgt_keys(const typename P::Row& row, uint32_t min_value, const uint4 q) {
  MgtPair<typename P::Key> k{P::zero(), P::zero(), mgt_eligible(q.x, q.y, min_value), mgt_eligible(q.z, q.w, min_value)};
  if (P::FREE || k.e0) k.k0 = row.key(q.x, q.y);
  if (P::FREE || k.e1) k.k1 = row.key(q.z, q.w);
  return k;
}

// A wave as "every lane" of a row's selection.  fetch: this lane's two cells of the 128 at p0 (every lane takes every step: the
// steps hold ballots); or_words: over every lane, to every lane; hist_zero, pick: around a pass -- the bins emptied before
// it, mgt_pick after it, the wave's LDS traffic fenced for the wave alone.
struct MgtWave {
  static constexpr uint32_t STEP = 128;
  uint32_t* hist;                                          // this wave's 256 bins
  uint32_t lane;
  __device__ __forceinline__ uint4 fetch(const uint4* cells, uint32_t size, uint32_t p0) const {
    const uint32_t p = p0 + 2 * lane;
    return p < size ? cells[p >> 1] : make_uint4(0, 0, 0, 0);
  }
  template <uint32_t N>
  __device__ __forceinline__ void or_words(uint32_t (&w)[N]) const {
#pragma unroll
    for (uint32_t i = 0; i < N; i++) w[i] = mg_wave_or(w[i]);
  }
  __device__ __forceinline__ void hist_zero() const {
    for (uint32_t i = lane; i < 256; i += 64) hist[i] = 0;
    mgt_wave_sync();
  }
  __device__ __forceinline__ void pick(uint32_t need, uint32_t& d, uint32_t& above, uint32_t& bucket) const {
    mgt_wave_sync();
    mgt_pick<false>(hist, need, lane, d, above, bucket);
    mgt_wave_sync();
  }
};

// The selection of one row of up to GETROW_WAVE_MAX cells by a wave: -> the row's threshold, to every lane; elig and head as
// cnt[] wants them; this lane's non-empty cells added to seen.
template <typename P>
__device__ __forceinline__ typename P::Key mgt_select_row(const MgtWave& sc, const typename P::Src& src, const uint4* cells, uint32_t size,
                                                          uint32_t x, uint32_t m, uint32_t min_value, uint32_t& seen, uint32_t& elig,
                                                          uint32_t& head) {
  using S = MgtWave;
  constexpr bool HOLD = P::HOLD;                           // (a row of one step keeps its keys in registers)
  typename P::Row row = src.blank();
  if (P::FREE) row = src.row(x);
  typename P::Acc a = P::acc0();
  uint4 q0 = make_uint4(0, 0, 0, 0);                       // the lane's first two cells: all of a row of one step
  elig = 0; head = 0;
  for (uint32_t p0 = 0; p0 < size; p0 += S::STEP) {
    const uint4 q = sc.fetch(cells, size, p0);
    if (HOLD && p0 == 0) q0 = q;
    seen += ((q.x | q.y) != 0) + ((q.z | q.w) != 0);
    head |= (q.x == 0 && q.y != 0 && q.y >= min_value) | (q.z == 0 && q.w != 0 && q.w >= min_value);
    if (P::FREE) {
      const MgtPair<typename P::Key> k = mgt_keys<P>(row, min_value, q);
      if (k.e0) { elig++; P::acc_add(a, k.k0); }
      if (k.e1) { elig++; P::acc_add(a, k.k1); }
    } else {
      elig += mgt_eligible(q.x, q.y, min_value) + mgt_eligible(q.z, q.w, min_value);
    }
  }
  elig = mg_wave_sum(elig);
  head = mg_wave_or(head);
  if (elig <= m) return P::zero();
  if (!P::FREE) row = src.row(x);
  const bool held = HOLD && size <= S::STEP;
  MgtPair<typename P::Key> k_held{P::zero(), P::zero(), false, false};
  if (held) k_held = mgt_keys<P>(row, min_value, q0);
  auto keys = [&](uint32_t p0) -> MgtPair<typename P::Key> { return held ? k_held : mgt_keys<P>(row, min_value, sc.fetch(cells, size, p0)); };
  if (!P::FREE)
    for (uint32_t p0 = 0; p0 < size; p0 += S::STEP) {
      const MgtPair<typename P::Key> k = keys(p0);
      if (k.e0) P::acc_add(a, k.k0);
      if (k.e1) P::acc_add(a, k.k1);
    }
  sc.or_words(a.w);
  typename P::Key prefix;
  uint32_t dg = P::start(a, prefix), need = m;
  for (;;) {
    sc.hist_zero();
    for (uint32_t p0 = 0; p0 < size; p0 += S::STEP) {
      const MgtPair<typename P::Key> k = keys(p0);
      mgt_hist_add(sc.hist, k.e0 && P::agrees_above(k.k0, prefix, dg), P::digit(k.k0, dg), sc.lane);
      mgt_hist_add(sc.hist, k.e1 && P::agrees_above(k.k1, prefix, dg), P::digit(k.k1, dg), sc.lane);
    }
    uint32_t d, above, bucket;
    sc.pick(need, d, above, bucket);
    need -= above;
    P::take_digit(prefix, dg, d);
    if (dg == 0) return prefix;
    if (bucket == 1) {                                     // the one key that agrees down to this digit
      uint32_t w[P::W] = {};
      for (uint32_t p0 = 0; p0 < size; p0 += S::STEP) {
        const MgtPair<typename P::Key> k = keys(p0);
        if (k.e0 && P::agrees_down(k.k0, prefix, dg)) P::or_words(w, k.k0);
        if (k.e1 && P::agrees_down(k.k1, prefix, dg)) P::or_words(w, k.k1);
      }
      sc.or_words(w);
      return P::from_words(w);
    }
    dg--;
  }
}

// the rows of the row list, a wave each (the wave's number and the number of waves come from the kernel, as in mg_emit_rows)
template <typename P>
__device__ __forceinline__ void mgt_select_rows(const DirSlot* dir, uint8_t* arena, uint32_t n, const uint64_t* __restrict__ items,
                                                uint32_t m, uint32_t min_value, const typename P::Src src, const typename P::Thr thr,
                                                uint32_t* __restrict__ cnt, uint32_t* big, unsigned long long* tot, const uint32_t wave,
                                                const uint32_t nwaves) {
  __shared__ __attribute__((aligned(16))) uint32_t s_hist[4][256];
  const MgtWave sc{s_hist[threadIdx.x >> 6], threadIdx.x & 63};
  uint32_t seen = 0;
  for (uint32_t r = wave; r < n; r += nwaves) {
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    const uint32_t size = s.z ? 1u << meta_lg(s.x) : 0u;
    if (size > GETROW_WAVE_MAX) {
      if (sc.lane == 0) big[1 + atomicAdd(&big[0], 1u)] = r;
      continue;
    }
    const uint4* cells = s.z ? reinterpret_cast<const uint4*>(row_cells(arena, s.z)) : nullptr;
    uint32_t elig, head;
    const typename P::Key t = mgt_select_row<P>(sc, src, cells, size, s.y, m, min_value, seen, elig, head);
    if (sc.lane == 0) { thr.store(r, t); cnt[r] = (elig < m ? elig : m) + head; }
  }
  seen = mg_wave_sum(seen);                                // (a wave's rows hold < 2^32 cells: rows * 8192 / waves)
  if (sc.lane == 0 && seen) atomicAdd(tot, (unsigned long long)seen);
}

// ---- the workgroup-per-row selections, per key (see above) -----------------------------------------------------------------
__device__ __forceinline__ uint64_t mgt_key(uint32_t y, uint32_t v) { return ((uint64_t)v << 32) | (0xFFFFFFFFu - y); }
// (the shift is 56 at most; in two steps, so that 56 + 8 is no shift by 64)
__device__ __forceinline__ bool mgt_agrees_above(uint64_t k, uint64_t prefix, uint32_t shift) { return (((k ^ prefix) >> shift) >> 8) == 0; }

// the end, when one key agrees with the prefix down to `shift`: that key, ORed into (hi, lo), if it is one of the two cells in q
__device__ __forceinline__ void mgt_fetch_key(const uint4 q, uint32_t min_value, uint64_t prefix, uint32_t shift, uint32_t& hi, uint32_t& lo) {
  const uint64_t k0 = mgt_key(q.x, q.y), k1 = mgt_key(q.z, q.w);
  if (mgt_eligible(q.x, q.y, min_value) && ((k0 ^ prefix) >> shift) == 0) { hi |= (uint32_t)(k0 >> 32); lo |= (uint32_t)k0; }
  if (mgt_eligible(q.z, q.w, min_value) && ((k1 ^ prefix) >> shift) == 0) { hi |= (uint32_t)(k1 >> 32); lo |= (uint32_t)k1; }
}
struct MgcPair {                                           // the two cells a lane holds at one step, as rank keys
  uint64_t s0, s1;                                         // score bits
  uint32_t c0, c1;                                         // 0xFFFFFFFF - y
  bool e0, e1;                                             // eligible
};

__device__ __forceinline__ MgcPair mgc_keys(DirSlot* dir, uint32_t dmask, uint8_t* arena, double sa, uint32_t min_value, const uint4 q) {
  MgcPair k{0, 0, ~q.x, ~q.z, mgt_eligible(q.x, q.y, min_value), mgt_eligible(q.z, q.w, min_value)};
  if (k.e0) k.s0 = mgc_score_bits(dir, dmask, arena, sa, q.x, q.y);
  if (k.e1) k.s1 = mgc_score_bits(dir, dmask, arena, sa, q.z, q.w);
  return k;
}

// digit dg of the key: 11 .. 4 are the score's bytes 7 .. 0, 3 .. 0 the column key's
__device__ __forceinline__ uint32_t mgc_digit(uint64_t s, uint32_t c, uint32_t dg) {
  return dg >= 4 ? (uint32_t)(s >> (8 * (dg - 4))) & 255u : (c >> (8 * dg)) & 255u;
}
// the key agrees with the prefix in every digit above dg / down to dg (shifts in two steps: 56 + 8 is no shift by 64)
__device__ __forceinline__ bool mgc_agrees_above(uint64_t s, uint32_t c, uint64_t ps, uint32_t pc, uint32_t dg) {
  return dg >= 4 ? (((s ^ ps) >> (8 * (dg - 4))) >> 8) == 0 : s == ps && (((c ^ pc) >> (8 * dg)) >> 8) == 0;
}
__device__ __forceinline__ bool mgc_agrees_down(uint64_t s, uint32_t c, uint64_t ps, uint32_t pc, uint32_t dg) {
  return dg >= 4 ? ((s ^ ps) >> (8 * (dg - 4))) == 0 : s == ps && ((c ^ pc) >> (8 * dg)) == 0;
}
// where the passes start, from the OR and the AND of two keys and more: the highest digit in which they differ (keys are
// unique: there is one), and the digits above it -- common to all keys -- as the prefix
__device__ __forceinline__ void mgc_start(uint64_t or_s, uint64_t and_s, uint32_t or_c, uint32_t and_c, uint32_t& dg, uint64_t& ps, uint32_t& pc) {
  const uint64_t ds = or_s ^ and_s;
  const uint32_t dc = or_c ^ and_c;
  if (ds) {
    const uint32_t sh = (63u - (uint32_t)__clzll((long long)ds)) & ~7u;
    dg = 4 + (sh >> 3);
    ps = ((and_s >> sh) >> 8) << 8 << sh;
    pc = 0;
  } else {
    const uint32_t sh = dc ? (31u - (uint32_t)__clz((int)dc)) & ~7u : 0u;
    dg = sh >> 3;
    ps = and_s;
    pc = ((and_c >> sh) >> 8) << 8 << sh;
  }
}
__device__ __forceinline__ void mgc_take_digit(uint64_t& ps, uint32_t& pc, uint32_t dg, uint32_t d) {
  if (dg >= 4) ps |= (uint64_t)d << (8 * (dg - 4));
  else pc |= d << (8 * dg);
}

__device__ __forceinline__ uint32_t mg_wave_and(uint32_t v) {
  for (uint32_t d = 32; d; d >>= 1) v &= (uint32_t)__shfl_xor((int)v, d);
  return v;
}

__global__ __launch_bounds__(256) void k_mgt_select(const DirSlot* __restrict__ dir, uint8_t* arena, uint32_t n,
                                                    const uint64_t* __restrict__ items, uint32_t m, uint32_t min_value,
                                                    uint64_t* __restrict__ thr, uint32_t* __restrict__ cnt, uint32_t* big,
                                                    unsigned long long* tot) {
  mgt_select_rows<MgtValueKey>(dir, arena, n, items, m, min_value, {}, {thr}, cnt, big, tot,
                               (blockIdx.x * blockDim.x + threadIdx.x) >> 6, (gridDim.x * blockDim.x) >> 6);
}

__global__ __launch_bounds__(1024) void k_mgt_select_big(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                         uint32_t m, uint32_t min_value, uint64_t* __restrict__ thr,
                                                         uint32_t* __restrict__ cnt, const uint32_t* big, unsigned long long* tot) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[256];
  __shared__ uint32_t wacc[5][16];                         // per wave: eligible, seen, head, OR of the keys (hi, lo)
  __shared__ uint32_t acc[8];                              // 3, 4: the key found; 5 .. 7: d, above, bucket
  auto uni = [&](uint32_t i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)acc[i]); };   // (scalar control flow)
  const uint32_t nent = big[0];
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t e = blockIdx.x; e < nent; e += gridDim.x) {
    const uint32_t r = big[1 + e];
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    const uint32_t size = 1u << meta_lg(s.x);                          // > GETROW_WAVE_MAX: a multiple of 2048
    const uint4* cells = reinterpret_cast<const uint4*>(row_cells(arena, s.z));
    {
      uint32_t elig = 0, seen = 0, head = 0, or_hi = 0, or_lo = 0;
      for (uint32_t p0 = 0; p0 < size; p0 += 2048) {
        const uint4 q = cells[(p0 >> 1) + threadIdx.x];
        seen += ((q.x | q.y) != 0) + ((q.z | q.w) != 0);
        head |= (q.x == 0 && q.y != 0 && q.y >= min_value) | (q.z == 0 && q.w != 0 && q.w >= min_value);
        if (mgt_eligible(q.x, q.y, min_value)) { elig++; or_hi |= q.y; or_lo |= ~q.x; }
        if (mgt_eligible(q.z, q.w, min_value)) { elig++; or_hi |= q.w; or_lo |= ~q.z; }
      }
      elig = mg_wave_sum(elig); seen = mg_wave_sum(seen);
      head = mg_wave_or(head); or_hi = mg_wave_or(or_hi); or_lo = mg_wave_or(or_lo);
      const uint32_t w = threadIdx.x >> 6;
      if (lane == 0) { wacc[0][w] = elig; wacc[1][w] = seen; wacc[2][w] = head; wacc[3][w] = or_hi; wacc[4][w] = or_lo; }
    }
    __syncthreads();
    uint32_t elig = 0, seen = 0, head = 0, or_hi = 0, or_lo = 0;
    for (uint32_t i = 0; i < 16; i++) { elig += wacc[0][i]; seen += wacc[1][i]; head |= wacc[2][i]; or_hi |= wacc[3][i]; or_lo |= wacc[4][i]; }
    elig = (uint32_t)__builtin_amdgcn_readfirstlane((int)elig);
    const uint64_t orall = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)or_hi) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)or_lo);
    if (threadIdx.x == 0 && seen) atomicAdd(tot, (unsigned long long)seen);
    uint64_t t = 0;
    if (elig > m) {                                                    // (from LDS: the same on every lane)
      uint32_t shift = (63u - (uint32_t)__clzll((long long)orall)) & ~7u, need = m;
      uint64_t prefix = 0;
      for (;;) {
        __syncthreads();                                               // (acc and hist were read by every lane)
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t p0 = 0; p0 < size; p0 += 2048) {
          const uint4 q = cells[(p0 >> 1) + threadIdx.x];
          const uint64_t k0 = mgt_key(q.x, q.y), k1 = mgt_key(q.z, q.w);
          mgt_hist_add(hist, mgt_eligible(q.x, q.y, min_value) && mgt_agrees_above(k0, prefix, shift), (uint32_t)(k0 >> shift) & 255u, lane);
          mgt_hist_add(hist, mgt_eligible(q.z, q.w, min_value) && mgt_agrees_above(k1, prefix, shift), (uint32_t)(k1 >> shift) & 255u, lane);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
          uint32_t d, above, bucket;
          mgt_pick<true>(hist, need, lane, d, above, bucket);
          if (lane == 0) { acc[5] = d; acc[6] = above; acc[7] = bucket; }
        }
        __syncthreads();
        need -= uni(6);
        prefix |= (uint64_t)uni(5) << shift;
        if (shift == 0) { t = prefix; break; }
        if (uni(7) == 1) {
          if (threadIdx.x < 2) acc[3 + threadIdx.x] = 0;
          __syncthreads();
          uint32_t hi = 0, lo = 0;
          for (uint32_t p0 = 0; p0 < size; p0 += 2048) mgt_fetch_key(cells[(p0 >> 1) + threadIdx.x], min_value, prefix, shift, hi, lo);
          if (hi | lo) { acc[3] = hi; acc[4] = lo; }                     // (one lane of the workgroup: keys are unique)
          __syncthreads();
          t = ((uint64_t)acc[3] << 32) | acc[4];
          break;
        }
        shift -= 8;
      }
    }
    if (threadIdx.x == 0) { thr[r] = t; cnt[r] = (elig < m ? elig : m) + head; }
    __syncthreads();                                                   // (wacc and acc are the next row's)
  }
}

__global__ __launch_bounds__(256) void k_mgc_select(DirSlot* dir, uint32_t dmask, uint8_t* arena, uint32_t n,
                                                    const uint64_t* __restrict__ items, uint32_t m, uint32_t min_value,
                                                    uint64_t* __restrict__ thr, uint32_t* __restrict__ thr_col,
                                                    uint32_t* __restrict__ cnt, uint32_t* big, unsigned long long* tot) {
  mgt_select_rows<MgtCosineKey>(dir, arena, n, items, m, min_value, {dir, arena, items, dmask}, {thr, thr_col}, cnt, big, tot,
                                (blockIdx.x * blockDim.x + threadIdx.x) >> 6, (gridDim.x * blockDim.x) >> 6);
}

__global__ __launch_bounds__(1024) void k_mgc_select_big(DirSlot* dir, uint32_t dmask, uint8_t* arena, const uint64_t* __restrict__ items,
                                                         uint32_t m, uint32_t min_value, uint64_t* __restrict__ thr,
                                                         uint32_t* __restrict__ thr_col, uint32_t* __restrict__ cnt, const uint32_t* big,
                                                         unsigned long long* tot) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[256];
  __shared__ uint32_t wacc[6][16];                         // per wave: eligible, seen, head; then OR (hi, lo, col) and AND of the keys
  __shared__ uint32_t acc[8];                              // 2 .. 4: the key found; 5 .. 7: d, above, bucket
  auto uni = [&](uint32_t i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)acc[i]); };   // (scalar control flow)
  const uint32_t nent = big[0];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t e = blockIdx.x; e < nent; e += gridDim.x) {
    const uint32_t r = big[1 + e];
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    const uint32_t size = 1u << meta_lg(s.x);                          // > GETROW_WAVE_MAX: a multiple of 2048
    const uint4* cells = reinterpret_cast<const uint4*>(row_cells(arena, s.z));
    {
      uint32_t elig = 0, seen = 0, head = 0;
      for (uint32_t p0 = 0; p0 < size; p0 += 2048) {
        const uint4 q = cells[(p0 >> 1) + threadIdx.x];
        seen += ((q.x | q.y) != 0) + ((q.z | q.w) != 0);
        head |= (q.x == 0 && q.y != 0 && q.y >= min_value) | (q.z == 0 && q.w != 0 && q.w >= min_value);
        elig += mgt_eligible(q.x, q.y, min_value) + mgt_eligible(q.z, q.w, min_value);
      }
      elig = mg_wave_sum(elig); seen = mg_wave_sum(seen); head = mg_wave_or(head);
      if (lane == 0) { wacc[0][w] = elig; wacc[1][w] = seen; wacc[2][w] = head; }
    }
    __syncthreads();
    uint32_t elig = 0, seen = 0, head = 0;
    for (uint32_t i = 0; i < 16; i++) { elig += wacc[0][i]; seen += wacc[1][i]; head |= wacc[2][i]; }
    elig = (uint32_t)__builtin_amdgcn_readfirstlane((int)elig);
    if (threadIdx.x == 0 && seen) atomicAdd(tot, (unsigned long long)seen);
    uint64_t ts = 0;
    uint32_t tc = 0;
    if (elig > m) {                                                    // (from LDS: the same on every lane)
      bool dummy = false;
      const double sa = sqrt((double)apply_one<OP_GET>(dir, dmask, arena, s.y, 0u, 0u, &dummy));
      __syncthreads();                                                 // (wacc was read by every lane)
      {
        uint32_t or_h = 0, or_l = 0, or_c = 0, and_h = ~0u, and_l = ~0u, and_c = ~0u;
        for (uint32_t p0 = 0; p0 < size; p0 += 2048) {
          const MgcPair k = mgc_keys(dir, dmask, arena, sa, min_value, cells[(p0 >> 1) + threadIdx.x]);
          if (k.e0) { or_h |= (uint32_t)(k.s0 >> 32); or_l |= (uint32_t)k.s0; or_c |= k.c0; and_h &= (uint32_t)(k.s0 >> 32); and_l &= (uint32_t)k.s0; and_c &= k.c0; }
          if (k.e1) { or_h |= (uint32_t)(k.s1 >> 32); or_l |= (uint32_t)k.s1; or_c |= k.c1; and_h &= (uint32_t)(k.s1 >> 32); and_l &= (uint32_t)k.s1; and_c &= k.c1; }
        }
        or_h = mg_wave_or(or_h); or_l = mg_wave_or(or_l); or_c = mg_wave_or(or_c);
        and_h = mg_wave_and(and_h); and_l = mg_wave_and(and_l); and_c = mg_wave_and(and_c);
        if (lane == 0) { wacc[0][w] = or_h; wacc[1][w] = or_l; wacc[2][w] = or_c; wacc[3][w] = and_h; wacc[4][w] = and_l; wacc[5][w] = and_c; }
      }
      __syncthreads();
      uint32_t dg, need = m, pc;
      uint64_t ps;
      {
        uint32_t or_h = 0, or_l = 0, or_c = 0, and_h = ~0u, and_l = ~0u, and_c = ~0u;
        for (uint32_t i = 0; i < 16; i++) { or_h |= wacc[0][i]; or_l |= wacc[1][i]; or_c |= wacc[2][i]; and_h &= wacc[3][i]; and_l &= wacc[4][i]; and_c &= wacc[5][i]; }
        auto sc = [](uint32_t v) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
        mgc_start(((uint64_t)sc(or_h) << 32) | sc(or_l), ((uint64_t)sc(and_h) << 32) | sc(and_l), sc(or_c), sc(and_c), dg, ps, pc);
      }
      for (;;) {
        __syncthreads();                                               // (acc and hist were read by every lane)
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t p0 = 0; p0 < size; p0 += 2048) {
          const MgcPair k = mgc_keys(dir, dmask, arena, sa, min_value, cells[(p0 >> 1) + threadIdx.x]);
          mgt_hist_add(hist, k.e0 && mgc_agrees_above(k.s0, k.c0, ps, pc, dg), mgc_digit(k.s0, k.c0, dg), lane);
          mgt_hist_add(hist, k.e1 && mgc_agrees_above(k.s1, k.c1, ps, pc, dg), mgc_digit(k.s1, k.c1, dg), lane);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
          uint32_t d, above, bucket;
          mgt_pick<true>(hist, need, lane, d, above, bucket);
          if (lane == 0) { acc[5] = d; acc[6] = above; acc[7] = bucket; }
        }
        __syncthreads();
        need -= uni(6);
        mgc_take_digit(ps, pc, dg, uni(5));
        if (dg == 0) break;
        if (uni(7) == 1) {
          if (threadIdx.x < 3) acc[2 + threadIdx.x] = 0;
          __syncthreads();
          for (uint32_t p0 = 0; p0 < size; p0 += 2048) {               // (one lane of the workgroup: keys are unique)
            const MgcPair k = mgc_keys(dir, dmask, arena, sa, min_value, cells[(p0 >> 1) + threadIdx.x]);
            if (k.e0 && mgc_agrees_down(k.s0, k.c0, ps, pc, dg)) { acc[2] = (uint32_t)(k.s0 >> 32); acc[3] = (uint32_t)k.s0; acc[4] = k.c0; }
            if (k.e1 && mgc_agrees_down(k.s1, k.c1, ps, pc, dg)) { acc[2] = (uint32_t)(k.s1 >> 32); acc[3] = (uint32_t)k.s1; acc[4] = k.c1; }
          }
          __syncthreads();
          ps = ((uint64_t)uni(2) << 32) | uni(3);
          pc = uni(4);
          break;
        }
        dg--;
      }
      ts = ps; tc = pc;
    }
    if (threadIdx.x == 0) { thr[r] = ts; thr_col[r] = tc; cnt[r] = (elig < m ? elig : m) + head; }
    __syncthreads();                                                   // (wacc and acc are the next row's)
  }
}

// the emission: the walkers above with the per-row threshold
__global__ __launch_bounds__(256) void k_mgt_emit(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                  const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t r1,
                                                  uint32_t* __restrict__ rec, uint32_t* big, const MgTopk f) {
  mg_emit_rows(dir, arena, items, ptr, r0, r1, rec, big, (blockIdx.x * blockDim.x + threadIdx.x) >> 6, (gridDim.x * blockDim.x) >> 6, f);
}

template <bool COUNT>
__global__ __launch_bounds__(1024) void k_mgt_emit_big(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                       const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t* __restrict__ rec,
                                                       const uint32_t* big, uint32_t* seg_cnt, const MgTopk f) {
  mg_emit_segs<COUNT>(dir, arena, items, ptr, r0, rec, big, seg_cnt, f);
}

__global__ __launch_bounds__(256) void k_mgc_emit(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                  const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t r1,
                                                  uint32_t* __restrict__ rec, uint32_t* big, const MgCos f) {
  mg_emit_rows(dir, arena, items, ptr, r0, r1, rec, big, (blockIdx.x * blockDim.x + threadIdx.x) >> 6, (gridDim.x * blockDim.x) >> 6, f);
}

template <bool COUNT>
__global__ __launch_bounds__(1024) void k_mgc_emit_big(const DirSlot* __restrict__ dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                       const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t* __restrict__ rec,
                                                       const uint32_t* big, uint32_t* seg_cnt, const MgCos f) {
  mg_emit_segs<COUNT>(dir, arena, items, ptr, r0, rec, big, seg_cnt, f);
}

// ---- smatrix_merge_topk_sim: the four kernels over MgtSimKey ------------------------------------------------------------------
// The workgroup-per-row selection, written ONCE over a key policy of RkCosine's shape (a 96-bit key that costs a gather: no key
// in the counting pass, the start from the OR and the AND of the keys): k_mgc_select_big's steps, with the key arithmetic taken
// from the policy.  k_mgc_select_big itself stays written out (see above: the fold measured slower for the value key, and the
// cosine kernel's registers are pinned by the build it was written with); a third written-out copy would add nothing.
template <typename P>
__device__ __forceinline__ void mgr_select_big_rows(const DirSlot* dir, uint8_t* arena, const uint64_t* __restrict__ items, uint32_t m,
                                                    uint32_t min_value, const typename P::Src src, const typename P::Thr thr,
                                                    uint32_t* __restrict__ cnt, const uint32_t* big, unsigned long long* tot) {
  typedef typename P::Key Key;
  static_assert(P::W == 3 && !P::FREE, "a 96-bit key made by a gather");
  __shared__ __attribute__((aligned(16))) uint32_t hist[256];
  __shared__ uint32_t wacc[6][16];                         // per wave: eligible, seen, head; then the six words of P::Acc
  __shared__ uint32_t acc[8];                              // 2 .. 4: the key found; 5 .. 7: d, above, bucket
  auto uni = [&](uint32_t i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)acc[i]); };   // (scalar control flow)
  const uint32_t nent = big[0];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t e = blockIdx.x; e < nent; e += gridDim.x) {
    const uint32_t r = big[1 + e];
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    const uint32_t size = 1u << meta_lg(s.x);                          // > GETROW_WAVE_MAX: a multiple of 2048
    const uint4* cells = reinterpret_cast<const uint4*>(row_cells(arena, s.z));
    {
      uint32_t elig = 0, seen = 0, head = 0;
      for (uint32_t p0 = 0; p0 < size; p0 += 2048) {
        const uint4 q = cells[(p0 >> 1) + threadIdx.x];
        seen += ((q.x | q.y) != 0) + ((q.z | q.w) != 0);
        head |= (q.x == 0 && q.y != 0 && q.y >= min_value) | (q.z == 0 && q.w != 0 && q.w >= min_value);
        elig += mgt_eligible(q.x, q.y, min_value) + mgt_eligible(q.z, q.w, min_value);
      }
      elig = mg_wave_sum(elig); seen = mg_wave_sum(seen); head = mg_wave_or(head);
      if (lane == 0) { wacc[0][w] = elig; wacc[1][w] = seen; wacc[2][w] = head; }
    }
    __syncthreads();
    uint32_t elig = 0, seen = 0, head = 0;
    for (uint32_t i = 0; i < 16; i++) { elig += wacc[0][i]; seen += wacc[1][i]; head |= wacc[2][i]; }
    elig = (uint32_t)__builtin_amdgcn_readfirstlane((int)elig);
    if (threadIdx.x == 0 && seen) atomicAdd(tot, (unsigned long long)seen);
    Key t = P::zero();
    if (elig > m) {                                                    // (from LDS: the same on every lane)
      const typename P::Row row = src.row(s.y);
      __syncthreads();                                                 // (wacc was read by every lane)
      {
        typename P::Acc a = P::acc0();
        for (uint32_t p0 = 0; p0 < size; p0 += 2048) {
          const MgtPair<Key> k = mgt_keys<P>(row, min_value, cells[(p0 >> 1) + threadIdx.x]);
          if (k.e0) P::acc_add(a, k.k0);
          if (k.e1) P::acc_add(a, k.k1);
        }
#pragma unroll
        for (uint32_t i = 0; i < 6; i++) { const uint32_t v = mg_wave_or(a.w[i]); if (lane == 0) wacc[i][w] = v; }
      }
      __syncthreads();
      uint32_t need = m;
      typename P::Acc a = P::acc0();
#pragma unroll
      for (uint32_t i = 0; i < 6; i++) {
        uint32_t v = 0;
        for (uint32_t j = 0; j < 16; j++) v |= wacc[i][j];
        a.w[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
      }
      Key prefix;
      uint32_t dg = P::start(a, prefix);
      for (;;) {
        __syncthreads();                                               // (acc and hist were read by every lane)
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t p0 = 0; p0 < size; p0 += 2048) {
          const MgtPair<Key> k = mgt_keys<P>(row, min_value, cells[(p0 >> 1) + threadIdx.x]);
          mgt_hist_add(hist, k.e0 && P::agrees_above(k.k0, prefix, dg), P::digit(k.k0, dg), lane);
          mgt_hist_add(hist, k.e1 && P::agrees_above(k.k1, prefix, dg), P::digit(k.k1, dg), lane);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
          uint32_t d, above, bucket;
          mgt_pick<true>(hist, need, lane, d, above, bucket);
          if (lane == 0) { acc[5] = d; acc[6] = above; acc[7] = bucket; }
        }
        __syncthreads();
        need -= uni(6);
        P::take_digit(prefix, dg, uni(5));
        if (dg == 0) break;
        if (uni(7) == 1) {
          if (threadIdx.x < 3) acc[2 + threadIdx.x] = 0;
          __syncthreads();
          for (uint32_t p0 = 0; p0 < size; p0 += 2048) {               // (one lane of the workgroup: keys are unique)
            const MgtPair<Key> k = mgt_keys<P>(row, min_value, cells[(p0 >> 1) + threadIdx.x]);
            const bool h0 = k.e0 && P::agrees_down(k.k0, prefix, dg), h1 = k.e1 && P::agrees_down(k.k1, prefix, dg);
            if (h0 || h1) {
              uint32_t kw[3] = {0, 0, 0};
              P::or_words(kw, h0 ? k.k0 : k.k1);
              acc[2] = kw[0]; acc[3] = kw[1]; acc[4] = kw[2];
            }
          }
          __syncthreads();
          const uint32_t kw[3] = {uni(2), uni(3), uni(4)};
          prefix = P::from_words(kw);
          break;
        }
        dg--;
      }
      t = prefix;
    }
    if (threadIdx.x == 0) { thr.store(r, t); cnt[r] = (elig < m ? elig : m) + head; }
    __syncthreads();                                                   // (wacc and acc are the next row's)
  }
}

__global__ __launch_bounds__(256) void k_mgs_select(DirSlot* dir, uint32_t dmask, uint8_t* arena, uint32_t n,
                                                    const uint64_t* __restrict__ items, uint32_t m, uint32_t min_value, const SimArgs sim,
                                                    uint64_t* __restrict__ thr, uint32_t* __restrict__ thr_col,
                                                    uint32_t* __restrict__ cnt, uint32_t* big, unsigned long long* tot) {
  mgt_select_rows<MgtSimKey>(dir, arena, n, items, m, min_value, {dir, arena, items, dmask, sim}, {thr, thr_col}, cnt, big, tot,
                             (blockIdx.x * blockDim.x + threadIdx.x) >> 6, (gridDim.x * blockDim.x) >> 6);
}

__global__ __launch_bounds__(1024) void k_mgs_select_big(DirSlot* dir, uint32_t dmask, uint8_t* arena, const uint64_t* __restrict__ items,
                                                         uint32_t m, uint32_t min_value, const SimArgs sim, uint64_t* __restrict__ thr,
                                                         uint32_t* __restrict__ thr_col, uint32_t* __restrict__ cnt, const uint32_t* big,
                                                         unsigned long long* tot) {
  mgr_select_big_rows<MgtSimKey>(dir, arena, items, m, min_value, {dir, arena, items, dmask, sim}, {thr, thr_col}, cnt, big, tot);
}

// The emission's filter as the kernels take it: MgSim without the directory, the arena and the row list, which every emission
// kernel is handed anyway -- as a second copy in the argument they are six scalar registers the compiler cannot tell from the
// first, and k_mgs_emit_big<false> has none to spare.
struct MgSimArgs {
  uint64_t* thr;
  uint32_t* thr_col;
  uint32_t dmask, min_value;
  SimArgs sim;
  __device__ __forceinline__ MgSim over(const DirSlot* dir, uint8_t* arena, const uint64_t* items) const {
    return MgSim{{thr, thr_col}, {const_cast<DirSlot*>(dir), arena, items, dmask, sim}, min_value};
  }
};

__global__ __launch_bounds__(256) void k_mgs_emit(const DirSlot* dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                  const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t r1,
                                                  uint32_t* __restrict__ rec, uint32_t* big, const MgSimArgs f) {
  mg_emit_rows(dir, arena, items, ptr, r0, r1, rec, big, (blockIdx.x * blockDim.x + threadIdx.x) >> 6, (gridDim.x * blockDim.x) >> 6,
               f.over(dir, arena, items));
}

template <bool COUNT>
__global__ __launch_bounds__(1024) void k_mgs_emit_big(const DirSlot* dir, uint8_t* arena, const uint64_t* __restrict__ items,
                                                       const uint64_t* __restrict__ ptr, uint32_t r0, uint32_t* __restrict__ rec,
                                                       const uint32_t* big, uint32_t* seg_cnt, const MgSimArgs f) {
  mg_emit_segs<COUNT>(dir, arena, items, ptr, r0, rec, big, seg_cnt, f.over(dir, arena, items));
}

// ---- from a CSR in smatrix_export's layout ------------------------------------------------------------------------------------
// k_mg_csr_check: *bad |= 1 unless row_ptr[0] == 0 and row_ptr[i] <= row_ptr[i + 1] for every i < n_rows (before the first write)
__global__ __launch_bounds__(256) void k_mg_csr_check(uint64_t n_rows, const uint64_t* __restrict__ row_ptr, uint32_t* bad) {
  bool b = false;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += stride) b |= row_ptr[i] > row_ptr[i + 1];
  if (blockIdx.x == 0 && threadIdx.x == 0) b |= row_ptr[0] != 0;
  if (__any(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

// A lane per pair of [t0, t0 + count); `pairs` points at pair t0.  The pair's row is the last r with row_ptr[r] <= t (rows of
// length 0 share their successor's row_ptr and are never that one).  Two lanes of the workgroup search all of row_ptr for the
// tile's first and last pair; every lane then searches between those two rows only -- one row in the common case, any number
// of empty rows or a row longer than the tile in the others.
__device__ inline uint64_t mg_row_of(const uint64_t* __restrict__ row_ptr, uint64_t lo, uint64_t hi, uint64_t t) {
  while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (row_ptr[mid] <= t) lo = mid; else hi = mid; }
  return lo;                                                           // row_ptr[lo] <= t < row_ptr[hi]
}

__global__ __launch_bounds__(256) void k_mg_emit_csr(uint64_t n_rows, const uint32_t* __restrict__ rows, const uint64_t* __restrict__ row_ptr,
                                                     const uint32_t* __restrict__ pairs, uint64_t t0, uint32_t count,
                                                     uint32_t* __restrict__ rec) {
  __shared__ uint64_t s_row[2];
  const uint32_t k0 = blockIdx.x * blockDim.x;                         // (the grid covers count exactly: k0 < count)
  if (threadIdx.x < 2) {
    const uint32_t k = threadIdx.x == 0 ? k0 : min(k0 + blockDim.x, count) - 1u;
    s_row[threadIdx.x] = mg_row_of(row_ptr, 0, n_rows, t0 + k);
  }
  __syncthreads();
  const uint32_t k = k0 + threadIdx.x;
  if (k >= count) return;
  const uint64_t r = mg_row_of(row_ptr, s_row[0], s_row[1] + 1, t0 + k);
  mg_put(rec, k, rows[r], pairs[2 * (uint64_t)k], pairs[2 * (uint64_t)k + 1]);    // (a caller's uint32 array: 4-byte aligned is all that is known)
}
