// kernels/import_events.hpp -- the windowed, weighted, reversible session import (include/smatrix_batch.h
// smatrix_cf_import_events): the ops of every session generated on the device and compacted, chunk by chunk, into the arrays
// the ordinary write path applies.  Host side: smx_import.inc.
// A fragment of smx_kernels.hpp: included there after explain.hpp, INSIDE namespace smx.
//
// The slot space.  A session of L positions owns L * C slots, C = imp_cols(L, window, flags) candidate columns per position:
//     window == 0          C = L                      (no limit)
//     both directions      C = min(L, 2 * window + 1)
//     IMP_FORWARD          C = min(L, window + 1)
// Slot r of the session is position p = r / C and candidate c = r % C.  Its partner position q is
//     both directions      q = start + c, start = p - window clamped to [0, L - C]: the C positions of the session nearest to p
//     IMP_FORWARD          q = p + c
// so every q within reach of p is named by exactly one slot of p, and q == p (one slot per position) is the head op.  A slot
// emits nothing when q falls outside the session or the window (the padding of the clamp), when an amount is 0, or for a
// self-pair under IMP_NO_SELF.  With the default arguments C = L, q = c and every slot emits: k_cf_expand's enumeration.
//   k_imp_scan_*   soff[s] = the slots of the sessions before s (n + 1 entries), by a three-kernel scan over tiles of IMP_TILE
//                  sessions.  Every add saturates at IMP_SAT = 2^63, and a session whose offsets decrease counts IMP_SAT slots:
//                  soff[n] >= 2^63 is the one thing the host has to read to refuse a call.
//   k_imp_emit     a lane per slot of the chunk [t0, t0 + count): the session by binary search in soff, (p, c) by one division,
//                  no loop over a session.  The emitting lanes of a wave are counted by a ballot, numbered by mbcnt, and given
//                  their place in the chunk's output by ONE atomic add per wave on the chunk's counter; their ops go through
//                  the wave's part of an LDS buffer so that the stores to xs / ys / vs come from the wave's first lanes, to
//                  consecutive entries (imp_compact).  The chunk holds at most `count` ops: nothing is written beyond entry
//                  count - 1.  With ImpArgs::heads false the slots with q == p emit nothing: the pair ops alone.
//   k_imp_heads    the head ops alone, a lane per position of ids, compacted the same way.  A DECR call applies the pair ops
//                  first and the head ops behind them, in batches of their own (smx_import.inc says why).

constexpr uint64_t IMP_SAT = 1ull << 63;
constexpr uint32_t IMP_FORWARD = 1u, IMP_NO_SELF = 2u;
constexpr uint32_t IMP_THREADS = 256, IMP_PER_THREAD = 8, IMP_TILE = IMP_THREADS * IMP_PER_THREAD;

__host__ __device__ inline uint64_t imp_sat_add(uint64_t a, uint64_t b) {           // a, b <= IMP_SAT
  const uint64_t s = a + b;
  return (s < a || s > IMP_SAT) ? IMP_SAT : s;
}
__host__ __device__ inline uint64_t imp_cols(uint64_t L, uint32_t window, uint32_t flags) {
  if (window == 0) return L;
  const uint64_t c = (flags & IMP_FORWARD) ? (uint64_t)window + 1 : 2 * (uint64_t)window + 1;
  return c < L ? c : L;
}
// the slots of the session [b0, b1) of the offsets
__host__ __device__ inline uint64_t imp_slots(uint64_t b0, uint64_t b1, uint32_t window, uint32_t flags) {
  if (b1 < b0) return IMP_SAT;
  const uint64_t L = b1 - b0, c = imp_cols(L, window, flags);
  return (c && L > IMP_SAT / c) ? IMP_SAT : L * c;
}

// inclusive saturating scan of one value per thread over the block (IMP_THREADS lanes); sh[IMP_THREADS - 1] = the block's sum
__device__ __forceinline__ uint64_t imp_block_scan(uint64_t v, uint64_t* sh) {
  const uint32_t t = threadIdx.x;
  __syncthreads();                                                   // (sh may still be read from the call before)
  sh[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < IMP_THREADS; d <<= 1) {
    const uint64_t o = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    v = imp_sat_add(v, o);
    sh[t] = v;
    __syncthreads();
  }
  return v;
}

// part[b] = the slots of tile b's sessions
__global__ __launch_bounds__(IMP_THREADS) void k_imp_scan_reduce(uint32_t n, const uint64_t* __restrict__ off, uint32_t window,
                                                                 uint32_t flags, uint64_t* __restrict__ part) {
  __shared__ uint64_t sh[IMP_THREADS];
  const uint64_t s0 = (uint64_t)blockIdx.x * IMP_TILE + (uint64_t)threadIdx.x * IMP_PER_THREAD;
  uint64_t sum = 0;
  for (uint32_t j = 0; j < IMP_PER_THREAD; j++)
    if (s0 + j < n) sum = imp_sat_add(sum, imp_slots(off[s0 + j], off[s0 + j + 1], window, flags));
  imp_block_scan(sum, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = sh[IMP_THREADS - 1];
}

// part[0 .. nt) -> its exclusive scan, part[nt] = the total; one block
__global__ __launch_bounds__(IMP_THREADS) void k_imp_scan_part(uint64_t* part, uint32_t nt) {
  __shared__ uint64_t sh[IMP_THREADS];
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < nt; b0 += IMP_THREADS) {                // (block-uniform loop)
    const uint32_t b = b0 + threadIdx.x;
    const uint64_t v = b < nt ? part[b] : 0ull;
    imp_block_scan(v, sh);
    if (b < nt) part[b] = imp_sat_add(carry, threadIdx.x ? sh[threadIdx.x - 1] : 0ull);
    carry = imp_sat_add(carry, sh[IMP_THREADS - 1]);
  }
  if (threadIdx.x == 0) part[nt] = carry;
}

// soff[s] = part[tile of s] + the slots of the tile's sessions before s; soff[n] = part[nt]
__global__ __launch_bounds__(IMP_THREADS) void k_imp_scan_apply(uint32_t n, const uint64_t* __restrict__ off, uint32_t window,
                                                                uint32_t flags, const uint64_t* __restrict__ part, uint32_t nt,
                                                                uint64_t* __restrict__ soff) {
  __shared__ uint64_t sh[IMP_THREADS];
  const uint64_t s0 = (uint64_t)blockIdx.x * IMP_TILE + (uint64_t)threadIdx.x * IMP_PER_THREAD;
  uint64_t c[IMP_PER_THREAD], sum = 0;
  for (uint32_t j = 0; j < IMP_PER_THREAD; j++) {
    c[j] = s0 + j < n ? imp_slots(off[s0 + j], off[s0 + j + 1], window, flags) : 0ull;
    sum = imp_sat_add(sum, c[j]);
  }
  imp_block_scan(sum, sh);
  uint64_t run = imp_sat_add(part[blockIdx.x], threadIdx.x ? sh[threadIdx.x - 1] : 0ull);
  for (uint32_t j = 0; j < IMP_PER_THREAD; j++) {
    if (s0 + j < n) soff[s0 + j] = run;
    run = imp_sat_add(run, c[j]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) soff[n] = part[nt];
}

struct ImpArgs {
  const uint64_t* off;                        // n + 1: session s is ids[off[s] .. off[s+1])
  const uint32_t* ids;
  const uint32_t* amt;                        // per entry of ids, or NULL: every amount 1
  const uint64_t* soff;                       // n + 1: the slots before session s (k_imp_scan_apply)
  uint32_t n, window, flags;
  bool heads;                                 // the slots with q == p emit their head op (false: the pair ops alone)
};

// The compaction, for every lane of a 256-lane workgroup (no lane may have returned): the op (x, y, v) of the lanes with `emit`
// goes to the next free entries of xs / ys / vs, counted in *cnt; nothing is written at or beyond entry `count`.
__device__ __forceinline__ void imp_compact(bool emit, uint32_t x, uint32_t y, uint32_t v, uint32_t count, uint32_t* cnt,
                                            uint32_t* __restrict__ xs, uint32_t* __restrict__ ys, uint32_t* __restrict__ vs) {
  __shared__ uint32_t l_x[256], l_y[256], l_v[256];
  const uint32_t lane = threadIdx.x & 63u, w0 = threadIdx.x & ~63u;
  const uint64_t m = __ballot(emit);
  const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  const uint32_t total = (uint32_t)__popcll(m);
  uint32_t base = 0;
  if (lane == 0 && total) base = atomicAdd(cnt, total);
  base = (uint32_t)__shfl((int)base, 0);
  if (emit) { l_x[w0 + before] = x; l_y[w0 + before] = y; l_v[w0 + before] = v; }
  __syncthreads();
  if (lane < total && base + lane < count) {
    xs[base + lane] = l_x[w0 + lane]; ys[base + lane] = l_y[w0 + lane]; vs[base + lane] = l_v[w0 + lane];
  }
}

// the head ops alone, a lane per position of the range [i0, i0 + count) of ids: (ids[i], 0, amt[i]) where the amount is not 0
__global__ __launch_bounds__(256) void k_imp_heads(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ amt, uint64_t i0,
                                                   uint32_t count, uint32_t* cnt, uint32_t* __restrict__ xs,
                                                   uint32_t* __restrict__ ys, uint32_t* __restrict__ vs) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t x = 0, v = 0;
  if (k < count) { x = ids[i0 + k]; v = amt ? amt[i0 + k] : 1u; }
  imp_compact(v != 0, x, 0u, v, count, cnt, xs, ys, vs);
}

__global__ __launch_bounds__(256) void k_imp_emit(ImpArgs a, uint64_t t0, uint32_t count, uint32_t* cnt, uint32_t* __restrict__ xs,
                                                  uint32_t* __restrict__ ys, uint32_t* __restrict__ vs) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  bool emit = false;
  uint32_t x = 0, y = 0, v = 0;
  if (k < count) {
    const uint64_t t = t0 + k;
    uint32_t lo = 0, hi = a.n;                             // the last session with soff[s] <= t
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (a.soff[mid] <= t) lo = mid; else hi = mid; }
    const uint64_t first = a.off[lo], L = a.off[lo + 1] - first, r = t - a.soff[lo];
    const uint64_t C = imp_cols(L, a.window, a.flags);
    if (C) {
      const uint64_t p = r / C, c = r - p * C;
      uint64_t q;
      bool ok;
      if (a.flags & IMP_FORWARD) {
        q = p + c;
        ok = q < L;
      } else {
        uint64_t start = (a.window && p > a.window) ? p - a.window : 0ull;
        if (start > L - C) start = L - C;
        q = start + c;
        ok = a.window == 0 || (q > p ? q - p : p - q) <= a.window;
      }
      if (ok && p < L) {
        const uint32_t idp = a.ids[first + p], wp = a.amt ? a.amt[first + p] : 1u;
        if (q == p) {
          emit = a.heads && wp != 0; x = idp; y = 0u; v = wp;
        } else {
          const uint32_t idq = a.ids[first + q], wq = a.amt ? a.amt[first + q] : 1u;
          emit = wp != 0 && wq != 0 && !((a.flags & IMP_NO_SELF) && idp == idq);
          x = idp; y = idq; v = wp < wq ? wp : wq;
        }
      }
    }
  }
  imp_compact(emit, x, y, v, count, cnt, xs, ys, vs);
}
