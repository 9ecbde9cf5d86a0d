// kernels/export.hpp -- whole-matrix export (include/smatrix_batch.h smatrix_export): the row list, exact pair counts, scans,
// and the sorts of the SORTED order.  The pairs themselves are written by k_getrow / k_getrow_big (rows.hpp): this file has no
// second row walker.
// A fragment of smx_kernels.hpp: included there, after rows.hpp, INSIDE namespace smx; not a header of its own.
//
// Everything here is deterministic: lists are built by per-tile counts, a scan and an ordered write (never by atomics that
// reserve list space), and the sorts are stable LSD radix sorts or LDS bitonic sorts of unique keys.  The only atomics are
// integer sums (the pair count of a big row over its segments) and the tier lists of the per-row sort, whose order does not
// reach the output (every row is sorted in its own range, which the row pointers fix).
//
// A list entry (row list, radix sort item, pair) is one 64-bit word whose LOW word is the sort key: {row id, directory slot}
// for the row list, {column, value} for the pairs -- so one radix sort serves both.

constexpr uint32_t EX_THREADS = 256;               // every tile kernel: 4 waves
constexpr uint32_t EX_PER_THREAD = 16;
constexpr uint32_t EX_TILE = EX_THREADS * EX_PER_THREAD;   // 4096 entries per tile
constexpr uint32_t EX_LDS_SMALL = 512;             // rows of up to this many pairs: a 64-lane workgroup sorts them in LDS (4 KiB)
constexpr uint32_t EX_LDS_MID = 4096;              // ... up to this many: a 256-lane workgroup (32 KiB); longer rows: the segmented radix sort

// exclusive prefix of v over the 256 lanes of the workgroup; *total = the sum.  wsum: 4 words of LDS.  Ends with a barrier, so
// wsum may be reused at once.
__device__ inline uint64_t ex_block_excl(uint64_t v, uint64_t* wsum, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t incl = v;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  uint64_t before = 0, tot = 0;
  for (uint32_t i = 0; i < EX_THREADS / 64; i++) { const uint64_t t = wsum[i]; if (i < w) before += t; tot += t; }
  *total = tot;
  __syncthreads();
  return before + incl - v;
}

// ---- scan: u32 counts -> u64 exclusive prefix (n + 1 entries, the last = the total) ----------------------------------------
//   k_ex_scan_reduce  part[t] = sum of tile t
//   k_ex_scan_part    one workgroup: part[0 .. nt] = exclusive prefix of the tile sums, part[nt] = total
//   k_ex_scan_apply   out[i] = part[tile] + prefix inside the tile;  out[n] = total
__global__ __launch_bounds__(256) void k_ex_scan_reduce(const uint32_t* __restrict__ in, uint64_t n, uint64_t* __restrict__ part) {
  __shared__ uint64_t wsum[4];
  const uint64_t t = blockIdx.x, i0 = t * EX_TILE + (uint64_t)threadIdx.x * EX_PER_THREAD;
  uint64_t s = 0;
  for (uint32_t k = 0; k < EX_PER_THREAD; k++) if (i0 + k < n) s += in[i0 + k];
  uint64_t tot;
  ex_block_excl(s, wsum, &tot);
  if (threadIdx.x == 0) part[t] = tot;
}

__global__ __launch_bounds__(256) void k_ex_scan_part(uint64_t* part, uint32_t nt) {
  __shared__ uint64_t wsum[4];
  __shared__ uint64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t b = 0; b < nt; b += EX_THREADS) {
    const uint32_t i = b + threadIdx.x;
    const uint64_t v = i < nt ? part[i] : 0;
    uint64_t tot;
    const uint64_t ex = ex_block_excl(v, wsum, &tot);
    const uint64_t c = carry;
    if (i < nt) part[i] = c + ex;
    __syncthreads();
    if (threadIdx.x == 0) carry = c + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) part[nt] = carry;
}

__global__ __launch_bounds__(256) void k_ex_scan_apply(const uint32_t* __restrict__ in, uint64_t n, const uint64_t* __restrict__ part,
                                                       uint32_t nt, uint64_t* __restrict__ out) {
  __shared__ uint64_t wsum[4];
  const uint64_t t = blockIdx.x, i0 = t * EX_TILE + (uint64_t)threadIdx.x * EX_PER_THREAD;
  uint32_t v[EX_PER_THREAD];
  uint64_t s = 0;
  for (uint32_t k = 0; k < EX_PER_THREAD; k++) { v[k] = i0 + k < n ? in[i0 + k] : 0u; s += v[k]; }
  uint64_t tot;
  uint64_t run = part[t] + ex_block_excl(s, wsum, &tot);
  for (uint32_t k = 0; k < EX_PER_THREAD; k++) {
    if (i0 + k < n) out[i0 + k] = run;
    run += v[k];
  }
  if (t == 0 && threadIdx.x == 0) out[n] = part[nt];
}

// ---- the row list: the USED directory slots in slot order -------------------------------------------------------------------
// The row set is what smatrix_row_info answers 1 for: every USED slot, a row whose block is not allocated yet (base 0) included.
__global__ __launch_bounds__(256) void k_ex_dir_count(const DirSlot* __restrict__ dir, uint32_t dir_size, uint32_t* __restrict__ tcnt) {
  __shared__ uint64_t wsum[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * EX_TILE + (uint64_t)threadIdx.x * EX_PER_THREAD;
  uint64_t c = 0;
  for (uint32_t k = 0; k < EX_PER_THREAD; k++) if (i0 + k < dir_size) c += dir[i0 + k].meta & META_USED;
  uint64_t tot;
  ex_block_excl(c, wsum, &tot);
  if (threadIdx.x == 0) tcnt[blockIdx.x] = (uint32_t)tot;
}

// items[toff[tile] + rank] = {row id, directory slot}, in slot order
__global__ __launch_bounds__(256) void k_ex_dir_write(const DirSlot* __restrict__ dir, uint32_t dir_size, const uint64_t* __restrict__ toff,
                                                      uint64_t* __restrict__ items) {
  __shared__ uint64_t wsum[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * EX_TILE + (uint64_t)threadIdx.x * EX_PER_THREAD;
  uint32_t used = 0;
  for (uint32_t k = 0; k < EX_PER_THREAD; k++) if (i0 + k < dir_size && (dir[i0 + k].meta & META_USED)) used |= 1u << k;
  uint64_t tot;
  uint64_t o = toff[blockIdx.x] + ex_block_excl((uint64_t)__popc(used), wsum, &tot);
  for (uint32_t k = 0; k < EX_PER_THREAD; k++)
    if (used >> k & 1u) items[o++] = (uint64_t)dir[i0 + k].x | ((i0 + k) << 32);
}

__global__ __launch_bounds__(256) void k_ex_rows(uint32_t n, const uint64_t* __restrict__ items, uint32_t* __restrict__ rows) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rows[i] = (uint32_t)items[i];
}

// ---- exact pair counts: the non-empty cells among the row's 2^lg cells (never the sub-counter lines or the at-home bitmap
// behind a big row's cells).  A wave per row up to GETROW_WAVE_MAX cells, as k_getrow; longer rows get cnt 0 here, are noted in
// big[] and counted by k_ex_count_big, a workgroup per GETROW_SEG segment, as k_getrow_big.
__global__ __launch_bounds__(256) void k_ex_count(const DirSlot* __restrict__ dir, uint8_t* arena, uint32_t n,
                                                  const uint64_t* __restrict__ items, uint32_t* __restrict__ cnt, uint32_t* big) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n; r += nwaves) {
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    const uint32_t size = s.z ? 1u << meta_lg(s.x) : 0u;
    if (size > GETROW_WAVE_MAX) {
      if (lane == 0) { cnt[r] = 0; big[1 + atomicAdd(&big[0], 1u)] = r; }
      continue;
    }
    const uint4* cells = s.z ? reinterpret_cast<const uint4*>(row_cells(arena, s.z)) : nullptr;
    uint32_t c = 0;
    for (uint32_t p = 2 * lane; p < size; p += 128) {
      const uint4 q = cells[p >> 1];
      c += ((q.x | q.y) != 0) + ((q.z | q.w) != 0);
    }
    for (uint32_t d = 32; d; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d);
    if (lane == 0) cnt[r] = c;
  }
}

__global__ __launch_bounds__(1024) void k_ex_count_big(const DirSlot* __restrict__ dir, uint8_t* arena,
                                                       const uint64_t* __restrict__ items, uint32_t* cnt, const uint32_t* big) {
  __shared__ uint32_t wsum[16];
  const uint32_t nbig = big[0], G = gridDim.x;
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t j = 0; j < nbig; j++) {
    const uint32_t r = big[1 + j];
    const uint4 s = *reinterpret_cast<const uint4*>(&dir[(uint32_t)(items[r] >> 32)]);
    const uint32_t size = 1u << meta_lg(s.x);                        // > GETROW_WAVE_MAX: a multiple of 2048
    const uint32_t seg = size < GETROW_SEG ? size : GETROW_SEG, nseg = size / seg;
    const uint4* cells = reinterpret_cast<const uint4*>(row_cells(arena, s.z));
    for (uint32_t g = (blockIdx.x + G - j % G) % G; g < nseg; g += G) {   // rows' segments rotate over the workgroups
      uint32_t c = 0;
      for (uint32_t p0 = g * seg; p0 < (g + 1) * seg; p0 += 2048) {
        const uint4 q = cells[(p0 >> 1) + threadIdx.x];
        c += ((q.x | q.y) != 0) + ((q.z | q.w) != 0);
      }
      for (uint32_t d = 32; d; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d);
      if (lane == 0) wsum[w] = c;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t i = 0; i < 16; i++) t += wsum[i];
        atomicAdd(&cnt[r], t);
      }
      __syncthreads();
    }
  }
}

// what k_getrow wrote must be what was counted: a difference under the matrix lock is a library bug (the host aborts)
__global__ __launch_bounds__(256) void k_ex_check(uint32_t n, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ got,
                                                  uint32_t* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && cnt[i] != got[i]) atomicOr(bad, 1u);
}

// ---- SORTED: the rows' pairs by column ---------------------------------------------------------------------------------------
// tiers: rows of 2..EX_LDS_SMALL pairs -> list 0, .. EX_LDS_MID -> list 1, longer -> list 2 (ctr[0..2] = lengths)
__global__ __launch_bounds__(256) void k_ex_classify(uint32_t n, const uint64_t* __restrict__ row_ptr, uint32_t* ctr,
                                                     uint32_t* __restrict__ l0, uint32_t* __restrict__ l1, uint32_t* __restrict__ l2) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t c = row_ptr[i + 1] - row_ptr[i];
  if (c < 2) return;
  if (c <= EX_LDS_SMALL) l0[atomicAdd(&ctr[0], 1u)] = (uint32_t)i;
  else if (c <= EX_LDS_MID) l1[atomicAdd(&ctr[1], 1u)] = (uint32_t)i;
  else l2[atomicAdd(&ctr[2], 1u)] = (uint32_t)i;
}

// bitonic sort of one row at a time in LDS, padded to a power of two with ~0 (a real pair equal to it -- column and value
// 0xffffffff -- is the same bits, so where it lands does not matter).  Order: column, then value (columns are unique in a row).
__device__ __forceinline__ uint64_t ex_colkey(uint64_t p) { return (p << 32) | (p >> 32); }

template <uint32_t T, uint32_t P>
__global__ __launch_bounds__(T) void k_ex_sort_lds(const uint32_t* __restrict__ list, const uint32_t* ctr, uint32_t which,
                                                   const uint64_t* __restrict__ row_ptr, uint64_t* pairs) {
  __shared__ uint64_t buf[P];
  const uint32_t nl = ctr[which];
  for (uint32_t li = blockIdx.x; li < nl; li += gridDim.x) {
    const uint32_t r = list[li];
    const uint64_t off = row_ptr[r];
    const uint32_t c = (uint32_t)(row_ptr[r + 1] - off);              // 2 .. P (the tier)
    uint32_t p = 2;
    while (p < c) p <<= 1;
    for (uint32_t i = threadIdx.x; i < p; i += T) buf[i] = i < c ? ex_colkey(pairs[off + i]) : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= p; k <<= 1) {
      for (uint32_t j = k >> 1; j; j >>= 1) {
        for (uint32_t i = threadIdx.x; i < p; i += T) {
          const uint32_t ij = i ^ j;
          if (ij > i) {
            const uint64_t a = buf[i], b = buf[ij];
            if (((i & k) == 0) == (a > b)) { buf[i] = b; buf[ij] = a; }
          }
        }
        __syncthreads();
      }
    }
    for (uint32_t i = threadIdx.x; i < c; i += T) pairs[off + i] = ex_colkey(buf[i]);
    __syncthreads();
  }
}

// ---- segmented LSD radix sort on the low word of 64-bit entries, 8 bits per pass, stable ------------------------------------
// nseg segments; segment b has cnt[b] entries at src + soff[b] (and goes to dst + doff[b]) and the tiles tstart[b] .. tstart[b+1]
// of EX_TILE entries (a tile never spans two segments).  Per pass:
//   k_ex_rs_hist     per tile, the 256 digit counts -> hist[256 * tstart[b] + digit * ntiles(b) + tile in b]
//   (scan of hist, u64: a segment's block of 256 * ntiles entries sums to its count, so inside the block the scan is the
//    position in the segment once the value at the block's start is taken off)
//   k_ex_rs_scatter  per tile, every entry to its place: block scan + entries of the same digit before it in the tile
__device__ inline uint32_t ex_seg_of(const uint32_t* tstart, uint32_t nseg, uint32_t t) {
  uint32_t lo = 0, hi = nseg;                                        // the last b with tstart[b] <= t
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (tstart[mid] <= t) lo = mid; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(256) void k_ex_rs_hist(const uint64_t* __restrict__ src, const uint64_t* __restrict__ soff,
                                                    const uint64_t* __restrict__ cnt, const uint32_t* __restrict__ tstart, uint32_t nseg,
                                                    uint32_t shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const uint32_t t = blockIdx.x, b = ex_seg_of(tstart, nseg, t), j = t - tstart[b], nt = tstart[b + 1] - tstart[b];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t e0 = (uint64_t)j * EX_TILE, e1 = min(cnt[b], e0 + EX_TILE);
  const uint64_t* s = src + soff[b];
  for (uint64_t e = e0 + threadIdx.x; e < e1; e += EX_THREADS) atomicAdd(&h[(uint32_t)(s[e] >> shift) & 255u], 1u);
  __syncthreads();
  hist[256ull * tstart[b] + (uint64_t)threadIdx.x * nt + j] = h[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_ex_rs_scatter(const uint64_t* __restrict__ src, const uint64_t* __restrict__ soff,
                                                       uint64_t* __restrict__ dst, const uint64_t* __restrict__ doff,
                                                       const uint64_t* __restrict__ cnt, const uint32_t* __restrict__ tstart, uint32_t nseg,
                                                       uint32_t shift, const uint64_t* __restrict__ hscan) {
  __shared__ uint64_t run[256];
  __shared__ uint32_t wcnt[4][256];
  const uint32_t t = blockIdx.x, b = ex_seg_of(tstart, nseg, t), j = t - tstart[b], nt = tstart[b + 1] - tstart[b];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1;
  const uint64_t blk = 256ull * tstart[b];
  run[threadIdx.x] = hscan[blk + (uint64_t)threadIdx.x * nt + j] - hscan[blk];
  for (uint32_t k = 0; k < 4; k++) wcnt[k][threadIdx.x] = 0;
  __syncthreads();
  const uint64_t e0 = (uint64_t)j * EX_TILE, e1 = min(cnt[b], e0 + EX_TILE);
  const uint64_t* s = src + soff[b];
  uint64_t* d = dst + doff[b];
  for (uint64_t base = e0; base < e1; base += EX_THREADS) {         // 256 entries at a time, in order: stable
    const uint64_t e = base + threadIdx.x;
    const bool valid = e < e1;
    const uint64_t v = valid ? s[e] : 0;
    const uint32_t dg = (uint32_t)(v >> shift) & 255u;
    uint64_t peers = __ballot(valid);                                // the lanes of this wave with the same digit
    for (uint32_t bit = 0; bit < 8; bit++) {
      const uint64_t m = __ballot(valid && (dg >> bit & 1u));
      peers &= (dg >> bit & 1u) ? m : ~m;
    }
    if (valid && (peers & lt) == 0) wcnt[w][dg] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint64_t pos = run[dg] + (uint32_t)__popcll(peers & lt);
      for (uint32_t k = 0; k < w; k++) pos += wcnt[k][dg];
      d[pos] = v;
    }
    __syncthreads();
    run[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
    for (uint32_t k = 0; k < 4; k++) wcnt[k][threadIdx.x] = 0;
    __syncthreads();
  }
}

// the long rows of the SORTED order: {pair offset, count} of every listed row
__global__ __launch_bounds__(256) void k_ex_big_info(uint32_t nl, const uint32_t* __restrict__ list, const uint64_t* __restrict__ row_ptr,
                                                     uint64_t* __restrict__ info) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nl) return;
  const uint32_t r = list[i];
  info[2 * i] = row_ptr[r];
  info[2 * i + 1] = row_ptr[r + 1] - row_ptr[r];
}
