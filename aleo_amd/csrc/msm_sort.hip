// msm_sort.hip — the scalar side of the Pippenger multi-scalar multiplications, shared by G1 (msm.hip) and G2 (g2.hip): everything msm_common.h
// declares — the plan and the table tiers' set capacities, signed balanced digits, the two-level counting sort into contiguous bucket runs of 4-byte
// point indices (bit 31 = negate), slices (whole buckets up to 2x the mean size, longer ones cut at the mean; sorted by length so a wave's lanes run equal trips), the slice metadata's way to the host.  None of it depends on the group.
#include <algorithm>
#include "ec.h"
#include "msm_common.h"

namespace aleo_mi355x {

// Window width of the fixed-base table, by size of the pinned set: the bucket reduction is latency-bound and its work
// grows with 2^(c-1), so small SRS (real Aleo circuits are 2^15..2^17) get narrower windows than the 2^20+ sets.
//   c = 20: 13 rows, 2^19 shared buckets   c = 17: 15 rows, 2^16 buckets   c = 16: 16 rows, 2^15 buckets
// (widths whose TOP window keeps >= 13 bits of the 253-bit scalar: c = 18 or 19 would leave it 1 or 6 bits, i.e. a
// handful of buckets holding n/2 points each)
MsmPlan make_plan(size_t n, int pre_c) {
  MsmPlan p;
  if (pre_c) {   // one shared bucket set: "W = 1 window of 2^(c-1) buckets" for everything after the sort
    // running-sum chunk: 2S dependent additions per lane pair vs. one more level of masked sums per halving; measured
    // best at 16 for 2^19 buckets (enough chunks to fill the chip) and 4 for 2^15..2^16 buckets (latency only)
    p.c = (uint32_t)pre_c; p.W = 1; p.B = 1u << (pre_c - 1); p.M = p.B; p.S = pre_c >= 20 ? 16 : 4;
    return p;
  }
  uint32_t lg = 0; while (((size_t)1 << (lg + 1)) <= n) ++lg;
  int c = (int)lg - 4; if (c < 2) c = 2; if (c > 16) c = 16;
  p.c = (uint32_t)c; p.W = (SCALAR_BITS + p.c - 1) / p.c; p.B = 1u << (p.c - 1); p.M = p.W * p.B;
  p.S = p.B >= 8 ? 8 : p.B;                  // buckets per running-sum chunk
  return p;
}

// ---- scalar access ----------------------------------------------------------------------------
template <bool MONT> __device__ __forceinline__ void load_scalar(const void* scalars, uint32_t i, uint32_t (&s)[8]) {
  const uint4* p = (const uint4*)scalars + 2 * (size_t)i;
  uint4 a = p[0], b = p[1];
  s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
  if constexpr (MONT) {   // KZG10::commit path: polynomial coefficients are Montgomery Fr -> canonical bigint
    Fr f; for (int k = 0; k < 8; ++k) f.v[k] = s[k];
    f = Fr::from_mont(f);
    for (int k = 0; k < 8; ++k) s[k] = f.v[k];
  }
}
// (window geometry: win_count / win_full / win_width / win_offset, msm_common.h)
template <int C, int W_IDX> __device__ __forceinline__ uint32_t window_raw(const uint32_t (&s)[8]) {
  constexpr int bit = win_offset(C, W_IDX), width = win_width(C, W_IDX), limb = bit >> 5, off = bit & 31;
  uint32_t v = 0;
  if constexpr (limb < 8) {
    v = s[limb] >> off;
    if constexpr (off + width > 32 && limb + 1 < 8) v |= s[limb + 1] << (32 - off);
  }
  return v & ((1u << width) - 1u);
}

// Calls f(w, bucket_index_0based, negate) for every non-zero signed digit of the scalar.
template <int C, int W_IDX, class F> __device__ __forceinline__ void for_each_digit(const uint32_t (&s)[8], uint32_t carry, F&& f) {
  constexpr int W = win_count(C);
  if constexpr (W_IDX < W) {
    constexpr int width = win_width(C, W_IDX);
    constexpr uint32_t B = 1u << (width - 1);
    uint32_t d = window_raw<C, W_IDX>(s) + carry;
    uint32_t neg = d > B ? 1u : 0u;
    uint32_t mag = neg ? (1u << width) - d : d;
    if (mag) f((uint32_t)W_IDX, mag - 1u, neg);
    for_each_digit<C, W_IDX + 1>(s, neg, f);
  }
}

// ---- counting sort of the n*W (bucket, point) pairs: two LDS-partitioned levels, no global atomics ----
// (A first version drew one global atomic per pair: 1.5 ms at 2^20 uniform and 4.9 ms on witness-like scalars,
//  whose 0/1 values pile onto a few counters — profiles/r01_v1_kernel_stats.csv.)
// Level 1 splits by (window, high bucket bits) into <= 2048 coarse bins: every block histograms a tile of 2048
// scalars in LDS, an exclusive scan over the [bin][block] count matrix gives each block a private output run per
// bin, and the scatter pass ranks items with LDS atomics.  Level 2 gives one block per coarse bin: an LDS
// histogram over the low 8 bucket bits yields the final per-bucket counts and positions.
static constexpr uint32_t PART_TILE = 2048;       // scalars per block in the level-1 passes (SegArgs::tile: 2048, or 4096 / 8192 for chains of >= 2^21 / 2^22 points — a block's run in a
                                                  // coarse bin is tile * windows / bins items of 8 bytes: ~100 bytes at 2048, and the PMC write counter showed 3.3 x the bytes stored)
static constexpr uint32_t MAX_COARSE = 2048;      // coarse bins of ONE set: W * (B >> LB) at c = 16 (the LDS tables of the level-1 passes)
static constexpr uint32_t MAX_COARSE_ALL = 4096;  // coarse bins of all sets of a chain (k_bin_parts: one block, 16 bins per lane): 32 sets at c = 16, 16 at c = 17

// PRE = the base set carries precomputed window multiples 2^(c*w) * P_i (fixed-base MSM, see msm_precompute):
// every window then feeds ONE shared set of buckets, and the point of digit w of scalar i is table entry w*n + i.
// Batched calls (several scalar vectors against ONE pinned set, msm_run's `k`): blockIdx.y is the vector ("set"); every
// set owns its own 2^(c-1) buckets, so its coarse bins are [set * CB, (set + 1) * CB) and everything after the sort sees
// k * 2^(c-1) buckets.  Only the table path batches (PRE), where one set is one window's worth of buckets.
template <int C, bool PRE> struct SortGeom {
  static constexpr uint32_t W = (SCALAR_BITS + C - 1) / C, B = 1u << (C - 1);
  static constexpr uint32_t LB = (C - 1) < 8 ? (C - 1) : 8;       // low bucket bits, sorted in level 2
  static constexpr uint32_t CB = B >> LB, NCB = PRE ? CB : W * CB;      // coarse bins of ONE set
  static_assert(NCB <= MAX_COARSE, "coarse bin table too small");
  __device__ static uint32_t bin(uint32_t w, uint32_t b) { return PRE ? (b >> LB) : w * CB + (b >> LB); }
};

// Workgroups are dealt round-robin over the eight XCDs (b and b + 8 share one, with its L2).  The level-1 scatter writes, for every coarse bin, the runs
// of consecutive TILES next to each other — a run is ~100 bytes, so a 128-byte line holds pieces of two tiles: with tile = workgroup the two pieces
// come from different L2s and reach HBM as partial lines.  Dealing consecutive tiles to workgroups of ONE XCD lets its L2 merge them.
#ifdef ALEO_NO_XCD_TILE
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t) { return b; }
#else
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t g) { return (g & 7u) ? b : (b & 7u) * (g >> 3) + (b >> 3); }
#endif
template <int C, bool MONT, bool PRE>
__global__ void __launch_bounds__(256) k_part_count(SegArgs segs, const uint8_t* inf, uint32_t* __restrict__ cnt) {
  using Gm = SortGeom<C, PRE>;
  __shared__ uint32_t h[MAX_COARSE];
  const uint32_t bx = xcd_tile(blockIdx.x, gridDim.x);
  const uint32_t n = segs.n[blockIdx.y], base = bx * segs.tile;
  if (base >= n) return;                                      // the grid is as wide as the longest segment
  for (uint32_t i = threadIdx.x; i < Gm::NCB; i += 256) h[i] = 0;
  __syncthreads();
  const char* scalars = segs.ptr[blockIdx.y]; const uint32_t off = segs.off[blockIdx.y], nblk = segs.ncol;
  cnt += (size_t)segs.set[blockIdx.y] * Gm::NCB * nblk + segs.col0[blockIdx.y];
  for (uint32_t q = 0; q < segs.tile / 256; ++q) {
    uint32_t i = base + q * 256 + threadIdx.x;
    if (i < n && !(inf && inf[off + i])) {
      uint32_t s[8]; load_scalar<MONT>(scalars, i, s);
      for_each_digit<C, 0>(s, 0u, [&](uint32_t w, uint32_t b, uint32_t) { atomicAdd(&h[Gm::bin(w, b)], 1u); });
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < Gm::NCB; i += 256) cnt[(size_t)i * nblk + bx] = h[i];     // [bin][tile]
}

// plain exclusive scan of uint32 (tiles of SCAN_TILE + one top block); position(i) = local[i] + blk[i / SCAN_TILE]
__global__ void __launch_bounds__(256) k_scan32_tiles(const uint32_t* __restrict__ in, uint32_t len, uint32_t* __restrict__ local, uint32_t* __restrict__ tile_tot) {
  __shared__ uint32_t wsum[4];
  uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * 8;
  uint32_t c[8], pre[8], run = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = (base + k < len) ? in[base + k] : 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) { pre[k] = run; run += c[k]; }
  uint32_t inc = run; int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t woff = 0; for (int k = 0; k < wv; ++k) woff += wsum[k];
  uint32_t excl = woff + inc - run;
#pragma unroll
  for (int k = 0; k < 8; ++k) if (base + k < len) local[base + k] = excl + pre[k];
  if (threadIdx.x == 255) tile_tot[blockIdx.x] = woff + inc;
}
__global__ void __launch_bounds__(256) k_scan32_top(const uint32_t* __restrict__ tile_tot, uint32_t ntiles, uint32_t* __restrict__ blk, uint32_t aux) {
  __shared__ uint32_t sh[256]; __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < ntiles; b0 += 256) {
    uint32_t i = b0 + threadIdx.x, v = i < ntiles ? tile_tot[i] : 0u;
    sh[threadIdx.x] = v; __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      uint32_t o = threadIdx.x >= (uint32_t)d ? sh[threadIdx.x - d] : 0u;
      __syncthreads(); sh[threadIdx.x] += o; __syncthreads();
    }
    uint32_t inc = sh[threadIdx.x], cr = carry;
    if (i < ntiles) blk[i] = cr + inc - v;
    __syncthreads();
    if (threadIdx.x == 255) carry = cr + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) { blk[ntiles] = carry; blk[ntiles + 1] = aux; }       // grand total; aux rides along (pick_rule's fill target)
}
__device__ __forceinline__ uint32_t scan32_at(const uint32_t* local, const uint32_t* blk, size_t i) { return local[i] + blk[i / SCAN_TILE]; }

template <int C, bool MONT, bool PRE>
__global__ void __launch_bounds__(256) k_part_scatter(SegArgs segs, const uint8_t* inf, uint32_t row_stride,
                                                      const uint32_t* __restrict__ off_local, const uint32_t* __restrict__ off_blk, uint2* __restrict__ items) {
  using Gm = SortGeom<C, PRE>;
  __shared__ uint32_t cur[MAX_COARSE];
  const uint32_t bx = xcd_tile(blockIdx.x, gridDim.x);
  const uint32_t n = segs.n[blockIdx.y], base = bx * segs.tile;
  if (base >= n) return;
  const char* scalars = segs.ptr[blockIdx.y]; const uint32_t off = segs.off[blockIdx.y], nblk = segs.ncol;
  const size_t row0 = (size_t)segs.set[blockIdx.y] * Gm::NCB; const uint32_t col = segs.col0[blockIdx.y] + bx;
  for (uint32_t i = threadIdx.x; i < Gm::NCB; i += 256) cur[i] = scan32_at(off_local, off_blk, (row0 + i) * nblk + col);
  __syncthreads();
  for (uint32_t q = 0; q < segs.tile / 256; ++q) {
    uint32_t i = base + q * 256 + threadIdx.x;
    if (i < n && !(inf && inf[off + i])) {
      uint32_t s[8]; load_scalar<MONT>(scalars, i, s);
      for_each_digit<C, 0>(s, 0u, [&](uint32_t w, uint32_t b, uint32_t neg) {
        uint32_t pos = atomicAdd(&cur[Gm::bin(w, b)], 1u);
        items[pos] = make_uint2((PRE ? w * row_stride + off + i : off + i) | (neg << 31), b & ((1u << Gm::LB) - 1u));
      });
    }
  }
}

// Level 2: the low LB bucket bits.  A coarse bin is cut into parts of BIN_PART items, one block each, so a bin that
// skewed scalars overfill (a fifth of a witness vector is the constant 1: one bucket, one bin) is sorted by many blocks
// instead of one (it was 1.5 ms of a 4.1 ms MSM at 2^22), and every part is ranked and staged in LDS so that the index
// stream is written in runs per bucket rather than as scattered 4-byte stores (64-byte write granules: 3.5 GB for 54 M
// stores at 2^22).  k_bin_hist adds the parts' LDS histograms into hist[]; k_bin_scatter claims each part's range
// of a bucket with one global atomic per (part, bucket).
static constexpr uint32_t BIN_PART = 4096;

__global__ void __launch_bounds__(256) k_bin_parts(const uint32_t* __restrict__ off_local, const uint32_t* __restrict__ off_blk, uint32_t nblk, uint32_t ncb,
                                                   uint32_t cnt_tiles, uint32_t* __restrict__ part_start) {
  __shared__ uint32_t wsum[4];
  const uint32_t tid = threadIdx.x; const int lane = tid & 63, wv = tid >> 6;
  constexpr int PER = MAX_COARSE_ALL / 256;
  uint32_t pre[PER], run = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const uint32_t bin = tid * PER + k; pre[k] = run;
    if (bin < ncb) {
      const uint32_t st = scan32_at(off_local, off_blk, (size_t)bin * nblk);
      const uint32_t en = (bin + 1 < ncb) ? scan32_at(off_local, off_blk, (size_t)(bin + 1) * nblk) : off_blk[cnt_tiles];
      run += (en - st + BIN_PART - 1) / BIN_PART;
    }
  }
  uint32_t inc = run;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t woff = 0; for (int k = 0; k < wv; ++k) woff += wsum[k];
  const uint32_t excl = woff + inc - run;
#pragma unroll
  for (int k = 0; k < PER; ++k) if (tid * PER + k < ncb) part_start[tid * PER + k] = excl + pre[k];
  if (tid == 255) part_start[ncb] = woff + inc;
}

struct BinPart { uint32_t bin, bstart, lo, hi; bool live; };
__device__ __forceinline__ BinPart locate_part(const uint32_t* __restrict__ off_local, const uint32_t* __restrict__ off_blk, uint32_t nblk, uint32_t ncb,
                                               uint32_t cnt_tiles, const uint32_t* __restrict__ part_start) {
  BinPart r; r.live = blockIdx.x < part_start[ncb];
  if (!r.live) return r;
  uint32_t lo = 0, hi = ncb;                           // largest bin with part_start[bin] <= block (empty bins share their successor's start)
  while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (part_start[mid] <= blockIdx.x) lo = mid; else hi = mid; }
  r.bin = lo;
  r.bstart = scan32_at(off_local, off_blk, (size_t)lo * nblk);
  const uint32_t bend = (lo + 1 < ncb) ? scan32_at(off_local, off_blk, (size_t)(lo + 1) * nblk) : off_blk[cnt_tiles];
  r.lo = r.bstart + (blockIdx.x - part_start[lo]) * BIN_PART;
  r.hi = r.lo + BIN_PART < bend ? r.lo + BIN_PART : bend;
  return r;
}

// Rank of each of the wave's keys in the block's LDS histogram.  The lanes that share the first lane's key go through one
// LDS atomic (the all-equal case of skewed scalars would otherwise serialise 4096 atomics on one address).
__device__ __forceinline__ uint32_t lds_rank(uint32_t* h, uint32_t key, bool valid, int lane) {
  const uint64_t vm = __ballot(valid);
  if (!vm) return 0u;
  const int first = __ffsll((unsigned long long)vm) - 1;
  const uint32_t k0 = __shfl(key, first);
  const bool grp = valid && key == k0;
  const uint64_t same = __ballot(grp);
  uint32_t base = 0;
  if (lane == first) base = atomicAdd(&h[k0], (uint32_t)__popcll(same));
  base = __shfl(base, first);
  if (grp) return base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
  return valid ? atomicAdd(&h[key], 1u) : 0u;
}

__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, int lane, int wv) {    // 256 threads; wsum: 4 words of LDS
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
  __syncthreads();
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t woff = 0; for (int k = 0; k < wv; ++k) woff += wsum[k];
  return woff + inc - v;
}

__global__ void __launch_bounds__(256) k_bin_hist(const uint2* __restrict__ items, const uint32_t* __restrict__ off_local, const uint32_t* __restrict__ off_blk,
                                                  uint32_t nblk, uint32_t ncb, uint32_t cnt_tiles, uint32_t LB, const uint32_t* __restrict__ part_start,
                                                  uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const uint32_t tid = threadIdx.x; const int lane = tid & 63;
  const BinPart P = locate_part(off_local, off_blk, nblk, ncb, cnt_tiles, part_start);
  if (!P.live) return;
  h[tid] = 0;
  __syncthreads();
#pragma unroll 4
  for (uint32_t u = 0; u < BIN_PART / 256; ++u) {
    const uint32_t i = P.lo + u * 256 + tid; const bool valid = i < P.hi;
    const uint32_t key = valid ? items[i].y : 0u;
    (void)lds_rank(h, key, valid, lane);
  }
  __syncthreads();
  const uint32_t v = h[tid];
  if (v && tid < (1u << LB)) atomicAdd(&hist[((size_t)P.bin << LB) + tid], v);
}

__global__ void __launch_bounds__(256) k_bin_scatter(const uint2* __restrict__ items, const uint32_t* __restrict__ off_local, const uint32_t* __restrict__ off_blk,
                                                     uint32_t nblk, uint32_t ncb, uint32_t cnt_tiles, uint32_t LB, const uint32_t* __restrict__ part_start,
                                                     const uint32_t* __restrict__ hist, uint32_t* __restrict__ cursor, uint32_t* __restrict__ sorted) {
  __shared__ uint32_t h[256], gb[256], wsum[4];
  __shared__ uint32_t l_idx[BIN_PART], l_dst[BIN_PART];
  const uint32_t tid = threadIdx.x; const int lane = tid & 63, wv = tid >> 6;
  const BinPart P = locate_part(off_local, off_blk, nblk, ncb, cnt_tiles, part_start);
  if (!P.live) return;
  h[tid] = 0;
  __syncthreads();
  constexpr int U = BIN_PART / 256;
  uint2 it[U]; uint32_t rank[U];
#pragma unroll
  for (int u = 0; u < U; ++u) { const uint32_t i = P.lo + u * 256 + tid; it[u] = i < P.hi ? items[i] : make_uint2(0u, 0xffffffffu); }
#pragma unroll
  for (int u = 0; u < U; ++u) rank[u] = lds_rank(h, it[u].y, it[u].y != 0xffffffffu, lane);
  __syncthreads();
  const uint32_t v = h[tid];                                                 // this part's count of bucket tid
  const uint32_t loff = block_excl_scan(v, wsum, lane, wv);                  // its offset inside the part's sorted tile
  const uint32_t g = tid < (1u << LB) ? hist[((size_t)P.bin << LB) + tid] : 0u;
  const uint32_t gexcl = block_excl_scan(g, wsum, lane, wv);                 // the bucket's offset inside the bin
  gb[tid] = P.bstart + gexcl + (v ? atomicAdd(&cursor[((size_t)P.bin << LB) + tid], v) : 0u);
  __syncthreads();
  h[tid] = loff;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < U; ++u) if (it[u].y != 0xffffffffu) {
    const uint32_t lp = h[it[u].y] + rank[u];
    l_idx[lp] = it[u].x; l_dst[lp] = gb[it[u].y] + rank[u];
  }
  __syncthreads();
  const uint32_t cnt = P.hi - P.lo;
  for (uint32_t q = tid; q < cnt; q += 256) sorted[l_dst[q]] = l_idx[q];
}

// ---- exclusive scan of (count, slices) over the M buckets --------------------------------------
// scan_local[g] = prefix inside the 2048-bucket tile; scan_blk[tile] = prefix of the tiles.  meta[0] = total
// slices, meta[1] = max slices of one bucket, meta[2] = total pairs.
// Slice sizing.  A bucket of <= T_SINGLE points is one slice (one lane); larger buckets are cut into slices of
// <= T_SPLIT.  One lane needs ~10-20 us per mixed addition, so the longest slice bounds the kernel from below: 128-point
// slices (tried) put a 2.7 ms floor under a 2.4 ms kernel, because the top window of a 253-bit scalar only has 13 bits
// and its 4779 buckets hold ~300 points each.  64/32 keeps the floor at about half the kernel time.
// Sparse inputs (witness-like scalars, small n) use 32/32 so that the accumulation still fills every SIMD.
// The same pass counts the slice LENGTHS (len_count, the histogram k_slice_order sorts by): a bucket of cnt points cut into m slices has cnt mod m slices of
// ceil(cnt / m) points and the rest of floor(cnt / m) — slice_len() telescopes to cnt and every term is one of the two — so a bucket is two LDS increments and a
// block one global add per length it met.  Multi-slice buckets are ranked by the block's scan as well: a block claims its stretch of either list with ONE global
// atomic (one atomic per bucket before: the 4779 top-window buckets of a 2^20-point call sit in three tiles and drew theirs from one address).
__global__ void __launch_bounds__(256) k_scan_tiles(const uint32_t* hist, uint32_t M, const uint32_t* total_pairs, uint2* scan_local, uint2* tile_tot, uint32_t* meta,
                                                    uint32_t* __restrict__ heavy, uint32_t* __restrict__ len_count) {
  __shared__ uint2 wsum[4]; __shared__ uint32_t wlist[4], claim[2], lh[MAX_SLICE + 1];
  for (uint32_t i = threadIdx.x; i <= MAX_SLICE; i += 256) lh[i] = 0;
  __syncthreads();
  uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * 8;
  const SliceRule rule = pick_rule(total_pairs, M);
  uint32_t c[8], ms[8]; uint32_t mx = 0, mxc = 0, lists = 0;      // lists: this lane's common-list buckets | super-list buckets << 16 (a tile has <= 2048 of either)
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = (base + k < M) ? hist[base + k] : 0u;
  uint2 pre[8]; uint2 run = make_uint2(0, 0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    pre[k] = run; const uint32_t m = ms[k] = slices_of(c[k], rule); run.x += c[k]; run.y += m; mx = mx > m ? mx : m;
    if (m) { const uint32_t q = c[k] / m, r = c[k] - q * m; if (r) atomicAdd(&lh[q + 1], r); atomicAdd(&lh[q], m - r); }
    // multi-slice buckets are the only work of the slice tree; the few with > 16 slices (skewed scalars) get their own
    // list so that the launch width of the common list stays at 8 pairs per bucket
    if (m > 16) lists += 1u << 16;
    else if (m > 1) { lists += 1u; mxc = mxc > m ? mxc : m; }
  }
  // wave inclusive scan of the per-thread totals
  uint2 inc = run; uint32_t linc = lists; int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t ox = __shfl_up(inc.x, d), oy = __shfl_up(inc.y, d), ol = __shfl_up(linc, d);
    if (lane >= d) { inc.x += ox; inc.y += oy; linc += ol; }
  }
  if (lane == 63) { wsum[wv] = inc; wlist[wv] = linc; }
  __syncthreads();
  uint2 woff = make_uint2(0, 0); uint32_t loff = 0;
  for (int k = 0; k < wv; ++k) { woff.x += wsum[k].x; woff.y += wsum[k].y; loff += wlist[k]; }
  uint2 excl = make_uint2(woff.x + inc.x - run.x, woff.y + inc.y - run.y);
#pragma unroll
  for (int k = 0; k < 8; ++k) if (base + k < M) scan_local[base + k] = make_uint2(excl.x + pre[k].x, excl.y + pre[k].y);
  if (threadIdx.x == 255) {
    tile_tot[blockIdx.x] = make_uint2(woff.x + inc.x, woff.y + inc.y);
    const uint32_t tot = loff + linc, nc = tot & 0xffffu, ns = tot >> 16;
    claim[0] = nc ? atomicAdd(&meta[3], nc) : 0u; claim[1] = ns ? atomicAdd(&meta[5], ns) : 0u;
  }
  __syncthreads();
  if (lists) {
    const uint32_t lexcl = loff + linc - lists; uint32_t qc = claim[0] + (lexcl & 0xffffu), qs = claim[1] + (lexcl >> 16);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (ms[k] > 16) { const uint32_t q = qs++; if (q < SUPER_CAP) heavy[M + 2048 + q] = base + k; else heavy[atomicAdd(&meta[3], 1u)] = base + k; }      // list full: over to the common one
      else if (ms[k] > 1) heavy[qc++] = base + k;
    }
  }
  for (uint32_t i = threadIdx.x; i <= MAX_SLICE; i += 256) if (lh[i]) atomicAdd(&len_count[i], lh[i]);
  for (int d = 32; d >= 1; d >>= 1) { uint32_t o = __shfl_xor(mx, d), oc = __shfl_xor(mxc, d); mx = mx > o ? mx : o; mxc = mxc > oc ? mxc : oc; }
  if (lane == 0 && mx) atomicMax(&meta[1], mx);
  if (lane == 0 && mxc > 1) atomicMax(&meta[6], mxc);       // most slices of a common-list bucket: the depth of ITS tree (msm_run)
}

// host_meta (device pointer of the slot's mapped pinned buffer): meta[0..7] go there followed by the call's sequence number at word 8, so the host reads the
// slice counts by polling — no copy on a side stream, no event on the launch stream (an event record between two kernels costs ~6 us of idle GPU on this runtime)
__global__ void __launch_bounds__(256) k_scan_top(const uint2* tile_tot, uint32_t ntiles, uint2* scan_blk, uint32_t* meta, volatile uint32_t* host_meta, uint32_t seq) {
  // one block; ntiles <= a few thousand: serial chunks of 256 with a running offset
  __shared__ uint2 sh[256]; __shared__ uint2 carry;
  if (threadIdx.x == 0) carry = make_uint2(0, 0);
  __syncthreads();
  for (uint32_t b0 = 0; b0 < ntiles; b0 += 256) {
    uint32_t i = b0 + threadIdx.x;
    uint2 v = i < ntiles ? tile_tot[i] : make_uint2(0, 0);
    sh[threadIdx.x] = v; __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      uint2 o = threadIdx.x >= (uint32_t)d ? sh[threadIdx.x - d] : make_uint2(0, 0);
      __syncthreads();
      sh[threadIdx.x].x += o.x; sh[threadIdx.x].y += o.y; __syncthreads();
    }
    uint2 inc = sh[threadIdx.x]; uint2 cr = carry;
    if (i < ntiles) scan_blk[i] = make_uint2(cr.x + inc.x - v.x, cr.y + inc.y - v.y);
    __syncthreads();
    if (threadIdx.x == 255) { carry.x = cr.x + inc.x; carry.y = cr.y + inc.y; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    meta[0] = carry.y; meta[2] = carry.x;
    if (host_meta) {
      host_meta[0] = carry.y; host_meta[2] = carry.x;
      for (int i : {1, 3, 4, 5, 6, 7}) host_meta[i] = meta[i];      // written by k_scan_tiles (the launch before this one)
      __threadfence_system();
      host_meta[8] = seq;
    }
  }
}

// ---- slice ordering: lanes of one wave should run the same trip count --------------------------------
// Slices are at most 512 points long; bucket sizes are Poisson, so slice lengths vary 2:1 inside a wave if
// taken in bucket order (measured: 31 % of the accumulation's lanes idle).  A counting sort by length (longest
// first) costs ONE launch behind the bucket scan, which has left the length counts (len_count) behind:
//   a block takes ORDER_BATCH consecutive slice ids, 8 per lane.  It finds the buckets of its first and its last slice with two rounds of loads (every lane
//   looks at tile prefixes, then at 8 buckets of the one tile), marks the first slice of every non-empty bucket in between in LDS and spreads the marks with
//   a running maximum: sid -> bucket (task_g) without a search per slice (a binary search over all M buckets was 19 dependent rounds of two global loads
//   per lane), and a bucket of thousands of slices (witness-like scalars) is spread over the lanes of as many blocks as it has batches.  Where the stretch of
//   buckets is longer than STRETCH_CAP (sparse input: mostly empty buckets, few slices, few blocks) the lanes binary-search that stretch instead (>= 13 dependent rounds).
//   Lengths are ranked in an LDS histogram with wave-aggregated atomics (lds_rank) and a block draws one global atomic per length it holds.
// (len_start[l] = number of slices longer than l is recomputed by every block from the ~513 length counts — a single-block launch of its own, k_len_starts,
//  cost ~6 us per chain at the sizes of real circuits)
// FUSED (<= 512 scan tiles — every chain of a prover round): the exclusive scan of the tile totals, otherwise the single-block launch k_scan_top
// (~5-8 us per chain at real-circuit sizes), runs in every block's prologue over LDS; block 0 also leaves scan_blk, the totals and the host's copy of the slice
// metadata behind for the kernels that follow (the accumulation, the trees and the reduction read them from memory as before).
// The grid comes from slice_bound(), about twice the real slice count: a block beyond it leaves as soon as it knows the count, before the set-up of the ordering
// (length offsets, histogram, marks) — at once where k_scan_top has left the count in meta[0]; FUSED blocks must take the prologue's scan (two loads, an LDS scan
// over <= 512 tile totals, two barriers) to learn it.
static constexpr uint32_t FUSED_TILES = 512;
static constexpr uint32_t ORDER_BATCH = 2048;     // slices per block: 8 per lane
static constexpr uint32_t STRETCH_CAP = 8192;     // buckets a block walks to mark its slices' owners (32 per lane)
template <bool FUSED>
__global__ void __launch_bounds__(256) k_slice_order(const uint32_t* __restrict__ hist, const uint2* __restrict__ scan_local, uint2* scan_blk, const uint2* __restrict__ tile_tot,
                                                     uint32_t ntiles, const uint32_t* __restrict__ total_pairs, uint32_t M, uint32_t* meta, uint32_t* __restrict__ task_g,
                                                     const uint32_t* __restrict__ len_count, uint32_t* __restrict__ len_cursor, uint32_t* __restrict__ order,
                                                     volatile uint32_t* host_meta, uint32_t seq) {
  __shared__ uint2 sblk[FUSED ? FUSED_TILES : 1]; __shared__ uint2 wtot2[4];
  __shared__ uint32_t s_total, s_tile[2], s_loc[2], wtot[4];
  __shared__ __attribute__((aligned(16))) uint32_t mark[ORDER_BATCH];
  __shared__ uint32_t h[MAX_SLICE + 1], base[MAX_SLICE + 1], len_start[MAX_SLICE + 2];
  const uint32_t tid = threadIdx.x; const int lane = tid & 63, wv = tid >> 6;
  uint32_t total;
  if constexpr (FUSED) {
    const uint2 v0 = 2 * tid < ntiles ? tile_tot[2 * tid] : make_uint2(0u, 0u), v1 = 2 * tid + 1 < ntiles ? tile_tot[2 * tid + 1] : make_uint2(0u, 0u);
    uint2 inc = make_uint2(v0.x + v1.x, v0.y + v1.y);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t ox = __shfl_up(inc.x, d), oy = __shfl_up(inc.y, d); if (lane >= d) { inc.x += ox; inc.y += oy; } }
    if (lane == 63) wtot2[wv] = inc;
    __syncthreads();
    uint2 off = make_uint2(0u, 0u); for (int k = 0; k < wv; ++k) { off.x += wtot2[k].x; off.y += wtot2[k].y; }
    const uint2 excl = make_uint2(off.x + inc.x - v0.x - v1.x, off.y + inc.y - v0.y - v1.y);
    if (2 * tid < FUSED_TILES) sblk[2 * tid] = excl;
    if (2 * tid + 1 < FUSED_TILES) sblk[2 * tid + 1] = make_uint2(excl.x + v0.x, excl.y + v0.y);
    if (tid == 255) s_total = off.y + inc.y;
    if (blockIdx.x == 0) {
      if (2 * tid < ntiles) scan_blk[2 * tid] = excl;
      if (2 * tid + 1 < ntiles) scan_blk[2 * tid + 1] = make_uint2(excl.x + v0.x, excl.y + v0.y);
      if (tid == 255) {
        const uint32_t slices = off.y + inc.y, pairs = off.x + inc.x;
        meta[0] = slices; meta[2] = pairs;
        if (host_meta) {
          host_meta[0] = slices; host_meta[2] = pairs;
          for (int i : {1, 3, 4, 5, 6, 7}) host_meta[i] = meta[i];      // written by k_scan_tiles (the launch before this one)
          __threadfence_system();
          host_meta[8] = seq;
        }
      }
    }
    __syncthreads();
    total = s_total;
  } else {
    total = meta[0];
  }
  const uint32_t s0 = blockIdx.x * ORDER_BATCH;
  if (s0 >= total) return;
  const uint32_t s1 = (total - s0 < ORDER_BATCH ? total : s0 + ORDER_BATCH) - 1;      // this block's slices: s0 .. s1
  auto blk_y = [&](uint32_t T) -> uint32_t { if constexpr (FUSED) return sblk[T].y; else return scan_blk[T].y; };
  auto first_slice = [&](uint32_t g) -> uint32_t { return scan_local[g].y + blk_y(g / SCAN_TILE); };

  {                                                        // suffix sums of len_count: lane t owns the lengths PER t .. PER t + PER - 1
    constexpr uint32_t PER = (MAX_SLICE + 1 + 255) / 256;
    uint32_t cnt[PER], tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) { const uint32_t l = PER * tid + k; cnt[k] = l <= MAX_SLICE ? len_count[l] : 0u; tot += cnt[k]; }
    uint32_t inc = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_down(inc, d); if (lane + d < 64) inc += o; }      // inclusive suffix sum inside the wave
    if (lane == 0) wtot[wv] = inc;
    __syncthreads();
    uint32_t run = inc - tot; for (int k = wv + 1; k < 4; ++k) run += wtot[k];      // slices longer than this lane's last length
#pragma unroll
    for (uint32_t k = PER; k-- > 0;) { const uint32_t l = PER * tid + k; if (l <= MAX_SLICE) len_start[l] = run; run += cnt[k]; }
  }
  for (uint32_t i = tid; i <= MAX_SLICE; i += 256) h[i] = 0;
  for (uint32_t i = tid; i < ORDER_BATCH; i += 256) mark[i] = 0;

  // the buckets of slices s0 and s1: the largest g with first_slice(g) <= s (empty buckets share their successor's first slice) — first its tile, then its place in the tile
  for (uint32_t T = tid; T < ntiles; T += 256) {
    const uint32_t y = blk_y(T), yn = T + 1 < ntiles ? blk_y(T + 1) : 0xffffffffu;
    if (y <= s0 && yn > s0) s_tile[0] = T;
    if (y <= s1 && yn > s1) s_tile[1] = T;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t s = j ? s1 : s0, T = s_tile[j], by = blk_y(T), e0 = T * SCAN_TILE + tid * 8;
    uint32_t v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = (e0 + k < M && tid * 8 + k < SCAN_TILE) ? scan_local[e0 + k].y + by : 0xffffffffu;      // (the next tile starts beyond s)
#pragma unroll
    for (int k = 0; k < 8; ++k) if (v[k] <= s && v[k + 1] > s) s_loc[j] = e0 + k;
  }
  __syncthreads();
  const uint32_t g_lo = s_loc[0], g_hi = s_loc[1];
  const bool walk = g_hi - g_lo < STRETCH_CAP;
  uint32_t gq[8];
  if (walk) {
#pragma unroll 4
    for (uint32_t g = g_lo + tid; g <= g_hi; g += 256)
      if (hist[g]) { const uint32_t slot = g == g_lo ? 0u : first_slice(g) - s0; if (slot < ORDER_BATCH) mark[slot] = g + 1u; }      // first slices of distinct non-empty buckets differ; those behind g_lo's lie in (s0, s1]
    __syncthreads();
    const uint4 m0 = ((const uint4*)mark)[2 * tid], m1 = ((const uint4*)mark)[2 * tid + 1];
    gq[0] = m0.x; gq[1] = m0.y; gq[2] = m0.z; gq[3] = m0.w; gq[4] = m1.x; gq[5] = m1.y; gq[6] = m1.z; gq[7] = m1.w;
#pragma unroll
    for (int k = 1; k < 8; ++k) gq[k] = gq[k] > gq[k - 1] ? gq[k] : gq[k - 1];
    uint32_t inc = gq[7];                                  // running maximum over the lanes before this one
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if (lane >= d && o > inc) inc = o; }
    if (lane == 63) wtot[wv] = inc;
    uint32_t before = __shfl_up(inc, 1); if (lane == 0) before = 0;
    __syncthreads();
    for (int k = 0; k < wv; ++k) before = wtot[k] > before ? wtot[k] : before;
#pragma unroll
    for (int k = 0; k < 8; ++k) gq[k] = (gq[k] > before ? gq[k] : before) - 1u;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t sid = s0 + tid * 8 + k;
      uint32_t lo = g_lo, hi = g_hi;
      if (sid <= s1) while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (first_slice(mid) <= sid) lo = mid; else hi = mid - 1; }
      gq[k] = lo;
    }
  }
  const SliceRule rule = pick_rule(total_pairs, M);
  uint32_t len[8], rank[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t sid = s0 + tid * 8 + k; len[k] = 0;
    if (sid <= s1) { const uint32_t g = gq[k], cnt = hist[g]; len[k] = slice_len(cnt, slices_of(cnt, rule), sid - first_slice(g)); }
  }
  if (s0 + tid * 8 + 7 <= s1) {
    uint4* dst = (uint4*)(task_g + s0 + tid * 8);
    dst[0] = make_uint4(gq[0], gq[1], gq[2], gq[3]); dst[1] = make_uint4(gq[4], gq[5], gq[6], gq[7]);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) if (s0 + tid * 8 + k <= s1) task_g[s0 + tid * 8 + k] = gq[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) rank[k] = lds_rank(h, len[k], s0 + tid * 8 + k <= s1, lane);
  __syncthreads();
  for (uint32_t i = tid; i <= MAX_SLICE; i += 256)
    if (h[i]) base[i] = len_start[i] + atomicAdd(&len_cursor[i], h[i]);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) if (s0 + tid * 8 + k <= s1) order[base[len[k]] + rank[k]] = s0 + tid * 8 + k;
}

// ---- dispatch on the window width ---------------------------------------------------------------
struct SortArgs { SegArgs segs; const uint8_t* inf; uint32_t nblk_x, row_stride; uint32_t* cnt; uint32_t* off_local; uint32_t* off_blk; uint2* items; };
template <int C, bool MONT, bool PRE> static void launch_sort_c(const SortArgs& a, int phase, hipStream_t s) {
  if (phase == 0) hipLaunchKernelGGL((k_part_count<C, MONT, PRE>), dim3(a.nblk_x, a.segs.nseg), dim3(256), 0, s, a.segs, a.inf, a.cnt);
  else hipLaunchKernelGGL((k_part_scatter<C, MONT, PRE>), dim3(a.nblk_x, a.segs.nseg), dim3(256), 0, s, a.segs, a.inf, a.row_stride, a.off_local, a.off_blk, a.items);
}
template <bool MONT> static void launch_sort(int c, bool pre, const SortArgs& a, int phase, hipStream_t s) {
#define CASE(C, PRE) case C: launch_sort_c<C, MONT, PRE>(a, phase, s); break;
  if (pre) switch (c) { CASE(13, true) CASE(16, true) CASE(17, true) CASE(20, true) }
  else switch (c) {
    CASE(2, false) CASE(3, false) CASE(4, false) CASE(5, false) CASE(6, false) CASE(7, false) CASE(8, false) CASE(9, false) CASE(10, false) CASE(11, false) CASE(12, false)
    CASE(13, false) CASE(14, false) CASE(15, false) CASE(16, false)
  }
#undef CASE
}
static bool sort_has_case(int c, bool pre) { return pre ? (c == 13 || c == 16 || c == 17 || c == 20) : (c >= 2 && c <= 16); }      // the widths launch_sort instantiates

// lg of the slice count pick_rule() aims for when it cuts buckets to fill the chip (2^17 = 2 waves per SIMD: measured equal to 2^18 on uniform input, 4 % better on witness-like scalars)
static constexpr uint32_t FILL_SHIFT = 17;

// Upper bound of the slice count the device will compute (k_scan_tiles / pick_rule), from what the host knows: `pairs_max`
// (>= the real pair count) and the bucket count M.  Every non-empty bucket is at least one slice; a bucket cut at `split`
// adds cnt / split more.  pick_rule's split is >= 8 (4 below 2^18 pairs) always; it is >= pairs / 2^FILL_SHIFT / 1.125 while the fill rule decides and
// >= the mean bucket size while the mean rule decides, until the 256-point cap takes over.  The grids of the slice kernels
// and of the accumulation are sized by this bound, so no launch waits for the device's own count to reach the host.
static size_t slice_bound(size_t pairs_max, size_t M) {
  const size_t nonempty = M < pairs_max ? M : pairs_max;
  const size_t fill_cap = ((size_t)9 << FILL_SHIFT) >> 3;          // pairs / fill < 1.125 * 2^FILL_SHIFT while the fill rule decides
  const size_t by_rule = M + fill_cap + pairs_max / 256;
  const size_t by_min = pairs_max / 4;          // pick_rule's shortest split (the device decides 4 or 8 from its own pair count, which may be far below pairs_max)
  return nonempty + (by_min < by_rule ? by_min : by_rule) + 1;
}

const PinnedBases::PreTable* msm_tier(const PinnedBases& pb, size_t n) { for (const auto& t : pb.tab) if (t.d && n >= t.min_n && n <= t.cover) return &t; return nullptr; }
static uint32_t sets_of_window(int c) {
  const uint32_t B = 1u << (c - 1), LB = 8, cb = B >> LB, cap = MAX_COARSE_ALL / (cb ? cb : 1);
  return cap < MAX_SETS ? (cap ? cap : 1) : MAX_SETS;
}
uint32_t msm_max_sets(const PinnedBases& pb, size_t n) { const PinnedBases::PreTable* t = msm_tier(pb, n); return t ? sets_of_window(t->c) : 1; }
uint32_t msm_range_sets(const PinnedBases& pb) { return sets_of_window(pb.range.c); }

// Everything behind the bucket histogram: bucket scan (+ slice lengths, multi-slice lists), top scan (a launch of its own, or fused into the next one), slice ordering.
// ev (optional) is recorded behind the scan, in front of the slice ordering.
static int32_t launch_slice_stage(const SortPhase& sp, uint2* tile_tot, const uint32_t* total_pairs, uint32_t* host_meta, bool fuse_top, hipEvent_t ev, hipStream_t s) {
  const uint32_t M = sp.M, ntiles = (M + SCAN_TILE - 1) / SCAN_TILE;
  uint32_t* len_count = sp.meta + 16; uint32_t* len_cursor = len_count + MAX_SLICE + 1;   // zeroed with hist/meta
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(256), 0, s, sp.hist, M, total_pairs, sp.scan_local, tile_tot, sp.meta, sp.heavy, len_count);
  if (!fuse_top) hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(256), 0, s, tile_tot, ntiles, sp.scan_blk, sp.meta, (volatile uint32_t*)host_meta, sp.meta_seq);
  HIPCHK(hipGetLastError());
  if (ev) HIPCHK(hipEventRecord(ev, s));
  const uint32_t blocks = (uint32_t)((sp.slices_max + ORDER_BATCH - 1) / ORDER_BATCH);
  hipLaunchKernelGGL(fuse_top ? k_slice_order<true> : k_slice_order<false>, dim3(blocks), dim3(256), 0, s, sp.hist, sp.scan_local, sp.scan_blk, (const uint2*)tile_tot, ntiles,
                     total_pairs, M, sp.meta, sp.task_g, len_count, len_cursor, sp.order, fuse_top ? (volatile uint32_t*)host_meta : nullptr, fuse_top ? sp.meta_seq : 0u);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

int32_t msm_sort_phase(Ctx* c, SegArgs& segs, size_t pts, bool mont, const uint8_t* d_inf, uint32_t row_stride,
                       const MsmPlan& P, bool pre, hipStream_t s, SortPhase* out, bool lean, uint32_t tile) {
  SortPhase& sp = *out; sp.P = P;
  // columns of the level-1 count matrix: the blocks of a set's segments side by side; every row is as wide as the widest set
  uint32_t width[MAX_SETS] = {}, nblk_x = 0;
  segs.tile = tile ? tile : pts >= ((size_t)1 << 22) ? 8192u : (pts >= ((size_t)1 << 21) ? 4096u : PART_TILE);      // (tile != 0: selftest_sort_pairs alone)
  for (uint32_t q = 0; q < segs.nseg; ++q) {
    const uint32_t nb = (segs.n[q] + segs.tile - 1) / segs.tile, st = pre ? segs.set[q] : 0;
    segs.col0[q] = width[st]; width[st] += nb; nblk_x = nb > nblk_x ? nb : nblk_x;
  }
  uint32_t nblk = 1; for (uint32_t w : width) nblk = w > nblk ? w : nblk;
  segs.ncol = nblk;
  sp.digitsW = (SCALAR_BITS + P.c - 1) / P.c;
  const uint32_t M = sp.M = P.M, ntiles = (M + SCAN_TILE - 1) / SCAN_TILE;
  const size_t pairs_max = sp.pairs_max = pts * (size_t)sp.digitsW;
  if (pairs_max >= (1ull << 32)) { g_last_error = "msm: n * windows exceeds 2^32 (shard the MSM across GPUs)"; return ALEO_MI355X_ERR_BAD_ARG; }
  const size_t slices_max = sp.slices_max = slice_bound(pairs_max, M);
  sp.slice_blocks = (uint32_t)((slices_max + 255) / 256);
  int32_t rc;
  // hist | heavy list | meta | super list | level-2 cursors | the level-1 count matrix live in one allocation, zeroed by ONE fill
  const size_t hist_words = 3 * (size_t)M + 2048 + SUPER_CAP;
  if ((rc = c->scan_local.reserve((size_t)M * 8))) return rc;
  if ((rc = c->scan_blk.reserve(2 * (size_t)ntiles * 8 + 64))) return rc;
  if ((rc = c->sorted.reserve(pairs_max * 4))) return rc;
  const uint32_t LB = (P.c - 1) < 8 ? (P.c - 1) : 8, ncb = P.W * (P.B >> LB);      // coarse bins of all sets / windows
  const size_t cnt_len = (size_t)ncb * nblk;
  if (ncb > MAX_COARSE_ALL || cnt_len >= (1ull << 32)) { g_last_error = "msm: partition table too large"; return ALEO_MI355X_ERR_BAD_ARG; }
  const uint32_t cnt_tiles = (uint32_t)((cnt_len + SCAN_TILE - 1) / SCAN_TILE);
  if ((rc = c->hist.reserve((hist_words + cnt_len) * 4))) return rc;
  if ((rc = c->part_cnt.reserve((cnt_len + 2 * (size_t)cnt_tiles + 16 + MAX_COARSE_ALL) * 4))) return rc;     // off_local | tile_tot | off_blk | part_start
  if ((rc = c->part_items.reserve(pairs_max * 8))) return rc;
  if ((rc = c->task_g.reserve(2 * slices_max * 4))) return rc;     // task_g | order
  if ((rc = ensure_host_pinned(c, 64))) return rc;

  uint32_t* hist = sp.hist = c->hist.as<uint32_t>(); uint32_t* heavy = sp.heavy = hist + M; uint32_t* meta = sp.meta = heavy + M;     // heavy: <= M bucket ids
  sp.super_list = heavy + M + 2048;
  uint32_t* bin_cursor = hist + 2 * (size_t)M + 2048 + SUPER_CAP;
  uint2* scan_local = sp.scan_local = c->scan_local.as<uint2>();
  uint2* tile_tot = c->scan_blk.as<uint2>(); uint2* scan_blk = sp.scan_blk = tile_tot + ntiles;
  uint32_t* sorted = sp.sorted = c->sorted.as<uint32_t>(); uint32_t* task_g = sp.task_g = c->task_g.as<uint32_t>(); uint32_t* order = sp.order = task_g + slices_max;

  if (!lean) HIPCHK(hipEventRecord(c->ev[0], s));
  sp.zero_bytes = (hist_words + cnt_len) * 4;
  const bool cleared_ahead = c->hist_clean >= sp.zero_bytes && c->hist_clean_stream == s && c->hist_clean_ptr == (void*)hist;      // the previous chain on this stream left it clean (msm.hip msm_reduce_queue)
  c->hist_clean = 0;                                        // (about to be dirtied)
  if (!cleared_ahead) HIPCHK(hipMemsetAsync(hist, 0, sp.zero_bytes, s));          // (count matrix: columns no block of a set owns, and tiles past a segment's end, count zero)
  SortArgs sa;
  sa.segs = segs; sa.nblk_x = nblk_x ? nblk_x : 1;
  sa.inf = d_inf; sa.row_stride = row_stride;
  sa.cnt = hist + hist_words; sa.off_local = c->part_cnt.as<uint32_t>();
  uint32_t* cnt_tile_tot = sa.off_local + cnt_len; sa.off_blk = cnt_tile_tot + cnt_tiles;
  sa.items = c->part_items.as<uint2>();
  const uint32_t* total_pairs = sp.total_pairs = sa.off_blk + cnt_tiles;          // grand total of the level-1 scan
  uint32_t* part_start = sa.off_blk + cnt_tiles + 4;             // ncb + 1 prefix counts of the level-2 parts
  const uint32_t nparts_max = ncb + (uint32_t)(pairs_max / BIN_PART) + 1;
  if (mont) launch_sort<true>(P.c, pre, sa, 0, s); else launch_sort<false>(P.c, pre, sa, 0, s);
  hipLaunchKernelGGL(k_scan32_tiles, dim3(cnt_tiles), dim3(256), 0, s, sa.cnt, (uint32_t)cnt_len, sa.off_local, cnt_tile_tot);
  hipLaunchKernelGGL(k_scan32_top, dim3(1), dim3(256), 0, s, cnt_tile_tot, cnt_tiles, sa.off_blk, FILL_SHIFT);
  if (mont) launch_sort<true>(P.c, pre, sa, 1, s); else launch_sort<false>(P.c, pre, sa, 1, s);
  hipLaunchKernelGGL(k_bin_parts, dim3(1), dim3(256), 0, s, sa.off_local, sa.off_blk, nblk, ncb, cnt_tiles, part_start);
  hipLaunchKernelGGL(k_bin_hist, dim3(nparts_max), dim3(256), 0, s, sa.items, sa.off_local, sa.off_blk, nblk, ncb, cnt_tiles, LB, part_start, hist);
  hipLaunchKernelGGL(k_bin_scatter, dim3(nparts_max), dim3(256), 0, s, sa.items, sa.off_local, sa.off_blk, nblk, ncb, cnt_tiles, LB, part_start, hist, bin_cursor, sorted);
  // The slice count, the longest bucket and the list lengths size the slice-tree launches.  k_scan_top (or block 0 of the fused k_slice_order) stores them (and this
  // call's sequence number behind them) into the slot's pinned, device-mapped buffer; the slice ordering and the accumulation — launched with grids from slice_bound() —
  // follow on `s` at once, and the host polls the sequence number long before the accumulation ends (msm_wait_meta): the GPU never waits for the round trip, and nothing
  // but kernels sits on the stream (rounds 1-4 copied the words back on the side stream behind an event of `s`: a copy launch and ~6 us of idle GPU per chain).
  uint32_t* host_meta = nullptr;
  HIPCHK(hipHostGetDevicePointer((void**)&host_meta, c->h_pinned, 0));
  sp.meta_seq = ++c->meta_seq;
  const bool fuse_top = lean && ntiles <= FUSED_TILES;      // (calls that time their phases keep the sort / slice-order boundary at ev[1])
  if ((rc = launch_slice_stage(sp, tile_tot, total_pairs, host_meta, fuse_top, lean ? nullptr : c->ev[1], s))) return rc;
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

int32_t msm_wait_meta(Ctx* c, const SortPhase& sp, hipStream_t s, SliceMeta* m) {
  const volatile uint32_t* h_meta = (const volatile uint32_t*)c->h_pinned;
  // poll the sequence number (it arrives ~0.15 ms after the sort was queued).  A stream that has drained or failed without delivering it is an error, not a hang.
  for (uint64_t spins = 0; h_meta[8] != sp.meta_seq; ++spins) {
    __builtin_ia32_pause();
    if ((spins & 0xfff) == 0xfff) {
      const hipError_t q = hipStreamQuery(s);
      if (q == hipErrorNotReady) continue;
      if (q == hipSuccess && h_meta[8] == sp.meta_seq) break;
      if (q == hipSuccess) { (void)hipStreamSynchronize(s); if (h_meta[8] == sp.meta_seq) break; }
      g_last_error = std::string("msm: the slice metadata never arrived (") + hipGetErrorString(q) + ")"; return ALEO_MI355X_ERR_HIP;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  m->NT = h_meta[0]; m->max_m = h_meta[1]; m->n_heavy = h_meta[3];
  m->max_common = h_meta[6] < 16u ? h_meta[6] : 16u;
  m->n_super = h_meta[5] < SUPER_CAP ? h_meta[5] : SUPER_CAP;
  m->super_overflow = h_meta[5] > SUPER_CAP;          // then the common list also holds very long buckets
  if (m->NT > sp.slices_max) {          // cannot happen (slice_bound); the kernels only touched threads below the bound
    (void)hipStreamSynchronize(s); g_last_error = "msm: internal slice count overflow"; return ALEO_MI355X_ERR_HIP;
  }
  return ALEO_MI355X_OK;
}

// Test hook (aleo_mi355x_selftest_slice_order): the slice stage alone — bucket scan, top scan (fused or not), slice ordering — on a histogram from the host, and
// what it left behind checked against a host recount.  A mis-sorted `order` leaves every sum right and only costs time: no result test can see it.
int32_t selftest_slice_order(Ctx* c, const uint32_t* h_hist, uint32_t M, uint32_t pairs, bool fused, uint32_t* violations) {
  const uint32_t ntiles = (M + SCAN_TILE - 1) / SCAN_TILE;
  uint64_t sum = 0; for (uint32_t g = 0; g < M; ++g) sum += h_hist[g];
  if (!M || M > (1u << 20) || sum >= (1ull << 31) || (fused && ntiles > FUSED_TILES)) { g_last_error = "selftest_slice_order: bad argument"; return ALEO_MI355X_ERR_BAD_ARG; }
  SortPhase sp; sp.M = M; sp.pairs_max = sum > pairs ? (size_t)sum : pairs; sp.slices_max = slice_bound(sp.pairs_max, M);
  const size_t hist_words = 3 * (size_t)M + 2048 + SUPER_CAP;
  int32_t rc;
  if ((rc = c->hist.reserve(hist_words * 4))) return rc;
  if ((rc = c->scan_local.reserve((size_t)M * 8))) return rc;
  if ((rc = c->scan_blk.reserve(2 * (size_t)ntiles * 8 + 64))) return rc;
  if ((rc = c->task_g.reserve(2 * sp.slices_max * 4))) return rc;
  if ((rc = c->part_cnt.reserve(16))) return rc;
  if ((rc = ensure_host_pinned(c, 64))) return rc;
  // the host's recount — first, so that a histogram the reservations (slice_bound) do not cover is refused and never launched
  const uint32_t tp[2] = {pairs, FILL_SHIFT};
  const SliceRule rule = pick_rule(tp, M);
  std::vector<uint32_t> first(M + 1), len_want(MAX_SLICE + 1, 0);
  uint32_t NT = 0, max_m = 0, max_common = 0, n_common = 0, n_super = 0;
  for (uint32_t g = 0; g < M; ++g) {
    const uint32_t cnt = h_hist[g], m = slices_of(cnt, rule);
    first[g] = NT; NT += m; max_m = m > max_m ? m : max_m;
    if (m > 16) ++n_super; else if (m > 1) { ++n_common; max_common = m > max_common ? m : max_common; }
    for (uint32_t k = 0; k < m; ++k) { const uint32_t l = slice_len(cnt, m, k); if (l <= MAX_SLICE) ++len_want[l]; }
  }
  first[M] = NT;
  if (pairs < sum || NT > sp.slices_max) { g_last_error = "selftest_slice_order: total_pairs below the histogram's sum"; return ALEO_MI355X_ERR_BAD_ARG; }      // (the rule would cut finer than slice_bound() allows for)
  hipStream_t s = c->stream;
  sp.hist = c->hist.as<uint32_t>(); sp.heavy = sp.hist + M; sp.meta = sp.heavy + M; sp.super_list = sp.heavy + M + 2048;
  sp.scan_local = c->scan_local.as<uint2>(); uint2* tile_tot = c->scan_blk.as<uint2>(); sp.scan_blk = tile_tot + ntiles;
  sp.task_g = c->task_g.as<uint32_t>(); sp.order = sp.task_g + sp.slices_max;
  uint32_t* total_pairs = c->part_cnt.as<uint32_t>();
  c->hist_clean = 0;
  HIPCHK(hipMemsetAsync(sp.hist, 0, hist_words * 4, s));
  HIPCHK(hipMemcpyAsync(sp.hist, h_hist, (size_t)M * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(total_pairs, tp, 8, hipMemcpyHostToDevice, s));
  uint32_t* host_meta = nullptr;
  HIPCHK(hipHostGetDevicePointer((void**)&host_meta, c->h_pinned, 0));
  sp.meta_seq = ++c->meta_seq;
  if ((rc = launch_slice_stage(sp, tile_tot, total_pairs, host_meta, fused, nullptr, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));

  uint32_t bad = 0;
  uint32_t meta[8 + 8 + MAX_SLICE + 1];
  HIPCHK(hipMemcpy(meta, sp.meta, sizeof meta, hipMemcpyDeviceToHost));
  const uint32_t over = n_super > SUPER_CAP ? n_super - SUPER_CAP : 0;
  const uint32_t want[7] = {NT, max_m, (uint32_t)sum, n_common + over, 0u, n_super, max_common};
  const volatile uint32_t* hm = (const volatile uint32_t*)c->h_pinned;
  for (int i = 0; i < 7; ++i) { bad += meta[i] != want[i]; bad += hm[i] != want[i]; }
  bad += hm[8] != sp.meta_seq;
  for (uint32_t l = 0; l <= MAX_SLICE; ++l) bad += meta[16 + l] != len_want[l];
  // both lists as sets: every multi-slice bucket once; the super list holds buckets of > 16 slices only, the common list such buckets only past SUPER_CAP
  if (meta[3] == want[3] && meta[5] == want[5]) {
    const uint32_t ns = n_super < SUPER_CAP ? n_super : SUPER_CAP;
    std::vector<uint32_t> lc(want[3]), ls(ns), seen(M, 0);
    if (!lc.empty()) HIPCHK(hipMemcpy(lc.data(), sp.heavy, lc.size() * 4, hipMemcpyDeviceToHost));
    if (!ls.empty()) HIPCHK(hipMemcpy(ls.data(), sp.super_list, ls.size() * 4, hipMemcpyDeviceToHost));
    uint32_t long_in_common = 0;
    for (uint32_t g : lc) { if (g >= M) { ++bad; continue; } const uint32_t m = slices_of(h_hist[g], rule); bad += m <= 1; long_in_common += m > 16; bad += seen[g]++ != 0; }
    for (uint32_t g : ls) { if (g >= M) { ++bad; continue; } bad += slices_of(h_hist[g], rule) <= 16; bad += seen[g]++ != 0; }
    bad += long_in_common != over;
  }
  if (meta[0] == NT && NT) {
    std::vector<uint32_t> task(NT), ord(NT), hit(NT, 0);
    HIPCHK(hipMemcpy(task.data(), sp.task_g, (size_t)NT * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ord.data(), sp.order, (size_t)NT * 4, hipMemcpyDeviceToHost));
    for (uint32_t sid = 0; sid < NT; ++sid) { const uint32_t g = task[sid]; bad += !(g < M && first[g] <= sid && sid < first[g + 1]); }
    uint32_t prev = 0xffffffffu;
    for (uint32_t t = 0; t < NT; ++t) {
      const uint32_t sid = ord[t];
      if (sid >= NT || hit[sid]++) { ++bad; continue; }      // not a permutation of [0, NT)
      uint32_t g = (uint32_t)(std::upper_bound(first.begin(), first.begin() + M, sid) - first.begin()) - 1;
      const uint32_t cnt = h_hist[g], l = slice_len(cnt, slices_of(cnt, rule), sid - first[g]);
      bad += l > prev; prev = l;                            // longest first
    }
  }
  *violations = bad;
  return ALEO_MI355X_OK;
}

// Test hook (aleo_mi355x_selftest_sort_pairs): msm_sort_phase itself on scalars, segments and infinity flags from the host, and what it left behind — hist[], the index
// stream, the level-1 scan's grand total — copied back for a test to compare with the digits of the scalars in integers.  Everything the kernels index is checked here first
// (a width without an instance, a set the count matrix has no rows for, a flag or table index past row_stride are refused before anything is launched).
int32_t selftest_sort_pairs(Ctx* c, const void* h_scalars, const uint32_t* seg_n, const uint32_t* seg_off, const uint8_t* seg_set, uint32_t nseg, int cbits, bool pre, bool mont,
                            uint32_t k_sets, uint32_t row_stride, const uint8_t* h_inf, uint32_t tile, uint32_t* hist_out, uint32_t* sorted_io, size_t sorted_cap, uint32_t* pairs_out) {
  auto refuse = [](const char* why) { g_last_error = std::string("selftest_sort_pairs: ") + why; return ALEO_MI355X_ERR_BAD_ARG; };
  if (!sort_has_case(cbits, pre)) return refuse("no sort instance of this window width on this path");
  if (!nseg || nseg > MAX_SEGS) return refuse("1 .. MAX_SEGS segments");
  if (!k_sets || k_sets > sets_of_window(cbits) || (!pre && k_sets != 1)) return refuse("more sets than a chain of this width holds (the plain path: one)");
  if (tile && tile != 2048 && tile != 4096 && tile != 8192) return refuse("tile is 0, 2048, 4096 or 8192");
  const uint32_t W = (uint32_t)win_count(cbits);
  size_t pts = 0;
  for (uint32_t q = 0; q < nseg; ++q) {
    if (!seg_n[q]) return refuse("empty segment");
    if (seg_set[q] >= k_sets) return refuse("segment of a set the call does not have");
    if ((uint64_t)seg_off[q] + seg_n[q] > row_stride) return refuse("a segment reaches past row_stride");
    pts += seg_n[q];
  }
  if (pts > ((size_t)1 << 20)) return refuse("at most 2^20 scalars");
  if ((uint64_t)W * row_stride >= (1ull << 31)) return refuse("windows * row_stride reaches bit 31 of an index");
  const size_t pairs_max = pts * W;
  if (sorted_cap < pairs_max) return refuse("sorted_io is shorter than scalars * windows");

  MsmPlan P; P.c = (uint32_t)cbits; P.B = 1u << (cbits - 1); P.W = pre ? k_sets : W; P.M = P.W * P.B; P.S = P.B >= 8 ? 8 : P.B;
  DevTmp d_scalars, d_inf; int32_t rc;
  if ((rc = d_scalars.alloc(pts * 32))) return rc;
  if (h_inf && (rc = d_inf.alloc(row_stride))) return rc;
  if ((rc = c->sorted.reserve(pairs_max * 4))) return rc;      // (what msm_sort_phase reserves: it keeps this buffer)
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(d_scalars.p, h_scalars, pts * 32, hipMemcpyHostToDevice, s));
  if (h_inf) HIPCHK(hipMemcpyAsync(d_inf.p, h_inf, row_stride, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->sorted.p, sorted_io, pairs_max * 4, hipMemcpyHostToDevice, s));      // the caller's fill: what the sort does not write comes back as it went in
  SegArgs segs{}; size_t at = 0;
  for (uint32_t q = 0; q < nseg; ++q) {
    segs.ptr[q] = (const char*)d_scalars.p + at * 32; segs.n[q] = seg_n[q]; segs.off[q] = seg_off[q]; segs.set[q] = seg_set[q]; at += seg_n[q];
  }
  segs.nseg = nseg;
  SortPhase sp;
  rc = msm_sort_phase(c, segs, pts, mont, (const uint8_t*)d_inf.p, row_stride, P, pre, s, &sp, true, tile);
  const hipError_t drained = hipStreamSynchronize(s);          // before d_scalars / d_inf go out of scope, whatever was queued
  if (rc) return rc;
  HIPCHK(drained);
  if (sp.sorted != c->sorted.as<uint32_t>() || sp.M != P.M) { g_last_error = "selftest_sort_pairs: internal: workspace moved"; return ALEO_MI355X_ERR_HIP; }
  HIPCHK(hipMemcpy(hist_out, sp.hist, (size_t)P.M * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(sorted_io, sp.sorted, pairs_max * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(pairs_out, sp.total_pairs, 4, hipMemcpyDeviceToHost));
  return ALEO_MI355X_OK;
}


}  // namespace aleo_mi355x
