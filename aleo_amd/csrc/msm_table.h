// msm_table.h — the table path behind the accumulation, as device function templates over the point format of the partial sums: what is left of the slice
// trees, the chunk sums of the bucket reduction and the sum tree of the chunk weights.  msm.hip wraps them into its kernels for 28-bit XYZZ points (Pt28),
// msm_te.hip for the extended Edwards points of the whole-set tier (PtTE, te28.h) — one text, two formats.
#pragma once
#include "msm_reduce.h"
#include "te28.h"

namespace aleo_mi355x {

__device__ __forceinline__ const char* chain_sum(const FrontChain& ch, uint32_t g) {
  for (uint32_t i = 0; i < ch.n; ++i) if (ch.v[i].hist[g]) return ch.v[i].partial + (size_t)scan_at(ch.v[i].scan_local, ch.v[i].scan_blk, g).y * 224u;
  return nullptr;
}

// Every kernel from here to the host tail is a chain of full XYZZ additions with little parallelism, so each addition
// is shared by a lane pair (ec.h xyzz_add_pair: same work, half the latency).  "op" below = pair index = thread / 2.
__device__ __forceinline__ void pair_fence() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }
template <uint32_t LANES, uint32_t BYTES> __device__ __forceinline__ void grp_copy(const char* src, char* dst) {      // BYTES / LANES per lane
  const uint32_t o = (threadIdx.x & (LANES - 1)) * (BYTES / LANES);
  const uint2* s2 = (const uint2*)(src + o); uint2* d2 = (uint2*)(dst + o);
#pragma unroll
  for (int i = 0; i < (int)(BYTES / LANES / 8); ++i) d2[i] = s2[i];
}
template <uint32_t LANES, uint32_t BYTES> __device__ __forceinline__ void grp_zero(char* dst) {
  uint2* d2 = (uint2*)(dst + (threadIdx.x & (LANES - 1)) * (BYTES / LANES));
#pragma unroll
  for (int i = 0; i < (int)(BYTES / LANES / 8); ++i) d2[i] = make_uint2(0, 0);
}
// lanes per addition for a launch of `ops` independent additions: quads up to two waves per SIMD (2^17 lanes), pairs beyond.  Measured: k_seg_fold 90 -> 57 us,
// k_tree_pass 15 -> 11 us, a 2^15-constraint proof 6.9 -> 6.6 ms; with the cut at 2^16 lanes the proof is at 6.8 ms.  (The 2^15-chunk kernel of the
// widest window is the exception: 2^17 quad lanes take what 2^16 pair lanes take, 330 against 321 us — it keeps the pair form.)
static constexpr uint32_t QUAD_MAX_LG = 17;  // lg of the most quad lanes a launch may have
static constexpr uint32_t ASIDE_MAX = 8;  // super-heavy buckets whose slice trees may run beside the reduction (msm_run)
static inline uint32_t grp_lanes(uint64_t ops) { return ops * 4 <= ((uint64_t)1 << QUAD_MAX_LG) ? 4u : 2u; }
// One launch of `ops` independent additions on `lanes` lanes each: the quad (k4) or the pair (k2) instantiation of a kernel, blocks of 256 threads.
template <class... KA, class... A>
static void launch_grp(uint32_t lanes, void (*k4)(KA...), void (*k2)(KA...), uint64_t ops, hipStream_t s, A... args) {
  hipLaunchKernelGGL(lanes == 4 ? k4 : k2, dim3((uint32_t)((lanes * ops + 255) / 256)), dim3(256), 0, s, args...);
}

// ---- the formats of the table path ------------------------------------------------------------------------------------------------------------------
// PtTE: extended Edwards points (te28.h), 224 bytes like a 28-bit XYZZ point.  The identity is an ordinary point, (0 : 1 : 1 : 0) where the XYZZ form writes
// zeros; an addition has no special cases but reports Z3 == 0 (operands that differ by a point of even order: bases outside G1), which the caller records in
// the chain's flag word (msm_reduce.h TE_FLAG_WORD), which the last kernels of a chain hand to the host.
__host__ __device__ __forceinline__ uint32_t* te_flag_of(const uint32_t* meta) { return (uint32_t*)meta + TE_FLAG_WORD; }
struct PtTE {
  static constexpr uint32_t BYTES = 224, WORDS = BYTES / 4; static constexpr bool TE = true;
  template <uint32_t LANES> static __device__ __forceinline__ int add(const char* pa, const char* pb, char* out) { if constexpr (LANES == 4) return te28_add_quad(pa, pb, out); else return te28_add_pair(pa, pb, out); }
};
template <class PT, uint32_t LANES> __device__ __forceinline__ void pt_add(const char* pa, const char* pb, char* out, uint32_t* flag) {
  if constexpr (PT::TE) { if (PT::template add<LANES>(pa, pb, out)) *flag = 1u; }
  else PT::template add<LANES>(pa, pb, out);
}
// the identity written by the LANES lanes of a group, BYTES / LANES each
template <class PT, uint32_t LANES> __device__ __forceinline__ void pt_zero(char* dst) {
  if constexpr (PT::TE) {
    const uint32_t l = threadIdx.x & (LANES - 1);
#pragma unroll
    for (uint32_t k = 0; k < 4 / LANES; ++k) { const uint32_t co = l * (4 / LANES) + k; store_f28(dst + 56 * co, (co == 1 || co == 2) ? te28_const(TE_ONE_28) : f28_const(Limbs14{})); }
  } else grp_zero<LANES, PT::BYTES>(dst);
}

// What is left of the common list's trees after the first level (at most 4 partial sums per bucket when no bucket had more than 8 slices) folded by ONE launch:
// a lane quad per multi-slice bucket adds its partials 1.. into partial 0 one after the other.  Two or three dependent additions of ~7 us inside one launch
// instead of two launches of one level each (~10 us of launch floor + its addition per level): the chains of real-circuit-sized proofs are made of such steps.
template <class PT, uint32_t LANES>
__device__ __forceinline__ void tree_rest_body(char* __restrict__ partial, const uint32_t* __restrict__ list, uint32_t list_len, const uint2* __restrict__ scan_local,
                                                   const uint2* __restrict__ scan_blk, uint32_t M, const uint32_t* __restrict__ meta) {
  constexpr uint32_t PB = PT::BYTES;
  const uint32_t h = (blockIdx.x * 256 + threadIdx.x) >> lg_lanes(LANES);
  if (h >= list_len) return;
  const uint32_t g = list[h];
  const uint32_t ft = scan_at(scan_local, scan_blk, g).y, fn = (g + 1 < M) ? scan_at(scan_local, scan_blk, g + 1).y : meta[0];
  const uint32_t L1 = (fn - ft + 1) >> 1;                   // partial sums the first level left at ft .. ft + L1 - 1
  char* pa = partial + (size_t)ft * PB;
  for (uint32_t i = 1; i < L1; ++i) pt_add<PT, LANES>(pa, pa + (size_t)i * PB, pa, te_flag_of(meta));
}

// The sums of slices 1.. of the super-heavy buckets (k_tree_pass with skip_b = 1 left them in slice 1) and the buckets' numbers, to the host.
// (flag: the Edwards tier hands the side stream's Z3 == 0 word to the host behind the records; null otherwise)
__device__ __forceinline__ void gather_super_body(const char* __restrict__ partial, const uint32_t* __restrict__ list, uint32_t len, const uint2* __restrict__ scan_local,
                               const uint2* __restrict__ scan_blk, uint32_t* __restrict__ dst, const uint32_t* flag) {
  constexpr uint32_t PW = Pt28::WORDS;
  const uint32_t t = blockIdx.x * 256 + threadIdx.x, h = t / (PW + 1), w = t % (PW + 1);
  if (flag && t == 0) dst[len * (PW + 1)] = flag[0];
  if (h >= len) return;
  const uint32_t g = list[h];
  dst[h * (PW + 1) + w] = w == PW ? g : ((const uint32_t*)(partial + (size_t)(scan_at(scan_local, scan_blk, g).y + 1) * Pt28::BYTES))[w];
}

static constexpr uint32_t PB28 = 224, PW28 = 56;      // every format of the table path
// ---- bucket reduction -----------------------------------------------------------------------------
// One lane QUAD per chunk of S consecutive buckets: running sums run_k = run_{k-1} + S_b (b descending) and acc += run_{k-1}
// are independent once run_{k-1} exists, so two lane pairs work one step apart (S + 1 dependent additions instead of 2S):
// sub-pair 0 extends the running sum (double-buffered in LDS), sub-pair 1 folds the previous one into acc.  Both make the
// SAME addition call with per-lane pointers (a branch per sub-pair would serialise them inside the wave).
// acc = sum_{b in chunk} (b - base + 1) * S_b and run = chunk total go to HBM (V, Vrun); the chunk weights are applied by
// masked sums (fixed-base path).
static constexpr uint32_t CHUNK_QUADS = 64;         // chunks per 256-thread block (LANES = 2: two lane pairs per chunk; 32 with LANES = 4: two lane quads)
// (flag_off: the Edwards tier's Z3 == 0 word, as an offset from `hist` — the same offset in every chunk of a request, whose earlier chunks' words are folded in here)
template <class PT, uint32_t LANES>
__device__ __forceinline__ void bucket_chunks_body(const char* __restrict__ partial, const uint32_t* __restrict__ hist, const uint2* __restrict__ scan_local,
                                                       const uint2* __restrict__ scan_blk, uint32_t B, uint32_t S, uint32_t nchunks_total, char* __restrict__ V,
                                                       uint32_t v_set_stride, char* __restrict__ Vrun, const FrontChain& older, uint32_t flag_off) {
  constexpr uint32_t PB = PT::BYTES, PW = PT::WORDS;
  constexpr uint32_t CPB = 128 / LANES;                  // chunks per block: two groups of LANES lanes each
  __shared__ __attribute__((aligned(16))) uint32_t lds[(3 * CPB + 1) * PW];
  const uint32_t qd = threadIdx.x >> (lg_lanes(LANES) + 1), sp = (threadIdx.x >> lg_lanes(LANES)) & 1u, t = blockIdx.x * CPB + qd;
  char* zero = (char*)(lds + 3 * CPB * PW);
  if (threadIdx.x < LANES) pt_zero<PT, LANES>(zero);
  uint32_t* const flag = (uint32_t*)hist + flag_off;
  if constexpr (PT::TE) { if (blockIdx.x == 0 && threadIdx.x == 0) for (uint32_t i = 0; i < older.n; ++i) if (older.v[i].hist[flag_off]) flag[0] = 1u; }
  __syncthreads();
  if (t >= nchunks_total) return;
  char* buf0 = (char*)(lds + (3 * qd) * PW); char* buf1 = buf0 + PB; char* acc = buf1 + PB;
  pt_zero<PT, LANES>(sp ? acc : buf0); if (!sp) pt_zero<PT, LANES>(buf1);
  pair_fence();
  const uint32_t cpw = B / S, w = t / cpw, j = t % cpw, g0 = w * B + j * S;
  // the address of the next bucket's sum (two dependent loads: histogram, scan) is fetched one step ahead of the addition that uses it
  auto sum_of = [&](uint32_t g) -> const char* { if (hist[g]) return partial + (size_t)scan_at(scan_local, scan_blk, g).y * PB; const char* o = chain_sum(older, g); return o ? o : zero; };
  const char* nxt = sp ? zero : sum_of(g0 + S - 1);
  for (uint32_t k = 0; k <= S; ++k) {
    char* rprev = (k & 1) ? buf0 : buf1; char* rnext = (k & 1) ? buf1 : buf0;      // run_k lives in buf[k & 1]; run_{-1} = 0
    const char* add = k < S ? nxt : zero;
    nxt = (!sp && k + 1 < S) ? sum_of(g0 + S - 2 - k) : zero;
    const char* pa = sp ? acc : rprev; const char* pb = sp ? rprev : add; char* out = sp ? acc : rnext;
    pt_add<PT, LANES>(pa, pb, out, flag);
    pair_fence();
  }
  // after step S: buf[S & 1] holds run_{S-1} again (step S copied it forward), acc holds sum_k run_k
  grp_copy<LANES, PB>(sp ? acc : ((S & 1) ? buf1 : buf0), sp ? V + ((size_t)w * v_set_stride + j) * PB : Vrun + (size_t)t * PB);
}

static constexpr uint32_t FOLD = 256;      // points one block folds into one through LDS
// ---- the chunk weights by ONE sum tree (wide tables, round 3) -------------------------------------------------------------------------------------
// sum_j j * run_j = sum_l 2^l T_l, T_l = the sum of run_j over the j with bit l set.  k_masked_pairs builds every T_l as its own tree over half of
// the chunks: lg(N) / 2 additions per chunk.  But T_l is also the sum of the RIGHT children of level l of the plain sum tree over the chunks — so one
// pairwise pass per level does it all: node'[i] = node[2i] + node[2i+1], the odd nodes node[2i+1] start the segment T_l, and every segment born
// earlier (T_0 .. T_{l-1}, and A = the chunks' own weighted sums acc_j) is halved the same way.  After pass s every segment is N / 2^(s+1) long:
// (s + 3) N / 2^(s+1) additions per pass, 3 N in all instead of (lg N + 4) N / 2 — which is what lets the chunks shrink (fewer dependent additions
// in k_bucket_chunks) without the weights paying for it.  Layout of a set after pass s: [node | A | T_0 | ... | T_s], contiguous.
template <class PT, uint32_t LANES>
__device__ __forceinline__ void prog_pass_body(const char* __restrict__ node, uint32_t node_set_stride, const char* __restrict__ A, uint32_t a_set_stride,
                                                   const char* __restrict__ T, uint32_t t_set_stride, uint32_t nT, uint32_t L, uint32_t nsets,
                                                   char* __restrict__ out, uint32_t out_set_stride, uint32_t* flag) {
  const uint32_t half = L >> 1, per_set = (2 + nT) * half;
  const uint32_t op = (blockIdx.x * 256 + threadIdx.x) >> lg_lanes(LANES);
  if (op >= per_set * nsets) return;
  const uint32_t q = op / per_set, r = op % per_set, g = r / half, i = r % half;
  const char* src = g == 0 ? node + ((size_t)q * node_set_stride + 2 * i) * PB28
                  : g == 1 ? A + ((size_t)q * a_set_stride + 2 * i) * PB28
                           : T + ((size_t)q * t_set_stride + (size_t)(g - 2) * L + 2 * i) * PB28;
  char* dst = out + ((size_t)q * out_set_stride + (size_t)g * half + i) * PB28;
  pt_add<PT, LANES>(src, src + PB28, dst, flag);
  if (g == 0) grp_copy<LANES, PB28>(src + PB28, out + ((size_t)q * out_set_stride + (size_t)(2 + nT) * half + i) * PB28);      // T_s is born: the right children of this level
}
// TWO levels in one launch while the passes are latency-bound (lane quads): an octet of lanes per four consecutive points of a segment.  Step 1: quad 0 adds points
// 0 + 1, quad 1 adds 2 + 3, into LDS; step 2: quad 0 adds the two halves (the point of the segment two levels up) while quad 1, on the node segment, adds points
// 1 + 3 (T_nT, born at the first of the two levels, already halved by the second) and copies 2 + 3 out (T_(nT+1), born at the second).  Same sums as two k_prog_pass
// launches — the grouping of the additions differs, the points they represent do not — for two dependent additions and ONE launch instead of two and two:
// ~9 us less per pair of levels (a launch boundary costs about as much as a lane-quad addition).  Output layout as after two single passes:
// [node | A | T_0 .. T_(nT-1) | T_nT | T_(nT+1)], every segment L / 4 long.
template <class PT>
__device__ __forceinline__ void prog_pass2_body(const char* __restrict__ node, uint32_t node_set_stride, const char* __restrict__ A, uint32_t a_set_stride,
                                                    const char* __restrict__ T, uint32_t t_set_stride, uint32_t nT, uint32_t L, uint32_t nsets,
                                                    char* __restrict__ out, uint32_t out_set_stride, uint32_t* flag) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[(2 * 32 + 1) * PW28];
  char* zero = (char*)(lds + 64 * PW28);
  if (threadIdx.x < 4) pt_zero<PT, 4>(zero);
  __syncthreads();
  const uint32_t quarter = L >> 2, per_set = (2 + nT) * quarter;
  const uint32_t oct = threadIdx.x >> 3, y = (threadIdx.x >> 2) & 1u, op = blockIdx.x * 32 + oct;
  if (op >= per_set * nsets) return;
  const uint32_t q = op / per_set, r = op % per_set, g = r / quarter, i = r % quarter;
  const char* src = g == 0 ? node + ((size_t)q * node_set_stride + 4 * i) * PB28
                  : g == 1 ? A + ((size_t)q * a_set_stride + 4 * i) * PB28
                           : T + ((size_t)q * t_set_stride + (size_t)(g - 2) * L + 4 * i) * PB28;
  char* slot = (char*)(lds + (2 * oct) * PW28);
  pt_add<PT, 4>(src + (size_t)(2 * y) * PB28, src + (size_t)(2 * y + 1) * PB28, slot + y * PB28, flag);
  pair_fence();
  char* base = out + (size_t)q * out_set_stride * PB28;
  const bool born = y && g == 0;
  const char* pa = y ? (born ? src + PB28 : zero) : slot;
  const char* pb = y ? (born ? src + 3 * PB28 : zero) : slot + PB28;
  char* dst = y ? (born ? base + ((size_t)(2 + nT) * quarter + i) * PB28 : zero) : base + ((size_t)g * quarter + i) * PB28;      // (an idle quad: 0 + 0 onto the zero point, nothing is written)
  pt_add<PT, 4>(pa, pb, dst, flag);
  if (born) grp_copy<4, PB28>(slot + PB28, base + ((size_t)(3 + nT) * quarter + i) * PB28);
}
// The last levels, one block per result point: A and every T_l already born are plain folds of their (<= 256-point) segments; the weights of the
// remaining lg L bits come from the node segment itself, T_(nT + b) = the sum of the nodes whose index has bit b set.  Output point o of set q:
// 0 = A, 1 + l = T_l.
// (Edwards tier: the block's own Z3 == 0 reports gather in LDS and go, with the chain's device word `flag`, to host_flags[block] — the last kernel of the chain,
// so the host finds every report of the chain in the words of its blocks)
template <class PT, uint32_t LANES>
__device__ __forceinline__ void prog_final_body(const char* __restrict__ in, uint32_t in_set_stride, uint32_t L, uint32_t nT, uint32_t lgL, uint32_t nsets,
                                                            char* __restrict__ out, const uint32_t* flag, uint32_t* host_flags) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[2][(FOLD / 2) * PW28];
  __shared__ uint32_t mine;
  if constexpr (PT::TE) { if (threadIdx.x == 0) mine = 0; __syncthreads(); }
  const uint32_t per_set = 1 + nT + lgL, q = blockIdx.x / per_set, o = blockIdx.x % per_set, pr = threadIdx.x >> lg_lanes(LANES);
  if (q >= nsets) return;
  const char* set = in + (size_t)q * in_set_stride * PB28;
  {
    char* dst = (char*)(lds[0] + pr * PW28);
    if (o <= nT) {                                         // plain fold of segment 1 (A) or 2 + (o - 1) (T_{o-1})
      const char* seg = set + (size_t)(o == 0 ? 1 : 1 + o) * L * PB28; const uint32_t e0 = 2 * pr;
      if (e0 + 1 < L) pt_add<PT, LANES>(seg + (size_t)e0 * PB28, seg + (size_t)(e0 + 1) * PB28, dst, &mine);
      else if (e0 < L) grp_copy<LANES, PB28>(seg + (size_t)e0 * PB28, dst);
      else pt_zero<PT, LANES>(dst);
    } else {                                               // bit b of the node index: the L / 2 nodes that have it set, in pairs
      const uint32_t b = o - 1 - nT;
      auto ins = [&](uint32_t x) { return ((x >> b) << (b + 1)) | (1u << b) | (x & ((1u << b) - 1u)); };
      if (L >= 4 && 4 * pr + 3 < L) pt_add<PT, LANES>(set + (size_t)ins(2 * pr) * PB28, set + (size_t)ins(2 * pr + 1) * PB28, dst, &mine);
      else if (L == 2 && pr == 0) grp_copy<LANES, PB28>(set + PB28, dst);
      else pt_zero<PT, LANES>(dst);
    }
  }
  uint32_t cur = 0;
  for (uint32_t n = FOLD / 2; n > 1; n >>= 1) {
    __syncthreads();
    if (pr < (n >> 1)) pt_add<PT, LANES>((const char*)(lds[cur] + (2 * pr) * PW28), (const char*)(lds[cur] + (2 * pr + 1) * PW28), (char*)(lds[cur ^ 1] + pr * PW28), &mine);
    cur ^= 1;
  }
  __syncthreads();
  if (pr == 0) grp_copy<LANES, PB28>((const char*)lds[cur], out + ((size_t)q * per_set + o) * PB28);
  if constexpr (PT::TE) { if (threadIdx.x == 0) host_flags[blockIdx.x] = mine | flag[0]; }
}

}  // namespace aleo_mi355x
