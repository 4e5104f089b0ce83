// ntt.hip — radix-2 number-theoretic transform over the BLS12-377 scalar field Fr for MI355X (gfx950).
//
// Replaces snarkvm-algorithms 0.14.5  algorithms/src/fft/domain.rs  EvaluationDomain::<Fr>::
// {fft,ifft,coset_fft,coset_ifft}_in_place  [UPSTREAM-RECALL; pin /root/reference/Cargo.lock:2200], the second
// operator of Varuna's prover.  Same function: out[k] = sum_j x[j] * w^(jk) with
// w = TWO_ADIC_ROOT_OF_UNITY^(2^(47-lg_n)), natural order in and out; coset variants shift by g = 22;
// the inverse multiplies by n^-1.  The schedule is GPU-first:
//
//   n = n1*n2*n3 (each <= 2^11; ntt_plan.h plan_passes).  Pass i runs all length-n_i DFTs of its axis inside LDS (one HBM read and one
//   HBM write of the data per pass: 1-3 passes instead of lg_n), as radix-2 DIF butterflies over limb-planar
//   LDS tiles (conflict-free 4-byte accesses), followed by the inter-pass twiddle w^(k*j_rest) taken from a
//   two-level table (hi*lo) or, for two-pass sizes, from an n-entry table.  Tiles are T adjacent transforms wide so every HBM access is a
//   >=128-byte run; the last pass writes straight to the natural-order position (index-transposed store), so there is no separate
//   bit-reversal pass.  The data in HBM is 8 x 32-bit words (Montgomery, R = 2^256), canonical after the last pass.
//
// One pair of kernels (k_ntt_strided, k_ntt_final) serves two limb forms; three configurations have an instance (ntt_plan.h choose_form):
//   Limbs32,  512-element tile (16 KiB), 256 threads, one butterfly stage per LDS round trip: the latency form of small calls
//   Limbs29, 4096-element tile (9 planes: 144 KiB of the CU's 160 KiB), 512 threads, three-stage register groups: 2^20..2^22 in TWO passes
//   Limbs29, 2048-element tile (72 KiB, two blocks per CU), 256 threads, three-stage register groups: everything else
//
// HBM traffic: 64 bytes per element per pass (read + write), algorithmic minimum 64 bytes per element.
#include "ctx.h"
#include "fp.h"
#include "fr29.h"
#include "host_field.hpp"
#include "ntt_plan.h"
#include <cstdlib>

namespace aleo_mi355x {

struct FrArg { uint32_t v[8]; };
// Out-of-place, zero-padded input of a transform's FIRST pass (ntt_run_from): transform b of the batch reads element i from p + (b * stride + i) * 32 when
// i < len and takes 0 otherwise; p == nullptr = the ordinary in-place call.  (A prover round pads |H| coefficients to 4|H| and |K| to 2|K| before it
// evaluates: a fill and one copy per polynomial in rounds 1-4 — launches of ~4.5 us each at the sizes of real circuits.)
struct NttSrc { const char* p = nullptr; uint32_t len = 0, stride = 0; };

__device__ __forceinline__ uint32_t bitrev(uint32_t x, uint32_t bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }

// planar LDS tile: limb l of element e at lds[l * TE + sw(e)].  sw() XORs the low five index bits with the next five: a bijection
// that leaves runs of consecutive elements conflict-free and spreads the stride-4 / stride-8 accesses of the last register groups
// (elements base + j * q with q = 1, 4: every lane of a wave used to hit the same 4-8 of the 32 banks) over the banks.
__device__ __forceinline__ uint32_t sw(uint32_t e) { return e ^ ((e >> 5) & 31u); }
template <class F, uint32_t TE> __device__ __forceinline__ typename F::Elem lds_load(const uint32_t* lds, uint32_t e) {
  typename F::Elem r;
  const uint32_t x = sw(e);
#pragma unroll
  for (int l = 0; l < F::PLANES; ++l) r.v[l] = lds[l * TE + x];
  return r;
}
template <class F, uint32_t TE> __device__ __forceinline__ void lds_store(uint32_t* lds, uint32_t e, const typename F::Elem& a) {
  const uint32_t x = sw(e);
#pragma unroll
  for (int l = 0; l < F::PLANES; ++l) lds[l * TE + x] = a.v[l];
}

// w^e from the two-level table (one product; Limbs32: result < 2r)
template <class F> __device__ __forceinline__ typename F::Elem two_level(const char* hi, const char* lo, uint32_t e, uint32_t lo_bits) {
  return F::mul(F::load_entry(hi + (size_t)(e >> lo_bits) * 32), F::load_entry(lo + (size_t)(e & ((1u << lo_bits) - 1u)) * 32));
}

// ---- the two limb forms: what a kernel needs to know about its elements ----------------------------------------------------------------------------
// Both fill a tile of T rows of L = 2^lgL elements through the kernel's index maps: where(elem, t, l) gives the row t and the position l in the row of
// the elem-th element of the tile (in the order that makes adjacent lanes read adjacent addresses) and returns its index in HBM; coset_exp(t, l) is the j
// of x[j] *= g^j.  (L is passed beside lgL so that kernel and fill share one value: the compiler folds the masks L - 1 differently otherwise.)

// 8 x 32-bit limbs (fp.h): values stay lazily reduced in [0, 2r) and are made canonical at the final store.
struct Limbs32 {
  using Elem = Fr; using ScaleArg = FrArg;
  static constexpr int PLANES = 8, SET = 0;
  static constexpr uint32_t DIRECT_MAX_LG = 18;             // the n-entry inter-pass table: every size this form runs from 2^12 on
  static __device__ __forceinline__ Fr load_entry(const char* p) { return load_fp<Fr>(p); }
  static __device__ __forceinline__ Fr load_inner(const char* inner, uint32_t i) { return load_fp<Fr>(inner + (size_t)i * 32); }
  static __device__ __forceinline__ Fr mul(const Fr& a, const Fr& b) { return Fr::mul(a, b); }
  // two lanes per element, a uint4 each: half-elements go straight to their four planes; the coset factor takes a sweep of its own
  template <uint32_t TE, uint32_t NT, class Where, class CosetExp>
  static __device__ __forceinline__ void fill(uint32_t* lds, const char* src, const NttSrc& ext, uint32_t lgL, uint32_t L, uint32_t T, int pre_coset, const char* cs_hi,
                                              const char* cs_lo, uint32_t lo_bits, Where where, CosetExp coset_exp) {
    const uint32_t nq = (T * L) << 1;
    for (uint32_t q = threadIdx.x; q < nq; q += NT) {
      uint32_t hf = q & 1, t, l;
      size_t gi = where(q >> 1, t, l);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (!ext.p || gi < ext.len) v = *(const uint4*)(src + gi * 32 + hf * 16);
      uint32_t e = t * L + l, p = hf * 4;
      const uint32_t ex = sw(e);
      lds[(p + 0) * TE + ex] = v.x; lds[(p + 1) * TE + ex] = v.y; lds[(p + 2) * TE + ex] = v.z; lds[(p + 3) * TE + ex] = v.w;
    }
    __syncthreads();
    if (pre_coset) {
      for (uint32_t e = threadIdx.x; e < T * L; e += NT) {
        uint32_t t = e >> lgL, l = e & (L - 1u);
        Fr x = lds_load<Limbs32, TE>(lds, e);
        x = Fr::mul(x, two_level<Limbs32>(cs_hi, cs_lo, coset_exp(t, l), lo_bits));   // 1*2/13.7+1 -> < 2r
        lds_store<Limbs32, TE>(lds, e, x);
      }
      __syncthreads();
    }
  }
  // one radix-2 DIF butterfly: (lo, hi) <- (lo + hi, (lo - hi) * tw); lgh == 0: the twiddle is 1.  In and out < 2r, so a group needs nothing before a stage or at its end.
  template <int G> static __device__ __forceinline__ void before_stage(Fr (&)[1 << G], int) {}
  static __device__ __forceinline__ void butterfly(Fr& lo, Fr& hi, Fr tw, uint32_t lgh) {
    Fr u = lo, x = hi;
    lo = Fr::cond_sub<2>(Fr::add(u, x));                      // < 4r -> < 2r
    Fr dif = Fr::sub<2>(u, x);                                // u + 2r - x < 4r
    hi = lgh ? Fr::mul(dif, tw) : Fr::cond_sub<2>(dif);       // 4*1/13.7 + 1 -> < 2r
  }
  template <int K> static __device__ __forceinline__ void after_group(Fr (&)[K]) {}
  // what a pass stores: < 2r between passes, canonical after the last (whether or not a last product — coset power or n^-1 — came before)
  // (store_final takes base and index, not the address: the reduction comes first in the instruction stream, as it always has)
  static __device__ __forceinline__ Fr to_words(const Fr& x) { return x; }
  static __device__ __forceinline__ void no_last_product(Fr&) {}
  static __device__ __forceinline__ void store_final(char* dst, size_t i, const Fr& x, bool) { const Fr y = Fr::reduce(x); store_fp<Fr>(dst + i * 32, y); }
};

// 9 x 29-bit limbs (fr29.h; tables in the Montgomery form of R = 2^261): butterflies without conditional subtractions.
// Bounds inside a register group, for values that enter it normalised and below 4.5 r:
//   sum  lo = u + x            lazy: limbs and value double per stage (8 x at most: limbs <= 2^32 - 8, value < 36 r)
//   diff hi = (u + 19 r - x) w  the padded constant keeps every limb non-negative for x with limbs <= 2^30 - 2 and a value < 18 r; the product takes
//                               a multiplicand with limbs < 2^31.4 and returns a normalised value < (37 / 445 + 1) r
//   before the third stage of a three-stage group registers 0 and 1 (sums of sums: limbs < 2^31) are normalised; at the end the sums of the last
//   stage are normalised and register 0 — the only one that was a sum in every stage — is brought below 3 r (f29_reduce_partial).
//   A stage whose twiddle is 1 (half-size 1) normalises and reduces its differences instead of multiplying them.
// So every value a group stores is normalised and below 4.5 r (the largest: a sum of two sums of products, 4.4 r).
struct Limbs29 {
  using Elem = F29; using ScaleArg = F29Arg;
  static constexpr int PLANES = 9, SET = 1;
  static constexpr uint32_t DIRECT_MAX_LG = 21;      // 2^21: 0.286 -> 0.271 ms with the table, 2^22: 0.549 -> 0.564 ms (the extra 32 B per element of HBM reads cost more than the product; round 4: fetching a lane's eight table entries in one go ahead of the products changes nothing — 2^22 0.581 / 0.588 ms without / with the table, 2^21 0.277 / 0.283 ms with the entries fetched late / ahead)
  static __device__ __forceinline__ F29 load_entry(const char* p) { return f29_load_packed(p); }
  static __device__ __forceinline__ F29 load_inner(const char* inner, uint32_t i) { return f29_load48(inner + (size_t)i * 48); }
  static __device__ __forceinline__ F29 mul(const F29& a, const F29& b) { return f29_mul(a, b); }
  // one lane loads and repacks a whole element and applies the coset factor on the way
  template <uint32_t TE, uint32_t NT, class Where, class CosetExp>
  static __device__ __forceinline__ void fill(uint32_t* lds, const char* src, const NttSrc& ext, uint32_t lgL, uint32_t L, uint32_t T, int pre_coset, const char* cs_hi,
                                              const char* cs_lo, uint32_t lo_bits, Where where, CosetExp coset_exp) {
    for (uint32_t elem = threadIdx.x; elem < T * L; elem += NT) {
      uint32_t t, l;
      const size_t gi = where(elem, t, l);
#if defined(ALEO_NTT_PROBE) && ALEO_NTT_PROBE == 3
      F29 x; for (int i = 0; i < 9; ++i) x.v[i] = (uint32_t)(gi * 2654435761u + i) & 0x1fffffffu;      // timing probe: no HBM reads
#else
      F29 x;
      if (!ext.p || gi < ext.len) x = f29_load_packed(src + gi * 32);
      else { for (int i = 0; i < 9; ++i) x.v[i] = 0u; }
#endif
      if (pre_coset) x = f29_mul(x, two_level<Limbs29>(cs_hi, cs_lo, coset_exp(t, l), lo_bits));
      lds_store<Limbs29, TE>(lds, t * L + l, x);
    }
    __syncthreads();
  }
  template <int G> static __device__ __forceinline__ void before_stage(F29 (&v)[1 << G], int t) {
    if (G == 3 && t == 2) { f29_normalise(v[0]); f29_normalise(v[1]); }
  }
  static __device__ __forceinline__ void butterfly(F29& lo, F29& hi, F29 tw, uint32_t lgh) {
    const F29 u = lo, x = hi;
    lo = f29_add(u, x);
    F29 dif = f29_sub_pad(u, x);
    if (lgh) hi = f29_mul(dif, tw);
    else { f29_normalise(dif); f29_reduce_partial(dif); hi = dif; }
  }
  template <int K> static __device__ __forceinline__ void after_group(F29 (&v)[K]) {
#pragma unroll
    for (int j = 0; j < K; j += 2) f29_normalise(v[j]);       // the sums of the last stage
    f29_reduce_partial(v[0]);
  }
  // what a pass stores.  Between passes, after the inter-pass product: < 1.1 r, the next pass repacks it.  After the last: an output that passed a last
  // product (the coset power, n^-1; a table product in k_build_direct) is below 1.1 r and one conditional subtraction makes it canonical; the others
  // (plain forward transform: < 4.5 r) are reduced below 3 r first (no_last_product, in place of the last product) and take two more.
  static __device__ __forceinline__ Fr to_words(const F29& x) { return f29_to_fr(x); }
  static __device__ __forceinline__ void no_last_product(F29& x) { f29_reduce_partial(x); }
  static __device__ __forceinline__ void store_final(char* dst, size_t i, const F29& x, bool after_product) {
    Fr y = f29_to_fr(x);
    if (!after_product) y = Fr::cond_sub<2>(y);
    store_fp<Fr>(dst + i * 32, Fr::cond_sub<1>(y));
  }
};

// G consecutive radix-2 DIF stages (first one = stage s) on 2^G elements held in registers: one LDS read and one LDS
// write per element per GROUP instead of per stage, a third of the barriers, 7 twiddle loads per 8 elements per 3
// stages instead of 12.  Element j of the super-butterfly sits at base + j*q, q = L >> (s + G).
template <class F, uint32_t TE, int G> __device__ __forceinline__ void dif_group(uint32_t* lds, uint32_t lgL, uint32_t s, uint32_t sb, const char* __restrict__ inner) {
  constexpr int K = 1 << G;
  const uint32_t lgq = lgL - s - G, q = 1u << lgq, per_row_lg = lgL - G;
  const uint32_t row = sb >> per_row_lg, w = sb & ((1u << per_row_lg) - 1u);
  const uint32_t grp = w >> lgq, pos = w & (q - 1u);
  const uint32_t base = (row << lgL) + (grp << (lgq + G)) + pos;
  typename F::Elem v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = lds_load<F, TE>(lds, base + ((uint32_t)j << lgq));
#pragma unroll
  for (int t = 0; t < G; ++t) {
    const int d = 1 << (G - 1 - t);                               // partner distance in units of q
    const uint32_t lgh = lgq + (uint32_t)(G - 1 - t);             // lg of the butterfly half-size in elements
    F::template before_stage<G>(v, t);
#pragma unroll
    for (int r = 0; r < d; ++r) {                                 // distinct twiddles of this stage
      typename F::Elem tw;
      if (lgh) tw = F::load_inner(inner, (((uint32_t)r << lgq) + pos) << (INNER_MAX_LG - 1 - lgh));
#pragma unroll
      for (int blk = 0; blk < K / (2 * d); ++blk) F::butterfly(v[blk * 2 * d + r], v[blk * 2 * d + r + d], tw, lgh);
    }
  }
  F::template after_group<K>(v);
#pragma unroll
  for (int j = 0; j < K; ++j) lds_store<F, TE>(lds, base + ((uint32_t)j << lgq), v[j]);
}

// All radix-2 DIF stages of T length-L transforms held in the tile (row t at [t*L, (t+1)*L)).  Output k of row t ends at position t*L + bitrev(k).
// GM = 3: register groups of 3 stages (then 2 or 1).
// GM = 1 (the latency form for a lone small transform): one stage per LDS round trip, one butterfly per lane — a 512-element tile keeps 256 lanes busy
// for 9 short steps instead of 64 lanes for 3 long ones (12 dependent products each).
template <class F, uint32_t TE, uint32_t NT, int GM> __device__ __forceinline__ void tile_dif(uint32_t* lds, uint32_t lgL, uint32_t T, const char* __restrict__ inner) {
  static_assert(GM == 1 || GM == 3, "group sizes with a kernel instance");
#if defined(ALEO_NTT_PROBE) && (ALEO_NTT_PROBE == 1 || ALEO_NTT_PROBE == 2)
  return;                                                   // timing probe: memory phases only
#endif
  const uint32_t total = T << lgL;
  if constexpr (GM == 1) {
    for (uint32_t s = 0; s < lgL; ++s) {
      for (uint32_t sb = threadIdx.x; sb < (total >> 1); sb += NT) dif_group<F, TE, 1>(lds, lgL, s, sb, inner);
      __syncthreads();
    }
  } else {
    uint32_t s = 0;
    for (; s + 3 <= lgL; s += 3) {
      for (uint32_t sb = threadIdx.x; sb < (total >> 3); sb += NT) dif_group<F, TE, 3>(lds, lgL, s, sb, inner);
      __syncthreads();
    }
    if (lgL - s == 2) {
      for (uint32_t sb = threadIdx.x; sb < (total >> 2); sb += NT) dif_group<F, TE, 2>(lds, lgL, s, sb, inner);
      __syncthreads();
    } else if (lgL - s == 1) {
      for (uint32_t sb = threadIdx.x; sb < (total >> 1); sb += NT) dif_group<F, TE, 1>(lds, lgL, s, sb, inner);
      __syncthreads();
    }
  }
}

// Pass over axis l of the view [A][L][Bn] (index = (a*L + l)*Bn + b), tile = one a, T adjacent b.
// dst may alias src (same positions).  After the transform, element (k, b) is multiplied by w_n^(tw_scale*k*b).
template <class F, uint32_t TE, uint32_t NT, int GM>
__global__ void __launch_bounds__(NT) k_ntt_strided(const char* src, char* dst, uint32_t lgL, uint32_t lgBn, uint32_t lgT,
                                                     uint32_t tw_scale, uint32_t lg_n, uint32_t lo_bits, const char* __restrict__ inner,
                                                     const char* __restrict__ tw_hi, const char* __restrict__ tw_lo,
                                                     const char* __restrict__ cs_hi, const char* __restrict__ cs_lo, int pre_coset,
                                                     const char* __restrict__ direct, NttSrc ext) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  src = ext.p ? ext.p + (size_t)blockIdx.y * ext.stride * 32 : src + ((size_t)blockIdx.y << (lg_n + 5)); dst += (size_t)blockIdx.y << (lg_n + 5);      // blockIdx.y: independent transform of a batch
  const uint32_t L = 1u << lgL, T = 1u << lgT, tiles_per_a = 1u << (lgBn - lgT);
  const uint32_t a = blockIdx.x / tiles_per_a, b0 = (blockIdx.x % tiles_per_a) << lgT;
  F::template fill<TE, NT>(lds, src, ext, lgL, L, T, pre_coset, cs_hi, cs_lo, lo_bits,
                           [=](uint32_t elem, uint32_t& t, uint32_t& l) { t = elem & (T - 1u); l = elem >> lgT; return ((((size_t)a << lgL) + l) << lgBn) + b0 + t; },
                           [=](uint32_t t, uint32_t l) { return (l << lgBn) + b0 + t; });      // coset_fft: only the first pass (A == 1, j = l*Bn + b)
  tile_dif<F, TE, NT, GM>(lds, lgL, T, inner);
  const uint32_t nmask = (lg_n >= 32) ? 0xffffffffu : ((1u << lg_n) - 1u);
  for (uint32_t e = threadIdx.x; e < T * L; e += NT) {
    const uint32_t t = e & (T - 1u), k = e >> lgT;
    typename F::Elem x = lds_load<F, TE>(lds, t * L + bitrev(k, lgL));
    const uint32_t b = b0 + t;
    const size_t gi = ((((size_t)a << lgL) + k) << lgBn) + b;
#if !(defined(ALEO_NTT_PROBE) && ALEO_NTT_PROBE == 2)
    if (direct) x = F::mul(x, F::load_entry(direct + gi * 32));     // the factor sits where its element goes: one coalesced 32-byte read instead of a product
    else x = F::mul(x, two_level<F>(tw_hi, tw_lo, (uint32_t)(((uint64_t)tw_scale * k * b) & nmask), lo_bits));
#endif
#if defined(ALEO_NTT_PROBE) && ALEO_NTT_PROBE == 3
    if (x.v[0] == 0x12345678u && x.v[5] == 0x1u)              // timing probe: (practically) no HBM writes
#endif
    store_fp<Fr>(dst + gi * 32, F::to_words(x));
  }
}

// Last pass: rows a = k1*n2 + k2 are contiguous (Bn == 1); tile = T adjacent k1 at one k2; output k of that row
// goes to natural position k1 + n1*(k2 + n2*k).  src != dst unless n1 == n2 == 1.
template <class F, uint32_t TE, uint32_t NT, int GM>
__global__ void __launch_bounds__(NT) k_ntt_final(const char* src, char* dst, uint32_t lgL, uint32_t lgN1, uint32_t lgN2, uint32_t lgT,
                                                   uint32_t lo_bits, const char* __restrict__ inner, const char* __restrict__ cs_hi, const char* __restrict__ cs_lo,
                                                   int pre_coset, int post_coset, int do_scale, typename F::ScaleArg scale, NttSrc ext) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  src = ext.p ? ext.p + (size_t)blockIdx.y * ext.stride * 32 : src + ((size_t)blockIdx.y << (lgL + lgN1 + lgN2 + 5)); dst += (size_t)blockIdx.y << (lgL + lgN1 + lgN2 + 5);
  const uint32_t L = 1u << lgL, T = 1u << lgT;
  const uint32_t tiles_k1 = 1u << (lgN1 - lgT);
  const uint32_t k2 = blockIdx.x / tiles_k1, k10 = (blockIdx.x % tiles_k1) << lgT;
  F::template fill<TE, NT>(lds, src, ext, lgL, L, T, pre_coset, cs_hi, cs_lo, lo_bits,
                           [=](uint32_t elem, uint32_t& t, uint32_t& l) { l = elem & (L - 1u); t = elem >> lgL; return (((((size_t)(k10 + t) << lgN2) + k2) << lgL) + l); },
                           [=](uint32_t, uint32_t l) { return l; });                           // single-pass coset_fft: j = l
  tile_dif<F, TE, NT, GM>(lds, lgL, T, inner);
  typename F::Elem sc;
#pragma unroll
  for (int i = 0; i < F::PLANES; ++i) sc.v[i] = scale.v[i];
  for (uint32_t e = threadIdx.x; e < T * L; e += NT) {
    const uint32_t t = e & (T - 1u), k = e >> lgT;
    typename F::Elem x = lds_load<F, TE>(lds, t * L + bitrev(k, lgL));
    const size_t o = (size_t)(k10 + t) + (((size_t)k2 + ((size_t)k << lgN2)) << lgN1);
    if (post_coset) x = F::mul(x, two_level<F>(cs_hi, cs_lo, (uint32_t)o, lo_bits));       // g^-o * n^-1
    else if (do_scale) x = F::mul(x, sc);
    else F::no_last_product(x);
#if defined(ALEO_NTT_PROBE) && ALEO_NTT_PROBE == 3
    if (x.v[0] == 0x12345678u && x.v[5] == 0x1u)
#endif
    F::store_final(dst, o, x, post_coset || do_scale);
  }
}

// direct[(k << lgBn) + b] = w_n^(k * b): the inter-pass factor of a two-pass transform, one entry per element (built once per
// (size, direction, form) on first use; 32 n bytes of HBM buy one product per element per transform)
template <class F>
__global__ void __launch_bounds__(256) k_build_direct(char* __restrict__ out, uint32_t lg_n, uint32_t lgBn, uint32_t lo_bits, const char* __restrict__ tw_hi,
                                                      const char* __restrict__ tw_lo) {
  const size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gi >> lg_n) return;
  const uint32_t k = (uint32_t)(gi >> lgBn), b = (uint32_t)(gi & (((size_t)1 << lgBn) - 1));
  const uint32_t nmask = (lg_n >= 32) ? 0xffffffffu : ((1u << lg_n) - 1u);
  F::store_final(out, gi, two_level<F>(tw_hi, tw_lo, (uint32_t)(((uint64_t)k * b) & nmask), lo_bits), true);
}

__global__ void __launch_bounds__(256) k_bitrev_copy(const char* __restrict__ src, char* __restrict__ dst, uint32_t lg_n) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ((size_t)1 << lg_n)) return;
  src += (size_t)blockIdx.y << (lg_n + 5); dst += (size_t)blockIdx.y << (lg_n + 5);
  uint32_t j = bitrev((uint32_t)i, lg_n);
  const uint4* s = (const uint4*)(src + i * 32); uint4* d = (uint4*)(dst + (size_t)j * 32);
  d[0] = s[0]; d[1] = s[1];
}

// ---- host side: tables -----------------------------------------------------------------------------
// One limb form's tables of one (size, direction).  Limbs32: Montgomery numbers of R = 2^256.  Limbs29: every entry times 2^5, i.e. in the Montgomery form
// of R = 2^261; packed 32-byte numbers except the inner twiddles (9 limbs at a 48-byte stride).  The set owns its device memory.
struct TableSet {
  DevTmp inner;                // w_{2048}^t, t < 1024            (inner butterflies; shorter transforms stride it)
  DevTmp tw_hi, tw_lo;         // w_n^(e_hi << lo_bits), w_n^(e_lo)
  DevTmp cs_hi, cs_lo;         // coset powers: g^(j_hi << lo_bits), g^(j_lo)        (inverse: g^-(...), g^-(j_lo) * n^-1)
  DevTmp direct;               // two-pass sizes: w_n^(k * b) at the position (k << lgBn) + b of the element it multiplies after pass 1; built on first use (direct_table)
  uint32_t direct_lgBn = 0;    // the pass split `direct` was built for
  uint32_t scale[9] = {};      // n^-1 in the form's limbs: applied at the final store of a plain inverse transform
};
struct NttTables {             // immutable once built, but for the lazy `direct` tables (under Device::mu)
  uint32_t lg_n = 0, lo_bits = 0;
  TableSet set[2];             // [Form::SET]
};

static int32_t upload(DevTmp& d, const void* p, size_t bytes) {
  int32_t rc = d.alloc(bytes);
  if (rc) return rc;
  HIPCHK(hipMemcpy(d.p, p, bytes, hipMemcpyHostToDevice));
  return ALEO_MI355X_OK;
}
static int32_t upload_fr(DevTmp& d, const std::vector<host::HFr>& v) { return upload(d, v.data(), v.size() * 32); }

static int32_t build_tables(NttTables* t, uint32_t lg_n, int direction) {
  using namespace host;
  t->lg_n = lg_n; t->lo_bits = (lg_n + 1) / 2;
  const uint32_t hi_bits = lg_n - t->lo_bits;
  HFr root; std::memcpy(root.l, FR_TWO_ADIC_ROOT_CANON, 32); root = HFr::to_mont(root);
  // w_n = TWO_ADIC_ROOT^(2^(47 - lg_n)); w_2048 likewise
  HFr wn = root; for (uint32_t i = lg_n; i < (uint32_t)FR_TWO_ADICITY; ++i) wn = HFr::sqr(wn);
  HFr w1k = root; for (uint32_t i = INNER_MAX_LG; i < (uint32_t)FR_TWO_ADICITY; ++i) w1k = HFr::sqr(w1k);
  HFr g = HFr::from_u64(FR_GENERATOR);
  HFr ninv = HFr::inv(HFr::from_u64((uint64_t)1 << lg_n));
  if (direction == ALEO_NTT_INVERSE) { wn = HFr::inv(wn); w1k = HFr::inv(w1k); g = HFr::inv(g); }
  const HFr lo_scale = direction == ALEO_NTT_INVERSE ? ninv : HFr::one();
  std::vector<HFr> inner(1024), hi((size_t)1 << hi_bits), lo((size_t)1 << t->lo_bits), chi((size_t)1 << hi_bits), clo((size_t)1 << t->lo_bits);
  inner[0] = HFr::one(); for (size_t i = 1; i < inner.size(); ++i) inner[i] = HFr::mul(inner[i - 1], w1k);
  auto fill = [&](std::vector<HFr>& v, HFr first, HFr step) { v[0] = first; for (size_t i = 1; i < v.size(); ++i) v[i] = HFr::mul(v[i - 1], step); };
  HFr wn_hi = wn, g_hi = g;
  for (uint32_t i = 0; i < t->lo_bits; ++i) { wn_hi = HFr::sqr(wn_hi); g_hi = HFr::sqr(g_hi); }
  fill(lo, HFr::one(), wn); fill(hi, HFr::one(), wn_hi);
  fill(clo, lo_scale, g); fill(chi, HFr::one(), g_hi);
  int32_t rc;
  TableSet& a = t->set[Limbs32::SET];
  std::memcpy(a.scale, ninv.l, 32);
  if ((rc = upload_fr(a.inner, inner))) return rc;
  if ((rc = upload_fr(a.tw_hi, hi))) return rc;
  if ((rc = upload_fr(a.tw_lo, lo))) return rc;
  if ((rc = upload_fr(a.cs_hi, chi))) return rc;
  if ((rc = upload_fr(a.cs_lo, clo))) return rc;
  // the 29-bit-limb set: x * 2^261 = (x * 2^256) * 2^5 — one host product by 32 per entry; the number itself is what is uploaded
  TableSet& b = t->set[Limbs29::SET];
  const HFr k32 = HFr::from_u64(32);
  auto form29 = [&](std::vector<HFr> v) { for (auto& e : v) e = HFr::mul(e, k32); return v; };
  if ((rc = upload_fr(b.tw_hi, form29(hi)))) return rc;
  if ((rc = upload_fr(b.tw_lo, form29(lo)))) return rc;
  if ((rc = upload_fr(b.cs_hi, form29(chi)))) return rc;
  if ((rc = upload_fr(b.cs_lo, form29(clo)))) return rc;
  auto limbs29 = [](const HFr& e, uint32_t* out) {           // canonical number -> 9 x 29-bit limbs
    for (int i = 0; i < 9; ++i) { const int bit = 29 * i, w = bit >> 6, sh = bit & 63; uint64_t x = e.l[w] >> sh; if (sh > 35 && w + 1 < 4) x |= e.l[w + 1] << (64 - sh); out[i] = (uint32_t)x & 0x1fffffffu; }
  };
  std::vector<uint32_t> in29(12 * inner.size(), 0);
  for (size_t i = 0; i < inner.size(); ++i) limbs29(HFr::mul(inner[i], k32), &in29[12 * i]);
  if ((rc = upload(b.inner, in29.data(), in29.size() * 4))) return rc;
  limbs29(HFr::mul(ninv, k32), b.scale);
  return ALEO_MI355X_OK;
}

// The n-entry inter-pass table of a two-pass size, built on the form's first such call and shared by all slots from then on.  The split it is built
// for is a function of lg_n alone ((lg_n + 1) / 2 whatever the tile) and is stored with it; nullptr for another split.
template <class F> static int32_t direct_table(Ctx* c, NttTables* t, uint32_t lgBn, hipStream_t s, const char** out) {
  TableSet& ts = t->set[F::SET];
  std::lock_guard<std::mutex> lk(c->dev->mu);
  if (!ts.direct.p) {
    int32_t rc = ts.direct.alloc((size_t)32 << t->lg_n);
    if (rc) return rc;
    hipLaunchKernelGGL(k_build_direct<F>, dim3((uint32_t)((((size_t)1 << t->lg_n) + 255) / 256)), dim3(256), 0, s, (char*)ts.direct.p, t->lg_n, lgBn, t->lo_bits,
                       (const char*)ts.tw_hi.p, (const char*)ts.tw_lo.p);
    HIPCHK(hipStreamSynchronize(s));           // once per (size, direction, form): later calls on other streams may use it at once
    ts.direct_lgBn = lgBn;
  }
  *out = ts.direct_lgBn == lgBn ? (const char*)ts.direct.p : nullptr;
  return ALEO_MI355X_OK;
}

// which kernel instances had their dynamic-LDS limit raised (Device::ntt_attr_mask: the limit is a property of (kernel, device))
enum : int { NTT_ATTR_TILE_2048 = 4, NTT_ATTR_TILE_4096 = 8 };

// One transform (or `batch` of them) through the passes of its plan on one kernel configuration.
template <class F, uint32_t TE, uint32_t NT, int GM>
static int32_t run_passes(Ctx* c, char* buf, char* tmp, uint32_t lg_n, uint32_t batch, NttTables* t, int pre_coset, int post_coset, int do_scale, hipStream_t s, NttSrc ext) {
  static_assert(TE == 4096 || TE == 2048 || TE == 512, "tile sizes with a kernel instance");
  constexpr uint32_t lgTE = TE == 4096 ? 12 : TE == 2048 ? 11 : 9;
  constexpr size_t lds_bytes = (size_t)TE * 4 * F::PLANES;
  if constexpr (lds_bytes > 64 * 1024) {
    constexpr int attr_bit = TE == 4096 ? NTT_ATTR_TILE_4096 : NTT_ATTR_TILE_2048;
    if (!(c->dev->ntt_attr_mask.load() & attr_bit)) {
      HIPCHK(hipFuncSetAttribute((const void*)k_ntt_strided<F, TE, NT, GM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
      HIPCHK(hipFuncSetAttribute((const void*)k_ntt_final<F, TE, NT, GM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
      c->dev->ntt_attr_mask.fetch_or(attr_bit);
    }
  }
  const NttPlan plan = plan_passes(lg_n, lgTE);
  if (!plan.npass) { g_last_error = "ntt: size beyond three passes of this tile"; return ALEO_MI355X_ERR_BAD_ARG; }
  const TableSet& ts = t->set[F::SET];
  const char* inner = (const char*)ts.inner.p; const char* twh = (const char*)ts.tw_hi.p; const char* twl = (const char*)ts.tw_lo.p;
  const char* csh = (const char*)ts.cs_hi.p; const char* csl = (const char*)ts.cs_lo.p;
  typename F::ScaleArg sc; std::memcpy(sc.v, ts.scale, sizeof sc.v);
  const char* direct = nullptr;
  if (plan.npass == 2 && lg_n >= 12 && lg_n <= F::DIRECT_MAX_LG) { int32_t rc = direct_table<F>(c, t, plan.pass[0].lgBn, s, &direct); if (rc) return rc; }
  for (uint32_t i = 0; i < plan.npass; ++i) {
    const NttPass& p = plan.pass[i];
    const char* src = p.src_tmp ? tmp : buf; char* dst = p.dst_tmp ? tmp : buf;
    const int pre = i == 0 ? pre_coset : 0; const NttSrc in = i == 0 ? ext : NttSrc{};      // the coset shift and the padded source belong to the first pass
    if (i + 1 < plan.npass) hipLaunchKernelGGL((k_ntt_strided<F, TE, NT, GM>), dim3(p.grid_x, batch), dim3(NT), lds_bytes, s, src, dst, p.lgL, p.lgBn, p.lgT, p.tw_scale, lg_n, t->lo_bits, inner, twh, twl, csh, csl, pre, direct, in);
    else hipLaunchKernelGGL((k_ntt_final<F, TE, NT, GM>), dim3(p.grid_x, batch), dim3(NT), lds_bytes, s, src, dst, p.lgL, p.lgN1, p.lgN2, p.lgT, t->lo_bits, inner, csh, csl, pre, post_coset, do_scale, sc, in);
  }
  return ALEO_MI355X_OK;
}

// dst[c][r] = src[r][c] for 32-byte elements (rows x cols -> cols x rows): the three layout changes of a 4-step transform (columns contiguous for the
// column transforms, rows for the row transforms, natural order out).  32 x 32-element tiles through LDS: both sides move 1-KiB runs.
__global__ void __launch_bounds__(256) k_transpose32(const char* __restrict__ src, char* __restrict__ dst, uint64_t rows, uint64_t cols) {
  __shared__ uint4 tile[32][33][2];
  const uint64_t r0 = (uint64_t)blockIdx.y * 32, c0 = (uint64_t)blockIdx.x * 32;
  const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;                     // 32 x 8 threads
  for (uint32_t j = ty; j < 32; j += 8) {
    const uint64_t r = r0 + j, c = c0 + tx;
    if (r < rows && c < cols) { const uint4* e = (const uint4*)(src + (r * cols + c) * 32); tile[j][tx][0] = e[0]; tile[j][tx][1] = e[1]; }
  }
  __syncthreads();
  for (uint32_t j = ty; j < 32; j += 8) {
    const uint64_t c = c0 + j, r = r0 + tx;
    if (r < rows && c < cols) { uint4* e = (uint4*)(dst + (c * rows + r) * 32); e[0] = tile[tx][j][0]; e[1] = tile[tx][j][1]; }
  }
}
int32_t fr_transpose(Ctx* c, void* d_dst, const void* d_src, uint64_t rows, uint64_t cols, hipStream_t s) {
  (void)c;
  if (!rows || !cols) return ALEO_MI355X_OK;
  if ((rows + 31) / 32 > 65535) { g_last_error = "fr_transpose: more than 2^21 rows"; return ALEO_MI355X_ERR_BAD_ARG; }
  hipLaunchKernelGGL(k_transpose32, dim3((uint32_t)((cols + 31) / 32), (uint32_t)((rows + 31) / 32)), dim3(256), 0, s, (const char*)d_src, (char*)d_dst, rows, cols);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

// ---- sharded (4-step) transform support: per-element factors over a 2-D block of the size-n index space -----------
// mode 0: x[r][c] *= w_n^((row0 + r) * (col0 + c))       (the twiddle between the column and the row transforms)
// mode 1: x[r][c] *= g^((row0 + r) * ld + col0 + c)      (coset shift of a block of the coefficient matrix)
// inverse direction: w^-1 / g^-1 (tables of the inverse domain; the n^-1 folded into its coset table is cancelled by K = n).
__global__ void __launch_bounds__(256) k_grid_scale(char* __restrict__ data, uint64_t rows, uint64_t cols, uint64_t row0, uint64_t col0, uint64_t ld,
                                                    int mode, uint32_t lg_n, uint32_t lo_bits, const char* __restrict__ hi, const char* __restrict__ lo,
                                                    int use_k, FrArg K) {
  const uint64_t total = rows * cols, nmask = ((uint64_t)1 << lg_n) - 1u;
  Fr k; for (int i = 0; i < 8; ++i) k.v[i] = K.v[i];
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t r = row0 + i / cols, c = col0 + i % cols;
    const uint32_t e = (uint32_t)((mode == 0 ? r * c : r * ld + c) & nmask);
    Fr f = two_level<Limbs32>(hi, lo, e, lo_bits);            // < 2r
    if (use_k) f = Fr::mul(f, k);
    Fr x = load_fp<Fr>(data + i * 32);
    store_fp<Fr>(data + i * 32, Fr::reduce(Fr::mul(x, f)));
  }
}

static int32_t get_tables(Ctx* c, uint32_t lg_n, int32_t direction, NttTables** out);

int32_t fr_grid_scale(Ctx* c, void* d_data, uint32_t lg_n, uint64_t rows, uint64_t cols, uint64_t row0, uint64_t col0, uint64_t ld, int32_t mode,
                      int32_t direction, hipStream_t s) {
  if (rows == 0 || cols == 0) return ALEO_MI355X_OK;
  NttTables* t = nullptr; int32_t rc;
  if ((rc = get_tables(c, lg_n, direction, &t))) return rc;
  FrArg K; std::memset(K.v, 0, 32); int use_k = 0;
  if (mode == 1 && direction == ALEO_NTT_INVERSE) {           // cs_lo of the inverse domain carries n^-1: multiply it back out
    host::HFr nn = host::HFr::from_u64((uint64_t)1 << lg_n); std::memcpy(K.v, nn.l, 32); use_k = 1;
  }
  const uint64_t total = rows * cols; const uint32_t grid = (uint32_t)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  const TableSet& ts = t->set[Limbs32::SET];
  const char* hi = (const char*)(mode == 0 ? ts.tw_hi.p : ts.cs_hi.p); const char* lo = (const char*)(mode == 0 ? ts.tw_lo.p : ts.cs_lo.p);
  hipLaunchKernelGGL(k_grid_scale, dim3(grid), dim3(256), 0, s, (char*)d_data, rows, cols, row0, col0, ld, mode, lg_n, t->lo_bits, hi, lo, use_k, K);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

static int32_t get_tables(Ctx* c, uint32_t lg_n, int32_t direction, NttTables** out) {
  uint64_t key = ((uint64_t)lg_n << 1) | (uint64_t)direction;
  std::lock_guard<std::mutex> lk(c->dev->mu);       // tables are shared by all slots and immutable once built
  auto it = c->dev->ntt_tables.find(key);
  if (it == c->dev->ntt_tables.end()) {
    NttTables* t = new NttTables();
    int32_t rc = build_tables(t, lg_n, direction);
    if (rc) { delete t; return rc; }                // frees what was uploaded before the failure
    c->dev->ntt_tables[key] = t; *out = t;
  } else *out = it->second;
  return ALEO_MI355X_OK;
}

static int32_t ntt_run_chunk(Ctx* c, void* d_inout, uint32_t lg_n, uint32_t batch, int32_t order, int32_t direction, int32_t type, hipStream_t s, NttSrc ext = NttSrc{});
// `batch` independent transforms of 2^lg_n elements each, contiguous in d_inout (blockIdx.y walks them)
int32_t ntt_run(Ctx* c, void* d_inout, uint32_t lg_n, size_t batch_total, int32_t order, int32_t direction, int32_t type, hipStream_t s) {
  if (lg_n == 0 || batch_total == 0) return ALEO_MI355X_OK;     // n = 1: every variant is the identity (g^0 = 1, 1^-1 = 1)
  const size_t n = (size_t)1 << lg_n;
  for (size_t b0 = 0; b0 < batch_total; b0 += 32768) {            // gridDim.y <= 65535
    const uint32_t batch = (uint32_t)(batch_total - b0 < 32768 ? batch_total - b0 : 32768);
    int32_t rcb = ntt_run_chunk(c, (char*)d_inout + b0 * n * 32, lg_n, batch, order, direction, type, s);
    if (rcb) return rcb;
  }
  return ALEO_MI355X_OK;
}

// The same with the first pass reading transform b's coefficients from d_src + b * src_stride elements, zero beyond src_len (natural order in and out; d_out
// must not overlap d_src): what `memset + copy + ntt_run` did in three or more launches.
int32_t ntt_run_from(Ctx* c, void* d_out, const void* d_src, size_t src_stride, size_t src_len, uint32_t lg_n, size_t batch_total, int32_t direction, int32_t type, hipStream_t s) {
  if (batch_total == 0) return ALEO_MI355X_OK;
  const size_t n = (size_t)1 << lg_n;
  if (src_len > n || src_stride >= (1ull << 32) || !d_src || !d_out) { g_last_error = "ntt_run_from: bad argument"; return ALEO_MI355X_ERR_BAD_ARG; }
  if (lg_n == 0) { for (size_t b = 0; b < batch_total; ++b) { if (src_len) HIPCHK(hipMemcpyAsync((char*)d_out + b * 32, (const char*)d_src + b * src_stride * 32, 32, hipMemcpyDeviceToDevice, s)); else HIPCHK(hipMemsetAsync((char*)d_out + b * 32, 0, 32, s)); } return ALEO_MI355X_OK; }
  for (size_t b0 = 0; b0 < batch_total; b0 += 32768) {
    const uint32_t batch = (uint32_t)(batch_total - b0 < 32768 ? batch_total - b0 : 32768);
    NttSrc ext; ext.p = (const char*)d_src + b0 * src_stride * 32; ext.len = (uint32_t)src_len; ext.stride = (uint32_t)src_stride;
    const int32_t rcb = ntt_run_chunk(c, (char*)d_out + b0 * n * 32, lg_n, batch, ALEO_NTT_ORDER_NN, direction, type, s, ext);
    if (rcb) return rcb;
  }
  return ALEO_MI355X_OK;
}

static int32_t ntt_run_chunk(Ctx* c, void* d_inout, uint32_t lg_n, uint32_t batch, int32_t order, int32_t direction, int32_t type, hipStream_t s, NttSrc ext) {
  const size_t n = (size_t)1 << lg_n, bytes = n * 32 * batch;
  int32_t rc;
  NttTables* t = nullptr;
  if ((rc = get_tables(c, lg_n, direction, &t))) return rc;
  return with_scratch(c, c->ntt_tmp, bytes, s, [&]() -> int32_t {      // ordered after the slot's previous asynchronous user
    char* buf = (char*)d_inout; char* tmp = c->ntt_tmp.as<char>();
    const bool in_rev = (order == ALEO_NTT_ORDER_RN || order == ALEO_NTT_ORDER_RR), out_rev = (order == ALEO_NTT_ORDER_NR || order == ALEO_NTT_ORDER_RR);
    const dim3 gperm((uint32_t)((n + 255) / 256), batch);
    if (in_rev) {
      hipLaunchKernelGGL(k_bitrev_copy, gperm, dim3(256), 0, s, buf, tmp, lg_n);
      HIPCHK(hipMemcpyAsync(buf, tmp, bytes, hipMemcpyDeviceToDevice, s));
    }
    const int coset = (type == ALEO_NTT_COSET), inv = (direction == ALEO_NTT_INVERSE);
    const int pre_coset = coset && !inv, post_coset = coset && inv, do_scale = inv && !coset;   // cs_lo carries n^-1 for coset_ifft
    switch (choose_form(lg_n, batch)) {
      case NttForm::Latency512: rc = run_passes<Limbs32, 512, 256, 1>(c, buf, tmp, lg_n, batch, t, pre_coset, post_coset, do_scale, s, ext); break;
      case NttForm::Tile4096: rc = run_passes<Limbs29, 4096, 512, 3>(c, buf, tmp, lg_n, batch, t, pre_coset, post_coset, do_scale, s, ext); break;
      case NttForm::Tile2048: rc = run_passes<Limbs29, 2048, 256, 3>(c, buf, tmp, lg_n, batch, t, pre_coset, post_coset, do_scale, s, ext); break;
    }
    if (rc) return rc;
    if (out_rev) {
      hipLaunchKernelGGL(k_bitrev_copy, gperm, dim3(256), 0, s, buf, tmp, lg_n);
      HIPCHK(hipMemcpyAsync(buf, tmp, bytes, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipGetLastError());
    return ALEO_MI355X_OK;
  });
}

}  // namespace aleo_mi355x

