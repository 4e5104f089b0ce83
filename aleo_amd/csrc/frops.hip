// frops.hip — field-only vector kernels around the two operators: element-wise Fr products /
// sums / differences of evaluation vectors and batch inversion, on data that already lives in HBM between an NTT and
// the next NTT / commitment.
//
// Replaces (on the device) the loops snarkVM 0.14.5 runs on the CPU between FFTs in Varuna's rounds [UPSTREAM-RECALL]:
//   algorithms/src/fft/evaluations.rs      Evaluations::{mul_assign, add_assign, sub_assign}  (pointwise on a domain)
//   fields/src/traits/field.rs / lib.rs    snarkvm_fields::batch_inversion (Montgomery's trick; zeros stay zero)
// reached from the same call sites as the NTT: /root/reference/rust/src/program/execute.rs:74,177, transfer.rs:99.
//
// Element-wise ops are HBM-bound (96 algorithmic bytes per element against one 305-instruction product): 16-byte
// coalesced accesses, one element per lane, grid-stride.  Batch inversion: every lane owns a strided subsequence (so a
// wave's accesses stay contiguous), keeps prefix products in an HBM scratch vector and shares ONE Fermat inversion
// (a^(r-2), ~380 products) over its K elements: 3 + 380/K products per element.
#include "frops.h"
#include "fr_kernels.h"
#include "chacha.h"
#include "host_field.hpp"

namespace aleo_mi355x {

template <int OP>
__global__ void __launch_bounds__(256) k_fr_vec_op(char* dst, const char* a, const char* b, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    Fr x = load_fp<Fr>(a + i * 32), y = load_fp<Fr>(b + i * 32), r;
    if constexpr (OP == 0) r = Fr::mul(x, y);               // canonical inputs: < 2r
    else if constexpr (OP == 1) r = Fr::add(x, y);          // < 2r
    else r = Fr::sub<1>(x, y);                              // x + r - y < 2r
    store_fp<Fr>(dst + i * 32, Fr::cond_sub<1>(r));
  }
}

__device__ __constant__ uint32_t FR_R_MINUS_2[8] = {0xffffffffu, 0x0a117fffu, 0xd0000001u, 0x59aa76feu, 0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu};
__device__ __noinline__ void fr_mul_ni(Fr* r, const Fr* a, const Fr* b) { *r = Fr::mul(*a, *b); }
__device__ __noinline__ void fr_inverse_ni(Fr* io) {       // a^(r-2); a < 2r, result < 2r
  Fr a = *io, acc = Fr::one();
  for (int bit = 252; bit >= 0; --bit) {
    fr_mul_ni(&acc, &acc, &acc);
    if ((FR_R_MINUS_2[bit >> 5] >> (bit & 31)) & 1u) fr_mul_ni(&acc, &acc, &a);
  }
  *io = acc;
}

// lane t owns elements t, t + T, t + 2T, ... (T = total lanes)
__global__ void __launch_bounds__(256) k_fr_batch_inverse(char* __restrict__ data, char* __restrict__ prefix, size_t n, size_t T) {
  size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  Fr prod = Fr::one();
  for (size_t i = t; i < n; i += T) {
    store_fp<Fr>(prefix + i * 32, prod);                      // product of this lane's earlier non-zero elements (< 2r)
    Fr v = load_fp<Fr>(data + i * 32);
    if (!v.is_zero_raw()) prod = Fr::mul(prod, v);
  }
  fr_inverse_ni(&prod);
  size_t cnt = (n - t + T - 1) / T;
  for (size_t k = cnt; k-- > 0;) {
    size_t i = t + k * T;
    Fr v = load_fp<Fr>(data + i * 32);
    if (v.is_zero_raw()) continue;                            // batch_inversion leaves zeros in place
    Fr pre = load_fp<Fr>(prefix + i * 32);
    Fr inv = Fr::mul(prod, pre);
    prod = Fr::mul(prod, v);
    store_fp<Fr>(data + i * 32, Fr::reduce(inv));
  }
}

int32_t fr_vec_op(Ctx* c, void* d_dst, const void* d_a, const void* d_b, size_t n, int32_t op, hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  if (op < 0 || op > 2) { g_last_error = "fr_vec_op: unknown op"; return ALEO_MI355X_ERR_BAD_ARG; }
  return launch(op == 0 ? k_fr_vec_op<0> : op == 1 ? k_fr_vec_op<1> : k_fr_vec_op<2>, grid_for(n, 8192), dim3(256), s, (char*)d_dst, (const char*)d_a, (const char*)d_b, n);
}

int32_t fr_batch_inverse(Ctx* c, void* d_inout, size_t n, hipStream_t s) {
  if (n == 0) return ALEO_MI355X_OK;
  // ~64 elements per lane keeps the shared inversion at ~6 products per element; small inputs use fewer per lane
  size_t T = (n + 63) / 64; if (T < 4096) T = n < 4096 ? n : 4096;
  return with_scratch(c, c->ntt_tmp, n * 32, s, [&] { return launch(k_fr_batch_inverse, dim3((uint32_t)((T + 255) / 256)), dim3(256), s, (char*)d_inout, c->ntt_tmp.as<char>(), n, T); });
}

// dst[i] = c0 + c1 * a[i] + c2 * b[i] with host-side constants (Montgomery): the scalar-times-vector, shifted and blended forms
// of the AHP rounds (alpha - h_i before a batch inversion, eta-weighted sums of z_a, z_b, the linear combinations opened at
// beta and gamma) [UPSTREAM-RECALL: snark/varuna/ahp/prover/round_functions/{second,third,fourth}.rs run these as rayon maps].
template <bool HAS_A, bool HAS_B>
__global__ void __launch_bounds__(256) k_fr_lin(char* dst, size_t n, FrK k0, FrK k1, const char* a, FrK k2, const char* b) {
  const Fr c0 = fr_arg(k0), c1 = fr_arg(k1), c2 = fr_arg(k2);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    Fr r = c0;                                                                                    // canonical: < r
    if constexpr (HAS_A) r = add_lt2r(r, Fr::mul(c1, load_fp<Fr>(a + i * 32)));    // < 3r -> < 2r
    if constexpr (HAS_B) r = add_lt2r(r, Fr::mul(c2, load_fp<Fr>(b + i * 32)));    // < 4r -> < 2r
    store_fp<Fr>(dst + i * 32, Fr::cond_sub<1>(r));
  }
}

int32_t fr_lin(Ctx* c, void* d_dst, size_t n, const void* c0, const void* c1, const void* d_a, const void* c2, const void* d_b, hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  if (d_a && !c1) { g_last_error = "fr_lin: a without c1"; return ALEO_MI355X_ERR_BAD_ARG; }
  if (d_b && !c2) { g_last_error = "fr_lin: b without c2"; return ALEO_MI355X_ERR_BAD_ARG; }
  const char* a = (const char*)d_a; const char* b = (const char*)d_b;
  return launch(a ? (b ? k_fr_lin<true, true> : k_fr_lin<true, false>) : (b ? k_fr_lin<false, true> : k_fr_lin<false, false>), grid_for(n, 8192), dim3(256), s,
                (char*)d_dst, n, c0 ? load_k(c0) : FrK{}, a ? load_k(c1) : FrK{}, a, b ? load_k(c2) : FrK{}, b);
}

// dst[i] = c0 [i == 0] + sum_j coeff_j * term_j[i] over up to LC_MAX ragged terms (term j ends at len_j): the linear combinations a
// proof opens at beta and gamma, and the delta-weighted sum of the fourth round, in one pass over the data.
static constexpr uint32_t LC_MAX = 28;
struct LcArgs { const char* p[LC_MAX]; size_t n[LC_MAX]; FrK k[LC_MAX]; uint32_t terms; };
__global__ void __launch_bounds__(256) k_fr_lincomb(char* dst, size_t n, LcArgs a, FrK k0) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    Fr r = i == 0 ? fr_arg(k0) : Fr::zero();
    for (uint32_t j = 0; j < a.terms; ++j)
      if (i < a.n[j]) r = add_lt2r(r, Fr::mul(fr_arg(a.k[j]), load_fp<Fr>(a.p[j] + i * 32)));      // < 4r -> < 2r
    store_fp<Fr>(dst + i * 32, Fr::cond_sub<1>(r));
  }
}
int32_t fr_lincomb(Ctx* c, void* d_dst, size_t n, const void* c0, const void* const* d_terms, const size_t* lens, const void* coeffs, size_t k, hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  if (k > LC_MAX) { g_last_error = "fr_lincomb: more than 28 terms in one call"; return ALEO_MI355X_ERR_BAD_ARG; }
  LcArgs a{}; a.terms = (uint32_t)k;
  for (size_t j = 0; j < k; ++j) {
    if (!d_terms[j] && lens[j]) { g_last_error = "fr_lincomb: null term"; return ALEO_MI355X_ERR_BAD_ARG; }
    a.p[j] = (const char*)d_terms[j]; a.n[j] = lens[j] < n ? lens[j] : n; a.k[j] = load_k((const char*)coeffs + 32 * j);
  }
  return launch(k_fr_lincomb, grid_for(n, 8192), dim3(256), s, (char*)d_dst, n, a, c0 ? load_k(c0) : FrK{});
}

// dst[i] += src[i mod n_src] (n_src a power of two dividing n): multiplication of a block of n_src coefficients by 1 + X^n_src + X^(2 n_src) + ...,
// the selector v_{H*} / v_H that puts a smaller circuit's remainder on the largest constraint domain of a proof (varuna_proof.hip).
__global__ void __launch_bounds__(256) k_fr_add_tiled(char* dst, size_t n, const char* __restrict__ src, size_t mask) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    store_fp<Fr>(dst + i * 32, Fr::cond_sub<1>(Fr::add(load_fp<Fr>(dst + i * 32), load_fp<Fr>(src + (i & mask) * 32))));      // canonical inputs: < 2r
}
int32_t fr_add_tiled(Ctx* c, void* d_dst, size_t n, const void* d_src, size_t n_src, hipStream_t s) {
  (void)c;
  if (!n_src || (n_src & (n_src - 1)) || n % n_src) { g_last_error = "fr_add_tiled: block size must be a power of two dividing n"; return ALEO_MI355X_ERR_BAD_ARG; }
  if (n == 0) return ALEO_MI355X_OK;
  return launch(k_fr_add_tiled, grid_for(n, 8192), dim3(256), s, (char*)d_dst, n, (const char*)d_src, n_src - 1);
}

// dst = (a - b) * m element-wise (the witness polynomial's values: (z - x̂) / v_X off X)
__global__ void __launch_bounds__(256) k_fr_sub_mul(char* __restrict__ dst, const char* __restrict__ a, const char* __restrict__ b, const char* __restrict__ m, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const Fr d = Fr::cond_sub<1>(Fr::sub<1>(load_fp<Fr>(a + i * 32), load_fp<Fr>(b + i * 32)));
    store_fp<Fr>(dst + i * 32, Fr::cond_sub<1>(Fr::mul(d, load_fp<Fr>(m + i * 32))));
  }
}
int32_t fr_sub_mul(Ctx* c, void* d_dst, const void* d_a, const void* d_b, const void* d_m, size_t n, hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  return launch(k_fr_sub_mul, grid_for(n, 8192), dim3(256), s, (char*)d_dst, (const char*)d_a, (const char*)d_b, (const char*)d_m, n);
}

// dst[r][i] = k_r * src[i], r < rows <= 4 (the eta-scaled copies of u_H(alpha, .) the transpose product reads)
struct FrK4 { FrK k[4]; };
__global__ void __launch_bounds__(256) k_fr_scale_rows(char* __restrict__ dst, const char* __restrict__ src, size_t n, uint32_t rows, FrK4 K) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const Fr x = load_fp<Fr>(src + i * 32);
    for (uint32_t r = 0; r < rows; ++r) store_fp<Fr>(dst + ((size_t)r * n + i) * 32, Fr::reduce(Fr::mul(fr_arg(K.k[r]), x)));
  }
}
int32_t fr_scale_rows(Ctx* c, void* d_dst, const void* d_src, size_t n, size_t rows, const void* consts_mont, hipStream_t s) {
  (void)c;
  if (n == 0 || rows == 0) return ALEO_MI355X_OK;
  if (rows > 4) { g_last_error = "fr_scale_rows: at most 4 rows"; return ALEO_MI355X_ERR_BAD_ARG; }
  FrK4 K{}; std::memcpy(K.k, consts_mont, rows * 32);
  return launch(k_fr_scale_rows, grid_for(n, 8192), dim3(256), s, (char*)d_dst, (const char*)d_src, n, (uint32_t)rows, K);
}

// up to 8 single elements gathered into consecutive 32-byte slots of dst (device memory, or the device pointer of pinned host memory: a read-back without a copy launch each)
struct PickArgs { const char* src[8]; };
__global__ void k_fr_pick(char* __restrict__ dst, PickArgs a, uint32_t count) {
  const uint32_t t = threadIdx.x;
  if (t < count * 8) ((uint32_t*)dst)[t] = ((const uint32_t*)a.src[t >> 3])[t & 7];
}
int32_t fr_pick(Ctx* c, void* dst_devptr, const void* const* d_src, size_t count, hipStream_t s) {
  (void)c;
  if (count == 0) return ALEO_MI355X_OK;
  if (count > 8) { g_last_error = "fr_pick: at most 8 elements"; return ALEO_MI355X_ERR_BAD_ARG; }
  PickArgs a{}; for (size_t i = 0; i < count; ++i) a.src[i] = (const char*)d_src[i];
  return launch(k_fr_pick, dim3(1), dim3(64), s, (char*)dst_devptr, a, (uint32_t)count);
}

// ---- geometric sequences and gathers (with the batched evaluation of fr_divide.hip): what lets the AHP rounds run without a single field inversion on the device ----
// u_H(a, X) = (v_H(a) - v_H(X)) / (a - X) = sum_k a^(|H|-1-k) X^k, so the polynomial r(alpha, X) IS the reversed powers of alpha and its
// values v_H(alpha) / (alpha - h) over H are one NTT of them; the third round's 1 / ((alpha - row)(beta - col)) are then two gathers from
// those tables by the row / column index of every non-zero entry [UPSTREAM-RECALL: snarkVM gets the same values through batch inversions
// in round_functions/{second,third}.rs].
static constexpr uint32_t POW_K = 16;
// dst[k] = first * ratio^k: every lane raises ratio to its first index, then walks POW_K consecutive elements
__global__ void __launch_bounds__(256) k_fr_powers(char* __restrict__ dst, size_t n, FrK kfirst, FrK kratio) {
  const size_t lo = ((size_t)blockIdx.x * 256 + threadIdx.x) * POW_K;
  if (lo >= n) return;
  const Fr ratio = fr_arg(kratio);
  Fr x = ratio; fr_pow_u64_ni(&x, lo);
  x = Fr::mul(x, fr_arg(kfirst));
  for (uint32_t k = 0; k < POW_K && lo + k < n; ++k) {
    store_fp<Fr>(dst + (lo + k) * 32, Fr::reduce(x));
    x = Fr::mul(x, ratio);
  }
}
// The latency form for sequences of up to 2^26 elements (the prover's r(alpha, X), r(beta, X): 2^15 elements took 29 us as ~30 dependent products per lane for
// the lane's starting power + 16 for its walk): the squarings ratio^(4 2^i) come from the host (28 constants by value), a lane multiplies the ones its index
// selects (no squaring on the device: ~lg(n) / 2 products) and walks 4 elements.
static constexpr uint32_t POW_KS = 4, POW_SQ = 24;
struct FrSq { FrK v[POW_SQ]; };
__global__ void __launch_bounds__(256) k_fr_powers_fast(char* __restrict__ dst, uint32_t n, FrK kfirst, FrK kratio, FrSq sq) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x, lo = t * POW_KS;
  if (lo >= n) return;
  Fr x = fr_arg(kfirst);
  for (uint32_t i = 0, b = t; b; ++i, b >>= 1) if (b & 1u) x = Fr::mul(x, fr_arg(sq.v[i]));      // first * ratio^(4 t)
  const Fr ratio = fr_arg(kratio);
  for (uint32_t k = 0; k < POW_KS && lo + k < n; ++k) {
    store_fp<Fr>(dst + (size_t)(lo + k) * 32, Fr::reduce(x));
    x = Fr::mul(x, ratio);
  }
}
int32_t fr_powers(Ctx* c, void* d_dst, size_t n, const void* first, const void* ratio, hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  if (n <= ((size_t)POW_KS << POW_SQ)) {
    FrSq sq; host::HFr r; std::memcpy(r.l, ratio, 32);
    r = host::HFr::sqr(host::HFr::sqr(r));                   // ratio^4
    for (uint32_t i = 0; i < POW_SQ; ++i) { sq.v[i] = load_k(r.l); r = host::HFr::sqr(r); }
    const size_t lanes = (n + POW_KS - 1) / POW_KS;
    return launch(k_fr_powers_fast, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), s, (char*)d_dst, (uint32_t)n, load_k(first), load_k(ratio), sq);
  }
  const size_t lanes = (n + POW_K - 1) / POW_K;
  return launch(k_fr_powers, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), s, (char*)d_dst, n, load_k(first), load_k(ratio));
}

// dst[i] = scale[i] * t1[idx1[i]] * t2[idx2[i]]   (scale and the second table optional)
template <bool HAS_SCALE, bool HAS_T2>
__global__ void __launch_bounds__(256) k_fr_gather_mul(char* __restrict__ dst, size_t n, const char* scale, const char* __restrict__ t1,
                                                       const uint32_t* __restrict__ idx1, const char* __restrict__ t2, const uint32_t* __restrict__ idx2) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    Fr r = load_fp<Fr>(t1 + (size_t)idx1[i] * 32);
    if constexpr (HAS_T2) r = Fr::mul(r, load_fp<Fr>(t2 + (size_t)idx2[i] * 32));
    if constexpr (HAS_SCALE) r = Fr::mul(r, load_fp<Fr>(scale + i * 32));
    store_fp<Fr>(dst + i * 32, Fr::reduce(r));
  }
}
int32_t fr_gather_mul(Ctx* c, void* d_dst, size_t n, const void* d_scale, const void* d_t1, const void* d_idx1, const void* d_t2, const void* d_idx2, hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  const char* sc = (const char*)d_scale; const char* t2 = (const char*)d_t2;
  return launch(sc ? (t2 ? k_fr_gather_mul<true, true> : k_fr_gather_mul<true, false>) : (t2 ? k_fr_gather_mul<false, true> : k_fr_gather_mul<false, false>), grid_for(n, 16384), dim3(256), s,
                (char*)d_dst, n, sc, (const char*)d_t1, (const uint32_t*)d_idx1, t2, (const uint32_t*)d_idx2);
}

// The same for up to three index ranges in ONE launch (the third round's f_A, f_B, f_C: three short launches were three times the ~4.5 us launch floor)
struct GatherMul3 { char* dst[3]; const char* scale[3]; const uint32_t* idx1[3]; const uint32_t* idx2[3]; uint32_t n[3]; uint32_t cnt; };
__global__ void __launch_bounds__(256) k_fr_gather_mul3(GatherMul3 a, const char* __restrict__ t1, const char* __restrict__ t2) {
  const uint32_t total = a.n[0] + a.n[1] + a.n[2];
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
    const uint32_t m = g < a.n[0] ? 0u : (g < a.n[0] + a.n[1] ? 1u : 2u); const size_t i = g - (m == 0 ? 0u : (m == 1 ? a.n[0] : a.n[0] + a.n[1]));
    Fr r = Fr::mul(load_fp<Fr>(t1 + (size_t)a.idx1[m][i] * 32), load_fp<Fr>(t2 + (size_t)a.idx2[m][i] * 32));
    r = Fr::mul(r, load_fp<Fr>(a.scale[m] + i * 32));
    store_fp<Fr>(a.dst[m] + i * 32, Fr::reduce(r));
  }
}
int32_t fr_gather_mul3(Ctx* c, void* const* d_dst, const size_t* n, const void* const* d_scale, const void* d_t1, const void* const* d_idx1, const void* d_t2, const void* const* d_idx2, uint32_t count, hipStream_t s) {
  (void)c;
  if (count == 0 || count > 3) { g_last_error = "fr_gather_mul3: one to three ranges"; return ALEO_MI355X_ERR_BAD_ARG; }
  GatherMul3 a{}; a.cnt = count; size_t total = 0;
  for (uint32_t m = 0; m < count; ++m) {
    if (n[m] >= (1ull << 31)) { g_last_error = "fr_gather_mul3: range too long"; return ALEO_MI355X_ERR_BAD_ARG; }
    a.dst[m] = (char*)d_dst[m]; a.scale[m] = (const char*)d_scale[m]; a.idx1[m] = (const uint32_t*)d_idx1[m]; a.idx2[m] = (const uint32_t*)d_idx2[m]; a.n[m] = (uint32_t)n[m]; total += n[m];
  }
  if (total == 0) return ALEO_MI355X_OK;
  if (total >= (1ull << 32)) { g_last_error = "fr_gather_mul3: ranges too long"; return ALEO_MI355X_ERR_BAD_ARG; }
  return launch(k_fr_gather_mul3, grid_for(total, 16384), dim3(256), s, a, (const char*)d_t1, (const char*)d_t2);
}

// ---- prover randomness generated where it is used ------------------------------------------------------------------------------
// Element i of the stream under the proof's 32-byte seed: ChaCha20 in counter mode with rejection sampling below r (chacha.h).
// A counter-based definition: any element can be produced anywhere (the host draws the handful of blinding scalars it needs, the device
// the 3|H| mask coefficients) [UPSTREAM-RECALL: snarkVM draws Fr::rand from the caller's CSPRNG in prover/round_functions/first.rs].
__global__ void __launch_bounds__(256) k_fr_random(char* __restrict__ dst, size_t n, Seed32 seed, uint64_t first, int mont) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    Fr v; chacha_fr(v.v, seed.w, first + i);                    // chacha.h: one ChaCha20 block per attempt, accepted with probability 0.83
    if (mont) v = Fr::to_mont(v);
    store_fp<Fr>(dst + i * 32, v);
  }
}
int32_t fr_random(Ctx* c, void* d_dst, size_t n, const uint8_t* seed32, uint64_t first, int32_t mont, hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  Seed32 sd; std::memcpy(sd.w, seed32, 32);
  return launch(k_fr_random, grid_for(n, 8192), dim3(256), s, (char*)d_dst, n, sd, first, mont ? 1 : 0);
}

// dst[pos[v]] = to_mont(src[v]): the assignment (canonical, variable order) laid out on H in Montgomery form — dst zeroed by the caller.
// An entry that is not below r (the Montgomery product assumes bounded inputs) raises *flag: the caller reads it with its next small read-back.
__global__ void __launch_bounds__(256) k_scatter_to_mont(char* __restrict__ dst, const char* __restrict__ src, const uint32_t* __restrict__ pos, size_t n, uint32_t* flag) {
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
    const Fr x = load_fp<Fr>(src + v * 32);
    bool lt = false;
    for (int k = 7; k >= 0; --k) { const uint32_t m = FrParams::P.v[k]; if (x.v[k] != m) { lt = x.v[k] < m; break; } }
    if (!lt && flag) atomicOr(flag, 1u);
    store_fp<Fr>(dst + (size_t)pos[v] * 32, Fr::to_mont(x));
  }
}
int32_t fr_scatter_to_mont(Ctx* c, void* d_dst, const void* d_src, const void* d_pos, size_t n, void* d_flag, hipStream_t s) {
  (void)c;
  if (!n) return ALEO_MI355X_OK;
  return launch(k_scatter_to_mont, grid_for(n, 8192), dim3(256), s, (char*)d_dst, (const char*)d_src, (const uint32_t*)d_pos, n, (uint32_t*)d_flag);
}

// ---- element-wise products (parity tests pin the device arithmetic with these) -------------------
template <class F, bool SQR> __global__ void __launch_bounds__(256) k_fp_mul(char* r, const char* a, const char* b, uint32_t n) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  constexpr int bytes = F::N * 4;
  F x = load_fp<F>(a + (size_t)i * bytes), y = load_fp<F>(b + (size_t)i * bytes);
  store_fp<F>(r + (size_t)i * bytes, F::reduce(SQR ? F::sqr(x) : F::mul(x, y)));
}
template <class F> static int32_t launch_fp_mul(Ctx* c, void* r, const void* a, const void* b, size_t n) {
  constexpr size_t bytes = F::N * 4;
  if (n == 0) return ALEO_MI355X_OK;
  int32_t rc; if ((rc = c->scalars_stage.reserve(3 * n * bytes))) return rc;
  char* da = c->scalars_stage.as<char>(); char* db = da + n * bytes; char* dr = db + n * bytes;
  HIPCHK(hipMemcpyAsync(da, a, n * bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(db, b, n * bytes, hipMemcpyHostToDevice, c->stream));
  if (a == b)     // same host buffer for both operands: pin the dedicated squaring block instead of the general product
    hipLaunchKernelGGL((k_fp_mul<F, true>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, dr, da, db, (uint32_t)n);
  else
    hipLaunchKernelGGL((k_fp_mul<F, false>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, dr, da, db, (uint32_t)n);
  HIPCHK(hipMemcpyAsync(r, dr, n * bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}
int32_t launch_fq_mul(Ctx* c, void* r, const void* a, const void* b, size_t n) { return launch_fp_mul<Fq>(c, r, a, b, n); }
int32_t launch_fr_mul(Ctx* c, void* r, const void* a, const void* b, size_t n) { return launch_fp_mul<Fr>(c, r, a, b, n); }

}  // namespace aleo_mi355x
