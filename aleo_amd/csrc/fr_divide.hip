// fr_divide.hip — division by (X - z): the witness polynomial of a KZG10 opening; and p_q(z_q) for a batch of polynomials, the same scan stopped early.
// Replaces snarkVM 0.14.5 algorithms/src/polycommit/kzg10  KZG10::compute_witness_polynomial / open  [UPSTREAM-RECALL]:
// w(X) = (p(X) - p(z)) / (X - z), followed by the commitment to w (SURVEY.md §2c polycommit row; the two opening MSMs of row a6).
// Synthetic division is the recurrence s_j = p_j + z * s_(j+1) (s_n = 0): w_(j-1) = s_j and p(z) = s_0.  A linear recurrence
// with a constant multiplier is a suffix scan, done in three levels with the multipliers z^16, (z^16)^256, ...:
//   k_div_blocks_many   every lane folds its 16 coefficients (Horner), every 256-lane block folds its lanes -> E_b
//   k_div_carries_many  one block: carry C_b into every block = tail of the polynomial behind it, from the E_b
//   k_div_finish_many   every block scans its lanes' values seeded with C_b, every lane replays its 16 steps and writes w
// 96 algorithmic bytes per coefficient (p read twice, w written once); values stay lazily reduced below 4r (fp.h).
#include "frops.h"
#include "fr_kernels.h"

namespace aleo_mi355x {

static constexpr uint32_t DIV_K = 16, DIV_B = 256, DIV_TILE = DIV_K * DIV_B;
__device__ __forceinline__ void lds_put(uint32_t* l, uint32_t t, const Fr& a) { for (int i = 0; i < 8; ++i) l[i * DIV_B + t] = a.v[i]; }
__device__ __forceinline__ Fr lds_get(const uint32_t* l, uint32_t t) { Fr r; for (int i = 0; i < 8; ++i) r.v[i] = l[i * DIV_B + t]; return r; }
// value of the lane's 16 coefficients at z: sum_k p[lo + k] z^k (coefficients past n are zero); result < 3r
__device__ __forceinline__ Fr div_lane_fold(const char* __restrict__ p, size_t lo, size_t n, const Fr& z) {
  Fr h = Fr::zero();
  for (int k = (int)DIV_K - 1; k >= 0; --k) {
    const size_t i = lo + (size_t)k;
    Fr m = Fr::mul(h, z);                                   // < 2r
    h = i < n ? Fr::add(m, load_fp<Fr>(p + i * 32)) : m;    // canonical coefficient: < 3r
  }
  return h;
}
__device__ __forceinline__ void div_blocks_body(uint32_t* l, uint32_t blk, const char* __restrict__ p, size_t n, const FrK& zk, char* __restrict__ E) {
  const uint32_t t = threadIdx.x; const Fr z = fr_arg(zk);
  Fr x = Fr::cond_sub<2>(div_lane_fold(p, ((size_t)blk * DIV_B + t) * DIV_K, n, z));
  Fr w = z; for (int i = 0; i < 4; ++i) w = Fr::sqr(w);     // Z = z^16, < 2r
  for (uint32_t d = 1; d < DIV_B; d <<= 1) {               // x_t += Z^d * x_(t+d) on the lanes that are multiples of 2d
    lds_put(l, t, x); __syncthreads();
    if ((t & (2 * d - 1)) == 0) x = add_lt2r(x, Fr::mul(lds_get(l, t + d), w));
    __syncthreads();
    w = Fr::sqr(w);
  }
  if (t == 0) store_fp<Fr>(E + (size_t)blk * 32, x);
}
// One block.  C[b] = sum_(u > b) E[u] * ZB^(u - b - 1), ZB = z^(16 * 256): lane q owns `per` consecutive blocks.
__device__ __forceinline__ void div_carries_body(uint32_t* l, const char* __restrict__ E, uint32_t nb, uint32_t per, const FrK& zk, char* __restrict__ C) {
  const uint32_t t = threadIdx.x; Fr zb = fr_arg(zk);
  for (int i = 0; i < 12; ++i) zb = Fr::sqr(zb);            // z^4096, < 2r
  const uint32_t lo = t * per, hi = lo + per < nb ? lo + per : nb;
  Fr g = Fr::zero();
  for (uint32_t b = hi; b-- > lo;) g = add_lt2r(Fr::mul(g, zb), load_fp<Fr>(E + (size_t)b * 32));
  Fr w = Fr::one();                                         // ZB^per by square-and-multiply
  for (int bit = 31 - __clz(per | 1u); bit >= 0; --bit) { w = Fr::sqr(w); if ((per >> bit) & 1u) w = Fr::mul(w, zb); }
  Fr x = g;
  for (uint32_t d = 1; d < DIV_B; d <<= 1) {               // suffix scan over the 256 lanes (Hillis-Steele): x_t += W^d * x_(t+d)
    lds_put(l, t, x); __syncthreads();
    if (t + d < DIV_B) x = add_lt2r(x, Fr::mul(lds_get(l, t + d), w));
    __syncthreads();
    w = Fr::sqr(w);
  }
  lds_put(l, t, x); __syncthreads();
  Fr c = t + 1 < DIV_B ? lds_get(l, t + 1) : Fr::zero();    // everything behind this lane's blocks
  for (uint32_t b = hi; b-- > lo;) {
    store_fp<Fr>(C + (size_t)b * 32, c);
    c = add_lt2r(Fr::mul(c, zb), load_fp<Fr>(E + (size_t)b * 32));
  }
}
__device__ __forceinline__ void div_finish_body(uint32_t* l, uint32_t blk, const char* __restrict__ p, size_t n, const FrK& zk, const char* __restrict__ C, char* __restrict__ q, char* __restrict__ eval) {
  const uint32_t t = threadIdx.x; const Fr z = fr_arg(zk);
  const size_t lo = ((size_t)blk * DIV_B + t) * DIV_K;
  Fr x = Fr::cond_sub<2>(div_lane_fold(p, lo, n, z));
  Fr w = z; for (int i = 0; i < 4; ++i) w = Fr::sqr(w);     // Z = z^16
  if (t == DIV_B - 1) x = add_lt2r(x, Fr::mul(load_fp<Fr>(C + (size_t)blk * 32), w));     // the block's carry enters behind its last lane
  for (uint32_t d = 1; d < DIV_B; d <<= 1) {
    lds_put(l, t, x); __syncthreads();
    if (t + d < DIV_B) x = add_lt2r(x, Fr::mul(lds_get(l, t + d), w));
    __syncthreads();
    w = Fr::sqr(w);
  }
  lds_put(l, t, x); __syncthreads();
  Fr s = t + 1 < DIV_B ? lds_get(l, t + 1) : load_fp<Fr>(C + (size_t)blk * 32);      // s_(lo + 16)
  for (int k = (int)DIV_K - 1; k >= 0; --k) {              // s_j = p_j + z s_(j+1);  w_(j-1) = s_j;  p(z) = s_0
    const size_t j = lo + (size_t)k;
    if (j >= n) continue;
    s = Fr::add(Fr::mul(s, z), load_fp<Fr>(p + j * 32));    // < 3r
    if (j) { if (q) store_fp<Fr>(q + (j - 1) * 32, Fr::reduce(s)); } else if (eval) store_fp<Fr>(eval, Fr::reduce(s));
  }
}
// Up to DIV_MANY independent divisions in the same three launches (blockIdx.y picks the division): the two witness polynomials of a proof's openings are
// latency-bound chains of ~100 us each (the middle kernel is ONE block) that used to run one after the other.
static constexpr uint32_t DIV_MANY = 4;
struct DivJob { const char* p; size_t n; FrK z; char* q; char* eval; char* E; char* C; uint32_t nb, per; };
struct DivJobs { DivJob j[DIV_MANY]; };
__global__ void __launch_bounds__(256) k_div_blocks_many(DivJobs J) {
  __shared__ uint32_t l[8 * DIV_B];
  const DivJob& d = J.j[blockIdx.y];
  if (blockIdx.x >= d.nb) return;
  div_blocks_body(l, blockIdx.x, d.p, d.n, d.z, d.E);
}
__global__ void __launch_bounds__(256) k_div_carries_many(DivJobs J) {
  __shared__ uint32_t l[8 * DIV_B];
  const DivJob& d = J.j[blockIdx.x];
  div_carries_body(l, d.E, d.nb, d.per, d.z, d.C);
}
__global__ void __launch_bounds__(256) k_div_finish_many(DivJobs J) {
  __shared__ uint32_t l[8 * DIV_B];
  const DivJob& d = J.j[blockIdx.y];
  if (blockIdx.x >= d.nb) return;
  div_finish_body(l, blockIdx.x, d.p, d.n, d.z, d.C, d.q, d.eval);
}

// The shape of one division: its blocks, the blocks a lane of the carry kernel owns, and where its E | C (nb elements each) lie in the scratch.
static int32_t div_shape(DivJob& d, size_t n, Carve& scratch, size_t* at) {
  const size_t nb = (n + DIV_TILE - 1) / DIV_TILE;
  if (nb >= (1ull << 31)) { g_last_error = "fr_divide_by_linear: polynomial too long"; return ALEO_MI355X_ERR_BAD_ARG; }
  d.n = n; d.nb = (uint32_t)nb; d.per = (uint32_t)((nb + DIV_B - 1) / DIV_B); *at = scratch.part(2 * nb * 32);
  return ALEO_MI355X_OK;
}

int32_t fr_divide_by_linear_many(Ctx* c, void* const* d_q, void* const* d_eval, const void* const* d_p, const size_t* n, const void* const* z_mont32, size_t count, hipStream_t s) {
  if (count == 0) return ALEO_MI355X_OK;
  if (count > DIV_MANY) { g_last_error = "fr_divide_by_linear_many: at most 4 divisions per call"; return ALEO_MI355X_ERR_BAD_ARG; }
  DivJobs J{}; Carve scratch; size_t at[DIV_MANY]; uint32_t nb_max = 0;
  for (size_t i = 0; i < count; ++i) {
    if (n[i] == 0) { g_last_error = "fr_divide_by_linear_many: empty polynomial"; return ALEO_MI355X_ERR_BAD_ARG; }
    if (int32_t rc = div_shape(J.j[i], n[i], scratch, &at[i])) return rc;
    nb_max = J.j[i].nb > nb_max ? J.j[i].nb : nb_max;
  }
  return with_scratch(c, c->ntt_tmp, scratch.total, s, [&]() -> int32_t {
    for (size_t i = 0; i < count; ++i) {
      DivJob& d = J.j[i]; d.p = (const char*)d_p[i]; d.z = load_k(z_mont32[i]); d.q = (char*)d_q[i]; d.eval = d_eval ? (char*)d_eval[i] : nullptr;
      d.E = c->ntt_tmp.as<char>() + at[i]; d.C = d.E + (size_t)d.nb * 32;
    }
    hipLaunchKernelGGL(k_div_blocks_many, dim3(nb_max, (uint32_t)count), dim3(256), 0, s, J);
    hipLaunchKernelGGL(k_div_carries_many, dim3((uint32_t)count), dim3(256), 0, s, J);
    return launch(k_div_finish_many, dim3(nb_max, (uint32_t)count), dim3(256), s, J);
  });
}

// One division is the road of many with one job; the empty polynomial (no block to run) has the value 0 and no quotient.
int32_t fr_divide_by_linear(Ctx* c, void* d_q, void* d_eval, const void* d_p, size_t n, const void* z_mont32, hipStream_t s) {
  if (n == 0) { if (d_eval) HIPCHK(hipMemsetAsync(d_eval, 0, 32, s)); return ALEO_MI355X_OK; }
  return fr_divide_by_linear_many(c, &d_q, &d_eval, &d_p, &n, &z_mont32, 1, s);
}

// p_q(z_q) for up to EVAL_MAX (12) polynomials in two launches: the per-block folds of the division's first kernel for all of them at once, then one
// block per polynomial combines its folds (Horner over its lanes' runs of blocks, then a sum over the lanes weighted by powers of z^4096).
static constexpr uint32_t EVAL_MAX = 12;
struct EvalArgs { const char* p[EVAL_MAX]; size_t n[EVAL_MAX]; FrK z[EVAL_MAX]; uint32_t first_block[EVAL_MAX + 1]; uint32_t k; };
__global__ void __launch_bounds__(256) k_eval_blocks(EvalArgs a, char* __restrict__ E) {
  __shared__ uint32_t l[8 * DIV_B];
  uint32_t q = 0; while (q + 1 < a.k && blockIdx.x >= a.first_block[q + 1]) ++q;
  div_blocks_body(l, blockIdx.x - a.first_block[q], a.p[q], a.n[q], a.z[q], E + (size_t)a.first_block[q] * 32);      // block b of polynomial q -> slot first_block[q] + b
}
__global__ void __launch_bounds__(256) k_eval_combine(EvalArgs a, const char* __restrict__ E, char* __restrict__ out) {
  __shared__ uint32_t l[8 * DIV_B];
  const uint32_t q = blockIdx.x, t = threadIdx.x, nb = a.first_block[q + 1] - a.first_block[q];
  const char* Eq = E + (size_t)a.first_block[q] * 32;
  Fr zb = fr_arg(a.z[q]); for (int i = 0; i < 12; ++i) zb = Fr::sqr(zb);                 // z^4096
  const uint32_t per = (nb + DIV_B - 1) / DIV_B, lo = t * per, hi = lo + per < nb ? lo + per : nb;
  Fr g = Fr::zero();
  for (uint32_t b = hi; b-- > lo && hi > lo;) g = add_lt2r(Fr::mul(g, zb), load_fp<Fr>(Eq + (size_t)b * 32));
  Fr w = zb; fr_pow_u64_ni(&w, (uint64_t)lo);                                             // weight of this lane's run
  Fr x = lo < nb ? Fr::cond_sub<1>(Fr::mul(g, w)) : Fr::zero();                            // < r
  for (uint32_t d = DIV_B / 2; d >= 1; d >>= 1) {
    lds_put(l, t, x); __syncthreads();
    if (t < d) x = Fr::cond_sub<1>(Fr::add(x, lds_get(l, t + d)));                          // < 2r -> < r
    __syncthreads();
  }
  if (t == 0) store_fp<Fr>(out + (size_t)q * 32, x);
}
int32_t fr_eval_batch(Ctx* c, void* d_out, const void* const* d_polys, const size_t* lens, const void* z_mont, size_t k, hipStream_t s) {
  if (k == 0) return ALEO_MI355X_OK;
  if (k > EVAL_MAX) { g_last_error = "fr_eval_batch: more than 12 polynomials in one call"; return ALEO_MI355X_ERR_BAD_ARG; }
  EvalArgs a{}; a.k = (uint32_t)k; uint64_t total = 0;
  for (size_t q = 0; q < k; ++q) {
    if (!d_polys[q] && lens[q]) { g_last_error = "fr_eval_batch: null polynomial"; return ALEO_MI355X_ERR_BAD_ARG; }
    a.p[q] = (const char*)d_polys[q]; a.n[q] = lens[q]; a.z[q] = load_k((const char*)z_mont + 32 * q);
    a.first_block[q] = (uint32_t)total; total += (lens[q] + DIV_TILE - 1) / DIV_TILE;     // an empty polynomial owns no block: its value is 0
    if (total >= (1ull << 31)) { g_last_error = "fr_eval_batch: polynomials too long"; return ALEO_MI355X_ERR_BAD_ARG; }
  }
  a.first_block[k] = (uint32_t)total;
  return with_scratch(c, c->ntt_tmp, (total + 1) * 32, s, [&]() -> int32_t {
    char* E = c->ntt_tmp.as<char>();
    if (total) hipLaunchKernelGGL(k_eval_blocks, dim3((uint32_t)total), dim3(256), 0, s, a, E);
    return launch(k_eval_combine, dim3((uint32_t)k), dim3(256), s, a, (const char*)E, (char*)d_out);
  });
}

}  // namespace aleo_mi355x
