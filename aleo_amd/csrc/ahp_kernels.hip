// ahp_kernels.hip — small fused kernels of the prover's rounds (round 5: every launch of a real-circuit-sized proof is ~4.5 us of GPU time even when it moves a few KB):
// the two sumcheck numerators, the layout steps of the first two rounds and the split of the first sumcheck's quotient, one launch each.
#include "frops.h"
#include "fr_kernels.h"

namespace aleo_mi355x {

// The two sumcheck numerators, each one pass over evaluations that already sit in HBM (values of the operands on the larger domain):
//   first  (domain 4|H|): dst = r * (a + eta_b b + eta_c a b) − t * z          [UPSTREAM-RECALL: round_functions/second.rs, the summed polynomial]
//   matrix (domain 2|K|): dst = sum_M delta_M (vv val_M − (alpha beta − beta row_M − alpha col_M + row_col_M) f_M)   [fourth.rs]
__global__ void __launch_bounds__(256) k_ahp_first_sumcheck(char* dst, size_t n, const char* r, const char* a, const char* b, const char* t,
                                                            const char* z, FrK keb, FrK kec) {
  const Fr eb = fr_arg(keb), ec = fr_arg(kec);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const Fr va = load_fp<Fr>(a + i * 32), vb = load_fp<Fr>(b + i * 32);
    Fr u = add_lt2r(va, Fr::mul(eb, vb));                                                   // < 3r -> < 2r
    u = add_lt2r(u, Fr::mul(ec, Fr::mul(va, vb)));                                          // < 4r -> < 2r
    u = Fr::mul(load_fp<Fr>(r + i * 32), u);                                                // < 2r
    const Fr w = Fr::mul(load_fp<Fr>(t + i * 32), load_fp<Fr>(z + i * 32));                 // < 2r
    store_fp<Fr>(dst + i * 32, Fr::reduce(Fr::sub<2>(u, w)));                               // u + 2r − w < 4r
  }
}
int32_t ahp_first_sumcheck(Ctx* c, void* d_dst, size_t n, const void* d_r, const void* d_a, const void* d_b, const void* d_t, const void* d_z,
                           const void* eta_b, const void* eta_c, hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  return launch(k_ahp_first_sumcheck, grid_for(n, 16384), dim3(256), s, (char*)d_dst, n, (const char*)d_r, (const char*)d_a, (const char*)d_b, (const char*)d_t,
                (const char*)d_z, load_k(eta_b), load_k(eta_c));
}
struct MatArgs { const char* idx[3]; const char* f[3]; FrK delta[3]; FrK ab, nalpha, nbeta, vv; size_t stride; };      // idx[m] == nullptr: matrix m is absent
__global__ void __launch_bounds__(256) k_ahp_matrix_sumcheck(char* __restrict__ dst, size_t n, MatArgs a) {
  const Fr ab = fr_arg(a.ab), na = fr_arg(a.nalpha), nb = fr_arg(a.nbeta), vv = fr_arg(a.vv);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    Fr acc = Fr::zero();
    for (int m = 0; m < 3; ++m) {
      if (!a.idx[m]) continue;                                                                // (uniform across the grid)
      const char* e = a.idx[m] + i * 32;                                                    // row, col, val, row_col: `stride` bytes apart
      Fr bq = add_lt2r(ab, Fr::mul(nb, load_fp<Fr>(e)));                                     // alpha beta − beta row            < 2r
      bq = add_lt2r(bq, Fr::mul(na, load_fp<Fr>(e + a.stride)));                             // − alpha col                      < 2r
      bq = add_lt2r(bq, load_fp<Fr>(e + 3 * a.stride));                                      // + row_col                        < 2r
      const Fr bf = Fr::mul(bq, load_fp<Fr>(a.f[m] + i * 32));                               // < 2r
      const Fr pm = Fr::cond_sub<2>(Fr::sub<2>(Fr::mul(vv, load_fp<Fr>(e + 2 * a.stride)), bf));      // vv val − b f: < 4r -> < 2r
      acc = add_lt2r(acc, Fr::mul(fr_arg(a.delta[m]), pm));                                  // < 2r
    }
    store_fp<Fr>(dst + i * 32, Fr::cond_sub<1>(acc));
  }
}
// consts: 7 Montgomery values on the host — delta_a, delta_b, delta_c, alpha beta, −alpha, −beta, v_H(alpha) v_H(beta)
int32_t ahp_matrix_sumcheck(Ctx* c, void* d_dst, size_t n, const void* const* d_index, size_t index_stride_elems, const void* const* d_f, const void* consts,
                            hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  MatArgs a{}; const char* k = (const char*)consts;
  for (int m = 0; m < 3; ++m) { a.idx[m] = (const char*)d_index[m]; a.f[m] = (const char*)d_f[m]; a.delta[m] = load_k(k + 32 * m); }
  a.ab = load_k(k + 96); a.nalpha = load_k(k + 128); a.nbeta = load_k(k + 160); a.vv = load_k(k + 192);
  a.stride = index_stride_elems * 32;
  return launch(k_ahp_matrix_sumcheck, grid_for(n, 16384), dim3(256), s, (char*)d_dst, n, a);
}

// Two layout steps of the prover's first two rounds, one launch each for all instances (they were 3 launches per polynomial and 5 per instance):
//   blind rows:  dst[q] (n + 1 coefficients) = src[q] (n coefficients) + rho_q (X^n − 1)        — w, z_a, z_b after the inverse transform
//   sumcheck operands of instance i on the 4n domain, zero padded:  z_i = w_i (X^|X| − 1) + x̂_i,  z_a,i,  z_b,i   (rows 3i, 3i+1, 3i+2 of dst)
static constexpr uint32_t BLIND_MAX = 24;
struct BlindArgs { FrK rho[BLIND_MAX]; };
__global__ void __launch_bounds__(256) k_blind_rows(char* __restrict__ dst, const char* __restrict__ src, size_t n, uint32_t rows, BlindArgs a) {
  const size_t L = n + 1;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < L * rows; t += (size_t)gridDim.x * 256) {
    const uint32_t q = (uint32_t)(t / L); const size_t i = t % L;
    Fr v = i < n ? load_fp<Fr>(src + ((size_t)q * n + i) * 32) : fr_arg(a.rho[q]);
    if (i == 0) v = Fr::cond_sub<1>(Fr::sub<1>(v, fr_arg(a.rho[q])));                         // v + r − rho < 2r -> < r
    store_fp<Fr>(dst + t * 32, v);
  }
}
int32_t fr_blind_rows(Ctx* c, void* d_dst, const void* d_src, size_t n, size_t rows, const void* rho_mont, hipStream_t s) {
  (void)c;
  if (!rows || !n) return ALEO_MI355X_OK;
  if (rows > BLIND_MAX) { g_last_error = "fr_blind_rows: more than 24 rows"; return ALEO_MI355X_ERR_BAD_ARG; }
  BlindArgs a{}; std::memcpy(a.rho, rho_mont, rows * 32);
  return launch(k_blind_rows, grid_for((n + 1) * rows, 16384), dim3(256), s, (char*)d_dst, (const char*)d_src, n, (uint32_t)rows, a);
}
// wit: 3 rows of n + 1 coefficients per instance (w, z_a, z_b); xp: |X| coefficients of x̂ per instance; dst: 3 rows of n4 per instance
__global__ void __launch_bounds__(256) k_sumcheck_operands(char* __restrict__ dst, const char* __restrict__ wit, const char* __restrict__ xp, size_t n, size_t n_x,
                                                           size_t n4, uint32_t instances) {
  const size_t L = n + 1;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n4 * 3 * instances; t += (size_t)gridDim.x * 256) {
    const size_t row = t / n4, j = t % n4, i = row / 3, kind = row % 3;
    const char* w = wit + (3 * i) * L * 32;
    Fr v = Fr::zero();
    if (kind == 0) {
      if (j >= n_x && j < L + n_x) v = load_fp<Fr>(w + (j - n_x) * 32);                       // + w X^|X|
      if (j < L) v = Fr::sub<1>(v, load_fp<Fr>(w + j * 32));                                  // − w             (< 2r)
      if (j < n_x) v = Fr::add(v, load_fp<Fr>(xp + (i * n_x + j) * 32));                      // + x̂             (< 3r)
      v = Fr::cond_sub<1>(Fr::cond_sub<2>(v));
    } else if (j < L) v = load_fp<Fr>(w + (kind * L + j) * 32);
    store_fp<Fr>(dst + t * 32, v);
  }
}
int32_t ahp_sumcheck_operands(Ctx* c, void* d_dst, const void* d_wit, const void* d_xp, size_t n, size_t n_x, size_t instances, hipStream_t s) {
  (void)c;
  if (!instances || !n) return ALEO_MI355X_OK;
  const size_t n4 = 4 * n;
  return launch(k_sumcheck_operands, grid_for(n4 * 3 * instances, 32768), dim3(256), s, (char*)d_dst, (const char*)d_wit, (const char*)d_xp, n, n_x, n4, (uint32_t)instances);
}

// The quotient and remainder of q (3n coefficients, blocks p0 | p1 | p2; + mask when given) by X^n - 1:  hq = [p1 + p2 | p2],  rq = p0 + p1 + p2;
// rq[0] — the sum of the first sumcheck's summand over H — also goes to `host_sum` (a device pointer of pinned host memory) when given.
__global__ void __launch_bounds__(256) k_split_quotient(const char* __restrict__ q, const char* __restrict__ mask, size_t n, char* __restrict__ hq, char* __restrict__ rq, char* __restrict__ host_sum) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    Fr p0 = load_fp<Fr>(q + i * 32), p1 = load_fp<Fr>(q + (n + i) * 32), p2 = load_fp<Fr>(q + (2 * n + i) * 32);
    if (mask) {
      p0 = Fr::cond_sub<1>(Fr::add(p0, load_fp<Fr>(mask + i * 32))); p1 = Fr::cond_sub<1>(Fr::add(p1, load_fp<Fr>(mask + (n + i) * 32)));
      p2 = Fr::cond_sub<1>(Fr::add(p2, load_fp<Fr>(mask + (2 * n + i) * 32)));
    }
    const Fr h0 = Fr::cond_sub<1>(Fr::add(p1, p2)), r0 = Fr::cond_sub<1>(Fr::add(p0, h0));
    store_fp<Fr>(hq + (n + i) * 32, p2); store_fp<Fr>(hq + i * 32, h0); store_fp<Fr>(rq + i * 32, r0);
    if (i == 0 && host_sum) store_fp<Fr>(host_sum, r0);
  }
}
int32_t fr_split_quotient(Ctx* c, void* d_hq, void* d_rq, const void* d_q, const void* d_mask, size_t n, void* host_sum_devptr, hipStream_t s) {
  (void)c;
  if (n == 0) return ALEO_MI355X_OK;
  return launch(k_split_quotient, grid_for(n, 8192), dim3(256), s, (const char*)d_q, (const char*)d_mask, n, (char*)d_hq, (char*)d_rq, (char*)host_sum_devptr);
}

}  // namespace aleo_mi355x
