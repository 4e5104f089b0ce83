// varuna_rounds.hip — one circuit's share of each round of a proof (Prover::*, upstream AHPForR1CS::prover_{first,second,third,fourth}_round): the
// kernels that turn its assignments, then each round's challenges, into the polynomials the proof commits to.  Queued on the proof's stream; no transcript.
#include "varuna_host.h"

namespace aleo_mi355x {

int32_t Prover::setup() {
  n_h = ix.n_h; n_x = ix.n_x; L = n_h + 1; n4 = 4 * n_h;
  nk[0] = ix.n_k_a; nk[1] = ix.n_k_b; nk[2] = ix.n_k_c; ko[0] = 0; ko[1] = nk[0]; ko[2] = nk[0] + nk[1]; k_sum = nk[0] + nk[1] + nk[2];
  n_k = nk[0] > nk[1] ? (nk[0] > nk[2] ? nk[0] : nk[2]) : (nk[1] > nk[2] ? nk[1] : nk[2]);      // the largest non-zero domain of this circuit
  const uint64_t D = ix.max_degree; const PinnedBases& pb = sh.pb;
  bool k_ok = true; for (int m = 0; m < 3; ++m) k_ok = k_ok && nk[m] >= 2 && !(nk[m] & (nk[m] - 1));
  if (k < 1 || k > MAX_INSTANCES || n_h < 2 || !k_ok || n_x < 1 || n_h < 2 * n_x || (n_h & (n_h - 1)) || (n_x & (n_x - 1)) ||
      ix.n_public > n_x || ix.n_vars > n_h || ix.gamma_offset + HC > pb.n || (ix.lagrange_offset && ix.lagrange_offset + n_h + 1 > pb.n) || D + 1 > pb.n || 3 * n_h > D + 1 || n_k > D + 1) {
    g_last_error = "varuna_prove: inconsistent index / key sizes"; return ALEO_MI355X_ERR_BAD_ARG;
  }
  if (!ix.a_row_ptr || !ix.a_col || !ix.a_val || !ix.b_row_ptr || !ix.b_col || !ix.b_val || !ix.t_row_ptr || !ix.t_col || !ix.t_val || !ix.vx_inv || !ix.k_evals || !ix.k_idx ||
      !ix.k_polys || !ix.k2_evals || !ix.positions || !ix.vk_bytes || ix.vk_len != 12 * 48 + 40) {
    g_last_error = "varuna_prove: the index struct has a null array (or vk_len != 616)"; return ALEO_MI355X_ERR_BAD_ARG;
  }
  lg_h = lg2(n_h); for (int m = 0; m < 3; ++m) lg_km[m] = lg2(nk[m]);
  return ALEO_MI355X_OK;
}

int32_t Prover::first_round(const void* const* assignments, std::vector<MsmSeg>& sg) {
  Ctx* c = sh.c; hipStream_t s = sh.s; Arena& ar = sh.ar; char* pin = sh.pin + pin_off * 32; char* stage = sh.stage;
  char *zH, *ev, *xh; RC(ar.take(zH, k * n_h + 8)); RC(ar.take(ev, 3 * k * n_h)); RC(ar.take(xh, k * n_h));
  RC(ar.take(xp, k * n_x)); RC(ar.take(wit, 3 * k * L));      // (zH + 8: the canonical-input flag sits behind z on H, cleared by the same fill)
  x_poly.assign(k, {});
  const size_t xb0 = sh.x_mont.size(); sh.x_mont.resize(xb0 + k * n_x, HFr::zero());          // the padded public inputs: what the transcript absorbs per instance
  const HFr one = sh.one, gx_inv = HFr::inv(domain_gen(n_x)), nx_inv = inv_pow2(lg2(n_x));
  const uint32_t* pos = (const uint32_t*)ix.positions;
  const bool host_layout = ix.positions_device == nullptr;      // without the positions in HBM the host lays the assignment out on H (pinned staging)
  if (host_layout) std::memset(pin, 0, k * n_h * 32);
  else for (size_t v = 0; v < ix.n_vars; ++v) if (pos[v] >= n_h) { g_last_error = "varuna_prove: variable position outside H"; return ALEO_MI355X_ERR_BAD_ARG; }
  for (size_t i = 0; i < k; ++i) {
    const uint8_t* z = (const uint8_t*)assignments[i];
    if (host_layout)
      for (size_t v = 0; v < ix.n_vars; ++v) {
        if (pos[v] >= n_h) { g_last_error = "varuna_prove: variable position outside H"; return ALEO_MI355X_ERR_BAD_ARG; }
        if (HFr::geq_p((const uint64_t*)(z + v * 32))) { g_last_error = "varuna_prove: assignment not canonical"; return ALEO_MI355X_ERR_BAD_ARG; }
        std::memcpy(pin + (i * n_h + pos[v]) * 32, z + v * 32, 32);
      }
    std::vector<HFr> xe(n_x, HFr::zero());
    for (size_t t = 0; t < ix.n_public; ++t) { HFr v; std::memcpy(v.l, z + t * 32, 32); if (HFr::geq_p(v.l)) { g_last_error = "varuna_prove: assignment not canonical"; return ALEO_MI355X_ERR_BAD_ARG; } xe[t] = HFr::to_mont(v); sh.x_mont[xb0 + i * n_x + t] = xe[t]; }
    x_poly[i] = xe;                                        // inverse DFT over X on the host: |X| is the (padded) number of public inputs
    host_ntt(x_poly[i], gx_inv);
    for (auto& v : x_poly[i]) v = HFr::mul(v, nx_inv);
  }
  for (size_t i = 0; i < k; ++i) std::memcpy(stage + (x_off + i * n_x) * 32, x_poly[i].data(), n_x * 32);
  if (host_layout) {
    HIPCHK(hipMemcpyAsync(zH, pin, k * n_h * 32, hipMemcpyHostToDevice, s));
    RC(fr_lin(c, zH, k * n_h, nullptr, sh.r2.l, zH, nullptr, nullptr, s));                // canonical -> Montgomery
  } else {                                                                                  // upload in variable order; scatter + Montgomery form on the device
    char* zraw; RC(ar.take(zraw, k * ix.n_vars));
    if (!sh.flag) sh.flag = zH + k * n_h * 32;                                               // raised by the scatter when an entry is not below r
    HIPCHK(hipMemsetAsync(zH, 0, (k * n_h + 8) * 32, s));
    for (size_t i = 0; i < k; ++i) {
      HIPCHK(hipMemcpyAsync(zraw + i * ix.n_vars * 32, assignments[i], ix.n_vars * 32, hipMemcpyHostToDevice, s));
      RC(fr_scatter_to_mont(c, zH + i * n_h * 32, zraw + i * ix.n_vars * 32, ix.positions_device, ix.n_vars, sh.flag, s));
    }
  }
  HIPCHK(hipMemcpyAsync(xp, stage + x_off * 32, k * n_x * 32, hipMemcpyHostToDevice, s));
  RC(p_ntt_from(c, sh.pb, xh, xp, n_x, n_x, lg_h, k, s));      // x̂ of every instance on H: |X| coefficients each, zero-padded by the transform's first pass
  for (size_t i = 0; i < k; ++i) {
    char* e0 = ev + 3 * i * n_h * 32; char* z_i = zH + i * n_h * 32; char* xh_i = xh + i * n_h * 32;
    RC(fr_spmv(c, e0 + n_h * 32, ix.a_row_ptr, ix.a_col, ix.a_val, z_i, n_h, s, ix.max_row[0]));
    RC(fr_spmv(c, e0 + 2 * n_h * 32, ix.b_row_ptr, ix.b_col, ix.b_val, z_i, n_h, s, ix.max_row[1]));
    RC(fr_sub_mul(c, e0, z_i, xh_i, ix.vx_inv, n_h, s));                                    // (z − x̂) / v_X off X, 0 on X
  }
  if (lagrange()) {                                        // KZG10::commit_lagrange for w, z_a, z_b: commit the evaluations (kept here) against L_i(tau) G
    RC(ar.take(evals_h, 3 * k * n_h)); RC(ar.take(rho_dev, 3 * k));
    HIPCHK(hipMemcpyAsync(evals_h, ev, 3 * k * n_h * 32, hipMemcpyDeviceToDevice, s));
  }
  RC(p_ntt(c, sh.pb, ev, lg_h, 3 * k, 1, 0, s));
  {
    HFr rho[3 * MAX_INSTANCES];                                                             // rho_w, rho_a, rho_b of instance q / 3
    for (size_t q = 0; q < 3 * k; ++q) {
      rho[q] = random_fr(sh.seed, 3 * q0 + q);
      for (size_t t = 0; t < HC; ++t) sh.blind[(3 * q0 + q) * HC + t] = random_fr(sh.seed, sh.lay_blind + HC * (3 * q0 + q) + t);
    }
    for (size_t at = 0; at < 3 * k; at += 24) RC(fr_blind_rows(c, wit + at * L * 32, ev + at * n_h * 32, n_h, 3 * k - at < 24 ? 3 * k - at : 24, rho + at, s));      // + rho (X^|H| − 1), 24 polynomials per launch
    if (lagrange()) { char* st = stage + (sh.st_rho() + 3 * q0) * 32; std::memcpy(st, rho, 3 * k * 32); HIPCHK(hipMemcpyAsync(rho_dev, st, 3 * k * 32, hipMemcpyHostToDevice, s)); }
  }
  for (size_t q = 0; q < 3 * k; ++q) {
    const size_t out = 3 * q0 + q;
    if (lagrange()) {                                                                       // sum_i evals_i L_i(tau) G + rho v_H(tau) G
      sg.push_back(seg(evals_h + q * n_h * 32, n_h, ix.lagrange_offset, out));
      sg.push_back(seg(rho_dev + q * 32, 1, ix.lagrange_offset + n_h, out));
    } else sg.push_back(seg(wit + q * L * 32, L, 0, out));
    sg.push_back(seg(sh.bl + out * HC * 32, HC, ix.gamma_offset, out));
  }
  return ALEO_MI355X_OK;
}

int32_t Prover::second_round_early() {
  Ctx* c = sh.c; hipStream_t s = sh.s;
  RC(sh.ar.take(E, (2 + 3 * k) * n4));      // rows 0, 1: r, t (second_round); then ẑ_i, z_a,i, z_b,i per instance
  RC(ahp_sumcheck_operands(c, E + 2 * n4 * 32, wit, xp, n_h, n_x, k, s));                    // ẑ_i = w_i (X^|X| − 1) + x̂_i, z_a,i, z_b,i — every row written in full
  return p_ntt(c, sh.pb, E + 2 * n4 * 32, lg_h + 2, 3 * k, 0, 0, s);
}

int32_t Prover::second_round() {
  Ctx* c = sh.c; hipStream_t s = sh.s; Arena& ar = sh.ar; const HFr &alpha = sh.alpha, &eta_b = sh.eta_b, &eta_c = sh.eta_c;
  vh_alpha = vanish(n_h, alpha);
  if (vh_alpha.is_zero()) { g_last_error = "varuna_prove: alpha landed in H"; return ALEO_MI355X_ERR_HIP; }
  char *rt, *Q; RC(ar.take(ext, 3 * n_h)); RC(ar.take(rt, 2 * n_h)); RC(ar.take(Q, n4));
  if (lead()) { hq = sh.h1; rq = sh.g1; } else { RC(ar.take(hq, 2 * n_h)); RC(ar.take(rq, n_h)); }
  {
    const HFr first = HFr::pow_u64(alpha, n_h - 1), ratio = HFr::inv(alpha);
    RC(fr_powers(c, rt, n_h, first.l, ratio.l, s));                                          // r(alpha, X) = sum_k alpha^(|H|-1-k) X^k
  }
  RC(p_ntt_from(c, sh.pb, ext, rt, n_h, n_h, lg_h, 1, s));    // v_H(alpha) / (alpha − h) on H: no inversion on the device
  { const HFr eta[2] = {eta_b, eta_c}; RC(fr_scale_rows(c, ext + n_h * 32, ext, n_h, 2, eta, s)); }      // the eta_b- and eta_c-scaled copies B^T and C^T multiply
  RC(fr_spmv(c, rt + n_h * 32, ix.t_row_ptr, ix.t_col, ix.t_val, ext, n_h, s, ix.max_row[2]));
  RC(p_ntt(c, sh.pb, rt + n_h * 32, lg_h, 1, 1, 0, s));                                       // t(X)
  RC(p_ntt_from(c, sh.pb, E, rt, n_h, n_h, lg_h + 2, 2, s));  // r, t on 4|H|: |H| coefficients each, zero-padded by the first pass (the operands of the instances are there already: second_round_early)
  for (size_t i = 0; i < k; ++i) {
    char* e_z = E + (2 + 3 * i) * n4 * 32;
    RC(ahp_first_sumcheck(c, e_z + n4 * 32, n4, E, e_z + n4 * 32, e_z + 2 * n4 * 32, E + n4 * 32, e_z, eta_b.l, eta_c.l, s));
  }
  char* q1 = E + 3 * n4 * 32;
  if (k > 1 || q0 != 0) {                                                 // sum_i c_i numerator_i (the proof's first instance has c = 1)
    Terms sum;
    for (size_t i = 0; i < k; ++i) sum.add(E + (3 + 3 * i) * n4 * 32, n4, sh.comb[q0 + i]);
    RC(sum.run(c, Q, n4, HFr::zero(), s)); q1 = Q;      // 29..32 instances of one circuit: more terms than one fr_lincomb launch takes
  }
  RC(p_ntt(c, sh.pb, q1, lg_h + 2, 1, 1, 0, s));
  // q (+ the mask, which rides with the largest domain) = h (X^|H| − 1) + X g, degree < 3|H|: quotient blocks p1 + p2 | p2, remainder p0 + p1 + p2; the remainder's
  // constant term — this circuit's sum over H — goes straight into pinned host memory (read with the commitments).  One launch (rounds 1-4: a copy, three vector ops, a read-back)
  RC(fr_split_quotient(c, hq, rq, q1, lead() ? sh.mask : nullptr, n_h, sh.pin_small_dev + PIN_SUMS + 32 * j, s));
  return ALEO_MI355X_OK;
}

int32_t Prover::third_round() {
  Ctx* c = sh.c; hipStream_t s = sh.s; Arena& ar = sh.ar; const HFr& beta = sh.beta;
  vh_beta = vanish(n_h, beta);
  if (vh_beta.is_zero()) { g_last_error = "varuna_prove: beta landed in H"; return ALEO_MI355X_ERR_HIP; }
  vv = HFr::mul(vh_alpha, vh_beta);
  char* rb; RC(ar.take(f, k_sum)); RC(ar.take(rb, n_h));                                                           // f_M at element ko[M], |K_M| values
  {
    const HFr first = HFr::pow_u64(beta, n_h - 1), ratio = HFr::inv(beta);
    RC(fr_powers(c, rb, n_h, first.l, ratio.l, s));
  }
  RC(p_ntt(c, sh.pb, rb, lg_h, 1, 0, 0, s));
  {                                                                                          // f_M = val u_H(alpha, row) u_H(beta, col) on K_M: two gathers; the three matrices in one launch
    void* dst[3]; size_t cnt[3]; const void* sc[3]; const void* i1[3]; const void* i2[3];
    for (size_t m = 0; m < 3; ++m) {
      const uint32_t* ri = (const uint32_t*)ix.k_idx + 2 * ko[m];
      dst[m] = f + ko[m] * 32; cnt[m] = nk[m]; sc[m] = (const char*)ix.k_evals + (4 * ko[m] + 2 * nk[m]) * 32; i1[m] = ri; i2[m] = ri + nk[m];
    }
    RC(fr_gather_mul3(c, dst, cnt, sc, ext, i1, rb, i2, 3, s));
  }
  // maximal runs of consecutive matrices with equal domains share batched transforms (and, in round 4, one numerator pass)
  nrun = 0;
  for (size_t m = 0; m < 3;) { size_t cnt = 1; while (m + cnt < 3 && nk[m + cnt] == nk[m]) ++cnt; run0[nrun] = m; runc[nrun++] = cnt; m += cnt; }
  for (size_t r = 0; r < nrun; ++r) RC(p_ntt(c, sh.pb, f + ko[run0[r]] * 32, lg_km[run0[r]], runc[r], 1, 0, s));
  { const void* src[3] = {f + ko[0] * 32, f + ko[1] * 32, f + ko[2] * 32}; RC(fr_pick(c, sh.pin_small_dev + 32 * (3 * j), src, 3, s)); }      // f_M(0): one launch into pinned host memory
  return ALEO_MI355X_OK;
}

int32_t Prover::fourth_round_early() {
  Ctx* c = sh.c; hipStream_t s = sh.s;
  RC(sh.ar.take(F, 2 * k_sum));                                                                   // f_M zero-padded to 2|K_M|, then its values there
  for (size_t r = 0; r < nrun; ++r)                          // the polynomials of a run are contiguous in f (|K| apart): zero-padded to 2|K| by the transform's first pass
    RC(p_ntt_from(c, sh.pb, F + 2 * ko[run0[r]] * 32, f + ko[run0[r]] * 32, nk[run0[r]], nk[run0[r]], lg_km[run0[r]] + 1, runc[r], s));
  return ALEO_MI355X_OK;
}

int32_t Prover::fourth_round(Terms& h2) {
  Ctx* c = sh.c; hipStream_t s = sh.s; Arena& ar = sh.ar; const HFr &alpha = sh.alpha, &beta = sh.beta;
  char* B; RC(ar.take(B, 2 * k_sum));      // per matrix on its own domain of size 2|K_M| (F: fourth_round_early)
  for (size_t r = 0; r < nrun; ++r) {
    const size_t m0 = run0[r], cnt = runc[r], n2 = 2 * nk[m0]; char* Br = B + 2 * ko[m0] * 32;
    HFr consts[7] = {HFr::zero(), HFr::zero(), HFr::zero(), HFr::mul(alpha, beta), HFr::neg(alpha), HFr::neg(beta), vv};
    const void* idx[3] = {nullptr, nullptr, nullptr}; const void* ff[3] = {nullptr, nullptr, nullptr};
    for (size_t t = 0; t < cnt; ++t) {
      const size_t m = m0 + t;
      idx[t] = (const char*)ix.k2_evals + 8 * ko[m] * 32; ff[t] = F + 2 * ko[m] * 32; consts[t] = delta[m];
    }
    RC(ahp_matrix_sumcheck(c, Br, n2, idx, n2, ff, consts, s));                                // sum over the run of delta_M (vv val_M − b_M f_M) = h (X^|K| − 1)
    RC(p_ntt(c, sh.pb, Br, lg_km[m0] + 1, 1, 1, 0, s));
    h2.add(Br + nk[m0] * 32, nk[m0], sh.one);                                                // its upper half
  }
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
