// varuna_proof.hip — one proof above its circuits (Batch::*): sizes and workspace slices, the Fiat-Shamir transcript and the challenges it yields, the
// shared polynomials of each round and the commitments it asks for, the evaluations, the two openings, and the proof's bytes (`write`).
#include "varuna_host.h"

namespace aleo_mi355x {

int32_t Batch::setup() {
  Ctx* c = sh.c; const aleo_mi355x_varuna_index* const* ixs = rq.ixs.data(); const size_t m = rq.ixs.size(); const size_t* ks = rq.ks;
  if (m < 1 || m > MAX_INSTANCES) { g_last_error = "varuna_prove: 1..32 circuits per proof"; return ALEO_MI355X_ERR_BAD_ARG; }
  sh.m = m; sh.K = 0;
  for (size_t j = 0; j < m; ++j) {
    if (!ixs[j] || !ixs[j]->positions || !ixs[j]->vk_bytes) { g_last_error = "varuna_prove: null index"; return ALEO_MI355X_ERR_BAD_ARG; }
    if (ks[j] < 1 || ks[j] > MAX_INSTANCES) { g_last_error = "varuna_prove: 1..32 instances per circuit"; return ALEO_MI355X_ERR_BAD_ARG; }
    P.emplace_back(new Prover(sh, *ixs[j], j, ks[j], sh.K)); sh.K += ks[j];
    RC(P[j]->setup());
    if (ixs[j]->committer_key != ixs[0]->committer_key || ixs[j]->max_degree != ixs[0]->max_degree || ixs[j]->gamma_offset != ixs[0]->gamma_offset) {
      g_last_error = "varuna_prove: the circuits of one proof must share one committer key"; return ALEO_MI355X_ERR_BAD_ARG;
    }
  }
  if (sh.K > MAX_INSTANCES) { g_last_error = "varuna_prove: at most 32 instances per proof"; return ALEO_MI355X_ERR_BAD_ARG; }
  sh.D = ixs[0]->max_degree; sh.gamma_offset = ixs[0]->gamma_offset;
  sh.N = 0; sh.n_kmax = 0; sh.x_total = 0; size_t pin_elems = 0, elems = 0;
  for (size_t j = 0; j < m; ++j) {
    Prover& p = *P[j];
    if (p.n_h > sh.N) { sh.N = p.n_h; sh.lead = j; }                                        // the first circuit with the largest constraint domain carries mask, g_1, h_1
    if (p.n_k > sh.n_kmax) sh.n_kmax = p.n_k;
    p.x_off = sh.x_total; sh.x_total += p.k * p.n_x; p.pin_off = pin_elems; pin_elems += p.k * p.n_h; elems += p.workspace_elems();
  }
  sh.s = c->stream;
  sh.t_mark[0] = now_ms();
  // ---- workspace sizes (attach() places the proof in its slices) ---------------------------------------------------------------------
  elems += m > 1 ? 16 * sh.N + 4 * sh.n_kmax + 4096 : 0;                                  // the shared polynomials beside the per-circuit accounting (which already covers one circuit's)
  need_ws_bytes = (elems * 32 + (64 << 10) + 255) & ~(size_t)255;                   // (both sizes in steps of 256 bytes: the proofs of a call lie side by side)
  this->pin_elems = pin_elems;
  stage_elems = sh.x_total + (3 * sh.K + 1) * HC + HC + 3 * sh.K;                          // x̂ coefficients, hiding polynomials, the opening's hiding quotient, rho: staged through pinned memory
  need_pin_bytes = ((pin_elems + stage_elems) * 32 + PIN_SMALL_BYTES + 255) & ~(size_t)255;
  sh.one = HFr::one(); sh.neg1 = HFr::neg(sh.one); std::memcpy(sh.r2.l, host::HParams<4>::R2, 32);
  // randomness layout (oracle/varuna_ref.py randomness_layout over the largest |H| and all instances)
  sh.lay_mask = 3 * sh.K; sh.lay_blind = 3 * sh.K + 3 * sh.N; sh.lay_blind_mask = sh.lay_blind + 3 * HC * sh.K;
  return ALEO_MI355X_OK;
}

int32_t Batch::attach(char* ws, size_t ws_bytes, char* pin) {
  sh.ar = Arena{ws, 0, ws_bytes};
  sh.pin = pin; sh.stage = sh.pin + pin_elems * 32; sh.pin_small = sh.stage + stage_elems * 32;      // PIN_SMALL_BYTES for small read-backs
  void* dp = nullptr; HIPCHK(hipHostGetDevicePointer(&dp, sh.pin_small, 0)); sh.pin_small_dev = (char*)dp;
  return ALEO_MI355X_OK;
}
// Varuna::init_sponge [UPSTREAM-RECALL]: the protocol name; per circuit its batch size (u64 LE as bytes) and the padded public inputs of each of its
// instances (one non-native absorb per instance); then every circuit's twelve index commitments.
int32_t Batch::init_sponge() {
  static const uint8_t NAME[] = "VARUNA-2023";
  sh.fs.absorb_bytes(NAME, sizeof NAME - 1);
  for (auto& p : P) {
    const uint64_t k64 = p->k; uint8_t kb[8]; for (int i = 0; i < 8; ++i) kb[i] = (uint8_t)(k64 >> (8 * i));
    sh.fs.absorb_bytes(kb, 8);
    for (size_t i = 0; i < p->k; ++i) sh.fs.absorb_fr(&sh.x_mont[p->x_off + i * p->n_x], p->n_x);
  }
  for (auto& p : P) {
    if (p->ix.vk_affine) { sh.fs.absorb_g1((const uint8_t*)p->ix.vk_affine, 104, 12); continue; }
    uint8_t aff[12 * 104];                                  // an index struct without the affine form: decompress (twelve square roots, ~ 0.5 ms)
    RC(aleo_mi355x_g1_decompress(aff, p->ix.vk_bytes, 12, 0));
    sh.fs.absorb_g1(aff, 104, 12);
  }
  return ALEO_MI355X_OK;
}

int32_t Batch::first_prepare() {
  Ctx* c = sh.c; hipStream_t s = sh.s; const size_t K = sh.K, N = sh.N;
  RC(sh.ar.take(sh.bl, (3 * K + 1) * HC)); RC(sh.ar.take(sh.mask, 3 * N));
  sh.blind.assign((3 * K + 1) * HC, HFr::zero()); sh.x_mont.clear();
  std::vector<MsmSeg>& sg = job[0].segs; std::vector<MsmSeg>& sm = job[1].segs; sg.clear(); sm.clear();
  // the mask polynomial needs nothing from the assignments: queued FIRST, it runs while the host stages and uploads them (a pageable 1-MB copy keeps the calling thread ~50 us)
  RC(fr_random(c, sh.mask, 3 * N, (const uint8_t*)sh.seed.w, sh.lay_mask, 1, s));
  RC(fr_lin(c, sh.mask, 1, nullptr, sh.neg1.l, sh.mask + N * 32, sh.neg1.l, sh.mask + 2 * N * 32, s));   // sum over H* = |H*| (m_0 + m_|H*| + m_2|H*|) = 0
  for (auto& p : P) RC(p->first_round(rq.assignments + p->q0, sg));
  if (sh.flag) HIPCHK(hipMemcpyAsync(sh.pin_small + PIN_FLAG, sh.flag, 4, hipMemcpyDeviceToHost, s));      // read after the round's commitments
  for (size_t t = 0; t < HC; ++t) sh.blind[3 * K * HC + t] = random_fr(sh.seed, sh.lay_blind_mask + t);
  std::memcpy(sh.stage + sh.st_blind() * 32, sh.blind.data(), sh.blind.size() * 32);
  HIPCHK(hipMemcpyAsync(sh.bl, sh.stage + sh.st_blind() * 32, sh.blind.size() * 32, hipMemcpyHostToDevice, s));
  sh.wit_aff.assign(104 * (3 * K + 1), 0);
  {
    // with the evaluations against the Lagrange powers AND a narrow-window table over [hiding powers | Lagrange powers | v_H G] the 3K witness
    // commitments are one sparse chain (their scalars are mostly 0 / 1), the mask (uniform coefficients against the monomial powers) another
    const PinnedBases& pb = sh.pb;
    bool split = pb.range.d != nullptr;
    for (auto& p : P) split = split && p->lagrange() && pb.range_off <= p->ix.gamma_offset && p->ix.lagrange_offset + p->n_h + 1 <= pb.range_off + pb.range.cover &&
                              p->ix.lagrange_offset >= pb.range_off && p->ix.gamma_offset + HC <= pb.range_off + pb.range.cover;
    std::vector<MsmSeg>& dst = split ? sm : sg;
    dst.push_back(seg(sh.mask, 3 * N, 0, split ? 0 : 3 * K));
    dst.push_back(seg(sh.bl + 3 * K * HC * 32, HC, sh.gamma_offset, split ? 0 : 3 * K));
    // needs no challenge: behind the (last) commitment chain — the operands of the sumcheck on the device, and on the host the part of the
    // transcript that precedes the first commitments (Varuna::init_sponge: ~ 20 permutations while the GPU accumulates)
    auto behind = [this]() -> int32_t { for (auto& p : P) RC(p->second_round_early()); return init_sponge(); };
    if (split) commit_split(3 * K, sh.wit_aff.data(), behind); else commit_one(3 * K + 1, sh.wit_aff.data(), behind);
  }
  return ALEO_MI355X_OK;
}

int32_t Batch::first_finish() {
  const size_t K = sh.K;
  if (sh.flag) { uint32_t f; std::memcpy(&f, sh.pin_small + PIN_FLAG, 4); if (f) { g_last_error = "varuna_prove: assignment not canonical (an entry is not below r)"; return ALEO_MI355X_ERR_BAD_ARG; } }
  sh.fs.absorb_g1(sh.wit_aff.data(), 104, 3 * K + 1);
  // verifier_first_round [UPSTREAM-RECALL]: per circuit k_j − 1 instance combiners and (but for the first circuit) a circuit combiner in one squeeze,
  // then alpha, eta_b, eta_c in one squeeze; an instance's combiner = circuit combiner * instance combiner
  sh.comb.assign(K, sh.one);
  for (auto& p : P) {
    HFr el[MAX_INSTANCES]; const size_t cnt = p->k - 1 + (p->j ? 1 : 0);
    sh.fs.squeeze_full(el, cnt);
    const HFr cc = p->j ? el[p->k - 1] : sh.one;
    sh.comb[p->q0] = cc;
    for (size_t i = 1; i < p->k; ++i) sh.comb[p->q0 + i] = HFr::mul(cc, el[i - 1]);
  }
  { HFr el[3]; sh.fs.squeeze_full(el, 3); sh.alpha = el[0]; sh.eta_b = el[1]; sh.eta_c = el[2]; }
  sh.t_mark[1] = now_ms();
  return ALEO_MI355X_OK;
}

int32_t Batch::second_prepare() {
  Ctx* c = sh.c; hipStream_t s = sh.s; const size_t N = sh.N;
  RC(sh.ar.take(sh.h1, 2 * N)); RC(sh.ar.take(sh.g1, N));
  RC(P[sh.lead]->second_round());                                                             // writes h_1, X g_1 (with the mask) in place
  for (auto& p : P) {
    if (p->lead()) continue;
    RC(p->second_round());
    RC(fr_vec_op(c, sh.h1, sh.h1, p->hq, 2 * p->n_h, 1, s));                                  // s_j h_j v_{H_j} = h_j v_{H*}
    RC(fr_add_tiled(c, sh.g1, N, p->rq, p->n_h, s));                                          // s_j (X g_j): the remainder block repeated |H*| / |H_j| times
  }
  job[0].segs = {seg(sh.g1 + 32, N - 1, sh.D - (N - 2), 0), seg(sh.h1, 2 * N, 0, 1)};            // g_1 with degree bound |H*| − 2: shifted powers
  commit_one(2, sh.aff2);
  return ALEO_MI355X_OK;
}

int32_t Batch::second_finish() {
  for (size_t j = 0; j < sh.m; ++j) {                                                         // the commitments returned after the stream drained: the copies have landed
    uint64_t sum[4]; std::memcpy(sum, sh.pin_small + PIN_SUMS + 32 * j, 32);
    if (sum[0] | sum[1] | sum[2] | sum[3]) { g_last_error = "varuna_prove: the assignment does not satisfy the circuit (first sumcheck: the sum over H is not zero)"; return ALEO_MI355X_ERR_UNSATISFIED; }
  }
  sh.fs.absorb_g1(sh.aff2, 104, 2);
  sh.fs.squeeze_full(&sh.beta, 1);
  sh.t_mark[2] = now_ms();
  return ALEO_MI355X_OK;
}

int32_t Batch::third_prepare() {
  const size_t m = sh.m;
  for (auto& p : P) RC(p->third_round());
  std::vector<MsmSeg>& sg = job[0].segs; sg.clear();
  for (auto& p : P) for (size_t M = 0; M < 3; ++M) sg.push_back(seg(p->f + (p->ko[M] + 1) * 32, p->nk[M] - 1, sh.D - (p->nk[M] - 2), 3 * p->j + M));
  sh.aff3.assign(312 * m, 0);
  commit_one(3 * m, sh.aff3.data(), [this]() -> int32_t { for (auto& p : P) RC(p->fourth_round_early()); return ALEO_MI355X_OK; });
  return ALEO_MI355X_OK;
}

int32_t Batch::third_finish() {
  const size_t m = sh.m;
  for (auto& p : P)                                                                           // the sums f_{j,M}(0) |K| were copied out ahead of the commitments: no stream sync of their own
    for (size_t M = 0; M < 3; ++M) { HFr v; std::memcpy(v.l, sh.pin_small + 32 * (3 * p->j + M), 32); p->sigma[M] = HFr::mul(v, HFr::from_u64(p->nk[M])); }
  sh.fs.absorb_g1(sh.aff3.data(), 104, 3 * m);                                                  // absorb_with_msg: the commitments, then the sums circuit by circuit
  for (auto& p : P) sh.fs.absorb_fr(p->sigma, 3);
  {
    std::vector<HFr> el(3 * m); el[0] = sh.one; sh.fs.squeeze_full(el.data() + 1, 3 * m - 1);   // delta_{0,a} = 1, the rest from one squeeze
    for (auto& p : P) for (size_t M = 0; M < 3; ++M) p->delta[M] = el[3 * p->j + M];
  }
  sh.t_mark[3] = now_ms();
  return ALEO_MI355X_OK;
}

int32_t Batch::fourth_prepare() {
  Ctx* c = sh.c; hipStream_t s = sh.s;
  RC(sh.ar.take(sh.h2, sh.n_kmax));
  Terms sum;
  for (auto& p : P) RC(p->fourth_round(sum));
  RC(sum.run(c, sh.h2, sh.n_kmax, HFr::zero(), s));                                           // h_2 = sum_{j,M} delta_{j,M} h_{j,M}
  job[0].segs = {seg(sh.h2, sh.n_kmax, 0, 0)};
  commit_one(1, sh.aff4);
  return ALEO_MI355X_OK;
}

int32_t Batch::fourth_finish() {
  sh.fs.absorb_g1(sh.aff4, 104, 1);
  sh.fs.squeeze_full(&sh.gamma, 1);
  sh.t_mark[4] = now_ms();
  return ALEO_MI355X_OK;
}

int32_t Batch::open_evaluate() {
  Ctx* c = sh.c; hipStream_t s = sh.s; const size_t K = sh.K, N = sh.N, m = sh.m, ne = K + 1 + 3 * m;
  const HFr &beta = sh.beta, &gamma = sh.gamma;
  // ---- evaluations -------------------------------------------------------------------------------------------------------------------------------
  RC(sh.ar.take(sh.evd, ne + 8));
  char* evd = sh.evd;
  {
    std::vector<const void*> polys; std::vector<size_t> lens; std::vector<HFr> pts;
    for (auto& p : P) for (size_t i = 0; i < p->k; ++i) { polys.push_back(p->wit + (3 * i + 2) * p->L * 32); lens.push_back(p->L); pts.push_back(beta); }
    polys.push_back(sh.g1 + 32); lens.push_back(N - 1); pts.push_back(beta);
    for (auto& p : P) for (size_t M = 0; M < 3; ++M) { polys.push_back(p->f + (p->ko[M] + 1) * 32); lens.push_back(p->nk[M] - 1); pts.push_back(gamma); }
    for (size_t at = 0; at < ne; at += 12) { const size_t cnt = ne - at < 12 ? ne - at : 12; RC(fr_eval_batch(c, evd + at * 32, polys.data() + at, lens.data() + at, pts.data() + at, cnt, s)); }
  }
  HIPCHK(hipMemcpyAsync(sh.pin_small, evd, ne * 32, hipMemcpyDeviceToHost, s));
  return ALEO_MI355X_OK;                                                                      // the caller synchronises the stream (once for all proofs of a lockstep call)
}

int32_t Batch::open_prepare() {
  Ctx* c = sh.c; hipStream_t s = sh.s; const size_t K = sh.K, N = sh.N, m = sh.m, n_k = sh.n_kmax, ne = K + 1 + 3 * m;
  const HFr &alpha = sh.alpha, &beta = sh.beta, &gamma = sh.gamma, &eta_b = sh.eta_b, &eta_c = sh.eta_c, &one = sh.one;
  char* evd = sh.evd;
  Arena& ar = sh.ar; char *pbeta, *wq, *blq, *pg, *gq;
  RC(ar.take(pbeta, 3 * N)); RC(ar.take(wq, 3 * N)); RC(ar.take(blq, HC)); RC(ar.take(pg, n_k)); RC(ar.take(gq, n_k));
  sh.evals.assign(ne, HFr::zero());
  for (size_t i = 0; i < ne; ++i) std::memcpy(sh.evals[i].l, sh.pin_small + 32 * i, 32);
  {
    std::vector<HFr> ser(sh.evals.begin(), sh.evals.begin() + K + 1);                          // Evaluations as serialised: z_b's, g_1, every g_a, every g_b, every g_c
    for (size_t M = 0; M < 3; ++M) for (size_t j = 0; j < m; ++j) ser.push_back(sh.evals[K + 1 + 3 * j + M]);
    sh.fs.absorb_fr(ser.data(), ser.size());
  }
  // one short challenge per polynomial of an opening [UPSTREAM-RECALL: sonic_pc combine_for_open], the point beta first:
  // beta: g_1, z_b of every instance, the lincheck combination;  gamma: g_{j,M} circuit by circuit, the matrix combination
  sh.ch_b.resize(K + 2); sh.ch_g.resize(3 * m + 1);
  for (auto& v : sh.ch_b) v = sh.fs.squeeze_short();          // (ch_g: squeezed below, behind the launch of the beta combination — the same sponge calls in the same order, ~2 permutations off the GPU's idle time)
  const HFr g1_beta = sh.evals[K];
  // one inversion for everything the openings divide by: alpha − beta, v_{H_j}(beta) (selectors), v_{K_{j,M}}(gamma)
  std::vector<HFr> inv(1 + 4 * m);
  inv[0] = HFr::sub(alpha, beta);
  for (auto& p : P) { inv[1 + p->j] = p->vh_beta; for (size_t M = 0; M < 3; ++M) inv[1 + m + 3 * p->j + M] = vanish(p->nk[M], gamma); }
  for (size_t i = 1 + m; i < inv.size(); ++i) if (inv[i].is_zero()) { g_last_error = "varuna_prove: gamma landed in K"; return ALEO_MI355X_ERR_HIP; }
  if (inv[0].is_zero()) { g_last_error = "varuna_prove: alpha equals beta"; return ALEO_MI355X_ERR_HIP; }
  batch_inverse_vec(inv);
  // ---- the linear combination of the first sumcheck, opened at beta together with g_1 and the z_b,i -----------------------------------------------
  const HFr xl = sh.ch_b[K + 1], vN_beta = vanish(N, beta);
  HFr cst = HFr::neg(HFr::mul(beta, g1_beta));
  HFr blw[3];                                                                     // blw: (bl(X) − bl(beta)) / (X − beta), uploaded below
  {
    Terms lc;
    lc.add(sh.mask, 3 * N, xl); lc.add(sh.h1, 2 * N, HFr::neg(HFr::mul(xl, vN_beta))); lc.add(sh.g1 + 32, N - 1, sh.ch_b[0]);
    HFr blc[3] = {HFr::zero(), HFr::zero(), HFr::zero()};
    auto axpy = [&](const HFr& coef, const HFr* src) { for (size_t t = 0; t < HC; ++t) blc[t] = HFr::add(blc[t], HFr::mul(coef, src[t])); };
    axpy(xl, &sh.blind[3 * K * HC]);
    for (auto& pp : P) {
      Prover& p = *pp;
      const HFr r_ab = HFr::mul(HFr::sub(p.vh_alpha, p.vh_beta), inv[0]);
      const HFr t_beta = HFr::add(p.sigma[0], HFr::add(HFr::mul(eta_b, p.sigma[1]), HFr::mul(eta_c, p.sigma[2])));
      const HFr sel = p.n_h == N ? one : HFr::mul(vN_beta, inv[1 + p.j]), vx_beta = vanish(p.n_x, beta);      // s_j(beta) = v_{H*}(beta) / v_{H_j}(beta)
      for (size_t i = 0; i < p.k; ++i) {
        const size_t q = p.q0 + i; const HFr& xpow = sh.ch_b[1 + q];
        const HFr x_beta = horner(p.x_poly[i], beta), zb = sh.evals[q], ci = HFr::mul(sh.comb[q], sel);
        const HFr k_za = HFr::mul(HFr::mul(xl, ci), HFr::mul(r_ab, HFr::add(one, HFr::mul(eta_c, zb))));
        const HFr k_w = HFr::neg(HFr::mul(HFr::mul(xl, ci), HFr::mul(t_beta, vx_beta)));
        cst = HFr::add(cst, HFr::mul(ci, HFr::sub(HFr::mul(HFr::mul(r_ab, eta_b), zb), HFr::mul(t_beta, x_beta))));
        lc.add(p.wit + (3 * i + 1) * p.L * 32, p.L, k_za); lc.add(p.wit + (3 * i) * p.L * 32, p.L, k_w); lc.add(p.wit + (3 * i + 2) * p.L * 32, p.L, xpow);
        axpy(k_w, &sh.blind[(3 * q) * HC]); axpy(k_za, &sh.blind[(3 * q + 1) * HC]); axpy(xpow, &sh.blind[(3 * q + 2) * HC]);
      }
    }
    RC(lc.run(c, pbeta, 3 * N, HFr::mul(xl, cst), s));
    for (auto& v : sh.ch_g) v = sh.fs.squeeze_short();
    sh.random_v = HFr::add(blc[0], HFr::mul(beta, HFr::add(blc[1], HFr::mul(beta, blc[2]))));
    blw[1] = blc[2]; blw[0] = HFr::add(blc[1], HFr::mul(beta, blc[2])); blw[2] = HFr::zero();
    char* st = sh.stage + sh.st_blq() * 32; std::memcpy(st, blw, HC * 32);
    HIPCHK(hipMemcpyAsync(blq, st, HC * 32, hipMemcpyHostToDevice, s));
  }
  // ---- the linear combination of the second sumcheck, opened at gamma together with every g_{j,M} ------------------------------------------------------
  {
    const HFr xi3m = sh.ch_g[3 * m], vk_gamma = vanish(n_k, gamma);
    Terms lc; HFr cg = HFr::zero();
    for (auto& pp : P) {
      Prover& p = *pp;
      for (size_t M = 0; M < 3; ++M) {
        const HFr fm = HFr::add(HFr::mul(gamma, sh.evals[K + 1 + 3 * p.j + M]), HFr::mul(p.sigma[M], inv_pow2(p.lg_km[M])));
        const HFr d = HFr::mul(HFr::mul(p.delta[M], xi3m), HFr::mul(vk_gamma, inv[1 + m + 3 * p.j + M]));     // selector v_{K*} / v_{K_M} at gamma
        const HFr dfm = HFr::mul(d, fm);
        const HFr cf[4] = {HFr::mul(dfm, beta), HFr::mul(dfm, alpha), HFr::mul(d, p.vv), HFr::neg(dfm)};      // row, col, val, row_col
        for (int t = 0; t < 4; ++t) lc.add((const char*)p.ix.k_polys + (4 * p.ko[M] + (size_t)t * p.nk[M]) * 32, p.nk[M], cf[t]);
        cg = HFr::sub(cg, HFr::mul(HFr::mul(dfm, alpha), beta));
      }
    }
    lc.add(sh.h2, n_k, HFr::neg(HFr::mul(xi3m, vk_gamma)));
    for (auto& pp : P) for (size_t M = 0; M < 3; ++M) lc.add(pp->f + (pp->ko[M] + 1) * 32, pp->nk[M] - 1, sh.ch_g[3 * pp->j + M]);
    RC(lc.run(c, pg, n_k, cg, s));
  }
  {                                                                                          // both witness polynomials in the same three launches
    void* q[2] = {wq, gq}; void* ev2[2] = {evd + (ne + 1) * 32, evd + (ne + 2) * 32}; const void* pp[2] = {pbeta, pg}; const size_t nn[2] = {3 * N, n_k}; const void* zz[2] = {beta.l, gamma.l};
    RC(fr_divide_by_linear_many(c, q, ev2, pp, nn, zz, 2, s));
  }
  job[0].segs = {seg(wq, 3 * N - 1, 0, 0), seg(blq, HC - 1, sh.gamma_offset, 0), seg(gq, n_k - 1, 0, 1)};
  commit_one(2, sh.aff5);                                                                     // both witness commitments in one call
  return ALEO_MI355X_OK;
}

int32_t Batch::write() {
  sh.t_mark[5] = now_ms();
  // ---- the proof in upstream's layout ---------------------------------------------------------------------------------------------------------------
  aleo_mi355x_proof_parts parts{}; std::vector<uint64_t> batch; std::vector<HFr> sums;
  for (auto& p : P) { batch.push_back(p->k); for (size_t M = 0; M < 3; ++M) sums.push_back(p->sigma[M]); }
  uint8_t has_v[2] = {1, 0}; HFr rv[2] = {sh.random_v, HFr::zero()};
  parts.batch_sizes = batch.data(); parts.n_circuits = sh.m; parts.witness_commitments = sh.wit_aff.data(); parts.mask_poly = sh.wit_aff.data() + 104 * 3 * sh.K;
  parts.g_1 = sh.aff2; parts.h_1 = sh.aff2 + 104; parts.g_abc = sh.aff3.data(); parts.h_2 = sh.aff4;
  parts.evaluations = sh.evals.data(); parts.n_evaluations = sh.evals.size(); parts.sums = sums.data();
  parts.opening_points = sh.aff5; parts.opening_random_v = rv; parts.opening_has_v = has_v; parts.n_openings = 2;
  RC(aleo_mi355x_proof_to_bytes(rq.out, rq.out_len, &parts));
  for (int i = 0; i < 5; ++i) g_varuna_timing[i] = sh.t_mark[i + 1] - sh.t_mark[i];
  g_varuna_timing[5] = sh.t_mark[5] - sh.t_mark[0];
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
