// varuna_host.h — private to the prover's host side (varuna*.hip): the host helpers it shares (field odds and ends, the workspace arena, MSM segments,
// term lists) and the declarations of what crosses its files — the state of a proof (Shared, Prover, Batch) and the routed transforms / commitments.
#pragma once
#include "ctx.h"
#include "frops.h"
#include "host_field.hpp"
#include "poseidon.hpp"
#include "chacha.h"
#include <chrono>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

namespace aleo_mi355x {

using host::HFr;

#define RC(call) { int32_t rc_ = (call); if (rc_) return rc_; }

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline uint32_t lg2(uint64_t n) { uint32_t lg = 0; while ((1ull << lg) < n) ++lg; return lg; }      // ceil(log2 n)
inline MsmSeg seg(const void* d_ptr, size_t len, size_t off, size_t out) { return MsmSeg{d_ptr, len, off, (uint32_t)out}; }
// element `index` of the proof's random stream (chacha.h; the same definition as k_fr_random in frops.hip), Montgomery form
inline HFr random_fr(const Seed32& seed, uint64_t index) {
  uint32_t w[8]; chacha_fr(w, seed.w, index);
  HFr v; std::memcpy(v.l, w, 32); return HFr::to_mont(v);
}
inline HFr vanish(uint64_t size, const HFr& x) { return HFr::sub(HFr::pow_u64(x, size), HFr::one()); }     // x^size − 1
inline HFr domain_gen(uint64_t size) {                    // TWO_ADIC_ROOT^(2^(47 − lg size))
  HFr g; std::memcpy(g.l, host::FR_TWO_ADIC_ROOT_CANON, 32); g = HFr::to_mont(g);
  for (int i = (int)lg2(size); i < host::FR_TWO_ADICITY; ++i) g = HFr::sqr(g);
  return g;
}
inline HFr inv_pow2(uint32_t lg) {                          // 1 / 2^lg: lg products by 1/2 instead of a Fermat chain
  static const HFr half = HFr::inv(HFr::from_u64(2));
  HFr r = HFr::one(); for (uint32_t i = 0; i < lg; ++i) r = HFr::mul(r, half); return r;
}
// a <- (sum_t a_t w^(t u))_u for a primitive |a|-th root w, |a| a power of two: bit-reversal + radix-2 butterflies, O(n log n) host products
inline void host_ntt(std::vector<HFr>& a, const HFr& w) {
  const size_t n = a.size();
  for (size_t i = 1, j = 0; i < n; ++i) { size_t bit = n >> 1; for (; j & bit; bit >>= 1) j ^= bit; j ^= bit; if (i < j) std::swap(a[i], a[j]); }
  std::vector<HFr> tw(n > 1 ? n / 2 : 1);
  tw[0] = HFr::one(); for (size_t i = 1; i < n / 2; ++i) tw[i] = HFr::mul(tw[i - 1], w);
  for (size_t len = 2; len <= n; len <<= 1)
    for (size_t i = 0; i < n; i += len)
      for (size_t t = 0; t < len / 2; ++t) {
        const HFr u = a[i + t], v = HFr::mul(a[i + t + len / 2], tw[t * (n / len)]);
        a[i + t] = HFr::add(u, v); a[i + t + len / 2] = HFr::sub(u, v);
      }
}
inline HFr horner(const std::vector<HFr>& p, const HFr& x) { HFr a = HFr::zero(); for (size_t i = p.size(); i-- > 0;) a = HFr::add(HFr::mul(a, x), p[i]); return a; }
inline void batch_inverse_vec(std::vector<HFr>& v) {        // Montgomery's trick on the host: one inversion for all (non-zero) values
  std::vector<HFr> pre(v.size()); HFr acc = HFr::one();
  for (size_t i = 0; i < v.size(); ++i) { pre[i] = acc; acc = HFr::mul(acc, v[i]); }
  acc = HFr::inv(acc);
  for (size_t i = v.size(); i-- > 0;) { const HFr t = HFr::mul(acc, pre[i]); acc = HFr::mul(acc, v[i]); v[i] = t; }
}

struct Arena {                                             // bump allocation inside the slot's prover workspace
  char* base; size_t off = 0, cap;
  int32_t take(char*& p, size_t elems) {                   // p <- the next block of `elems` field elements
    p = base + off; off += (elems * 32 + 255) & ~(size_t)255; if (off <= cap) return ALEO_MI355X_OK;
    p = nullptr; g_last_error = "varuna_prove: workspace accounting"; return ALEO_MI355X_ERR_HIP;
  }
};
static constexpr size_t HC = 3;                            // coefficients of a hiding polynomial (hiding bound 1)
static constexpr size_t MAX_INSTANCES = 32;               // one proof covers one transaction: at most 32 transitions, in any split over circuits
static constexpr size_t PIN_SUMS = 8192, PIN_FLAG = 9216, PIN_SMALL_BYTES = 12288;      // small read-backs behind the staging area: evaluations / sigma values from 0 (<= 129 x 32 bytes), the circuits' sums over H, the canonical-input flag
// sum_i co_i p_i over polynomials of any lengths, collected entry by entry
struct Terms {
  std::vector<const void*> ptr; std::vector<size_t> len; std::vector<HFr> co;
  void add(const void* p, size_t n, const HFr& k) { ptr.push_back(p); len.push_back(n); co.push_back(k); }
  // dst (n values) = c0 at X^0 + the sum: fr_lincomb takes 28 terms per launch, later launches carry dst along as a term
  int32_t run(Ctx* c, char* dst, size_t n, const HFr& c0, hipStream_t s) const {
    constexpr size_t LC = 28; size_t at = 0; bool first = true;
    do {
      const void* t[LC]; size_t l[LC]; HFr k[LC]; size_t nt = 0;
      if (!first) { t[nt] = dst; l[nt] = n; k[nt++] = HFr::one(); }
      while (nt < LC && at < ptr.size()) { t[nt] = ptr[at]; l[nt] = len[at]; k[nt++] = co[at++]; }
      RC(fr_lincomb(c, dst, n, first ? c0.l : nullptr, t, l, k, nt, s));
      first = false;
    } while (at < ptr.size());
    return ALEO_MI355X_OK;
  }
};

// The state of one proof between the rounds (upstream: varuna::ahp::prover::State) and the round functions in the order upstream calls them.
// A proof covers m circuits (`keys_to_constraints: BTreeMap<&ProvingKey, &[Assignment]>`), each with its own instances: `Shared` is what they share —
// the transcript and every challenge, the mask and g_1, h_1 over the largest constraint domain H*, h_2 over the largest non-zero domain K*, the two
// openings — and one `Prover` per circuit holds that circuit's polynomials.  Circuit j enters the first sumcheck behind the selector
// s_j = v_{H*} / v_{H_j} = sum_t X^(t |H_j|): its quotient adds into h_1 as it is, its remainder block tiles over H* (fr_add_tiled); see
// oracle/varuna_ref.py prove_batch for the algebra.  With one circuit nothing is added or tiled: the circuit writes the shared buffers directly.
struct Shared {
  Ctx* c; const PinnedBases& pb; Seed32 seed;
  Shared(Ctx* c_, const PinnedBases& pb_, const uint8_t* seed32) : c(c_), pb(pb_) { std::memcpy(seed.w, seed32, 32); }
  size_t m = 0, K = 0, N = 0, n_kmax = 0, lead = 0, x_total = 0; uint64_t D = 0, gamma_offset = 0;
  hipStream_t s = nullptr; double t_mark[7] = {}; Arena ar{nullptr, 0, 0}; char* pin = nullptr; char* stage = nullptr; char* pin_small = nullptr; char* pin_small_dev = nullptr;      // pin_small_dev: the device's address of pin_small (kernels store small read-backs there)
  HFr one, neg1, r2; host::FiatShamir fs; uint64_t lay_mask = 0, lay_blind = 0, lay_blind_mask = 0;
  char *mask = nullptr, *bl = nullptr, *h1 = nullptr, *g1 = nullptr, *h2 = nullptr, *flag = nullptr, *evd = nullptr;
  std::vector<HFr> blind, comb, evals, x_mont, ch_b, ch_g; std::vector<uint8_t> wit_aff, aff3;
  uint8_t aff2[208], aff4[104], aff5[208];
  HFr alpha, eta_b, eta_c, beta, gamma, random_v;
  // staging offsets (elements of 32 bytes inside `stage`): x̂ coefficients | hiding polynomials | the opening's hiding quotient | rho
  size_t st_blind() const { return x_total; }
  size_t st_blq() const { return x_total + (3 * K + 1) * HC; }
  size_t st_rho() const { return st_blq() + HC; }
};

struct Prover {                                            // one circuit of the proof
  Shared& sh; const aleo_mi355x_varuna_index& ix; const size_t j, k, q0;      // circuit number, its instances, the number of its first instance in the proof
  Prover(Shared& sh_, const aleo_mi355x_varuna_index& ix_, size_t j_, size_t k_, size_t q0_) : sh(sh_), ix(ix_), j(j_), k(k_), q0(q0_) {}
  size_t n_h = 0, n_x = 0, L = 0, n4 = 0, nk[3] = {}, ko[3] = {}, k_sum = 0, n_k = 0, x_off = 0, pin_off = 0; uint32_t lg_h = 0, lg_km[3] = {};
  char *xp = nullptr, *wit = nullptr, *ext = nullptr, *hq = nullptr, *rq = nullptr, *f = nullptr, *evals_h = nullptr, *rho_dev = nullptr;
  char *E = nullptr, *F = nullptr;
  std::vector<std::vector<HFr>> x_poly;
  HFr vh_alpha, vh_beta, vv, sigma[3], delta[3];
  size_t run0[3] = {}, runc[3] = {}, nrun = 0;
  bool lead() const { return sh.lead == j; }
  bool lagrange() const { return ix.lagrange_offset != 0; }

  int32_t setup();
  size_t workspace_elems() const { return n_h * (41 + 24 * k) + k_sum * 6 + n_k * 4 + 4096; }
  int32_t first_round(const void* const* assignments, std::vector<MsmSeg>& sg);      // AHPForR1CS::prover_first_round for this circuit's instances
  int32_t second_round_early();                            // its challenge-free part (operands of the sumcheck on 4|H|): queued behind round 1's commitments
  int32_t second_round();                                  // prover_second_round: t, this circuit's summand of the first sumcheck, its quotient and remainder
  int32_t third_round();                                   // prover_third_round: f_M (sigma_M, g_M follow the read-back)
  int32_t fourth_round_early();                            // its challenge-free part (f_M on the domains of size 2|K_M|): queued behind round 3's commitments
  int32_t fourth_round(Terms& h2);                         // prover_fourth_round: the quotients h_M of this circuit, delta-weighted, run by run: terms of h_2
};
// ---- the proof: rounds over all circuits, commitments and transcript in between -----------------------------------------------------------------------
// Every round is three steps: prepare (queue the round's kernels on the stream, list the commitments it needs as RoundJobs), the commitment(s)
// (run_commits, varuna.hip: ONE launch chain for the jobs of every proof of the call), finish (absorb the commitments, squeeze the challenges).
struct RoundJob { std::vector<MsmSeg> segs; uint32_t k = 0; bool sparse = false; uint8_t* out = nullptr; };      // k results (104-byte affine) to `out`
struct Batch {
  Shared sh; std::vector<std::unique_ptr<Prover>> P;
  ProveRequest& rq;                                     // what to prove, where the proof goes (assignments: the instances of circuit 0, then of circuit 1, ...)
  RoundJob job[2]; int njobs = 0; std::function<int32_t()> hook;      // this round's commitments; kernels to queue behind the last commitment chain
  size_t need_ws_bytes = 0, need_pin_bytes = 0, pin_elems = 0, stage_elems = 0;
  Batch(Ctx* c, const PinnedBases& pb, ProveRequest& rq_) : sh(c, pb, rq_.seed32), rq(rq_) {}
  // the round commits job[0].segs to k results at `out`; the split first round: job[0].segs sparse to k at `out`, then job[1].segs to one more behind them
  void commit_one(size_t k, uint8_t* out, std::function<int32_t()> behind = nullptr, bool sparse = false) {
    njobs = 1; job[0].k = (uint32_t)k; job[0].sparse = sparse; job[0].out = out; hook = std::move(behind);
  }
  void commit_split(size_t k, uint8_t* out, std::function<int32_t()> behind) {
    commit_one(k, out, std::move(behind), true); njobs = 2; job[1].k = 1; job[1].sparse = false; job[1].out = out + 104 * k;
  }
  int32_t init_sponge();                                   // Varuna::init_sponge: protocol name, batch sizes, public inputs, index commitments
  int32_t setup();                                         // checks + sizes (need_ws_bytes, need_pin_bytes)
  int32_t attach(char* ws, size_t ws_bytes, char* pin);    // the slices of the slot's device workspace and pinned staging this proof works in
  int32_t first_prepare(); int32_t first_finish();      // the 3K + 1 hiding commitments
  int32_t second_prepare(); int32_t second_finish();       // g_1, h_1
  int32_t third_prepare(); int32_t third_finish();         // sigma_{j,M}, g_{j,M}
  int32_t fourth_prepare(); int32_t fourth_finish();       // h_2
  int32_t open_evaluate();                                 // the evaluation kernels and their read-back (queued; the caller synchronises)
  int32_t open_prepare();                                  // evaluations into the transcript, the two linear combinations, both witness polynomials
  int32_t write();                                         // Proof::write_le, the timing of the rounds
};

// varuna.hip: the prover's transforms and commitments, over the devices of a sharded committer key where one is attached
int32_t p_ntt(Ctx* c, const PinnedBases& pb, void* data, uint32_t lg, size_t batch, int32_t direction, int32_t type, hipStream_t s);
int32_t p_ntt_from(Ctx* c, const PinnedBases& pb, void* out, const void* src, size_t src_stride, size_t src_len, uint32_t lg, size_t batch, hipStream_t s);
int32_t commit(Ctx* c, const PinnedBases& pb, const std::vector<MsmSeg>& segs, uint32_t k, uint8_t* out104, hipStream_t s, bool sparse = false,
               std::function<int32_t()> behind = nullptr);

}  // namespace aleo_mi355x
