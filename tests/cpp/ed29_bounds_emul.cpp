// The field and point helpers of aleo_amd/csrc/edwards29.h (f29_tidy, f29_canonical, ed29_cache, ed29_add, ed29_dbl) and the power, square-root and Poseidon
// helpers of records_lane.h (f29_pow, f29_sqrt_fixed, psd_pow17, psd_row, psd_full, the partial rounds inside the permutation) run on the HOST over values and
// bounds together (checked_f29.h), at the CORNERS of their entry classes instead of through a whole lane: every operand is tagged with the bounds of its
// contract — an Ed29 coordinate exact digits below ED29_V r, a cached operand tidied, a tidy input lazy and below 445 r, a multiplicand with limbs up to
// 5 * 2^29 and a value below 438 r (2^261 = 438.79 r) — whatever its concrete limbs are, and the concrete values are lifted by multiples of r to sit at that edge.  Results are
// compared with host_field.hpp's HFr: the affine Edwards law on -x^2 + y^2 = 1 + 3021 x^2 y^2, HFr::pow, host::poseidon_permute<4, 8>.
//   hipcc -x c++ -std=c++17 -O2 -mbmi2 -madx -I aleo_amd/csrc tests/cpp/ed29_bounds_emul.cpp      (tests/test_ed29_bounds.py builds and runs it;
//   -DF29_HEADER='"dir/records_host.hpp"' points it at a copy that has patched copies of records_lane.h / edwards29.h beside it: the negative controls).
#include "checked_f29.h"
#include <vector>

static constexpr uint64_t ED29_V = 3;                            // edwards29.h: an Ed29 coordinate is exact digits below 3 r
static unsigned long g_mismatches;
static void mismatch(const char* what, const char* why, int id) { if (g_mismatches++ < 10) std::fprintf(stderr, "mismatch: %s, case %d: %s\n", what, id, why); }

// ---- representatives ------------------------------------------------------------------------------------------------------------------------------------
static Big big_add(const Big& a, const Big& b) { Big r; uint64_t c = 0; for (int i = 0; i < 5; ++i) { const u128 t = (u128)a.w[i] + b.w[i] + c; r.w[i] = (uint64_t)t; c = (uint64_t)(t >> 64); } return r; }
static Big big_sub(const Big& a, const Big& b) { Big r; uint64_t br = 0; for (int i = 0; i < 5; ++i) { const u128 t = (u128)a.w[i] - b.w[i] - br; r.w[i] = (uint64_t)t; br = (uint64_t)(t >> 64) & 1; } return r; }
static void big_digits29(const Big& a, uint32_t* v9) {
  for (int i = 0; i < 8; ++i) v9[i] = (uint32_t)big_shr(a, 29 * i).w[0] & M29;
  const Big top = big_shr(a, 232); if (top.w[0] >> 32 || top.w[1]) { std::fprintf(stderr, "big_digits29: value does not fit 9 limbs\n"); std::exit(2); }
  v9[8] = (uint32_t)top.w[0];
}
// the digits of x 2^261 mod r + k r
static void lifted(uint32_t* v9, const HFr& x, uint32_t k) { uint32_t c[9]; put29(c, x); big_digits29(big_add(big_of_limbs(c), big_mul64(RB, k)), v9); }
// ... tagged exact digits below vmul r: the bounds of a contract
static F29 tagged(const HFr& x, uint32_t k, uint64_t vmul) { uint32_t d[9]; lifted(d, x, k); return exact_below(d, vmul * UNIT); }
// ... with every limb lending `units` to the one below, tagged lazy: limbs 0..7 below (units + 1) 2^29, value below vmul r
static F29 tagged_lazy(const HFr& x, uint32_t k, uint64_t vmul, uint32_t units) {
  F29 r; lifted(r.v, x, k);
  for (int i = 7; i >= 0; --i) { const uint32_t q = r.v[i + 1] < units ? r.v[i + 1] : units; r.v[i + 1] -= q; r.v[i] += q << 29; }
  for (int i = 0; i < 8; ++i) r.b[i] = (((uint64_t)units + 1) << 29) - 1;
  r.vb = vmul * UNIT; r.b[8] = top_limb_below(r.vb); r.exact = false; return r;
}
static const HFr INV32 = HFr::inv(HFr::from_u64(32));
static HFr residue(const F29& a) {                               // the field element a stands for, whatever multiple of r its limbs carry
  Big v = big_of_limbs(a.v); while (big_cmp(v, RB) >= 0) v = big_sub(v, RB);
  HFr h; for (int i = 0; i < 4; ++i) h.l[i] = v.w[i];
  return HFr::mul(h, INV32);
}
static HFr rnd_hfr() { uint8_t b[32]; rnd_fr(b); HFr v; std::memcpy(v.l, b, 32); return HFr::to_mont(v); }

// ---- the affine law ---------------------------------------------------------------------------------------------------------------------------------------
struct Aff { HFr x, y; };
static const HFr D = HFr::from_u64(ED_D);
static bool on_curve(const Aff& p) { const HFr xx = HFr::sqr(p.x), yy = HFr::sqr(p.y); return HFr::sub(yy, xx) == HFr::add(HFr::one(), HFr::mul(D, HFr::mul(xx, yy))); }
static Aff aff_add(const Aff& p, const Aff& q) {
  const HFr t = HFr::mul(D, HFr::mul(HFr::mul(p.x, q.x), HFr::mul(p.y, q.y))), one = HFr::one();
  Aff r; r.x = HFr::mul(HFr::add(HFr::mul(p.x, q.y), HFr::mul(p.y, q.x)), HFr::inv(HFr::add(one, t)));
  r.y = HFr::mul(HFr::add(HFr::mul(p.y, q.y), HFr::mul(p.x, q.x)), HFr::inv(HFr::sub(one, t)));
  return r;
}
static Aff aff_neg(const Aff& p) { Aff r; r.x = HFr::neg(p.x); r.y = p.y; return r; }
static Aff rnd_point() {
  for (;;) {
    Aff p; p.x = rnd_hfr(); const HFr xx = HFr::sqr(p.x);
    if (hfr_sqrt(p.y, HFr::mul(HFr::add(HFr::one(), xx), HFr::inv(HFr::sub(HFr::one(), HFr::mul(D, xx)))), records_consts().sq) && on_curve(p)) return p;
  }
}
struct Rep { uint32_t k[4]; };                                   // the multiple of r added to X, Y, Z, T
static const Rep REPS[3] = {{{0, 0, 0, 0}}, {{2, 2, 2, 2}}, {{2, 0, 1, 2}}};      // canonical; the largest below 3 r; a mix
static Ed29 make_point(const Aff& p, const HFr& z, const Rep& r) {
  Ed29 e; e.X = tagged(HFr::mul(p.x, z), r.k[0], ED29_V); e.Y = tagged(HFr::mul(p.y, z), r.k[1], ED29_V);
  e.Z = tagged(z, r.k[2], ED29_V); e.T = tagged(HFr::mul(HFr::mul(p.x, p.y), z), r.k[3], ED29_V); return e;
}
static void check_point(const Ed29& p, const Aff& want, const char* what, int id) {
  const HFr X = residue(p.X), Y = residue(p.Y), Z = residue(p.Z), T = residue(p.T);
  if (Z.is_zero()) { mismatch(what, "Z is 0 mod r", id); return; }
  if (!(HFr::mul(T, Z) == HFr::mul(X, Y))) mismatch(what, "T Z != X Y", id);
  const HFr zi = HFr::inv(Z);
  if (!(HFr::mul(X, zi) == want.x) || !(HFr::mul(Y, zi) == want.y)) mismatch(what, "not the affine sum", id);
}
static void closure(const Ed29& p, const char* fn, bool with_t = true) {
  f29_closure(p.X, ED29_V * UNIT, 0, "a returned X is not exact digits below 3 r", fn); f29_closure(p.Y, ED29_V * UNIT, 1, "a returned Y is not exact digits below 3 r", fn);
  f29_closure(p.Z, ED29_V * UNIT, 2, "a returned Z is not exact digits below 3 r", fn);
  if (with_t) f29_closure(p.T, ED29_V * UNIT, 3, "a returned T is not exact digits below 3 r", fn);
}
static void retag(Ed29& p) { p.X = exact_below(p.X.v, ED29_V * UNIT); p.Y = exact_below(p.Y.v, ED29_V * UNIT); p.Z = exact_below(p.Z.v, ED29_V * UNIT); p.T = exact_below(p.T.v, ED29_V * UNIT); }

static unsigned long n_tidy, n_canonical, n_cache, n_add[2], n_dbl[2], n_pow, n_sqrt, n_pow17, n_row, n_full[2], n_permute[2];
static unsigned long b_canonical_subtracts, b_canonical_keeps, b_sqrt_square, b_sqrt_nonsquare, b_sqrt_zero, b_add_same, b_add_opposite, b_identity_operand, b_order4_operand;

static const uint32_t* K;
static void run_add(Ed29 p, const Aff& P, const Ed29& q, const Aff& Q, bool neg, bool cached_at_edge, int id) {
  t_formula = "ed29_cache"; Ed29Cached c = ed29_cache(q, rk_const(K, RK_D2)); ++n_cache;
  { const F29* f[4] = {&c.ym, &c.yp, &c.k, &c.z2}; for (int i = 0; i < 4; ++i) f29_closure(*f[i], ED29_V * UNIT, i, "a cached operand is not exact digits below 3 r", "ed29_cache"); }
  if (cached_at_edge) { c.ym = exact_below(c.ym.v, ED29_V * UNIT); c.yp = exact_below(c.yp.v, ED29_V * UNIT); c.k = exact_below(c.k.v, ED29_V * UNIT); c.z2 = exact_below(c.z2.v, ED29_V * UNIT); }
  t_formula = "ed29_add"; ed29_add(p, c, neg); ++n_add[neg]; closure(p, "ed29_add"); t_formula = nullptr;
  check_point(p, aff_add(P, neg ? aff_neg(Q) : Q), neg ? "ed29_add (neg)" : "ed29_add", id);
}
static void run_dbl(Ed29 p, const Aff& P, bool want_t, int id) {
  const Ed29 before = p;
  t_formula = "ed29_dbl"; ed29_dbl(p, want_t); ++n_dbl[want_t]; closure(p, "ed29_dbl", want_t); t_formula = nullptr;
  if (!want_t) {
    if (std::memcmp(p.T.v, before.T.v, 36)) mismatch("ed29_dbl", "T touched though it was not wanted", id);
    p.T = tagged(HFr::mul(HFr::mul(residue(p.X), residue(p.Y)), HFr::inv(residue(p.Z))), 0, ED29_V);      // for the check below only
  }
  check_point(p, aff_add(P, P), "ed29_dbl", id);
}

int main() {
  const RecordsConsts& C = records_consts(); K = C.words.data();
  const HFr one = HFr::one(), zero = HFr::zero();
  int id = 0;

  // ---- f29_tidy: lazy limbs (every limb seven units of 2^29), values up to the last multiple below 445 r
  for (int i = 0; i < 24; ++i) {
    const HFr x = i == 0 ? zero : (i == 1 ? HFr::neg(one) : rnd_hfr());
    const uint32_t k = (i & 1) ? 444 : (i & 2 ? 17 : 0);
    F29 a = tagged_lazy(x, k, 445, (i & 4) ? 6 : 0);
    t_formula = "f29_tidy"; f29_tidy(a); ++n_tidy;
    f29_closure(a, 3 * UNIT, 0, "f29_tidy returns more than exact digits below 3 r", "f29_tidy"); t_formula = nullptr;
    if (!(residue(a) == x)) mismatch("f29_tidy", "another residue", ++id);
  }
  // ---- f29_canonical: a multiplicand at the edge of its class (limbs up to 5 * 2^29 - 1, value below 438 r < 2^261); 0 and r themselves
  for (int i = 0; i < 24; ++i) {
    const HFr x = i < 4 ? zero : (i < 6 ? HFr::neg(one) : rnd_hfr());      // -1: the canonical number r - 1
    const uint32_t k = i < 4 ? (uint32_t)i % 2 * (i < 2 ? 1 : 437) : ((i & 1) ? 437 : 0);
    const F29 a = tagged_lazy(x, k, 438, (i & 2) ? 4 : 0);
    t_formula = "f29_canonical"; const F29 c = f29_canonical(a); ++n_canonical; t_formula = nullptr;
    uint32_t want[9]; put_plain29(want, HFr::from_mont(x).l);
    if (std::memcmp(c.v, want, 36)) mismatch("f29_canonical", "not the canonical number", ++id);
    if (x.is_zero() && k) ++b_canonical_subtracts; else ++b_canonical_keeps;            // a non-zero multiple of r leaves exactly r: the one case that subtracts
  }

  // ---- the points
  std::vector<Aff> P; for (int i = 0; i < 3; ++i) P.push_back(rnd_point());
  HFr im; if (!hfr_sqrt(im, HFr::neg(one), C.sq)) return 2;      // sqrt(-1)
  const Aff O{zero, one}, M{zero, HFr::neg(one)}, I4{im, zero}, I4n{HFr::neg(im), zero};
  auto times = [&](Aff p, int n) { Aff r = O; for (int i = 0; i < n; ++i) r = aff_add(r, p); return r; };
  const Aff L = times(P[0], 4), L2 = aff_add(L, M), L4 = aff_add(L, I4);      // order l, 2 l, 4 l (P[0] has order dividing 4 l)
  for (const Aff& p : {O, M, I4, I4n, L, L2, L4, P[0], P[1], P[2]}) if (!on_curve(p)) { std::fprintf(stderr, "a test point is not on the curve\n"); return 2; }
  if (!(HFr::mul(im, im) == HFr::neg(one)) || !(aff_add(I4, I4).y == M.y)) return 2;
  const std::vector<Aff> pts = {O, M, I4, I4n, L, L2, L4, P[1], P[2]};
  const HFr zs[3] = {one, rnd_hfr(), rnd_hfr()};
  int n = 0;
  for (size_t a = 0; a < pts.size(); ++a) for (size_t b = 0; b < pts.size(); ++b) {
    const Rep &ra = REPS[(a + b) % 3], &rb = REPS[(a + 2 * b + 1) % 3]; const HFr &za = zs[(a + b) % 3], &zb = zs[(2 * a + b + 1) % 3];
    const Ed29 p = make_point(pts[a], za, ra), q = make_point(pts[b], zb, rb);
    for (int neg = 0; neg < 2; ++neg) run_add(p, pts[a], q, pts[b], neg, (n++ & 1) != 0, ++id);
    b_identity_operand += a == 0 || b == 0; b_order4_operand += a == 2 || a == 3 || b == 2 || b == 3; b_add_same += a == b;
  }
  for (size_t a = 0; a < pts.size(); ++a) for (int rep = 0; rep < 3; ++rep) {
    const Ed29 p = make_point(pts[a], zs[(a + rep) % 3], REPS[rep]);
    run_add(p, pts[a], make_point(aff_neg(pts[a]), zs[rep], REPS[(rep + 1) % 3]), aff_neg(pts[a]), false, rep == 1, ++id); ++b_add_opposite;      // P + (-P)
    run_dbl(p, pts[a], true, ++id); run_dbl(p, pts[a], false, ++id);
  }
  // chains: what a formula returns is the next one's operand, with the bounds it came back with, then re-tagged with the contract alone
  for (int chain = 0; chain < 2; ++chain) {
    Ed29 p = make_point(L4, zs[1], REPS[1]); Aff sum = L4;
    const Ed29 q = make_point(P[1], zs[2], REPS[2]);
    t_formula = "ed29_cache"; const Ed29Cached qc = ed29_cache(q, rk_const(K, RK_D2)); ++n_cache;
    for (int s = 0; s < 12; ++s) {
      const bool t = (s % 3) != 0, neg = (s & 1) != 0;
      t_formula = "ed29_dbl"; ed29_dbl(p, t); ++n_dbl[t]; closure(p, "ed29_dbl", t); sum = aff_add(sum, sum);
      if (t) { t_formula = "ed29_add"; ed29_add(p, qc, neg); ++n_add[neg]; closure(p, "ed29_add"); sum = aff_add(sum, neg ? aff_neg(P[1]) : P[1]); check_point(p, sum, "chain", ++id); }
      if (chain) retag(p);
    }
    t_formula = nullptr;
  }

  // ---- f29_pow, f29_sqrt_fixed: a normalised base below 3 r
  for (int i = 0; i < 6; ++i) {
    const HFr x = i == 0 ? zero : (i == 1 ? one : rnd_hfr());
    const F29 a = tagged(x, i & 1 ? 2 : 0, 3);
    t_formula = "f29_pow"; const F29 inv = f29_pow(a, K + RK_EXP_INV, RK_INV_BITS); ++n_pow; t_formula = nullptr;
    if (!(residue(inv) == (x.is_zero() ? zero : HFr::inv(x)))) mismatch("f29_pow", "not x^(r-2)", ++id);
  }
  for (int i = 0; i < 8; ++i) {
    const HFr y = rnd_hfr(); HFr x = i == 0 ? zero : HFr::sqr(y);
    if (i >= 5) x = HFr::mul(x, HFr::from_u64(host::FR_GENERATOR));      // a non-residue times a square
    const F29 a = tagged(x, i & 1 ? 2 : 0, 3);
    t_formula = "f29_sqrt_fixed"; const F29 s = f29_sqrt_fixed(a, K); ++n_sqrt; t_formula = nullptr;
    const bool is_root = HFr::sqr(residue(s)) == x;
    if (i >= 5) { ++b_sqrt_nonsquare; if (is_root) mismatch("f29_sqrt_fixed", "a root of a non-square", ++id); }
    else { if (i == 0) ++b_sqrt_zero; else ++b_sqrt_square; if (!is_root) mismatch("f29_sqrt_fixed", "not a root", ++id); }
  }

  // ---- Poseidon: the state's entry class is a tidied element (below 3 r) plus a product or a constant (lazy, below 5 r)
  const auto& PP = host::PoseidonParams<4, 8>::get();
  auto pow17 = [](const HFr& v) { HFr a = HFr::sqr(v); a = HFr::sqr(a); a = HFr::sqr(a); a = HFr::sqr(a); return HFr::mul(a, v); };
  auto entry = [&](const HFr& v, int i) {                        // v as tidied part + product part, both lifted to their edges
    const HFr part = rnd_hfr(); t_formula = "psd_entry";
    return f29_add(tagged(HFr::sub(v, part), (i & 1) ? 2 : 0, 3), tagged(part, (i & 2) ? 1 : 0, 2));
  };
  for (int round = 0; round < 4; ++round) {
    HFr h[9]; F29 s[9];
    for (int i = 0; i < 9; ++i) { h[i] = (round == 0 && i < 2) ? (i ? HFr::neg(one) : zero) : rnd_hfr(); s[i] = entry(h[i], i + round); }
    // psd_pow17 on the lazy sum, psd_row over products and tidied elements
    for (int i = 0; i < 9; ++i) { t_formula = "psd_pow17"; const F29 p = psd_pow17(s[i]); ++n_pow17; t_formula = nullptr; if (!(residue(p) == pow17(h[i]))) mismatch("psd_pow17", "not x^17", ++id); }
    {
      F29 t[9]; HFr want = zero;
      for (int j = 0; j < 9; ++j) { t[j] = tagged(h[j], (j + round) % 3, 3); want = HFr::add(want, HFr::mul(h[j], PP.mds[round][j])); }
      t_formula = "psd_row"; const F29 row = psd_row(t, K, RK_MDS + 9 * round); ++n_row;
      f29_closure(row, 3 * UNIT, 0, "psd_row returns more than exact digits below 3 r", "psd_row"); t_formula = nullptr;
      if (!(residue(row) == want)) mismatch("psd_row", "not the row's sum", ++id);
    }
    // one full round, all of it and the last one's single element
    HFr w[9]; for (int i = 0; i < 9; ++i) w[i] = pow17(HFr::add(h[i], PP.ark[0][i]));
    F29 f[9]; for (int i = 0; i < 9; ++i) f[i] = s[i];
    t_formula = "psd_full"; psd_full<false>(f, K, RK_ARK_HEAD, RK_MDS); ++n_full[0]; t_formula = nullptr;
    for (int i = 0; i < 9; ++i) { HFr want = zero; for (int j = 0; j < 9; ++j) want = HFr::add(want, HFr::mul(w[j], PP.mds[i][j])); if (!(residue(f[i]) == want)) mismatch("psd_full<false>", "not the round", ++id); }
    for (int i = 0; i < 9; ++i) f[i] = s[i];
    t_formula = "psd_full"; psd_full<true>(f, K, RK_ARK_HEAD, RK_MDS); ++n_full[1]; t_formula = nullptr;
    { HFr want = zero; for (int j = 0; j < 9; ++j) want = HFr::add(want, HFr::mul(w[j], PP.mds[1][j])); if (!(residue(f[1]) == want)) mismatch("psd_full<true>", "not element 1 of the round", ++id); }
    // the whole permutation (its 31 partial rounds are in no function of their own): every element, and element 1 alone
    HFr ref[9]; for (int i = 0; i < 9; ++i) ref[i] = h[i];
    host::poseidon_permute<4, 8>(ref);
    for (int i = 0; i < 9; ++i) f[i] = s[i];
    t_formula = "psd_permute"; psd_permute(f, K); ++n_permute[0];
    for (int i = 0; i < 9; ++i) { f29_closure(f[i], 3 * UNIT, 0, "psd_permute returns more than exact digits below 3 r", "psd_permute"); if (!(residue(f[i]) == ref[i])) mismatch("psd_permute", "not the permutation", ++id); }
    // ... and again from what it returned, one more lazy summand on an element: the sponge's next block
    for (int i = 0; i < 9; ++i) h[i] = ref[i];
    const HFr extra = rnd_hfr(); h[2] = HFr::add(h[2], extra); f[2] = f29_add(f[2], tagged(extra, 1, 2));
    for (int i = 0; i < 9; ++i) ref[i] = h[i];
    host::poseidon_permute<4, 8>(ref);
    t_formula = "psd_permute_take1"; const F29 one_out = psd_permute_take1(f, K); ++n_permute[1]; t_formula = nullptr;
    if (!(residue(one_out) == ref[1])) mismatch("psd_permute_take1", "not element 1 of the permutation", ++id);
  }

  std::printf("calls: tidy %lu, canonical %lu, cache %lu, add %lu, add_neg %lu, dbl %lu, dbl_t %lu, pow %lu, sqrt %lu, pow17 %lu, row %lu, full %lu, full_last %lu, permute %lu, permute_take1 %lu\n",
              n_tidy, n_canonical, n_cache, n_add[0], n_add[1], n_dbl[0], n_dbl[1], n_pow, n_sqrt, n_pow17, n_row, n_full[0], n_full[1], n_permute[0], n_permute[1]);
  std::printf("branches: canonical_subtracts %lu, canonical_keeps %lu, sqrt_square %lu, sqrt_nonsquare %lu, sqrt_zero %lu, add_same_point %lu, add_opposite %lu, identity_operand %lu, order4_operand %lu\n",
              b_canonical_subtracts, b_canonical_keeps, b_sqrt_square, b_sqrt_nonsquare, b_sqrt_zero, b_add_same, b_add_opposite, b_identity_operand, b_order4_operand);
  std::printf("ed29_bounds_emul: %lu point operations, %lu mismatches, %lu limb-rule violations\n", n_cache + n_add[0] + n_add[1] + n_dbl[0] + n_dbl[1], g_mismatches, g_violations);
  return g_mismatches || g_violations ? 1 : 0;
}
