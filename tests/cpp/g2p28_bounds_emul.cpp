// The G2 lane-pair formulas of aleo_amd/csrc/g2p28.h (g2p_madd_fast, g2p_double, g2p_add, g2p_add_any, g2p_double_any, with fq2p_mul, f28_neg5 and
// g2p_negate_entry under them) run on the HOST as two threads, over values and bounds together, against the affine group law over host_field.hpp's HFq2.
//
// The harness is checked_f28.h (which fp28_bounds_emul.cpp and te28_bounds_emul.cpp use too): limbs that carry a bound each, a value bound in multiples of q,
// an exact-digits flag; primitives that compute what the device computes, propagate the bounds from the operation alone and check their preconditions
// against the BOUNDS.  Operands are TAGGED with the full stated invariant whatever their concrete limbs are — a stored point or accumulator: X exact < 12q,
// Y exact < 6q, ZZ / ZZZ exact < 2q; an entry: exact < 2q; a negated entry: what g2p_negate_entry makes of a canonical row — so one run speaks for every
// input inside the invariant:
//   limb     no 32-bit limb wraps in add / sub / 5 v / normalise; no limb 0..12 of a difference (K q - 5 v with its spread of 6 included) can go negative
//   column   every column of the merged product x b1 + ox b2, carry-in included, stays below 2^64 (and what is left for the top limb below 2^32)
//   value    the subtrahend's top limb fits the constant's (5 v < K q; X1 < 16q; ...); normalise sees < 2^392; the == 0 (mod q) tests see exact digits < 2q
//   closure  what a formula stores, and what g2p_madd_fast leaves in acc, satisfies the stored invariant again
//   sound    every concrete limb and value is within its tracked bound (the bookkeeping itself)
// A broken rule prints itself with the g2p28.h line and is counted.  The concrete operands: representatives lifted independently per component (canonical,
// the largest lift below 12q / 6q / 2q, a-component and b-component lifted differently), Z = 1 / in the base field / general, the same point, opposite
// points, the identity on either side and on both, y = (0, 0) (2-torsion), x = (0, 0), components that are 0, the negated entry of y = 0 (exactly 2q), and
// operands whose x and Z lie in the base field, for which ZZ3 = (z, 0) with z != 0: one zero component is not the zero of Fq2.
// The a = 0 formulas never use the curve's b, so every case brings its own curve y^2 = x^3 + b on which its operands lie (checked): pick x1, x2, w, then
// y1 = ((x2^3 - x1^3) / w - w) / 2 and y2 = y1 + w share a b — special inputs without a square root in Fq2.
//   hipcc -x c++ -std=c++17 -O2 -mbmi2 -madx -pthread -I aleo_amd/csrc tests/cpp/g2p28_bounds_emul.cpp      (tests/test_g2p28_bounds.py builds and runs it;
//   -DG2P28_HEADER='"path"' points it at a patched copy of g2p28.h: the negative controls)
#include "checked_f28.h"       // the bounds-carrying F28, the books, the lanes; includes fp28.h

#ifndef G2P28_HEADER
#define G2P28_HEADER "g2p28.h"
#endif
#include G2P28_HEADER

using aleo_mi355x::host::HFq2;

// ---- the reference: the affine group law on y^2 = x^3 + b over HFq2 (b never enters) ------------------------------------------------------------------
static bool eq2(const HFq2& x, const HFq2& y) { return x.a == y.a && x.b == y.b; }
static HFq2 neg2(const HFq2& x) { HFq2 r; r.a = HFq::neg(x.a); r.b = HFq::neg(x.b); return r; }
static HFq2 cube2(const HFq2& x) { return HFq2::mul(HFq2::sqr(x), x); }
static HFq2 small2(uint64_t v) { HFq2 r; r.a = HFq::from_u64(v); r.b = HFq::zero(); return r; }
struct Aff2 { bool inf; HFq2 x, y; };
static Aff2 aff2(const HFq2& x, const HFq2& y) { Aff2 r; r.inf = false; r.x = x; r.y = y; return r; }
static Aff2 aff2_inf() { Aff2 r; r.inf = true; r.x = HFq2::zero(); r.y = HFq2::zero(); return r; }
static Aff2 aff2_neg(const Aff2& p) { Aff2 r = p; r.y = neg2(p.y); return r; }
static Aff2 aff2_add(const Aff2& p, const Aff2& q) {
  if (p.inf) return q;
  if (q.inf) return p;
  HFq2 lam;
  if (eq2(p.x, q.x)) {
    if (!eq2(p.y, q.y) || p.y.is_zero()) return aff2_inf();                     // opposite points; a 2-torsion point twice
    const HFq2 xx = HFq2::sqr(p.x); lam = HFq2::mul(HFq2::add(HFq2::dbl(xx), xx), HFq2::inv(HFq2::dbl(p.y)));
  } else lam = HFq2::mul(HFq2::sub(q.y, p.y), HFq2::inv(HFq2::sub(q.x, p.x)));
  Aff2 r; r.inf = false;
  r.x = HFq2::sub(HFq2::sub(HFq2::sqr(lam), p.x), q.x);
  r.y = HFq2::sub(HFq2::mul(lam, HFq2::sub(p.x, r.x)), p.y);
  return r;
}
static HFq2 curve_b(const Aff2& p) { return HFq2::sub(HFq2::sqr(p.y), cube2(p.x)); }
static bool same_curve(const Aff2& p, const Aff2& q) { return p.inf || q.inf || eq2(curve_b(p), curve_b(q)); }
static HFq2 rnd_fq2() { HFq2 r; r.a = rnd_fq(); r.b = rnd_fq(); return r; }
static HFq2 base_field(const HFq& v) { HFq2 r; r.a = v; r.b = HFq::zero(); return r; }
// two points with the given x on one curve, their y apart by w (x1 != x2, w != 0)
static void pair_on_a_curve(const HFq2& x1, const HFq2& x2, const HFq2& w, Aff2& p1, Aff2& p2) {
  const HFq2 d = HFq2::sub(cube2(x2), cube2(x1));
  const HFq2 y1 = HFq2::mul(HFq2::sub(HFq2::mul(d, HFq2::inv(w)), w), HFq2::inv(small2(2)));
  p1 = aff2(x1, y1); p2 = aff2(x2, HFq2::add(y1, w));
  if (!same_curve(p1, p2)) { std::fprintf(stderr, "pair_on_a_curve: the two points do not share a curve\n"); std::exit(2); }
}

// ---- representatives: 448-byte points X.a | X.b | Y.a | Y.b | ZZ.a | ZZ.b | ZZZ.a | ZZZ.b; 224-byte entries x.a | y.a | x.b | y.b -----------------------
struct Rep2 { uint32_t k[8]; };                                    // the lift of each component, in the stored order
static const Rep2 REPS2[5] = {{{0, 0, 0, 0, 0, 0, 0, 0}}, {{11, 11, 5, 5, 1, 1, 1, 1}}, {{11, 0, 0, 5, 1, 0, 0, 1}}, {{0, 11, 5, 0, 0, 1, 1, 0}}, {{7, 3, 2, 4, 0, 0, 1, 1}}};
static void make_row2(uint32_t* row, const Aff2& p, const HFq2& z, const Rep2& r) {
  if (p.inf) { std::memset(row, 0, 448); return; }
  const HFq2 zz = HFq2::sqr(z), zzz = HFq2::mul(zz, z), X = HFq2::mul(p.x, zz), Y = HFq2::mul(p.y, zzz);
  const HFq* c[8] = {&X.a, &X.b, &Y.a, &Y.b, &zz.a, &zz.b, &zzz.a, &zzz.b};
  for (int i = 0; i < 8; ++i) big_digits(mont28_value(*c[i], r.k[i]), row + 14 * i);
}
static bool point_is2(const uint32_t* row, const Aff2& want, const char** why) {
  bool zero = true; for (int i = 0; i < 112; ++i) zero = zero && !row[i];
  uint32_t zz_raw = 0; for (int i = 56; i < 84; ++i) zz_raw |= row[i];
  if (want.inf) { *why = "expected the identity (all zero)"; return zero; }
  if (zz_raw == 0) { *why = "the identity where a finite point is expected"; return false; }
  const HFq2 X = HFq2::from28(row), Y = HFq2::from28(row + 28), ZZ = HFq2::from28(row + 56), ZZZ = HFq2::from28(row + 84);
  if (ZZ.is_zero()) { *why = "ZZ is zero for a finite point"; return false; }
  if (!eq2(cube2(ZZ), HFq2::sqr(ZZZ))) { *why = "ZZ^3 != ZZZ^2"; return false; }
  if (!eq2(HFq2::mul(X, HFq2::inv(ZZ)), want.x)) { *why = "x differs"; return false; }
  if (!eq2(HFq2::mul(Y, HFq2::inv(ZZZ)), want.y)) { *why = "y differs"; return false; }
  return true;
}

// ---- running the pair: two host threads, lane 0 the a-component, lane 1 the b-component -----------------------------------------------------------------------
static unsigned long g_n_add_any, g_n_double_any, g_n_add, g_n_double, g_n_madd;
static unsigned long g_b_madd_refused, g_b_identity_left, g_b_identity_right, g_b_same_doubled, g_b_opposite, g_b_same_two_torsion, g_b_double_identity, g_b_double_two_torsion,
    g_b_zz3_one_component_zero, g_b_add_zz3_one_component_zero, g_b_negated_zero_entry, g_alias_cases;
template <class F> static void on_pair(const char* formula, F body) {
  Group g; g.lanes = 2; std::thread th[2];
  for (int l = 0; l < 2; ++l) th[l] = std::thread([&, l] { t_grp = &g; t_lane = (uint32_t)l; t_formula = formula; body(l); });
  for (int l = 0; l < 2; ++l) th[l].join();
}
// commits the held stores: every byte of `out` written exactly once
static void commit(char* out, const char* what, int id) {
  uint8_t seen[448] = {}; bool twice = false;
  for (const Pending& s : g_pending) {
    const ptrdiff_t o = s.p - out; if (o < 0 || o + s.bytes > 448) { mismatch(what, "a store lands outside `out`", id); continue; }
    for (int i = 0; i < s.bytes; ++i) { twice = twice || seen[o + i]; seen[o + i] = 1; }
    std::memcpy(s.p, s.w, s.bytes);
  }
  size_t written = 0; for (int i = 0; i < 448; ++i) written += seen[i];
  if (twice || written != 448) mismatch(what, "the lanes do not write `out` exactly once", id);
}
static char* slot(int i) { return (char*)g_arena[2 * i]; }        // 448-byte points at an even row of the arena
// what a formula hands back (not yet stored) against the stored invariant, and into the formula's own slack line
static void closure(const XYZZ2P& r, const char* fn) {
  static const uint64_t vb[4] = {12 * UNIT, 6 * UNIT, 2 * UNIT, 2 * UNIT};
  static const char* const what[4] = {"X is not exact digits below 12q", "Y is not exact digits below 6q", "ZZ is not exact digits below 2q", "ZZZ is not exact digits below 2q"};
  const F28* f[4] = {&r.X, &r.Y, &r.ZZ, &r.ZZZ};
  for (int i = 0; i < 4; ++i) {
    rule(f[i]->exact && f[i]->vb <= vb[i], CLOSURE, what[i], 0, fn);
    std::lock_guard<std::mutex> lk(g_mu); Slack& s = g_slack[fn]; const double v = (double)f[i]->vb / (double)UNIT; if (v > s.stored[i]) s.stored[i] = v;
  }
}
// the direct formulas on loaded operands (tags: the stored invariant), for their own slack lines and their return values
static void run_add_direct(const Aff2& A, const Aff2& B, int id) {
  bool ok[2], same[2] = {false, false};
  on_pair("g2p_add", [&](int l) { const XYZZ2P a = g2p_load(slot(0), l), b = g2p_load(slot(1), l); XYZZ2P r; ok[l] = g2p_add(a, b, l, r, &same[l]); if (ok[l]) closure(r, "g2p_add"); });
  ++g_n_add;
  const bool same_x = eq2(A.x, B.x), same_pt = same_x && eq2(A.y, B.y);
  if (ok[0] != ok[1] || ok[0] == same_x) mismatch("g2p_add", "the refusal is not 'same x' in both lanes", id);
  if (!ok[0] && (same[0] != same[1] || same[0] != same_pt)) mismatch("g2p_add", "*same is not 'same point' in both lanes", id);
}
static void run_double_direct(const Aff2& A, int id) {
  bool inf[2];
  on_pair("g2p_double", [&](int l) { const XYZZ2P a = g2p_load(slot(0), l); inf[l] = false; const XYZZ2P r = g2p_double(a, l, &inf[l]); if (!inf[l]) closure(r, "g2p_double"); });
  ++g_n_double;
  if (inf[0] != inf[1] || inf[0] != A.y.is_zero()) mismatch("g2p_double", "*is_inf is not 'y == 0' in both lanes", id);
}
static void run_add_any(const uint32_t* rowA, const uint32_t* rowB, int alias, const Aff2& A, const Aff2& B, int id) {
  std::memcpy(slot(0), rowA, 448); std::memcpy(slot(1), rowB, 448); std::memset(slot(2), 0xff, 448);
  char* out = alias == 1 ? slot(0) : alias == 2 ? slot(1) : slot(2);
  g_pending.clear();
  on_pair("g2p_add_any", [&](int) { g2p_add_any(slot(0), slot(1), out); });
  commit(out, "g2p_add_any", id);
  const char* why = ""; if (!point_is2((const uint32_t*)out, aff2_add(A, B), &why)) mismatch("g2p_add_any", why, id);
  ++g_n_add_any; g_alias_cases += alias != 0;
  { const HFq2 zz3 = HFq2::from28((const uint32_t*)out + 56); if (!alias && !A.inf && !B.inf && zz3.b.is_zero() && !zz3.a.is_zero()) ++g_b_add_zz3_one_component_zero; }
  if (alias) return;                                             // the branches and the direct runs once per case
  if (A.inf) ++g_b_identity_left; else if (B.inf) ++g_b_identity_right;
  else {
    if (eq2(A.x, B.x)) { if (!eq2(A.y, B.y)) ++g_b_opposite; else if (A.y.is_zero()) ++g_b_same_two_torsion; else ++g_b_same_doubled; }
    g_pending.clear(); run_add_direct(A, B, id); run_double_direct(A, id); g_pending.clear();
  }
}
static void run_double_any(const uint32_t* rowA, bool alias, const Aff2& A, int id) {
  std::memcpy(slot(0), rowA, 448); std::memset(slot(2), 0xff, 448);
  char* out = alias ? slot(0) : slot(2);
  g_pending.clear();
  on_pair("g2p_double_any", [&](int) { g2p_double_any(slot(0), out); });
  commit(out, "g2p_double_any", id);
  const char* why = ""; if (!point_is2((const uint32_t*)out, aff2_add(A, A), &why)) mismatch("g2p_double_any", why, id);
  ++g_n_double_any; g_alias_cases += alias;
  if (!alias) { if (A.inf) ++g_b_double_identity; else if (A.y.is_zero()) ++g_b_double_two_torsion; }
}
static int g_case = 0;
static void add_case(const Aff2& A, const HFq2& za, const Rep2& ra, const Aff2& B, const HFq2& zb, const Rep2& rb) {
  if (!same_curve(A, B)) { std::fprintf(stderr, "case %d: the operands do not share a curve\n", g_case + 1); std::exit(2); }
  uint32_t rowA[112], rowB[112]; make_row2(rowA, A, za, ra); make_row2(rowB, B, zb, rb);
  ++g_case;
  for (int alias = 0; alias < 3; ++alias) run_add_any(rowA, rowB, alias, A, B, g_case);
  for (int alias = 0; alias < 2; ++alias) run_double_any(rowA, alias, A, g_case);
}

// ---- the mixed addition of the accumulation loop ----------------------------------------------------------------------------------------------------------------
struct Acc2 { XYZZ2P lane[2]; };
static Acc2 acc_of_row(const uint32_t* row) {                      // tagged with the invariant alone
  Acc2 a;
  for (int l = 0; l < 2; ++l) {
    a.lane[l].X = exact_below(row + 14 * l, 12 * UNIT); a.lane[l].Y = exact_below(row + 28 + 14 * l, 6 * UNIT);
    a.lane[l].ZZ = exact_below(row + 56 + 14 * l, 2 * UNIT); a.lane[l].ZZZ = exact_below(row + 84 + 14 * l, 2 * UNIT);
  }
  return a;
}
static void row_of_acc(uint32_t* row, const Acc2& a) {
  for (int l = 0; l < 2; ++l) { std::memcpy(row + 14 * l, a.lane[l].X.v, 56); std::memcpy(row + 28 + 14 * l, a.lane[l].Y.v, 56); std::memcpy(row + 56 + 14 * l, a.lane[l].ZZ.v, 56); std::memcpy(row + 84 + 14 * l, a.lane[l].ZZZ.v, 56); }
}
// acc (representing A) += the entry of E, taken with a minus sign when `neg` (then it is -E that is added: the device negates the canonical row itself);
// kx, ky: the lifts of the entry's components (a, b) when it is taken as it is — a tagged-below-2q entry may be any representative
static bool run_madd(Acc2& acc, const Aff2& A, const Aff2& E, bool neg, const uint32_t kx[2], const uint32_t ky[2], int id) {
  const Aff2 P = neg ? aff2_neg(E) : E;
  if (!same_curve(A, P)) { std::fprintf(stderr, "madd case %d: the operands do not share a curve\n", id); std::exit(2); }
  const HFq *xc[2] = {&E.x.a, &E.x.b}, *yc[2] = {&E.y.a, &E.y.b};
  const Acc2 before = acc; bool ok[2];
  on_pair("g2p_madd_fast", [&](int l) {
    const F28 x2 = tagged(*xc[l], neg ? 0 : kx[l], 2 * UNIT);
    const F28 y2 = neg ? g2p_negate_entry(tagged(*yc[l], 0, UNIT)) : tagged(*yc[l], ky[l], 2 * UNIT);      // rows are canonical where the device negates them
    ok[l] = g2p_madd_fast(acc.lane[l], x2, y2, l);
  });
  ++g_n_madd;
  if (neg && E.y.is_zero()) ++g_b_negated_zero_entry;
  uint32_t r0[112], r1[112]; row_of_acc(r0, before); row_of_acc(r1, acc);
  const bool same_x = eq2(A.x, P.x);
  if (ok[0] != ok[1]) { mismatch("g2p_madd_fast", "the two lanes disagree about the refusal", id); return false; }
  if (ok[0] == same_x) mismatch("g2p_madd_fast", ok[0] ? "accepted P == +-acc" : "refused a point that is not +-acc", id);
  if (!ok[0]) { ++g_b_madd_refused; if (std::memcmp(r0, r1, 448)) mismatch("g2p_madd_fast", "acc changed by a refused addition", id); return false; }
  const char* why = ""; if (!point_is2(r1, aff2_add(A, P), &why)) mismatch("g2p_madd_fast", why, id);
  { const HFq2 zz3 = HFq2::from28(r1 + 56); if (zz3.b.is_zero() && !zz3.a.is_zero()) ++g_b_zz3_one_component_zero; }
  for (int l = 0; l < 2; ++l) closure(acc.lane[l], "g2p_madd_fast");
  return true;
}
static Acc2 make_acc(const Aff2& A, const HFq2& z, const Rep2& r) { uint32_t row[112]; make_row2(row, A, z, r); return acc_of_row(row); }
// the first point of a slice as k_g2_accum28 builds it: (x, +-y, (1, 0), (1, 0)) from the canonical row, with the invariant's tags
static Acc2 first_point(const Aff2& E, bool neg) {
  Acc2 a; const HFq *xc[2] = {&E.x.a, &E.x.b}, *yc[2] = {&E.y.a, &E.y.b};
  for (int l = 0; l < 2; ++l) {
    a.lane[l].X = tagged(*xc[l], 0, UNIT); a.lane[l].Y = tagged(*yc[l], 0, UNIT); if (neg) a.lane[l].Y = g2p_negate_entry(a.lane[l].Y);
    a.lane[l].ZZ = l ? f28_const(Limbs14{}) : f28_const(ONE28); a.lane[l].ZZZ = a.lane[l].ZZ;
  }
  return a;
}

int main() {
  t_grp = nullptr; t_lane = 0; g_formula_header = "g2p28.h"; g_components = 2; g_stored_y_exact = true;
  const HFq2 one = HFq2::one();
  const HFq2 zs[3] = {one, base_field(rnd_fq()), rnd_fq2()};                      // Z = 1, in the base field, general
  const Aff2 O = aff2_inf();
  // four points on one curve (two by construction, then sums), and two whose x lie in the base field (their Z will too)
  std::vector<Aff2> P(4), B(2);
  pair_on_a_curve(rnd_fq2(), rnd_fq2(), rnd_fq2(), P[0], P[1]); P[2] = aff2_add(P[0], P[1]); P[3] = aff2_add(P[2], P[0]);
  pair_on_a_curve(base_field(rnd_fq()), base_field(rnd_fq()), rnd_fq2(), B[0], B[1]);
  for (int i = 1; i < 4; ++i) if (!same_curve(P[0], P[i])) { std::fprintf(stderr, "a test point left its curve\n"); return 2; }
  // y = (0, 0): the 2-torsion point T = (t, 0) of y^2 = x^3 - t^3, and a second point of that curve: with t = (s^3 - 1) m^2, (s t, (s^3 - 1)^2 m^3) lies on it
  const HFq2 ts = rnd_fq2(), tm = rnd_fq2(), s31 = HFq2::sub(cube2(ts), one), tx = HFq2::mul(s31, HFq2::sqr(tm));
  const Aff2 T = aff2(tx, HFq2::zero()), Tp = aff2(HFq2::mul(ts, tx), HFq2::mul(HFq2::sqr(s31), cube2(tm)));
  if (!same_curve(T, Tp)) { std::fprintf(stderr, "the 2-torsion point and its companion do not share a curve\n"); return 2; }
  Aff2 W, Wp; pair_on_a_curve(HFq2::zero(), rnd_fq2(), rnd_fq2(), W, Wp);         // x = (0, 0), and a second point of its curve
  HFq2 yb; yb.a = HFq::zero(); yb.b = rnd_fq(); const Aff2 Ya = aff2(rnd_fq2(), yb);      // y.a = 0
  HFq2 ya; ya.a = rnd_fq(); ya.b = HFq::zero(); const Aff2 Yb = aff2(base_field(rnd_fq()), ya);      // x.b = 0 and y.b = 0

  // ---- g2p_add_any / g2p_double_any (and g2p_add, g2p_double directly): out apart, out == pa, out == pb
  for (int a = 0; a < 5; ++a) for (int b = 0; b < 5; ++b) {
    const Rep2 &ra = REPS2[a], &rb = REPS2[b]; const HFq2 &za = zs[(a + b) % 3], &zb = zs[(a + 2 * b + 1) % 3];
    add_case(P[a % 4], za, ra, P[(a + 1 + b % 3) % 4], zb, rb);                 // distinct points
    add_case(P[a % 4], za, ra, P[a % 4], zb, rb);                               // the same point: other representatives, other Z -> doubling
    add_case(P[b % 4], za, ra, aff2_neg(P[b % 4]), zb, rb);                     // opposite points -> the identity
    add_case(B[a & 1], zs[1], ra, B[(a + 1) & 1], zs[b & 1], rb);       // x and Z in the base field: ZZ3 = (z, 0)
    add_case(B[a & 1], zs[1], ra, B[a & 1], zs[b & 1], rb);                     // the same there: ZZ3 = (0, 0) must still be seen
    add_case(T, za, ra, T, zb, rb);                                             // the 2-torsion point twice, and doubled
    add_case(T, za, ra, Tp, zb, rb); add_case(Tp, za, ra, T, zb, rb);
    add_case(W, za, ra, W, zb, rb); add_case(W, za, ra, aff2_neg(W), zb, rb);   // x = (0, 0) doubled and cancelled
    add_case(W, za, ra, Wp, zb, rb); add_case(Wp, za, ra, aff2_neg(W), zb, rb);
    add_case(Ya, za, ra, Ya, zb, rb); add_case(Ya, za, ra, aff2_neg(Ya), zb, rb);      // y.a = 0
    add_case(Yb, za, ra, Yb, zb, rb); add_case(Yb, za, ra, aff2_neg(Yb), zb, rb);      // x.b = y.b = 0
  }
  for (int a = 0; a < 5; ++a) {
    add_case(O, one, REPS2[0], P[a % 4], zs[a % 3], REPS2[a]); add_case(P[a % 4], zs[a % 3], REPS2[a], O, one, REPS2[0]);
    add_case(O, one, REPS2[0], T, zs[a % 3], REPS2[a]); add_case(W, zs[a % 3], REPS2[a], O, one, REPS2[0]);
  }
  add_case(O, one, REPS2[0], O, one, REPS2[0]);
  const int add_cases = g_case;

  // ---- g2p_madd_fast
  int id = 0;
  static const uint32_t LIFT[4][2] = {{0, 0}, {1, 1}, {1, 0}, {0, 1}};
  for (int a = 0; a < 5; ++a) for (int e = 0; e < 4; ++e) for (int neg = 0; neg < 2; ++neg) {
    const Rep2& r = REPS2[a]; const HFq2& z = zs[(a + e) % 3]; const uint32_t *kx = LIFT[e], *ky = LIFT[(e + 1) % 4];
    const Aff2& A = P[a % 4]; const Aff2& Q = P[(a + 1) % 4]; const Aff2& A1 = B[a & 1]; const Aff2& Q1 = B[(a + 1) & 1];
    { Acc2 acc = make_acc(A, z, r); run_madd(acc, A, Q, neg, kx, ky, ++id); }                                   // distinct
    { Acc2 acc = make_acc(A, z, r); run_madd(acc, A, A, neg, kx, ky, ++id); }                                   // P == +-acc: refused
    { Acc2 acc = make_acc(A, z, r); run_madd(acc, A, aff2_neg(A), neg, kx, ky, ++id); }
    { Acc2 acc = make_acc(A1, zs[1], r); run_madd(acc, A1, Q1, neg, kx, ky, ++id); }                            // base-field x and Z: ZZ3 = (z, 0), accepted
    { Acc2 acc = make_acc(A1, zs[1], r); run_madd(acc, A1, A1, neg, kx, ky, ++id); }                            // and refused when it is (0, 0)
    { Acc2 acc = first_point(A1, neg); run_madd(acc, neg ? aff2_neg(A1) : A1, Q1, neg, kx, ky, ++id); }         // the slice's first point, Z = (1, 0)
    { Acc2 acc = first_point(A, neg); run_madd(acc, neg ? aff2_neg(A) : A, Q, !neg, kx, ky, ++id); }
    { Acc2 acc = first_point(A, neg); run_madd(acc, neg ? aff2_neg(A) : A, A, neg, kx, ky, ++id); }             // the same base twice: refused at once
    { Acc2 acc = first_point(T, neg); run_madd(acc, T, T, !neg, kx, ky, ++id); }                                // y = 0 and its negation, exactly 2q: refused
    { Acc2 acc = make_acc(T, z, r); run_madd(acc, T, T, neg, kx, ky, ++id); }
    { Acc2 acc = make_acc(W, z, r); run_madd(acc, W, Wp, neg, kx, ky, ++id); }                                  // acc.X = (0, 0) or lifts of it
    { Acc2 acc = make_acc(Wp, z, r); run_madd(acc, Wp, W, neg, kx, ky, ++id); }                                 // the entry's x = (0, 0)
    { Acc2 acc = make_acc(W, z, r); run_madd(acc, W, W, neg, kx, ky, ++id); }
    { Acc2 acc = make_acc(Ya, z, r); run_madd(acc, Ya, Ya, neg, kx, ky, ++id); }
    { Acc2 acc = make_acc(Tp, z, r); run_madd(acc, Tp, T, neg, kx, ky, ++id); }                                 // the entry's y = 0; negated it is exactly 2q, and accepted
    { Acc2 acc = make_acc(T, z, r); run_madd(acc, T, Tp, neg, kx, ky, ++id); }                                  // acc.Y = (0, 0) or lifts of it
    // a chain: what an addition leaves is the next one's acc, re-tagged with the invariant alone
    Acc2 acc = first_point(A, neg); Aff2 sum = neg ? aff2_neg(A) : A;
    for (int s = 1; s <= 6; ++s) {
      const Aff2& Qs = P[(a + s) % 4]; const bool ng = (s + neg) & 1;
      if (!run_madd(acc, sum, Qs, ng, kx, ky, ++id)) break;
      sum = aff2_add(sum, ng ? aff2_neg(Qs) : Qs);
      uint32_t row[112]; row_of_acc(row, acc); acc = acc_of_row(row);
    }
  }

  unsigned long viol = 0; for (int k = 0; k < NKINDS; ++k) viol += g_viol[k];
  for (const char* fn : {"g2p_madd_fast", "g2p_double", "g2p_add", "g2p_add_any", "g2p_double_any", "g2p_negate_entry"}) {
    const Slack& s = g_slack[fn];
    std::printf("slack %s: largest column %.4f of 2^64 (line %d); smallest subtrahend-limb margin %.0f units (line %d), top limb %.2f q (line %d); largest limb %.4f of 2^32 (line %d); "
                "largest value into normalise %.6f of 2^392 (line %d); largest kept/stored X %.4f q, Y %.4f q, ZZ %.4f q, ZZZ %.4f q\n",
                fn, s.col, s.col_line, s.margin, s.margin_line, s.top_margin, s.top_margin_line, s.wrap, s.wrap_line, s.norm, s.norm_line, s.stored[0], s.stored[1], s.stored[2], s.stored[3]);
  }
  std::printf("calls: madd %lu, add %lu, double %lu, add_any %lu, double_any %lu (%d add cases; %lu runs with out aliasing an operand)\n", g_n_madd, g_n_add, g_n_double, g_n_add_any, g_n_double_any, add_cases, g_alias_cases);
  std::printf("branches: madd_refused %lu, madd_zz3_one_component_zero %lu, negated_zero_entry %lu, add_zz3_one_component_zero %lu, identity_left %lu, identity_right %lu, same_doubled %lu, opposite_to_identity %lu, "
              "same_two_torsion %lu, double_identity %lu, double_two_torsion %lu\n",
              g_b_madd_refused, g_b_zz3_one_component_zero, g_b_negated_zero_entry, g_b_add_zz3_one_component_zero, g_b_identity_left, g_b_identity_right, g_b_same_doubled, g_b_opposite, g_b_same_two_torsion,
              g_b_double_identity, g_b_double_two_torsion);
  std::printf("violations: limb %lu, column %lu, value %lu, closure %lu, sound %lu\n", g_viol[LIMB], g_viol[COLUMN], g_viol[VALUE], g_viol[CLOSURE], g_viol[SOUND]);
  std::printf("g2p28_bounds_emul: %lu additions, %lu doublings, %lu mixed additions, %lu mismatches, %lu limb-rule violations\n", g_n_add_any, g_n_double_any, g_n_madd, g_mismatches, viol);
  return g_mismatches || viol ? 1 : 0;
}
