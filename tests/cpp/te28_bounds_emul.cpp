// The Edwards-form formulas of aleo_amd/csrc/te28.h (te28_madd in its two halves, te28_first, te28_row_negate_if, te28_add_pair, te28_add_quad) run on the HOST over values
// and bounds together, against the affine group law on y^2 = x^3 + 1 in host_field.hpp's HFq carried through the map of tools/te28_model.py.
//
// The harness is checked_f28.h, which fp28_bounds_emul.cpp uses too: limbs that carry a bound each, a value bound in multiples of q and an
// exact-digits flag; primitives that compute what the device computes, propagate the bounds from the operation alone and check their preconditions
// against the BOUNDS (limb, column, value rules), lanes as host threads in lockstep at every exchange, stores held back until every lane has returned.
// What this file adds: load_te28 / store_te28 with the stored invariant of an Edwards point (every coordinate exact digits < 2q; a store that breaks
// it is a closure violation), the map, and the cases.  One run speaks for every input inside the stated invariants; the results are compared with the
// group law besides: distinct points, P = acc, P = -acc, the identity on either side, negated rows, Z = 1 and Z != 1, values lifted by q, chains, and a
// pair of points that differ by a 2-torsion point at infinity of the Edwards model, for which every form must report Z3 == 0.
//   hipcc -x c++ -std=c++17 -O2 -mbmi2 -madx -pthread -I aleo_amd/csrc tests/cpp/te28_bounds_emul.cpp      (tests/test_te28_bounds.py builds and runs it,
//   also with -fsanitize=address,undefined; -DTE28_HEADER='"path"' points it at a patched copy of te28.h: the negative controls)
#include "checked_f28.h"       // the bounds-carrying F28, the books, the lanes; includes fp28.h
#include "g1_affine_ref.h"     // the reference

#ifndef TE28_HEADER
#define TE28_HEADER "te28.h"
#endif

namespace aleo_mi355x {
inline F28 load_te28(const void* p, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  field_of(p, line, fn); uint32_t w[14]; std::memcpy(w, p, 56);
  F28 r = exact_below(w, 2 * UNIT); sound(r, line, fn); return r;
}
inline void store_te28(void* p, const F28& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  const int f = field_of(p, line, fn);
  rule(a.exact && a.vb <= 2 * UNIT, CLOSURE, "a stored Edwards coordinate is not exact digits below 2q", line, fn);
  { std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[fn]; const double v = (double)a.vb / (double)UNIT; if (v > s.stored[f]) s.stored[f] = v; }
  hold((char*)p, a.v, 56);
}
}  // namespace aleo_mi355x

#define ALEO_TE28_PROVIDED
#include TE28_HEADER

// ---- the map (tools/te28_model.py) over HFq, with the constants of te28_consts.h -------------------------------------------------------------------
static HFq hfq_of32(const uint32_t (&w)[12]) { HFq r; for (int i = 0; i < 6; ++i) r.l[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32); return r; }
struct Ed { HFq x, y; };                                           // affine; the identity is (0, 1)
static bool to_edwards(const Aff& p, Ed& e) {
  if (p.inf) { e.x = HFq::zero(); e.y = HFq::one(); return true; }
  const HFq s = hfq_of32(TE_S_32), f = hfq_of32(TE_F_32);
  const HFq u = HFq::mul(s, HFq::add(p.x, HFq::one())), v = HFq::mul(s, p.y), up1 = HFq::add(u, HFq::one());
  if (v.is_zero() || up1.is_zero()) return false;
  e.x = HFq::mul(HFq::mul(f, u), HFq::inv(v)); e.y = HFq::mul(HFq::sub(u, HFq::one()), HFq::inv(up1));
  return true;
}
static bool ed_on_curve(const Ed& e) {
  const HFq xx = HFq::sqr(e.x), yy = HFq::sqr(e.y);
  return HFq::sub(yy, xx) == HFq::add(HFq::one(), HFq::mul(hfq_of32(TE_D_32), HFq::mul(xx, yy)));
}
static Aff aff_mul(const Aff& p, const uint64_t* k, int nl) {
  Aff r = aff_inf();
  for (int i = 64 * nl - 1; i >= 0; --i) { r = aff_add(r, r); if ((k[i >> 6] >> (i & 63)) & 1) r = aff_add(r, p); }
  return r;
}
static Aff rnd_g1_point() { static const uint64_t h[2] = {0x0000000000000000ull, 0x170B5D4430000000ull}; return aff_mul(rnd_point(), h, 2); }      // cofactor cleared

// ---- representatives and checks ----------------------------------------------------------------------------------------------------------------
static unsigned long g_te_madds, g_te_firsts, g_te_adds[2], g_te_z3_zero, g_te_identity_results, g_te_alias;
static void te_row(uint32_t* row, const Ed& e, const HFq& z, const uint32_t k[4]) {       // (x z : y z : z : x y z), coordinate i lifted by k[i] q
  big_digits(mont28_value(HFq::mul(e.x, z), k[0]), row); big_digits(mont28_value(HFq::mul(e.y, z), k[1]), row + 14);
  big_digits(mont28_value(z, k[2]), row + 28); big_digits(mont28_value(HFq::mul(HFq::mul(e.x, e.y), z), k[3]), row + 42);
}
static TE28 te_acc(const uint32_t* row) { TE28 a; a.X = exact_below(row, 2 * UNIT); a.Y = exact_below(row + 14, 2 * UNIT); a.Z = exact_below(row + 28, 2 * UNIT); a.T = exact_below(row + 42, 2 * UNIT); return a; }
static void acc_to_row(uint32_t* row, const TE28& a) { std::memcpy(row, a.X.v, 56); std::memcpy(row + 14, a.Y.v, 56); std::memcpy(row + 28, a.Z.v, 56); std::memcpy(row + 42, a.T.v, 56); }
static bool te_point_is(const uint32_t* row, const Aff& want, const char** why) {
  const HFq X = aleo_mi355x::host::hfq_from28(row), Y = aleo_mi355x::host::hfq_from28(row + 14), Z = aleo_mi355x::host::hfq_from28(row + 28), T = aleo_mi355x::host::hfq_from28(row + 42);
  Ed e; if (!to_edwards(want, e)) { *why = "the expected point has no Edwards image"; return false; }
  if (Z.is_zero()) { *why = "Z is zero"; return false; }
  if (!(HFq::mul(T, Z) == HFq::mul(X, Y))) { *why = "T Z != X Y"; return false; }
  const HFq zi = HFq::inv(Z);
  if (!(HFq::mul(X, zi) == e.x)) { *why = "x differs"; return false; }
  if (!(HFq::mul(Y, zi) == e.y)) { *why = "y differs"; return false; }
  if (want.inf) ++g_te_identity_results;
  return true;
}
static void make_entry(F28& r0, F28& r1, F28& r2, const Aff& P) {  // the table row of P: canonical exact digits
  Ed e; if (!to_edwards(P, e)) { std::fprintf(stderr, "a table point has no Edwards image\n"); std::exit(2); }
  const HFq k = hfq_of32(TE_K_32);
  r0 = tagged(HFq::sub(e.y, e.x), 0, UNIT); r1 = tagged(HFq::add(e.y, e.x), 0, UNIT); r2 = tagged(HFq::mul(k, HFq::mul(e.x, e.y)), 0, UNIT);
}
static void closure(const TE28& a, const char* fn) {
  const F28* f[4] = {&a.X, &a.Y, &a.Z, &a.T}; static const char* const what[4] = {"acc.X", "acc.Y", "acc.Z", "acc.T"};
  for (int i = 0; i < 4; ++i) {
    rule(f[i]->exact && f[i]->vb <= 2 * UNIT, CLOSURE, what[i], 0, fn);
    std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[fn]; const double v = (double)f[i]->vb / (double)UNIT; if (v > s.stored[i]) s.stored[i] = v;
  }
}
// acc (tagged with the invariant alone) + (neg ? -P : P) through the row of P; expect_zero: the operands differ by a point of even order
static void run_te_madd(TE28& acc, const Aff& A, const Aff& P, bool neg, bool expect_zero, int id) {
  F28 r0, r1, r2; make_entry(r0, r1, r2, P);
  te28_row_negate_if(neg, r0, r1, r2);
  const bool z = te28_madd(acc, r0, r1, r2);
  ++g_te_madds; g_te_z3_zero += z;
  if (z != expect_zero) { mismatch("te28_madd", z ? "reported Z3 == 0 for a regular pair" : "did not report Z3 == 0", id); return; }
  if (z) return;
  uint32_t row[56]; acc_to_row(row, acc);
  const char* why = ""; if (!te_point_is(row, aff_add(A, neg ? aff_neg(P) : P), &why)) mismatch("te28_madd", why, id);
  closure(acc, "te28_madd_finish");
}
static void run_te_first(TE28& acc, const Aff& P, bool neg, int id) {
  F28 r0, r1, r2; make_entry(r0, r1, r2, P);
  te28_row_negate_if(neg, r0, r1, r2);
  te28_first(acc, r0, r1, r2); ++g_te_firsts;
  uint32_t row[56]; acc_to_row(row, acc);
  const char* why = ""; if (!te_point_is(row, neg ? aff_neg(P) : P, &why)) mismatch("te28_first", why, id);
  closure(acc, "te28_first");
}
static void retag(TE28& a) { uint32_t row[56]; acc_to_row(row, a); a = te_acc(row); }
static void run_te_add(int lanes, const uint32_t* rowA, const uint32_t* rowB, bool alias, const Aff& A, const Aff& B, bool expect_zero, int id) {
  std::memcpy(g_arena[0], rowA, 224); std::memcpy(g_arena[1], rowB, 224); std::memset(g_arena[2], 0xff, 224);
  const char* pa = (const char*)g_arena[0]; const char* pb = (const char*)g_arena[1]; char* out = alias ? (char*)g_arena[0] : (char*)g_arena[2];
  Group g; g.lanes = lanes; g_pending.clear(); int flag[4] = {0, 0, 0, 0};
  std::thread th[4];
  for (int l = 0; l < lanes; ++l) th[l] = std::thread([&, l] { t_grp = &g; t_lane = (uint32_t)l; flag[l] = lanes == 4 ? te28_add_quad(pa, pb, out) : te28_add_pair(pa, pb, out); });
  for (int l = 0; l < lanes; ++l) th[l].join();
  const char* what = lanes == 4 ? "te28_add_quad" : "te28_add_pair";
  uint8_t seen[224] = {}; bool twice = false;
  for (const Pending& s : g_pending) {
    const ptrdiff_t o = s.p - out; if (o < 0 || o + s.bytes > 224) { mismatch(what, "a store lands outside `out`", id); continue; }
    for (int i = 0; i < s.bytes; ++i) { twice = twice || seen[o + i]; seen[o + i] = 1; }
    std::memcpy(s.p, s.w, s.bytes);
  }
  size_t written = 0; for (int i = 0; i < 224; ++i) written += seen[i];
  if (twice || written != 224) mismatch(what, "the lanes do not write `out` exactly once", id);
  int z = 0; for (int l = 0; l < lanes; ++l) z += flag[l];
  ++g_te_adds[lanes == 4]; g_te_alias += alias; g_te_z3_zero += z != 0;
  if (z > 1 || (z != 0) != expect_zero) { mismatch(what, z ? "reported Z3 == 0 for a regular pair (or in two lanes)" : "did not report Z3 == 0", id); return; }
  if (z) return;
  const char* why = ""; if (!te_point_is((const uint32_t*)out, aff_add(A, B), &why)) mismatch(what, why, id);
}
static int g_te_case = 0;
static void te_add_case(const Aff& A, const HFq& za, const uint32_t ka[4], const Aff& B, const HFq& zb, const uint32_t kb[4], bool expect_zero = false) {
  Ed ea, eb; if (!to_edwards(A, ea) || !to_edwards(B, eb)) { std::fprintf(stderr, "an operand has no Edwards image\n"); std::exit(2); }
  uint32_t rowA[56], rowB[56]; te_row(rowA, ea, za, ka); te_row(rowB, eb, zb, kb);
  ++g_te_case;
  for (int lanes = 2; lanes <= 4; lanes += 2) for (int alias = 0; alias < 2; ++alias) run_te_add(lanes, rowA, rowB, alias, A, B, expect_zero, g_te_case);
}

int main() {
  t_grp = nullptr; t_lane = 0; g_formula_header = "te28.h";
  const HFq one = HFq::one();
  std::vector<Aff> P; for (int i = 0; i < 4; ++i) P.push_back(rnd_g1_point());
  const Aff O = aff_inf();
  // (-w, 0) with w a primitive cube root of unity: a 2-torsion point that the map sends to infinity (adding (-1, 0), whose image is (0, -1), is regular)
  HFq rm3; if (!fq_sqrt(rm3, HFq::neg(HFq::from_u64(3)))) return 2;
  Aff T2; T2.inf = false; T2.x = HFq::neg(HFq::mul(HFq::sub(rm3, one), HFq::inv(HFq::from_u64(2)))); T2.y = HFq::zero();
  if (!on_curve(T2) || T2.x == HFq::neg(one)) return 2;
  for (const Aff& p : P) { Ed e; if (p.inf || !on_curve(p) || !to_edwards(p, e) || !ed_on_curve(e)) { std::fprintf(stderr, "a test point is not on the curves\n"); return 2; } }
  const HFq zs[3] = {one, rnd_fq(), rnd_fq()};
  static const uint32_t LIFT[4][4] = {{0, 0, 0, 0}, {1, 1, 1, 1}, {1, 0, 1, 0}, {0, 1, 0, 1}};

  // ---- pair and quad: every case in both forms, with `out` apart and with `out` aliasing `pa`
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) {
    const HFq &za = zs[(a + b) % 3], &zb = zs[(a + 2 * b + 1) % 3];
    te_add_case(P[a], za, LIFT[a], P[(a + 1 + b % 3) % 4], zb, LIFT[b]);          // distinct points
    te_add_case(P[a], za, LIFT[a], P[a], zb, LIFT[b]);                            // the same point, other representatives: no doubling branch
    te_add_case(P[b], za, LIFT[a], aff_neg(P[b]), zb, LIFT[b]);                   // opposite points: the identity, an ordinary result
    te_add_case(O, za, LIFT[a], P[b], zb, LIFT[b]); te_add_case(P[a], za, LIFT[a], O, zb, LIFT[b]);      // the identity (0 : z : z : 0) on either side
    te_add_case(P[a], one, LIFT[a], P[(a + 1) % 4], one, LIFT[b]);                // Z = 1 on both sides
    te_add_case(P[a], za, LIFT[a], aff_add(P[a], T2), zb, LIFT[b], true);         // operands that differ by that 2-torsion point: Z3 == 0 must be reported
  }
  te_add_case(O, zs[1], LIFT[1], O, zs[2], LIFT[0]);
  const int add_cases = g_te_case;

  // ---- the mixed addition and the first point of a slice
  int id = 0;
  for (int a = 0; a < 4; ++a) for (int lift = 0; lift < 4; ++lift) for (int neg = 0; neg < 2; ++neg) {
    const Aff& A = P[a]; const Aff& B = P[(a + 1) % 4]; const HFq& z = zs[(a + lift) % 3];
    Ed ea; to_edwards(A, ea); uint32_t row[56]; te_row(row, ea, z, LIFT[lift]);
    Ed eo; to_edwards(O, eo); uint32_t rowO[56]; te_row(rowO, eo, z, LIFT[lift]);
    { TE28 acc = te_acc(row); run_te_madd(acc, A, B, neg, false, ++id); }                      // distinct
    { TE28 acc = te_acc(row); run_te_madd(acc, A, A, neg, false, ++id); }                      // P == acc (doubling) / P == -acc (identity) by the sign
    { TE28 acc = te_acc(row); run_te_madd(acc, A, aff_neg(A), neg, false, ++id); }
    { TE28 acc = te_acc(row); run_te_madd(acc, A, O, neg, false, ++id); }                      // an identity base: the row (1, 1, 0)
    { TE28 acc = te_acc(rowO); run_te_madd(acc, O, B, neg, false, ++id); }                     // acc the identity
    if (!neg) { TE28 acc = te_acc(row); run_te_madd(acc, A, aff_add(A, T2), false, true, ++id); }      // A + (A + T2): the operands differ by that 2-torsion point, Z3 == 0 must be reported
    // a chain from the first point: what an addition leaves is the next one's acc, re-tagged with the invariant alone
    TE28 acc; run_te_first(acc, A, neg, ++id); Aff sum = neg ? aff_neg(A) : A;
    for (int s = 1; s <= 6; ++s) {
      retag(acc);
      const Aff& Q = s == 4 ? sum : P[(a + s) % 4]; const bool ng = s == 5 ? true : ((s + neg) & 1);      // step 4 doubles the running sum
      run_te_madd(acc, sum, Q, ng, false, ++id);
      sum = aff_add(sum, ng ? aff_neg(Q) : Q);
    }
    { TE28 f; run_te_first(f, O, neg, ++id); }                                                 // a slice that starts with an identity base
  }

  unsigned long viol = 0; for (int k = 0; k < NKINDS; ++k) viol += g_viol[k];
  for (const char* fn : {"te28_madd_rows", "te28_madd_finish", "te28_first", "te28_row_negate_if", "te28_add_pair", "te28_add_quad"}) {
    const Slack& s = g_slack[fn];
    std::printf("slack %s: largest column %.4f of 2^64 (line %d); smallest subtrahend-limb margin %.0f units (line %d), top limb %.2f q (line %d); largest limb %.4f of 2^32 (line %d); "
                "largest value into normalise %.6f of 2^392 (line %d); largest kept/stored X %.4f q, Y %.4f q, Z %.4f q, T %.4f q\n",
                fn, s.col, s.col_line, s.margin, s.margin_line, s.top_margin, s.top_margin_line, s.wrap, s.wrap_line, s.norm, s.norm_line, s.stored[0], s.stored[1], s.stored[2], s.stored[3]);
  }
  std::printf("calls: madd %lu, first %lu, pair %lu, quad %lu (%d add cases; %lu additions with out == pa)\n", g_te_madds, g_te_firsts, g_te_adds[0], g_te_adds[1], add_cases, g_te_alias);
  std::printf("branches: z3_zero %lu, identity_results %lu\n", g_te_z3_zero, g_te_identity_results);
  std::printf("violations: limb %lu, column %lu, value %lu, closure %lu, sound %lu\n", g_viol[LIMB], g_viol[COLUMN], g_viol[VALUE], g_viol[CLOSURE], g_viol[SOUND]);
  std::printf("te28_bounds_emul: %lu additions, %lu mixed additions, %lu mismatches, %lu limb-rule violations\n", g_te_adds[0] + g_te_adds[1], g_te_madds, g_mismatches, viol);
  return g_mismatches || viol ? 1 : 0;
}
