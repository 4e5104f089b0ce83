// The four point formulas of aleo_amd/csrc/fp28.h (xyzz28_madd_fast, xyzz28_double_both, xyzz28_add_pair, xyzz28_add_quad) run on the HOST, over
// values and bounds together, against the affine group law in host_field.hpp's HFq.
//
// fp28.h keeps everything that touches F28::v or a device builtin behind ALEO_F28_PROVIDED.  checked_f28.h defines the macro and supplies that part
// itself: an F28 that carries, next to its 14 concrete limbs, an upper bound per limb, an upper bound of the value as a multiple of q (32.32 fixed
// point, strict: value < vb q) and whether the digits are exact.  Every primitive computes the concrete result the way the device does (products
// column by column with R' = 2^392, differences with the spread constant of spread_kq), propagates the bounds from the operation alone — never
// from a comment — and checks its preconditions against the BOUNDS, so one run speaks for every input inside the stated invariants:
//   limb     no 32-bit limb wraps in add / sub / normalise / the doubled operand of a squaring; no limb 0..12 of a difference can go negative
//   column   every product column, carry-in included, stays below 2^64 (and what is left for the top limb below 2^32)
//   value    the subtrahend's top limb fits the constant's (b < K q as a value); normalise sees < 2^392; the == 0 (mod q) tests see exact digits
//            below 2q / 4q
//   closure  what a formula stores satisfies the stored invariant of that field (X exact < 12q; Y class L3 < 6q; ZZ, ZZZ exact < 2q), and what
//            xyzz28_madd_fast leaves in acc the accumulator's (Y exact < 2q): outputs are legal inputs again
//   sound    every concrete limb and value is within its tracked bound (the bookkeeping of this file itself)
// A broken rule prints itself with the fp28.h line (the primitives take __builtin_LINE() as a default argument) and is counted.  The lane pair /
// quad are 2 / 4 host threads with a barrier inside each exchange helper; stores are held back until all lanes have returned, which is what
// lockstep execution gives the device where `out` aliases `pa`.
//   hipcc -x c++ -std=c++17 -O2 -mbmi2 -madx -pthread -I aleo_amd/csrc tests/cpp/fp28_bounds_emul.cpp   (tests/test_fp28_bounds.py builds and runs it;
//   -DFP28_HEADER='"path"' points it at a patched copy of the header: the negative controls).
#include "checked_f28.h"       // the bounds-carrying F28, the books, the lanes; includes fp28.h
#include "g1_affine_ref.h"     // the reference

// ---- representatives --------------------------------------------------------------------------------------------------------------------------
static void relimb_up(uint32_t* v) {                             // same value, limbs raised towards 3 2^28 - 1: every limb lends two units to the one below
  for (int i = 12; i >= 0; --i) { const uint32_t k = v[i + 1] < 2 ? v[i + 1] : 2; v[i + 1] -= k; v[i] += k << 28; }
}
struct Rep { uint32_t kx, ky, kzz, kzzz; bool relimb_y; };
static const Rep REPS[4] = {{0, 0, 0, 0, false}, {11, 5, 1, 1, false}, {11, 5, 1, 1, true}, {0, 0, 1, 0, true}};
static void make_row(uint32_t* row, const Aff& p, const HFq& z, const Rep& r) {
  if (p.inf) { std::memset(row, 0, 224); return; }
  const HFq zz = HFq::sqr(z), zzz = HFq::mul(zz, z);
  big_digits(mont28_value(HFq::mul(p.x, zz), r.kx), row);
  big_digits(mont28_value(HFq::mul(p.y, zzz), r.ky), row + 14); if (r.relimb_y) relimb_up(row + 14);
  big_digits(mont28_value(zz, r.kzz), row + 28);
  big_digits(mont28_value(zzz, r.kzzz), row + 42);
}
// residues of a point in the 28-bit form; compares with an affine point after dividing by ZZ and ZZZ
static bool point_is(const uint32_t* row, const Aff& want, const char** why) {
  uint32_t z = 0; for (int i = 0; i < 14; ++i) z |= row[28 + i];
  const HFq X = aleo_mi355x::host::hfq_from28(row), Y = aleo_mi355x::host::hfq_from28(row + 14), ZZ = aleo_mi355x::host::hfq_from28(row + 28), ZZZ = aleo_mi355x::host::hfq_from28(row + 42);
  if (want.inf) { *why = "expected the identity (ZZ all zero)"; return z == 0; }
  if (z == 0 || ZZ.is_zero()) { *why = "ZZ is zero for a finite point"; return false; }
  if (!(HFq::mul(HFq::sqr(ZZ), ZZ) == HFq::sqr(ZZZ))) { *why = "ZZ^3 != ZZZ^2"; return false; }
  if (!(HFq::mul(X, HFq::inv(ZZ)) == want.x)) { *why = "x differs"; return false; }
  if (!(HFq::mul(Y, HFq::inv(ZZZ)) == want.y)) { *why = "y differs"; return false; }
  return true;
}

// ---- running the lane-group formulas --------------------------------------------------------------------------------------------------------------
static unsigned long g_adds[2], g_inf_cases, g_alias_cases;
static void run_add(int lanes, const uint32_t* rowA, const uint32_t* rowB, bool alias, const Aff& A, const Aff& B, int id) {
  std::memcpy(g_arena[0], rowA, 224); std::memcpy(g_arena[1], rowB, 224); std::memset(g_arena[2], 0xff, 224);
  const char* pa = (const char*)g_arena[0]; const char* pb = (const char*)g_arena[1]; char* out = alias ? (char*)g_arena[0] : (char*)g_arena[2];
  Group g; g.lanes = lanes; g_pending.clear();
  std::thread th[4];
  for (int l = 0; l < lanes; ++l) th[l] = std::thread([&, l] { t_grp = &g; t_lane = (uint32_t)l; if (lanes == 4) xyzz28_add_quad(pa, pb, out); else xyzz28_add_pair(pa, pb, out); });
  for (int l = 0; l < lanes; ++l) th[l].join();
  // commit: no byte written twice, and a result that is not one of the operands left in place written whole
  uint8_t seen[224] = {}; bool twice = false;
  for (const Pending& s : g_pending) {
    const ptrdiff_t o = s.p - out; if (o < 0 || o + s.bytes > 224) { mismatch("a store lands outside `out`", "", id); continue; }
    for (int i = 0; i < s.bytes; ++i) { twice = twice || seen[o + i]; seen[o + i] = 1; }
    std::memcpy(s.p, s.w, s.bytes);
  }
  size_t written = 0; for (int i = 0; i < 224; ++i) written += seen[i];
  const bool kept = alias && (B.inf);                            // A + O with out == pa: nothing to write
  if (twice || (written != 224 && !(kept && written == 0))) mismatch(lanes == 4 ? "quad" : "pair", "the lanes do not write `out` exactly once", id);
  const char* why = ""; if (!point_is((const uint32_t*)out, aff_add(A, B), &why)) mismatch(lanes == 4 ? "quad" : "pair", why, id);
  ++g_adds[lanes == 4]; g_inf_cases += A.inf || B.inf; g_alias_cases += alias;
}
static int g_case = 0;
static void add_case(const Aff& A, const HFq& za, const Rep& ra, const Aff& B, const HFq& zb, const Rep& rb) {
  uint32_t rowA[56], rowB[56]; make_row(rowA, A, za, ra); make_row(rowB, B, zb, rb);
  ++g_case;
  for (int lanes = 2; lanes <= 4; lanes += 2) for (int alias = 0; alias < 2; ++alias) run_add(lanes, rowA, rowB, alias, A, B, g_case);
}

// ---- the mixed addition --------------------------------------------------------------------------------------------------------------------------
static unsigned long g_madds, g_madd_refused;
static F28 l2_negation(const F28& y) { return f28_sub<2, 1>(f28_const(Limbs14{}), y); }      // as msm.hip builds it; y tagged canonical
static void acc_row(uint32_t* row, const XYZZ28& a) { std::memcpy(row, a.X.v, 56); std::memcpy(row + 14, a.Y.v, 56); std::memcpy(row + 28, a.ZZ.v, 56); std::memcpy(row + 42, a.ZZZ.v, 56); }
// acc: X exact < 12q, Y exact < 2q (or the L2 negation), ZZ / ZZZ exact < 2q — tagged with the invariant's bounds, whatever the concrete limbs are
static bool run_madd(XYZZ28& acc, const Aff& A, const Aff& P, bool neg_entry, int id) {
  F28 x2 = tagged(P.x, 0, UNIT), y2 = tagged(neg_entry ? HFq::neg(P.y) : P.y, 0, UNIT);
  if (neg_entry) y2 = l2_negation(y2);                            // the entry holds -P's y; the sign bit of the sorted index asks for 2q - y
  const XYZZ28 before = acc;
  const bool ok = xyzz28_madd_fast(acc, x2, y2);
  ++g_madds; g_madd_refused += !ok;
  const bool same_x = !A.inf && A.x == P.x;
  uint32_t r0[56], r1[56]; acc_row(r0, before); acc_row(r1, acc);
  if (ok == same_x) mismatch("madd", ok ? "accepted P == +-acc" : "refused a point that is not +-acc", id);
  if (!ok) { if (std::memcmp(r0, r1, 224)) mismatch("madd", "acc changed by a refused addition", id); return false; }
  const char* why = ""; if (!point_is(r1, aff_add(A, P), &why)) mismatch("madd", why, id);
  const char* fn = "xyzz28_madd_fast";
  rule(acc.X.exact && acc.X.vb <= 12 * UNIT, CLOSURE, "acc.X is not exact digits below 12q after the addition", 0, fn);
  rule(acc.Y.exact && acc.Y.vb <= 2 * UNIT, CLOSURE, "acc.Y is not exact digits below 2q after the addition", 0, fn);
  rule(acc.ZZ.exact && acc.ZZ.vb <= 2 * UNIT, CLOSURE, "acc.ZZ is not exact digits below 2q after the addition", 0, fn);
  rule(acc.ZZZ.exact && acc.ZZZ.vb <= 2 * UNIT, CLOSURE, "acc.ZZZ is not exact digits below 2q after the addition", 0, fn);
  {
    std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[fn]; const F28* f[4] = {&acc.X, &acc.Y, &acc.ZZ, &acc.ZZZ};
    for (int i = 0; i < 4; ++i) { const double v = (double)f[i]->vb / (double)UNIT; if (v > s.stored[i]) s.stored[i] = v; }
  }
  return true;
}
static XYZZ28 make_acc(const Aff& A, const HFq& z, uint32_t kx, uint32_t ky, uint32_t kz) {
  const HFq zz = HFq::sqr(z), zzz = HFq::mul(zz, z); XYZZ28 a;
  a.X = tagged(HFq::mul(A.x, zz), kx, 12 * UNIT); a.Y = tagged(HFq::mul(A.y, zzz), ky, 2 * UNIT);
  a.ZZ = tagged(zz, kz, 2 * UNIT); a.ZZZ = tagged(zzz, kz, 2 * UNIT); return a;
}
static XYZZ28 first_point(const Aff& A, bool neg) {               // acc = (x, +-y, 1, 1) as the accumulation kernel starts a slice: A = +-(entry)
  XYZZ28 a; const HFq ey = neg ? HFq::neg(A.y) : A.y;
  a.X = tagged(A.x, 0, UNIT); a.Y = tagged(ey, 0, UNIT); if (neg) a.Y = l2_negation(a.Y);
  Limbs14 one28; big_digits(mont28_value(HFq::one(), 0), one28.v);      // 2^392 mod q: fp28.h's ONE28
  a.ZZ = f28_const(one28); a.ZZZ = a.ZZ; return a;
}

int main() {
  t_grp = nullptr; t_lane = 0;
  const HFq one = HFq::one();
  std::vector<Aff> P; for (int i = 0; i < 4; ++i) P.push_back(rnd_point());
  const HFq z1 = rnd_fq(), z2 = rnd_fq();
  Aff T; T.inf = false; T.x = HFq::neg(one); T.y = HFq::zero();                // (-1, 0): 2-torsion
  Aff W; W.inf = false; W.x = HFq::zero(); W.y = one;                           // (0, 1): X has all limbs zero while ZZ does not
  const Aff O = aff_inf();
  for (const Aff& p : P) if (!on_curve(p)) { std::fprintf(stderr, "a test point is not on the curve\n"); return 2; }
  if (!on_curve(T) || !on_curve(W)) return 2;
  const HFq zs[3] = {one, z1, z2};

  // ---- pair and quad: every case in both forms, with `out` apart and with `out` aliasing `pa` (msm.hip's in-place folds)
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) {
    const Rep &ra = REPS[a], &rb = REPS[b]; const HFq &za = zs[(a + b) % 3], &zb = zs[(a + 2 * b + 1) % 3];
    add_case(P[a], za, ra, P[(a + 1 + b % 3) % 4], zb, rb);                   // distinct points
    add_case(P[a], za, ra, P[a], zb, rb);                                     // the same point: other representatives, other Z -> doubling
    add_case(P[b], za, ra, aff_neg(P[b]), zb, rb);                            // opposite points -> the identity
    add_case(T, za, ra, T, zb, rb);                                           // (-1, 0) + (-1, 0): the Y == 0 branch of the doubling
    add_case(T, za, ra, P[b], zb, rb); add_case(P[a], za, ra, T, zb, rb);
    add_case(W, za, ra, W, zb, rb); add_case(W, za, ra, aff_neg(W), zb, rb);  // (0, 1) doubled, (0, 1) + (0, -1)
    add_case(W, za, ra, P[b], zb, rb); add_case(P[a], za, ra, aff_neg(W), zb, rb);
    add_case(W, za, ra, T, zb, rb);                                           // (0, 1) + (-1, 0) = (2, -3)
    add_case(P[a], one, ra, P[(a + 1) % 4], one, rb);                         // Z = 1 on both sides
  }
  for (int a = 0; a < 4; ++a) {
    add_case(O, one, REPS[0], P[a], zs[a % 3], REPS[a]); add_case(P[a], zs[a % 3], REPS[a], O, one, REPS[0]);
    add_case(O, one, REPS[0], T, zs[a % 3], REPS[a]); add_case(W, zs[a % 3], REPS[a], O, one, REPS[0]);
  }
  add_case(O, one, REPS[0], O, one, REPS[0]);
  const int add_cases = g_case;

  // ---- the mixed addition of the accumulation loop
  int id = 0;
  for (int a = 0; a < 4; ++a) for (uint32_t lift = 0; lift < 2; ++lift) for (int neg = 0; neg < 2; ++neg) {
    const uint32_t kx = lift ? 11 : 0, ky = lift, kz = lift ^ (uint32_t)(a & 1); const HFq& z = zs[(a + lift) % 3];
    const Aff& A = P[a]; const Aff& B = P[(a + 1) % 4]; const Aff Bn = neg ? aff_neg(B) : B;
    { XYZZ28 acc = make_acc(A, z, kx, ky, kz); run_madd(acc, A, Bn, neg, ++id); }                       // distinct
    { XYZZ28 acc = make_acc(A, z, kx, ky, kz); run_madd(acc, A, A, neg, ++id); }                        // P == acc: refused
    { XYZZ28 acc = make_acc(A, z, kx, ky, kz); run_madd(acc, A, aff_neg(A), neg, ++id); }               // P == -acc: refused
    { XYZZ28 acc = first_point(A, neg); run_madd(acc, A, Bn, !neg, ++id); }                             // the first point (+-y, Z = 1), then another
    { XYZZ28 acc = first_point(A, neg); run_madd(acc, A, A, neg, ++id); }
    { XYZZ28 acc = first_point(A, neg); run_madd(acc, A, aff_neg(A), !neg, ++id); }
    { XYZZ28 acc = make_acc(T, z, kx, ky, kz); run_madd(acc, T, Bn, neg, ++id); }                       // acc = (-1, 0): Y is 0 or q
    { XYZZ28 acc = make_acc(T, z, kx, ky, kz); run_madd(acc, T, T, neg, ++id); }                        // (-1, 0) twice: refused
    { XYZZ28 acc = make_acc(W, z, kx, ky, kz); run_madd(acc, W, Bn, neg, ++id); }                       // acc = (0, 1): X is 0 or 11q
    { XYZZ28 acc = make_acc(W, z, kx, ky, kz); run_madd(acc, W, neg ? W : aff_neg(W), neg, ++id); }     // refused
    { XYZZ28 acc = make_acc(A, z, kx, ky, kz); run_madd(acc, A, W, neg, ++id); }                        // the entry is (0, 1): x2 all zero
    { XYZZ28 acc = first_point(W, neg); run_madd(acc, W, T, neg, ++id); }                               // y2 = 0 and its negation 2q
    // a chain: what an addition leaves is the next one's acc, re-tagged with the invariant alone
    XYZZ28 acc = first_point(A, neg); Aff sum = A;
    for (int s = 1; s <= 6; ++s) {
      const Aff& Q = P[(a + s) % 4]; const bool ng = (s + neg) & 1; const Aff Qs = ng ? aff_neg(Q) : Q;
      if (!run_madd(acc, sum, Qs, ng, ++id)) break;
      sum = aff_add(sum, Qs);
      acc.X = exact_below(acc.X.v, 12 * UNIT); acc.Y = exact_below(acc.Y.v, 2 * UNIT); acc.ZZ = exact_below(acc.ZZ.v, 2 * UNIT); acc.ZZZ = exact_below(acc.ZZZ.v, 2 * UNIT);
    }
  }

  unsigned long viol = 0; for (int k = 0; k < NKINDS; ++k) viol += g_viol[k];
  for (const char* fn : {"xyzz28_madd_fast", "xyzz28_double_both", "xyzz28_add_pair", "xyzz28_add_quad"}) {
    const Slack& s = g_slack[fn];
    std::printf("slack %s: largest column %.4f of 2^64 (line %d); smallest subtrahend-limb margin %.0f units (line %d), top limb %.2f q (line %d); largest limb %.4f of 2^32 (line %d); "
                "largest value into normalise %.6f of 2^392 (line %d); largest kept/stored X %.4f q, Y %.4f q (limbs %.4f x 2^28), ZZ %.4f q, ZZZ %.4f q\n",
                fn, s.col, s.col_line, s.margin, s.margin_line, s.top_margin, s.top_margin_line, s.wrap, s.wrap_line, s.norm, s.norm_line, s.stored[0], s.stored[1], s.stored_ylimb, s.stored[2], s.stored[3]);
  }
  std::printf("calls: madd %lu, double %lu, pair %lu, quad %lu (%d add cases; %lu additions with out == pa, %lu with an identity operand)\n", g_madds, g_calls_double, g_calls_pair, g_calls_quad, add_cases, g_alias_cases, g_inf_cases);
  std::printf("branches: madd_refused %lu, identity_copy_half %lu, identity_copy_quarter %lu, opposite_to_identity %lu, doubling %lu, two_torsion %lu, quad_to_pair %lu\n",
              g_madd_refused, g_copy_half, g_copy_quarter, g_identity, g_calls_double, g_two_torsion, g_quad_to_pair);
  std::printf("violations: limb %lu, column %lu, value %lu, closure %lu, sound %lu\n", g_viol[LIMB], g_viol[COLUMN], g_viol[VALUE], g_viol[CLOSURE], g_viol[SOUND]);
  std::printf("fp28_bounds_emul: %lu additions, %lu mixed additions, %lu mismatches, %lu limb-rule violations\n", g_adds[0] + g_adds[1], g_madds, g_mismatches, viol);
  return g_mismatches || viol ? 1 : 0;
}
