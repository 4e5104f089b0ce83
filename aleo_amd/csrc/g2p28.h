// g2p28.h — the G2 point formulas on 28-bit limbs, one LANE PAIR per point operation: what g2.hip's accumulation, slice trees and chunk sums run.
//
// An Fq2 value (Fq[u] / (u^2 + 5)) lives across the two lanes of a pair: the even lane holds the a-component, the odd lane the b-component, each as 14 x 28-bit limbs in the
// R' = 2^392 Montgomery form of fp28.h.  Sums, differences and normalisations are component-wise, so they are the F28 operations unchanged; a product
//   (x.a + x.b u)(y.a + y.b u) = (x.a y.a - 5 x.b y.b) + (x.a y.b + x.b y.a) u
// is ONE merged block per lane (mont28_muladd: two products under one reduction, 588 mads) after the lanes have swapped copies of their operands:
//   even lane:  x.a * y.a + x.b * (K q - 5 y.b)          odd lane:  x.b * y.a + x.a * y.b
// i.e. three product times of work per Fq2 product — what a one-lane Karatsuba costs — at half the registers per lane (an XYZZ accumulator over Fq2 is
// 112 limbs; one lane per slice with the ten products in line does not fit 256 VGPRs, and the out-of-line 32-bit version this replaces moved every
// operand through scratch memory).  Every operand of a product is normalised first (exact digits, class L1): a column then holds at most
// 14 (1 * 1 + 1 * 7) + 14 < 256 (fp28.h); value bounds are written at each step, with a < A q, b < B q -> a b < (A B / 38000 + 1) q.
// The mixed addition is fp28.h's xyzz28_madd_fast (EFD madd-2008-s) with F28 read as "my component"; P == +-acc (ZZ3 = 0 in BOTH components) leaves the
// loop for the general 32-bit code on the even lane, as in msm.hip.
//
// Like the formulas of fp28.h, everything here uses only the names of fp28.h's guarded block (ALEO_F28_PROVIDED): tests/cpp/g2p28_bounds_emul.cpp supplies
// those names on the host over limbs that carry their bounds, includes this file, and checks every "< k q", "limbs < k * 2^28" and column claim below
// mechanically for all inputs inside the stated invariants (tests/test_g2p28_bounds.py); selftest_g2p.hip runs the same source on rows the host built.
#pragma once
#include "fp28.h"

namespace aleo_mi355x {

template <uint32_t K> __device__ __forceinline__ F28 f28_neg5(const F28& v) {      // K q - 5 v for an exact-digit v with 5 v < K q: limbs < 7 * 2^28
  return f28_sub<K, 6>(f28_const(Limbs14{}), f28_times5(v));
}
// my component of x * y; x, y: exact digits; KY: 5 * (value bound of y in q) rounded up to a K with a spread constant
template <uint32_t KY> __device__ __forceinline__ F28 fq2p_mul(const F28& x, const F28& y, bool odd) {
  const F28 ox = f28_qperm<1, 0, 3, 2>(x), oy = f28_qperm<1, 0, 3, 2>(y);      // the partner lane's copies: DPP quad_perm moves (full-rate VALU; __shfl_xor compiled to ds_bpermute: an LDS-crossbar round trip per limb)
  const F28 b1 = f28_sel(odd, y, oy);                      // even: x.a * y.a        odd: x.b * y.a
  const F28 b2 = f28_sel(odd, f28_neg5<KY>(oy), y);        // even: x.b * (-5 y.b)   odd: x.a * y.b
  return f28_muladd(x, b1, ox, b2);
}
__device__ __forceinline__ bool pair_and(bool v) { return f28_pair_and(v); }      // true iff v holds in both lanes of the pair
__device__ __forceinline__ bool g2p_zero_mod(const F28& v_lt2q_exact) { return pair_and(f28_is_zero_mod_lt2q(v_lt2q_exact)); }      // an Fq2 value is 0 iff both components are
struct XYZZ2P { F28 X, Y, ZZ, ZZZ; };                      // my components of an XYZZ point over Fq2
// the entry of a base taken with a minus sign: 2q - y for a canonical row y, exact digits, <= 2q (= 2q exactly for y = 0)
__device__ __forceinline__ F28 g2p_negate_entry(const F28& y) { return f28_normalise(f28_sub<2, 1>(f28_const(Limbs14{}), y)); }
// acc += (x2, y2).  In: acc.X exact < 12q, acc.Y exact < 6q, acc.ZZ / ZZZ exact < 2q; x2, y2 exact <= 2q.  Out: the same.  false (acc untouched): P == +-acc.
__device__ __forceinline__ bool g2p_madd_fast(XYZZ2P& acc, const F28& x2, const F28& y2, bool odd) {
  const F28 U2 = fq2p_mul<16>(x2, acc.ZZ, odd);                                    // (2*2 + 2*16) / 38000 + 1 -> < 2q
  const F28 S2 = fq2p_mul<16>(y2, acc.ZZZ, odd);                                   // < 2q
  const F28 P = f28_normalise(f28_sub<16, 1>(U2, acc.X));                          // U2 + 16q - X1 < 18q
  const F28 R = f28_normalise(f28_sub<8, 1>(S2, acc.Y));                           // S2 + 8q - Y1 < 10q
  const F28 PP = fq2p_mul<96>(P, P, odd);                                          // (18*18 + 18*96) / 38000 + 1 -> < 2q
  const F28 ZZ3 = fq2p_mul<16>(acc.ZZ, PP, odd);                                   // < 2q
  {
    if (__builtin_expect(g2p_zero_mod(ZZ3), 0)) return false;
  }
  const F28 PPP = fq2p_mul<16>(P, PP, odd);                                        // (18*2 + 18*16) / 38000 + 1 -> < 2q
  const F28 Q = fq2p_mul<16>(acc.X, PP, odd);                                      // (12*2 + 12*16) / 38000 + 1 -> < 2q
  const F28 RR = fq2p_mul<64>(R, R, odd);                                          // (10*10 + 10*64) / 38000 + 1 -> < 2q
  const F28 t0 = f28_sub<4, 1>(RR, PPP);                                           // < 6q, limbs < 3 * 2^28
  const F28 X3 = f28_normalise(f28_sub<6, 2>(t0, f28_add(Q, Q)));                  // 2Q: limbs < 2 * 2^28, < 4q; X3 < 12q, exact digits
  const F28 t1 = f28_normalise(f28_sub<16, 1>(Q, X3));                             // Q + 16q - X3 < 18q
  const F28 RT = fq2p_mul<96>(R, t1, odd);                                         // (10*18 + 10*96) / 38000 + 1 -> < 2q
  const F28 YP = fq2p_mul<16>(acc.Y, PPP, odd);                                    // (6*2 + 6*16) / 38000 + 1 -> < 2q
  acc.Y = f28_normalise(f28_sub<4, 1>(RT, YP));                                    // RT + 4q - YP < 6q
  acc.X = X3;
  acc.ZZ = ZZ3;
  acc.ZZZ = fq2p_mul<16>(acc.ZZZ, PPP, odd);                                       // < 2q
  return true;
}
// ---- stored points of the pair form: 448 bytes = X.a | X.b | Y.a | Y.b | ZZ.a | ZZ.b | ZZZ.a | ZZZ.b, 14 x 28-bit limbs each --------------------------------
// Stored invariant (what g2p_madd_fast keeps for its accumulator): X exact digits < 12q, Y exact < 6q, ZZ / ZZZ exact < 2q; the identity = all zero.
// Everything below is pair-cooperative: both lanes of a pair call with the same pointers, each moves and computes its own component.
static constexpr uint32_t P2B = 448, ROW2 = 224;      // a stored point; a base's 28-bit row
__device__ __forceinline__ XYZZ2P g2p_load(const char* p, bool odd) {
  const char* c = p + (odd ? 56 : 0); XYZZ2P r; r.X = load_f28(c); r.Y = load_f28(c + 112); r.ZZ = load_f28(c + 224); r.ZZZ = load_f28(c + 336); return r;
}
__device__ __forceinline__ void g2p_store(char* p, bool odd, const XYZZ2P& a) {
  char* c = p + (odd ? 56 : 0); store_f28(c, a.X); store_f28(c + 112, a.Y); store_f28(c + 224, a.ZZ); store_f28(c + 336, a.ZZZ);
}
__device__ __forceinline__ void g2p_store_inf(char* p, bool odd) { XYZZ2P z; z.X = f28_const(Limbs14{}); z.Y = z.X; z.ZZ = z.X; z.ZZZ = z.X; g2p_store(p, odd, z); }
__device__ __forceinline__ bool g2p_is_inf(const XYZZ2P& a) { return pair_and(f28_is_zero_raw(a.ZZ)); }
// 2a (EFD dbl-2008-s-1, a = 0); a not the identity
__device__ __forceinline__ XYZZ2P g2p_double(const XYZZ2P& a, bool odd, bool* is_inf) {
  const F28 U = f28_normalise(f28_add(a.Y, a.Y));                                  // < 12q
  const F28 V = fq2p_mul<64>(U, U, odd);                                           // (12*12 + 12*64) / 38000 + 1 -> < 2q
  const F28 W = fq2p_mul<16>(U, V, odd);                                           // < 2q
  const F28 S = fq2p_mul<16>(a.X, V, odd);                                         // X < 12q -> < 2q
  const F28 XX = fq2p_mul<64>(a.X, a.X, odd);                                      // < 2q
  const F28 M = f28_normalise(f28_add(f28_add(XX, XX), XX));                       // < 6q
  const F28 MM = fq2p_mul<32>(M, M, odd);                                          // < 2q
  XYZZ2P r;
  r.X = f28_normalise(f28_sub<6, 2>(MM, f28_add(S, S)));                           // MM + 6q - 2S < 8q
  const F28 t1 = f28_normalise(f28_sub<8, 1>(S, r.X));                             // S + 8q - X3 < 10q
  const F28 MT = fq2p_mul<64>(M, t1, odd);                                         // (6*10 + 6*64) / 38000 + 1 -> < 2q
  const F28 WY = fq2p_mul<32>(W, a.Y, odd);                                        // (2*6 + 2*32) / 38000 + 1 -> < 2q
  r.Y = f28_normalise(f28_sub<4, 1>(MT, WY));                                      // < 6q
  r.ZZ = fq2p_mul<16>(V, a.ZZ, odd);
  r.ZZZ = fq2p_mul<16>(W, a.ZZZ, odd);
  *is_inf = g2p_zero_mod(r.ZZ);                                                    // y = 0: a 2-torsion point
  return r;
}
// a + b (EFD add-2008-s), neither the identity.  false: a == +-b (then *same tells which) and r is not written.
__device__ __forceinline__ bool g2p_add(const XYZZ2P& a, const XYZZ2P& b, bool odd, XYZZ2P& r, bool* same) {
  const F28 U1 = fq2p_mul<16>(a.X, b.ZZ, odd), U2 = fq2p_mul<16>(b.X, a.ZZ, odd);  // X < 12q: (12*2 + 12*16) / 38000 + 1 -> < 2q
  const F28 S1 = fq2p_mul<16>(a.Y, b.ZZZ, odd), S2 = fq2p_mul<16>(b.Y, a.ZZZ, odd);
  const F28 P = f28_normalise(f28_sub<4, 1>(U2, U1)), R = f28_normalise(f28_sub<4, 1>(S2, S1));      // < 6q each
  const F28 PP = fq2p_mul<32>(P, P, odd);                                          // (6*6 + 6*32) / 38000 + 1 -> < 2q
  const F28 ZZ12 = fq2p_mul<16>(a.ZZ, b.ZZ, odd);
  const F28 ZZ3 = fq2p_mul<16>(ZZ12, PP, odd);
  if (__builtin_expect(g2p_zero_mod(ZZ3), 0)) {                                    // P = 0 (the ZZ's are units): equal or opposite points
    *same = g2p_zero_mod(f28_mul(R, f28_const(ONE28)));                            // R brought below 2q (exact digits) first
    return false;
  }
  const F28 PPP = fq2p_mul<16>(P, PP, odd);
  const F28 Q = fq2p_mul<16>(U1, PP, odd);
  const F28 RR = fq2p_mul<32>(R, R, odd);
  const F28 t0 = f28_sub<4, 1>(RR, PPP);                                           // < 6q, limbs < 3 * 2^28
  r.X = f28_normalise(f28_sub<6, 2>(t0, f28_add(Q, Q)));                           // < 12q
  const F28 t1 = f28_normalise(f28_sub<16, 1>(Q, r.X));                            // < 18q
  const F28 RT = fq2p_mul<96>(R, t1, odd);                                         // (6*18 + 6*96) / 38000 + 1 -> < 2q
  const F28 SP = fq2p_mul<16>(S1, PPP, odd);
  r.Y = f28_normalise(f28_sub<4, 1>(RT, SP));                                      // < 6q
  r.ZZ = ZZ3;
  r.ZZZ = fq2p_mul<16>(fq2p_mul<16>(a.ZZZ, b.ZZZ, odd), PPP, odd);
  return true;
}
// out = pa + pb for stored points (any of them may be the identity, they may be equal or opposite; out may alias pa or pb).  Out of line: the reduction
// kernels are chains of these calls, and one copy of the ~20 product blocks per kernel is enough.
__device__ __noinline__ void g2p_add_any(const char* pa, const char* pb, char* out) {
  const bool odd = f28_lane() & 1;
  const XYZZ2P a = g2p_load(pa, odd), b = g2p_load(pb, odd);
  if (g2p_is_inf(a)) { g2p_store(out, odd, b); return; }
  if (g2p_is_inf(b)) { g2p_store(out, odd, a); return; }
  XYZZ2P r; bool same = false;
  if (!g2p_add(a, b, odd, r, &same)) {
    bool inf = true;
    if (same) r = g2p_double(a, odd, &inf);
    if (inf) { g2p_store_inf(out, odd); return; }
  }
  g2p_store(out, odd, r);
}
__device__ __noinline__ void g2p_double_any(const char* pa, char* out) {
  const bool odd = f28_lane() & 1;
  const XYZZ2P a = g2p_load(pa, odd);
  if (g2p_is_inf(a)) { g2p_store(out, odd, a); return; }
  bool inf = false; const XYZZ2P r = g2p_double(a, odd, &inf);
  if (inf) g2p_store_inf(out, odd); else g2p_store(out, odd, r);
}

}  // namespace aleo_mi355x
