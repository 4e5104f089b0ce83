// te28.h — G1 in twisted Edwards form, -x^2 + y^2 = 1 + d x^2 y^2, extended coordinates (X : Y : Z : T) on 14 x 28-bit limbs.
//
// Why: the mixed addition of the bucket accumulation costs 6 products, 2 squarings and a double product in XYZZ (fp28.h xyzz28_madd_fast: 3542 mads);
// against a precomputed affine row (y - x | y + x | 2 d x y) the Edwards form takes SEVEN products (EFD madd-2008-hwcd-3, Z2 = 1: 2744 mads), and the
// general addition 8 products and one by the constant k = 2d against fourteen.  The formulas are unified: P = acc, P = -acc and the identity go through
// the same code — there is no infinity flag, no doubling branch and no refusal; the identity is the ordinary stored point (0 : Z : Z : 0).
// The model, the map from y^2 = x^3 + 1 and every constant: tools/te28_model.py (checked against the oracle by tests/test_te28_model.py), which writes
// te28_consts.h.
//
// REQUIRES bases in the prime-order subgroup, which is all a snarkVM G1Affine can hold.  d is a square, so the law is not complete on E(Fq): two operands
// that differ by a point of even order give Z3 = 0 (mod q).  Every addition below tests its Z3 — the cost of the XYZZ form's ZZ3 test — and reports it;
// the caller must then discard the result and compute on another path.  Z3 != 0 means the result is right, for any curve points.
//
// Like fp28.h this header uses only the names of fp28.h's guarded block (f28_mul, f28_add, f28_sub<K, S>, f28_normalise, f28_sel, the lane exchanges) and
// load_te28 / store_te28 below, so tests/cpp/te28_bounds_emul.cpp can run it on the host over limbs that carry their bounds (tests/test_te28_bounds.py).
// Bounds notation as in fp28.h: "< k q" values, "class Lk" limbs < k 2^28, "exact" = base-2^28 digits; a product of La x Lb needs 14 a b + 14 < 256.
//
// Stored point, 224 bytes: X[14] | Y[14] | Z[14] | T[14], every coordinate exact digits < 2q (each is a product's result).
// Row of the mixed addition: r0 = y - x, r1 = y + x, r2 = 2 d x y, canonical exact digits; the identity's row is (1, 1, 0).
#pragma once
#include "fp28.h"
#include "te28_consts.h"

#ifndef ALEO_TE28_PROVIDED
namespace aleo_mi355x {
// a coordinate of a stored Edwards point (the stored invariant differs from XYZZ's, so the bounds harness supplies its own pair)
__device__ __forceinline__ F28 load_te28(const void* p) { return load_f28(p); }
__device__ __forceinline__ void store_te28(void* p, const F28& a) { store_f28(p, a); }
// Table rows: r0 | r1 | r2 at bytes 0, 64, 128 of a TE_ROW-byte row (every entry starts a 64-byte half line; 168 payload bytes never fit one 128-byte
// line, so a gathered row costs two lines at any stride — 192 keeps the table at 1.5x the XYZZ tier's bytes, 256 would make it 2x for the same two lines).
static constexpr size_t TE_ROW = 192;
__device__ __forceinline__ F28 load_te28_entry(const void* p) {      // 56 of the entry's 64 bytes
  F28 r; const uint4* s = (const uint4*)p;
#pragma unroll
  for (int i = 0; i < 3; ++i) { uint4 t = s[i]; r.v[4 * i] = t.x; r.v[4 * i + 1] = t.y; r.v[4 * i + 2] = t.z; r.v[4 * i + 3] = t.w; }
  const uint2 t = *(const uint2*)(s + 3); r.v[12] = t.x; r.v[13] = t.y;
  return r;
}
__device__ __forceinline__ void store_te28_row(void* p, const F28& r0, const F28& r1, const F28& r2) {
  store_f28(p, r0); store_f28((char*)p + 64, r1); store_f28((char*)p + 128, r2);
}
}  // namespace aleo_mi355x
#endif

namespace aleo_mi355x {

struct TE28 { F28 X, Y, Z, T; };

__device__ __forceinline__ F28 te28_const(const uint32_t (&k)[14]) {
  Limbs14 l{};
  for (int i = 0; i < 14; ++i) l.v[i] = k[i];
  return f28_const(l);
}

// -P's row from P's: (r1, r0, -r2).  2q - r2 is class L2 and <= 2q, which is all te28_madd and te28_first ask of r2.
__device__ __forceinline__ void te28_row_negate_if(bool neg, F28& r0, F28& r1, F28& r2) {
  const F28 a = f28_sel(neg, r0, r1), b = f28_sel(neg, r1, r0);       // canonical either way
  r2 = f28_sel(neg, r2, f28_sub<2, 1>(f28_const(Limbs14{}), r2));    // 2q - r2: limbs < 2^29, value <= 2q
  r0 = a; r1 = b;
}

// ---- the mixed addition of the accumulation loop (EFD madd-2008-hwcd-3 with Z2 = 1) --------------------------------------------------------
// Invariant of acc between additions, which is also the stored one: X, Y, Z, T exact digits < 2q.
// r0, r1: canonical exact digits; r2: canonical, or te28_row_negate_if's 2q - r2 (class L2, <= 2q).
// Returns true when Z3 == 0 (mod q): the operands differ by a point of even order, acc is then meaningless (see the head of this file).
// In two halves so that the accumulation loop can put the gather of the NEXT row between them: the first half is the last reader of r0, r1, r2 — each is
// consumed by exactly one product — and the four products of the second hide the latency, so a lane holds ONE row (42 registers), never two.
struct TE28Half { F28 A, B, C; };
__device__ __forceinline__ TE28Half te28_madd_rows(const TE28& acc, const F28& r0, const F28& r1, const F28& r2) {
  // operand order as in fp28.h: the product block works in place on its first argument
  TE28Half h;
  h.A = f28_mul(f28_sub<4, 1>(acc.Y, acc.X), r0);                  // Y1 + 4q - X1 < 6q, class L3; L3 x L1: 56; 6/38000 + 1 -> < 2q
  h.B = f28_mul(f28_add(acc.Y, acc.X), r1);                        // Y1 + X1 < 4q, class L2; < 2q
  h.C = f28_mul(acc.T, r2);                                        // L1 x L2: 42; 4/38000 + 1 -> < 2q
  return h;
}
__device__ __forceinline__ bool te28_madd_finish(TE28& acc, const TE28Half& h) {
  const F28 &A = h.A, &B = h.B, &C = h.C;                          // exact digits < 2q
  const F28 D = f28_add(acc.Z, acc.Z);                             // 2 Z1 < 4q, class L2
  const F28 E = f28_sub<4, 1>(B, A);                               // B + 4q - A < 6q, class L3
  const F28 F = f28_sub<4, 1>(D, C);                               // D + 4q - C < 8q, class L4
  const F28 G = f28_add(D, C);                                     // < 6q, class L3
  const F28 H = f28_add(B, A);                                     // < 4q, class L2
  acc.X = f28_mul(E, F);                                           // L3 x L4: 182 < 256; 48/38000 + 1 -> < 2q
  acc.Y = f28_mul(G, H);                                           // L3 x L2: 98; < 2q
  acc.T = f28_mul(E, H);                                           // L3 x L2: 98; < 2q
  acc.Z = f28_mul(F, G);                                           // L4 x L3: 182; 48/38000 + 1 -> < 2q
  return f28_is_zero_mod_lt2q(acc.Z);
}
__device__ __forceinline__ bool te28_madd(TE28& acc, const F28& r0, const F28& r1, const F28& r2) { return te28_madd_finish(acc, te28_madd_rows(acc, r0, r1, r2)); }
// The first point of a slice, identity + P, collapses: E = 2x, H = 2y, and up to the common factor (2x : 2y : 2 : 2xy) with 2xy = r2 / d.  Two products:
// T, and the one that brings r1 + 2q - r0 (< 3q, loose limbs) back under the invariant.
__device__ __forceinline__ void te28_first(TE28& acc, const F28& r0, const F28& r1, const F28& r2) {
  acc.X = f28_mul(f28_sub<2, 1>(r1, r0), te28_const(TE_ONE_28));    // L3 x L1: 56; < 2q
  acc.Y = f28_normalise(f28_add(r1, r0));                          // < 2q, exact digits
  acc.Z = te28_const(TE_TWO_28);                                   // canonical
  acc.T = f28_mul(te28_const(TE_D_INV_28), r2);                    // L1 x L2: 42; < 2q
}

// ---- the general addition (EFD add-2008-hwcd-3), shared by a lane pair: nine products in five levels ----------------------------------------
//   level 1   even: A = (Y1 - X1)(Y2 - X2)    odd: B = (Y1 + X1)(Y2 + X2)
//   level 2   even: T1 T2                     odd: Z1 Z2
//   level 3   even: C = k T1 T2               (odd repeats the product on its own operand: no divergence)
//   level 4   even: X3 = E F                  odd: Y3 = G H            E = B - A, F = D - C, G = D + C, H = B + A, D = 2 Z1 Z2
//   level 5   even: T3 = E H                  odd: Z3 = F G
// Operands and result are stored points (every coordinate exact < 2q); out may alias pa or pb (every load precedes the stores).
// Returns 1 in the odd lane when Z3 == 0 (mod q), 0 elsewhere.
__device__ __forceinline__ int te28_add_pair(const char* pa, const char* pb, char* out) {
  const bool odd = f28_lane() & 1;
  const F28 X1 = load_te28(pa), Y1 = load_te28(pa + 56), X2 = load_te28(pb), Y2 = load_te28(pb + 56);
  const F28 m1 = f28_sel(odd, f28_sub<4, 1>(Y1, X1), f28_add(Y1, X1));        // even: Y1 + 4q - X1 < 6q, class L3   odd: Y1 + X1 < 4q, class L2
  const F28 m2 = f28_sel(odd, f28_sub<4, 1>(Y2, X2), f28_add(Y2, X2));
  const F28 t1 = f28_mul(m1, m2);                                             // L3 x L3: 140 < 256; 36/38000 + 1 -> < 2q
  const F28 t2 = f28_mul(load_te28(pa + (odd ? 112 : 168)), load_te28(pb + (odd ? 112 : 168)));   // even: T1 T2   odd: Z1 Z2   (< 2q)
  const F28 t3 = f28_mul(t2, te28_const(TE_K_28));                            // even: C   (< 2q)
  const F28 pt1 = f28_xchg(t1), pt2 = f28_xchg(t2), pt3 = f28_xchg(t3);
  const F28 A = f28_sel(odd, t1, pt1), B = f28_sel(odd, pt1, t1), ZZ = f28_sel(odd, pt2, t2), C = f28_sel(odd, t3, pt3);
  const F28 D = f28_add(ZZ, ZZ);                                              // < 4q, class L2
  const F28 E = f28_sub<4, 1>(B, A), H = f28_add(B, A);                       // < 6q, class L3; < 4q, class L2
  const F28 F = f28_sub<4, 1>(D, C), G = f28_add(D, C);                       // < 8q, class L4; < 6q, class L3
  const F28 t4 = f28_mul(f28_sel(odd, E, G), f28_sel(odd, F, H));             // even: X3 = E F   odd: Y3 = G H   (L3 x L4: 182 < 256; 48/38000 + 1 -> < 2q)
  const F28 t5 = f28_mul(f28_sel(odd, E, F), f28_sel(odd, H, G));             // even: T3 = E H   odd: Z3 = F G   (L4 x L3: 182; < 2q)
  store_te28(out + (odd ? 56 : 0), t4);
  store_te28(out + (odd ? 112 : 168), t5);
  return (odd && f28_is_zero_mod_lt2q(t5)) ? 1 : 0;
}

// ---- the same addition on a lane QUAD: three levels, one product per lane per level ---------------------------------------------------------
//   level 1   q0: A = (Y1 - X1)(Y2 - X2)    q1: B = (Y1 + X1)(Y2 + X2)    q2: Z1 Z2      q3: T1 T2
//   level 2   C = k T1 T2 in every lane
//   level 3   q0: X3 = E F                  q1: Y3 = G H                  q2: Z3 = F G   q3: T3 = E H
// Lane q stores coordinate q.  Returns 1 in lane 2 of the quad when Z3 == 0 (mod q), 0 elsewhere.
__device__ __forceinline__ int te28_add_quad(const char* pa, const char* pb, char* out) {
  const uint32_t q = f28_lane() & 3u; const bool odd = q & 1u, hi = q & 2u;
  const uint32_t o1 = hi ? 56u * q : 56u, o2 = hi ? 56u * q : 0u;              // q0, q1: Y and X; q2: Z; q3: T (twice: one code path)
  const F28 u1 = load_te28(pa + o1), w1 = load_te28(pa + o2), u2 = load_te28(pb + o1), w2 = load_te28(pb + o2);
  const F28 m1 = f28_sel(hi, f28_sel(odd, f28_sub<4, 1>(u1, w1), f28_add(u1, w1)), u1);   // q0: < 6q, class L3; q1: < 4q, class L2; q2, q3: the coordinate
  const F28 m2 = f28_sel(hi, f28_sel(odd, f28_sub<4, 1>(u2, w2), f28_add(u2, w2)), u2);
  const F28 t1 = f28_mul(m1, m2);                                             // L3 x L3: 140 < 256; 36/38000 + 1 -> < 2q
  const F28 C = f28_mul(f28_qperm<3, 3, 3, 3>(t1), te28_const(TE_K_28));      // < 2q
  const F28 A = f28_qperm<0, 0, 0, 0>(t1), B = f28_qperm<1, 1, 1, 1>(t1), ZZ = f28_qperm<2, 2, 2, 2>(t1);
  const F28 D = f28_add(ZZ, ZZ);                                              // < 4q, class L2
  const F28 E = f28_sub<4, 1>(B, A), H = f28_add(B, A);                       // < 6q, class L3; < 4q, class L2 (every lane)
  const F28 F = f28_sub<4, 1>(D, C), G = f28_add(D, C);                       // < 8q, class L4; < 6q, class L3 (every lane)
  const F28 a3 = f28_sel(q == 1, f28_sel(q == 2, E, F), G);                   // q0: E   q1: G   q2: F   q3: E
  const F28 b3 = f28_sel(q == 0, f28_sel(q == 2, H, G), F);                   // q0: F   q1: H   q2: G   q3: H
  const F28 t3 = f28_mul(a3, b3);                                             // at most L4 x L4: 238 < 256; 64/38000 + 1 -> < 2q
  store_te28(out + 56u * q, t3);
  return (q == 2 && f28_is_zero_mod_lt2q(t3)) ? 1 : 0;
}

}  // namespace aleo_mi355x
