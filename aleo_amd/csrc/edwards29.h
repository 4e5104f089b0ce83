// edwards29.h — Edwards-BLS12 (-x^2 + y^2 = 1 + 3021 x^2 y^2 over Fr, cofactor 4) on the 29-bit-limb form of Fr (fr29.h), one point per lane:
// what the record scan (records.hip) needs of snarkVM's console group [UPSTREAM-RECALL: curves/src/edwards_bls12, TwistedEdwardsExtended].
//
// Extended coordinates (X : Y : Z : T), x = X / Z, y = Y / Z, T = X Y / Z, with the dedicated a = -1 formulas of Hisil, Wong, Carter and Dawson
// (add-2008-hwcd-3: 8 products with a cached second operand; dbl-2008-hwcd: 4 squarings + 3 products, + 1 when T is wanted).  -1 is a square in Fr
// and 3021 is not, so the addition is COMPLETE: it has no exceptional pair among the rational points, whatever their order — the scan multiplies
// points of order 4 l, 2 l and l alike and never branches on a point.
//
// Limb discipline (fr29.h): a product takes a lazy multiplicand (limbs < 2^31.4) and a normalised multiplier, and returns normalised limbs; a sum of
// two normalised values is a valid multiplicand; a padded difference a + 19 r - b wants b normalised and below 18 r.  Whatever is used as a multiplier
// or as a subtrahend is therefore "tidied" first (normalised, then brought below 3 r): ~45 simple instructions against the 206 of a product.
//
// The contracts below are what tests/cpp/checked_f29.h establishes when it runs this source over limbs that carry their bounds (tests/test_ed29_bounds.py, at the
// edges of every class; the lane programs of tests/cpp on top of it), and what tests/test_gpu_ed29_extremes.py holds the kernels to on rows built at those edges:
//   f29_tidy       any limbs whose carries fit 32 bits and a value below 445 r  ->  exact digits (limbs 0..7 below 2^29), below 3 r
//   f29_canonical  a multiplicand (limbs below 2^31.4, value below 2^261 = 438.79 r)  ->  the digits of the canonical number, below r
//   Ed29           every coordinate exact digits and below 3 r: a product (below 1.14 r from these formulas), a table constant (below r) or a tidied value (the
//                  lanes store w, s and f29_neg_tidy(..) into points).  ed29_add and ed29_dbl accept that and return X, Y, Z, T below 1.1373 r: closed.
//   Ed29Cached     ym, yp, z2, k exact digits and below 3 r (ed29_cache: three tidied values and a product below 1.01 r; a table entry: canonical numbers)
// With operands at those edges the largest product column is 0.47 of 2^64, the tightest padded difference is e = s - h of ed29_dbl (h = A + B lazy: 21 units
// of limb 0 to spare) and every subtrahend stays below 3 r of the 18 r the padding covers.
#pragma once
#ifndef ALEO_F29_PROVIDED      // tests/cpp/checked_f29.h supplies the same field on the host, with every bound above checked
#include "fr29.h"
#endif

#ifndef ALEO_F29_LIMB_WRITES_PROVIDED      // ... and, where it says so, the five below as well
namespace aleo_mi355x {
// Everything in the lanes that writes a limb other than through fr29.h: tests/cpp/checked_f29.h supplies these five with bounds, so the lanes' source runs on it unmodified
// (a host field that supplies fr29.h's part alone takes them as they stand here).
__device__ __forceinline__ F29 f29_limbs(const uint32_t* p, uint32_t at = 0) { F29 r;                // nine limbs as they lie in a table (from word `at`) or an argument block
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = p[at + i];
  return r; }
__device__ __forceinline__ F29 f29_small(uint32_t k) { F29 r; r.v[0] = k;                             // the plain number k
#pragma unroll
  for (int i = 1; i < 9; ++i) r.v[i] = 0;
  return r; }
__device__ __forceinline__ F29 f29_zero_if(bool c, const F29& a) { F29 r;                             // a malformed lane goes through the motions on zeros
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = c ? 0u : a.v[i];
  return r; }
__device__ __forceinline__ F29 f29_select(bool c, const F29& a, const F29& b) { F29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = c ? a.v[i] : b.v[i];
  return r; }
__device__ __forceinline__ F29 f29_sub_r_if_ge(F29 r) {                                               // exact digits, at most r -> below r
  bool ge = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) ge = r.v[i] > FR29_P[i] || (r.v[i] == FR29_P[i] && ge);
  int32_t br = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) { const int32_t t = (int32_t)r.v[i] - (ge ? (int32_t)FR29_P[i] : 0) + br; r.v[i] = (uint32_t)t & M29; br = t >> 29; }
  return r;
}
}  // namespace aleo_mi355x
#endif

namespace aleo_mi355x {

__device__ __forceinline__ void f29_tidy(F29& a) { f29_normalise(a); f29_reduce_partial(a); }       // any lazy value below 445 r -> exact digits, below 3 r
__device__ __forceinline__ F29 f29_sqr(const F29& a) { return f29_mul(a, a); }                       // a normalised
// Montgomery form -> the canonical number (limbs of a value below r): one product by the plain 1 leaves a value <= r, one conditional subtraction the rest
__device__ __forceinline__ F29 f29_canonical(const F29& a) {
  return f29_sub_r_if_ge(f29_mul(a, f29_small(1)));
}
__device__ __forceinline__ bool f29_same_limbs(const F29& a, const F29& b) { uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) o |= a.v[i] ^ b.v[i];
  return o == 0; }
__device__ __forceinline__ bool f29_below_r(const F29& a) {                                           // a normalised, below 2^256
  bool ge = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) ge = a.v[i] > FR29_P[i] || (a.v[i] == FR29_P[i] && ge);
  return !ge;
}

struct Ed29 { F29 X, Y, Z, T; };                         // every coordinate exact digits, below 3 r (a product, a table constant or a tidied value)
struct Ed29Cached { F29 ym, yp, k, z2; };                // Y - X, Y + X, 2 d T, 2 Z of a fixed second operand: exact digits, below 3 r (tidied; k a product)

__device__ __forceinline__ Ed29Cached ed29_cache(const Ed29& p, const F29& d2) {
  Ed29Cached c;
  c.ym = f29_sub_pad(p.Y, p.X); f29_tidy(c.ym);
  c.yp = f29_add(p.Y, p.X); f29_tidy(c.yp);
  c.k = f29_mul(p.T, d2);
  c.z2 = f29_add(p.Z, p.Z); f29_tidy(c.z2);
  return c;
}

// p <- p + q, or p - q when `neg` (the negative of (x, y) is (-x, y): the two cached sums change places and 2 d T changes sign)
__device__ __forceinline__ void ed29_add(Ed29& p, const Ed29Cached& q, bool neg) {
  const F29 a = f29_mul(f29_sub_pad(p.Y, p.X), f29_select(neg, q.yp, q.ym));
  const F29 b = f29_mul(f29_add(p.Y, p.X), f29_select(neg, q.ym, q.yp));
  const F29 c = f29_mul(p.T, q.k);
  const F29 d = f29_mul(p.Z, q.z2);
  const F29 e = f29_sub_pad(b, a);
  F29 h = f29_add(b, a);
  const F29 dmc = f29_sub_pad(d, c), dpc = f29_add(d, c);
  F29 f = f29_select(neg, dpc, dmc);
  const F29 g = f29_select(neg, dmc, dpc);
  f29_tidy(f); f29_tidy(h);
  p.X = f29_mul(e, f); p.Y = f29_mul(g, h); p.T = f29_mul(e, h); p.Z = f29_mul(g, f);
}

// p <- 2 p.  With A = X^2, B = Y^2: e = (X + Y)^2 - A - B, g = B - A, f = 2 Z^2 - g, h = A + B; (e f : g h : f g : e h) is the textbook result with
// all four coordinates negated, which is the same point and keeps every difference a padded one.
__device__ __forceinline__ void ed29_dbl(Ed29& p, bool want_t) {
  const F29 a = f29_sqr(p.X), b = f29_sqr(p.Y), zz = f29_sqr(p.Z);
  F29 xy = f29_add(p.X, p.Y); f29_normalise(xy);
  const F29 s = f29_sqr(xy);
  F29 h = f29_add(a, b);
  const F29 e = f29_sub_pad(s, h);
  F29 g = f29_sub_pad(b, a); f29_tidy(g);
  F29 f = f29_sub_pad(f29_add(zz, zz), g); f29_tidy(f);
  f29_normalise(h);
  p.X = f29_mul(e, f); p.Y = f29_mul(g, h); p.Z = f29_mul(f, g);
  if (want_t) p.T = f29_mul(e, h);
}

}  // namespace aleo_mi355x
