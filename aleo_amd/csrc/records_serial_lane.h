// records_serial_lane.h — what ONE lane of the serial-number kernel computes (records_serial.hip launches it, one commitment per lane):
// Record<N, Plaintext<N>>::serial_number(private_key, commitment) of snarkVM 0.14.5 [UPSTREAM-RECALL; every stage pinned by reference-held data:
// tests/serial_ref.py, tests/golden/reference_serial.json] — the step between "the account owns this record" and "it is unspent" in the reference's
// get_unspent_records (rust/src/api/blocking.rs:277).
//
//   (h0, h1) = Poseidon2 hash_many([D, cm], 2)            D = the domain separator "AleoSerialNumber0"
//   H        = 4 (Elligator2(h0) + Elligator2(h1))        the cofactor is cleared once, after the sum
//   gamma    = sk_sig H
//   nonce    = the low 250 bits of Poseidon2 hash([D, x(4 gamma)])
//   sn       = x(BHP512 hash of (D, cm)'s 506 bits + sum_i bit_i(nonce) R_i)
//
// The hashes.  Both preimages are [AleoPoseidon2, 2 | D, *]: the first permutation is the same for every lane and every call, so a lane starts from that
// state with D already added (SK_S0) and runs ONE width-3 permutation per hash, in the plain round form (a width-3 round is 9 products either way).
// Elligator2.  On y^2 = x^3 + a x^2 + b x with a = A / B, b = 1 / B^2 (A, B the Montgomery coefficients of the curve) and the non-residue u = d = 3021:
// q = 1 + d r^2, v = -a / q, e = the Legendre symbol of v^3 + a v^2 + b v, x = v or -v - a, y = -e sqrt(x^3 + a x^2 + b x) with the root that is not
// above (r - 1) / 2; Montgomery (x B, y B) = (s, t); Edwards (s / t, (s - 1) / (s + 1)) = (s (s + 1) : (s - 1) t : t (s + 1)), no inversion.  The two
// maps share the one inversion of q0 q1; the symbol is one exponentiation, the root is f29_sqrt_fixed (records_lane.h) of the side the symbol chose.
// Upstream returns Err for r = 0, a^2 d r^2 = b q^2, a zero v, x or y, and an inverse of zero (s + 1): the lane's flag 2, with the same tests.
// sk_sig H.  The key is the same for every lane: the host recodes it once (the odd one of {sk_sig, sk_sig + l}, non-adjacent form: H has order l) and
// passes the digit masks by value, as the scan does with the view key.  The addition law of edwards29.h is complete — a = -1 is a square and d is not,
// so no denominator 1 +- d x1 x2 y1 y2 vanishes for any pair of rational points, equal, opposite, the identity or of small order alike — so neither this
// loop nor the table additions below has an exceptional case to branch on, and a key of 0 (l H = O, x = 0) needs no case of its own.
// BHP512.  The one iteration hashes 758 bits = 253 chunks of 3.  Chunks 0 .. 167 hold the 252-bit prefix and 252 bits of D: the host sums them into a
// starting point (SK_START).  The lane adds chunks 168 .. 252 — 85 signed additions from an 85 x 4 table of cached affine points (k base_j, k = 1 .. 4) —
// then the randomizer from a table of 4-bit windows: 63 additions from 63 x 16 entries (entry 0 the identity: no lane branches on its digit).  Three
// elements per entry (y - x, y + x, 2 d x y; 2 Z is the constant 2), 108 bytes: 36 KB + 106 KB, with the constants 181 KB resident per device — a
// twentieth of one XCD's 4 MB of L2, which every wave of a launch reads.  5-bit windows would save 12 of ~150 additions for twice the table.
// One inversion brings x(4 gamma) to affine, one the result: three exponentiations by r - 2 in all.
#pragma once
#include "records_lane.h"

namespace aleo_mi355x {

// The constants of the serial numbers: the scan's (records_lane.h RK_*: R2, 1, d, 2 d, the roots and exponents of f29_sqrt_fixed) come first, unchanged,
// so that K serves rk_const and f29_sqrt_fixed as it stands; then, in units of one element from SK_E0 on (Montgomery form unless said otherwise):
enum : uint32_t {
  SK_E0 = (RK_WORDS + 8) / 9,
  SK_S0 = SK_E0,               // 3: the sponge after [AleoPoseidon2, 2], D added to its first rate element
  SK_ARK = SK_S0 + 3,          // 39 x 3
  SK_MDS = SK_ARK + 117,       // 3 x 3
  SK_A = SK_MDS + 9, SK_B, SK_NEGA, SK_A2, SK_MB, SK_TWO,      // a, b, -a, a^2, the Montgomery B, 2
  SK_START,                    // 4: X, Y, Z = 1, T of the sum of chunks 0 .. 167
  SK_HALF = SK_START + 4,      // (r - 1) / 2 as a plain number
  SK_CHUNK = SK_HALF + 1,      // 85 x 4 x 3
  SK_RND = SK_CHUNK + 1020,    // 63 x 16 x 3
  SK_ELEMS = SK_RND + 3024,
  SK_EXP_LEG = SK_ELEMS * 9,   // 8 words: (r - 1) / 2
  SK_WORDS = SK_EXP_LEG + 8
};
static constexpr int SK_LEG_BITS = 252, SK_FIRST_CHUNK = 168, SK_CHUNKS = 85, SK_RND_WINDOWS = 63, SK_NONCE_BITS = 250, SK_CM_AT = 505;

struct SerialArgs { uint32_t naf_pos[8], naf_neg[8], naf_len; };      // the digits of the odd one of {sk_sig, sk_sig + l}, as ScanArgs holds the view key's

__device__ __forceinline__ F29 f29_zero() { return f29_small(0); }
__device__ __forceinline__ bool f29_is_zero_limbs(const F29& a) { uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) o |= a.v[i];
  return o == 0; }
__device__ __forceinline__ F29 f29_neg_tidy(const F29& a) { F29 r = f29_sub_pad(f29_zero(), a); f29_tidy(r); return r; }      // a tidied
__device__ __forceinline__ bool f29_bit(const F29& canonical, int i) { return (canonical.v[i / 29] >> (i % 29)) & 1u; }

// One width-3 permutation, plain form: 4 full rounds, 31 partial, 4 full; every element of the result tidied.  ark, mds: where the table holds the 39 x 3 round
// constants and the 3 x 3 matrix (the account lane's table has them elsewhere: account_lane.h).
__device__ __forceinline__ void psd2_permute(F29 (&s)[3], const uint32_t* __restrict__ K, const uint32_t ark = SK_ARK, const uint32_t mds = SK_MDS) {
  for (int r = 0; r < 39; ++r) {
    const bool full = r < 4 || r >= 35;
    F29 t[3];
    t[0] = psd_pow17(f29_add(s[0], rk_const(K, ark + 3 * r)));
#pragma unroll
    for (int i = 1; i < 3; ++i) {
      t[i] = f29_add(s[i], rk_const(K, ark + 3 * r + i));
      if (full) t[i] = psd_pow17(t[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      F29 acc = f29_mul(t[0], rk_const(K, mds + 3 * i));
      acc = f29_add(acc, f29_mul(t[1], rk_const(K, mds + 3 * i + 1)));
      acc = f29_add(acc, f29_mul(t[2], rk_const(K, mds + 3 * i + 2)));
      f29_tidy(acc);
      s[i] = acc;
    }
  }
}

// What Elligator2 does with one input before and after the shared inversion.  r: tidied, Montgomery form.
struct Ell29 { F29 ur2, q; };
__device__ __forceinline__ Ell29 ell29_head(const F29& r, bool& bad, const uint32_t* __restrict__ K) {
  Ell29 e;
  bad = bad || f29_is_zero_limbs(f29_canonical(r));
  e.ur2 = f29_mul(f29_sqr(r), rk_const(K, RK_D));
  e.q = f29_add(e.ur2, rk_const(K, RK_ONE)); f29_tidy(e.q);
  const F29 lhs = f29_mul(e.ur2, rk_const(K, SK_A2)), rhs = f29_mul(f29_sqr(e.q), rk_const(K, SK_B));
  bad = bad || f29_same_limbs(f29_canonical(lhs), f29_canonical(rhs));
  return e;
}
// x^3 + a x^2 + b x; x tidied
__device__ __forceinline__ F29 ell29_curve(const F29& x, const uint32_t* __restrict__ K) {
  F29 t = f29_add(f29_add(f29_sqr(x), f29_mul(x, rk_const(K, SK_A))), rk_const(K, SK_B)); f29_tidy(t);
  return f29_mul(t, x);
}
__device__ __forceinline__ Ed29 ell29_tail(const Ell29& e, const F29& qinv, bool& bad, const uint32_t* __restrict__ K) {
  F29 v = f29_mul(qinv, rk_const(K, SK_NEGA)); f29_tidy(v);
  F29 gv = ell29_curve(v, K); f29_tidy(gv);
  const F29 leg = f29_canonical(f29_pow(gv, K + SK_EXP_LEG, SK_LEG_BITS));      // 1, r - 1 or 0, as a plain number
  const F29 one = f29_small(1);
  const bool qr = f29_same_limbs(leg, one);
  bad = bad || f29_is_zero_limbs(leg);                                          // v = 0 or e = 0
  F29 alt = f29_sub_pad(rk_const(K, SK_NEGA), v); f29_tidy(alt);                // -v - a
  const F29 x = f29_select(qr, v, alt);
  bad = bad || f29_is_zero_limbs(f29_canonical(x));
  F29 g = ell29_curve(x, K); f29_tidy(g);
  bad = bad || f29_is_zero_limbs(f29_canonical(g));                             // y = 0
  F29 s = f29_sqrt_fixed(g, K); f29_tidy(s);
  const F29 sc = f29_canonical(s), half = rk_const(K, SK_HALF);
  bool above = false;
#pragma unroll
  for (int i = 0; i < 9; ++i) above = sc.v[i] > half.v[i] || (sc.v[i] == half.v[i] && above);
  // y = -e * (the root not above (r - 1) / 2): the small root for e = -1, the other one for e = 1
  const F29 y = f29_select(above == qr, s, f29_neg_tidy(s));
  F29 u = f29_mul(x, rk_const(K, SK_MB)); f29_tidy(u);
  F29 w = f29_mul(y, rk_const(K, SK_MB)); f29_tidy(w);
  F29 up = f29_add(u, rk_const(K, RK_ONE)); f29_tidy(up);
  F29 um = f29_sub_pad(u, rk_const(K, RK_ONE)); f29_tidy(um);
  bad = bad || f29_is_zero_limbs(f29_canonical(up));
  Ed29 p; p.X = f29_mul(u, up); p.Y = f29_mul(um, w); p.Z = f29_mul(w, up); p.T = f29_mul(u, um);
  return p;
}

__device__ __forceinline__ Ed29Cached sk_entry(const uint32_t* __restrict__ K, uint32_t first) {
  Ed29Cached c; c.ym = rk_const(K, first); c.yp = rk_const(K, first + 1); c.k = rk_const(K, first + 2); c.z2 = rk_const(K, SK_TWO);
  return c;
}

// One commitment.  cmw: its canonical little-endian words.  Returns the flag (0 computed, 2 refused: the commitment is not below r, or Elligator2 refuses an
// input); `emit` is handed the canonical limbs of the serial number (zeros with flag 2).
template <class Emit>
__device__ __forceinline__ uint32_t records_serial_lane(const uint32_t (&cmw)[8], const uint32_t* __restrict__ K, const SerialArgs& A, Emit&& emit) {
  F29 cm = f29_from_words(cmw);
  bool bad = !f29_below_r(cm);
  cm = f29_zero_if(bad, cm);                                                      // a refused lane goes through the motions on zeros
  const F29 d2 = rk_const(K, RK_D2);
  // H
  F29 st[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) st[i] = rk_const(K, SK_S0 + i);
  st[2] = f29_add(st[2], f29_mul(cm, rk_const(K, RK_R2)));
  psd2_permute(st, K);
  const Ell29 e0 = ell29_head(st[1], bad, K), e1 = ell29_head(st[2], bad, K);
  const F29 inv = f29_pow(f29_mul(e0.q, e1.q), K + RK_EXP_INV, RK_INV_BITS);      // q is never 0: -1 / d is not a square
  Ed29 p = ell29_tail(e0, f29_mul(inv, e1.q), bad, K);
  {
    const Ed29 p1 = ell29_tail(e1, f29_mul(inv, e0.q), bad, K);
    ed29_add(p, ed29_cache(p1, d2), false);
  }
  ed29_dbl(p, false); ed29_dbl(p, true);
  // gamma = k H, then 4 gamma
  {
    const Ed29Cached pc = ed29_cache(p, d2);
    for (int i = (int)A.naf_len - 2; i >= 0; --i) {                               // the top digit is +1: the accumulator starts at the point itself
      const bool pos = (A.naf_pos[i >> 5] >> (i & 31)) & 1u, neg = (A.naf_neg[i >> 5] >> (i & 31)) & 1u;
      ed29_dbl(p, pos || neg);
      if (pos || neg) ed29_add(p, pc, neg);
    }
  }
  ed29_dbl(p, false); ed29_dbl(p, false);
  const F29 xg = f29_mul(p.X, f29_pow(p.Z, K + RK_EXP_INV, RK_INV_BITS));         // Z is never 0 (the law is complete)
  // the nonce
#pragma unroll
  for (int i = 0; i < 3; ++i) st[i] = rk_const(K, SK_S0 + i);
  st[2] = f29_add(st[2], xg);
  psd2_permute(st, K);
  const F29 nonce = f29_canonical(st[1]);
  // the commitment: chunks 168 .. 252 of [prefix | D | cm | padding], then the randomizer
  p.X = rk_const(K, SK_START); p.Y = rk_const(K, SK_START + 1); p.Z = rk_const(K, SK_START + 2); p.T = rk_const(K, SK_START + 3);
  auto cm_bit = [&](int at) -> uint32_t {                                         // bit `at` of the hashed bits, at >= 504: D's top bit (0), cm's 253 bits, padding
    const int j = at - SK_CM_AT;
    return j >= 0 && j < 253 ? (cmw[j >> 5] >> (j & 31)) & 1u : 0u;
  };
  for (int c = 0; c < SK_CHUNKS; ++c) {
    const int at = 3 * (SK_FIRST_CHUNK + c);
    const uint32_t m = cm_bit(at) | cm_bit(at + 1) << 1;
    ed29_add(p, sk_entry(K, SK_CHUNK + 3 * (4 * c + m)), cm_bit(at + 2) != 0);
  }
  for (int w = 0; w < SK_RND_WINDOWS; ++w) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) if (4 * w + b < SK_NONCE_BITS) v |= (uint32_t)f29_bit(nonce, 4 * w + b) << b;
    ed29_add(p, sk_entry(K, SK_RND + 3 * (16 * w + v)), false);
  }
  emit(f29_zero_if(bad, f29_canonical(f29_mul(p.X, f29_pow(p.Z, K + RK_EXP_INV, RK_INV_BITS)))));
  return bad ? 2u : 0u;
}

}  // namespace aleo_mi355x
