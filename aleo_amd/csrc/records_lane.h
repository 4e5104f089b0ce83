// records_lane.h — what ONE lane of the record scan computes (records.hip launches it, one record per lane): the ownership test of
// Record<N, Ciphertext<N>>::is_owner_with_address_x_coordinate for a private owner [UPSTREAM-RECALL; pinned by tests/golden/reference_records.json].
//
//   x = nonce, y^2 = (1 + x^2) / (1 - 3021 x^2);  rvk = x(k (x, y)),  k the odd one of {view key, view key + l};
//   randomizer = Poseidon8([encryption domain, rvk]);  owner <=> c0 - randomizer == address x.
//
// The root.  With u = 1 + x^2 and w = 1 - 3021 x^2 the point is taken projectively, (x w : s : w) with s^2 = u w, so the ratio needs no inversion and
// "u / w is not a square" is "u w is not a square".  Fr - 1 = 2^47 t: s comes from ONE exponentiation a^((t - 1) / 2) (205 squarings) and a
// Tonelli-Shanks correction run on a FIXED schedule (f29_sqrt_fixed: every lane of a wave executes the same instructions, whatever its correction is;
// the data-dependent loop would cost a wave its worst lane's length anyway), in chunks of eight bits: 265 squarings and 3 products per bit instead of the
// 1035 squarings of the bit-by-bit form.  The result is checked by squaring it (flag 2 otherwise).
// The scalar.  k is the same for every lane: the host recodes it into its non-adjacent form and passes the two digit masks by value; a lane doubles
// ~252 times and adds or subtracts its own point ~84 times, with no table (a fixed window of four bits would add 63 times from 8 stored points: the
// same number of products once the stored points' Z is paid for, and 1152 bytes of table per lane).  Branches are on uniform data only.
// The hash.  The first permutation of the preimage [AleoPoseidon8, 2, 0 x 6 | domain, rvk] does not depend on the record: the lane starts from that
// state (RecordsConsts::S0) and runs one width-9 permutation in the sparse form of poseidon.hpp, constants converted once by the host.
#pragma once
#include "edwards29.h"

namespace aleo_mi355x {

// The constants of a scan, in units of one element (9 words, Montgomery form unless said otherwise); the exponents follow as plain words.
enum : uint32_t {
  RK_R2 = 0,                   // 2^522 mod r: canonical number -> Montgomery form
  RK_ONE = 1, RK_D = 2, RK_D2 = 3,      // 1, 3021, 6042
  RK_S0 = 4,                   // the sponge's state after the first block, the encryption domain already added to its second element
  RK_ARK_HEAD = 13,            // 4 x 9: the constants of the first four full rounds
  RK_MDS = 49, RK_PRE = 130,   // 81 each: the MDS matrix, and the matrix of the fourth full round (poseidon.hpp `pre`)
  RK_PART = 211,               // 31 x 18: c, m00, v[8], w[8] of every partial round
  RK_ARK_AFTER = 769,          // 9
  RK_ARK_TAIL = 778,           // 3 x 9: the constants of the last three full rounds
  RK_ROOTS = 805,              // 47: g^(2^j), g a generator of the 2^47-th roots of unity
  RK_ELEMS = 852,
  RK_EXP_SQRT = RK_ELEMS * 9,  // 8 words: (t - 1) / 2
  RK_EXP_INV = RK_EXP_SQRT + 8,       // 8 words: r - 2
  RK_WORDS = RK_EXP_INV + 8
};
static constexpr int RK_SQRT_BITS = 205, RK_INV_BITS = 253, RK_TWO_ADICITY = 47;

struct ScanArgs { uint32_t naf_pos[8], naf_neg[8], naf_len; uint32_t addr[9]; };      // digits of k (bit i of pos / neg: digit i is +1 / -1), canonical limbs of the address x

__device__ __forceinline__ F29 rk_const(const uint32_t* __restrict__ K, uint32_t idx) { return f29_limbs(K, idx * 9); }

#ifdef __HIPCC__
// the 32 bytes at p (16-byte aligned) as eight words, by two 16-byte loads: how the kernels hand a lane a field that lies in device memory
__device__ __forceinline__ void load_words8(uint32_t (&w)[8], const char* p) {
  const uint4* q = (const uint4*)p; const uint4 l = q[0], h = q[1];
  w[0] = l.x; w[1] = l.y; w[2] = l.z; w[3] = l.w; w[4] = h.x; w[5] = h.y; w[6] = h.z; w[7] = h.w;
}
#endif

// a^e for an exponent of `bits` bits (its top bit set) held in uniform words; a normalised
__device__ __forceinline__ F29 f29_pow(const F29& a, const uint32_t* __restrict__ e, int bits) {
  F29 acc = a;
  for (int bit = bits - 2; bit >= 0; --bit) {
    acc = f29_sqr(acc);
    if ((e[bit >> 5] >> (bit & 31)) & 1u) acc = f29_mul(acc, a);
  }
  return acc;
}

// s with s^2 = a when a is a square (a = 0 included); anything otherwise — the caller squares it.
// x = a^((t+1)/2) and b = a^t satisfy x^2 = a b, and b is a 2^46-th root of unity: b g^(2E) = 1 for one 46-bit E, and x g^E is the root.  E is found in
// chunks of SQRT_CHUNK bits from the bottom (Pohlig-Hellman inside Tonelli-Shanks): h = b^(2^(46 - j0 - c)) has order at most 2^c and carries the chunk's c bits,
// which cost c (c - 1) / 2 squarings of h instead of squarings of b over the whole remaining height; every set bit multiplies x, b and h by the matching power
// of g (both results computed, one selected: no branch on lane data).
static constexpr int SQRT_CHUNK = 8;
__device__ __forceinline__ F29 f29_sqrt_fixed(const F29& a, const uint32_t* __restrict__ K) {
  const F29 y = f29_pow(a, K + RK_EXP_SQRT, RK_SQRT_BITS);
  F29 x = f29_mul(y, a), b = f29_mul(x, y);
  const F29 one = f29_small(1);
  constexpr int HEIGHT = RK_TWO_ADICITY - 1;                      // 46
  for (int j0 = 0; j0 < HEIGHT; j0 += SQRT_CHUNK) {
    const int c = HEIGHT - j0 < SQRT_CHUNK ? HEIGHT - j0 : SQRT_CHUNK;
    F29 h = b;
    for (int k = 0; k < HEIGHT - j0 - c; ++k) h = f29_sqr(h);
    for (int i = 0; i < c; ++i) {                                 // bit j0 + i of E: is h^(2^(c-1-i)) the number -1?
      F29 e = h;
      for (int k = 0; k < c - 1 - i; ++k) e = f29_sqr(e);
      const bool fix = !f29_same_limbs(f29_canonical(e), one);
      const F29 xm = f29_mul(x, rk_const(K, RK_ROOTS + j0 + i)), bm = f29_mul(b, rk_const(K, RK_ROOTS + j0 + i + 1)), hm = f29_mul(h, rk_const(K, RK_ROOTS + RK_TWO_ADICITY - c + i));
      x = f29_select(fix, xm, x); b = f29_select(fix, bm, b); h = f29_select(fix, hm, h);
    }
  }
  return x;
}

__device__ __forceinline__ F29 psd_pow17(F29 t) {
  f29_normalise(t);
  F29 a = f29_sqr(t); a = f29_sqr(a); a = f29_sqr(a); a = f29_sqr(a);
  return f29_mul(a, t);
}
// sum_j s[j] * K[row + j], tidied: a row of nine products reduced once (four lazy sums fit a limb, so the carries are pushed twice on the way)
__device__ __forceinline__ F29 psd_row(const F29 (&s)[9], const uint32_t* __restrict__ K, uint32_t row) {
  F29 acc = f29_mul(s[0], rk_const(K, row));
#pragma unroll
  for (int j = 1; j < 9; ++j) {
    acc = f29_add(acc, f29_mul(s[j], rk_const(K, row + j)));
    if (j == 3 || j == 6) f29_normalise(acc);
  }
  f29_tidy(acc);
  return acc;
}
template <bool LAST> __device__ __forceinline__ void psd_full(F29 (&s)[9], const uint32_t* __restrict__ K, uint32_t ark, uint32_t m) {
#pragma unroll
  for (int i = 0; i < 9; ++i) s[i] = psd_pow17(f29_add(s[i], rk_const(K, ark + i)));
  if constexpr (LAST) { s[1] = psd_row(s, K, m + 9); return; }      // only the first rate element leaves the sponge
  F29 o[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) o[i] = psd_row(s, K, m + 9 * i);
#pragma unroll
  for (int i = 0; i < 9; ++i) s[i] = o[i];
}
// The permutation of poseidon.hpp (poseidon_permute<4, 8>).  ALL: every element of the result is kept, tidied — the state a sponge goes on from — and the last
// round is one more turn of the second half's loop; otherwise it is written out and computes element 1 alone
template <bool ALL> __device__ __forceinline__ void psd_permute_rounds(F29 (&s)[9], const uint32_t* __restrict__ K) {
  for (int half = 0; half < 2; ++half) {
    const int rounds = half == 0 || ALL ? 4 : 3;
    for (int r = 0; r < rounds; ++r) {
      const uint32_t ark = half == 0 ? RK_ARK_HEAD + 9 * r : (r == 0 ? (uint32_t)RK_ARK_AFTER : RK_ARK_TAIL + 9 * (r - 1));
      psd_full<false>(s, K, ark, half == 0 && r == 3 ? (uint32_t)RK_PRE : (uint32_t)RK_MDS);
    }
    if (half == 0)
      for (int j = 0; j < 31; ++j) {
        const uint32_t base = RK_PART + 18 * j;
        F29 t[9];
        t[0] = psd_pow17(f29_add(s[0], rk_const(K, base)));
#pragma unroll
        for (int i = 1; i < 9; ++i) t[i] = s[i];
        const F29 s0 = psd_row(t, K, base + 1);                   // x m00 + sum s[i] v[i - 1]
#pragma unroll
        for (int i = 1; i < 9; ++i) { s[i] = f29_add(s[i], f29_mul(t[0], rk_const(K, base + 9 + i))); f29_tidy(s[i]); }
        s[0] = s0;
      }
  }
  if constexpr (!ALL) psd_full<true>(s, K, RK_ARK_TAIL + 18, RK_MDS);
}
// ... of which only element 1 of the result is kept (the scan: one randomizer)
__device__ __forceinline__ F29 psd_permute_take1(F29 (&s)[9], const uint32_t* __restrict__ K) { psd_permute_rounds<false>(s, K); return s[1]; }
// ... and the whole of it (records_decrypt_lane.h: eight randomizers per permutation)
__device__ __forceinline__ void psd_permute(F29 (&s)[9], const uint32_t* __restrict__ K) { psd_permute_rounds<true>(s, K); }

// One record.  c0w / nxw: the canonical little-endian words of the owner ciphertext's field and of the nonce x.  Returns the flag (0 not owner, 1 owner,
// 2 malformed).  `emit` is handed the canonical limbs of the record view key's x (zeros with flag 2) between the scalar multiplication and the hash,
// where the kernel stores them: the owner field is not converted before the last comparison either, so the hash phase carries neither in Montgomery form.
template <class Emit>
__device__ __forceinline__ uint32_t records_scan_lane(const uint32_t (&c0w)[8], const uint32_t (&nxw)[8], const uint32_t* __restrict__ K, const ScanArgs& A, Emit&& emit) {
  F29 nx = f29_from_words(nxw);
  bool bad = !f29_below_r(f29_from_words(c0w)) || !f29_below_r(nx);
  nx = f29_zero_if(bad, nx);                                                      // a malformed lane goes through the motions on zeros
  const F29 one = rk_const(K, RK_ONE);
  const F29 x = f29_mul(nx, rk_const(K, RK_R2));
  const F29 xx = f29_sqr(x);
  F29 w = f29_sub_pad(one, f29_mul(xx, rk_const(K, RK_D))); f29_tidy(w);        // 1 - d x^2 (never 0: d is not a square)
  const F29 a = f29_mul(f29_add(one, xx), w);                                     // u w
  const F29 s = f29_sqrt_fixed(a, K);
  bad = bad || !f29_same_limbs(f29_canonical(f29_sqr(s)), f29_canonical(a));      // x is not on the curve
  Ed29 p; p.X = f29_mul(x, w); p.Y = s; p.Z = w; p.T = f29_mul(x, s);
  const Ed29Cached pc = ed29_cache(p, rk_const(K, RK_D2));
  for (int i = (int)A.naf_len - 2; i >= 0; --i) {                                 // the top digit is +1: the accumulator starts at the point itself
    const bool pos = (A.naf_pos[i >> 5] >> (i & 31)) & 1u, neg = (A.naf_neg[i >> 5] >> (i & 31)) & 1u;
    ed29_dbl(p, pos || neg);
    if (pos || neg) ed29_add(p, pc, neg);
  }
  const F29 xq = f29_mul(p.X, f29_pow(p.Z, K + RK_EXP_INV, RK_INV_BITS));         // Z is never 0 (the law is complete)
  emit(f29_zero_if(bad, f29_canonical(xq)));
  F29 st[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) st[i] = rk_const(K, RK_S0 + i);
  st[2] = f29_add(st[2], xq);
  const F29 rnd = psd_permute_take1(st, K);
  const F29 c0 = f29_zero_if(bad, f29_from_words(c0w)), addr = f29_limbs(A.addr);
  const bool owner = f29_same_limbs(f29_canonical(f29_sub_pad(f29_mul(c0, rk_const(K, RK_R2)), rnd)), addr);
  return bad ? 2u : (owner ? 1u : 0u);
}

}  // namespace aleo_mi355x
