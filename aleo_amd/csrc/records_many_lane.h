// records_many_lane.h — what ONE lane of the grouped record scan computes (records_many.hip launches it): the ownership test of records_lane.h for ONE
// record against a GROUP of W accounts, sharing everything that depends on the record alone.
//
//   per record: the root that puts the nonce on the curve and the malformed test (as records_scan_lane), the doublings of the scalar multiplication, ONE inversion;
//   per key:    the additions of its own digits, the conversion of its rvk, one Poseidon permutation, the comparison with its address.
//
// The scalar, right to left.  The keys of a group are uniform over the launch, so every branch below is uniform.  One running point Q = 2^i P is doubled once
// per digit position for the whole group (T only when the next position holds a digit of some key), cached once per position that holds one, and added to or
// subtracted from the accumulator of every key whose digit there is not zero.  The accumulators start at the neutral point (0 : 1 : 1 : 0): the law is
// complete, so the first addition needs no special case, and an accumulator that never receives a digit (a padded place of the last group: all its masks are
// zero) stays neutral with Z = 1.  The loop runs to the longest digit string of the group; a key's masks are zero beyond its own length.
// The inversion.  Prefix products of the W accumulators' Z, one Fermat chain on the last of them, back-substitution: Z is never 0.
// The per-key tail runs as a loop over the live keys that is NOT unrolled (one copy of the permutation's code): a lane array indexed by that loop's counter
// would live in scratch, so the caller parks the W values x = X / Z between the two phases (`park(j, x)` with constant j, `fetch(j)` with the counter) —
// the kernel in LDS, the emulation in an array.  `emit(j, rvk)` is handed the canonical limbs of key j's record view key x (zeros with flag 2), `done(j, flag)`
// its flag; this header itself touches neither LDS nor thread indices nor memory other than K and A, and compiles as plain C++.
#pragma once
#include "records_lane.h"

namespace aleo_mi355x {

__device__ __forceinline__ bool naf_digit(const ScanArgs& a, uint32_t i, bool& neg) {      // digit i of a key is not zero; neg: it is -1
  const uint32_t p = (a.naf_pos[i >> 5] >> (i & 31)) & 1u, m = (a.naf_neg[i >> 5] >> (i & 31)) & 1u;
  neg = m != 0;
  return (p | m) != 0;
}
template <int W> __device__ __forceinline__ bool naf_any(const ScanArgs* __restrict__ A, uint32_t i) {
  uint32_t o = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) o |= A[j].naf_pos[i >> 5] | A[j].naf_neg[i >> 5];
  return (o >> (i & 31)) & 1u;
}

// One record against the keys A[0 .. W): the first `live` of them are answered (1 <= live <= W; the rest are padding, all masks zero), naf_len_max is the
// longest naf_len among them.  c0w / nxw as in records_scan_lane.
template <int W, class Park, class Fetch, class Emit, class Done>
__device__ __forceinline__ void records_scan_lane_many(const uint32_t (&c0w)[8], const uint32_t (&nxw)[8], const uint32_t* __restrict__ K, const ScanArgs* __restrict__ A,
                                                       uint32_t live, uint32_t naf_len_max, Park&& park, Fetch&& fetch, Emit&& emit, Done&& done) {
  // the record alone: exactly the head of records_scan_lane
  F29 nx = f29_from_words(nxw);
  bool bad = !f29_below_r(f29_from_words(c0w)) || !f29_below_r(nx);
  nx = f29_zero_if(bad, nx);
  const F29 one = rk_const(K, RK_ONE);
  Ed29 q;                                                                           // Q = 2^i P
  {
    const F29 x = f29_mul(nx, rk_const(K, RK_R2));
    const F29 xx = f29_sqr(x);
    F29 w = f29_sub_pad(one, f29_mul(xx, rk_const(K, RK_D))); f29_tidy(w);
    const F29 a = f29_mul(f29_add(one, xx), w);
    const F29 s = f29_sqrt_fixed(a, K);
    bad = bad || !f29_same_limbs(f29_canonical(f29_sqr(s)), f29_canonical(a));
    q.X = f29_mul(x, w); q.Y = s; q.Z = w; q.T = f29_mul(x, s);
  }
  Ed29 acc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    acc[j].Y = one; acc[j].Z = one;
    acc[j].X = f29_small(0); acc[j].T = f29_small(0);
  }
  const F29 d2 = rk_const(K, RK_D2);
  bool any = naf_len_max != 0;                                                      // every k is odd: position 0 holds a digit of every live key
  for (uint32_t i = 0; i < naf_len_max; ++i) {
    if (any) {
      const Ed29Cached qc = ed29_cache(q, d2);
#pragma unroll
      for (int j = 0; j < W; ++j) { bool neg; if (naf_digit(A[j], i, neg)) ed29_add(acc[j], qc, neg); }
    }
    if (i + 1 < naf_len_max) { any = naf_any<W>(A, i + 1); ed29_dbl(q, any); }
  }
  // one inversion for the group
  {
    F29 pre[W];
    pre[0] = acc[0].Z;
#pragma unroll
    for (int j = 1; j < W; ++j) pre[j] = f29_mul(pre[j - 1], acc[j].Z);
    F29 inv = f29_pow(pre[W - 1], K + RK_EXP_INV, RK_INV_BITS);
#pragma unroll
    for (int j = W - 1; j >= 1; --j) {
      park(j, f29_mul(acc[j].X, f29_mul(inv, pre[j - 1])));
      inv = f29_mul(inv, acc[j].Z);
    }
    park(0, f29_mul(acc[0].X, inv));
  }
  // per key: as the tail of records_scan_lane
  const F29 c0 = f29_mul(f29_zero_if(bad, f29_from_words(c0w)), rk_const(K, RK_R2));
  for (uint32_t j = 0; j < live; ++j) {
    const F29 xq = fetch(j);
    emit(j, f29_zero_if(bad, f29_canonical(xq)));
    F29 st[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) st[i] = rk_const(K, RK_S0 + i);
    st[2] = f29_add(st[2], xq);
    const F29 rnd = psd_permute_take1(st, K);
    const F29 addr = f29_limbs(A[j].addr);
    const bool owner = f29_same_limbs(f29_canonical(f29_sub_pad(c0, rnd)), addr);
    done(j, bad ? 2u : (owner ? 1u : 0u));
  }
}

}  // namespace aleo_mi355x
