// records_decrypt_lane.h — what ONE lane of the record decryption computes (records_decrypt.hip launches it, one record per lane): the plain fields of
// Record<N, Ciphertext<N>>::decrypt_symmetric_unchecked, snarkVM 0.14.5 console/program/src/data/record/decrypt.rs and ciphertext/decrypt.rs
// [UPSTREAM-RECALL; pinned by tests/golden/reference_records.json for a private owner and one private u64 entry].
//
//   randomizers = hash_many_psd8([encryption domain, rvk], m);  plain_i = c_i - randomizers_i,  i < m, the record's private fields in randomizer order.
//
// The sponge.  As in the scan (records_lane.h) the state after the first block does not depend on the record: the lane starts from RK_S0, adds its record
// view key to element 2 and squeezes: one width-9 permutation hands out eight randomizers (its rate elements 1..8 — the eight of which the scan keeps one), a
// record with more than eight private fields permutes again and goes on.  ~1 750 Fr products per permutation, against the ~5 500 of a scanned record.
// Lanes of a wave differ in m: the loop over blocks of eight is a loop on lane data, so a wave runs as long as its longest record and the shorter ones idle
// (the cost model, and why the records are not sorted).
// Plain C++ over f29_mul: the lane takes its fields through `load`, hands its rows to `emit` and touches no thread index, so the host runs the same code
// over a field that checks every limb rule (tests/cpp/records_decrypt_lane_emul.cpp).
#pragma once
#include "records_lane.h"

namespace aleo_mi355x {

// One record of m private fields.  rvkw: the canonical little-endian words of the record view key's x.  load(j, w): the words of ciphertext field j;
// emit(j, v): the canonical limbs of plain field j — each j < m once, in order, after every field has been loaded once (an emit may overwrite what load(j)
// read).  Returns the flag: 0 decrypted, 2 malformed (rvk or one of the fields is not below r: the lane goes through the motions on zeros and emits zero rows).
template <class Load, class Emit>
__device__ __forceinline__ uint32_t records_decrypt_lane(const uint32_t (&rvkw)[8], uint32_t m, const uint32_t* __restrict__ K, Load&& load, Emit&& emit) {
  F29 rv = f29_from_words(rvkw);
  bool bad = !f29_below_r(rv);
  for (uint32_t j = 0; j < m; ++j) { uint32_t w[8]; load(j, w); bad = bad || !f29_below_r(f29_from_words(w)); }
  rv = f29_zero_if(bad, rv);
  const F29 r2 = rk_const(K, RK_R2);
  F29 st[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) st[i] = rk_const(K, RK_S0 + i);
  st[2] = f29_add(st[2], f29_mul(rv, r2));
  for (uint32_t at = 0; at < m; at += 8) {
    psd_permute(st, K);                                           // every element tidied: a subtrahend below, a summand of the next permutation's first round
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j)
      if (at + j < m) {
        uint32_t w[8]; load(at + j, w);
        const F29 c = f29_zero_if(bad, f29_from_words(w));
        emit(at + j, f29_zero_if(bad, f29_canonical(f29_sub_pad(f29_mul(c, r2), st[1 + j]))));
      }
  }
  return bad ? 2u : 0u;
}

}  // namespace aleo_mi355x
