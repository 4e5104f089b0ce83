// signature_sign_lane.h — what ONE lane of the signing kernel computes (signatures.hip launches it, one signature per lane): Signature<N>::sign of snarkVM 0.14.5,
// console/account/src/signature [UPSTREAM-RECALL] — what the reference reaches through wasm/src/account/signature.rs:37-44, wasm/src/account/private_key.rs:92-96
// and sdk/src/account.ts:195.  Byte for byte signature_host.hpp's sign_with_nonce under nonce_of_seed, which is the definition; what of it is pinned by the
// reference's data and what is UNPINNED (the order of the preimage, the packing, the layout, the cap) is said there and in signature_lane.h, and holds here unchanged.
//
//   nonce      sg_nonce_of_seed(seed) (signature_lane.h): the one function the host path calls too; lanes of a wave leave its loop after different counts
//   key row    sk_sig | pk_sig.x | pr_sig.x | address.x, 32 canonical bytes each: one row for all lanes or one per lane, derived before this lane runs (on the
//              host for one key; by k_signer_keys, account_lane with its sink, for a key each)
//   g_r        nonce G: 63 additions from the resident table (sg_add_mul_g), one inversion for x
//   challenge  sg_challenge (signature_lane.h): the rate-8 sponge streams the message from global memory, the same code the verifying lane runs
//   response   nonce - challenge sk_sig mod l: an 8 x 8-word product, Barrett's reduction (HAC 14.42 with b = 2^32, k = 8: mu = floor(2^512 / l), nine words,
//              the quotient estimate at most 2 short, so two conditional subtractions of l), then a subtraction with l added back on a borrow — every step on
//              the lane's own 32-bit words, the words never indexed by lane data, no branch
//   row        challenge | response | pk_sig.x | pr_sig.x
// Flags: 0 signed; 3 no signature is made — the caller's `refused` (the key's seed is no canonical field element) or a message over the cap: such a lane goes
// through the motions on zeros to the end and its row is zeros.
// Neither this lane nor the host path is hardened against side channels: the table's lookups are indexed by the nonce's digits, as the account lane's are by the
// key's.
#pragma once
#include "account_lane.h"

namespace aleo_mi355x {

static constexpr uint32_t SIGN_OK = 0, SIGN_REFUSED = 3;
// floor(2^512 / l), least significant word first
static constexpr uint32_t SIG_BARRETT_MU[9] = {0xf087e05eu, 0xfa6edc84u, 0x3f4770bau, 0x298f7661u, 0xa805492au, 0xe51e49fau, 0x0b2c9ee4u, 0xd9491ec4u, 0x00000036u};

// out = a b, the low NO words of it (NO <= NA + NB): schoolbook, every index a constant
template <int NA, int NB, int NO>
__device__ __forceinline__ void sg_mul_words(uint32_t (&out)[NO], const uint32_t (&a)[NA], const uint32_t (&b)[NB]) {
#pragma unroll
  for (int i = 0; i < NO; ++i) out[i] = 0;
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (i + j < NO) {
        const uint64_t t = (uint64_t)a[i] * b[j] + out[i + j] + carry;            // at most (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
        out[i + j] = (uint32_t)t; carry = (uint32_t)(t >> 32);
      }
    }
    if (i + NB < NO) out[i + NB] = carry;                                         // untouched so far: row i is the first to reach it
  }
}

// a b mod l for a, b below 2^256 with a b below 2^512 (any two 8-word numbers); canonical
__device__ __forceinline__ void sg_mul_mod_order(uint32_t (&out)[8], const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint32_t p[16];
  sg_mul_words<8, 8, 16>(p, a, b);
  uint32_t q1[9], mu[9], l[8];
#pragma unroll
  for (int i = 0; i < 9; ++i) { q1[i] = p[7 + i]; mu[i] = SIG_BARRETT_MU[i]; }      // floor(p / 2^224)
#pragma unroll
  for (int i = 0; i < 8; ++i) l[i] = SIG_ORDER[i];
  uint32_t q2[18];
  sg_mul_words<9, 9, 18>(q2, q1, mu);
  uint32_t q3[8];                                                                 // floor(q2 / 2^288): the quotient or up to 2 less; its ninth word does not reach the low 256 bits' difference
#pragma unroll
  for (int i = 0; i < 8; ++i) q3[i] = q2[9 + i];
  uint32_t ql[8];
  sg_mul_words<8, 8, 8>(ql, q3, l);
  uint32_t borrow = 0;                                                            // p - q3 l is below 3 l < 2^253: exact in the low 256 bits
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)p[i] - ql[i] - borrow;
    out[i] = (uint32_t)d; borrow = (uint32_t)(d >> 32) & 1u;
  }
  ac_reduce_once(out); ac_reduce_once(out);
}

// a - b mod l; a, b below l
__device__ __forceinline__ void sg_sub_mod_order(uint32_t (&out)[8], const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)a[i] - b[i] - borrow;
    out[i] = (uint32_t)d; borrow = (uint32_t)(d >> 32) & 1u;
  }
  const uint32_t back = 0u - borrow;                                              // all ones where the difference went below 0
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)out[i] + (SIG_ORDER[i] & back) + carry;
    out[i] = (uint32_t)t; carry = (uint32_t)(t >> 32);
  }
}

// One signature.  seedw: the nonce seed's words.  key(k, w): the canonical words of the key row's part k = 0 .. 3 (sk_sig, pk_sig.x, pr_sig.x, address.x).
// refused: nonzero where the key is none.  len, byte: the message.  store(k, w): part k = 0 .. 3 of the row (challenge, response, pk_sig.x, pr_sig.x), each
// called once, at the end.  Returns the flag.
// phase(): called between the lane's phases, as signature_verify_lane's: the kernel stores a provisional flag byte there.
template <class Key, class Byte, class Store, class Phase>
__device__ __forceinline__ uint32_t signature_sign_lane(const uint32_t (&seedw)[8], Key&& key, uint32_t refused, uint32_t len, Byte&& byte, const uint32_t* K, Store&& store, Phase&& phase) {
  const bool bad = refused != 0 || len > SIG_MAX_BYTES;
  uint32_t keep = bad ? 0u : 0xffffffffu;                                         // what the lane's inputs and its row are masked with: a word of the lane's own
  ac_lane_word(keep);
  if (bad) len = 0;
  const uint32_t m = (8u * len + SIG_FIELD_BITS - 1u) / SIG_FIELD_BITS;
  uint32_t nonce[8];
  sg_nonce_of_seed(nonce, seedw);
#pragma unroll
  for (int i = 0; i < 8; ++i) nonce[i] &= keep;
  auto part = [&](uint32_t k, uint32_t (&w)[8]) { key(k, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] &= keep; };
  auto mont = [&](uint32_t k) { uint32_t w[8]; part(k, w); return f29_mul(f29_from_words(w), rk_const(K, RK_R2)); };
  phase();
  F29 grx;
  {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = nonce[i];
    Ed29 p; p.X = f29_zero(); p.Y = rk_const(K, RK_ONE); p.Z = p.Y; p.T = p.X;
    sg_add_mul_g(p, k, K);
    phase();
    grx = f29_mul(p.X, f29_pow(p.Z, K + RK_EXP_INV, RK_INV_BITS));               // Z is never 0 (the law is complete)
  }
  uint32_t ch[8];
  sg_challenge(ch, [&](uint32_t k) { return k == 0 ? grx : mont(k); }, len, m, byte, K, phase);
  phase();
  uint32_t w[8], t[8], rs[8];
  part(0, w);
  sg_mul_mod_order(t, ch, w);
  sg_sub_mod_order(rs, nonce, t);
#pragma unroll
  for (int i = 0; i < 8; ++i) { ch[i] &= keep; rs[i] &= keep; }
  store(0u, ch); store(1u, rs);
  part(1, w); store(2u, w);
  part(2, w); store(3u, w);
  return keep ? SIGN_OK : SIGN_REFUSED;
}

}  // namespace aleo_mi355x
