// signature_lane.h — what ONE lane of the signature kernel computes (signatures.hip launches it, one signature per lane): Signature<N>::verify(address, message)
// of snarkVM 0.14.5, console/account/src/signature/verify.rs [UPSTREAM-RECALL] — what the reference reaches through wasm/src/account/signature.rs:37-48 and
// wasm/src/account/address.rs:69-71.  Byte for byte signature_host.hpp's verify_one_host, which is the definition.
//
//   signature   challenge | response | pk_sig.x | pr_sig.x, 32 bytes each, canonical little-endian                                             UNPINNED (layout)
//   g_r         response G + challenge pk_sig                       G = hash_to_curve("AleoAccountEncryptionAndSignatureScheme0"), pinned by three accounts
//   challenge'  hash_to_scalar_psd8([g_r.x, pk_sig.x, pr_sig.x, address.x, message fields ...])                                UNPINNED (order of the preimage)
//   sk_prf      hash_to_scalar_psd4([pk_sig.x, pr_sig.x]);  address' = pk_sig + pr_sig + sk_prf G                              pinned by the three accounts
//   message     its bytes as bits, little-endian within a byte, cut into fields of 252 bits, the last one short; none for no bytes         UNPINNED (packing)
//   accepted    challenge' == challenge and address'.x == address.x; hash_to_scalar keeps the low 250 bits of the hash (pinned: the accounts' sk_sig)
//
// Flags: 0 verifies; 1 does not; 3 is no signature — a scalar not below the group order l, an x not below r, an x with no point in the prime-order subgroup, or a
// message of more than SIG_MAX_FIELDS fields (the cap: UNPINNED).  A lane with flag 3 goes through the motions on zeros to the end.
//
// Points from x.  As the record nonce's (records_lane.h): w = 1 - d x^2, s^2 = (1 + x^2) w, the point (x w : s : w), one fixed-schedule square root.  Of the two
// points (x, +-y) upstream takes the one in the subgroup.  The group is cyclic of order 4 l, so "in the subgroup" is "in 4 E", which the reduced Tate pairing with a
// point T4 of order four decides: with (u, v) = ((1 + y) / (1 - y), u / x) on the Montgomery form and t the tangent at T4 = (1, v4) (its slope is v4 too), the
// function t^2 / u has the divisor 4 (T4) - 4 (O), and psi(P) = (t^2 / u)(P)^((r - 1) / 4) is a constant kappa on 4 E, -kappa on the other half of 2 E — where
// (x, -y) = T2 - P is the point wanted — and +-i kappa on the rest, where neither point will do.  Denominators are cleared by fourth powers:
// psi = ((n d)^2 (w - s) (w + s)^3)^((r - 1) / 4) with n = (w + s) - v4 x (w - s) - 2 v4 x s, d = x (w - s): one exponentiation of 251 bits where l P costs 251
// doublings.  kappa is psi(G), computed by the host with the table; x = 0 (psi = 0) is the identity and is taken as such.  tests/cpp/signature_lane_emul.cpp
// checks the choice against l P on the host.
// response G and sk_prf G.  One table of G: 63 windows of 4 bits x 16 cached affine entries (y - x, y + x, 2 d x y; entry 0 the identity), 108 KB behind the
// scan's constants, resident per device; 63 additions, no doubling, the lookups diverge per lane and are served by L2 as the commitment table's are.
// challenge pk_sig.  Scalar and point are the lane's own: a double-and-add over the challenge's 250 bits, entirely in registers — the sum is always computed and
// selected, so a wave's lanes stay in step; the scalar's words are shifted, never indexed.  (Signed 4-bit windows over a per-lane table in LDS: DESIGN §12.)
// Only the challenge's low 250 bits are walked: one of 251 bits (below l still) cannot equal a hash cut to 250 and fails on the host path too, whatever g_r is.
// The hashes.  Rate 4 in the plain round form from the state after its constant first block (SG_S4); rate 8 through psd_permute (records_lane.h), its first
// block [AleoPoseidon8, 4 + m, 0 x 6] included since it holds the message's length.  The message is read from global memory field by field, eight per
// permutation, straight into the sponge: there is no per-lane buffer and no limit but the cap.
#pragma once
#include "records_serial_lane.h"
#include "chacha.h"

namespace aleo_mi355x {

static constexpr uint32_t SIG_OK = 0, SIG_INVALID = 1, SIG_MALFORMED = 3;
static constexpr uint32_t SIG_FIELD_BITS = 252;
static constexpr uint32_t SIG_MAX_FIELDS = (128u * 1024u * 8u) / SIG_FIELD_BITS;      // MAX_DATA_SIZE_IN_FIELDS: 128 KiB of data bits / 252 = 4161 [UPSTREAM-RECALL, UNPINNED]
static constexpr uint32_t SIG_MAX_BYTES = SIG_MAX_FIELDS * SIG_FIELD_BITS / 8;         // 131071: the longest message of at most that many fields
static constexpr uint32_t SIG_WINDOWS = 63, SIG_SCALAR_BITS = 250, SIG_QUART_BITS = 251;
// l as eight 32-bit words, least significant first
static constexpr uint32_t SIG_ORDER[8] = {0xc33fd9ffu, 0xb95aee9au, 0xc43c8afeu, 0x5293a3afu, 0x970dec00u, 0x982d1347u, 0xa68b2955u, 0x04aad957u};

// The lane's constants: the scan's first, unchanged (K serves rk_const, f29_pow, f29_sqrt_fixed and psd_permute as it stands), then in units of one element
enum : uint32_t {
  SG_E0 = (RK_WORDS + 8) / 9,
  SG_TWO = SG_E0,                          // 2: the 2 Z of every table entry
  SG_V4 = SG_TWO + 1, SG_V4X2,             // v4 and 2 v4: the tangent at T4
  SG_KIN = SG_V4 + 2, SG_KOUT,             // kappa and -kappa as plain numbers
  SG_DOM8 = SG_KIN + 2,                    // the domain separator "AleoPoseidon8"
  SG_S4 = SG_DOM8 + 1,                     // 5: the rate-4 sponge after [AleoPoseidon4, 2, 0, 0]
  SG_ARK4 = SG_S4 + 5,                     // 39 x 5
  SG_MDS4 = SG_ARK4 + 195,                 // 5 x 5
  SG_G = SG_MDS4 + 25,                     // 63 x 16 x 3
  SG_ELEMS = SG_G + SIG_WINDOWS * 16 * 3,
  SG_EXP_QUART = SG_ELEMS * 9,             // 8 words: (r - 1) / 4
  SG_WORDS = SG_EXP_QUART + 8
};

__device__ __forceinline__ bool sg_below_order(const uint32_t (&w)[8]) {
  bool ge = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) ge = w[i] > SIG_ORDER[i] || (w[i] == SIG_ORDER[i] && ge);
  return !ge;
}

// One width-5 permutation, plain form: 4 full rounds, 31 partial, 4 full; every element of the result tidied.  round(): signature_verify_lane's phase(), once a
// round — the matrix is the same in every round, and its 225 words are not to be fetched before the loop and held.
template <class Round>
__device__ __forceinline__ void psd4_permute(F29 (&s)[5], const uint32_t* K, Round&& round) {
  for (int r = 0; r < 39; ++r) {
    round();
    const bool full = r < 4 || r >= 35;
    F29 t[5];
    t[0] = psd_pow17(f29_add(s[0], rk_const(K, SG_ARK4 + 5 * r)));
#pragma unroll
    for (int i = 1; i < 5; ++i) {
      t[i] = f29_add(s[i], rk_const(K, SG_ARK4 + 5 * r + i));
      if (full) t[i] = psd_pow17(t[i]); else f29_normalise(t[i]);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      F29 acc = f29_mul(t[0], rk_const(K, SG_MDS4 + 5 * i));
#pragma unroll
      for (int j = 1; j < 5; ++j) {
        acc = f29_add(acc, f29_mul(t[j], rk_const(K, SG_MDS4 + 5 * i + j)));
        if (j == 3) f29_normalise(acc);
      }
      f29_tidy(acc);
      s[i] = acc;
    }
  }
}

// The point of the prime-order subgroup with the x-coordinate nx (canonical limbs), as (x w : +-s : w).  bad (a word of the lane's own, not a mask in scalar registers): set when there is none.
__device__ __forceinline__ Ed29 sg_point_from_x(const F29& nx, uint32_t& bad, const uint32_t* __restrict__ K) {
  const F29 one = rk_const(K, RK_ONE);
  const F29 x = f29_mul(nx, rk_const(K, RK_R2));
  const F29 xx = f29_sqr(x);
  F29 w = f29_sub_pad(one, f29_mul(xx, rk_const(K, RK_D))); f29_tidy(w);        // 1 - d x^2 (never 0: d is not a square)
  const F29 a = f29_mul(f29_add(one, xx), w);
  F29 s = f29_sqrt_fixed(a, K);
  bad |= !f29_same_limbs(f29_canonical(f29_sqr(s)), f29_canonical(a));            // x is not on the curve
  const bool x0 = f29_is_zero_limbs(nx);
  s = f29_select(x0, w, s);                                                       // x = 0: the identity (0 : w : w), not T2
  F29 nu = f29_add(w, s); f29_tidy(nu);
  F29 du = f29_sub_pad(w, s); f29_tidy(du);
  const F29 xs = f29_mul(x, s), dl = f29_mul(x, du);
  F29 t = f29_add(f29_mul(dl, rk_const(K, SG_V4)), f29_mul(xs, rk_const(K, SG_V4X2))); f29_tidy(t);
  F29 nl = f29_sub_pad(nu, t); f29_tidy(nl);
  const F29 q = f29_sqr(f29_mul(nl, dl));
  const F29 arg = f29_mul(f29_mul(q, du), f29_mul(f29_sqr(nu), nu));
  const F29 psi = f29_canonical(f29_pow(arg, K + SG_EXP_QUART, SIG_QUART_BITS));
  const bool in = f29_same_limbs(psi, rk_const(K, SG_KIN)), out = f29_same_limbs(psi, rk_const(K, SG_KOUT));
  bad |= !(in || out || x0);
  Ed29 p;
  p.X = f29_mul(x, w); p.Z = w; p.Y = s; p.T = xs;
  if (out) { p.Y = f29_neg_tidy(s); p.T = f29_neg_tidy(xs); }                     // (x, -y)
  return p;
}

__device__ __forceinline__ Ed29Cached sg_entry(const uint32_t* __restrict__ K, uint32_t window, uint32_t digit) {
  const uint32_t first = SG_G + 3u * (16u * window + digit);
  Ed29Cached c; c.ym = rk_const(K, first); c.yp = rk_const(K, first + 1); c.k = rk_const(K, first + 2); c.z2 = rk_const(K, SG_TWO);
  return c;
}
// p += k G for the scalar in k's words (below 2^252), which are used up
__device__ __forceinline__ void sg_add_mul_g(Ed29& p, uint32_t (&k)[8], const uint32_t* __restrict__ K) {
  for (uint32_t w = 0; w < SIG_WINDOWS; ++w) {
    ed29_add(p, sg_entry(K, w, k[0] & 15u), false);
#pragma unroll
    for (int q = 0; q < 7; ++q) k[q] = (k[q] >> 4) | (k[q + 1] << 28);            // the words move down: no lane indexes its registers
    k[7] >>= 4;
  }
}

// Field j of a message of `len` bytes (byte q through byte(q), q < len only): bits 252 j .. 252 j + 251 of the byte stream, as canonical words
template <class Byte>
__device__ __forceinline__ void sg_message_field(uint32_t j, uint32_t len, Byte&& byte, uint32_t (&w)[8]) {
  const uint32_t first = 31u * j + (j >> 1), sh = 4u * (j & 1u);
  const uint32_t last = len - 1u;                                                 // len > 0: the message has a field
  auto at = [&](uint32_t q) -> uint32_t { const uint32_t v = byte(q < last ? q : last); return q < len ? v : 0u; };      // the load is unconditional: a select, no branch
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = at(first + 4 * k) | at(first + 4 * k + 1) << 8 | at(first + 4 * k + 2) << 16 | at(first + 4 * k + 3) << 24;
  if (sh) {
    const uint32_t top = at(first + 32);
#pragma unroll
    for (int k = 0; k < 7; ++k) w[k] = (w[k] >> 4) | (w[k + 1] << 28);
    w[7] = (w[7] >> 4) | (top << 28);
  }
  w[7] &= 0x0fffffffu;
}

__device__ __forceinline__ void sg_hash_words(const F29& h, uint32_t (&w)[8]) {      // hash_to_scalar: the low 250 bits of the hash
  f29_to_words(f29_canonical(h), w);
  w[7] &= (1u << (SIG_SCALAR_BITS - 224)) - 1u;
}

// The challenge of a signature: hash_to_scalar_psd8 over [AleoPoseidon8, 4 + m, 0 x 6 | g_r.x, pk_sig.x, pr_sig.x, address.x | the message's m fields], eight to
// a permutation, the first block included.  head(k), k = 0 .. 3: the four elements before the message, Montgomery form, asked for once each when block 1 is
// built — the verifying and the signing lane (signature_sign_lane.h) both call this.
template <class Head, class Byte, class Phase>
__device__ __forceinline__ void sg_challenge(uint32_t (&out)[8], Head&& head, uint32_t len, uint32_t m, Byte&& byte, const uint32_t* K, Phase&& phase) {
  F29 st[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) st[i] = f29_zero();
  const uint32_t blocks = (12u + m + 7u) / 8u;
  for (uint32_t b = 0; b < blocks; ++b) {
    phase();
    if (b == 0) {
      const F29 count = f29_small(4u + m);
      st[1] = rk_const(K, SG_DOM8); st[2] = f29_mul(count, rk_const(K, RK_R2));
    } else {
      uint32_t j = 8u * b - 12u;                                                  // the field that st[1] takes; the four elements before field 0 in block 1
      if (b == 1) {
        st[1] = f29_add(st[1], head(0));
        st[2] = f29_add(st[2], head(1)); st[3] = f29_add(st[3], head(2)); st[4] = f29_add(st[4], head(3));
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if ((b > 1 || i >= 4) && j + (uint32_t)i < m) {
          uint32_t w[8];
          sg_message_field(j + (uint32_t)i, len, byte, w);
          st[1 + i] = f29_add(st[1 + i], f29_mul(f29_from_words(w), rk_const(K, RK_R2)));
        }
      }
    }
    psd_permute(st, K);
  }
  sg_hash_words(st[1], out);
}

// The nonce of a seed, on the host and in the signing lane alike: the ChaCha20 stream under the seed (counter 0, 1, ..., nonce word 0), two candidates of 32 bytes
// to a block, the low 251 bits of each; the first below l (rejection: uniform; l / 2^251 = 0.583 of the candidates pass, and the loop ends with probability 1 as
// chacha_fr's does).
__host__ __device__ inline void sg_nonce_of_seed(uint32_t (&out)[8], const uint32_t (&seedw)[8]) {
  const uint32_t order[8] = {0xc33fd9ffu, 0xb95aee9au, 0xc43c8afeu, 0x5293a3afu, 0x970dec00u, 0x982d1347u, 0xa68b2955u, 0x04aad957u};      // SIG_ORDER, for both compilers
  for (uint64_t counter = 0;; ++counter) {
    uint32_t blk[16]; chacha20_block(blk, seedw, counter, 0);
    for (int h = 0; h < 2; ++h) {
      uint32_t* c = blk + 8 * h; c[7] &= 0x07ffffffu;     // low 251 bits
      bool lt = false;
      for (int i = 7; i >= 0; --i) { if (c[i] != order[i]) { lt = c[i] < order[i]; break; } }
      if (lt) { for (int i = 0; i < 8; ++i) out[i] = c[i]; return; }
    }
  }
}

// One signature.  load(k, w): the canonical words of the signature's part k = 0 .. 3 (challenge, response, pk_sig.x, pr_sig.x) and, k = 4, of the address x;
// len, byte: the message.  Returns the flag.
// phase(): called between the lane's phases.  The kernel stores a provisional flag byte there, a store the table's loads may not be moved across: without it the
// compiler fetches every phase's constants once, at the top, and carries them through the ladder in scalar registers it does not have.
template <class Load, class Byte, class Phase>
__device__ __forceinline__ uint32_t signature_verify_lane(Load&& load, uint32_t len, Byte&& byte, const uint32_t* K, Phase&& phase) {
  uint32_t cw[8], w8[8];
  load(0, cw);
  uint32_t bad = !sg_below_order(cw) || len > SIG_MAX_BYTES;
  load(1, w8); bad |= !sg_below_order(w8);
  load(2, w8); bad |= !f29_below_r(f29_from_words(w8));
  load(3, w8); bad |= !f29_below_r(f29_from_words(w8));
  load(4, w8); bad |= !f29_below_r(f29_from_words(w8));
  auto part = [&](uint32_t k) { uint32_t w[8]; load(k, w); return f29_zero_if(bad, f29_from_words(w)); };      // a malformed lane goes through the motions on zeros
  if (bad) len = 0;
  const uint32_t m = (8u * len + SIG_FIELD_BITS - 1u) / SIG_FIELD_BITS;
  auto mont = [&](uint32_t k, uint32_t r2) { return f29_mul(part(k), rk_const(K, r2)); };      // part k in Montgomery form

  // sk_prf
  uint32_t prf[8];
  {
    F29 st[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) st[i] = rk_const(K, SG_S4 + i);
    st[1] = f29_add(st[1], mont(2, RK_R2)); st[2] = f29_add(st[2], mont(3, RK_R2));
    psd4_permute(st, K, phase);
    sg_hash_words(st[1], prf);
  }
  // Turn 0: g_r = challenge pk_sig + response G, of which x is kept.  Turn 1: the address of the compute key, pr_sig + pk_sig + sk_prf G, compared projectively.
  // One loop, so that the point from x and the walk over G's table are in the code once; the turn is uniform.
  Ed29Cached pk;
  F29 grx;
  bool address_ok = false;
#pragma unroll 1
  for (uint32_t turn = 0; turn < 2; ++turn) {
    phase();
    Ed29 p = sg_point_from_x(part(2 + turn), bad, K);
    phase();
    uint32_t k[8];
    if (turn == 0) {
      pk = ed29_cache(p, rk_const(K, RK_D2));
      uint32_t c[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) c[i] = bad ? 0u : cw[i];
      p.X = f29_zero(); p.Y = rk_const(K, RK_ONE); p.Z = p.Y; p.T = p.X;
#pragma unroll
      for (int i = 7; i > 0; --i) c[i] = (c[i] << 6) | (c[i - 1] >> 26);          // bit 249 to the top
      c[0] <<= 6;
      for (uint32_t i = 0; i < SIG_SCALAR_BITS; ++i) {
        const bool bit = c[7] >> 31;
#pragma unroll
        for (int q = 7; q > 0; --q) c[q] = (c[q] << 1) | (c[q - 1] >> 31);
        c[0] <<= 1;
        ed29_dbl(p, true);
        Ed29 t = p;
        ed29_add(t, pk, false);
        p.X = f29_select(bit, t.X, p.X); p.Y = f29_select(bit, t.Y, p.Y); p.Z = f29_select(bit, t.Z, p.Z); p.T = f29_select(bit, t.T, p.T);
      }
      load(1, k);
#pragma unroll
      for (int i = 0; i < 8; ++i) k[i] = bad ? 0u : k[i];
    } else {
      ed29_add(p, pk, false);
#pragma unroll
      for (int i = 0; i < 8; ++i) k[i] = prf[i];
    }
    phase();
    sg_add_mul_g(p, k, K);
    phase();
    if (turn == 0) grx = f29_mul(p.X, f29_pow(p.Z, K + RK_EXP_INV, RK_INV_BITS));  // Z is never 0 (the law is complete)
    else address_ok = f29_same_limbs(f29_canonical(p.X), f29_canonical(f29_mul(p.Z, mont(4, RK_R2))));
  }
  uint32_t got[8];
  sg_challenge(got, [&](uint32_t k) { return k == 0 ? grx : mont(1 + k, RK_R2); }, len, m, byte, K, phase);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= got[i] ^ cw[i];
  return bad ? SIG_MALFORMED : (diff == 0 && address_ok ? SIG_OK : SIG_INVALID);
}

}  // namespace aleo_mi355x
