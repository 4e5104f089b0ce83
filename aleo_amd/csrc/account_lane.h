// account_lane.h — what ONE lane of the account kernels computes (accounts.hip launches it, one account per lane): the account of a private key's seed,
// PrivateKey::try_from(seed) -> ComputeKey -> ViewKey -> Address of snarkVM 0.14.5 console/account [UPSTREAM-RECALL] — what the reference reaches through
// wasm/src/account/private_key.rs:38-86 (PrivateKey::new, from_seed_unchecked, to_view_key, to_address) and sdk/src/account.ts:82.  Byte for byte
// records_bits.hpp's serial::account_from_seed, which is the definition and is pinned by the three accounts of tests/golden/reference_account.json.
//
//   sk_sig    the low 250 bits of Poseidon2 hash([AleoAccountSignatureSecretKey0, seed])
//   r_sig     the same over the separator of "AleoAccountSignatureRandomizer0.0" (longer than a field: reduced mod r)
//   sk_prf    the low 250 bits of Poseidon4 hash([x(sk_sig G), x(r_sig G)])            G = hash_to_curve("AleoAccountEncryptionAndSignatureScheme0")
//   view key  sk_sig + r_sig + sk_prf mod l
//   address   x(view key G)
//
// Flags: 0 derived; 3 the seed is not a canonical field element (not below r) — such a lane goes through the motions on zeros to the end and its rows are zero,
// as signature_verify_lane's malformed lanes do.
// The hashes.  Both rate-2 preimages are [AleoPoseidon2, 2 | D, seed]: a lane starts from the state after the constant first block with D added (AC_S0, one per
// separator, as SK_S0 is for serial numbers) and runs ONE width-3 permutation per hash; rate 4 from SG_S4 through psd4_permute as the signature lane does.
// The multiplications.  Three of G by a scalar below 2^252, each 63 additions from the resident 63 x 16 table (sg_add_mul_g), no doubling, in ONE loop of three
// uniform turns so that the walk over the table is in the kernel once.  pk_sig and pr_sig share one inversion (of Z1 Z2); the address costs the second.
// The address is view key G and not pk_sig + pr_sig + sk_prf G — the same point: the second form costs one addition and one cached operand more and keeps two
// points alive across the rate-4 hash (by count of products and live registers; the two were not timed against each other).
// The view key.  Three numbers below 2^250 sum to less than 3 l: eight 32-bit words with carries and two conditional subtractions of l, the words shifted and
// never indexed.
// The string.  "aleo1" + 52 symbols of five bits (the 32 canonical bytes as a bit stream, the most significant bit of each byte first, the last symbol padded
// with zeros) + the six symbols of the bech32m checksum (BIP-350) over the expanded prefix "aleo": 63 ASCII bytes, handed out one by one.
// The table: the signature lane's words as they stand (so psd4_permute, sg_entry and sg_add_mul_g serve unchanged), then the rate-2 section below.
#pragma once
#include "signature_lane.h"
#include "chacha.h"

namespace aleo_mi355x {

static constexpr uint32_t ACC_OK = 0, ACC_BAD_SEED = 3;
static constexpr uint32_t ACC_ADDRESS_CHARS = 63, ACC_MAX_PREFIX = 12;

enum : uint32_t {
  AC_E0 = (SG_WORDS + 8) / 9,
  AC_S0 = AC_E0,               // 2 x 3: the rate-2 sponge after [AleoPoseidon2, 2] with the separator of sk_sig, then of r_sig, added to its first rate element
  AC_ARK = AC_S0 + 6,          // 39 x 3
  AC_MDS = AC_ARK + 117,       // 3 x 3
  AC_ELEMS = AC_MDS + 9,
  AC_WORDS = AC_ELEMS * 9
};

// v -= l where v is not below l; v below 2^252
__device__ __forceinline__ void ac_reduce_once(uint32_t (&v)[8]) {
  const bool ge = !sg_below_order(v);
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)v[i] - (ge ? SIG_ORDER[i] : 0u) - borrow;
    v[i] = (uint32_t)d; borrow = (uint32_t)(d >> 32) & 1u;
  }
}

// byte j (a constant) of the 32 little-endian bytes held in w
__device__ __forceinline__ uint32_t ac_byte(const uint32_t (&w)[8], int j) { return j < 32 ? (w[j >> 2] >> (8 * (j & 3))) & 0xffu : 0u; }
// symbol s (a constant, 0 .. 51) of the address: bits 5 s .. 5 s + 4 of the byte stream, the most significant bit of a byte first
__device__ __forceinline__ uint32_t ac_symbol(const uint32_t (&w)[8], int s) {
  const int at = 5 * s, b = at >> 3, sh = 11 - (at & 7);
  return (((ac_byte(w, b) << 8) | ac_byte(w, b + 1)) >> sh) & 31u;
}
// the character of a five-bit symbol: "qpzry9x8gf2tvdw0s3jn54khce6mua7l", four to a word, chosen by selects (no table in memory, no indexed register)
constexpr uint32_t ac_charset_word(int q) {
  constexpr char A[33] = "qpzry9x8gf2tvdw0s3jn54khce6mua7l";
  return (uint32_t)A[4 * q] | (uint32_t)A[4 * q + 1] << 8 | (uint32_t)A[4 * q + 2] << 16 | (uint32_t)A[4 * q + 3] << 24;
}
__device__ __forceinline__ uint32_t ac_char(uint32_t v) {
  constexpr uint32_t C[8] = {ac_charset_word(0), ac_charset_word(1), ac_charset_word(2), ac_charset_word(3), ac_charset_word(4), ac_charset_word(5), ac_charset_word(6), ac_charset_word(7)};
  uint32_t word = C[0];
#pragma unroll
  for (uint32_t q = 1; q < 8; ++q) word = (v >> 2) == q ? C[q] : word;
  return (word >> (8u * (v & 3u))) & 0xffu;
}
__device__ __forceinline__ uint32_t ac_polymod_step(uint32_t chk, uint32_t v) {
  constexpr uint32_t GEN[5] = {0x3b6a57b2u, 0x26508e6du, 0x1ea119fau, 0x3d4233ddu, 0x2a1462b3u};
  const uint32_t top = chk >> 25;
  chk = ((chk & 0x1ffffffu) << 5) ^ v;
#pragma unroll
  for (int i = 0; i < 5; ++i) chk ^= (top >> i) & 1u ? GEN[i] : 0u;
  return chk;
}
// The 63 characters "aleo1…" of an address x (canonical words): put(position, character), position 0 .. 62 in order
template <class Put>
__device__ __forceinline__ void ac_address_string(const uint32_t (&w)[8], Put&& put) {
  put(0u, (uint32_t)'a'); put(1u, (uint32_t)'l'); put(2u, (uint32_t)'e'); put(3u, (uint32_t)'o'); put(4u, (uint32_t)'1');
  uint32_t chk = 1;
  constexpr uint32_t HRP[9] = {3, 3, 3, 3, 0, 1, 12, 5, 15};      // "aleo": the high bits of its characters, 0, the low five bits
#pragma unroll
  for (int i = 0; i < 9; ++i) chk = ac_polymod_step(chk, HRP[i]);
#pragma unroll
  for (int s = 0; s < 52; ++s) { const uint32_t v = ac_symbol(w, s); chk = ac_polymod_step(chk, v); put(5u + (uint32_t)s, ac_char(v)); }
#pragma unroll
  for (int i = 0; i < 6; ++i) chk = ac_polymod_step(chk, 0u);
  chk ^= 0x2bc830a3u;
#pragma unroll
  for (int i = 0; i < 6; ++i) put(57u + (uint32_t)i, ac_char((chk >> (5 * (5 - i))) & 31u));
}
// the first 64 bits of an address's symbol stream: a prefix of p symbols is its top 5 p bits
__device__ __forceinline__ void ac_stream_head(const uint32_t (&w)[8], uint32_t& hi, uint32_t& lo) {
  auto swap = [](uint32_t v) { return (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24); };
  hi = swap(w[0]); lo = swap(w[1]);
}

// Pins a value to a register of the lane's own at this point (the compiler would otherwise turn a 0 / ~0 word back into the comparison it came from and keep that
// as a wave-wide mask in scalar registers); nothing on the host, where the emulation runs the same lane.
__device__ __forceinline__ void ac_lane_word(uint32_t& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __asm__ volatile("" : "+v"(v));
#else
  (void)v;
#endif
}

struct AccountWords { uint32_t sk_sig[8], view_key[8], address[8]; };      // canonical little-endian words; zeros with flag 3

// One account.  seedw: the seed's 32 bytes as little-endian words.  Returns the flag.
// phase(): called between the lane's phases, as signature_verify_lane's: the kernel stores a provisional flag byte there, a store the table's loads may not be
// moved across, so that no phase's constants are fetched ahead and carried through another phase in scalar registers the kernel does not have.
// sink(pkx, prx): handed x(pk_sig) and x(pr_sig), Montgomery form, where the lane has them (a refused lane's are those of the seed 0: the caller masks) — the
// signing flow's key rows take them (signatures.hip k_signer_keys); the account kernels pass none.
template <class Phase, class Sink>
__device__ __forceinline__ uint32_t account_lane(const uint32_t (&seedw)[8], const uint32_t* K, AccountWords& out, Phase&& phase, Sink&& sink) {
  F29 seed = f29_from_words(seedw);
  const bool bad = !f29_below_r(seed);
  seed = f29_zero_if(bad, seed);                                                  // a refused lane goes through the motions on zeros
  uint32_t keep = bad ? 0u : 0xffffffffu;                                         // what the results are masked with at the end: a word of the lane's own,
  ac_lane_word(keep);                                                             // not a mask held in two scalar registers through every phase
  const F29 sm = f29_mul(seed, rk_const(K, RK_R2));
  // sk_sig and r_sig: one loop, so that the width-3 permutation is in the code once
  uint32_t sk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
  for (uint32_t turn = 0; turn < 2; ++turn) {
    phase();
    F29 st[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) st[i] = rk_const(K, AC_S0 + 3 * turn + i);
    st[2] = f29_add(st[2], sm);
    psd2_permute(st, K, AC_ARK, AC_MDS);
    uint32_t h[8];
    sg_hash_words(st[1], h);
#pragma unroll
    for (int i = 0; i < 8; ++i) { sk[i] = turn == 0 ? h[i] : sk[i]; rs[i] = h[i]; }
  }
  // Turn 0: pk_sig = sk_sig G.  Turn 1: pr_sig = r_sig G, the two x-coordinates from one inversion, sk_prf and the view key.  Turn 2: the address, view key G.
  uint32_t view[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  F29 pkX = f29_zero(), pkZ = pkX, ax = pkX;
#pragma unroll 1
  for (uint32_t turn = 0; turn < 3; ++turn) {
    phase();
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = turn == 0 ? sk[i] : (turn == 1 ? rs[i] : view[i]);
    Ed29 p; p.X = f29_zero(); p.Y = rk_const(K, RK_ONE); p.Z = p.Y; p.T = p.X;
    sg_add_mul_g(p, k, K);
    phase();
    if (turn == 0) { pkX = p.X; pkZ = p.Z; continue; }
    const F29 den = turn == 1 ? f29_mul(pkZ, p.Z) : p.Z;                          // Z is never 0 (the law is complete)
    const F29 inv = f29_pow(den, K + RK_EXP_INV, RK_INV_BITS);
    if (turn == 2) { ax = f29_mul(p.X, inv); continue; }
    const F29 pkx = f29_mul(pkX, f29_mul(inv, p.Z)), prx = f29_mul(p.X, f29_mul(inv, pkZ));
    sink(pkx, prx);
    F29 st[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) st[i] = rk_const(K, SG_S4 + i);
    st[1] = f29_add(st[1], pkx); st[2] = f29_add(st[2], prx);
    psd4_permute(st, K, phase);
    uint32_t prf[8];
    sg_hash_words(st[1], prf);
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t t = (uint64_t)sk[i] + rs[i] + prf[i] + carry;
      view[i] = (uint32_t)t; carry = (uint32_t)(t >> 32);
    }
    ac_reduce_once(view); ac_reduce_once(view);
  }
  f29_to_words(f29_canonical(ax), out.address);
#pragma unroll
  for (int i = 0; i < 8; ++i) { out.sk_sig[i] = sk[i] & keep; out.view_key[i] = view[i] & keep; out.address[i] &= keep; }
  return keep ? ACC_OK : ACC_BAD_SEED;
}

template <class Phase>
__device__ __forceinline__ uint32_t account_lane(const uint32_t (&seedw)[8], const uint32_t* K, AccountWords& out, Phase&& phase) {
  return account_lane(seedw, K, out, phase, [](const F29&, const F29&) {});
}

// Candidate `index` of a search under a master seed: its private key's seed is element `index` of the ChaCha20 stream (chacha.h: uniform over Fr by rejection, a
// pure function of (master, index) on host and device; the counter is 64 bits wide all the way into the block function).
__host__ __device__ inline void account_candidate_seed(uint32_t (&seedw)[8], const uint32_t (&master)[8], uint64_t index) { chacha_fr(seedw, master, index); }

}  // namespace aleo_mi355x
