// key_ciphertext_lane.h — what ONE lane of the private-key-ciphertext kernel computes (key_ciphertexts.hip launches it, one (ciphertext string, secret) pair per
// lane): the seed of the private key a "ciphertext1…" string holds under a secret — Encryptor::decrypt_private_key_with_secret of the reference
// (rust/src/account/encryptor.rs:45-67, reached through wasm/src/account/private_key_ciphertext.rs:56-61 and private_key.rs:124-130) over snarkVM 0.14.5's
// Ciphertext::decrypt_symmetric and Plaintext::from_fields [UPSTREAM-RECALL].  Byte for byte key_ciphertext_host.hpp's open_one_host, which is the definition and
// is pinned, both ways, by the reference's own known answer (private_key_ciphertext.rs:115-128; tests/golden/reference_account.json "ciphertext_kat").
//
//   string      bech32m (BIP-350) under "ciphertext": u16 little-endian count | count x 32 bytes, each a canonical little-endian field element; the payload is
//               exactly 2 + 32 count bytes                                                                      UNPINNED: what upstream does with trailing bytes
//   s           the secret's bytes, little-endian, mod r (Field::new_domain_separator)                           UNPINNED: a secret of more than 31 bytes
//   rnd         hash_many_psd8([sep("AleoSymmetricEncryption0"), s], count);  p_i = c_i - rnd_i
//   plaintext   the low 252 bits of every p_i, one after another; bit 252 of a p_i is ignored                   UNPINNED: upstream's view of that bit
//   accepted    count == 3 and the 756 bits are the ONE layout Encryptor::encrypt_field writes (KC_* below): a struct of the two members "key" and "nonce", in that
//               order, each a field literal of 253 bits below r, the terminus bit at 680, zeros behind it.  A ciphertext that holds the two members in some other
//               valid Plaintext shape (another order, other widths of padding) is REFUSED here; upstream's parser would accept it.
//   seed        key / hash_psd2([sep("private_key"), nonce, s]);  a zero blinding does not decrypt
//
// Flags: 0 opened; 1 a ciphertext that does not decrypt under this secret (count != 3 included); 3 no ciphertext string — a character outside the alphabet, the
// checksum, the prefix, the payload's length, a field element not below r, or more than RS_MAX_CHARS characters.  A lane with a flag goes through the motions on
// zeros to the end; its seed is 32 x 0xff, which k_accounts_derive refuses, so that its account rows are zero without that kernel being told.
//
// The string.  The two passes of records_strings_lane.h: every symbol folded into the checksum from the state after the expanded prefix, then the count and the
// fields read through the symbols that cover them (records_symbols_lane.h) — no buffer.  kc_decode is plain C++ and runs on the host path as it stands.
// The secret.  At most 31 bytes are a field element as they lie; the host reduces a longer one before the upload and hands the lane its 32 canonical bytes (a
// device secret of 32 bytes is that, and nothing else is: the reduction in the lane would be a loop of products for what no reference secret needs).
// The randomizers.  The preimage [AleoPoseidon8, 2, 0 x 6 | domain, s] is the record scan's with s for the record view key: the lane starts from the same state
// after the constant first block (RK_S0) and runs ONE width-9 permutation, all of whose first three rate elements it keeps.
// The layout.  Three subtractions, the 756 bits as 24 words by constant shifts, one masked comparison per word against a compile-time template, `key` and `nonce`
// cut out by shifts across the field boundaries and compared with r: no walk over bits, no loop that depends on the lane's data.
// The blinding.  The preimage [AleoPoseidon2, 3 | sep("private_key"), nonce | s] is three width-3 permutations, the first of them constant: the lane starts from
// its state with the separator added (KC_S0) and runs two, in one loop so that the permutation is in the kernel once; one inversion, one product.
// The table: the account lane's words as they stand (so one resident table serves this kernel and the k_accounts_derive launched behind it), then KC_S0.
#pragma once
#include "account_lane.h"
#include "records_strings_lane.h"

namespace aleo_mi355x {

static constexpr uint32_t KC_OPENED = 0, KC_NOT_DECRYPTED = 1, KC_NO_CIPHERTEXT = 3;
static constexpr uint32_t KC_PREFIX_CHARS = 11;                                      // "ciphertext1"
static constexpr uint32_t KC_PREFIX_STATE = rs_polymod_prefix("ciphertext");
static constexpr uint32_t KC_FIELDS = 3, KC_CHARS = 174;                             // of a private key's ciphertext: 11 + ceil(8 x 98 / 5) + 6
static constexpr uint32_t KC_MAX_DEVICE_SECRET = 32;                                 // bytes of a secret as the kernel sees it: up to 31 as they are, 32 a reduced one

enum : uint32_t {
  KC_E0 = AC_ELEMS,
  KC_S0 = KC_E0,               // 3: the rate-2 sponge after [AleoPoseidon2, 3] with the separator of "private_key" added to its first rate element
  KC_ELEMS = KC_S0 + 3,
  KC_WORDS = KC_ELEMS * 9
};

// ---- the one accepted plaintext, as 24 words of bits (bit b of the plaintext is bit b % 32 of word b / 32) -----------------------------------------------------------
static constexpr uint32_t KC_KEY_AT = 84, KC_NONCE_AT = 427, KC_VALUE_BITS = 253, KC_TERMINUS_AT = 680, KC_PLAIN_BITS = 756, KC_DATA_BITS = 252;
struct KcTemplate { uint32_t want[24], mask[24]; };
constexpr KcTemplate kc_template() {
  KcTemplate t{};
  for (int i = 0; i < 24; ++i) { t.want[i] = 0; t.mask[i] = 0xffffffffu; }
  uint32_t at = 0;
  auto put = [&](uint64_t v, uint32_t bits) { for (uint32_t b = 0; b < bits; ++b, ++at) if ((v >> b) & 1u) t.want[at >> 5] |= 1u << (at & 31u); };
  auto hole = [&](uint32_t bits) { for (uint32_t b = 0; b < bits; ++b, ++at) t.mask[at >> 5] &= ~(1u << (at & 31u)); };
  put(2, 2); put(2, 8);                                                               // a struct (bits 0, 1) of two members
  put(24, 8); put((uint64_t)'k' | (uint64_t)'e' << 8 | (uint64_t)'y' << 16, 24);
  put(279, 16); put(0, 2); put(2, 8); put(253, 16);                                   // a literal (bits 0, 0) of type field, 253 bits
  hole(KC_VALUE_BITS);
  put(40, 8); put((uint64_t)'n' | (uint64_t)'o' << 8 | (uint64_t)'n' << 16 | (uint64_t)'c' << 24 | (uint64_t)'e' << 32, 40);
  put(279, 16); put(0, 2); put(2, 8); put(253, 16);
  hole(KC_VALUE_BITS);
  put(1, 1);                                                                          // the terminus; zeros to the end of the third field and of the words
  return t;
}
static_assert(kc_template().mask[2] == 0x000fffffu && (kc_template().want[21] >> 8 & 1u) == 1u, "the key begins at bit 84, the terminus is bit 680");

// r, in little-endian words: is v below it?
__host__ __device__ __forceinline__ bool kc_below_r(const uint32_t (&v)[8]) {
  bool ge = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) ge = v[i] > RS_FR_WORDS[i] || (v[i] == RS_FR_WORDS[i] && ge);
  return !ge;
}

// The 24 words of the low 252 bits of three numbers, one after another
__host__ __device__ __forceinline__ void kc_stream(const uint32_t (&p)[3][8], uint32_t (&s)[24]) {
#pragma unroll
  for (int i = 0; i < 24; ++i) s[i] = 0;
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const int at = (int)KC_DATA_BITS * f, w0 = at >> 5, sh = at & 31;                 // 0, 252, 504: constants once the loop is unrolled
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint32_t v = q == 7 ? p[f][7] & 0x0fffffffu : p[f][q];
      s[w0 + q] |= v << sh;
      if (sh && w0 + q + 1 < 24) s[w0 + q + 1] |= v >> (32 - sh);
    }
  }
}
// 253 bits of the stream from bit `at` (a constant, not a multiple of 32) on, as eight words
__host__ __device__ __forceinline__ void kc_cut(const uint32_t (&s)[24], uint32_t at, uint32_t (&v)[8]) {
  const uint32_t w0 = at >> 5, sh = at & 31u;
#pragma unroll
  for (uint32_t q = 0; q < 8; ++q) v[q] = (s[w0 + q] >> sh) | (s[w0 + q + 1] << (32u - sh));
  v[7] &= (1u << (KC_VALUE_BITS - 224u)) - 1u;
}
// The layout check: whether the three plain numbers are the accepted plaintext, and its `key` and `nonce` (anything where they are not)
__host__ __device__ __forceinline__ bool kc_layout(const uint32_t (&p)[3][8], uint32_t (&key)[8], uint32_t (&nonce)[8]) {
  constexpr KcTemplate T = kc_template();
  uint32_t s[24];
  kc_stream(p, s);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 24; ++i) diff |= (s[i] & T.mask[i]) ^ T.want[i];
  kc_cut(s, KC_KEY_AT, key); kc_cut(s, KC_NONCE_AT, nonce);
  return diff == 0 && kc_below_r(key) && kc_below_r(nonce);
}
// ... and its inverse, for the encryption: the three numbers of 252 bits that hold `key` and `nonce` (each below 2^253)
__host__ __device__ __forceinline__ void kc_plain_fields(const uint32_t (&key)[8], const uint32_t (&nonce)[8], uint32_t (&p)[3][8]) {
  constexpr KcTemplate T = kc_template();
  uint32_t s[25];
#pragma unroll
  for (int i = 0; i < 24; ++i) s[i] = T.want[i];
  s[24] = 0;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const uint32_t at = m ? KC_NONCE_AT : KC_KEY_AT, w0 = at >> 5, sh = at & 31u;
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) { const uint32_t v = m ? nonce[q] : key[q]; s[w0 + q] |= v << sh; s[w0 + q + 1] |= v >> (32u - sh); }
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const uint32_t at = KC_DATA_BITS * f, w0 = at >> 5, sh = at & 31u;
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) p[f][q] = sh ? (s[w0 + q] >> sh) | (s[w0 + q + 1] << (32u - sh)) : s[w0 + q];
    p[f][7] &= 0x0fffffffu;
  }
}

// ---- the string ------------------------------------------------------------------------------------------------------------------------------------------------------
// One string of `len` characters, character i through ch(i) (0 <= i < len, asked for in any order and more than once).  Returns KC_OPENED with the canonical words
// of the three field elements, KC_NOT_DECRYPTED for a well-formed ciphertext of another count, KC_NO_CIPHERTEXT for anything else; zeros in c with a flag.
template <class LoadChar>
__host__ __device__ __forceinline__ uint32_t kc_decode(LoadChar&& ch, uint32_t len, uint32_t (&c)[3][8]) {
  constexpr RsSymbols T = rs_symbols();
#pragma unroll
  for (int f = 0; f < 3; ++f) {
#pragma unroll
    for (int q = 0; q < 8; ++q) c[f][q] = 0;
  }
  if (len < KC_PREFIX_CHARS + RS_CHECKSUM_SYMBOLS || len > RS_MAX_CHARS) return KC_NO_CIPHERTEXT;      // the one early way out: what follows reads 17 characters at least
  // From here on one flat run: what is wrong is noted in `ok` and nothing is read that the string does not hold (a lane's early ways out are a wave's nested masks)
  const char prefix[KC_PREFIX_CHARS + 1] = "ciphertext1";
  bool ok = true;
  for (uint32_t i = 0; i < KC_PREFIX_CHARS; ++i) ok = ok && (uint8_t)ch(i) == (uint8_t)prefix[i];
  const uint32_t n_sym = len - KC_PREFIX_CHARS, D = n_sym - RS_CHECKSUM_SYMBOLS;
  auto sym = [&](uint32_t k) { return (uint32_t)T.of[(uint8_t)ch(KC_PREFIX_CHARS + k) & 127u] & 31u; };      // k < n_sym; the symbol of a string whose characters pass
  uint32_t chk = KC_PREFIX_STATE;
  for (uint32_t k = 0; k < n_sym; ++k) {
    const uint8_t ch_k = (uint8_t)ch(KC_PREFIX_CHARS + k);
    const int32_t s = ch_k < 128 ? T.of[ch_k] : -1;
    ok = ok && s >= 0;
    chk = rs_polymod_step(chk, (uint32_t)s & 31u);
  }
  ok = ok && chk == RS_BECH32M;
  const uint32_t left = (5u * D) & 7u, nb = (5u * D) >> 3;      // D <= 2^20: no overflow
  ok = ok && left < 5 && (sym(D ? D - 1 : 0) & ((1u << left) - 1u)) == 0;
  const uint32_t count = rs_byte_at(sym, 0) | (rs_byte_at(sym, 1) << 8);      // symbols 0 .. 3: there are six at least
  ok = ok && nb == 2u + 32u * count;                             // count < 2^16: no overflow; with it every field's symbols are data symbols
  const uint32_t fields = ok ? count : 0u;
  for (uint32_t f = 0; f < fields; ++f) {
    uint32_t w[8];
    ok = rs_field_at(sym, 2u + 32u * f, w) && ok;
#pragma unroll
    for (int q = 0; q < 8; ++q) { c[0][q] = f == 0 ? w[q] : c[0][q]; c[1][q] = f == 1 ? w[q] : c[1][q]; c[2][q] = f == 2 ? w[q] : c[2][q]; }
  }
  const uint32_t flag = !ok ? KC_NO_CIPHERTEXT : (count == KC_FIELDS ? KC_OPENED : KC_NOT_DECRYPTED);
#pragma unroll
  for (int f = 0; f < 3; ++f) {
#pragma unroll
    for (int q = 0; q < 8; ++q) c[f][q] = flag ? 0u : c[f][q];
  }
  return flag;
}

// The field element of a secret as the kernel is handed it: `len` <= 31 bytes as they lie, or the 32 canonical bytes of a reduced one; byte j through byte(j)
template <class Byte>
__host__ __device__ __forceinline__ void kc_secret_words(Byte&& byte, uint32_t len, uint32_t (&w)[8]) {
  const uint32_t last = len ? len - 1u : 0u;
  auto at = [&](uint32_t q) -> uint32_t { const uint32_t v = len ? (uint32_t)(uint8_t)byte(q < last ? q : last) : 0u; return q < len ? v : 0u; };      // the load is unconditional
  for (uint32_t k = 0; k < 8; ++k) w[k] = at(4 * k) | at(4 * k + 1) << 8 | at(4 * k + 2) << 16 | at(4 * k + 3) << 24;
}

// One pair, after kc_decode.  status: what kc_decode returned; c: its three fields; sw: the secret's field element (canonical words).  Returns the flag and the
// seed's canonical words, 0xffffffff x 8 with a flag.  phase(): called between the lane's phases, as account_lane's.
template <class Phase>
__device__ __forceinline__ uint32_t key_ciphertext_lane(uint32_t status, const uint32_t (&c)[3][8], const uint32_t (&sw)[8], const uint32_t* K, uint32_t (&seed)[8], Phase&& phase) {
  uint32_t bad = status;
  const F29 sm = f29_mul(f29_from_words(sw), rk_const(K, RK_R2));
  uint32_t p[3][8];
  {
    F29 st[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) st[i] = rk_const(K, RK_S0 + i);
    st[2] = f29_add(st[2], sm);
    psd_permute(st, K);
#pragma unroll
    for (int f = 0; f < 3; ++f) f29_to_words(f29_canonical(f29_sub_pad(f29_mul(f29_from_words(c[f]), rk_const(K, RK_R2)), st[1 + f])), p[f]);
  }
  phase();
  uint32_t key[8], nonce[8];
  bad |= kc_layout(p, key, nonce) ? 0u : KC_NOT_DECRYPTED;
#pragma unroll
  for (int i = 0; i < 8; ++i) { key[i] = bad ? 0u : key[i]; nonce[i] = bad ? 0u : nonce[i]; }
  // the blinding: [.. | private_key, nonce | s]: two turns of one loop
  F29 st[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) st[i] = rk_const(K, KC_S0 + i);
  const F29 nm = f29_mul(f29_from_words(nonce), rk_const(K, RK_R2));
#pragma unroll 1
  for (uint32_t turn = 0; turn < 2; ++turn) {
    phase();
    if (turn == 0) st[2] = f29_add(st[2], nm); else st[1] = f29_add(st[1], sm);
    psd2_permute(st, K, AC_ARK, AC_MDS);
  }
  phase();
  bad |= f29_is_zero_limbs(f29_canonical(st[1])) ? KC_NOT_DECRYPTED : 0u;
  const F29 inv = f29_pow(st[1], K + RK_EXP_INV, RK_INV_BITS);                      // of 0: 0, and the lane is flagged
  f29_to_words(f29_canonical(f29_mul(f29_mul(f29_from_words(key), rk_const(K, RK_R2)), inv)), seed);
#pragma unroll
  for (int i = 0; i < 8; ++i) seed[i] = bad ? 0xffffffffu : seed[i];
  return bad == 0 ? KC_OPENED : (bad & 2u ? KC_NO_CIPHERTEXT : KC_NOT_DECRYPTED);      // bad: 0, 1 or 3
}

}  // namespace aleo_mi355x
