// key_ciphertext_host.hpp — private key ciphertexts on the host: the reference's PrivateKeyCiphertext (wasm/src/account/private_key_ciphertext.rs:39-73
// encryptPrivateKey, decryptToPrivateKey; wasm/src/account/private_key.rs:102-130 newEncrypted, toCiphertext, fromPrivateKeyCiphertext), whose algorithm is
// rust/src/account/encryptor.rs:26-67 over snarkVM 0.14.5's Plaintext / Ciphertext [UPSTREAM-RECALL].  Plain C++ (no HIP, touches no device) over account_host.hpp
// and poseidon.hpp.  open_one_host is the DEFINITION of what a (ciphertext, secret) pair opens to; the lane (key_ciphertext_lane.h) computes the same bytes, and
// both walk the string and check the layout with the same functions (kc_decode, kc_layout).
//
// Pinned by data the reference holds (private_key_ciphertext.rs:115-128: a private key, its secret, the ciphertext and a corrupted copy of it, in
// tests/golden/reference_account.json "ciphertext_kat"): decryption, and encryption under the nonce recovered from that ciphertext, byte for byte.
//   UNPINNED  a secret of more than 31 bytes (reduced mod r; the reference's has 10); trailing payload bytes (refused); bit 252 of a decrypted field (ignored)
//   REFUSED though upstream accepts it: a ciphertext whose plaintext holds `key` and `nonce` in any valid Plaintext shape other than the one
//             Encryptor::encrypt_field writes (key_ciphertext_lane.h KC_*).
#pragma once
#include "account_host.hpp"
#include "key_ciphertext_lane.h"
#include <string>

namespace aleo_mi355x { namespace kct {

using host::HFr;

// sep(bytes): little-endian, mod r; Montgomery form.  At most 31 bytes are below r as they lie.
static HFr secret_field(const uint8_t* secret, size_t len) {
  if (len <= 31) { HFr v = HFr::zero(); if (len) std::memcpy(v.l, secret, len); return HFr::to_mont(v); }
  const HFr k = HFr::from_u64(256); HFr acc = HFr::zero();
  for (size_t i = len; i-- > 0;) acc = HFr::add(HFr::mul(acc, k), HFr::from_u64(secret[i]));
  return acc;
}
// The secret as the kernel is handed it: its own bytes where there are at most 31, else the 32 canonical bytes of its field element.  Returns the length.
static uint32_t device_secret(uint8_t* out32, const uint8_t* secret, size_t len) {
  if (len <= 31) { if (len) std::memcpy(out32, secret, len); return (uint32_t)len; }
  const HFr c = HFr::from_mont(secret_field(secret, len)); std::memcpy(out32, c.l, 32);
  return KC_MAX_DEVICE_SECRET;
}

static HFr blinding_of(const HFr& nonce_mont, const HFr& s_mont) {
  const HFr in[3] = {host::fr_domain_separator("private_key"), nonce_mont, s_mont};
  HFr b; host::poseidon_hash_many_fr<2>(in, 3, &b, 1);
  return b;
}
static void randomizers(HFr* rnd3, const HFr& s_mont) {
  const HFr in[2] = {host::fr_domain_separator("AleoSymmetricEncryption0"), s_mont};
  host::poseidon_hash_many_fr<8>(in, 2, rnd3, KC_FIELDS);
}

// ---- the device lane's table: account_host.hpp's words as they stand, then KC_S0 -------------------------------------------------------------------------------------
struct KeyCiphertextTables { std::vector<uint32_t> words; };
static const KeyCiphertextTables& key_ciphertext_tables() {
  static const KeyCiphertextTables T = [] {
    KeyCiphertextTables t;
    const std::vector<uint32_t>& ac = acct::account_tables().words;
    t.words.assign(KC_WORDS, 0);
    std::memcpy(t.words.data(), ac.data(), AC_WORDS * 4);
    HFr s[3] = {HFr::zero(), host::fr_domain_separator("AleoPoseidon2"), HFr::from_u64(3)};
    host::poseidon_permute<4, 2>(s);
    s[1] = HFr::add(s[1], host::fr_domain_separator("private_key"));
    for (uint32_t i = 0; i < 3; ++i) put29(t.words.data() + 9 * (KC_S0 + i), s[i]);
    return t;
  }();
  return T;
}

// ---- one pair ---------------------------------------------------------------------------------------------------------------------------------------------------------
// The flag (key_ciphertext_lane.h KC_*) and the seed's 32 canonical bytes, zeros with a flag.  text: `span` characters, no terminator.
static uint8_t open_one_host(uint8_t* seed32, const char* text, uint64_t span, const uint8_t* secret, size_t secret_len) {
  std::memset(seed32, 0, 32);
  uint32_t c[3][8];
  const uint8_t* mine = (const uint8_t*)text;
  const uint32_t status = kc_decode([&](uint32_t j) { return mine[j]; }, span > RS_MAX_CHARS ? RS_MAX_CHARS + 1 : (uint32_t)span, c);
  if (status) return (uint8_t)status;
  const HFr s = secret_field(secret, secret_len);
  HFr rnd[KC_FIELDS]; randomizers(rnd, s);
  uint32_t p[3][8];
  for (uint32_t f = 0; f < KC_FIELDS; ++f) { HFr v; std::memcpy(v.l, c[f], 32); v = HFr::from_mont(HFr::sub(HFr::to_mont(v), rnd[f])); std::memcpy(p[f], v.l, 32); }
  uint32_t key[8], nonce[8];
  if (!kc_layout(p, key, nonce)) return (uint8_t)KC_NOT_DECRYPTED;
  HFr k, n; std::memcpy(k.l, key, 32); std::memcpy(n.l, nonce, 32);
  const HFr b = blinding_of(HFr::to_mont(n), s);
  if (b.is_zero()) return (uint8_t)KC_NOT_DECRYPTED;
  const HFr seed = HFr::from_mont(HFr::mul(HFr::to_mont(k), HFr::inv(b)));
  std::memcpy(seed32, seed.l, 32);
  return (uint8_t)KC_OPENED;
}

// ---- the string of three field elements -------------------------------------------------------------------------------------------------------------------------------
static std::string ciphertext_string(const uint32_t (&c)[3][8]) {
  uint8_t raw[2 + 32 * KC_FIELDS] = {(uint8_t)KC_FIELDS, 0};
  std::memcpy(raw + 2, c, 32 * KC_FIELDS);
  uint8_t sym[(sizeof raw * 8 + 4) / 5 + RS_CHECKSUM_SYMBOLS]; size_t n = 0;
  uint32_t acc = 0; int bits = 0;
  for (size_t i = 0; i < sizeof raw; ++i) { acc = (acc << 8) | raw[i]; bits += 8; while (bits >= 5) { bits -= 5; sym[n++] = (acc >> bits) & 31; } }
  if (bits) sym[n++] = (acc << (5 - bits)) & 31;
  uint32_t chk = KC_PREFIX_STATE;
  for (size_t i = 0; i < n; ++i) chk = rs_polymod_step(chk, sym[i]);
  for (int i = 0; i < 6; ++i) chk = rs_polymod_step(chk, 0);
  chk ^= RS_BECH32M;
  for (int i = 0; i < 6; ++i) sym[n++] = (chk >> (5 * (5 - i))) & 31;
  std::string out = "ciphertext1";
  for (size_t i = 0; i < n; ++i) out.push_back(acct::B32[sym[i]]);
  return out;
}

// Encryptor::encrypt_private_key_with_secret for a nonce the caller chose: seed32 and nonce32 canonical field elements (the caller checked)
static std::string encrypt_host(const uint8_t* seed32, const uint8_t* secret, size_t secret_len, const uint8_t* nonce32) {
  const HFr s = secret_field(secret, secret_len);
  HFr seed, nonce; std::memcpy(seed.l, seed32, 32); std::memcpy(nonce.l, nonce32, 32);
  const HFr key = HFr::from_mont(HFr::mul(blinding_of(HFr::to_mont(nonce), s), HFr::to_mont(seed)));
  uint32_t kw[8], nw[8], p[3][8], c[3][8];
  std::memcpy(kw, key.l, 32); std::memcpy(nw, nonce32, 32);
  kc_plain_fields(kw, nw, p);
  HFr rnd[KC_FIELDS]; randomizers(rnd, s);
  for (uint32_t f = 0; f < KC_FIELDS; ++f) { HFr v; std::memcpy(v.l, p[f], 32); v = HFr::from_mont(HFr::add(HFr::to_mont(v), rnd[f])); std::memcpy(c[f], v.l, 32); }
  return ciphertext_string(c);
}

}}  // namespace aleo_mi355x::kct
