// account_host.hpp — accounts on the host: the account of a private key's seed (PrivateKey::try_from(seed) -> ComputeKey -> ViewKey -> Address of snarkVM 0.14.5
// console/account [UPSTREAM-RECALL]; the reference's wasm/src/account/private_key.rs:38-86 and sdk/src/account.ts:82), the strings around it, the search for an
// address with a chosen prefix, and the word table of the device lane (account_lane.h).  Plain C++ (no HIP, touches no device) over serial_host.hpp (the curve,
// the account generator), poseidon.hpp and signature_host.hpp (the table of G).  serial::account_from_seed is the DEFINITION of an account; the lane computes the
// same bytes.
//
//   sk_sig = hash_to_scalar_psd2([AleoAccountSignatureSecretKey0, seed]), r_sig likewise with "AleoAccountSignatureRandomizer0.0",
//   sk_prf = hash_to_scalar_psd4([x(sk_sig G), x(r_sig G)]), view key = sk_sig + r_sig + sk_prf mod l, address = x(view key G)
// Pinned by data the reference holds: the derivation by the three (private key, view key, address) triples of tests/golden/reference_account.json; the private key
// string of a seed by sdk/tests/data/account-data.ts:4,8 (tests/golden/reference_seed.json).
//   UNPINNED  seed_from_bytes for a value not below r — from_seed_unchecked's reduction mod r (private_key.rs:47-55) [UPSTREAM-RECALL]: the reference's one seed
//             is below r already
// A search.  Candidate i of a master seed has the private-key seed chacha_fr(master, i) (chacha.h: uniform over Fr, as PrivateKey::new(rng) draws it with
// Field::rand); it matches when the first p symbols of its address after "aleo1" are the prefix.
#pragma once
#include "signature_host.hpp"
#include "account_lane.h"
#include <string>

namespace aleo_mi355x { namespace serial {

static HFr domain_separator_mod_order(const char* text) {      // Field::new_domain_separator for a text of any length: its bytes, little-endian, mod r; Montgomery form
  const HFr k = HFr::from_u64(256); HFr acc = HFr::zero();
  for (size_t i = std::strlen(text); i-- > 0;) acc = HFr::add(HFr::mul(acc, k), HFr::from_u64((uint8_t)text[i]));
  return acc;
}
static EdA account_mul_g(const uint64_t* k) {                // k G for a scalar below l
  ScanArgs a; std::memset(&a, 0, sizeof a); recode_scalar(a, k);
  return edh_affine(edh_mul_naf(edh_of(account_generator()), a));
}
static void hash_to_scalar(uint64_t* out4, int rate, const HFr* in, size_t n) {      // the low 250 bits of the hash
  HFr h;
  if (rate == 2) host::poseidon_hash_many_fr<2>(in, n, &h, 1); else host::poseidon_hash_many_fr<4>(in, n, &h, 1);
  h = HFr::from_mont(h); h.l[3] &= (1ull << (SK_NONCE_BITS - 192)) - 1;
  std::memcpy(out4, h.l, 32);
}
// the three scalars of the account of a seed (32 canonical bytes, below r): sk_sig, r_sig and sk_prf (each below 2^250)
static void account_scalars_of_seed(const void* seed32, uint64_t* sk, uint64_t* rs, uint64_t* prf) {
  HFr seed; std::memcpy(seed.l, seed32, 32);
  const HFr in_sk[2] = {host::fr_domain_separator("AleoAccountSignatureSecretKey0"), HFr::to_mont(seed)};
  const HFr in_r[2] = {domain_separator_mod_order("AleoAccountSignatureRandomizer0.0"), in_sk[1]};
  hash_to_scalar(sk, 2, in_sk, 2); hash_to_scalar(rs, 2, in_r, 2);
  const HFr in_prf[2] = {account_mul_g(sk).x, account_mul_g(rs).x};
  hash_to_scalar(prf, 4, in_prf, 2);
}
// sk_sig, the view key and the address x of a seed below r; any output may be null.  subtractions (optional): how often l was taken off the sum.
static void account_from_seed(const void* seed32, void* sk_sig32, void* view_key32, void* address_x32, int* subtractions = nullptr) {
  uint64_t sk[4], rs[4], prf[4];
  account_scalars_of_seed(seed32, sk, rs, prf);
  uint64_t view[5] = {0, 0, 0, 0, 0};                        // three scalars below 2^250: the sum is below 3 l
  for (const uint64_t* t : {sk, rs, prf}) { unsigned __int128 cy = 0; for (int i = 0; i < 4; ++i) { cy += (unsigned __int128)view[i] + t[i]; view[i] = (uint64_t)cy; cy >>= 64; } }
  int taken = 0;
  while (!scalar_below_order(view)) { unsigned __int128 br = 0; for (int i = 0; i < 4; ++i) { const unsigned __int128 d = (unsigned __int128)view[i] - ED_ORDER[i] - (uint64_t)br; view[i] = (uint64_t)d; br = (d >> 64) & 1; } ++taken; }
  if (subtractions) *subtractions = taken;
  if (sk_sig32) std::memcpy(sk_sig32, sk, 32);
  if (view_key32) std::memcpy(view_key32, view, 32);
  if (address_x32) { const HFr c = HFr::from_mont(account_mul_g(view).x); std::memcpy(address_x32, c.l, 32); }
}

// ---- base58 and the two key strings ------------------------------------------------------------------------------------------------------------------------------
static const char* const B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
static bool base58_decode(std::vector<uint8_t>& out, const char* s, size_t want) {      // exactly `want` bytes, big-endian
  out.assign(want, 0);
  for (; *s; ++s) {
    const char* d = std::strchr(B58, *s);
    if (!d) return false;
    unsigned carry = (unsigned)(d - B58);
    for (size_t i = want; i-- > 0;) { carry += 58u * out[i]; out[i] = (uint8_t)carry; carry >>= 8; }
    if (carry) return false;
  }
  return true;
}
static std::string base58_encode(const uint8_t* b, size_t n) {      // big-endian bytes; a leading zero byte is a leading '1'
  std::vector<uint8_t> digits;                               // least significant first
  for (size_t i = 0; i < n; ++i) {
    unsigned carry = b[i];
    for (auto& d : digits) { carry += 256u * d; d = (uint8_t)(carry % 58u); carry /= 58u; }
    while (carry) { digits.push_back((uint8_t)(carry % 58u)); carry /= 58u; }
  }
  std::string out;
  for (size_t i = 0; i < n && b[i] == 0; ++i) out.push_back('1');
  for (size_t i = digits.size(); i-- > 0;) out.push_back(B58[digits[i]]);
  return out;
}
static const uint8_t PRIVATE_KEY_PREFIX[11] = {127, 134, 189, 116, 210, 221, 210, 137, 145, 18, 253};      // "APrivateKey1"
static const uint8_t VIEW_KEY_PREFIX[7] = {14, 138, 223, 204, 247, 224, 122};                               // "AViewKey1"
// the 32 seed bytes of an "APrivateKey1…" string; the reason where it is none (null: done)
static const char* private_key_seed_or_why(void* seed32, const char* private_key) {
  std::vector<uint8_t> raw;
  if (!private_key || !base58_decode(raw, private_key, 43) || std::memcmp(raw.data(), PRIVATE_KEY_PREFIX, 11)) return "not an Aleo private key";
  uint64_t seed[4]; std::memcpy(seed, raw.data() + 11, 32);
  if (HFr::geq_p(seed)) return "the seed is not a canonical field element";
  std::memcpy(seed32, seed, 32);
  return nullptr;
}
static std::string private_key_string(const uint8_t* seed32) { uint8_t raw[43]; std::memcpy(raw, PRIVATE_KEY_PREFIX, 11); std::memcpy(raw + 11, seed32, 32); return base58_encode(raw, 43); }
static std::string view_key_string(const uint8_t* view_key32) { uint8_t raw[39]; std::memcpy(raw, VIEW_KEY_PREFIX, 7); std::memcpy(raw + 7, view_key32, 32); return base58_encode(raw, 39); }

}}  // namespace aleo_mi355x::serial

namespace aleo_mi355x { namespace acct {

using host::HFr;

// ---- the device lane's table: signature_host.hpp's words as they stand, then the rate-2 section (account_lane.h AC_*) --------------------------------------------
struct AccountTables { std::vector<uint32_t> words; };
static const AccountTables& account_tables() {
  static const AccountTables T = [] {
    AccountTables t;
    const std::vector<uint32_t>& sg = sig::sig_tables().words;
    t.words.assign(AC_WORDS, 0);
    std::memcpy(t.words.data(), sg.data(), SG_WORDS * 4);
    auto put = [&](uint32_t idx, const HFr& v) { put29(t.words.data() + 9 * idx, v); };
    const HFr doms[2] = {host::fr_domain_separator("AleoAccountSignatureSecretKey0"), serial::domain_separator_mod_order("AleoAccountSignatureRandomizer0.0")};
    for (uint32_t k = 0; k < 2; ++k) {
      HFr s[3] = {HFr::zero(), host::fr_domain_separator("AleoPoseidon2"), HFr::from_u64(2)};
      host::poseidon_permute<4, 2>(s);
      s[1] = HFr::add(s[1], doms[k]);
      for (uint32_t i = 0; i < 3; ++i) put(AC_S0 + 3 * k + i, s[i]);
    }
    const auto& P = host::PoseidonParams<4, 2>::get();
    for (int r = 0; r < host::POSEIDON_ROUNDS; ++r) for (int i = 0; i < 3; ++i) put(AC_ARK + 3 * r + i, P.ark[r][i]);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) put(AC_MDS + 3 * i + j, P.mds[i][j]);
    return t;
  }();
  return T;
}

// ---- one account with its flag, as the lane returns it ---------------------------------------------------------------------------------------------------------------
// any output may be null; a refused seed's rows are zero
static uint8_t derive_one_host(const uint8_t* seed32, uint8_t* sk_sig32, uint8_t* view_key32, uint8_t* address_x32) {
  uint64_t seed[4]; std::memcpy(seed, seed32, 32);
  if (HFr::geq_p(seed)) {
    for (uint8_t* p : {sk_sig32, view_key32, address_x32}) if (p) std::memset(p, 0, 32);
    return (uint8_t)ACC_BAD_SEED;
  }
  serial::account_from_seed(seed32, sk_sig32, view_key32, address_x32);
  return (uint8_t)ACC_OK;
}

// what signing needs of the account of a seed below r (signature_host.hpp SignerKeys): derived once per key, whatever the number of signatures under it
static sig::SignerKeys signer_keys_of_seed(const uint8_t* seed32) {
  uint64_t sk[4], rs[4], prf[4];
  serial::account_scalars_of_seed(seed32, sk, rs, prf);
  sig::SignerKeys a;
  std::memcpy(a.sk_sig, sk, 32); sig::x_of_mul_g(a.pk_x, sk); sig::x_of_mul_g(a.pr_x, rs);
  serial::account_from_seed(seed32, nullptr, nullptr, a.address_x);
  return a;
}

// ---- the address string: bech32m (BIP-350) under "aleo", written out here and not shared with the lane ------------------------------------------------------------
static const char* const B32 = "qpzry9x8gf2tvdw0s3jn54khce6mua7l";
static uint32_t bech32_polymod(const uint8_t* v, size_t n) {
  static const uint32_t gen[5] = {0x3b6a57b2u, 0x26508e6du, 0x1ea119fau, 0x3d4233ddu, 0x2a1462b3u};
  uint32_t chk = 1;
  for (size_t k = 0; k < n; ++k) { const uint32_t b = chk >> 25; chk = ((chk & 0x1ffffffu) << 5) ^ v[k]; for (int i = 0; i < 5; ++i) if ((b >> i) & 1) chk ^= gen[i]; }
  return chk;
}
// the 52 symbols of 32 bytes: five bits at a time, the most significant bit of each byte first, the last one padded with zeros
static void address_symbols(uint8_t* sym52, const uint8_t* x32) {
  uint32_t acc = 0; int bits = 0, n = 0;
  for (int i = 0; i < 32; ++i) { acc = (acc << 8) | x32[i]; bits += 8; while (bits >= 5) { bits -= 5; sym52[n++] = (acc >> bits) & 31; } }
  sym52[n++] = (acc << (5 - bits)) & 31;
}
// 63 characters, no terminator
static void address_string(char* out63, const uint8_t* x32) {
  uint8_t v[9 + 52 + 6] = {3, 3, 3, 3, 0, 1, 12, 5, 15};      // "aleo" expanded
  address_symbols(v + 9, x32);
  std::memset(v + 61, 0, 6);
  const uint32_t pm = bech32_polymod(v, sizeof v) ^ 0x2bc830a3u;
  std::memcpy(out63, "aleo1", 5);
  for (int i = 0; i < 52; ++i) out63[5 + i] = B32[v[9 + i]];
  for (int i = 0; i < 6; ++i) out63[57 + i] = B32[(pm >> (5 * (5 - i))) & 31];
}

// ---- prefixes and the search -----------------------------------------------------------------------------------------------------------------------------------------
// A prefix of p symbols as the top 5 p bits of the first 64 bits of an address's symbol stream (account_lane.h ac_stream_head)
struct Prefix { uint32_t symbols; uint64_t want, mask; };
static const char* parse_prefix(Prefix& p, const char* s) {      // the reason where it is refused
  if (!s) return "null prefix";
  const size_t n = std::strlen(s);
  if (n > ACC_MAX_PREFIX) return "a prefix has at most 12 characters";
  p.symbols = (uint32_t)n; p.want = 0; p.mask = 0;
  for (size_t i = 0; i < n; ++i) {
    const char* q = std::strchr(B32, s[i]);
    if (!q) return "a prefix is made of the characters qpzry9x8gf2tvdw0s3jn54khce6mua7l";
    p.want |= (uint64_t)(q - B32) << (59 - 5 * i);
    p.mask |= (uint64_t)31 << (59 - 5 * i);
  }
  return nullptr;
}
static bool prefix_matches(const Prefix& p, const uint8_t* address_x32) {
  uint64_t head = 0;
  for (int i = 0; i < 8; ++i) head = (head << 8) | address_x32[i];
  return (head & p.mask) == p.want;
}
static void candidate_seed(uint8_t* seed32, const uint8_t* master32, uint64_t index) {
  uint32_t key[8], w[8]; std::memcpy(key, master32, 32);
  account_candidate_seed(w, key, index);
  std::memcpy(seed32, w, 32);
}
static bool candidate_matches(const uint8_t* master32, uint64_t index, const Prefix& p, uint8_t* seed32) {
  uint8_t ax[32];
  candidate_seed(seed32, master32, index);
  serial::account_from_seed(seed32, nullptr, nullptr, ax);
  return prefix_matches(p, ax);
}
// The first max_hits matching indices of [first, first + count), ascending; *next: the index after the last hit when there are max_hits of them, else the range's
// end.  hit_seed32 (optional): the hits' seeds.  The DEFINITION of a search's result.
static void search_host(const uint8_t* master32, uint64_t first, uint64_t count, const Prefix& p, size_t max_hits, uint64_t* hit_index, uint8_t* hit_seed32, size_t* n_hits, uint64_t* next) {
  size_t n = 0;
  *next = max_hits ? first + count : first;
  for (uint64_t i = first; n < max_hits && i < first + count; ++i) {
    uint8_t seed[32];
    if (!candidate_matches(master32, i, p, seed)) continue;
    hit_index[n] = i; if (hit_seed32) std::memcpy(hit_seed32 + 32 * n, seed, 32);
    if (++n == max_hits) *next = i + 1;
  }
  *n_hits = n;
}

// from_seed_unchecked's reduction: 32 arbitrary bytes, little-endian, mod r (UNPINNED above r: see the head of this file)
static void seed_from_bytes(uint8_t* seed32, const uint8_t* bytes32) {
  const HFr k = HFr::from_u64(256); HFr acc = HFr::zero();
  for (int i = 32; i-- > 0;) acc = HFr::add(HFr::mul(acc, k), HFr::from_u64(bytes32[i]));
  const HFr c = HFr::from_mont(acc); std::memcpy(seed32, c.l, 32);
}

}}  // namespace aleo_mi355x::acct
