// records_bits.hpp — a record as bits, and what is hashed from them: the checksum of a Record<Ciphertext>, the commitment of a Record<Plaintext>, and the
// account (sk_sig, view key, address) of a private key.  Plain C++ (no HIP) on the layout walk of records_plaintext.hpp and the hashes of serial_host.hpp.
// snarkVM 0.14.5 console/program/src/data/{record,plaintext,ciphertext,identifier}/to_bits.rs, record/to_commitment.rs, console/account [UPSTREAM-RECALL]:
//
//   RECORD BITS   owner | u32 number of data bits | data bits | the nonce x's 253 bits
//   owner         1 bit is_private | 253 bits: a public or decrypted owner's address x, or the one field of an owner still encrypted
//   data bits     per entry: the name's bits (8 per character) | 2 bits visibility (constant 00, public 01, private 10) | the value:
//                 private, still encrypted: 253 bits per field;  private, decrypted: its PLAINTEXT BITS (records_plaintext.hpp: the 252 data bits of each
//                 plain field, trailing zeros and the terminus bit dropped);  constant, public: the PLAINTEXT BITS of its plaintext bytes
//   checksum      hash_bhp1024(RECORD BITS of the ciphertext)                       pinned: the "checksum" of the record output in the reference's transaction
//   commitment    hash_bhp1024(program name bits | network bits | record name bits | RECORD BITS of the plaintext)              pinned: that output's "id"
//   account       sk_sig = hash_to_scalar_psd2([AleoAccountSignatureSecretKey0, seed]), r_sig likewise with "AleoAccountSignatureRandomizer0.0",
//                 sk_prf = hash_to_scalar_psd4([x(sk_sig G), x(r_sig G)]), view key = sk_sig + r_sig + sk_prf, address = view key G       pinned: three accounts
// The conversion of a constant or public entry's bytes into bits (literal: 00 | u8 type | u16 size | value, a string's size 8 per byte; struct: 01 | u8 member
// count | per member u8 name size in bits, name, u16 size, value) is [UPSTREAM-RECALL] and UNPINNED, as the reading of those bytes in records_plaintext.hpp is:
// nothing the reference holds shows such an entry.  A decrypted struct entry's bits are taken as they come out of the fields, and are pinned no further either.
#pragma once
#include "records_plaintext.hpp"
#include "serial_host.hpp"

namespace aleo_mi355x { namespace serial {

static inline void push_bits(std::vector<uint8_t>& bits, uint64_t v, int n) { for (int i = 0; i < n; ++i) bits.push_back((v >> i) & 1); }
static inline void push_bytes(std::vector<uint8_t>& bits, const uint8_t* p, size_t n) { for (size_t i = 0; i < n; ++i) push_bits(bits, p[i], 8); }

// PLAINTEXT BYTES -> PLAINTEXT BITS; false: `why` says what is wrong
static bool bytes_to_bits(std::vector<uint8_t>& out, const uint8_t* p, size_t& pos, size_t end, std::string& why, int depth = 0) {
  if (depth > plaintext::MAX_DEPTH) { why = "nested too deep"; return false; }
  if (pos + 1 > end) { why = "no variant"; return false; }
  const uint8_t variant = p[pos++];
  if (variant == 0) {
    if (pos + 2 > end) { why = "a literal is truncated"; return false; }
    const unsigned ty = p[pos] | (p[pos + 1] << 8); pos += 2;
    const int bits = plaintext::literal_bits(ty);
    if (!bits) { why = "unknown literal type " + std::to_string(ty); return false; }
    push_bits(out, 0, 2); push_bits(out, ty, 8);
    if (bits < 0) {
      if (pos + 2 > end) { why = "a string is truncated"; return false; }
      const size_t n = p[pos] | (p[pos + 1] << 8); pos += 2;
      if (pos + n > end || 8 * n > 65535) { why = "a string is truncated"; return false; }
      push_bits(out, 8 * n, 16); push_bytes(out, p + pos, n); pos += n;
    } else {
      const size_t n = (bits + 7) / 8;
      if (pos + n > end) { why = "a literal is truncated"; return false; }
      push_bits(out, (uint64_t)bits, 16);
      for (int i = 0; i < bits; ++i) out.push_back((p[pos + (i >> 3)] >> (i & 7)) & 1);
      pos += n;
    }
    return true;
  }
  if (variant != 1) { why = "unknown plaintext variant"; return false; }
  if (pos + 1 > end) { why = "a struct is truncated"; return false; }
  const unsigned n = p[pos++];
  out.push_back(0); out.push_back(1); push_bits(out, n, 8);
  for (unsigned k = 0; k < n; ++k) {
    if (pos + 1 > end || pos + 1 + p[pos] + 2 > end) { why = "a member's name is truncated"; return false; }
    const size_t nl = p[pos++];
    if (!plaintext::name_ok(p + pos, nl) || nl > 31) { why = "a member has no valid name"; return false; }
    push_bits(out, 8 * nl, 8); push_bytes(out, p + pos, nl); pos += nl;
    const size_t size = p[pos] | (p[pos + 1] << 8); pos += 2;
    if (pos + size > end) { why = "a member is truncated"; return false; }
    std::vector<uint8_t> inner; size_t q = pos;
    if (!bytes_to_bits(inner, p, q, pos + size, why, depth + 1)) return false;
    if (q != pos + size || inner.size() > 65535) { why = "a member's length is not that of its value"; return false; }
    pos = q;
    push_bits(out, inner.size(), 16); out.insert(out.end(), inner.begin(), inner.end());
  }
  return true;
}

// RECORD BITS of a parsed record: of the ciphertext as it stands (plain = nullptr), or of its plaintext from the r.n_private decrypted fields in randomizer order
static int32_t record_bits(std::vector<uint8_t>& bits, const plaintext::Record& r, const uint8_t* plain, const char* who) {
  auto refuse = [&](const std::string& why) { g_last_error = std::string(who) + ": " + why; return ALEO_MI355X_ERR_BAD_ARG; };
  auto field = [&](const uint8_t* p) { uint64_t v[4]; std::memcpy(v, p, 32); push_field_bits(bits, v); };
  bits.push_back(r.owner_kind == 1);
  field(r.owner_kind == 1 && plain ? plain : r.payload.data() + r.owner_at);
  std::vector<uint8_t> data; std::string why;
  for (const plaintext::Entry& e : r.entries) {
    push_bytes(data, (const uint8_t*)e.name.data(), e.name.size());
    data.push_back(e.visibility == 2); data.push_back(e.visibility == 1);
    if (e.visibility == 2 && plain) {
      plaintext::Bits B;
      if (!plaintext::fields_to_bits(B, plain + 32 * e.first_field, e.n_fields, why)) return refuse("entry '" + e.name + "': " + why);
      data.insert(data.end(), B.b.begin(), B.b.end());
    } else if (e.visibility == 2) {
      for (size_t i = 0; i < e.n_fields; ++i) { uint64_t v[4]; std::memcpy(v, r.payload.data() + e.at + 32 * i, 32); push_field_bits(data, v); }
    } else {
      size_t pos = e.at;
      if (!bytes_to_bits(data, r.payload.data(), pos, e.at + e.len, why) || pos != e.at + e.len) return refuse("entry '" + e.name + "' does not parse: " + (why.empty() ? "bytes are left over" : why));
    }
  }
  push_bits(bits, data.size(), 32);
  bits.insert(bits.end(), data.begin(), data.end());
  field(r.payload.data() + r.nonce_at);
  return ALEO_MI355X_OK;
}

// Identifier::from_str: a letter first, then letters, digits and underscores, at most 31 bytes (the data bits of a field)
static bool identifier_ok(const char* s, size_t n) {
  if (!n || n > 31 || !((s[0] >= 'a' && s[0] <= 'z') || (s[0] >= 'A' && s[0] <= 'Z'))) return false;
  return plaintext::name_ok((const uint8_t*)s, n);
}
// ProgramID::from_str: "<name>.<network>" with the network "aleo"; *dot = the position of the separator
static bool program_id_ok(const char* s, size_t* dot) {
  const char* d = std::strchr(s, '.');
  if (!d || std::strcmp(d + 1, "aleo") != 0 || !identifier_ok(s, (size_t)(d - s))) return false;
  *dot = (size_t)(d - s); return true;
}

static void store_canonical(void* out32, const HFr& mont) { const HFr c = HFr::from_mont(mont); std::memcpy(out32, c.l, 32); }

// ---- the account of a private key ----------------------------------------------------------------------------------------------------------------------------------
static bool base58_decode(std::vector<uint8_t>& out, const char* s, size_t want) {      // exactly `want` bytes, big-endian
  static const char* B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
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
// the three scalars of a private key's account: sk_sig, r_sig and sk_prf (each below 2^250)
static int32_t account_scalars(const char* private_key, uint64_t* sk, uint64_t* rs, uint64_t* prf) {
  static const uint8_t PREFIX[11] = {127, 134, 189, 116, 210, 221, 210, 137, 145, 18, 253};      // "APrivateKey1"
  auto refuse = [&](const char* why) { g_last_error = why; return ALEO_MI355X_ERR_BAD_ARG; };
  std::vector<uint8_t> raw;
  if (!private_key || !base58_decode(raw, private_key, 43) || std::memcmp(raw.data(), PREFIX, 11)) return refuse("account_from_private_key: not an Aleo private key");
  HFr seed; std::memcpy(seed.l, raw.data() + 11, 32);
  if (HFr::geq_p(seed.l)) return refuse("account_from_private_key: the seed is not a canonical field element");
  const HFr in_sk[2] = {host::fr_domain_separator("AleoAccountSignatureSecretKey0"), HFr::to_mont(seed)};
  const HFr in_r[2] = {domain_separator_mod_order("AleoAccountSignatureRandomizer0.0"), in_sk[1]};
  hash_to_scalar(sk, 2, in_sk, 2); hash_to_scalar(rs, 2, in_r, 2);
  const HFr in_prf[2] = {account_mul_g(sk).x, account_mul_g(rs).x};
  hash_to_scalar(prf, 4, in_prf, 2);
  return ALEO_MI355X_OK;
}
static int32_t account_from_private_key(const char* private_key, void* sk_sig32, void* view_key32, void* address_x32) {
  uint64_t sk[4], rs[4], prf[4];
  if (int32_t rc = account_scalars(private_key, sk, rs, prf)) return rc;
  uint64_t view[5] = {0, 0, 0, 0, 0};                        // three scalars below 2^250: the sum is below 3 l
  for (const uint64_t* t : {sk, rs, prf}) { unsigned __int128 cy = 0; for (int i = 0; i < 4; ++i) { cy += (unsigned __int128)view[i] + t[i]; view[i] = (uint64_t)cy; cy >>= 64; } }
  while (!scalar_below_order(view)) { unsigned __int128 br = 0; for (int i = 0; i < 4; ++i) { const unsigned __int128 d = (unsigned __int128)view[i] - ED_ORDER[i] - (uint64_t)br; view[i] = (uint64_t)d; br = (d >> 64) & 1; } }
  if (sk_sig32) std::memcpy(sk_sig32, sk, 32);
  if (view_key32) std::memcpy(view_key32, view, 32);
  if (address_x32) store_canonical(address_x32, account_mul_g(view).x);
  return ALEO_MI355X_OK;
}

}}  // namespace aleo_mi355x::serial
