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
#include "account_host.hpp"

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

// ---- the account of a private key: the string, then account_host.hpp's derivation from its seed ------------------------------------------------------------------
// The 32 seed bytes of an "APrivateKey1…" string; refused: what is no such string, a seed that is no canonical field element
static int32_t private_key_seed(void* seed32, const char* private_key) {
  if (const char* why = private_key_seed_or_why(seed32, private_key)) { g_last_error = std::string("account_from_private_key: ") + why; return ALEO_MI355X_ERR_BAD_ARG; }
  return ALEO_MI355X_OK;
}
// the three scalars of a private key's account: sk_sig, r_sig and sk_prf (each below 2^250)
static int32_t account_scalars(const char* private_key, uint64_t* sk, uint64_t* rs, uint64_t* prf) {
  uint8_t seed[32];
  if (int32_t rc = private_key_seed(seed, private_key)) return rc;
  account_scalars_of_seed(seed, sk, rs, prf);
  return ALEO_MI355X_OK;
}
static int32_t account_from_private_key(const char* private_key, void* sk_sig32, void* view_key32, void* address_x32) {
  uint8_t seed[32];
  if (int32_t rc = private_key_seed(seed, private_key)) return rc;
  account_from_seed(seed, sk_sig32, view_key32, address_x32);
  return ALEO_MI355X_OK;
}

}}  // namespace aleo_mi355x::serial
