// records_plaintext.hpp — a record's structure and its plaintext string on the host: what stands between the decrypted fields (records_decrypt.hip) and the
// `RecordPlaintext` string the reference's callers read (wasm/src/record/record_plaintext.rs; rust/src/api/blocking.rs:274-283 sums `microcredits()`).
// Plain C++ (no HIP).  snarkVM 0.14.5 console/program/src/data/{record, plaintext, literal} [UPSTREAM-RECALL]; what the reference pins is said line by line:
//
//   payload   u8 owner variant | owner | u8 entry count | per entry: u8 name length, name, u16 byte length, ENTRY | 32 B nonce x       (pinned: records.owner)
//   ENTRY     u8 visibility (0 constant, 1 public, 2 private) | private: u16 field count, that many 32 B fields                        (private: pinned)
//                                                             | constant, public: PLAINTEXT BYTES                                      (UNPINNED)
//   PLAINTEXT BYTES   u8 variant | 0 literal: u16 type, the value's little-endian bytes (string: u16 length, bytes)
//                                | 1 struct: u8 member count, per member: u8 name length, name, u16 byte length, PLAINTEXT BYTES       (UNPINNED: nothing the reference holds)
//   PLAINTEXT BITS (a private entry's plain fields: the low 252 bits of each, trailing zeros and the terminus 1 stripped; oracle/poseidon.py:222-247)
//             2 bits variant | 00 literal: u8 type, u16 size in bits, value | 01 struct: u8 member count, per member: u8 name size in bits, name, u16 size, PLAINTEXT BITS
//                                                                        (pinned: literal u64 by records.owner, struct and literal field by the private-key ciphertext)
//   literal types   0 address, 1 boolean, 2 field, 3 group, 4-8 i8..i128, 9-13 u8..u128, 14 scalar, 15 string   (0, 2, 12 pinned; the rest UPSTREAM-RECALL)
//   string    "{\n  owner: <aleo1…>.<visibility>,\n  <name>: <value>.<visibility>,\n  …  _nonce: <decimal>group.public\n}"              (pinned: plaintexts.owner)
//             struct entries: "{", one member per line two spaces deeper, every literal with the entry's visibility, "}" at the entry's own indentation (UNPINNED)
#pragma once
#include "ctx.h"
#include "host_field.hpp"
#include <cstring>
#include <string>
#include <vector>

namespace aleo_mi355x { namespace plaintext {

using host::HFr;

static constexpr uint64_t SCALAR_MODULUS[4] = {0xb95aee9ac33fd9ffULL, 0x5293a3afc43c8afeULL, 0x982d1347970dec00ULL, 0x04aad957a68b2955ULL};
static constexpr int MAX_DEPTH = 32, DATA_BITS = 252;
static const char* const VISIBILITY[3] = {"constant", "public", "private"};
static const char* const SUFFIX[16] = {"", "", "field", "group", "i8", "i16", "i32", "i64", "i128", "u8", "u16", "u32", "u64", "u128", "scalar", ""};

struct Entry { std::string name; uint8_t visibility; size_t at, len; size_t first_field, n_fields; };      // at / len: the PLAINTEXT BYTES, or the fields, inside the payload
struct Record {
  std::vector<uint8_t> payload;
  int owner_kind = 0; size_t owner_at = 0, nonce_at = 0;
  std::vector<Entry> entries;
  size_t n_private = 0;                                      // fields in randomizer order: the owner's (if private), then every private entry's
};

static bool name_ok(const uint8_t* p, size_t n) {
  if (!n) return false;
  for (size_t i = 0; i < n; ++i) { const uint8_t c = p[i]; if (!((c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_')) return false; }
  return true;
}

// The structure of a "record1…" string.  aleo_mi355x_record_parse has accepted it: the walk over the entries cannot leave the payload.
static int32_t parse(Record& r, const char* record1, const char* who) {
  int32_t kind; uint8_t owner[32], nonce[32];
  if (int32_t rc = aleo_mi355x_record_parse(record1, &kind, owner, nonce)) return rc;
  r.payload.resize(std::strlen(record1) + 1); size_t len = r.payload.size(); char hrp[16];
  if (int32_t rc = aleo_mi355x_bech32m_decode(r.payload.data(), &len, hrp, sizeof hrp, record1)) return rc;
  r.payload.resize(len);
  const uint8_t* b = r.payload.data();
  auto refuse = [&](const std::string& why) { g_last_error = std::string(who) + ": " + why; return ALEO_MI355X_ERR_BAD_ARG; };
  r.owner_kind = kind; r.owner_at = kind == 1 ? 3 : 1; r.n_private = kind == 1 ? 1 : 0;
  size_t at = r.owner_at + 32;
  const unsigned entries = b[at++];
  for (unsigned e = 0; e < entries; ++e) {
    Entry en; const size_t nl = b[at++];
    if (!name_ok(b + at, nl)) return refuse("entry " + std::to_string(e) + " has no valid name");
    en.name.assign((const char*)b + at, nl); at += nl;
    const size_t el = b[at] | (b[at + 1] << 8); at += 2;
    if (el < 1 || b[at] > 2) return refuse("entry '" + en.name + "' has no known visibility");
    en.visibility = b[at]; en.at = at + 1; en.len = el - 1; en.first_field = r.n_private; en.n_fields = 0;
    if (en.visibility == 2) {
      if (el < 3) return refuse("entry '" + en.name + "' is truncated");
      en.n_fields = b[at + 1] | (b[at + 2] << 8);
      if (el != 3 + 32 * en.n_fields) return refuse("entry '" + en.name + "': its length is not that of its field count");
      en.at = at + 3; en.len = 32 * en.n_fields;
      for (size_t i = 0; i < en.n_fields; ++i) { uint64_t v[4]; std::memcpy(v, b + en.at + 32 * i, 32); if (HFr::geq_p(v)) return refuse("entry '" + en.name + "' holds a field that is not canonical"); }
      r.n_private += en.n_fields;
    }
    at += el;
    r.entries.push_back(std::move(en));
  }
  r.nonce_at = at;
  return ALEO_MI355X_OK;
}

// the private fields in randomizer order, 32 bytes each
static void gather_fields(const Record& r, uint8_t* out) {
  size_t k = 0;
  if (r.owner_kind == 1) { std::memcpy(out, r.payload.data() + r.owner_at, 32); k = 1; }
  for (const Entry& e : r.entries) if (e.visibility == 2) { std::memcpy(out + 32 * k, r.payload.data() + e.at, e.len); k += e.n_fields; }
}

// ---- numbers ------------------------------------------------------------------------------------------------------------------------------------------
static bool geq(const uint64_t* a, const uint64_t* m) { for (int i = 3; i >= 0; --i) { if (a[i] > m[i]) return true; if (a[i] < m[i]) return false; } return true; }
static std::string decimal(const uint64_t* v4) {
  uint64_t v[4] = {v4[0], v4[1], v4[2], v4[3]};
  std::string out;
  while (v[0] | v[1] | v[2] | v[3]) {
    unsigned __int128 rem = 0;
    for (int i = 3; i >= 0; --i) { const unsigned __int128 cur = (rem << 64) | v[i]; v[i] = (uint64_t)(cur / 10u); rem = cur % 10u; }
    out.push_back((char)('0' + (unsigned)rem));
  }
  if (out.empty()) out = "0";
  return std::string(out.rbegin(), out.rend());
}
static int literal_bits(unsigned type) {                   // the size of a literal's value in bits; -1: any multiple of 8 (string); 0: unknown type
  if (type == 0 || type == 2 || type == 3) return 253;
  if (type == 1) return 1;
  if (type >= 4 && type <= 8) return 8 << (type - 4);
  if (type >= 9 && type <= 13) return 8 << (type - 9);
  if (type == 14) return 251;
  return type == 15 ? -1 : 0;
}

// "<value><suffix>.<visibility>" of a literal whose value is v (numbers: `bits` wide, little-endian limbs) or text (strings); false: `why` says what is wrong
static bool render_literal(std::string& out, unsigned type, const uint64_t* v, const std::string& text, const char* vis, std::string& why) {
  if (type == 0 || type == 2 || type == 3) {
    if (geq(v, host::HParams<4>::P)) { why = "a value is not below the field's modulus"; return false; }
    if (type == 0) {
      char s[80];
      if (aleo_mi355x_bech32m_encode(s, sizeof s, "aleo", v, 32)) { why = "an address does not encode"; return false; }
      out += s;
    } else out += decimal(v);
  } else if (type == 1) out += v[0] ? "true" : "false";
  else if (type >= 4 && type <= 8) {
    const int bits = literal_bits(type);
    uint64_t m[4] = {v[0], v[1], 0, 0};
    const bool negative = (v[(bits - 1) >> 6] >> ((bits - 1) & 63)) & 1;
    if (negative) {                                          // two's complement of `bits` bits
      unsigned __int128 x = ((unsigned __int128)v[1] << 64) | v[0];
      if (bits < 128) x |= ~(unsigned __int128)0 << bits;
      x = ~x + 1;
      m[0] = (uint64_t)x; m[1] = (uint64_t)(x >> 64);
      out += "-";
    }
    out += decimal(m);
  } else if (type >= 9 && type <= 13) out += decimal(v);
  else if (type == 14) {
    if (geq(v, SCALAR_MODULUS)) { why = "a scalar is not below the scalar field's modulus"; return false; }
    out += decimal(v);
  } else if (type == 15) {
    for (unsigned char c : text) if (c < 0x20 || c == '"' || c == 0x7f) { why = "a string holds a character that cannot be quoted"; return false; }
    out += "\"" + text + "\"";
  } else { why = "unknown literal type " + std::to_string(type); return false; }
  out += SUFFIX[type]; out += "."; out += vis;
  return true;
}

// ---- PLAINTEXT BITS -------------------------------------------------------------------------------------------------------------------------------------
struct Bits {
  std::vector<uint8_t> b;
  bool take(size_t& pos, size_t end, size_t n, uint64_t* v) const {      // n <= 256 bits, little-endian
    if (pos + n > end || n > 256) return false;
    v[0] = v[1] = v[2] = v[3] = 0;
    for (size_t i = 0; i < n; ++i) v[i >> 6] |= (uint64_t)b[pos + i] << (i & 63);
    pos += n; return true;
  }
};
static bool render_bits(std::string& out, const Bits& B, size_t pos, size_t end, int indent, const char* vis, std::string& why, int depth = 0) {
  uint64_t v[4];
  if (depth > MAX_DEPTH) { why = "nested too deep"; return false; }
  if (!B.take(pos, end, 2, v)) { why = "no variant"; return false; }
  if (v[0] == 0) {
    uint64_t ty[4], size[4];
    if (!B.take(pos, end, 8, ty) || !B.take(pos, end, 16, size)) { why = "a literal is truncated"; return false; }
    if (pos + size[0] != end) { why = "a literal's size is not what is left of it"; return false; }
    const int want = literal_bits((unsigned)ty[0]);
    if (!want) { why = "unknown literal type " + std::to_string(ty[0]); return false; }
    if (want > 0 ? size[0] != (uint64_t)want : size[0] % 8 != 0) { why = "a literal's size does not fit its type"; return false; }
    std::string text;
    if (want < 0) { for (size_t i = 0; i < size[0] / 8; ++i) { uint64_t c[4]; B.take(pos, end, 8, c); text.push_back((char)c[0]); } v[0] = v[1] = v[2] = v[3] = 0; }
    else B.take(pos, end, size[0], v);
    return render_literal(out, (unsigned)ty[0], v, text, vis, why);
  }
  if (v[0] != 2) { why = "unknown plaintext variant"; return false; }      // bits (0, 1)
  uint64_t n[4];
  if (!B.take(pos, end, 8, n)) { why = "a struct is truncated"; return false; }
  out += "{\n";
  for (uint64_t k = 0; k < n[0]; ++k) {
    uint64_t ln[4], size[4];
    if (!B.take(pos, end, 8, ln) || ln[0] % 8 || pos + ln[0] > end) { why = "a member's name is truncated"; return false; }
    std::string name;
    for (size_t i = 0; i < ln[0] / 8; ++i) { uint64_t c[4]; B.take(pos, end, 8, c); name.push_back((char)c[0]); }
    if (!name_ok((const uint8_t*)name.data(), name.size())) { why = "a member has no valid name"; return false; }
    if (!B.take(pos, end, 16, size) || pos + size[0] > end) { why = "member '" + name + "' is truncated"; return false; }
    out.append(indent + 2, ' '); out += name + ": ";
    if (!render_bits(out, B, pos, pos + size[0], indent + 2, vis, why, depth + 1)) return false;
    pos += size[0];
    out += k + 1 < n[0] ? ",\n" : "\n";
  }
  if (pos != end) { why = "a struct's size is not that of its members"; return false; }
  out.append(indent, ' '); out += "}";
  return true;
}
// the plain fields of a private entry -> its bits
static bool fields_to_bits(Bits& B, const uint8_t* fields, size_t n, std::string& why) {
  B.b.clear(); B.b.reserve(n * DATA_BITS);
  for (size_t f = 0; f < n; ++f)
    for (int i = 0; i < DATA_BITS; ++i) B.b.push_back((fields[32 * f + (i >> 3)] >> (i & 7)) & 1);
  while (!B.b.empty() && !B.b.back()) B.b.pop_back();
  if (B.b.empty()) { why = "no terminus bit"; return false; }
  B.b.pop_back();
  return true;
}

// ---- PLAINTEXT BYTES ----------------------------------------------------------------------------------------------------------------------------------
static bool render_bytes(std::string& out, const uint8_t* p, size_t& pos, size_t end, int indent, const char* vis, std::string& why, int depth = 0) {
  if (depth > MAX_DEPTH) { why = "nested too deep"; return false; }
  if (pos + 1 > end) { why = "no variant"; return false; }
  const uint8_t variant = p[pos++];
  if (variant == 0) {
    if (pos + 2 > end) { why = "a literal is truncated"; return false; }
    const unsigned ty = p[pos] | (p[pos + 1] << 8); pos += 2;
    const int bits = literal_bits(ty);
    if (!bits) { why = "unknown literal type " + std::to_string(ty); return false; }
    uint64_t v[4] = {0, 0, 0, 0}; std::string text;
    if (bits < 0) {
      if (pos + 2 > end) { why = "a string is truncated"; return false; }
      const size_t n = p[pos] | (p[pos + 1] << 8); pos += 2;
      if (pos + n > end) { why = "a string is truncated"; return false; }
      text.assign((const char*)p + pos, n); pos += n;
    } else {
      const size_t n = (bits + 7) / 8;
      if (pos + n > end) { why = "a literal is truncated"; return false; }
      std::memcpy(v, p + pos, n); pos += n;
      if (bits == 1 && v[0] > 1) { why = "a boolean is neither 0 nor 1"; return false; }
    }
    return render_literal(out, ty, v, text, vis, why);
  }
  if (variant != 1) { why = "unknown plaintext variant"; return false; }
  if (pos + 1 > end) { why = "a struct is truncated"; return false; }
  const unsigned n = p[pos++];
  out += "{\n";
  for (unsigned k = 0; k < n; ++k) {
    if (pos + 1 > end || pos + 1 + p[pos] + 2 > end) { why = "a member's name is truncated"; return false; }
    const size_t nl = p[pos++];
    if (!name_ok(p + pos, nl)) { why = "a member has no valid name"; return false; }
    const std::string name((const char*)p + pos, nl); pos += nl;
    const size_t size = p[pos] | (p[pos + 1] << 8); pos += 2;
    if (pos + size > end) { why = "member '" + name + "' is truncated"; return false; }
    out.append(indent + 2, ' '); out += name + ": ";
    size_t q = pos;
    if (!render_bytes(out, p, q, pos + size, indent + 2, vis, why, depth + 1)) return false;
    if (q != pos + size) { why = "member '" + name + "': its length is not that of its value"; return false; }
    pos = q;
    out += k + 1 < n ? ",\n" : "\n";
  }
  out.append(indent, ' '); out += "}";
  return true;
}

// ---- the record string ----------------------------------------------------------------------------------------------------------------------------------
// plain: r.n_private x 32 B, the decrypted fields in randomizer order.  address_x32 (optional): the decrypted or public owner must be it (ERR_NOT_OWNER).
static int32_t render(std::string& out, const Record& r, const uint8_t* plain, const uint8_t* address_x32, const char* who) {
  auto refuse = [&](const std::string& why) { g_last_error = std::string(who) + ": " + why; return ALEO_MI355X_ERR_BAD_ARG; };
  const uint8_t* owner = r.owner_kind == 1 ? plain : r.payload.data() + r.owner_at;
  if (address_x32 && std::memcmp(owner, address_x32, 32)) { g_last_error = std::string(who) + ": the record's owner is not the given address"; return ALEO_MI355X_ERR_NOT_OWNER; }
  std::string why;
  uint64_t v[4];
  out = "{\n  owner: ";
  std::memcpy(v, owner, 32);
  if (!render_literal(out, 0, v, "", VISIBILITY[r.owner_kind == 1 ? 2 : 1], why)) return refuse("the owner: " + why);
  out += ",\n";
  for (const Entry& e : r.entries) {
    out += "  " + e.name + ": ";
    bool ok;
    if (e.visibility == 2) {
      Bits B;
      ok = fields_to_bits(B, plain + 32 * e.first_field, e.n_fields, why) && render_bits(out, B, 0, B.b.size(), 2, VISIBILITY[2], why);
    } else {
      size_t pos = e.at;
      ok = render_bytes(out, r.payload.data(), pos, e.at + e.len, 2, VISIBILITY[e.visibility], why);
      if (ok && pos != e.at + e.len) { ok = false; why = "bytes are left over"; }
    }
    if (!ok) return refuse("entry '" + e.name + "' does not parse: " + why);
    out += ",\n";
  }
  std::memcpy(v, r.payload.data() + r.nonce_at, 32);
  out += "  _nonce: " + decimal(v) + "group.public\n}";
  return ALEO_MI355X_OK;
}

}}  // namespace aleo_mi355x::plaintext
