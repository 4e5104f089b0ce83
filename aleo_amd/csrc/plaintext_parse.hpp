// plaintext_parse.hpp — a RecordPlaintext STRING as a parsed record: the inverse of plaintext::render (records_plaintext.hpp), what RecordPlaintext.fromString of
// the reference reads (wasm/src/record/record_plaintext.rs:45-50) and every write call takes as `fee_record` / `amount_record` (wasm/src/programs/manager/transfer.rs:66-68).
// Plain C++ (no HIP).  snarkVM 0.14.5 console/program/src/data/{record, plaintext, literal}/parse.rs [UPSTREAM-RECALL]; pinned by the three strings the reference
// holds and the serial number of one of them (tests/golden/reference_plaintexts.json, reference_serial.json), which only show a private owner and one private u64.
//
//   record    "{" owner ":" ADDRESS "." ("public" | "private") "," { NAME ":" VALUE "," } "_nonce" ":" DECIMAL "group.public" "}"     whitespace (space, tab,
//             CR, LF) between any two tokens and around the whole; nothing else behind the closing brace
//   VALUE     LITERAL "." VISIBILITY  |  "{" NAME ":" VALUE { "," NAME ":" VALUE } "}"     every literal of an entry with the same visibility, which is the entry's
//   LITERAL   "aleo1" and 58 symbols (bech32m, the checksum and the zero padding checked, the x below r) | "true" | "false" | "\"" characters "\"" |
//             ["-"] DIGITS SUFFIX with SUFFIX one of plaintext::SUFFIX: field, group below r; scalar below the scalar field's modulus; u8 .. u128 and i8 .. i128 in
//             their range ("-" for the signed types only)
//   NAME      an identifier: a letter, then letters, digits and underscores, at most 31 bytes
//   RECORD BITS (records_bits.hpp:5-9) of what was read: an entry's value has the same bits whatever its visibility —
//             literal  00 | u8 type | u16 size | value          struct  01 | u8 member count | per member: u8 name size in bits, name, u16 size, value
//             — which are the PLAINTEXT BITS a private entry's decrypted fields hold and what serial::bytes_to_bits makes of a constant or public entry's bytes: for
//             every record the library decrypts and renders, record_bits(parse(render(record))) is serial::record_bits(record, plain fields).
// What the reference cannot pin, each choice marked:
//   UNPINNED  underscores behind a digit ("1_000u64") are skipped; leading zeros are read; "-0i8" is 0       (all three [UPSTREAM-RECALL]: snarkVM's integer parser)
//   UNPINNED  a sign on field, group, scalar and the unsigned types is refused
//   UNPINNED  no comments: "//" is refused like any other stray text
//   UNPINNED  at most MAX_ENTRIES = 255 entries, what the payload's u8 count holds (upstream's Network::MAX_DATA_ENTRIES is 32; the ciphertext road does not ask either)
//   UNPINNED  `owner` is refused as an entry's name (it would be a duplicate); `_nonce` is no identifier; duplicate names are refused among a struct's members too
//   UNPINNED  a struct has 1 .. 255 members and nests to plaintext::MAX_DEPTH; a quoted string holds no '"', no control character and no escape, at most 8191 bytes
//   UNPINNED  no comma behind the last member of a struct or behind the nonce
// parse() and the batch calls check CANONICAL ENCODING only, as render does: owner, nonce and `group` values are x-coordinates below r.  Whether they are
// x-coordinates of points of the prime-order subgroup is asked by aleo_mi355x_record_plaintext_parse alone (plaintexts.hip, with sig::point_from_x).
#pragma once
#include "records_bits.hpp"

namespace aleo_mi355x { namespace ptext {

using host::HFr;

static constexpr size_t MAX_ENTRIES = 255, MAX_STRING_BYTES = 8191;

struct Value {
  bool is_struct = false;
  unsigned type = 0; uint64_t v[4] = {0, 0, 0, 0}; std::string text;      // a literal: numbers as `literal_bits(type)` bits (two's complement), strings as text
  std::vector<std::pair<std::string, Value>> members;
};
struct Entry { std::string name; uint8_t visibility; Value value; };
struct Parsed { int owner_kind = 0; uint8_t owner[32], nonce[32]; std::vector<Entry> entries; };      // owner_kind: 0 public, 1 private, as aleo_mi355x_record_parse has it

static inline bool is_ws(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
static inline bool is_word(char c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; }

struct Reader {
  const char* s; size_t n, at = 0; std::string why;
  bool fail(const std::string& w) { if (why.empty()) why = w; return false; }
  void ws() { while (at < n && is_ws(s[at])) ++at; }
  bool eat(char c) { ws(); if (at < n && s[at] == c) { ++at; return true; } return false; }
  std::string word() { ws(); const size_t a = at; while (at < n && is_word(s[at])) ++at; return std::string(s + a, at - a); }
  bool starts(const char* w) const { const size_t k = std::strlen(w); return at + k <= n && !std::memcmp(s + at, w, k); }

  // DIGITS (underscores behind a digit skipped) into four words; false: no digit, or the number does not fit 256 bits
  bool decimal(uint64_t (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0;
    if (at >= n || s[at] < '0' || s[at] > '9') return fail("a number has no digits");
    for (; at < n && ((s[at] >= '0' && s[at] <= '9') || s[at] == '_'); ++at) {
      if (s[at] == '_') continue;
      unsigned __int128 cy = (unsigned)(s[at] - '0');
      for (int i = 0; i < 4; ++i) { cy += (unsigned __int128)v[i] * 10u; v[i] = (uint64_t)cy; cy >>= 64; }
      if (cy) return fail("a number is too large");
    }
    return true;
  }

  // ".<visibility>" behind a literal
  bool visibility(int& vis) {
    if (at >= n || s[at] != '.') return fail("a literal has no visibility");
    ++at;
    const size_t a = at; while (at < n && is_word(s[at])) ++at;
    const std::string w(s + a, at - a);
    for (int k = 0; k < 3; ++k) if (w == plaintext::VISIBILITY[k]) { vis = k; return true; }
    return fail("unknown visibility '" + w + "'");
  }

  bool literal(Value& out, int& vis) {
    out = Value();
    if (starts("aleo")) {
      const size_t a = at; while (at < n && is_word(s[at])) ++at;
      const std::string text(s + a, at - a);
      uint8_t raw[64]; size_t len = sizeof raw; char hrp[16];
      if (text.size() != 63 || aleo_mi355x_bech32m_decode(raw, &len, hrp, sizeof hrp, text.c_str()) || std::strcmp(hrp, "aleo") || len != 32) return fail("an address does not decode");
      std::memcpy(out.v, raw, 32);
      if (HFr::geq_p(out.v)) return fail("an address is not below the field's modulus");
      out.type = 0;
    } else if (starts("true") || starts("false")) {
      out.type = 1; out.v[0] = s[at] == 't'; at += out.v[0] ? 4 : 5;
    } else if (at < n && s[at] == '"') {
      const size_t a = ++at;
      while (at < n && s[at] != '"') { const unsigned char c = (unsigned char)s[at]; if (c < 0x20 || c == 0x7f) return fail("a string holds a character that cannot be quoted"); ++at; }
      if (at >= n) return fail("a string does not end");
      if (at - a > MAX_STRING_BYTES) return fail("a string is too long");
      out.type = 15; out.text.assign(s + a, at - a); ++at;
    } else {
      const bool negative = at < n && s[at] == '-';
      if (negative) ++at;
      uint64_t m[4];
      if (!decimal(m)) return false;
      const size_t a = at; while (at < n && is_word(s[at])) ++at;
      const std::string suffix(s + a, at - a);
      unsigned ty = 0;
      for (unsigned k = 2; k < 15; ++k) if (suffix == plaintext::SUFFIX[k]) ty = k;
      if (!ty) return fail("unknown literal type '" + suffix + "'");
      const int bits = plaintext::literal_bits(ty);
      const bool is_signed = ty >= 4 && ty <= 8;
      if (negative && !is_signed) return fail("a sign on a type that has none");
      if (ty == 2 || ty == 3) { if (HFr::geq_p(m)) return fail("a value is not below the field's modulus"); }
      else if (ty == 14) { if (plaintext::geq(m, plaintext::SCALAR_MODULUS)) return fail("a scalar is not below the scalar field's modulus"); }
      else {
        // the magnitude: below 2^bits (unsigned), below 2^(bits - 1) (signed, not negative), at most 2^(bits - 1) (negative)
        const int top = is_signed ? bits - 1 : bits;
        uint64_t lim[4] = {0, 0, 0, 0}; bool over;
        if (top < 256) lim[top >> 6] = 1ull << (top & 63);
        if (negative) { over = plaintext::geq(m, lim) && std::memcmp(m, lim, 32) != 0; } else over = plaintext::geq(m, lim);
        if (over) return fail("a value is out of its type's range");
        if (negative) {                                        // two's complement of `bits` bits
          unsigned __int128 x = ((unsigned __int128)m[1] << 64) | m[0];
          x = ~x + 1;
          if (bits < 128) x &= ((unsigned __int128)1 << bits) - 1;
          m[0] = (uint64_t)x; m[1] = (uint64_t)(x >> 64);
        }
      }
      out.type = ty; std::memcpy(out.v, m, 32);
    }
    return visibility(vis);
  }

  // vis: -1 on entry to an entry's value, then what its first literal says
  bool value(Value& out, int& vis, int depth) {
    ws();
    if (at < n && s[at] == '{') {
      if (depth >= plaintext::MAX_DEPTH) return fail("nested too deep");
      ++at; out = Value(); out.is_struct = true;
      for (;;) {
        const std::string name = word();
        if (!serial::identifier_ok(name.data(), name.size())) return fail("a member has no valid name");
        for (const auto& m : out.members) if (m.first == name) return fail("duplicate member '" + name + "'");
        if (!eat(':')) return fail("member '" + name + "' has no value");
        out.members.emplace_back(name, Value());
        if (!value(out.members.back().second, vis, depth + 1)) return false;
        if (out.members.size() > 255) return fail("a struct has more than 255 members");
        if (eat(',')) continue;
        if (eat('}')) return true;
        return fail("a struct does not end");
      }
    }
    int mine;
    if (!literal(out, mine)) return false;
    if (vis >= 0 && vis != mine) return fail("an entry's literals differ in visibility");
    vis = mine; return true;
  }
};

// The record of a string of n characters; false: `why` says what is wrong
static bool parse(Parsed& r, const char* s, size_t n, std::string& why) {
  Reader R{s, n};
  auto refuse = [&](const std::string& w) { R.fail(w); why = R.why; return false; };
  r = Parsed();
  if (!R.eat('{')) return refuse("no opening brace");
  if (R.word() != "owner" || !R.eat(':')) return refuse("the first entry is not the owner");
  Value v; int vis = -1;
  R.ws();
  if (!R.literal(v, vis)) return refuse("");
  if (v.type != 0 || vis == 0) return refuse("the owner is not a public or private address");
  r.owner_kind = vis == 2; std::memcpy(r.owner, v.v, 32);
  if (!R.eat(',')) return refuse("no comma behind the owner");
  for (;;) {
    R.ws();
    if (R.starts("_nonce")) {
      R.at += 6;
      if (!R.eat(':')) return refuse("the nonce has no value");
      R.ws();
      if (!R.literal(v, vis)) return refuse("");
      if (v.type != 3 || vis != 1) return refuse("the nonce is not a public group element");
      std::memcpy(r.nonce, v.v, 32);
      break;
    }
    Entry e; e.name = R.word();
    if (!serial::identifier_ok(e.name.data(), e.name.size())) return refuse("an entry has no valid name");
    if (e.name == "owner") return refuse("an entry is named owner");
    for (const Entry& o : r.entries) if (o.name == e.name) return refuse("duplicate entry '" + e.name + "'");
    if (r.entries.size() == MAX_ENTRIES) return refuse("more than 255 entries");
    if (!R.eat(':')) return refuse("entry '" + e.name + "' has no value");
    vis = -1;
    if (!R.value(e.value, vis, 0)) return refuse("");
    e.visibility = (uint8_t)vis;
    if (!R.eat(',')) return refuse("no comma behind entry '" + e.name + "'");
    r.entries.push_back(std::move(e));
  }
  if (!R.eat('}')) return refuse("no closing brace");
  R.ws();
  if (R.at != n) return refuse("trailing text");
  return true;
}

// a value's bits; false: a struct member longer than a u16 says
static bool value_bits(std::vector<uint8_t>& out, const Value& v) {
  if (!v.is_struct) {
    serial::push_bits(out, 0, 2); serial::push_bits(out, v.type, 8);
    if (v.type == 15) { serial::push_bits(out, 8 * v.text.size(), 16); serial::push_bytes(out, (const uint8_t*)v.text.data(), v.text.size()); return true; }
    const int bits = plaintext::literal_bits(v.type);
    serial::push_bits(out, (uint64_t)bits, 16);
    for (int i = 0; i < bits; ++i) out.push_back((v.v[i >> 6] >> (i & 63)) & 1);
    return true;
  }
  out.push_back(0); out.push_back(1); serial::push_bits(out, v.members.size(), 8);
  for (const auto& m : v.members) {
    serial::push_bits(out, 8 * m.first.size(), 8); serial::push_bytes(out, (const uint8_t*)m.first.data(), m.first.size());
    std::vector<uint8_t> inner;
    if (!value_bits(inner, m.second) || inner.size() > 65535) return false;
    serial::push_bits(out, inner.size(), 16); out.insert(out.end(), inner.begin(), inner.end());
  }
  return true;
}

// RECORD BITS, appended to `bits`, exactly as serial::record_bits lays them out
static bool record_bits(std::vector<uint8_t>& bits, const Parsed& r, std::string& why) {
  uint64_t v[4];
  bits.push_back(r.owner_kind == 1);
  std::memcpy(v, r.owner, 32); serial::push_field_bits(bits, v);
  std::vector<uint8_t> data;
  for (const Entry& e : r.entries) {
    serial::push_bytes(data, (const uint8_t*)e.name.data(), e.name.size());
    data.push_back(e.visibility == 2); data.push_back(e.visibility == 1);
    if (!value_bits(data, e.value)) { why = "entry '" + e.name + "': a member is longer than 65535 bits"; return false; }
  }
  serial::push_bits(bits, data.size(), 32);
  bits.insert(bits.end(), data.begin(), data.end());
  std::memcpy(v, r.nonce, 32); serial::push_field_bits(bits, v);
  return true;
}

// RecordPlaintext.microcredits(): the value of a top-level u64 entry of that name, else 0
static uint64_t microcredits(const Parsed& r) {
  for (const Entry& e : r.entries) if (e.name == "microcredits") return !e.value.is_struct && e.value.type == 12 ? e.value.v[0] : 0;
  return 0;
}

}}  // namespace aleo_mi355x::ptext
