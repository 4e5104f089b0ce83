// plaintexts_lane.h — what ONE lane of the plaintext kernel computes (plaintexts.hip launches it, one RecordPlaintext string per lane): the commitment
// Record<N, Plaintext<N>>::to_commitment(program_id, record_name) of the record the string says, byte for byte plaintext_parse.hpp's parse + record_bits and
// serial_host.hpp's BHP1024 — and the record's microcredits.  The hashing is records_commit_lane.h's commit_hash; this file is its second item source, over text.
//
// The lane COMPUTES OR ROUTES; it never refuses.  It computes a record whose entries are all numeric, boolean or address literals spelled as plaintext::render
// prints them, of at most PT_MAX_CHARS characters and PT_MAX_ENTRIES entries; whitespace (space, tab, CR, LF) may stand wherever plaintext_parse.hpp lets it.
// Everything else is ROUTED (COMMIT_ROUTED, which never leaves the library), and the calling thread computes or refuses that row with the host code:
//   a struct or a quoted string; a number with a leading zero, an underscore, "-0" or more than 77 digits; a sign on a type that has none; a value not below its
//   modulus or out of its type's range; an address whose characters, checksum or padding are not in order; a name that is no identifier or is `owner`; two names
//   of one length and one 32-bit hash (which is how duplicates are found: equal names are routed, and so is the rare pair that only collides); a string over the
//   caps; anything else that is not the grammar.
// Two walks, as records_commit_lane.h's: pt_measure reads the whole string, checks everything above and sums the data bits (which depend on names and literal
// types only); pt_next hands out the message in order as items of at most 256 bits — the owner, the u32 length, per entry the name's bytes, the 2 visibility
// bits with the literal's header (00 | u8 type | u16 size), the value — then the nonce.  Both read a field — the owner, an entry, the nonce — through the ONE pt_field / pt_literal.
// Decimal text becomes eight 32-bit words by multiply-by-10-and-add; ranges and moduli are compared in words; -…i8 .. i128 become two's complement.
// Plain C++: no thread index, the characters come through a callable, so tests/cpp/plaintexts_lane_emul.cpp runs it on the host.
#pragma once
#include "records_strings_lane.h"
#include "records_commit_lane.h"

namespace aleo_mi355x {

static constexpr uint32_t PT_MAX_CHARS = 1024, PT_MAX_ENTRIES = 8, PT_MAX_DIGITS = 77, PT_ADDRESS_CHARS = 63;
static constexpr uint32_t PT_ALEO_STATE = rs_polymod_prefix("aleo");
// the scalar field's modulus, in little-endian words (plaintext::SCALAR_MODULUS)
static constexpr uint32_t PT_SCALAR_WORDS[8] = {0xc33fd9ffu, 0xb95aee9au, 0xc43c8afeu, 0x5293a3afu, 0x970dec00u, 0x982d1347u, 0xa68b2955u, 0x04aad957u};

__host__ __device__ __forceinline__ bool pt_is_ws(uint32_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
__host__ __device__ __forceinline__ bool pt_is_digit(uint32_t c) { return c - '0' < 10u; }
__host__ __device__ __forceinline__ bool pt_is_letter(uint32_t c) { return (c | 32u) - 'a' < 26u; }
__host__ __device__ __forceinline__ bool pt_is_word(uint32_t c) { return pt_is_digit(c) || pt_is_letter(c) || c == '_'; }
__host__ __device__ __forceinline__ bool pt_below(const uint32_t (&w)[8], const uint32_t (&m)[8]) {
  bool below = false, decided = false;
#pragma unroll
  for (int q = 7; q >= 0; --q) if (!decided && w[q] != m[q]) { below = w[q] < m[q]; decided = true; }
  return below;
}
__host__ __device__ __forceinline__ uint32_t pt_literal_bits(uint32_t type) {
  return type == 1 ? 1u : type == 14 ? 251u : type >= 9 && type <= 13 ? 8u << (type - 9) : type >= 4 && type <= 8 ? 8u << (type - 4) : 253u;
}

// c(i): character i, 0 at and behind the end
template <class Ch> __host__ __device__ __forceinline__ void pt_skip_ws(Ch&& c, uint32_t& at) { while (pt_is_ws(c(at))) ++at; }
template <class Ch> __host__ __device__ __forceinline__ bool pt_punct(Ch&& c, uint32_t& at, uint32_t which) {      // whitespace, then the one character
  pt_skip_ws(c, at);
  if (c(at) != which) return false;
  ++at; return true;
}
// the run of word characters (letters, digits, underscores) from `at` on: its first eight packed little-endian into two words (32-bit compares take their
// constant as a literal; a 64-bit one would hold a pair of scalar registers per keyword), its length
struct PtWord { uint32_t lo, hi, n; };
template <class Ch> __host__ __device__ __forceinline__ PtWord pt_word(Ch&& c, uint32_t& at) {
  PtWord w{0, 0, 0};
  for (; pt_is_word(c(at)); ++w.n, ++at) { if (w.n < 4) w.lo |= c(at) << (8 * w.n); else if (w.n < 8) w.hi |= c(at) << (8 * (w.n - 4)); }
  return w;
}
constexpr uint32_t pt_pack(const char* s, int from) { uint32_t v = 0; int n = 0; while (s[n]) ++n; for (int i = from; i < from + 4 && i < n; ++i) v |= (uint32_t)(uint8_t)s[i] << (8 * (i - from)); return v; }
#define PT_IS(w, text) ((w).lo == pt_pack(text, 0) && (w).hi == pt_pack(text, 4) && (w).n == sizeof(text) - 1)

// "<literal>.<visibility>" from `at` on, in render's spelling: its type, its value's words (two's complement for the signed types), its visibility (0 constant,
// 1 public, 2 private); false: route
template <class Ch>
__host__ __device__ __forceinline__ bool pt_literal(Ch&& c, uint32_t& at, uint32_t& type, uint32_t (&v)[8], uint32_t& vis) {
  constexpr RsSymbols T = rs_symbols();
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = 0;
  const uint32_t c0 = c(at);
  if (c0 == 'a') {                                             // "aleo1" and 58 symbols: 52 of data (the last one's low 4 bits are padding), 6 of checksum
    const char prefix[6] = "aleo1";
    bool ok = true;
    for (uint32_t i = 0; i < 5; ++i) ok = ok && c(at + i) == (uint32_t)(uint8_t)prefix[i];
    uint32_t chk = PT_ALEO_STATE;
    for (uint32_t k = 5; k < PT_ADDRESS_CHARS; ++k) {
      const uint32_t x = c(at + k);
      const int32_t s = x < 128 ? T.of[x] : -1;
      ok = ok && s >= 0;
      chk = rs_polymod_step(chk, (uint32_t)s & 31u);
    }
    const uint32_t first = at + 5;
    auto sym = [&](uint32_t k) { return (uint32_t)T.of[c(first + k) & 127u] & 31u; };
    ok = ok && chk == RS_BECH32M && !(sym(51) & 15u);
    ok = rs_field_at(sym, 0, v) && ok;
    at += PT_ADDRESS_CHARS;
    if (!ok || pt_is_word(c(at))) return false;
    type = 0;
  } else {
    const bool negative = c0 == '-';
    if (negative) ++at;
    const bool number = pt_is_digit(c(at));
    if ((negative && !number) || (c(at) == '0' && (negative || pt_is_digit(c(at + 1))))) return false;      // a sign alone; a leading zero; "-0"
    uint32_t digits = 0, carry = 0;
    for (; pt_is_digit(c(at)); ++at, ++digits) {
      uint32_t in = c(at) - '0';
#pragma unroll
      for (int q = 0; q < 8; ++q) { const uint64_t t = (uint64_t)v[q] * 10u + in; v[q] = (uint32_t)t; in = (uint32_t)(t >> 32); }
      carry |= in;                                             // cannot happen below 78 digits: 10^77 < 2^256
    }
    if (digits > PT_MAX_DIGITS || carry) return false;
    const PtWord word = pt_word(c, at);                        // true, false, or the suffix: field, group, scalar, i8 .. i128, u8 .. u128
    if (!number) {
      if (PT_IS(word, "true")) v[0] = 1; else if (!PT_IS(word, "false")) return false;
      type = 1;
    } else {
      type = PT_IS(word, "field") ? 2u : PT_IS(word, "group") ? 3u : PT_IS(word, "scalar") ? 14u : PT_IS(word, "i8") ? 4u : PT_IS(word, "i16") ? 5u : PT_IS(word, "i32") ? 6u :
             PT_IS(word, "i64") ? 7u : PT_IS(word, "i128") ? 8u : PT_IS(word, "u8") ? 9u : PT_IS(word, "u16") ? 10u : PT_IS(word, "u32") ? 11u : PT_IS(word, "u64") ? 12u :
             PT_IS(word, "u128") ? 13u : 0u;
      if (!type) return false;
    }
    const bool is_signed = type >= 4 && type <= 8;
    if (negative && !is_signed) return false;
    // what the magnitude is below: r, the scalar field's modulus, 2^bits, 2^(bits - 1) — or that itself behind a sign
    const uint32_t bits = pt_literal_bits(type), top = is_signed ? bits - 1 : bits;
    const bool by_modulus = type == 2 || type == 3 || type == 14;
    uint32_t lim[8];
    bool equal = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      lim[q] = by_modulus ? (type == 14 ? PT_SCALAR_WORDS[q] : RS_FR_WORDS[q]) : (uint32_t)q == (top >> 5) ? 1u << (top & 31u) : 0u;
      equal = equal && v[q] == lim[q];
    }
    if (type != 1 && !(pt_below(v, lim) || (negative && equal))) return false;
    if (negative) {                                            // two's complement of `bits` bits
      uint32_t cy = 1;
#pragma unroll
      for (int q = 0; q < 4; ++q) { const uint64_t t = (uint64_t)(~v[q]) + cy; v[q] = (uint32_t)t; cy = (uint32_t)(t >> 32); }
      if (bits < 32) v[0] &= (1u << bits) - 1u;
#pragma unroll
      for (int q = 1; q < 4; ++q) if (32u * (uint32_t)q >= bits) v[q] = 0;
    }
  }
  if (c(at) != '.') return false;
  ++at;
  const PtWord word = pt_word(c, at);
  vis = PT_IS(word, "private") ? 2u : PT_IS(word, "public") ? 1u : 0u;
  return vis || PT_IS(word, "constant");
}

// One field of the record, "<name> : <literal>.<visibility>" from `at` on (whitespace skipped first): where the name — a run of word characters — stands and
// how long it is.  The owner and the nonce are fields too, which is why the ONE call of pt_literal is here.  false: route
struct PtField { uint32_t name_at, name_len, type, vis, v[8]; };
template <class Ch>
__host__ __device__ __forceinline__ bool pt_field(Ch&& c, uint32_t& at, PtField& F) {
  pt_skip_ws(c, at);
  F.name_at = at;
  while (pt_is_word(c(at))) ++at;
  F.name_len = at - F.name_at;
  if (!pt_punct(c, at, ':')) return false;
  pt_skip_ws(c, at);
  return pt_literal(c, at, F.type, F.v, F.vis);
}

// What the first walk leaves for the second
struct PtMeasure { uint32_t first_at, entries, data_bits; uint64_t microcredits; };

// The first walk over a string of `len` characters: everything the lane verifies.  Field 0 is the owner, fields 1 .. entries the entries, the last one the nonce.
// visit(F, which): every field once it has passed its checks, in order — which PT_OWNER, PT_ENTRY or PT_NONCE (records_encrypt_lane.h sizes its output there).
// false: route
static constexpr uint32_t PT_OWNER = 0, PT_ENTRY = 1, PT_NONCE = 2;
template <class Ch, class Visit>
__host__ __device__ __forceinline__ bool pt_measure(Ch&& c, uint32_t len, PtMeasure& M, Visit&& visit) {
  if (len > PT_MAX_CHARS) return false;
  uint32_t at = 0, hashes[PT_MAX_ENTRIES];
#pragma unroll
  for (uint32_t q = 0; q < PT_MAX_ENTRIES; ++q) hashes[q] = 0;
  M.entries = 0; M.data_bits = 0; M.microcredits = 0;
  if (!pt_punct(c, at, '{')) return false;
  M.first_at = at;
  for (uint32_t k = 0;; ++k) {
    PtField F;
    if (!pt_field(c, at, F)) return false;
    uint32_t h = 0x811c9dc5u ^ F.name_len;                     // FNV-1a over the length and the bytes; bit 31 set, so never the 0 of an empty place
    for (uint32_t i = 0; i < F.name_len; ++i) h = (h ^ c(F.name_at + i)) * 0x01000193u;
    h |= 0x80000000u;
    uint32_t name_at = F.name_at;
    const PtWord name = pt_word(c, name_at);                   // its first eight characters
    const bool is_owner = PT_IS(name, "owner"), is_nonce = PT_IS(name, "_nonce");
    if (k == 0) {
      if (!is_owner || F.type != 0 || F.vis == 0 || !pt_punct(c, at, ',')) return false;
      visit(F, PT_OWNER);
      continue;
    }
    if (is_nonce) {
      if (F.type != 3 || F.vis != 1 || !pt_punct(c, at, '}')) return false;
      visit(F, PT_NONCE);
      break;
    }
    if (is_owner || F.name_len > 31 || !pt_is_letter(c(F.name_at)) || M.entries == PT_MAX_ENTRIES || !pt_punct(c, at, ',')) return false;
    bool seen = false;
#pragma unroll
    for (uint32_t q = 0; q < PT_MAX_ENTRIES; ++q) { seen = seen || hashes[q] == h; if (q == M.entries) hashes[q] = h; }
    if (seen) return false;
    name_at = F.name_at + 8;
    const PtWord tail = pt_word(c, name_at);
    if (name.lo == pt_pack("microcre", 0) && name.hi == pt_pack("microcre", 4) && name.n == 12 && PT_IS(tail, "dits") && F.type == 12) M.microcredits = (uint64_t)F.v[0] | (uint64_t)F.v[1] << 32;
    M.data_bits += 8u * F.name_len + 2u + 26u + pt_literal_bits(F.type);
    ++M.entries;
    visit(F, PT_ENTRY);
  }
  pt_skip_ws(c, at);
  return at == len;
}
template <class Ch> __host__ __device__ __forceinline__ bool pt_measure(Ch&& c, uint32_t len, PtMeasure& M) { return pt_measure(c, len, M, [](const PtField&, uint32_t) {}); }

// The second walk: the message behind the names, item by item, of a string pt_measure accepted
struct PtWalk { uint32_t stage, at, k; PtField F; };
static constexpr uint32_t PW_OWNER = 0, PW_LENGTH = 1, PW_FIELD = 2, PW_HEADER = 3, PW_VALUE = 4, PW_DONE = 5;

template <class Ch>
__host__ __device__ __forceinline__ bool pt_next(PtWalk& W, Ch&& c, const PtMeasure& M, uint32_t (&w)[8], uint32_t& nbits) {
  if (W.stage == PW_LENGTH) { w[0] = M.data_bits; nbits = 32; W.stage = PW_FIELD; return true; }
  if (W.stage == PW_HEADER) {                                  // visibility (private 1 0, public 0 1, constant 0 0) | 00 | u8 type | u16 size
    w[0] = (W.F.vis == 2 ? 1u : 0u) | (W.F.vis == 1 ? 2u : 0u) | (W.F.type << 4) | (pt_literal_bits(W.F.type) << 12);
    nbits = 28; W.stage = PW_VALUE; return true;
  }
  if (W.stage == PW_VALUE) {
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = W.F.v[q];
    nbits = pt_literal_bits(W.F.type); W.stage = PW_FIELD; return true;
  }
  if (W.stage == PW_DONE) return false;
  if (W.stage == PW_OWNER) { W.at = M.first_at; W.k = 0; }
  (void)pt_field(c, W.at, W.F);                                // the owner, an entry or the nonce
  if (W.stage == PW_OWNER) {                                   // 1 for a private owner | the address x
    w[0] = (W.F.vis == 2 ? 1u : 0u) | (W.F.v[0] << 1);
#pragma unroll
    for (int q = 1; q < 8; ++q) w[q] = (W.F.v[q - 1] >> 31) | (W.F.v[q] << 1);
    nbits = 254; (void)pt_punct(c, W.at, ','); W.stage = PW_LENGTH; return true;
  }
  if (W.k == M.entries) {                                      // the nonce
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = W.F.v[q];
    nbits = 253; W.stage = PW_DONE; return true;
  }
  (void)pt_punct(c, W.at, ',');
#pragma unroll
  for (int q = 0; q < 8; ++q) {                                // the name: at most 31 bytes
    uint32_t x = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) if (4u * (uint32_t)q + b < W.F.name_len) x |= c(W.F.name_at + 4u * (uint32_t)q + b) << (8 * b);
    w[q] = x;
  }
  nbits = 8 * W.F.name_len; ++W.k; W.stage = PW_HEADER; return true;
}

// One string.  ch(i): character i of its `len` (never asked for at or behind the end).  Returns COMMIT_OK, with `emit` handed the canonical limbs of the
// commitment and `microcredits` set, or COMMIT_ROUTED.
template <class LoadChar, class Emit>
__device__ __forceinline__ uint32_t plaintexts_commit_lane(LoadChar&& ch, uint32_t len, const uint32_t* __restrict__ K, const CommitArgs& A, uint64_t& microcredits, Emit&& emit) {
  auto c = [&](uint32_t i) { return i < len ? (uint32_t)(uint8_t)ch(i) : 0u; };
  PtMeasure M;
  if (!pt_measure(c, len, M)) return COMMIT_ROUTED;
  PtWalk W{}; W.stage = PW_OWNER;
  emit(commit_hash([&](uint32_t (&w)[8], uint32_t& nbits) { return pt_next(W, c, M, w, nbits); }, A.name_bits + 254u + 32u + M.data_bits + 253u, K, A));
  microcredits = M.microcredits;
  return COMMIT_OK;
}

}  // namespace aleo_mi355x
