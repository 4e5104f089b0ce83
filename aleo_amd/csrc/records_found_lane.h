// records_found_lane.h — what ONE lane computes of an owned record's private fields (records_found.hip launches it, one "record1…" string per lane, and runs
// the same functions on the calling thread as its host path): the walk of records_plaintext.hpp::parse and gather_fields over the string's symbols, and the
// `microcredits` entry of RecordPlaintext.microcredits (aleo_amd/records.py).
//
// The string has passed records_parse_lane (records_strings_lane.h): its characters are symbols, the checksum holds and the entries end where the nonce begins,
// so the walk cannot leave the payload.  What is left to refuse is what aleo_mi355x_record_fields refuses on top of that (status FOUND_REFUSED):
//   an entry without a valid name ([0-9a-zA-Z_]+), of no bytes, or of a visibility above 2; a private entry shorter than its u16 field count, of a byte length
//   that is not 3 + 32 x count, or holding a field that is not below r.
// The private fields in randomizer order: the owner's one field if the owner is private, then every private entry's, in entry order.
//
// One function walks; what it does with a field is the caller's `emit` (nothing when counting, a store when gathering).  The entry named microcredits — the
// last of them, as a dict keeps the last of two equal names — is noted on the way:
//   private: where its fields lie among the record's; found_microcredits_private reads the value from the DECRYPTED fields (PLAINTEXT BITS: variant 00,
//            type 12, size 64, 64 value bits, the terminus, zeros up to bit 252 of every field), 0 for anything else;
//   constant or public: PLAINTEXT BYTES of exactly 11 bytes, variant 0, u16 type 12, 8 value bytes; 0 for anything else.
// Only that entry is looked at: a record whose OTHER entries record_plaintext cannot render still reports its microcredits here.
// Plain C++: no thread index, the characters come through a callable, so tests/cpp/records_found_lane_emul.cpp runs it on the host.
#pragma once
#include "records_symbols_lane.h"

namespace aleo_mi355x {

static constexpr uint32_t FOUND_OK = 0, FOUND_MALFORMED = 2, FOUND_REFUSED = 4;
static constexpr uint32_t FOUND_MC_NONE = 0, FOUND_MC_PRIVATE = 1, FOUND_MC_PUBLIC = 2;

struct FoundWalk {
  uint32_t fields, status;                                   // status: FOUND_OK or FOUND_REFUSED (then fields = 0)
  uint32_t mc_kind, mc_at, mc_n;                             // private: fields mc_at .. mc_at + mc_n of the record
  uint64_t mc_value;                                         // public: the value
};

// One accepted string of `len` characters, character i through ch(i); kind: its owner variant (0 public, 1 private).  emit(k, w): field k of the record, its
// canonical little-endian words — called in order, possibly before a later entry refuses the record.
template <class LoadChar, class Emit>
__host__ __device__ __forceinline__ FoundWalk records_found_walk(LoadChar&& ch, uint32_t len, int32_t kind, Emit&& emit) {
  constexpr RsSymbols T = rs_symbols();
  auto sym = [&](uint32_t k) { return (uint32_t)T.of[(uint8_t)ch(RS_PREFIX_CHARS + k) & 127u] & 31u; };
  auto byte_at = [&](uint32_t j) { return rs_byte_at(sym, j); };
  FoundWalk r{0, FOUND_OK, FOUND_MC_NONE, 0, 0, 0};
  auto refuse = [&]() { r.fields = 0; r.status = FOUND_REFUSED; r.mc_kind = FOUND_MC_NONE; r.mc_at = r.mc_n = 0; r.mc_value = 0; return r; };
  (void)len;
  uint32_t w[8];
  uint32_t at = kind == 1 ? 3u : 1u;
  if (kind == 1) { rs_field_at(sym, at, w); emit(r.fields++, w); }
  at += 32;
  const uint32_t entries = byte_at(at++);
  const char want[13] = "microcredits";
  for (uint32_t e = 0; e < entries; ++e) {
    const uint32_t nl = byte_at(at++);
    if (!nl) return refuse();
    bool named = nl == 12;
    for (uint32_t i = 0; i < nl; ++i) {
      const uint32_t c = byte_at(at + i);
      if (!((c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_')) return refuse();
      if (named && c != (uint32_t)(uint8_t)want[i]) named = false;      // i < 12 while named
    }
    at += nl;
    const uint32_t el = byte_at(at) | (byte_at(at + 1) << 8); at += 2;
    if (el < 1) return refuse();
    const uint32_t vis = byte_at(at);
    if (vis > 2) return refuse();
    if (vis == 2) {
      if (el < 3) return refuse();
      const uint32_t nf = byte_at(at + 1) | (byte_at(at + 2) << 8);
      if (el != 3u + 32u * nf) return refuse();
      if (named) { r.mc_kind = FOUND_MC_PRIVATE; r.mc_at = r.fields; r.mc_n = nf; r.mc_value = 0; }
      for (uint32_t i = 0; i < nf; ++i) {
        if (!rs_field_at(sym, at + 3 + 32 * i, w)) return refuse();
        emit(r.fields++, w);
      }
    } else if (named) {
      r.mc_kind = FOUND_MC_PUBLIC; r.mc_at = r.mc_n = 0; r.mc_value = 0;
      if (el == 12 && byte_at(at + 1) == 0 && byte_at(at + 2) == 12 && byte_at(at + 3) == 0)
        for (uint32_t i = 0; i < 8; ++i) r.mc_value |= (uint64_t)byte_at(at + 4 + i) << (8 * i);
    }
    at += el;
  }
  return r;
}

// The u64 of a private entry of n >= 1 decrypted fields, field i's little-endian words through load(i, w); 0 unless the entry's bits are exactly a u64 literal.
template <class LoadField>
__host__ __device__ __forceinline__ uint64_t found_microcredits_private(uint32_t n, LoadField&& load) {
  if (!n) return 0;
  uint32_t w[8];
  for (uint32_t i = 1; i < n; ++i) {                          // nothing but zeros behind the terminus, in the 252 data bits of every field
    load(i, w);
    uint32_t any = w[7] & 0x0fffffffu;
    for (int q = 0; q < 7; ++q) any |= w[q];
    if (any) return 0;
  }
  load(0, w);
  // bits 0-1 variant 00 | 2-9 type 12 | 10-25 size 64 | 26-89 the value | 90 the terminus | 91-251 zeros
  const uint64_t lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32), hi = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
  if ((lo & 0x3ffffffu) != ((12u << 2) | (64u << 10))) return 0;
  if ((hi >> 26) != 1u) return 0;
  if (w[4] | w[5] | w[6] | (w[7] & 0x0fffffffu)) return 0;
  return (lo >> 26) | (hi << 38);
}

}  // namespace aleo_mi355x
