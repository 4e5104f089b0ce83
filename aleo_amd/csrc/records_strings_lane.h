// records_strings_lane.h — what ONE lane of the record-string parse computes (records_strings.hip launches it, one "record1…" string per lane, and runs the
// same function on the calling thread as its host path): the bech32m decode, the checksum and the layout walk of aleo_mi355x_record_parse (wire.hip), which it
// accepts and refuses string for string [the layout: UPSTREAM-RECALL in wire.hip; pinned by tests/golden/reference_records.json].
//
//   "record1" | D data symbols | 6 checksum symbols, every symbol one of qpzry9x8gf2tvdw0s3jn54khce6mua7l (lower case only: wire.hip looks a character up in
//   that alphabet and nowhere else).  '1' is not in the alphabet, so "the last '1' ends the prefix and the prefix is `record`" is "the string starts with
//   record1 and no other '1' follows"; a NUL or any other byte outside the alphabet refuses the same way.
//   payload = floor(5 D / 8) bytes, the 5 D mod 8 bits left over fewer than 5 and zero:
//   u8 owner variant (0 public | 1 private: u16 field count = 1) | 32 B owner field, canonical | u8 entry count | per entry: u8 name length, name, u16 byte
//   length, that many bytes | 32 B nonce x, canonical | end.
//
// Two passes over the characters and no buffer.  The first folds every symbol into the checksum, starting from the state after the expanded prefix (a compile-time
// constant), and notes a character outside the alphabet.  The second walks the layout through byte_at(j) (records_symbols_lane.h), which reads the two or three
// symbols that cover payload byte j: the walk touches the count and length bytes and the two fields, a few dozen bytes of a record, whatever the entries hold.  A wave runs to its longest
// string; strings are not sorted by length (a wave's cost is its longest lane's either way, and an order costs a pass and a gather).
// Plain C++: no thread index, the characters come through a callable, so tests/cpp/records_strings_lane_emul.cpp runs it on the host.
#pragma once
#include "records_symbols_lane.h"

namespace aleo_mi355x {

static constexpr uint32_t RS_BECH32M = 0x2bc830a3u;

constexpr uint32_t rs_polymod_step(uint32_t chk, uint32_t v) {
  const uint32_t b = chk >> 25;
  return ((chk & 0x1ffffffu) << 5) ^ v ^ ((b & 1u) ? 0x3b6a57b2u : 0u) ^ ((b & 2u) ? 0x26508e6du : 0u) ^ ((b & 4u) ? 0x1ea119fau : 0u) ^ ((b & 8u) ? 0x3d4233ddu : 0u) ^
         ((b & 16u) ? 0x2a1462b3u : 0u);
}
// the checksum state after the expanded prefix: the high bits of every character, a zero, the low bits of every character
constexpr uint32_t rs_polymod_prefix(const char* hrp) {
  uint32_t chk = 1;
  for (const char* p = hrp; *p; ++p) chk = rs_polymod_step(chk, (uint32_t)(unsigned char)*p >> 5);
  chk = rs_polymod_step(chk, 0);
  for (const char* p = hrp; *p; ++p) chk = rs_polymod_step(chk, (uint32_t)(unsigned char)*p & 31u);
  return chk;
}
static constexpr uint32_t RS_PREFIX_STATE = rs_polymod_prefix("record");

// One string of `len` characters, character i through ch(i) (0 <= i < len, asked for in any order and more than once).  Returns the owner variant (0 public,
// 1 private) with the canonical words of the owner field and of the nonce x, or -1 for a string aleo_mi355x_record_parse refuses, both rows zeros.
template <class LoadChar>
__host__ __device__ __forceinline__ int32_t records_parse_lane(LoadChar&& ch, uint32_t len, uint32_t (&owner)[8], uint32_t (&nonce)[8]) {
  constexpr RsSymbols T = rs_symbols();
  for (int q = 0; q < 8; ++q) owner[q] = nonce[q] = 0;
  if (len < RS_PREFIX_CHARS + RS_CHECKSUM_SYMBOLS || len > RS_MAX_CHARS) return -1;      // the empty string, "record" without its '1', fewer than 6 symbols
  const char prefix[RS_PREFIX_CHARS + 1] = "record1";
  bool ok = true;
  for (uint32_t i = 0; i < RS_PREFIX_CHARS; ++i) ok = ok && (uint8_t)ch(i) == (uint8_t)prefix[i];
  if (!ok) return -1;
  const uint32_t n_sym = len - RS_PREFIX_CHARS, D = n_sym - RS_CHECKSUM_SYMBOLS;
  auto sym = [&](uint32_t k) { return (uint32_t)T.of[(uint8_t)ch(RS_PREFIX_CHARS + k) & 127u] & 31u; };      // of a string whose characters passed the first pass
  uint32_t chk = RS_PREFIX_STATE;
  for (uint32_t k = 0; k < n_sym; ++k) {
    const uint8_t c = (uint8_t)ch(RS_PREFIX_CHARS + k);
    const int32_t s = c < 128 ? T.of[c] : -1;
    ok = ok && s >= 0;
    chk = rs_polymod_step(chk, (uint32_t)s & 31u);
  }
  if (!ok || chk != RS_BECH32M) return -1;
  const uint32_t left = (5u * D) & 7u, nb = (5u * D) >> 3;      // D <= 2^20: no overflow
  if (left >= 5 || (left && (sym(D - 1) & ((1u << left) - 1u)))) return -1;
  auto byte_at = [&](uint32_t j) { return rs_byte_at(sym, j); };                    // records_symbols_lane.h
  // 32 bytes from byte j on, as little-endian words: the symbols are read once each, in order; returns whether the value is below r
  auto field = [&](uint32_t j, uint32_t (&w)[8]) {
    uint32_t k = (8u * j) / 5u;
    const uint32_t o = 8u * j - 5u * k;
    uint32_t bits = 5u - o, acc = sym(k++) & ((1u << bits) - 1u);
    for (int q = 0; q < 8; ++q) {
      uint32_t word = 0;
      for (int b = 0; b < 4; ++b) {
        while (bits < 8) { acc = (acc << 5) | sym(k++); bits += 5; }
        bits -= 8;
        word |= ((acc >> bits) & 0xffu) << (8 * b);
        acc &= (1u << bits) - 1u;
      }
      w[q] = word;
    }
    bool below = false, decided = false;
    for (int q = 7; q >= 0; --q) { if (!decided && w[q] != RS_FR_WORDS[q]) { below = w[q] < RS_FR_WORDS[q]; decided = true; } }
    return below;
  };
  uint32_t at = 0;
  auto need = [&](uint32_t k) { return at + k <= nb; };      // at <= nb <= 2^20 and k < 2^17: no overflow
  auto refuse = [&]() { for (int q = 0; q < 8; ++q) owner[q] = nonce[q] = 0; return -1; };
  if (!need(1)) return refuse();
  const uint32_t kind = byte_at(at++);
  if (kind > 1) return refuse();
  if (kind == 1) {
    if (!need(2)) return refuse();
    const uint32_t cnt = byte_at(at) | (byte_at(at + 1) << 8); at += 2;
    if (cnt != 1) return refuse();                             // a private owner is a ciphertext of one field
  }
  if (!need(32)) return refuse();
  if (!field(at, owner)) return refuse();
  at += 32;
  if (!need(1)) return refuse();
  const uint32_t entries = byte_at(at++);
  for (uint32_t e = 0; e < entries; ++e) {
    if (!need(1)) return refuse();
    const uint32_t nl = byte_at(at++);
    if (!need(nl + 2)) return refuse();
    at += nl;
    const uint32_t el = byte_at(at) | (byte_at(at + 1) << 8); at += 2;
    if (!need(el)) return refuse();
    at += el;
  }
  if (!need(32)) return refuse();
  if (!field(at, nonce)) return refuse();
  at += 32;
  if (at != nb) return refuse();                               // trailing bytes
  return (int32_t)kind;
}

}  // namespace aleo_mi355x
