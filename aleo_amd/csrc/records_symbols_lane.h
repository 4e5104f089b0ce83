// records_symbols_lane.h — reading payload bytes out of the bech32 symbols of a "record1…" string, for the lane functions that walk a record's layout
// without decoding it into a buffer: records_strings_lane.h (the parse) and records_found_lane.h (the private fields of an owned record).
// Plain C++: the symbols come through a callable sym(k) -> 0..31, k counted from the first data symbol.
#pragma once
#include <cstdint>

namespace aleo_mi355x {

static constexpr uint32_t RS_MAX_CHARS = 1u << 20;            // a longer string is refused (wire.hip: "record_parse: string too long")
static constexpr uint32_t RS_PREFIX_CHARS = 7, RS_CHECKSUM_SYMBOLS = 6;
// r, in little-endian words
static constexpr uint32_t RS_FR_WORDS[8] = {0x00000001u, 0x0a118000u, 0xd0000001u, 0x59aa76feu, 0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu};

// character -> symbol, -1 outside the alphabet
struct RsSymbols { int8_t of[128]; };
constexpr RsSymbols rs_symbols() {
  RsSymbols t{};
  for (int i = 0; i < 128; ++i) t.of[i] = -1;
  const char* alphabet = "qpzry9x8gf2tvdw0s3jn54khce6mua7l";
  for (int i = 0; i < 32; ++i) t.of[(unsigned char)alphabet[i]] = (int8_t)i;
  return t;
}

// payload byte j lies in symbols k = floor(8 j / 5) .. k + 2; k + 2 may be a checksum symbol, whose bits the shift drops
template <class Sym>
__host__ __device__ __forceinline__ uint32_t rs_byte_at(Sym&& sym, uint32_t j) {
  const uint32_t k = (8u * j) / 5u, o = 8u * j - 5u * k;
  uint32_t v = (sym(k) << 10) | (sym(k + 1) << 5);
  if (o >= 3) v |= sym(k + 2);
  return (v >> (7u - o)) & 0xffu;
}

// 32 bytes from byte j on, as little-endian words: the symbols are read once each, in order; returns whether the value is below r
template <class Sym>
__host__ __device__ __forceinline__ bool rs_field_at(Sym&& sym, uint32_t j, uint32_t (&w)[8]) {
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
}

}  // namespace aleo_mi355x
