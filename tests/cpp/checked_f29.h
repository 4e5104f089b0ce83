// The 29-bit-limb field of the device lanes (aleo_amd/csrc/fr29.h) for the programs that run a lane on the HOST (tests/cpp/*_lane_emul.cpp): restated in plain C++
// with every operand rule of its header turned into a check — a product's multiplicand has limbs below 2^31.4, its multiplier is normalised, its column sums fit
// 64 bits; a padded difference never borrows; a lazy sum never wraps — so a lane's code is exercised, limb for limb, without a GPU, and a broken bound shows as a
// count (g_violations) instead of as a wrong flag one record in a million.  With it: the qualifiers of device code defined away, the library's host path
// (records_host.hpp, which takes this F29 for the lanes it includes), the programs' generator of field elements, and the opening of a program's case file.
// One program includes it once; it builds under g++ and under hipcc -x c++.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__

static unsigned long g_violations = 0;
#define RULE(cond) do { if (!(cond)) { if (g_violations++ < 10) std::fprintf(stderr, "limb rule broken: %s (line %d)\n", #cond, __LINE__); } } while (0)

namespace aleo_mi355x {
struct F29 { uint32_t v[9]; };
static constexpr uint32_t M29 = 0x1fffffffu;
// r, and 19 r with its limbs raised by 2 * 2^29 (tools/gen_fr29_asm.py)
static constexpr uint32_t FR29_P[9] = {0x1u, 0x108c0000u, 0x42u, 0x14edfda0u, 0x1b00159au, 0x68f2e1bu, 0x155982d1u, 0xbd34594u, 0x12ab65u};
static constexpr uint32_t FR29_PAD[9] = {0x40000013u, 0x5a63fffeu, 0x400004edu, 0x4da9d2deu, 0x41019a78u, 0x5ca06c0fu, 0x55a4b584u, 0x40ae2a06u, 0x162b884u};
static constexpr uint32_t FR29_QMAGIC = 0xdb6u;
static constexpr uint32_t LAZY_MAX = 2833000000u;          // 2^31.4

inline F29 f29_from_words(const uint32_t (&w)[8]) {
  F29 r; r.v[0] = w[0] & M29;
  for (int i = 1; i < 8; ++i) r.v[i] = (uint32_t)((((uint64_t)w[i] << 32) | w[i - 1]) >> (32 - 3 * i)) & M29;
  r.v[8] = w[7] >> 8; return r;
}
inline void f29_to_words(const F29& a, uint32_t (&w)[8]) { for (int i = 0; i < 8; ++i) w[i] = (a.v[i] >> (3 * i)) | (a.v[i + 1] << (29 - 3 * i)); }
inline F29 f29_add(const F29& a, const F29& b) { F29 r; for (int i = 0; i < 9; ++i) { RULE((uint64_t)a.v[i] + b.v[i] < (1ull << 32)); r.v[i] = a.v[i] + b.v[i]; } return r; }
inline F29 f29_sub_pad(const F29& a, const F29& b) {
  F29 r;
  for (int i = 0; i < 9; ++i) {
    RULE(a.v[i] <= (1u << 30)); if (i < 8) RULE(b.v[i] <= (1u << 30) - 2);
    RULE((uint64_t)a.v[i] + FR29_PAD[i] >= b.v[i]);         // no limb goes negative (the top limb: b below 18 r)
    r.v[i] = a.v[i] + FR29_PAD[i] - b.v[i];
  }
  return r;
}
inline void f29_normalise(F29& a) { uint32_t c = 0; for (int i = 0; i < 8; ++i) { RULE((uint64_t)a.v[i] + c < (1ull << 32)); const uint32_t t = a.v[i] + c; c = t >> 29; a.v[i] = t & M29; } RULE((uint64_t)a.v[8] + c < (1ull << 32)); a.v[8] += c; }
inline void f29_reduce_partial(F29& a) {
  for (int i = 0; i < 8; ++i) RULE(a.v[i] <= M29);
  const uint32_t q = (uint32_t)(((uint64_t)a.v[8] * FR29_QMAGIC) >> 32);
  int64_t acc = 0;
  for (int i = 0; i < 8; ++i) { acc += (int64_t)a.v[i] - (int64_t)((uint64_t)q * FR29_P[i]); a.v[i] = (uint32_t)acc & M29; acc >>= 29; }
  const int64_t top = acc + (int64_t)a.v[8] - (int64_t)((uint64_t)q * FR29_P[8]);
  RULE(top >= 0 && top < (int64_t)3 * FR29_P[8] + 3);
  a.v[8] = (uint32_t)top;
}
// a * b * 2^-261 mod r with exact digits out, column by column as the generated device code does it
inline F29 f29_mul(const F29& a, const F29& b) {
  for (int i = 0; i < 9; ++i) { RULE(a.v[i] < LAZY_MAX); if (i < 8) RULE(b.v[i] <= M29); }
  uint32_t m[9]; F29 r; unsigned __int128 acc = 0;
  for (int col = 0; col < 17; ++col) {
    for (int j = 0; j < 9; ++j) { const int k = col - j; if (k >= 0 && k < 9) acc += (unsigned __int128)a.v[j] * b.v[k]; }
    for (int j = 0; j < 9 && j < col; ++j) { const int k = col - j; if (k >= 1 && k < 9) acc += (unsigned __int128)m[j] * FR29_P[k]; }
    if (col < 9) { m[col] = (uint32_t)(0 - (uint64_t)acc) & M29; acc += m[col]; RULE(((uint64_t)acc & M29) == 0); }
    else r.v[col - 9] = (uint32_t)acc & M29;
    RULE(acc < ((unsigned __int128)1 << 64));
    acc >>= 29;
  }
  r.v[8] = (uint32_t)acc; RULE(acc < ((unsigned __int128)1 << 32));      // the top limb holds what is left
  return r;
}
}  // namespace aleo_mi355x

#define ALEO_F29_PROVIDED
#include "records_host.hpp"

using namespace aleo_mi355x;

// the programs' generator: the same elements in every run
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static inline uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static inline void rnd_fr(uint8_t* out) { uint64_t v[4]; do { for (auto& x : v) x = rnd(); v[3] &= 0x1fffffffffffffffull; } while (HFr::geq_p(v)); std::memcpy(out, v, 32); }

// ---- a program's case file: its one argument, written by the test that runs it ---------------------------------------------------------------------------
static inline bool get(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
// The file, open, with the u32 it begins with in *count where one is asked for; null (the program returns 2) after the usage line, the system's error or a short file.
static inline std::FILE* open_cases(int argc, char** argv, uint32_t* count = nullptr) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return nullptr; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return nullptr; }
  if (count && !get(f, count, 4)) { std::fclose(f); return nullptr; }
  return f;
}
