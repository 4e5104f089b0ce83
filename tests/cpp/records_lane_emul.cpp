// The record scan's device lane (aleo_amd/csrc/records_lane.h, edwards29.h) run on the HOST, against the library's host path (records_host.hpp).
//
// The 29-bit-limb field of fr29.h is restated here in plain C++ with every operand rule of its header turned into a check — a product's multiplicand
// has limbs below 2^31.4, its multiplier is normalised, its column sums fit 64 bits; a padded difference never borrows; a lazy sum never wraps — so
// the lane's code is exercised, limb for limb, without a GPU, and a broken bound shows as a count instead of as a wrong flag one record in a million.
// Needs no library, only the compiler that builds it (the host arithmetic of host_field.hpp is written for clang's carry-chain intrinsics):
//   hipcc -x c++ -std=c++17 -O2 -mbmi2 -madx -I aleo_amd/csrc tests/cpp/records_lane_emul.cpp   (tests/test_records.py builds and runs it).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __device__
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

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static void rnd_fr(uint8_t* out) { uint64_t v[4]; do { for (auto& x : v) x = rnd(); v[3] &= 0x1fffffffffffffffull; } while (HFr::geq_p(v)); std::memcpy(out, v, 32); }

int main() {
  const RecordsConsts& C = records_consts();
  unsigned long bad = 0, owned = 0, malformed = 0, total = 0;
  for (int key = 0; key < 3; ++key) {
    uint8_t vk[32], ax[32];
    rnd_fr(vk); vk[31] &= 0x03;                               // below l (251 bits)
    if (key == 1) vk[0] &= 0xfe; else if (key == 2) vk[0] |= 1;      // an even and an odd key for sure
    rnd_fr(ax);
    ScanArgs A; HFr addr;
    if (const char* why = scan_args(A, addr, vk, ax)) { std::fprintf(stderr, "scan_args: %s\n", why); return 2; }
    for (int i = 0; i < 150; ++i, ++total) {
      uint8_t c0[32], nx[32], want_rvk[32];
      rnd_fr(c0); rnd_fr(nx);
      if (i == 0) std::memset(nx, 0, 32);                     // x = 0
      if (i == 1) std::memset(nx, 0xff, 32);                  // not below r
      if (i == 2) std::memset(c0, 0xff, 32);
      if (i == 3) { std::memcpy(c0, host::HParams<4>::P, 32); }      // exactly r
      uint8_t want = scan_one_host(want_rvk, c0, nx, A, addr, C);
      if (i % 4 == 0 && want == 0) {                          // make this one owned: c0 = address x + randomizer, read back from what the host path hashes
        HFr st[9]; for (int q = 0; q < 9; ++q) st[q] = C.s0[q];
        HFr rv; std::memcpy(rv.l, want_rvk, 32); st[2] = HFr::add(st[2], HFr::to_mont(rv));
        host::poseidon_permute<4, 8>(st);
        const HFr c = HFr::from_mont(HFr::add(addr, st[1])); std::memcpy(c0, c.l, 32);
        want = scan_one_host(want_rvk, c0, nx, A, addr, C);
        if (want != 1) { std::fprintf(stderr, "host path: a record encrypted to the address is not owned\n"); ++bad; }
      }
      uint32_t c0w[8], nxw[8]; std::memcpy(c0w, c0, 32); std::memcpy(nxw, nx, 32);
      F29 out; const uint32_t got = records_scan_lane(c0w, nxw, C.words.data(), A, [&](const F29& v) { out = v; });
      uint32_t ow[8]; f29_to_words(out, ow);
      if (got != want || std::memcmp(ow, want_rvk, 32)) { if (bad++ < 5) std::fprintf(stderr, "key %d record %d: lane flag %u, host flag %u, rvk %s\n", key, i, got, (unsigned)want, std::memcmp(ow, want_rvk, 32) ? "differs" : "equal"); }
      owned += want == 1; malformed += want == 2;
    }
  }
  std::printf("records_lane_emul: %lu records, %lu owned, %lu malformed, %lu mismatches, %lu limb-rule violations\n", total, owned, malformed, bad, g_violations);
  return bad || g_violations || !owned || !malformed ? 1 : 0;
}
