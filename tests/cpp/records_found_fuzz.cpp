// The host side of decrypt_strings under AddressSanitizer + UndefinedBehaviorSanitizer (tools/asan_records_found.sh builds this with the host-only sources of the
// library: wire.hip, sponge.hip, and the headers records_found_host.hpp includes): the parse lane, the two walks of records_found_lane.h and the whole host path
// (found_on_host) over the case list of tests/test_records_found.py, then over mutations of it:
//   bit flips in the payload and length bytes pointing past it, re-encoded so that the checksum holds (the walk is reached), and truncated strings (it is not).
// A lane must never ask for a character past its string's end; the sanitizers see everything else.
//   records_found_fuzz <case file> <view key, 64 hex digits, little-endian bytes> <address x, the same>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "aleo_mi355x.h"
// the two device intrinsics the scan's lane header (included by records_host.hpp, not run here) names
static inline uint32_t __funnelshift_r(uint32_t lo, uint32_t hi, uint32_t s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31u)); }
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
#include "../../aleo_amd/csrc/records_found_host.hpp"

using namespace aleo_mi355x;

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static bool unhex(uint8_t* out, const char* s) {
  if (std::strlen(s) != 64) return false;
  for (int i = 0; i < 32; ++i) { unsigned v; if (std::sscanf(s + 2 * i, "%2x", &v) != 1) return false; out[i] = (uint8_t)v; }
  return true;
}

static unsigned long walks = 0, past_the_end = 0, owned = 0, calls = 0;

// one string through the lanes, as the kernels run them
static void lanes(const std::string& s) {
  const uint32_t len = (uint32_t)s.size();
  std::vector<uint8_t> exact(s.begin(), s.end());             // no terminator: a read past the end is the sanitizer's
  uint32_t past = 0;
  auto ch = [&](uint32_t j) { if (j >= len) { ++past; return (uint8_t)0; } return exact[j]; };
  uint32_t ow[8], nw[8];
  const int32_t kind = records_parse_lane(ch, len, ow, nw);
  if (kind >= 0) {
    ++walks;
    const FoundWalk c = records_found_walk(ch, len, kind, [](uint32_t, const uint32_t (&)[8]) {});
    std::vector<uint32_t> rows;
    if (c.status == FOUND_OK) {
      rows.resize(8 * (size_t)c.fields);
      const FoundWalk g = records_found_walk(ch, len, kind, [&](uint32_t k, const uint32_t (&w)[8]) { std::memcpy(&rows.at(8 * (size_t)k), w, 32); });
      if (g.fields != c.fields || g.status != c.status) ++past;
      if (c.mc_kind == FOUND_MC_PRIVATE) (void)found_microcredits_private(c.mc_n, [&](uint32_t k, uint32_t (&w)[8]) { std::memcpy(w, &rows.at(8 * (size_t)(c.mc_at + k)), 32); });
    }
  }
  past_the_end += past;
}

static int whole(const std::vector<std::string>& strings, const ScanArgs& key, const HFr& addr) {
  std::string text; std::vector<uint64_t> off{0};
  for (const auto& s : strings) { text += s; off.push_back(text.size()); }
  std::vector<char> exact(text.begin(), text.end());
  Found R;
  if (found_on_host(R, exact.data(), off.data(), strings.size(), key, addr)) return 1;
  ++calls; owned += R.index.size();
  if (R.offsets.size() != R.index.size() + 1 || R.plain.size() != 32 * (size_t)R.offsets.back() || R.status.size() != R.index.size() || R.microcredits.size() != R.index.size() || R.rvk.size() != 32 * R.index.size()) return 1;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s <case file> <view key hex> <address x hex>\n", argv[0]); return 2; }
  uint8_t vk[32], ax[32];
  if (!unhex(vk, argv[2]) || !unhex(ax, argv[3])) return 2;
  ScanArgs key; HFr addr;
  if (scan_args(key, addr, vk, ax)) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  std::vector<std::string> cases;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t len = 0;
    if (std::fread(&len, 4, 1, f) != 1) return 2;
    std::string s(len, '\0');
    if (len && std::fread(&s[0], 1, len, f) != len) return 2;
    cases.push_back(std::move(s));
  }
  std::fclose(f);
  int fails = 0;
  for (const auto& s : cases) lanes(s);
  fails += whole(cases, key, addr);
  // mutations with a valid checksum: decode, change the payload, encode
  std::vector<std::string> mutated;
  std::vector<uint8_t> payload; char hrp[16]; std::vector<char> out;
  for (int round = 0; round < 1500; ++round) {
    const std::string& s = cases[rnd() % cases.size()];
    payload.assign(s.size() + 1, 0); size_t len = payload.size();
    if (std::memchr(s.data(), 0, s.size()) || aleo_mi355x_bech32m_decode(payload.data(), &len, hrp, sizeof hrp, s.c_str()) || len < 40) continue;
    payload.resize(len);
    switch (rnd() % 4) {
      case 0: payload[rnd() % len] ^= (uint8_t)(1u << (rnd() % 8)); break;                        // one bit anywhere
      case 1: payload[35 + rnd() % (len > 100 ? 64 : len - 36)] = (uint8_t)rnd(); break;          // a byte among the counts, names and lengths of the first entries
      case 2: { const size_t at = 36 + rnd() % (len - 38); payload[at] = 0xff; payload[at + 1] = 0xff; break; }      // a length pointing past the payload
      default: payload.resize(1 + rnd() % len); break;                                            // cut short, checksum valid
    }
    out.assign(2 * payload.size() + 32, 0);
    if (aleo_mi355x_bech32m_encode(out.data(), out.size(), "record", payload.data(), payload.size())) { ++fails; continue; }
    mutated.emplace_back(out.data());
    lanes(mutated.back());
    if (mutated.size() == 64) { fails += whole(mutated, key, addr); mutated.clear(); }
  }
  fails += whole(mutated, key, addr);
  // truncations and raw flips: the checksum fails, nothing walks
  for (const auto& s : cases)
    for (size_t cut = 0; cut < s.size() && cut < 400; cut += 7) { lanes(s.substr(0, cut)); if (cut) { std::string t = s; t[cut] ^= 1; lanes(t); } }
  std::printf("records_found_fuzz: %zu cases, %lu walks, %lu host calls with %lu owned records, %lu reads past the end, %d failures\n", cases.size(), walks, calls, owned, past_the_end, fails);
  if (fails || past_the_end || walks < 500 || !owned) return 1;
  std::printf("SANITIZED OK\n");
  return 0;
}
