// The walk of an owned record's private fields (aleo_amd/csrc/records_found_lane.h) run on the HOST, string by string against aleo_mi355x_record_fields: on every
// string the parse accepts, the counting walk must refuse exactly where record_fields refuses and count what it counts, and the gathering walk must emit the
// bytes it writes, in order, reading no character past the string's end.
//   records_found_lane_emul <file>    file: u32 count, then per string u32 length and the bytes (tests/test_records_found.py writes its case list and runs this).
//   g++ -std=c++17 -O2 -I include tests/cpp/records_found_lane_emul.cpp -L aleo_amd/lib -laleo_mi355x
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "aleo_mi355x.h"

#define __host__
#define __device__
#define __forceinline__ inline
#include "../../aleo_amd/csrc/records_strings_lane.h"
#include "../../aleo_amd/csrc/records_found_lane.h"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  unsigned long accepted = 0, refused = 0, unparsed = 0, fields = 0, bad = 0;
  std::vector<char> s;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t len = 0;
    if (std::fread(&len, 4, 1, f) != 1) return 2;
    s.assign((size_t)len + 1, 0);
    if (len && std::fread(s.data(), 1, len, f) != len) return 2;
    uint32_t ow[8], nw[8]; uint32_t past = 0;
    auto ch = [&](uint32_t j) { past += j >= len; return j < len ? (uint8_t)s[j] : (uint8_t)0; };
    const int32_t kind = aleo_mi355x::records_parse_lane(ch, len, ow, nw);
    if (kind < 0) { ++unparsed; continue; }
    std::vector<uint8_t> got;
    const aleo_mi355x::FoundWalk c = aleo_mi355x::records_found_walk(ch, len, kind, [](uint32_t, const uint32_t (&)[8]) {});
    uint32_t next = 0; bool in_order = true;
    const aleo_mi355x::FoundWalk g = aleo_mi355x::records_found_walk(ch, len, kind, [&](uint32_t k, const uint32_t (&w)[8]) { in_order = in_order && k == next++; got.insert(got.end(), (const uint8_t*)w, (const uint8_t*)w + 32); });
    size_t n = 0;
    const int32_t rc = aleo_mi355x_record_fields(s.data(), nullptr, 0, &n);
    bool ok = past == 0 && in_order && c.status == g.status && c.fields == g.fields && c.mc_kind == g.mc_kind && c.mc_at == g.mc_at && c.mc_n == g.mc_n && c.mc_value == g.mc_value;
    if (rc) { ++refused; ok = ok && c.status == aleo_mi355x::FOUND_REFUSED && c.fields == 0; }
    else {
      ++accepted; fields += n;
      std::vector<uint8_t> want(32 * n + 1);
      ok = ok && aleo_mi355x_record_fields(s.data(), want.data(), n, &n) == 0;
      ok = ok && c.status == aleo_mi355x::FOUND_OK && c.fields == n && got.size() == 32 * n && !std::memcmp(got.data(), want.data(), 32 * n);
      ok = ok && (c.mc_kind != aleo_mi355x::FOUND_MC_PRIVATE || c.mc_at + c.mc_n <= n);
    }
    if (!ok && bad++ < 10) std::fprintf(stderr, "string %u (%u characters): record_fields says %d with %zu fields, the walk status %u with %u fields, %u reads past the end\n", i, len, rc, n, c.status, c.fields, past);
  }
  std::fclose(f);
  std::printf("records_found_lane_emul: %u strings, %lu unparsed, %lu accepted, %lu refused, %lu fields, %lu mismatches\n", count, unparsed, accepted, refused, fields, bad);
  return bad || !accepted || !refused || !fields ? 1 : 0;
}
