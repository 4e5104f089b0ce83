// The record-string parse's device lane (aleo_amd/csrc/records_strings_lane.h) run on the HOST, string by string against aleo_mi355x_record_parse: the same
// owner variant, owner field and nonce x where the library accepts a string, a refusal exactly where it refuses.  A span with a NUL inside has no counterpart in
// a C string (the library would see it cut short): the lane must refuse it.
//   records_strings_lane_emul <file>    file: u32 count, then per string u32 length and the bytes (tests/test_records_strings.py writes its case list and runs this).
//   g++ -std=c++17 -O2 -I include tests/cpp/records_strings_lane_emul.cpp -L aleo_amd/lib -laleo_mi355x
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

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  unsigned long accepted = 0, refused = 0, with_nul = 0, bad = 0;
  std::vector<char> s;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t len = 0;
    if (std::fread(&len, 4, 1, f) != 1) return 2;
    s.assign((size_t)len + 1, 0);
    if (len && std::fread(s.data(), 1, len, f) != len) return 2;
    uint32_t ow[8], nw[8]; uint32_t asked_past_the_end = 0;
    const int32_t kind = aleo_mi355x::records_parse_lane([&](uint32_t j) { asked_past_the_end += j >= len; return j < len ? (uint8_t)s[j] : (uint8_t)0; }, len, ow, nw);
    bool ok = asked_past_the_end == 0 && kind >= -1 && kind <= 1;
    if (kind < 0) for (int q = 0; q < 8; ++q) ok = ok && !ow[q] && !nw[q];
    if (std::memchr(s.data(), 0, len)) { ++with_nul; ok = ok && kind == -1; }
    else {
      int32_t want_kind = -1; uint8_t owner[32], nonce[32];
      const int32_t rc = aleo_mi355x_record_parse(s.data(), &want_kind, owner, nonce);
      if (rc) ok = ok && kind == -1;
      else ok = ok && kind == want_kind && !std::memcmp(ow, owner, 32) && !std::memcmp(nw, nonce, 32);
      if (rc) ++refused; else ++accepted;
    }
    if (!ok && bad++ < 10) std::fprintf(stderr, "string %u (%u characters): the lane says %d, %u reads past the end\n", i, len, kind, asked_past_the_end);
  }
  std::fclose(f);
  std::printf("records_strings_lane_emul: %u strings, %lu accepted, %lu refused, %lu with a NUL, %lu mismatches\n", count, accepted, refused, with_nul, bad);
  return bad || !accepted || !refused || !with_nul ? 1 : 0;
}
