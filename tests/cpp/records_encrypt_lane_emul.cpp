// The two device lanes of the record encryption (aleo_amd/csrc/records_encrypt_lane.h: records_encrypt_keys_lane, then records_encrypt_text_lane over what it
// left) run on the HOST, string by string against the rows the library's host path returned (aleo_mi355x_records_encrypt_host: record_encrypt_host.hpp over
// plaintext_parse.hpp), with the table built by signature_host.hpp as the library builds it.
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of fr29.h is a check there, so a bound a lane breaks — the sum of a plain field and
// a randomizer, the state carried from one permutation into the next — shows as a count.  The lanes take their characters through a callable that gives 0 at
// and behind the end, as the kernels' does; the strings are held exactly, so a read that callable lets through is the sanitizer's.  The text lane must write
// exactly the characters the keys lane measured.  Plain
// C++ for the host compiler, built once plain and once with the address and undefined-behaviour sanitizers and run as a program of its own
// (tests/test_records_encrypt.py):
//   g++ -std=c++17 -O2 -fno-strict-aliasing -mbmi2 -madx [-fsanitize=address,undefined] -I aleo_amd/csrc tests/cpp/records_encrypt_lane_emul.cpp
//   records_encrypt_lane_emul <case file>
// The file: u32 count, then per string: u32 length and the characters, the 32 bytes of the randomizer, u8 the mode, u8 the lane's flag wanted (the host path's, or 8
// where the lane must route), u8 the host path's flag, u32 length and the characters of the host path's record1… string, the 32 bytes of its record view key.
#include "checked_f29.h"
#include "signature_host.hpp"
#include "records_encrypt_lane.h"
#include <string>
#include <vector>

static bool get_string(std::FILE* f, std::string& s) { uint32_t n; if (!get(f, &n, 4) || n > (1u << 22)) return false; s.assign(n, 0); return n == 0 || get(f, &s[0], n); }

int main(int argc, char** argv) {
  uint32_t count = 0;
  std::FILE* f = open_cases(argc, argv, &count);
  if (!f) return 2;
  const sig::SigTables& T = sig::sig_tables();
  unsigned long flags[4] = {0, 0, 0, 0}, routed = 0, refused = 0, bad = 0, fields = 0, squeezes[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < count; ++i) {
    std::string s, want; uint8_t randomizer[32], mode, want_flag, host_flag, want_rvk[32];
    if (!get_string(f, s) || !get(f, randomizer, 32) || !get(f, &mode, 1) || !get(f, &want_flag, 1) || !get(f, &host_flag, 1) || !get_string(f, want) || !get(f, want_rvk, 32)) return 2;
    const std::vector<char> exact(s.begin(), s.end());           // exact: a read past the end is the sanitizer's
    const uint32_t len = (uint32_t)exact.size();
    auto c = [&](uint32_t j) { return j < len ? (uint32_t)(uint8_t)exact[j] : 0u; };      // what the kernels hand the lanes: 0 at and behind the end
    uint32_t rw[8], nonce[8], rvk[8]; std::memcpy(rw, randomizer, 32);
    ReMeasure R;
    const uint32_t flag = records_encrypt_keys_lane(c, len, rw, (uint32_t)mode, T.words.data(), R, nonce, rvk, [] {});
    std::string got;
    if (flag == RE_OK) {
      got = "record1";
      records_encrypt_text_lane(c, R.info, nonce, rvk, T.words.data(), [&](uint32_t ch) { got.push_back((char)ch); });
    }
    bool ok = flag == want_flag;
    if (flag == RE_ROUTED) { ++routed; refused += host_flag != 0; ok = ok && R.chars == 0; }
    else {
      ++flags[flag & 3u];
      ok = ok && flag == host_flag && got == want && R.chars == got.size() && !std::memcmp(rvk, want_rvk, 32);
      if (flag == RE_OK) { const uint32_t m = (R.info >> 8) & 0xffu; fields += m; ++squeezes[(m + 7) / 8 < 4 ? (m + 7) / 8 : 3]; }
    }
    if (!ok && bad++ < 8)
      std::fprintf(stderr, "string %u: lane flag %u, wanted %u (host flag %u); %u characters measured, %zu written, %zu wanted, the text %s, the key %s\n", i, flag, (unsigned)want_flag,
                   (unsigned)host_flag, R.chars, got.size(), want.size(), got == want ? "equal" : "differs", std::memcmp(rvk, want_rvk, 32) ? "differs" : "equal");
  }
  std::fclose(f);
  std::printf("records_encrypt_lane_emul: %u strings, %lu encrypted, %lu nonce mismatches, %lu bad keys, %lu routed, %lu of them refused, %lu mismatches, "
              "%lu limb-rule violations; %lu private fields, squeezes 0: %lu, 1: %lu, 2: %lu, 3: %lu\n",
              count, flags[0], flags[1], flags[2], routed, refused, bad, g_violations, fields, squeezes[0], squeezes[1], squeezes[2], squeezes[3]);
  return bad || g_violations ? 1 : 0;
}
