// The commitment kernel's device lane (aleo_amd/csrc/records_commit_lane.h) run on the HOST, record by record against the rows the library's host path returned
// (aleo_mi355x_records_commitments_found_host: records_bits.hpp's record_bits and serial_host.hpp's BHP1024, the code of aleo_mi355x_record_commitment), with the
// table and the call's starting point built by commit_host.hpp as the library builds them.
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of
// fr29.h is a check there, so a bound the lane breaks in its table additions or where an iteration's digest is fed back shows as a count.  A lane must never ask
// for a character past its string's end or for a field past its record's.  Plain C++ for the host compiler, built once plain and once with the address and
// undefined-behaviour sanitizers and run as a program of its own (tests/test_records_commit.py):
//   g++ -std=c++17 -O2 -mbmi2 -madx [-fsanitize=address,undefined] -I aleo_amd/csrc tests/cpp/records_commit_lane_emul.cpp
//   records_commit_lane_emul <case file>
// The file: u32 length and bytes of the program id, the same of the record name, u32 count, then per record: u32 length and the characters, i32 owner variant,
// u32 number of plain fields and their 32 bytes each, u8 the flag wanted (0 computed, 4 refused, 8 routed to the host: the lane must say so) and the 32-byte row.
#include "checked_f29.h"
#include "commit_host.hpp"
#include <string>
#include <vector>

static bool get_string(std::FILE* f, std::string& s) { uint32_t n; if (!get(f, &n, 4) || n > (1u << 22)) return false; s.assign(n, 0); return get(f, &s[0], n); }

int main(int argc, char** argv) {
  std::FILE* f = open_cases(argc, argv);
  if (!f) return 2;
  std::string program_id, record_name;
  uint32_t count = 0;
  if (!get_string(f, program_id) || !get_string(f, record_name) || !get(f, &count, 4)) return 2;
  const size_t dot = program_id.find('.');
  if (dot == std::string::npos) return 2;
  const serial::CommitTables& T = serial::commit_tables();
  const std::vector<uint8_t> name_bits = serial::commit_name_bits(program_id.c_str(), dot, record_name.c_str());
  const CommitArgs A = serial::commit_args(name_bits);
  unsigned long computed = 0, refused = 0, routed = 0, bad = 0, past = 0, iterations[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < count; ++i) {
    std::string s; int32_t kind; uint32_t nf; uint8_t want_flag, want[32];
    if (!get_string(f, s) || !get(f, &kind, 4) || !get(f, &nf, 4) || nf > (1u << 16)) return 2;
    std::vector<uint8_t> plain((size_t)nf * 32);                 // exact: a read past the end is the sanitizer's
    if (!get(f, plain.data(), plain.size()) || !get(f, &want_flag, 1) || !get(f, want, 32)) return 2;
    const std::vector<char> exact(s.begin(), s.end());
    const uint32_t len = (uint32_t)exact.size();
    auto ch = [&](uint32_t j) { if (j >= len) { ++past; return (uint8_t)0; } return (uint8_t)exact[j]; };
    auto load = [&](uint32_t k, uint32_t (&w)[8]) { if (k >= nf) { ++past; std::memset(w, 0, 32); return; } std::memcpy(w, plain.data() + 32 * (size_t)k, 32); };
    uint8_t got[32] = {0};
    const uint32_t flag = records_commit_lane(ch, len, kind, nf, load, T.words.data(), A, [&](const F29& v) { uint32_t w[8]; f29_to_words(v, w); std::memcpy(got, w, 32); });
    if (flag != want_flag || (flag == COMMIT_OK && std::memcmp(got, want, 32))) {
      if (bad++ < 8) std::fprintf(stderr, "record %u: lane flag %u, wanted %u, commitment %s\n", i, flag, (unsigned)want_flag, std::memcmp(got, want, 32) ? "differs" : "equal");
    }
    computed += flag == COMMIT_OK; refused += flag == COMMIT_REFUSED; routed += flag == COMMIT_ROUTED;
    if (flag == COMMIT_OK) {                                     // how many iterations the record's message takes
      constexpr RsSymbols S = rs_symbols();
      auto sym = [&](uint32_t k) { return RS_PREFIX_CHARS + k < len ? (uint32_t)S.of[(uint8_t)exact[RS_PREFIX_CHARS + k] & 127u] & 31u : 0u; };
      uint32_t data_bits = 0; (void)commit_measure(sym, kind, nf, load, data_bits);
      const uint32_t bits = A.name_bits + 254 + 32 + data_bits + 253, it = (bits + 1043) / 1044;
      ++iterations[it < 4 ? it : 0];
      std::printf("record %u: %u bits\n", i, bits);
    }
  }
  std::fclose(f);
  std::printf("records_commit_lane_emul: %u records, %lu computed, %lu refused, %lu routed, %lu mismatches, %lu reads past an end, %lu limb-rule violations; iterations 1: %lu, 2: %lu, 3: %lu, other: %lu\n",
              count, computed, refused, routed, bad, past, g_violations, iterations[1], iterations[2], iterations[3], iterations[0]);
  return bad || past || g_violations ? 1 : 0;
}
