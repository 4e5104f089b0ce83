// The plaintext kernel's device lane (aleo_amd/csrc/plaintexts_lane.h over records_commit_lane.h's commit_hash) run on the HOST, string by string against the rows
// the library's host path returned (aleo_mi355x_plaintexts_commitments_host: plaintext_parse.hpp's parse and record_bits, serial_host.hpp's BHP1024), with the table
// and the call's starting point built by commit_host.hpp as the library builds them.
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of fr29.h is a check there.  A lane must never ask for a character at or behind
// its string's end: the strings are held exactly, so such a read is counted here and is the sanitizer's.  Plain C++ for the host compiler, built once plain and
// once with the address and undefined-behaviour sanitizers and run as a program of its own (tests/test_plaintexts.py):
//   g++ -std=c++17 -O2 -mbmi2 -madx [-fsanitize=address,undefined] -I aleo_amd/csrc tests/cpp/plaintexts_lane_emul.cpp
//   plaintexts_lane_emul <case file>
// The file: u32 length and bytes of the program id, the same of the record name, u32 count, then per string: u32 length and the characters, u8 the lane's flag
// wanted (0 computed, 8 routed to the host: the lane must say so), u8 the host path's flag (0, or 3 not a record plaintext), the 32-byte row and the u64
// microcredits of the host path.  The lane's row and microcredits are compared where it computes; a string the host path refuses must be routed.
#include "checked_f29.h"
#include "commit_host.hpp"
#include "plaintexts_lane.h"
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
    std::string s; uint8_t want_flag, host_flag, want[32]; uint64_t want_mc;
    if (!get_string(f, s) || !get(f, &want_flag, 1) || !get(f, &host_flag, 1) || !get(f, want, 32) || !get(f, &want_mc, 8)) return 2;
    const std::vector<char> exact(s.begin(), s.end());           // exact: a read past the end is the sanitizer's
    const uint32_t len = (uint32_t)exact.size();
    auto ch = [&](uint32_t j) { if (j >= len) { ++past; return (uint8_t)0; } return (uint8_t)exact[j]; };
    uint8_t got[32] = {0}; uint64_t mc = 0;
    const uint32_t flag = plaintexts_commit_lane(ch, len, T.words.data(), A, mc, [&](const F29& v) { uint32_t w[8]; f29_to_words(v, w); std::memcpy(got, w, 32); });
    const bool row_ok = flag != COMMIT_OK || (!std::memcmp(got, want, 32) && mc == want_mc && host_flag == 0);
    if (flag != want_flag || !row_ok) {
      if (bad++ < 8) std::fprintf(stderr, "string %u: lane flag %u, wanted %u (host flag %u), commitment %s, microcredits %llu / %llu\n", i, flag, (unsigned)want_flag, (unsigned)host_flag,
                                  std::memcmp(got, want, 32) ? "differs" : "equal", (unsigned long long)mc, (unsigned long long)want_mc);
    }
    computed += flag == COMMIT_OK; routed += flag == COMMIT_ROUTED; refused += flag == COMMIT_ROUTED && host_flag != 0;
    if (flag == COMMIT_OK) {                                     // how many iterations the record's message takes
      auto c = [&](uint32_t j) { return j < len ? (uint32_t)(uint8_t)exact[j] : 0u; };
      PtMeasure M; (void)pt_measure(c, len, M);
      const uint32_t bits = A.name_bits + 254 + 32 + M.data_bits + 253, it = (bits + 1043) / 1044;
      ++iterations[it < 4 ? it : 0];
      std::printf("string %u: %u bits\n", i, bits);
    }
  }
  std::fclose(f);
  std::printf("plaintexts_lane_emul: %u strings, %lu computed, %lu refused, %lu routed, %lu mismatches, %lu reads past an end, %lu limb-rule violations; iterations 1: %lu, 2: %lu, 3: %lu, other: %lu\n",
              count, computed, refused, routed, bad, past, g_violations, iterations[1], iterations[2], iterations[3], iterations[0]);
  return bad || past || g_violations ? 1 : 0;
}
