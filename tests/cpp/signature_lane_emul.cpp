// The signature kernel's device lane (aleo_amd/csrc/signature_lane.h) run on the HOST, signature by signature against the flags the library's host path returned
// (aleo_mi355x_signatures_verify_host) and against signature_host.hpp's verify_one_host compiled into this program, with the table built by signature_host.hpp
// as the library builds it.  The lane picks the point of an x-coordinate with one exponentiation where the host path multiplies by the group order: every case
// that reaches a point checks the one against the other.
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of
// fr29.h is a check there, so a bound the lane breaks shows as a count.  A lane must never ask for a byte past its message's end.  Plain C++ for the host
// compiler, built once plain and once with the address and undefined-behaviour sanitizers and run as a program of its own (tests/test_signatures.py):
//   g++ -std=c++17 -O2 -fno-strict-aliasing -mbmi2 -madx [-fsanitize=address,undefined] -I aleo_amd/csrc tests/cpp/signature_lane_emul.cpp
//   signature_lane_emul <case file>
// The file: u32 count, then per signature: its 128 bytes, the 32 bytes of the address x, u32 length and the bytes of the message, u8 the flag wanted.
#include "checked_f29.h"
#include "signature_host.hpp"
#include <vector>


int main(int argc, char** argv) {
  uint32_t count = 0;
  std::FILE* f = open_cases(argc, argv, &count);
  if (!f) return 2;
  const sig::SigTables& T = sig::sig_tables();
  unsigned long flags[4] = {0, 0, 0, 0}, bad = 0, past = 0, permutations = 0;
  for (uint32_t i = 0; i < count; ++i) {
    uint8_t s[128], addr[32], want; uint32_t len;
    if (!get(f, s, 128) || !get(f, addr, 32) || !get(f, &len, 4) || len > (1u << 22)) return 2;
    std::vector<uint8_t> msg(len);                               // exact: a read past the end is the sanitizer's
    if (!get(f, msg.data(), len) || !get(f, &want, 1)) return 2;
    auto load = [&](uint32_t k, uint32_t (&w)[8]) { std::memcpy(w, k < 4 ? s + 32 * k : addr, 32); };
    auto byte = [&](uint32_t q) { if (q >= len) { ++past; return (uint8_t)0; } return msg[q]; };
    const uint32_t flag = signature_verify_lane(load, len, byte, T.words.data(), [] {});
    const uint32_t host = sig::verify_one_host(s, addr, msg.data(), len);
    if (flag != want || host != want) { if (bad++ < 8) std::fprintf(stderr, "signature %u: lane flag %u, host flag %u, wanted %u\n", i, flag, host, (unsigned)want); }
    ++flags[flag & 3u];
    if (flag != SIG_MALFORMED) permutations += (12 + (8ul * len + 251) / 252 + 7) / 8;
  }
  std::fclose(f);
  std::printf("signature_lane_emul: %u signatures, %lu verify, %lu do not, %lu malformed, %lu mismatches, %lu reads past an end, %lu limb-rule violations; %lu rate-8 permutations\n",
              count, flags[0], flags[1], flags[3], bad, past, g_violations, permutations);
  return bad || past || g_violations ? 1 : 0;
}
