// The serial-number kernel's device lane (aleo_amd/csrc/records_serial_lane.h) run on the HOST, against the library's host path (serial_host.hpp), and that
// path against the same computation written from the definitions without the tables (serial_one_plain).
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of
// fr29.h is a check there, so a bound the lane breaks — in the width-3 permutation, Elligator2's sums and differences, the table additions — shows as a count.
// Plain C++ for the host compiler, built with the address and undefined-behaviour sanitizers and run as a program of its own (tests/test_records_serial.py):
//   g++ -std=c++17 -O2 -mbmi2 -madx -fsanitize=address,undefined -I aleo_amd/csrc tests/cpp/records_serial_lane_emul.cpp
// argv[1] (optional): a file of 32-byte commitments to use instead of the built-in ones; argv[2]: where to write the host path's rows for the first key (flag byte
// and 32 bytes each), so that the test compares them with what the library's C ABI returns for the same commitments.
#include "checked_f29.h"
#include "serial_host.hpp"
#include <vector>

int main(int argc, char** argv) {
  const serial::SerialTables& T = serial::serial_tables();
  std::vector<uint8_t> cms;
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "rb"); if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint8_t row[32]; while (std::fread(row, 1, 32, f) == 32) cms.insert(cms.end(), row, row + 32);
    std::fclose(f);
  } else {
    cms.assign(32 * 24, 0);
    for (int i = 0; i < 24; ++i) rnd_fr(cms.data() + 32 * i);
    std::memset(cms.data(), 0, 32);                                         // 0
    cms[32] = 1; std::memset(cms.data() + 33, 0, 31);                      // 1
    std::memcpy(cms.data() + 64, host::HParams<4>::P, 32); cms[64] -= 1;    // r - 1
    std::memcpy(cms.data() + 96, host::HParams<4>::P, 32);                  // r: refused
    std::memset(cms.data() + 128, 0xff, 32);                                // 2^256 - 1: refused
  }
  const size_t n = cms.size() / 32;
  uint8_t keys[4][32]; std::memset(keys, 0, sizeof keys);
  rnd_fr(keys[0]); keys[0][31] &= 0x03;                                      // below l (251 bits)
  keys[2][0] = 1;                                                           // 1; keys[1] = 0
  std::memcpy(keys[3], ED_ORDER, 32); keys[3][0] -= 1;                      // l - 1
  if (argc > 3) { FILE* f = std::fopen(argv[3], "rb"); if (!f || std::fread(keys[0], 1, 32, f) != 32) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; } std::fclose(f); }
  unsigned long bad = 0, refused = 0, total = 0, plain_bad = 0;
  FILE* dump = argc > 2 ? std::fopen(argv[2], "wb") : nullptr;
  for (int k = 0; k < 4; ++k) {
    ScanArgs key; if (!serial::serial_key(key, keys[k])) { std::fprintf(stderr, "key %d refused\n", k); return 2; }
    SerialArgs A; std::memcpy(A.naf_pos, key.naf_pos, sizeof A.naf_pos); std::memcpy(A.naf_neg, key.naf_neg, sizeof A.naf_neg); A.naf_len = key.naf_len;
    for (size_t i = 0; i < n; ++i, ++total) {
      uint8_t want[32], plain[32];
      const uint8_t flag = serial::serial_one_host(want, cms.data() + 32 * i, key, T);
      if (k == 0 || i < 6) { const uint8_t pf = serial::serial_one_plain(plain, cms.data() + 32 * i, key, T); if (pf != flag || std::memcmp(plain, want, 32)) { if (plain_bad++ < 5) std::fprintf(stderr, "key %d commitment %zu: the tables and the definitions disagree\n", k, i); } }
      if (k == 0 && dump) { std::fwrite(&flag, 1, 1, dump); std::fwrite(want, 1, 32, dump); }
      uint32_t cw[8]; std::memcpy(cw, cms.data() + 32 * i, 32);
      F29 out; const uint32_t got = records_serial_lane(cw, T.words.data(), A, [&](const F29& v) { out = v; });
      uint32_t ow[8]; f29_to_words(out, ow);
      if (got != flag || std::memcmp(ow, want, 32)) { if (bad++ < 5) std::fprintf(stderr, "key %d commitment %zu: lane flag %u, host flag %u, serial number %s\n", k, i, got, (unsigned)flag, std::memcmp(ow, want, 32) ? "differs" : "equal"); }
      refused += flag == 2;
    }
  }
  if (dump) std::fclose(dump);
  // Elligator2 on 0: the refusal no hash reaches.  The lane's head sets the flag; the host's map returns false.
  bool lane_bad = false; F29 zero = f29_zero(); (void)ell29_head(zero, lane_bad, T.words.data());
  EdH e; const bool host_ok = serial::elligator2(e, HFr::zero(), T);
  if (!lane_bad || host_ok) { std::fprintf(stderr, "Elligator2(0) is not refused: lane %d host %d\n", (int)lane_bad, (int)!host_ok); ++bad; }
  std::printf("records_serial_lane_emul: %lu commitments, %lu refused, %lu mismatches, %lu table mismatches, %lu limb-rule violations\n", total, refused, bad, plain_bad, g_violations);
  return bad || plain_bad || g_violations || (argc <= 1 && !refused) ? 1 : 0;
}
