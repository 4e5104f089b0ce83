// The record scan's device lane (aleo_amd/csrc/records_lane.h, edwards29.h) run on the HOST, against the library's host path (records_host.hpp).
//
// The 29-bit-limb field is the checked one of checked_f29.h: every operand rule of fr29.h is a check there, so the lane's code is exercised, limb for
// limb, without a GPU, and a bound the lane breaks shows as a count.
// Needs no library, only the compiler that builds it (the host arithmetic of host_field.hpp is written for clang's carry-chain intrinsics):
//   hipcc -x c++ -std=c++17 -O2 -mbmi2 -madx -I aleo_amd/csrc tests/cpp/records_lane_emul.cpp   (tests/test_records.py builds and runs it).
#include "checked_f29.h"

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
