// The private-key-ciphertext kernel's device lane (aleo_amd/csrc/key_ciphertext_lane.h) run on the HOST, pair by pair against the bytes the library's host path
// returned (aleo_mi355x_private_keys_open_host) and against key_ciphertext_host.hpp's open_one_host compiled into this program, with the table built by
// key_ciphertext_host.hpp as the library builds it and the secret handed over as the kernel gets it (kct::device_secret: a long one reduced by the host).
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of
// fr29.h is a check there, so a bound the lane breaks shows as a count.  Every character and every secret byte the lane asks for is checked against the length
// of what it was given, and both are held in buffers of exactly that length.  Plain C++ for the host compiler, built once plain and once with the address and
// undefined-behaviour sanitizers and run as a program of its own (tests/test_key_ciphertexts.py):
//   g++ -std=c++17 -O2 -fno-strict-aliasing -mbmi2 -madx [-fsanitize=address,undefined] -I aleo_amd/csrc tests/cpp/key_ciphertext_lane_emul.cpp
//   key_ciphertext_lane_emul <case file>
// The file: u32 count, then per pair: u32 length and the characters of the string, u32 length and the bytes of the secret, u8 the flag wanted, the 32 bytes of
// the seed wanted (zeros with a flag).
#include "checked_f29.h"
#include "key_ciphertext_host.hpp"
#include <vector>


int main(int argc, char** argv) {
  uint32_t count = 0;
  std::FILE* f = open_cases(argc, argv, &count);
  if (!f) return 2;
  const kct::KeyCiphertextTables& T = kct::key_ciphertext_tables();
  unsigned long flags[4] = {0, 0, 0, 0}, bad = 0, past = 0;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t tl = 0, sl = 0; uint8_t want_flag, want_seed[32];
    if (!get(f, &tl, 4) || tl > (1u << 22)) return 2;
    std::vector<uint8_t> text(tl);
    if (!get(f, text.data(), tl) || !get(f, &sl, 4) || sl > (1u << 16)) return 2;
    std::vector<uint8_t> secret(sl);
    if (!get(f, secret.data(), sl) || !get(f, &want_flag, 1) || !get(f, want_seed, 32)) return 2;
    uint8_t dev[KC_MAX_DEVICE_SECRET];
    const uint32_t dl = kct::device_secret(dev, secret.data(), sl);
    std::vector<uint8_t> dsec(dev, dev + dl);                    // exact: a read past the end is the sanitizer's
    uint32_t c[3][8], sw[8], seed[8];
    const uint32_t status = kc_decode([&](uint32_t j) -> uint8_t { if (j >= tl) { ++past; return 0; } return text[j]; }, tl, c);
    kc_secret_words([&](uint32_t j) -> uint8_t { if (j >= dl) { ++past; return 0; } return dsec[j]; }, dl, sw);
    const uint32_t flag = key_ciphertext_lane(status, c, sw, T.words.data(), seed, [] {});
    uint8_t got[32]; std::memcpy(got, seed, 32);
    if (flag) { bool all_ff = true; for (int k = 0; k < 32; ++k) all_ff = all_ff && got[k] == 0xff; if (!all_ff) { if (bad++ < 8) std::fprintf(stderr, "pair %u: a flagged lane's seed is not 32 x 0xff\n", i); } std::memset(got, 0, 32); }
    uint8_t host_seed[32];
    const uint32_t host_flag = kct::open_one_host(host_seed, (const char*)text.data(), tl, secret.data(), sl);
    const bool same = flag == want_flag && host_flag == want_flag && !std::memcmp(got, want_seed, 32) && !std::memcmp(host_seed, want_seed, 32);
    if (!same && bad++ < 8) std::fprintf(stderr, "pair %u: lane flag %u, host flag %u, wanted %u; lane seed %s, host seed %s\n", i, flag, host_flag, (unsigned)want_flag,
                                         std::memcmp(got, want_seed, 32) ? "differs" : "equal", std::memcmp(host_seed, want_seed, 32) ? "differs" : "equal");
    ++flags[flag & 3u];
  }
  std::fclose(f);
  std::printf("key_ciphertext_lane_emul: %u pairs, %lu opened, %lu not decrypted, %lu no ciphertext, %lu mismatches, %lu reads past an end, %lu limb-rule violations\n",
              count, flags[0], flags[1], flags[3], bad, past, g_violations);
  return bad || past || g_violations ? 1 : 0;
}
