// The record decryption's device lane (aleo_amd/csrc/records_decrypt_lane.h) run on the HOST, against what the library's host path computes:
// plain_i = c_i - hash_many_psd8([encryption domain, rvk], m)_i through host::poseidon_hash_many_fr<8> (poseidon.hpp).
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of
// fr29.h is a check there, so a bound the lane breaks — the state it carries from one permutation into the next, the subtrahend of the last step — shows as a count.
//   hipcc -x c++ -std=c++17 -O2 -mbmi2 -madx -I aleo_amd/csrc tests/cpp/records_decrypt_lane_emul.cpp   (tests/test_records_decrypt.py builds and runs it).
#include "checked_f29.h"
#include "records_decrypt_lane.h"
#include <vector>

int main() {
  const RecordsConsts& C = records_consts();
  const HFr dom = host::fr_domain_separator("AleoSymmetricEncryption0");
  static const int counts[] = {0, 1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 40};
  unsigned long bad = 0, malformed = 0, records = 0, fields = 0, wrapped = 0;
  for (int round = 0; round < 6; ++round)
    for (int m : counts) {
      uint8_t rvk[32]; rnd_fr(rvk);
      std::vector<uint8_t> c(32 * (size_t)m + 32), want(32 * (size_t)m + 32, 0), got(32 * (size_t)m + 32, 0xee);
      for (int j = 0; j < m; ++j) rnd_fr(c.data() + 32 * j);
      if (round == 1) std::memset(rvk, 0, 32);                            // rvk = 0
      if (round == 2 && m) std::memset(c.data(), 0, 32);                  // c = 0: the difference wraps below zero
      if (round == 3) std::memcpy(rvk, host::HParams<4>::P, 32);          // rvk = r
      if (round == 4 && m) std::memset(c.data() + 32 * (m - 1), 0xff, 32);      // the last field is not below r
      if (round == 5 && m > 1) std::memcpy(c.data(), host::HParams<4>::P, 32);  // the first field is exactly r
      // the host path
      HFr rv; std::memcpy(rv.l, rvk, 32);
      bool is_bad = HFr::geq_p(rv.l);
      for (int j = 0; j < m; ++j) { HFr f; std::memcpy(f.l, c.data() + 32 * j, 32); is_bad = is_bad || HFr::geq_p(f.l); }
      if (!is_bad && m) {
        const HFr in[2] = {dom, HFr::to_mont(rv)}; std::vector<HFr> rnd(m);
        host::poseidon_hash_many_fr<8>(in, 2, rnd.data(), m);
        for (int j = 0; j < m; ++j) {
          HFr f; std::memcpy(f.l, c.data() + 32 * j, 32);
          const HFr r = HFr::from_mont(rnd[j]); bool below = false;
          for (int q = 3; q >= 0; --q) { if (f.l[q] < r.l[q]) { below = true; break; } if (f.l[q] > r.l[q]) break; }
          wrapped += below;
          const HFr o = HFr::from_mont(HFr::sub(HFr::to_mont(f), rnd[j])); std::memcpy(want.data() + 32 * j, o.l, 32);
        }
      }
      // the lane, in place as the kernel runs it
      std::memcpy(got.data(), c.data(), 32 * (size_t)m);
      uint32_t rw[8]; std::memcpy(rw, rvk, 32);
      uint32_t emitted = 0, order_ok = 1;
      const uint32_t flag = records_decrypt_lane(rw, (uint32_t)m, C.words.data(),
        [&](uint32_t j, uint32_t (&w)[8]) { std::memcpy(w, got.data() + 32 * j, 32); },
        [&](uint32_t j, const F29& v) { uint32_t w[8]; f29_to_words(v, w); std::memcpy(got.data() + 32 * j, w, 32); order_ok &= j == emitted; ++emitted; });
      if (flag != (is_bad ? 2u : 0u) || emitted != (uint32_t)m || !order_ok || std::memcmp(got.data(), want.data(), 32 * (size_t)m)) {
        if (bad++ < 5) std::fprintf(stderr, "round %d m %d: lane flag %u (host %u), %u rows emitted, rows %s\n", round, m, flag, is_bad ? 2u : 0u, emitted, std::memcmp(got.data(), want.data(), 32 * (size_t)m) ? "differ" : "equal");
      }
      malformed += is_bad; ++records; fields += m;
    }
  std::printf("records_decrypt_lane_emul: %lu records, %lu fields, %lu malformed, %lu differences wrapped, %lu mismatches, %lu limb-rule violations\n", records, fields, malformed, wrapped, bad, g_violations);
  return bad || g_violations || !malformed || !wrapped ? 1 : 0;
}
