// The signing kernels' device lanes (aleo_amd/csrc/signature_sign_lane.h, and account_lane.h with the sink that hands out pk_sig.x and pr_sig.x) run on the HOST:
// first the product and the difference modulo the group order alone, row by row against numbers the test computed with Python integers; then signature by
// signature — the key row from the derive lane as k_signer_keys builds it, the signature from the signing lane as k_signatures_sign runs it — against the bytes the
// library's host path returned (aleo_mi355x_signatures_sign_host) and against signature_host.hpp's sign_with_nonce compiled into this program, with the table
// built by account_host.hpp as the library builds it.
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of
// fr29.h is a check there, so a bound a lane breaks shows as a count.  A lane must never ask for a byte past its message's end, and stores each part of its row
// once.  Plain C++ for the host compiler, built once plain and once with the address and undefined-behaviour sanitizers and run as a program of its own
// (tests/test_signatures_sign.py):
//   g++ -std=c++17 -O2 -fno-strict-aliasing -mbmi2 -madx [-fsanitize=address,undefined] -I aleo_amd/csrc tests/cpp/signature_sign_lane_emul.cpp
//   signature_sign_lane_emul <case file>
// The file: u32 count, then per product: 32 bytes each of k, c, s and of k - c s mod l; u32 count, then per signature: the 32 bytes of the key's seed, the 32 of the
// nonce seed, u32 length and the bytes of the message, u8 the flag wanted, the 128 bytes wanted.
#include "checked_f29.h"
#include "account_host.hpp"
#include "signature_sign_lane.h"
#include <vector>


int main(int argc, char** argv) {
  std::FILE* f = open_cases(argc, argv);
  if (!f) return 2;
  unsigned long bad = 0, past = 0, flags[4] = {0, 0, 0, 0};
  uint32_t products = 0, count = 0;
  if (!get(f, &products, 4)) return 2;
  for (uint32_t i = 0; i < products; ++i) {
    uint32_t k[8], c[8], s[8], want[8], t[8], got[8];
    if (!get(f, k, 32) || !get(f, c, 32) || !get(f, s, 32) || !get(f, want, 32)) return 2;
    sg_mul_mod_order(t, c, s);
    sg_sub_mod_order(got, k, t);
    uint64_t hc[4], hs[4], hk[4], ht[4], hr[4];                  // and the host path's two functions, which define the value
    std::memcpy(hc, c, 32); std::memcpy(hs, s, 32); std::memcpy(hk, k, 32);
    sig::scalar_mul(ht, hc, hs); sig::scalar_sub(hr, hk, ht);
    if ((std::memcmp(got, want, 32) || std::memcmp(hr, want, 32)) && bad++ < 8) std::fprintf(stderr, "product %u: lane %s, host %s\n", i, std::memcmp(got, want, 32) ? "differs" : "equal", std::memcmp(hr, want, 32) ? "differs" : "equal");
  }
  if (!get(f, &count, 4)) return 2;
  const acct::AccountTables& T = acct::account_tables();
  const uint32_t* K = T.words.data();
  for (uint32_t i = 0; i < count; ++i) {
    uint8_t key_seed[32], nonce_seed[32], want_flag, want[128]; uint32_t len;
    if (!get(f, key_seed, 32) || !get(f, nonce_seed, 32) || !get(f, &len, 4) || len > (1u << 22)) return 2;
    std::vector<uint8_t> msg(len);                               // exact: a read past the end is the sanitizer's
    if (!get(f, msg.data(), len) || !get(f, &want_flag, 1) || !get(f, want, 128)) return 2;
    // the key row, as k_signer_keys fills it
    uint32_t seedw[8], row[4][8];
    std::memcpy(seedw, key_seed, 32); std::memset(row, 0xee, sizeof row);
    AccountWords a;
    unsigned sunk = 0;
    const uint32_t key_flag = account_lane(seedw, K, a, [] {}, [&](const F29& pkx, const F29& prx) {
      f29_to_words(f29_canonical(pkx), row[1]); f29_to_words(f29_canonical(prx), row[2]); ++sunk; });
    std::memcpy(row[0], a.sk_sig, 32); std::memcpy(row[3], a.address, 32);
    const uint32_t host_key_flag = acct::derive_one_host(key_seed, nullptr, nullptr, nullptr);
    sig::SignerKeys keys; std::memset(&keys, 0, sizeof keys);
    if (!host_key_flag) {
      keys = acct::signer_keys_of_seed(key_seed);
      if (std::memcmp(row[0], keys.sk_sig, 32) || std::memcmp(row[1], keys.pk_x, 32) || std::memcmp(row[2], keys.pr_x, 32) || std::memcmp(row[3], keys.address_x, 32)) { if (bad++ < 8) std::fprintf(stderr, "signature %u: the derive lane's key row differs from the host's\n", i); }
    }
    if (key_flag != host_key_flag || sunk != 1) { if (bad++ < 8) std::fprintf(stderr, "signature %u: derive lane flag %u, host %u, sink calls %u\n", i, key_flag, host_key_flag, sunk); }
    // the signature
    uint32_t nseed[8]; std::memcpy(nseed, nonce_seed, 32);
    uint8_t got[128]; std::memset(got, 0xee, 128);
    unsigned stored[4] = {0, 0, 0, 0};
    auto byte = [&](uint32_t q) { if (q >= len) { ++past; return (uint8_t)0; } return msg[q]; };
    const uint32_t flag = signature_sign_lane(nseed, [&](uint32_t k, uint32_t (&w)[8]) { if (k > 3) { ++past; k = 0; } std::memcpy(w, row[k], 32); }, key_flag, len, byte, K,
                                              [&](uint32_t k, const uint32_t (&w)[8]) { if (k > 3) { ++past; return; } ++stored[k]; std::memcpy(got + 32 * k, w, 32); }, [] {});
    if (stored[0] != 1 || stored[1] != 1 || stored[2] != 1 || stored[3] != 1) ++past;
    uint8_t host[128]; std::memset(host, 0, 128);
    const uint32_t host_flag = host_key_flag || len > SIG_MAX_BYTES ? SIGN_REFUSED : SIGN_OK;
    if (!host_flag) { uint64_t nonce[4]; sig::nonce_of_seed(nonce, nonce_seed); sig::sign_with_nonce(host, keys, nonce, msg.data(), len); }
    const bool same = flag == want_flag && host_flag == want_flag && !std::memcmp(got, want, 128) && !std::memcmp(host, want, 128);
    if (!same && bad++ < 8) std::fprintf(stderr, "signature %u: lane flag %u, host flag %u, wanted %u; lane row %s, host row %s\n", i, flag, host_flag, (unsigned)want_flag,
                                         std::memcmp(got, want, 128) ? "differs" : "equal", std::memcmp(host, want, 128) ? "differs" : "equal");
    ++flags[flag & 3u];
  }
  std::fclose(f);
  std::printf("signature_sign_lane_emul: %u products, %u signatures, %lu signed, %lu refused, %lu mismatches, %lu reads past an end, %lu limb-rule violations\n",
              products, count, flags[0], flags[3], bad, past, g_violations);
  return bad || past || g_violations ? 1 : 0;
}
