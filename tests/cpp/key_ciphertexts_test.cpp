// encrypt_private_key, decrypt_private_key, open_private_keys and PrivateAccount::from_ciphertext / to_ciphertext of include/aleo_mi355x.hpp through the C ABI:
//   key_ciphertexts_test <private key> <secret> <ciphertext> <corrupted ciphertext> <n>
// The ciphertext decrypts to the private key under the secret and under no other; the corrupted one is no ciphertext.  n pairs — keys from seeds made here,
// encrypted under secrets and nonces made here, every fifth with a wrong secret and every seventh a broken string — are opened in one routed call and on the host:
// the same flags and accounts, the accounts those of the keys.  tests/test_key_ciphertexts.py runs it on the host path and on the kernel.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static bool same_account(const PrivateAccount& a, const PrivateAccount& b) {
  return !std::memcmp(a.sk_sig, b.sk_sig, 32) && !std::memcmp(a.view_key.scalar, b.view_key.scalar, 32) && !std::memcmp(a.address.x, b.address.x, 32) && a.private_key == b.private_key;
}

int main(int argc, char** argv) {
  if (argc != 6) { std::printf("usage: key_ciphertexts_test private_key secret ciphertext corrupted_ciphertext n\n"); return 2; }
  const std::string key = argv[1], secret = argv[2], ciphertext = argv[3], corrupted = argv[4];
  const size_t n = (size_t)std::atoi(argv[5]);
  // one ciphertext
  auto plain = decrypt_private_key(ciphertext, secret);
  CHECK(plain.is_ok() && *plain.value == key);
  auto wrong = decrypt_private_key(ciphertext, secret + "x");
  CHECK(!wrong.is_ok() && wrong.error.code == ALEO_MI355X_ERR_NOT_OWNER);
  auto broken = decrypt_private_key(corrupted, secret);
  CHECK(!broken.is_ok() && broken.error.code == ALEO_MI355X_ERR_BAD_ARG);
  uint8_t nonce[32] = {5}, big[32]; std::memset(big, 0xff, 32);
  auto again = encrypt_private_key(key, secret, nonce), other = encrypt_private_key(key, secret, big);
  CHECK(again.is_ok() && again.value->size() == 174 && !other.is_ok());
  if (!again.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
  CHECK(*again.value != ciphertext && decrypt_private_key(*again.value, secret).is_ok() && *decrypt_private_key(*again.value, secret).value == key);
  auto account = PrivateAccount::from_ciphertext(ciphertext, secret), direct = account_from_private_key(key);
  CHECK(account.is_ok() && direct.is_ok());
  if (!account.is_ok() || !direct.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
  CHECK(same_account(*account.value, *direct.value));
  auto sealed = account.value->to_ciphertext(secret, nonce);
  CHECK(sealed.is_ok() && *sealed.value == *again.value);
  CHECK(!PrivateAccount::from_ciphertext(ciphertext, "").is_ok());
  // n pairs in one call
  std::vector<std::string> texts(n), secrets(n), keys(n); std::vector<uint8_t> want(n, 0);
  for (size_t i = 0; i < n; ++i) {
    uint8_t raw[32]; std::memset(raw, (int)(i * 41 + 3), 32); raw[0] = (uint8_t)i; raw[1] = (uint8_t)(i >> 8);
    auto k = private_key_from_seed(seed_from_bytes(raw));
    CHECK(k.is_ok());
    if (!k.is_ok()) break;
    keys[i] = *k.value;
    secrets[i] = std::string(i % 40, (char)('a' + i % 26)) + std::string(1, (char)(0x80 + i % 100));      // 1 to 40 bytes, the last no ASCII
    raw[2] ^= 0x5a;
    const KeySeed nc = seed_from_bytes(raw);                   // a nonce of its own
    auto c = encrypt_private_key(keys[i], secrets[i], nc.data());
    CHECK(c.is_ok());
    if (!c.is_ok()) break;
    texts[i] = *c.value;
    if (i % 5 == 2) { secrets[i] += "!"; want[i] = 1; }
    if (i % 7 == 4) { texts[i][20 + i % 100] = texts[i][20 + i % 100] == 'q' ? 'p' : 'q'; want[i] = 3; }
  }
  if (n) { texts[0] = ciphertext; secrets[0] = secret; keys[0] = key; want[0] = 0; }
  auto routed = open_private_keys(texts, secrets), host = open_private_keys(texts, secrets, true);
  CHECK(routed.is_ok() && host.is_ok());
  if (routed.is_ok() && host.is_ok()) {
    CHECK(routed.value->flags == want && host.value->flags == want && routed.value->accounts.size() == n);
    for (size_t i = 0; i < n && i < routed.value->accounts.size(); ++i) {
      CHECK(same_account(routed.value->accounts[i], host.value->accounts[i]));
      if (want[i]) { PrivateAccount zero{}; CHECK(same_account(routed.value->accounts[i], zero)); continue; }
      auto a = account_from_private_key(keys[i]);
      CHECK(a.is_ok() && same_account(routed.value->accounts[i], *a.value));
    }
  }
  CHECK(!open_private_keys(texts, {}).is_ok() || n == 0);
  auto none = open_private_keys({}, {});
  CHECK(none.is_ok() && none.value->accounts.empty());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
