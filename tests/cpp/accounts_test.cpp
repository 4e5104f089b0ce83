// derive_accounts, accounts_from_private_keys, account_from_seed, search_accounts and the seed and key strings of include/aleo_mi355x.hpp through the C ABI:
//   accounts_test <private key> <address> <n>
// The account of the private key has the given address.  n seeds are derived in one routed call and on the host: the same accounts, whose address strings are
// those bech32m_encode gives; the private key comes back from its seed; a search of max(n, 64) candidates for the prefix "q" returns on the routed path what it
// returns on the host, hits whose addresses begin with "aleo1q" and whose private keys derive them.  tests/test_accounts.py runs it on the host path and on the kernel.
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
  if (argc != 4) { std::printf("usage: accounts_test private_key address n\n"); return 2; }
  const std::string key = argv[1], address = argv[2];
  const size_t n = (size_t)std::atoi(argv[3]);
  // the strings
  auto seed = private_key_seed(key);
  CHECK(seed.is_ok());
  if (!seed.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
  auto back = private_key_from_seed(*seed.value);
  CHECK(back.is_ok() && *back.value == key);
  CHECK(!private_key_seed(address).is_ok() && !private_key_seed("APrivateKey1nonsense").is_ok());
  KeySeed ones; ones.fill(0xff);
  CHECK(!private_key_from_seed(ones).is_ok());
  CHECK(seed_from_bytes(seed.value->data()) == *seed.value);           // below r: unchanged
  CHECK(seed_from_bytes(ones.data()) != ones && private_key_from_seed(seed_from_bytes(ones.data())).is_ok());
  // one account, three ways
  auto one = account_from_private_key(key);
  auto many = accounts_from_private_keys({key, key}), many_host = accounts_from_private_keys({key, key}, true);
  auto from_seed = account_from_seed(seed.value->data());
  CHECK(one.is_ok() && many.is_ok() && many_host.is_ok() && from_seed.is_ok());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  CHECK(many.value->size() == 2 && same_account((*many.value)[0], *one.value) && same_account((*many.value)[1], *one.value) && same_account((*many_host.value)[1], *one.value));
  CHECK(same_account(*from_seed.value, *one.value));
  auto addr = Address::from_string(address);
  CHECK(addr.is_ok() && !std::memcmp(addr.value->x, one.value->address.x, 32));
  CHECK(view_key_to_string(one.value->view_key).rfind("AViewKey1", 0) == 0 && ViewKey::from_string(view_key_to_string(one.value->view_key)).is_ok());
  // n seeds in one call
  std::vector<KeySeed> seeds(n);
  for (size_t i = 0; i < n; ++i) { uint8_t raw[32]; std::memset(raw, (int)(i * 37 + 1), 32); raw[0] = (uint8_t)i; raw[1] = (uint8_t)(i >> 8); seeds[i] = seed_from_bytes(raw); }
  if (n) seeds[0] = *seed.value;
  std::vector<std::string> text, text_host;
  auto routed = derive_accounts(seeds, false, &text), host = derive_accounts(seeds, true, &text_host);
  CHECK(routed.is_ok() && host.is_ok());
  if (routed.is_ok() && host.is_ok()) {
    CHECK(routed.value->size() == n && host.value->size() == n && text == text_host && text.size() == n);
    for (size_t i = 0; i < n; ++i) {
      CHECK(same_account((*routed.value)[i], (*host.value)[i]));
      char want[80];
      CHECK(aleo_mi355x_bech32m_encode(want, sizeof want, "aleo", (*host.value)[i].address.x, 32) == 0 && text[i] == want);
    }
    if (n) CHECK(same_account((*routed.value)[0], *one.value) && text[0] == address);
  }
  std::vector<KeySeed> with_bad = seeds; with_bad.push_back(ones);
  CHECK(!derive_accounts(with_bad).is_ok() && !derive_accounts(with_bad, true).is_ok());
  // a search
  uint8_t master[32]; for (int i = 0; i < 32; ++i) master[i] = (uint8_t)(7 * i + 3);
  const uint64_t count = n > 64 ? n : 64;
  for (size_t max_hits : {(size_t)1, (size_t)2, (size_t)1000}) {
    auto found = search_accounts(master, "q", 0, count, max_hits), found_host = search_accounts(master, "q", 0, count, max_hits, true);
    CHECK(found.is_ok() && found_host.is_ok());
    if (!found.is_ok() || !found_host.is_ok()) continue;
    CHECK(found.value->index == found_host.value->index && found.value->next == found_host.value->next && found.value->accounts.size() == found.value->index.size());
    CHECK(found.value->index.size() <= max_hits && (found.value->index.size() == max_hits ? found.value->next == found.value->index.back() + 1 : found.value->next == count));
    for (size_t i = 0; i < found.value->accounts.size(); ++i) {
      const PrivateAccount& a = found.value->accounts[i];
      char text63[80];
      CHECK(aleo_mi355x_bech32m_encode(text63, sizeof text63, "aleo", a.address.x, 32) == 0 && !std::strncmp(text63, "aleo1q", 6));
      auto again = account_from_private_key(a.private_key);
      CHECK(again.is_ok() && same_account(*again.value, a) && same_account(found_host.value->accounts[i], a));
    }
  }
  CHECK(!search_accounts(master, "b", 0, count).is_ok() && !search_accounts(master, "qqqqqqqqqqqqq", 0, count).is_ok() && search_accounts(master, "", 0, 1).is_ok());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
