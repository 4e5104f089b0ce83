// sign_many and PrivateAccount::sign_many of include/aleo_mi355x.hpp through the C ABI:
//   signatures_sign_test <private key> <another private key> <address of the first> <n>
// n messages are signed in one call under the first key, and in one call under the two keys in turn: every row equals the one-signature call's for the same key,
// message and seed, the routed call returns what the host form returns, the rows of the first key verify under its address in one verify_many call, a message
// over the cap gets flag 3 and a row of zeros, and two equal seeds are refused.  tests/test_signatures_sign.py runs it on the host path and on the kernel.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main(int argc, char** argv) {
  if (argc != 5) { std::printf("usage: signatures_sign_test private_key other_private_key address n\n"); return 2; }
  auto acct = account_from_private_key(argv[1]);
  auto addr = Address::from_string(argv[3]);
  const size_t n = (size_t)std::atoi(argv[4]);
  CHECK(acct.is_ok() && addr.is_ok() && n >= 3);
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::vector<std::string> messages, keys;
  std::vector<uint8_t> seeds(32 * n, 0);
  for (size_t i = 0; i < n; ++i) {
    seeds[32 * i] = (uint8_t)i; seeds[32 * i + 1] = (uint8_t)(i >> 8); seeds[32 * i + 31] = 0xa5;
    messages.push_back("message " + std::to_string(i) + std::string(i % 70, '.'));
    keys.push_back(argv[1 + i % 2]);
  }
  messages[2] = std::string(131072, 'x');                        // one byte over the cap
  auto one = acct.value->sign_many(messages, seeds.data()), one_host = sign_many({argv[1]}, messages, seeds.data(), true);
  auto each = sign_many(keys, messages, seeds.data()), each_host = sign_many(keys, messages, seeds.data(), true);
  CHECK(one.is_ok() && one_host.is_ok() && each.is_ok() && each_host.is_ok());
  if (fails) { std::printf("%d FAILED: %s\n", fails, aleo_mi355x_last_error()); return 1; }
  const Signature zero = {};
  std::vector<Signature> mine; std::vector<std::string> mine_messages;
  for (size_t i = 0; i < n; ++i) {
    CHECK(!std::memcmp(one.value->signatures[i].bytes, one_host.value->signatures[i].bytes, 128) && one.value->flags[i] == one_host.value->flags[i]);
    CHECK(!std::memcmp(each.value->signatures[i].bytes, each_host.value->signatures[i].bytes, 128) && each.value->flags[i] == each_host.value->flags[i]);
    if (i == 2) { CHECK(one.value->flags[i] == 3 && each.value->flags[i] == 3 && !std::memcmp(one.value->signatures[i].bytes, zero.bytes, 128) && !std::memcmp(each.value->signatures[i].bytes, zero.bytes, 128)); continue; }
    CHECK(one.value->flags[i] == 0 && each.value->flags[i] == 0);
    auto s = sign(argv[1], messages[i].data(), messages[i].size(), seeds.data() + 32 * i), t = sign(keys[i], messages[i].data(), messages[i].size(), seeds.data() + 32 * i);
    CHECK(s.is_ok() && t.is_ok());
    if (!s.is_ok() || !t.is_ok()) break;
    CHECK(!std::memcmp(s.value->bytes, one.value->signatures[i].bytes, 128) && !std::memcmp(t.value->bytes, each.value->signatures[i].bytes, 128));
    mine.push_back(one.value->signatures[i]); mine_messages.push_back(messages[i]);
  }
  auto flags = verify_many(mine, {*addr.value}, mine_messages);
  CHECK(flags.is_ok() && *flags.value == std::vector<uint8_t>(mine.size(), 0));
  std::memcpy(seeds.data() + 32 * (n - 1), seeds.data(), 32);      // the last seed is the first again
  auto twice = sign_many({argv[1]}, messages, seeds.data());
  CHECK(!twice.is_ok() && twice.error.code == ALEO_MI355X_ERR_BAD_ARG && std::strstr(aleo_mi355x_last_error(), (" 0 and " + std::to_string(n - 1)).c_str()));
  PrivateAccount parts = *acct.value; parts.private_key.clear();
  CHECK(!parts.sign_many(messages, seeds.data()).is_ok());
  CHECK(!sign_many({argv[1], argv[2]}, messages, seeds.data()).is_ok() || n == 2);
  auto none = sign_many({argv[1]}, {}, nullptr);
  CHECK(none.is_ok() && none.value->signatures.empty());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
