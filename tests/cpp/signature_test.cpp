// Signature, sign, verify, verify_many and PrivateAccount::sign / verify of include/aleo_mi355x.hpp through the C ABI:
//   signature_test <private key> <address> <n>
// The account of the private key has the given address.  n messages are signed; each signature survives its string, verifies under the account and not over
// another message; of the n in one verify_many call every third has its message changed and every fifth is made malformed (a response of 2^256 - 1): the routed
// call returns what the host form returns, and that is 0, 1 and 3 where expected.  tests/test_signatures.py runs it on the host path and on the kernel.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main(int argc, char** argv) {
  if (argc != 4) { std::printf("usage: signature_test private_key address n\n"); return 2; }
  auto acct = account_from_private_key(argv[1]);
  auto addr = Address::from_string(argv[2]);
  const size_t n = (size_t)std::atoi(argv[3]);
  CHECK(acct.is_ok() && addr.is_ok());
  if (!acct.is_ok() || !addr.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
  CHECK(!std::memcmp(acct.value->address.x, addr.value->x, 32));
  std::vector<Signature> sigs; std::vector<std::string> messages; std::vector<uint8_t> want;
  for (size_t i = 0; i < n; ++i) {
    uint8_t seed[32]; std::memset(seed, 0, 32); seed[0] = (uint8_t)i; seed[1] = (uint8_t)(i >> 8); seed[31] = 0x5a;
    std::string m = "message " + std::to_string(i) + std::string(i % 70, '.');
    auto s = acct.value->sign(m.data(), m.size(), seed);
    CHECK(s.is_ok());
    if (!s.is_ok()) break;
    if (i < 4) {
      const std::string text = s.value->to_string();
      auto back = Signature::from_string(text);
      CHECK(text.rfind("sign1", 0) == 0 && back.is_ok() && !std::memcmp(back.value->bytes, s.value->bytes, 128));
      CHECK(acct.value->verify(m.data(), m.size(), *s.value) && verify(*s.value, *addr.value, m.data(), m.size()));
      CHECK(!acct.value->verify(m.data(), m.size() - 1, *s.value));
      auto again = sign(argv[1], m.data(), m.size(), seed);
      CHECK(again.is_ok() && !std::memcmp(again.value->bytes, s.value->bytes, 128));
    }
    uint8_t w = 0;
    if (i % 3 == 1) { m[0] ^= 1; w = 1; }
    if (i % 5 == 2) { std::memset(s.value->bytes + 32, 0xff, 32); w = 3; }
    sigs.push_back(*s.value); messages.push_back(m); want.push_back(w);
  }
  CHECK(!Signature::from_string(argv[2]).is_ok());
  PrivateAccount parts = *acct.value; parts.private_key.clear();
  CHECK(!parts.sign("x", 1, acct.value->sk_sig).is_ok());
  auto routed = verify_many(sigs, {*addr.value}, messages), host = verify_many(sigs, {*addr.value}, messages, true);
  CHECK(routed.is_ok() && host.is_ok());
  if (routed.is_ok() && host.is_ok()) CHECK(*routed.value == *host.value && *host.value == want);
  std::vector<Address> each(sigs.size(), *addr.value);
  if (each.size() > 1) { each[0].x[0] ^= 1; want[0] = want[0] == 3 ? 3 : 1; }
  auto per = verify_many(sigs, each, messages), per_host = verify_many(sigs, each, messages, true);
  CHECK(per.is_ok() && per_host.is_ok());
  if (per.is_ok() && per_host.is_ok() && each.size() > 1) CHECK(*per.value == *per_host.value && *per_host.value == want);
  CHECK(!verify_many(sigs, {}, messages).is_ok());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
