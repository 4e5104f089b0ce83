// plaintext_commitments, plaintext_serial_numbers, plaintexts_unspent and plaintext_microcredits of include/aleo_mi355x.hpp through the C ABI:
//   plaintexts_test <private key> <program id> <record name> <expected serial number: 64 hex digits> <microcredits> <plaintext string> <a string that is no record>
// Seventy copies of the plaintext with the other string at every tenth place: the routed calls equal their host forms byte for byte, the plaintext's serial number
// under the private key's sk_sig is the expected one, with it spent nothing is unspent, and a bad program id fails with the reference's text.
// tests/test_plaintexts.py runs it on the host path and on the kernel.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static bool hex32(const char* s, uint8_t* out) {
  if (std::strlen(s) != 64) return false;
  for (int i = 0; i < 32; ++i) { unsigned v; if (std::sscanf(s + 2 * i, "%2x", &v) != 1) return false; out[i] = (uint8_t)v; }
  return true;
}

int main(int argc, char** argv) {
  uint8_t expected[32];
  if (argc != 8 || !hex32(argv[4], expected)) { std::printf("usage: plaintexts_test private_key program_id record_name serial_number microcredits plaintext other\n"); return 2; }
  auto acct = account_from_private_key(argv[1]);
  CHECK(acct.is_ok());
  if (!acct.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
  const std::string program_id = argv[2], record_name = argv[3];
  const uint64_t microcredits = std::strtoull(argv[5], nullptr, 10);
  std::vector<std::string> strings;
  for (int i = 0; i < 70; ++i) strings.push_back(i % 10 == 9 ? argv[7] : argv[6]);
  const size_t n = strings.size();
  RecordBatch batch(strings);
  auto mc = plaintext_microcredits(argv[6]);
  CHECK(mc.is_ok() && *mc.value == microcredits && !plaintext_microcredits(argv[7]).is_ok());
  auto cms = plaintext_commitments(batch, program_id, record_name);
  auto rows = plaintext_serial_numbers(batch, program_id, record_name, acct.value->sk_sig);
  CHECK(cms.is_ok() && rows.is_ok());
  if (cms.is_ok() && rows.is_ok()) {
    std::vector<uint8_t> sn(32 * n), cm(32 * n), flags(n, 9); std::vector<uint64_t> m(n, 9);
    CHECK(aleo_mi355x_plaintexts_serial_numbers_host(sn.data(), cm.data(), m.data(), flags.data(), batch.text(), batch.offsets(), n, program_id.c_str(), record_name.c_str(), acct.value->sk_sig, nullptr, 0) == 0);
    CHECK(sn == rows.value->serials && cm == rows.value->commitments && flags == rows.value->flags && m == rows.value->microcredits);
    CHECK(cm == cms.value->commitments && flags == cms.value->flags && m == cms.value->microcredits);
    for (size_t i = 0; i < n; ++i) {
      if (i % 10 == 9) CHECK(flags[i] == 3 && m[i] == 0);
      else CHECK(flags[i] == 0 && m[i] == microcredits && !std::memcmp(rows.value->serial(i), expected, 32));
    }
  }
  auto all = plaintexts_unspent(batch, program_id, record_name, *acct.value);
  auto none = plaintexts_unspent(batch, program_id, record_name, *acct.value, expected, 1);
  CHECK(all.is_ok() && all.value->size() == 63 && none.is_ok() && none.value->empty());
  CHECK(!plaintext_commitments(batch, "credits", record_name).is_ok() && std::string(aleo_mi355x_last_error()) == "Invalid ProgramID specified");
  CHECK(!plaintext_serial_numbers(batch, program_id, "9lives", acct.value->sk_sig).is_ok() && std::string(aleo_mi355x_last_error()) == "Invalid Identifier specified for record");
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
