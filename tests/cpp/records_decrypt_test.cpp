// The record-decryption mirror of include/aleo_mi355x.hpp through the C ABI: view key string, address string, the indices the account owns ("3,17,…"), the
// plaintext string every owned record must give ("" = not checked), then the record strings (tests/test_records_decrypt.py passes the reference's own among
// synthetic ones).  decrypt_owned against find_owned, against RecordCiphertext::decrypt one by one, and records_decrypt_fields against its host path.
// With ALEO_MI355X_MIN_RECORDS=0 and ALEO_MI355X_MIN_DECRYPT=0 the scan and the decryption here run their kernels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main(int argc, char** argv) {
  if (argc < 6) { std::printf("usage: records_decrypt_test view_key address indices expected_string record...\n"); return 2; }
  auto vk = ViewKey::from_string(argv[1]); auto addr = Address::from_string(argv[2]);
  CHECK(vk.is_ok() && addr.is_ok());
  if (!vk.is_ok() || !addr.is_ok()) return 1;
  std::vector<size_t> want;
  for (const char* p = argv[3]; *p;) { char* end; want.push_back(std::strtoul(p, &end, 10)); p = *end ? end + 1 : end; }
  const std::string expected = argv[4];
  std::vector<RecordCiphertext> batch;
  for (int a = 5; a < argc; ++a) { auto r = RecordCiphertext::from_string(argv[a]); CHECK(r.is_ok()); if (r.is_ok()) batch.push_back(*r.value); }
  auto got = decrypt_owned(batch, *vk.value, *addr.value);
  auto found = find_owned(batch, *vk.value, *addr.value);
  CHECK(got.is_ok() && found.is_ok());
  if (!got.is_ok() || !found.is_ok()) { std::printf("%s\n", got.error.message().c_str()); return 1; }
  CHECK(got.value->size() == want.size() && found.value->size() == want.size());
  Address other = *addr.value; other.x[0] ^= 1;
  for (size_t k = 0; k < got.value->size() && k < want.size(); ++k) {
    const DecryptedRecord& d = (*got.value)[k];
    CHECK(d.index == want[k] && (*found.value)[k].index == want[k]);
    auto one = batch[d.index].decrypt(*vk.value, *addr.value);
    CHECK(one.is_ok() && one.value->to_string() == d.plaintext.to_string());
    if (!expected.empty()) CHECK(d.plaintext.to_string() == expected && d.plaintext.microcredits() == 1500000000000000ull);
    auto wrong = batch[d.index].decrypt(*vk.value, other);
    CHECK(!wrong.is_ok() && wrong.error.not_owner());
    // the fields of this record alone: the routed call and the host path give the same bytes
    auto f = batch[d.index].fields();
    CHECK(f.is_ok());
    if (!f.is_ok() || !(*found.value)[k].has_view_key) continue;
    const uint32_t offsets[2] = {0, (uint32_t)(f.value->size() / 32)};
    std::vector<uint8_t> p1(f.value->size()), p2(f.value->size()); uint8_t f1 = 9, f2 = 9;
    CHECK(aleo_mi355x_records_decrypt_fields(p1.data(), &f1, (*found.value)[k].record_view_key_x, offsets, f.value->data(), 1) == 0);
    CHECK(aleo_mi355x_records_decrypt_fields_host(p2.data(), &f2, (*found.value)[k].record_view_key_x, offsets, f.value->data(), 1) == 0);
    CHECK(f1 == 0 && f2 == 0 && p1 == p2);
    auto again = batch[d.index].plaintext(p1.data(), offsets[1], *addr.value);
    CHECK(again.is_ok() && again.value->to_string() == d.plaintext.to_string());
  }
  CHECK(!RecordPlaintext("{\n  owner: x.private,\n  microcredits: 5u32.private,\n  _nonce: 0group.public\n}").microcredits());
  std::printf(fails ? "%d FAILED\n" : "ALL OK\n", fails);
  return fails ? 1 : 0;
}
