// The string overloads of include/aleo_mi355x.hpp (RecordBatch; find_owned, find_owned_many, decrypt_owned) through the C ABI:
//   records_strings_test <view key> <address> <expected plaintext of every owned record, or ""> <record string>...
// Each must return from the strings what it returns from RecordCiphertext objects; with a string that does not parse in the batch each fails with what
// RecordCiphertext::from_string returns for it; and the raw call must equal its host form byte for byte.  tests/test_records_strings.py runs it with
// ALEO_MI355X_MIN_RECORDS=0, so that every scan here runs the kernels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static bool same(const std::vector<OwnedRecord>& a, const std::vector<OwnedRecord>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].index != b[i].index || a[i].has_view_key != b[i].has_view_key || std::memcmp(a[i].record_view_key_x, b[i].record_view_key_x, 32)) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 5) { std::printf("usage: records_strings_test view_key address plaintext record...\n"); return 2; }
  auto vk = ViewKey::from_string(argv[1]); auto addr = Address::from_string(argv[2]);
  CHECK(vk.is_ok() && addr.is_ok());
  if (!vk.is_ok() || !addr.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
  const std::string plaintext = argv[3];
  std::vector<std::string> strings(argv + 4, argv + argc);
  std::vector<RecordCiphertext> objects;
  for (const auto& s : strings) { auto r = RecordCiphertext::from_string(s); CHECK(r.is_ok()); if (r.is_ok()) objects.push_back(*r.value); }
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  RecordBatch batch(strings);
  std::string text; for (const auto& s : strings) text += s + "\n";
  RecordBatch lines = RecordBatch::from_text(text);
  CHECK(batch.size() == strings.size() && lines.size() == strings.size());
  for (size_t i = 0; i < strings.size(); ++i) CHECK(batch.string(i) == strings[i] && lines.string(i) == strings[i]);

  auto want = find_owned(objects, *vk.value, *addr.value); auto got = find_owned(batch, *vk.value, *addr.value); auto got_lines = find_owned(lines, *vk.value, *addr.value);
  CHECK(want.is_ok() && got.is_ok() && got_lines.is_ok());
  if (want.is_ok() && got.is_ok() && got_lines.is_ok()) { CHECK(same(*want.value, *got.value) && same(*want.value, *got_lines.value)); CHECK(!want.value->empty()); }
  std::vector<Account> accounts{Account{*vk.value, *addr.value}, Account{*vk.value, *addr.value}};
  auto many_want = find_owned_many(objects, accounts); auto many = find_owned_many(batch, accounts);
  CHECK(many_want.is_ok() && many.is_ok());
  if (many_want.is_ok() && many.is_ok()) { CHECK(many.value->size() == 2); for (size_t a = 0; a < many.value->size(); ++a) CHECK(same((*many_want.value)[a], (*many.value)[a])); }
  CHECK(find_owned_many(batch, std::vector<Account>{}).is_ok() && find_owned_many(batch, std::vector<Account>{}).value->empty());
  auto dec_want = decrypt_owned(objects, *vk.value, *addr.value); auto dec = decrypt_owned(batch, *vk.value, *addr.value);
  CHECK(dec_want.is_ok() && dec.is_ok());
  if (dec_want.is_ok() && dec.is_ok()) {
    CHECK(dec.value->size() == dec_want.value->size() && want.is_ok() && dec.value->size() == want.value->size());
    for (size_t j = 0; j < dec.value->size() && j < dec_want.value->size(); ++j) {
      CHECK((*dec.value)[j].index == (*dec_want.value)[j].index && (*dec.value)[j].plaintext.to_string() == (*dec_want.value)[j].plaintext.to_string());
      if (!plaintext.empty()) CHECK((*dec.value)[j].plaintext.to_string() == plaintext);
    }
  }
  // a string that does not parse: what from_string says of it
  std::vector<std::string> with_bad = strings; with_bad.insert(with_bad.begin() + 1, "garbage");
  RecordBatch bad(with_bad);
  const int32_t rc = RecordCiphertext::from_string("garbage").error.code;
  CHECK(rc != 0);
  CHECK(!find_owned(bad, *vk.value, *addr.value).is_ok() && find_owned(bad, *vk.value, *addr.value).error.code == rc);
  CHECK(!find_owned_many(bad, accounts).is_ok() && !find_owned_many(bad, std::vector<Account>{}).is_ok() && !decrypt_owned(bad, *vk.value, *addr.value).is_ok());
  // the raw call against its host form: the refused string is an answer, not a failure
  const size_t n = bad.size();
  std::vector<uint8_t> f1(n, 9), f2(n, 9), r1(32 * n, 9), r2(32 * n, 9); std::vector<int8_t> k1(n, 9), k2(n, 9);
  CHECK(aleo_mi355x_records_scan_strings(f1.data(), k1.data(), r1.data(), bad.text(), bad.offsets(), n, vk.value->scalar, addr.value->x, 1) == 0);
  CHECK(aleo_mi355x_records_scan_strings_host(f2.data(), k2.data(), r2.data(), bad.text(), bad.offsets(), n, vk.value->scalar, addr.value->x, 1) == 0);
  CHECK(f1 == f2 && k1 == k2 && r1 == r2 && f1[1] == 3 && k1[1] == -1);
  std::printf(fails ? "%d FAILED\n" : "ALL OK\n", fails);
  return fails ? 1 : 0;
}
