// decrypt_strings_many and balances of include/aleo_mi355x.hpp through the C ABI:
//   records_found_many_test <accounts K> <view key> <address> (K times) <record string>...   (the last string: one that does not parse)
// Every account's result must equal, byte for byte, what decrypt_strings returns for it alone and what the host form of the call returns, its balance what
// balance returns, and a string that does not parse must fail balances as it fails balance.  tests/test_records_found_many.py runs it on the host path and, with
// ALEO_MI355X_MIN_RECORDS=0, on the kernels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static bool same(const aleo_mi355x_found* a, const aleo_mi355x_found* h) {
  const size_t c = aleo_mi355x_found_count(a), nf = aleo_mi355x_found_fields(a);
  if (c != aleo_mi355x_found_count(h) || nf != aleo_mi355x_found_fields(h)) return false;
  if (aleo_mi355x_found_unparsed(a) != aleo_mi355x_found_unparsed(h) || aleo_mi355x_found_first_unparsed(a) != aleo_mi355x_found_first_unparsed(h)) return false;
  return !std::memcmp(aleo_mi355x_found_index(a), aleo_mi355x_found_index(h), 4 * c) && !std::memcmp(aleo_mi355x_found_kind(a), aleo_mi355x_found_kind(h), c) &&
         !std::memcmp(aleo_mi355x_found_rvk(a), aleo_mi355x_found_rvk(h), 32 * c) && !std::memcmp(aleo_mi355x_found_offsets(a), aleo_mi355x_found_offsets(h), 4 * (c + 1)) &&
         !std::memcmp(aleo_mi355x_found_plain(a), aleo_mi355x_found_plain(h), 32 * nf) && !std::memcmp(aleo_mi355x_found_status(a), aleo_mi355x_found_status(h), c) &&
         !std::memcmp(aleo_mi355x_found_microcredits(a), aleo_mi355x_found_microcredits(h), 8 * c);
}

int main(int argc, char** argv) {
  const size_t K = argc > 1 ? std::strtoul(argv[1], nullptr, 10) : 0;
  if (K < 1 || (size_t)argc < 2 + 2 * K + 2) { std::printf("usage: records_found_many_test K (view_key address) x K record... unparsable\n"); return 2; }
  std::vector<Account> accounts; std::vector<uint8_t> vks, axs;
  for (size_t a = 0; a < K; ++a) {
    auto vk = ViewKey::from_string(argv[2 + 2 * a]); auto addr = Address::from_string(argv[3 + 2 * a]);
    CHECK(vk.is_ok() && addr.is_ok());
    if (!vk.is_ok() || !addr.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
    accounts.push_back(Account{*vk.value, *addr.value});
    vks.insert(vks.end(), vk.value->scalar, vk.value->scalar + 32); axs.insert(axs.end(), addr.value->x, addr.value->x + 32);
  }
  std::vector<std::string> strings(argv + 2 + 2 * K, argv + argc - 1);
  RecordBatch batch(strings);
  auto many = decrypt_strings_many(batch, accounts);
  auto sums = balances(batch, accounts);
  CHECK(many.is_ok() && sums.is_ok());
  size_t owned = 0;
  if (many.is_ok() && sums.is_ok()) {
    CHECK(many.value->size() == K && sums.value->size() == K);
    for (size_t a = 0; a < K && a < many.value->size(); ++a) {
      const FoundRecords& f = (*many.value)[a];
      auto one = decrypt_strings(batch, accounts[a].view_key, accounts[a].address);
      auto sum = balance(batch, accounts[a].view_key, accounts[a].address);
      CHECK(one.is_ok() && sum.is_ok());
      if (!one.is_ok() || !sum.is_ok()) continue;
      CHECK(f.size() == one.value->size() && f.total_fields() == one.value->total_fields() && f.unparsed() == 0 && f.first_unparsed() == strings.size());
      if (f.size() == one.value->size() && f.total_fields() == one.value->total_fields()) {
        CHECK(!std::memcmp(f.index(), one.value->index(), 4 * f.size()) && !std::memcmp(f.offsets(), one.value->offsets(), 4 * (f.size() + 1)) && !std::memcmp(f.status(), one.value->status(), f.size()));
        CHECK(!std::memcmp(f.microcredits(), one.value->microcredits(), 8 * f.size()) && !std::memcmp(f.kind(), one.value->kind(), f.size()));
        if (f.size()) CHECK(!std::memcmp(f.rvk(0), one.value->rvk(0), 32 * f.size()) && !std::memcmp(f.fields(0), one.value->fields(0), 32 * f.total_fields()));
      }
      CHECK((*sums.value)[a].microcredits == sum.value->microcredits && (*sums.value)[a].indices == sum.value->indices);
      owned += f.size();
    }
    CHECK(owned > 0);
  }
  // the routed call against its host form, byte for byte, with the string that does not parse in the middle
  std::vector<std::string> with_bad = strings; with_bad.insert(with_bad.begin() + 1, argv[argc - 1]);
  RecordBatch bad(with_bad);
  std::vector<aleo_mi355x_found*> a(K, nullptr), h(K, nullptr);
  CHECK(aleo_mi355x_records_decrypt_strings_many(a.data(), bad.text(), bad.offsets(), bad.size(), vks.data(), axs.data(), K) == 0);
  CHECK(aleo_mi355x_records_decrypt_strings_many_host(h.data(), bad.text(), bad.offsets(), bad.size(), vks.data(), axs.data(), K) == 0);
  for (size_t j = 0; j < K; ++j) {
    CHECK(a[j] && h[j]);
    if (a[j] && h[j]) CHECK(same(a[j], h[j]) && aleo_mi355x_found_unparsed(a[j]) == 1 && aleo_mi355x_found_first_unparsed(a[j]) == 1);
    aleo_mi355x_found_free(a[j]); aleo_mi355x_found_free(h[j]);
  }
  const int32_t rc = RecordCiphertext::from_string(argv[argc - 1]).error.code;
  CHECK(rc != 0 && !balances(bad, accounts).is_ok() && balances(bad, accounts).error.code == rc);
  // nothing to search, nobody to search for, too many to search for
  auto none = decrypt_strings_many(RecordBatch(std::vector<std::string>{}), accounts);
  CHECK(none.is_ok() && none.value->size() == K);
  if (none.is_ok()) for (const FoundRecords& f : *none.value) CHECK(f.size() == 0 && f.total_fields() == 0 && f.offsets()[0] == 0);
  auto nobody = balances(batch, std::vector<Account>{});
  CHECK(nobody.is_ok() && nobody.value->empty());
  CHECK(!decrypt_strings_many(batch, std::vector<Account>(65, accounts[0])).is_ok());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
