// find_owned_many of include/aleo_mi355x.hpp through the C ABI: groups of four arguments — record string, view key string, address string, expected 1 / 0
// (tests/test_records_many.py passes the reference's own assertions).  Every group's account is asked about every group's record in ONE call; the answer must
// be what find_owned gives account by account, must hold the expected booleans, and the raw call must equal its host form byte for byte.  With
// ALEO_MI355X_MIN_RECORDS=0 every scan here runs the kernels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 1) % 4) { std::printf("usage: records_scan_many_test (record view_key address expected)...\n"); return 2; }
  std::vector<RecordCiphertext> batch; std::vector<Account> accounts; std::vector<bool> expected;
  for (int a = 1; a + 3 < argc; a += 4) {
    auto rec = RecordCiphertext::from_string(argv[a]); auto vk = ViewKey::from_string(argv[a + 1]); auto addr = Address::from_string(argv[a + 2]);
    CHECK(rec.is_ok() && vk.is_ok() && addr.is_ok());
    if (!rec.is_ok() || !vk.is_ok() || !addr.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
    batch.push_back(*rec.value); accounts.push_back(Account{*vk.value, *addr.value}); expected.push_back(std::atoi(argv[a + 3]) != 0);
  }
  const size_t k = accounts.size(), n = batch.size();
  auto many = find_owned_many(batch, accounts);
  CHECK(many.is_ok());
  if (many.is_ok()) {
    CHECK(many.value->size() == k);
    for (size_t a = 0; a < k && a < many.value->size(); ++a) {
      auto one = find_owned(batch, accounts[a].view_key, accounts[a].address);
      CHECK(one.is_ok());
      if (!one.is_ok()) continue;
      const auto& got = (*many.value)[a];
      CHECK(got.size() == one.value->size());
      bool has_own = false;
      for (size_t i = 0; i < got.size() && i < one.value->size(); ++i) {
        const auto& w = (*one.value)[i];
        CHECK(got[i].index == w.index && got[i].has_view_key == w.has_view_key && !std::memcmp(got[i].record_view_key_x, w.record_view_key_x, 32));
        has_own = has_own || got[i].index == a;
      }
      CHECK(has_own == expected[a]);                             // group a's account and group a's record: the reference's assertion
    }
  }
  CHECK(find_owned_many(batch, {}).is_ok() && find_owned_many(batch, {}).value->empty());
  CHECK(find_owned_many({}, accounts).is_ok() && find_owned_many({}, accounts).value->size() == k);
  // the raw call against its host form, and a refused key
  std::vector<uint8_t> c0, nx, vks, axs;
  for (const auto& r : batch) { c0.insert(c0.end(), r.owner_field(), r.owner_field() + 32); nx.insert(nx.end(), r.nonce_x(), r.nonce_x() + 32); }
  for (const auto& a : accounts) { vks.insert(vks.end(), a.view_key.scalar, a.view_key.scalar + 32); axs.insert(axs.end(), a.address.x, a.address.x + 32); }
  std::vector<uint8_t> f1(k * n, 9), f2(k * n, 9), r1(32 * k * n, 9), r2(32 * k * n, 9);
  CHECK(aleo_mi355x_records_scan_many(f1.data(), r1.data(), c0.data(), nx.data(), n, vks.data(), axs.data(), k) == 0);
  CHECK(aleo_mi355x_records_scan_many_host(f2.data(), r2.data(), c0.data(), nx.data(), n, vks.data(), axs.data(), k) == 0);
  CHECK(f1 == f2 && r1 == r2);
  for (size_t a = 0; a < k; ++a) CHECK((f1[a * n + a] == 1) == expected[a]);
  std::memset(vks.data() + 32 * (k - 1), 0xff, 32);
  CHECK(aleo_mi355x_records_scan_many(f1.data(), nullptr, c0.data(), nx.data(), n, vks.data(), axs.data(), k) == ALEO_MI355X_ERR_BAD_ARG);
  CHECK(std::strstr(aleo_mi355x_last_error(), ("key " + std::to_string(k - 1)).c_str()) != nullptr);
  std::printf(fails ? "%d FAILED\n" : "ALL OK\n", fails);
  return fails ? 1 : 0;
}
