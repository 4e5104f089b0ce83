// The record-ownership mirror of include/aleo_mi355x.hpp through the C ABI: groups of four arguments — record string, view key string, address string,
// expected 1 / 0 (tests/test_records.py passes the reference's own assertions) — checked one by one with is_owner and together with find_owned, against the
// host path (aleo_mi355x_records_scan_host) as well.  With ALEO_MI355X_MIN_RECORDS=0 every scan here runs the kernel.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 1) % 4) { std::printf("usage: records_scan_test (record view_key address expected)...\n"); return 2; }
  CHECK(!RecordCiphertext::from_string("garbage").is_ok());
  CHECK(!ViewKey::from_string("AViewKey1notbase58!").is_ok() && !Address::from_string("aleo1qqqq").is_ok());
  for (int a = 1; a + 3 < argc; a += 4) {
    auto rec = RecordCiphertext::from_string(argv[a]); auto vk = ViewKey::from_string(argv[a + 1]); auto addr = Address::from_string(argv[a + 2]);
    const bool expected = std::atoi(argv[a + 3]) != 0;
    CHECK(rec.is_ok() && vk.is_ok() && addr.is_ok());
    if (!rec.is_ok() || !vk.is_ok() || !addr.is_ok()) continue;
    CHECK(rec.value->to_string() == argv[a] && rec.value->owner_is_private());
    auto own = rec.value->is_owner(*vk.value, *addr.value);
    CHECK(own.is_ok() && *own.value == expected);
    // the batch form: this record three times over, between two copies of every other record given
    std::vector<RecordCiphertext> batch;
    for (int b = 1; b + 3 < argc; b += 4) { auto o = RecordCiphertext::from_string(argv[b]); if (o.is_ok()) batch.push_back(*o.value); }
    const size_t others = batch.size();
    for (int k = 0; k < 3; ++k) batch.push_back(*rec.value);
    auto found = find_owned(batch, *vk.value, *addr.value);
    CHECK(found.is_ok());
    if (!found.is_ok()) continue;
    size_t tail = 0;
    for (const auto& o : *found.value) if (o.index >= others) { ++tail; CHECK(o.has_view_key); }
    CHECK(tail == (expected ? 3u : 0u));
    // and the host path gives the same bytes
    uint8_t f1 = 9, f2 = 9, r1[32], r2[32];
    CHECK(aleo_mi355x_records_scan(&f1, r1, rec.value->owner_field(), rec.value->nonce_x(), 1, vk.value->scalar, addr.value->x) == 0);
    CHECK(aleo_mi355x_records_scan_host(&f2, r2, rec.value->owner_field(), rec.value->nonce_x(), 1, vk.value->scalar, addr.value->x) == 0);
    CHECK(f1 == f2 && f1 == (expected ? 1 : 0) && !std::memcmp(r1, r2, 32));
    if (expected && !found.value->empty()) CHECK(!std::memcmp(found.value->back().record_view_key_x, r2, 32));
  }
  std::printf(fails ? "%d FAILED\n" : "ALL OK\n", fails);
  return fails ? 1 : 0;
}
