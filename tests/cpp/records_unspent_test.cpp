// unspent_strings and unspent_strings_many of include/aleo_mi355x.hpp through the C ABI:
//   records_unspent_test <private key> <view key> <address> <commitment: 64 hex digits> <expected serial number: 64 hex digits> <record string>...
// The account is the private key's sk_sig with the given view key and address (the reference's serial-number test signs with a key that is not the owner's); it
// owns the strings at the even places, all of them the same record with the given commitment.  With no spent set every one of
// them is kept with the expected serial number; with that serial number spent none is, and owned() still counts them; the routed call equals its host form
// byte for byte; a second account with another sk_sig gets other serial numbers.  tests/test_records_unspent.py runs it on the host path and on the kernels.
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
  uint8_t cm[32], expected[32];
  if (argc < 8 || !hex32(argv[4], cm) || !hex32(argv[5], expected)) { std::printf("usage: records_unspent_test private_key view_key address commitment serial_number record...\n"); return 2; }
  auto acct = account_from_private_key(argv[1]);
  auto vk = ViewKey::from_string(argv[2]); auto addr = Address::from_string(argv[3]);
  CHECK(acct.is_ok() && vk.is_ok() && addr.is_ok());
  if (!acct.is_ok() || !vk.is_ok() || !addr.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
  acct.value->view_key = *vk.value; acct.value->address = *addr.value;
  std::vector<std::string> strings(argv + 6, argv + argc);
  const size_t n = strings.size(), mine = (n + 1) / 2;
  RecordBatch batch(strings);
  std::vector<uint8_t> cms(32 * n);
  for (size_t i = 0; i < n; ++i) std::memcpy(cms.data() + 32 * i, cm, 32);
  auto all = unspent_strings(batch, cms.data(), *acct.value);
  CHECK(all.is_ok());
  if (all.is_ok()) {
    const FoundRecords& f = *all.value;
    CHECK(f.size() == mine && f.owned() == mine && f.serials() != nullptr && f.unparsed() == 0);
    for (size_t k = 0; k < f.size(); ++k) CHECK(f.index()[k] == 2 * k && !std::memcmp(f.serial(k), expected, 32) && f.status()[k] == 0 && f.microcredits()[k] == 1500000000000000ull);
  }
  auto none = unspent_strings(batch, cms.data(), *acct.value, expected, 1);
  CHECK(none.is_ok() && none.value->size() == 0 && none.value->owned() == mine && none.value->total_fields() == 0);
  // two accounts: the same one under sk_sig and under sk_sig + 1; only the first one's serial numbers are spent
  PrivateAccount other = *acct.value; other.sk_sig[0] ^= 1;
  std::vector<PrivateAccount> both{*acct.value, other};
  auto many = unspent_strings_many(batch, cms.data(), both, expected, 1);
  CHECK(many.is_ok() && many.value->size() == 2);
  if (many.is_ok() && many.value->size() == 2) {
    const FoundRecords& a = (*many.value)[0]; const FoundRecords& b = (*many.value)[1];
    CHECK(a.size() == 0 && a.owned() == mine && b.size() == mine && b.owned() == mine);
    for (size_t k = 0; k < b.size(); ++k) CHECK(std::memcmp(b.serial(k), expected, 32) != 0 && !std::memcmp(b.serial(k), b.serial(0), 32) && b.index()[k] == 2 * k);
    // the routed call against its host form
    std::vector<uint8_t> sks, vks, axs;
    for (const auto& p : both) { sks.insert(sks.end(), p.sk_sig, p.sk_sig + 32); vks.insert(vks.end(), p.view_key.scalar, p.view_key.scalar + 32); axs.insert(axs.end(), p.address.x, p.address.x + 32); }
    aleo_mi355x_found* h[2] = {nullptr, nullptr};
    CHECK(aleo_mi355x_records_unspent_strings_many_host(h, batch.text(), batch.offsets(), n, cms.data(), sks.data(), vks.data(), axs.data(), 2, expected, 1) == 0);
    if (h[1]) {
      const size_t c = aleo_mi355x_found_count(h[1]);
      CHECK(c == b.size() && aleo_mi355x_found_owned(h[1]) == b.owned() && aleo_mi355x_found_fields(h[1]) == b.total_fields());
      if (c == b.size() && c) CHECK(!std::memcmp(aleo_mi355x_found_serials(h[1]), b.serials(), 32 * c) && !std::memcmp(aleo_mi355x_found_index(h[1]), b.index(), 4 * c) &&
                                    !std::memcmp(aleo_mi355x_found_plain(h[1]), b.fields(0), 32 * b.total_fields()) && !std::memcmp(aleo_mi355x_found_offsets(h[1]), b.offsets(), 4 * (c + 1)) &&
                                    !std::memcmp(aleo_mi355x_found_rvk(h[1]), b.rvk(0), 32 * c) && !std::memcmp(aleo_mi355x_found_microcredits(h[1]), b.microcredits(), 8 * c));
    }
    CHECK(h[0] && aleo_mi355x_found_count(h[0]) == 0);
    aleo_mi355x_found_free(h[0]); aleo_mi355x_found_free(h[1]);
  }
  // a result of decrypt_strings has no serial numbers and owns what it holds
  auto plain = decrypt_strings(batch, acct.value->view_key, acct.value->address);
  CHECK(plain.is_ok() && plain.value->serials() == nullptr && plain.value->owned() == plain.value->size() && plain.value->size() == mine);
  // a string that does not parse fails the call as balance fails; nobody to search for; too many
  std::vector<std::string> with_bad = strings; with_bad.insert(with_bad.begin() + 1, "garbage");
  RecordBatch bad(with_bad);
  std::vector<uint8_t> cms_bad(32 * (n + 1), 1);
  const int32_t rc = RecordCiphertext::from_string("garbage").error.code;
  CHECK(rc != 0 && !unspent_strings(bad, cms_bad.data(), *acct.value).is_ok() && unspent_strings(bad, cms_bad.data(), *acct.value).error.code == rc);
  CHECK(!unspent_strings_many(bad, cms_bad.data(), both).is_ok());
  auto nobody = unspent_strings_many(batch, cms.data(), std::vector<PrivateAccount>{});
  CHECK(nobody.is_ok() && nobody.value->empty());
  CHECK(!unspent_strings_many(batch, cms.data(), std::vector<PrivateAccount>(65, *acct.value)).is_ok());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
