// found_commitments, unspent_named and unspent_named_many of include/aleo_mi355x.hpp through the C ABI:
//   records_commit_test <private key> <view key> <address> <program id> <record name> <commitment: 64 hex digits> <expected serial number: 64 hex digits> <record string>...
// The account is the private key's sk_sig with the given view key and address (the reference's serial-number test signs with a key that is not the owner's); it
// owns the strings at the even places, all of them the same record, whose commitment under (program id, record name) and serial number are given.  The calls that
// take no commitments must find both; with the serial number spent nothing is kept; the routed calls equal their host forms byte for byte; a bad program id or
// record name fails with the reference's text.  tests/test_records_commit.py runs it on the host path and on the kernels.
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
  if (argc < 10 || !hex32(argv[6], cm) || !hex32(argv[7], expected)) { std::printf("usage: records_commit_test private_key view_key address program_id record_name commitment serial_number record...\n"); return 2; }
  auto acct = account_from_private_key(argv[1]);
  auto vk = ViewKey::from_string(argv[2]); auto addr = Address::from_string(argv[3]);
  CHECK(acct.is_ok() && vk.is_ok() && addr.is_ok());
  if (!acct.is_ok() || !vk.is_ok() || !addr.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
  acct.value->view_key = *vk.value; acct.value->address = *addr.value;
  const std::string program_id = argv[4], record_name = argv[5];
  std::vector<std::string> strings(argv + 8, argv + argc);
  const size_t n = strings.size(), mine = (n + 1) / 2;
  RecordBatch batch(strings);
  // the commitments of a decrypt_strings result, routed and on the host
  auto found = decrypt_strings(batch, acct.value->view_key, acct.value->address);
  CHECK(found.is_ok() && found.value->size() == mine && found.value->commitments() == nullptr);
  if (found.is_ok()) {
    auto cms = found_commitments(batch, *found.value, program_id, record_name);
    CHECK(cms.is_ok() && cms.value->size() == mine);
    if (cms.is_ok()) for (size_t k = 0; k < cms.value->size(); ++k) CHECK(cms.value->flags[k] == 0 && !std::memcmp(cms.value->row(k), cm, 32));
    std::vector<uint8_t> rows(32 * mine), flags(mine, 9);
    CHECK(aleo_mi355x_records_commitments_found_host(rows.data(), flags.data(), found.value->handle(), batch.text(), batch.offsets(), n, program_id.c_str(), record_name.c_str()) == 0);
    if (cms.is_ok()) CHECK(rows == cms.value->rows && flags == cms.value->flags);
    CHECK(!found_commitments(batch, *found.value, "credits", record_name).is_ok() && std::string(aleo_mi355x_last_error()) == "Invalid ProgramID specified");
    CHECK(!found_commitments(batch, *found.value, program_id, "9lives").is_ok() && std::string(aleo_mi355x_last_error()) == "Invalid Identifier specified for record");
  }
  auto all = unspent_named(batch, program_id, record_name, *acct.value);
  CHECK(all.is_ok());
  if (all.is_ok()) {
    const FoundRecords& f = *all.value;
    CHECK(f.size() == mine && f.owned() == mine && f.serials() != nullptr && f.commitments() != nullptr && f.unparsed() == 0);
    for (size_t k = 0; k < f.size(); ++k) CHECK(f.index()[k] == 2 * k && !std::memcmp(f.serial(k), expected, 32) && !std::memcmp(f.commitment(k), cm, 32) && f.status()[k] == 0);
  }
  auto none = unspent_named(batch, program_id, record_name, *acct.value, expected, 1);
  CHECK(none.is_ok() && none.value->size() == 0 && none.value->owned() == mine && none.value->total_fields() == 0 && none.value->commitments() != nullptr);
  CHECK(!unspent_named(batch, "credits.eth", record_name, *acct.value).is_ok() && std::string(aleo_mi355x_last_error()) == "Invalid ProgramID specified");
  // two accounts: the same one under sk_sig and under another; only the first one's serial numbers are spent
  PrivateAccount other = *acct.value; other.sk_sig[0] ^= 1;
  std::vector<PrivateAccount> both{*acct.value, other};
  auto many = unspent_named_many(batch, program_id, record_name, both, expected, 1);
  CHECK(many.is_ok() && many.value->size() == 2);
  if (many.is_ok() && many.value->size() == 2) {
    const FoundRecords& a = (*many.value)[0]; const FoundRecords& b = (*many.value)[1];
    CHECK(a.size() == 0 && a.owned() == mine && b.size() == mine && b.owned() == mine);
    for (size_t k = 0; k < b.size(); ++k) CHECK(std::memcmp(b.serial(k), expected, 32) != 0 && !std::memcmp(b.commitment(k), cm, 32) && b.index()[k] == 2 * k);
    std::vector<uint8_t> sks, vks, axs;
    for (const auto& p : both) { sks.insert(sks.end(), p.sk_sig, p.sk_sig + 32); vks.insert(vks.end(), p.view_key.scalar, p.view_key.scalar + 32); axs.insert(axs.end(), p.address.x, p.address.x + 32); }
    aleo_mi355x_found* h[2] = {nullptr, nullptr};
    CHECK(aleo_mi355x_records_unspent_named_many_host(h, batch.text(), batch.offsets(), n, program_id.c_str(), record_name.c_str(), sks.data(), vks.data(), axs.data(), 2, expected, 1) == 0);
    if (h[1]) {
      const size_t c = aleo_mi355x_found_count(h[1]);
      CHECK(c == b.size() && aleo_mi355x_found_owned(h[1]) == b.owned() && aleo_mi355x_found_fields(h[1]) == b.total_fields());
      if (c == b.size() && c) CHECK(!std::memcmp(aleo_mi355x_found_serials(h[1]), b.serials(), 32 * c) && !std::memcmp(aleo_mi355x_found_commitments(h[1]), b.commitments(), 32 * c) &&
                                    !std::memcmp(aleo_mi355x_found_index(h[1]), b.index(), 4 * c) && !std::memcmp(aleo_mi355x_found_plain(h[1]), b.fields(0), 32 * b.total_fields()) &&
                                    !std::memcmp(aleo_mi355x_found_offsets(h[1]), b.offsets(), 4 * (c + 1)) && !std::memcmp(aleo_mi355x_found_microcredits(h[1]), b.microcredits(), 8 * c));
    }
    CHECK(h[0] && aleo_mi355x_found_count(h[0]) == 0);
    aleo_mi355x_found_free(h[0]); aleo_mi355x_found_free(h[1]);
  }
  auto nobody = unspent_named_many(batch, program_id, record_name, std::vector<PrivateAccount>{});
  CHECK(nobody.is_ok() && nobody.value->empty());
  CHECK(!unspent_named_many(batch, program_id, record_name, std::vector<PrivateAccount>(65, *acct.value)).is_ok());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
