// decrypt_strings and balance of include/aleo_mi355x.hpp through the C ABI:
//   records_found_test <view key> <address> <expected plaintext of every owned record> <expected microcredits of each> <record string>...   (the last string: one that does not parse)
// The owned records must be those decrypt_owned returns from RecordCiphertext objects, their plain fields must render to the expected plaintext, and the raw call
// must equal its host form byte for byte.  tests/test_records_found.py runs it on the host path and, with ALEO_MI355X_MIN_RECORDS=0, on the kernels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main(int argc, char** argv) {
  if (argc < 7) { std::printf("usage: records_found_test view_key address plaintext microcredits record... unparsable\n"); return 2; }
  auto vk = ViewKey::from_string(argv[1]); auto addr = Address::from_string(argv[2]);
  CHECK(vk.is_ok() && addr.is_ok());
  if (!vk.is_ok() || !addr.is_ok()) { std::printf("%d FAILED\n", fails); return 1; }
  const std::string plaintext = argv[3]; const uint64_t each = std::strtoull(argv[4], nullptr, 10);
  std::vector<std::string> strings(argv + 5, argv + argc - 1);
  std::vector<RecordCiphertext> objects;
  for (const auto& s : strings) { auto r = RecordCiphertext::from_string(s); CHECK(r.is_ok()); if (r.is_ok()) objects.push_back(*r.value); }
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  RecordBatch batch(strings);
  auto want = decrypt_owned(objects, *vk.value, *addr.value);
  auto found = decrypt_strings(batch, *vk.value, *addr.value);
  CHECK(want.is_ok() && found.is_ok());
  if (want.is_ok() && found.is_ok()) {
    const FoundRecords& f = *found.value;
    CHECK(f.size() == want.value->size() && f.size() > 0 && f.unparsed() == 0 && f.first_unparsed() == strings.size());
    for (size_t k = 0; k < f.size() && k < want.value->size(); ++k) {
      CHECK(f.index()[k] == (*want.value)[k].index && f.status()[k] == 0 && f.kind()[k] == 1 && f.microcredits()[k] == each);
      auto p = objects[f.index()[k]].plaintext(f.fields(k), f.n_fields(k), *addr.value);
      CHECK(p.is_ok() && p.value->to_string() == plaintext && p.value->to_string() == (*want.value)[k].plaintext.to_string() && p.value->microcredits() == each);
    }
    auto b = balance(batch, *vk.value, *addr.value);
    CHECK(b.is_ok());
    if (b.is_ok()) { CHECK(b.value->microcredits == (unsigned __int128)each * f.size() && b.value->indices.size() == f.size()); for (size_t k = 0; k < f.size(); ++k) CHECK(b.value->indices[k] == f.index()[k]); }
    FoundRecords moved = std::move(*found.value);
    CHECK(moved.size() == want.value->size());
  }
  // the routed call against its host form, byte for byte, with the string that does not parse in the middle
  std::vector<std::string> with_bad = strings; with_bad.insert(with_bad.begin() + 1, argv[argc - 1]);
  RecordBatch bad(with_bad);
  aleo_mi355x_found *a = nullptr, *h = nullptr;
  CHECK(aleo_mi355x_records_decrypt_strings(&a, bad.text(), bad.offsets(), bad.size(), vk.value->scalar, addr.value->x) == 0);
  CHECK(aleo_mi355x_records_decrypt_strings_host(&h, bad.text(), bad.offsets(), bad.size(), vk.value->scalar, addr.value->x) == 0);
  if (a && h) {
    const size_t c = aleo_mi355x_found_count(a), nf = aleo_mi355x_found_fields(a);
    CHECK(c == aleo_mi355x_found_count(h) && nf == aleo_mi355x_found_fields(h) && c > 0 && nf >= c);
    CHECK(aleo_mi355x_found_unparsed(a) == 1 && aleo_mi355x_found_unparsed(h) == 1 && aleo_mi355x_found_first_unparsed(a) == 1 && aleo_mi355x_found_first_unparsed(h) == 1);
    if (c == aleo_mi355x_found_count(h) && nf == aleo_mi355x_found_fields(h)) {
      CHECK(!std::memcmp(aleo_mi355x_found_index(a), aleo_mi355x_found_index(h), 4 * c) && !std::memcmp(aleo_mi355x_found_kind(a), aleo_mi355x_found_kind(h), c));
      CHECK(!std::memcmp(aleo_mi355x_found_rvk(a), aleo_mi355x_found_rvk(h), 32 * c) && !std::memcmp(aleo_mi355x_found_offsets(a), aleo_mi355x_found_offsets(h), 4 * (c + 1)));
      CHECK(!std::memcmp(aleo_mi355x_found_plain(a), aleo_mi355x_found_plain(h), 32 * nf) && !std::memcmp(aleo_mi355x_found_status(a), aleo_mi355x_found_status(h), c));
      CHECK(!std::memcmp(aleo_mi355x_found_microcredits(a), aleo_mi355x_found_microcredits(h), 8 * c));
    }
  }
  aleo_mi355x_found_free(a); aleo_mi355x_found_free(h);
  const int32_t rc = RecordCiphertext::from_string(argv[argc - 1]).error.code;
  CHECK(rc != 0 && !balance(bad, *vk.value, *addr.value).is_ok() && balance(bad, *vk.value, *addr.value).error.code == rc);
  auto none = decrypt_strings(RecordBatch(std::vector<std::string>{}), *vk.value, *addr.value);
  CHECK(none.is_ok() && none.value->size() == 0 && none.value->total_fields() == 0 && none.value->offsets()[0] == 0);
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
