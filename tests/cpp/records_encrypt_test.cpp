// encrypt_record and encrypt_records of include/aleo_mi355x.hpp through the C ABI:
//   records_encrypt_test <view key> <address> <plaintext string> <its record1… string> <a plaintext the device lane routes> <a string that is no record>
// The record decrypts to the plaintext; the plaintext encrypted under a randomizer (the nonce set) decrypts to the same plaintext but for its nonce.  Seventy rows —
// the plaintext, with the routed one at every seventh and the other string at every tenth place — under seventy randomizers: the routed call equals its host form
// byte for byte, every row but the non-records is encrypted, and decrypt_strings under the view key finds exactly the plaintext's rows with its microcredits.
// tests/test_records_encrypt.py runs it on the host path and on the kernels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aleo_mi355x.hpp"

using namespace aleo_mi355x;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static std::string without_nonce(const std::string& s) { const size_t at = s.find("_nonce"); return at == std::string::npos ? s : s.substr(0, at); }

int main(int argc, char** argv) {
  if (argc != 7) { std::printf("usage: records_encrypt_test view_key address plaintext record routed other\n"); return 2; }
  auto vk = ViewKey::from_string(argv[1]); auto addr = Address::from_string(argv[2]);
  CHECK(vk.is_ok() && addr.is_ok());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  const RecordPlaintext plain{std::string(argv[3])};
  auto rec = RecordCiphertext::from_string(argv[4]);
  CHECK(rec.is_ok() && rec.value->decrypt(*vk.value, *addr.value).is_ok() && rec.value->decrypt(*vk.value, *addr.value).value->to_string() == plain.to_string());
  uint8_t r[32] = {0x39, 0x05};
  CHECK(!encrypt_record(plain, r).is_ok());                      // upstream's encrypt: this randomizer's nonce is not the string's
  auto one = encrypt_record(plain, r, true);
  CHECK(one.is_ok());
  if (one.is_ok()) {
    auto back = one.value->decrypt(*vk.value, *addr.value);
    uint8_t nonce[32];
    CHECK(back.is_ok() && without_nonce(back.value->to_string()) == without_nonce(plain.to_string()) && back.value->microcredits() == plain.microcredits());
    CHECK(aleo_mi355x_record_nonce(nonce, r) == 0 && !std::memcmp(nonce, one.value->nonce_x(), 32));
    CHECK(back.is_ok() && encrypt_record(*back.value, r).is_ok() && encrypt_record(*back.value, r).value->to_string() == one.value->to_string());      // and now it is
  }
  std::vector<std::string> strings; std::vector<uint8_t> rs;
  for (int i = 0; i < 70; ++i) { strings.push_back(i % 10 == 9 ? argv[6] : i % 7 == 6 ? argv[5] : argv[3]); uint8_t k[32] = {(uint8_t)(i + 1), 7}; rs.insert(rs.end(), k, k + 32); }
  RecordBatch batch(strings);
  auto got = encrypt_records(batch, rs.data(), true), want = encrypt_records(batch, rs.data(), true, true);
  CHECK(got.is_ok() && want.is_ok());
  if (got.is_ok() && want.is_ok()) {
    CHECK(got.value->flags == want.value->flags && got.value->rvk == want.value->rvk && got.value->batch.size() == 70);
    size_t mine = 0;
    for (size_t i = 0; i < 70; ++i) {
      CHECK(got.value->batch.string(i) == want.value->batch.string(i));
      CHECK(got.value->flags[i] == (i % 10 == 9 ? 3 : 0) && got.value->batch.string(i).empty() == (i % 10 == 9));
      mine += strings[i] == argv[3];
    }
    auto found = decrypt_strings(got.value->batch, *vk.value, *addr.value);
    CHECK(found.is_ok());
    if (found.is_ok()) {
      size_t hits = 0;
      for (size_t k = 0; k < found.value->size(); ++k) {
        const size_t i = found.value->index()[k];
        if (strings[i] != argv[3]) continue;
        ++hits;
        CHECK(found.value->status()[k] == 0 && found.value->microcredits()[k] == plain.microcredits() && !std::memcmp(found.value->rvk(k), got.value->record_view_key_x(i), 32));
      }
      CHECK(hits == mine && found.value->unparsed() == 7);
    }
  }
  CHECK(!encrypt_records(batch, nullptr).is_ok() && encrypt_records(RecordBatch(std::vector<std::string>{}), nullptr).is_ok());
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
