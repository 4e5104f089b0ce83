// records_found_host.hpp — the result of decrypt_strings and its host path (records_found.hip): the existing host calls put together, per string the lane parse
// and the host scan of scan_strings_host, then for an owned record records_plaintext.hpp's structure as aleo_mi355x_record_fields reads it and the host
// decryption.  It shares no code with the device's walk (records_found_lane.h) except the reading of a u64 out of plain fields, which is what the device tests
// compare it with.  Plain C++ (no kernel, no HIP call): tests/cpp/records_found_fuzz.cpp builds it with the sanitizers.
#pragma once
#include "entry.h"
#include "records_host.hpp"
#include "records_strings_lane.h"
#include "records_found_lane.h"
#include "records_plaintext.hpp"
#include <string>
#include <vector>

struct aleo_mi355x_found {
  std::vector<uint32_t> index, offsets{0};
  std::vector<int8_t> kind;
  std::vector<uint8_t> rvk, plain, status;
  std::vector<uint64_t> microcredits;
  size_t unparsed = 0, first_unparsed = 0;
  // records_unspent_strings[_many] (records_unspent.hip): the result holds the records that are left of `owned`, and their serial numbers
  bool filtered = false; size_t owned = 0;
  std::vector<uint8_t> serials;
  // records_unspent_named[_many]: their commitments as well, which the call computed itself
  bool named = false;
  std::vector<uint8_t> commitments;
};

namespace aleo_mi355x {

using Found = ::aleo_mi355x_found;

static uint64_t microcredits_on_host(const plaintext::Record& r, const uint8_t* plain) {
  const plaintext::Entry* mc = nullptr;
  for (const plaintext::Entry& e : r.entries) if (e.name == "microcredits") mc = &e;      // the last of them, as a dict keeps it
  if (!mc) return 0;
  if (mc->visibility == 2)
    return found_microcredits_private((uint32_t)mc->n_fields, [&](uint32_t i, uint32_t (&w)[8]) { std::memcpy(w, plain + 32 * (mc->first_field + i), 32); });
  const uint8_t* b = r.payload.data() + mc->at;
  if (mc->len != 11 || b[0] != 0 || b[1] != 12 || b[2] != 0) return 0;
  uint64_t v; std::memcpy(&v, b + 3, 8);
  return v;
}

static int32_t found_on_host(Found& R, const char* text, const uint64_t* offsets, size_t n, const ScanArgs& key, const HFr& addr_mont) {
  const RecordsConsts& C = records_consts();
  const HFr a = HFr::from_mont(addr_mont);
  R.first_unparsed = n;
  std::vector<uint8_t> fields;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t span = offsets[i + 1] - offsets[i];
    const uint8_t* mine = (const uint8_t*)text + offsets[i];
    uint32_t ow[8], nw[8];
    const int32_t kind = records_parse_lane([&](uint32_t j) { return mine[j]; }, span > RS_MAX_CHARS ? RS_MAX_CHARS + 1 : (uint32_t)span, ow, nw);
    if (kind < 0) { if (!R.unparsed++) R.first_unparsed = i; continue; }
    uint8_t rvk[32];
    const uint8_t flag = scan_one_host(rvk, (const uint8_t*)ow, (const uint8_t*)nw, key, addr_mont, C);      // zeros into rvk where the nonce is malformed
    if (kind == 1 ? flag != 1 : std::memcmp(ow, a.l, 32) != 0) continue;
    if (R.index.size() >= UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 owned records");
    R.index.push_back((uint32_t)i); R.kind.push_back((int8_t)kind); R.rvk.insert(R.rvk.end(), rvk, rvk + 32);
    const std::string s((const char*)mine, (size_t)span);      // an accepted string holds no NUL
    plaintext::Record r;
    uint8_t status = FOUND_OK; uint64_t mc = 0;
    if (plaintext::parse(r, s.c_str(), "record_fields")) status = FOUND_REFUSED;
    else if (r.n_private) {
      if ((size_t)R.offsets.back() + r.n_private > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 private fields");
      const size_t at = R.plain.size();
      R.plain.resize(at + 32 * r.n_private, 0);
      if (kind == 0 && flag == 2) status = FOUND_MALFORMED;      // a public owner's nonce is not on the curve: no key to decrypt its entries with
      else {
        fields.resize(32 * r.n_private);
        plaintext::gather_fields(r, fields.data());
        status = decrypt_one_host(R.plain.data() + at, rvk, fields.data(), r.n_private);
      }
    }
    if (status == FOUND_OK) mc = microcredits_on_host(r, R.plain.data() + 32 * (size_t)R.offsets.back());
    R.offsets.push_back(R.offsets.back() + (uint32_t)(status == FOUND_REFUSED ? 0 : r.n_private));
    R.status.push_back(status); R.microcredits.push_back(mc);
  }
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
