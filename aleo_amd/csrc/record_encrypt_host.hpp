// record_encrypt_host.hpp — a record PLAINTEXT as the "record1…" ciphertext a transition publishes: Record<N, Plaintext<N>>::encrypt(randomizer) and
// encrypt_symmetric_unchecked(record_view_key) of snarkVM 0.14.5, console/program/src/data/record/encrypt.rs [UPSTREAM-RECALL] — what every execute, transfer,
// split and join of the reference runs for each output record (rust/src/program/execute.rs:74,177, transfer.rs:99-106).  Plain C++ (no HIP, touches no device) over
// plaintext_parse.hpp's parse tree (there is no second parser), signature_host.hpp's table of G and point from x, and poseidon.hpp.  encrypt_one_host is the
// DEFINITION of a row; the device lanes (records_encrypt_lane.h) return the same bytes.
//
//   nonce     x(r G), G the account generator; r the randomizer, a scalar below the subgroup order l (r = 0 is computed by the formula: nonce 0, rvk 0)
//   rvk       x(r Owner), Owner the point of the prime-order subgroup with the owner's x  (= x(view key . nonce point): what the scan and the decryption compute)
//   fields    in randomizer order: the owner's x if the owner is private; then for every private entry its PLAINTEXT BITS (plaintext_parse.hpp value_bits), a
//             terminus 1, zeros up to a multiple of 252, 252 bits to a field
//   c_i       plain_i + hash_many_psd8([domain "AleoSymmetricEncryption0", rvk], m)_i  mod r
//   bytes     the inverse of records_plaintext.hpp's reader: owner `00 | x` or `01 | u16 1 | c_0`; u8 entry count; per entry u8 name length | name | u16 body length
//             | body, the body `02 | u16 fields | fields` (private) or `00` / `01` and the PLAINTEXT BYTES (constant, public); the nonce's 32 bytes; bech32m under "record"
// Pinned: the symmetric half — the reference's own plaintext under x(view key . nonce) gives the reference's record1… string character for character
// (tests/golden/reference_records.json).  UNPINNED, [UPSTREAM-RECALL]: the byte layout of constant and public entries (as records_plaintext.hpp reads them);
// everything about the randomizer that the randomizer-free known answer cannot reach — nonce = x(r G), rvk = x(r Owner), which rest on r A = view key . (r G) and
// are tested by the round trip through the scan and the decryption — and that upstream refuses what is refused here.
// Refused (flag 3): a record that does not fit the layout's counters — an entry's body over 65535 bytes (a private entry of more than 2047 fields).
#pragma once
#include "plaintext_parse.hpp"
#include "signature_host.hpp"

namespace aleo_mi355x { namespace renc {

using host::HFr;

static constexpr uint8_t ENC_OK = 0, ENC_NONCE_MISMATCH = 1, ENC_BAD_KEY = 2, ENC_NOT_A_RECORD = 3;

static inline void put_u16(std::vector<uint8_t>& b, size_t v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }

// PLAINTEXT BYTES of a value (records_plaintext.hpp render_bytes is the reader); false: a member's bytes pass what its u16 length holds
static bool value_bytes(std::vector<uint8_t>& out, const ptext::Value& v) {
  if (!v.is_struct) {
    out.push_back(0); put_u16(out, v.type);
    if (v.type == 15) { put_u16(out, v.text.size()); out.insert(out.end(), v.text.begin(), v.text.end()); return true; }
    const size_t n = ((size_t)plaintext::literal_bits(v.type) + 7) / 8;
    const uint8_t* p = (const uint8_t*)v.v;
    out.insert(out.end(), p, p + n);
    return true;
  }
  out.push_back(1); out.push_back((uint8_t)v.members.size());
  for (const auto& m : v.members) {
    std::vector<uint8_t> inner;
    if (!value_bytes(inner, m.second) || inner.size() > 65535) return false;
    out.push_back((uint8_t)m.first.size()); out.insert(out.end(), m.first.begin(), m.first.end());
    put_u16(out, inner.size()); out.insert(out.end(), inner.begin(), inner.end());
  }
  return true;
}

// A record laid out with its private fields still plain: the payload, and where each of the m fields in randomizer order lies in it
struct Layout { std::vector<uint8_t> payload; std::vector<size_t> field_at; size_t nonce_at = 0; };

static bool layout(Layout& L, const ptext::Parsed& r, std::string& why) {
  std::vector<uint8_t>& b = L.payload;
  b.clear(); L.field_at.clear();
  if (r.owner_kind == 1) { b.push_back(1); put_u16(b, 1); L.field_at.push_back(b.size()); } else b.push_back(0);
  b.insert(b.end(), r.owner, r.owner + 32);
  b.push_back((uint8_t)r.entries.size());                    // parse admits at most 255
  for (const ptext::Entry& e : r.entries) {
    b.push_back((uint8_t)e.name.size()); b.insert(b.end(), e.name.begin(), e.name.end());
    std::vector<uint8_t> body;
    size_t fields = 0;
    if (e.visibility == 2) {
      std::vector<uint8_t> bits;
      if (!ptext::value_bits(bits, e.value)) { why = "entry '" + e.name + "': a member is longer than 65535 bits"; return false; }
      bits.push_back(1);                                       // the terminus
      fields = (bits.size() + plaintext::DATA_BITS - 1) / plaintext::DATA_BITS;
      bits.resize(fields * plaintext::DATA_BITS, 0);
      body.push_back(2); put_u16(body, fields);
      body.resize(3 + 32 * fields, 0);
      for (size_t i = 0; i < bits.size(); ++i) if (bits[i]) { const size_t f = i / plaintext::DATA_BITS, k = i % plaintext::DATA_BITS; body[3 + 32 * f + (k >> 3)] |= (uint8_t)(1u << (k & 7)); }
    } else {
      body.push_back(e.visibility);
      if (!value_bytes(body, e.value)) { why = "entry '" + e.name + "': a member is longer than 65535 bytes"; return false; }
    }
    if (body.size() > 65535) { why = "entry '" + e.name + "' is longer than 65535 bytes"; return false; }
    put_u16(b, body.size());
    for (size_t f = 0; f < fields; ++f) L.field_at.push_back(b.size() + 3 + 32 * f);
    b.insert(b.end(), body.begin(), body.end());
  }
  L.nonce_at = b.size();
  b.insert(b.end(), r.nonce, r.nonce + 32);
  return true;
}

// c_i = plain_i + randomizer_i in place, under the canonical record view key x (below r: the caller's to see to)
static void encrypt_fields(Layout& L, const uint8_t* rvk32) {
  const size_t m = L.field_at.size();
  if (!m) return;
  static const HFr dom = host::fr_domain_separator("AleoSymmetricEncryption0");
  HFr rv; std::memcpy(rv.l, rvk32, 32);
  const HFr in[2] = {dom, HFr::to_mont(rv)};
  std::vector<HFr> rnd(m);
  host::poseidon_hash_many_fr<8>(in, 2, rnd.data(), m);
  for (size_t j = 0; j < m; ++j) {
    HFr p; std::memcpy(p.l, L.payload.data() + L.field_at[j], 32);      // below 2^252 or an x below r
    const HFr c = HFr::from_mont(HFr::add(HFr::to_mont(p), rnd[j]));
    std::memcpy(L.payload.data() + L.field_at[j], c.l, 32);
  }
}

static std::string record_string(const Layout& L) {
  std::string s(7 + (8 * L.payload.size() + 4) / 5 + 6 + 1, 0);
  (void)aleo_mi355x_bech32m_encode(&s[0], s.size(), "record", L.payload.data(), L.payload.size());
  s.resize(s.size() - 1);
  return s;
}

// x(r G) as canonical bytes; r below 2^252
static void nonce_of(uint8_t* out32, const uint64_t* r4) { sig::x_of_mul_g(out32, r4); }

// One string under a randomizer.  mode 0: the string's nonce must be x(r G); 1: it is replaced by it.  The flag, the string (empty with a flag) and the record view
// key's canonical x (zeros with a flag).
static uint8_t encrypt_one_host(std::string& out, uint8_t* rvk32, const char* s, size_t chars, const uint8_t* randomizer32, int mode) {
  out.clear(); std::memset(rvk32, 0, 32);
  ptext::Parsed r; std::string why; Layout L;
  if (!ptext::parse(r, s, chars, why) || !layout(L, r, why)) return ENC_NOT_A_RECORD;
  uint64_t k[4]; std::memcpy(k, randomizer32, 32);
  HFr ox; std::memcpy(ox.l, r.owner, 32);
  EdH owner;
  if (sig::geq_l(k) || !sig::point_from_x(owner, ox)) return ENC_BAD_KEY;
  uint8_t nonce[32]; nonce_of(nonce, k);
  if (mode == 0 && std::memcmp(nonce, r.nonce, 32)) return ENC_NONCE_MISMATCH;
  std::memcpy(L.payload.data() + L.nonce_at, nonce, 32);
  const HFr rv = HFr::from_mont(serial::edh_affine(sig::edh_mul_words(owner, k)).x);
  std::memcpy(rvk32, rv.l, 32);
  encrypt_fields(L, rvk32);
  out = record_string(L);
  return ENC_OK;
}

// One string under a record view key given as it is: no randomizer, no owner point, the nonce kept.  The flag (0, 2: rvk is not below r, 3).
static uint8_t encrypt_symmetric_host(std::string& out, const char* s, size_t chars, const uint8_t* rvk32) {
  out.clear();
  ptext::Parsed r; std::string why; Layout L;
  if (!ptext::parse(r, s, chars, why) || !layout(L, r, why)) return ENC_NOT_A_RECORD;
  uint64_t v[4]; std::memcpy(v, rvk32, 32);
  if (HFr::geq_p(v)) return ENC_BAD_KEY;
  encrypt_fields(L, rvk32);
  out = record_string(L);
  return ENC_OK;
}

}}  // namespace aleo_mi355x::renc
