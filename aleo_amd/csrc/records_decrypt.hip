// records_decrypt.hip — decrypting the records an account owns, in batches, down to their plaintext strings: the second half of the record search.
//
// Replaces, for batches, what the reference runs record by record right after the ownership test: `record.decrypt(&view_key)` at rust/src/api/blocking.rs:279
// (get_unspent_records, which then sums `microcredits()`) and RecordCiphertext.decrypt(viewKey) -> RecordPlaintext (wasm/src/record/record_ciphertext.rs:48-57) —
// snarkVM 0.14.5 console/program/src/data/record/decrypt.rs, ciphertext/decrypt.rs [UPSTREAM-RECALL; pinned by tests/golden/reference_records.json]:
//   the private fields of a record in randomizer order: the owner's one field if the owner is private, then the fields of every private entry, m in all;
//   randomizers = hash_many_psd8([domain "AleoSymmetricEncryption0", rvk], m);  plain_i = c_i - randomizers_i;  rvk = x(view_key * nonce), which the scan returns.
//
// The field arithmetic has three entry points, as the scan has: the kernel (one record per lane: records_decrypt_lane.h), the same bytes on the host
// (poseidon.hpp — the fallback, what small batches take, and the checker), and the routing threshold between them.  The rest is host work by nature (a few
// hundred bytes of parsing and formatting per record: records_plaintext.hpp): the private fields of a record string, the plaintext string from the decrypted
// fields, and the one-record decrypt on the host.
#include "entry.h"
#include "records_host.hpp"
#include "records_decrypt_lane.h"
#include "records_plaintext.hpp"
#include "records_strings.h"
#include <cstdlib>
#include <string>
#include <vector>

namespace aleo_mi355x {

static constexpr uint32_t DECRYPT_BLOCK = 256;
static constexpr size_t DECRYPT_CHUNK_RECORDS = (size_t)1 << 20;      // per launch, with records_strings.h DECRYPT_CHUNK_FIELDS: 37 B a record and 32 B a field of slot scratch (~170 MB)
static constexpr size_t DECRYPT_MAX_FIELDS = 65535;        // of one record: upstream's u16 field count

// what both paths refuse before they compute; *perms: the permutations of the call, sum of ceil(m / 8)
static int32_t decrypt_args_ok(const void* plain_out, const uint8_t* flags, const void* rvk, const uint32_t* offsets, const void* fields, size_t n, size_t* perms) {
  *perms = 0;
  if (!n) return ALEO_MI355X_OK;
  if (!flags || !rvk || !offsets) return bad_arg("records_decrypt_fields: null buffer");
  if (offsets[0] != 0) return bad_arg("records_decrypt_fields: offsets[0] is not 0");
  for (size_t i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i]) return bad_arg("records_decrypt_fields: offsets decrease");
    const size_t m = offsets[i + 1] - offsets[i];
    if (m > DECRYPT_MAX_FIELDS) return bad_arg("records_decrypt_fields: a record has more than 65535 fields");
    *perms += (m + 7) / 8;
  }
  if (offsets[n] && (!plain_out || !fields)) return bad_arg("records_decrypt_fields: null buffer");
  return ALEO_MI355X_OK;
}

static int32_t decrypt_on_host(uint8_t* plain, uint8_t* flags, const uint8_t* rvk, const uint32_t* offsets, const uint8_t* fields, size_t n) {
  for (size_t i = 0; i < n; ++i) flags[i] = decrypt_one_host(plain + (size_t)offsets[i] * 32, rvk + 32 * i, fields + (size_t)offsets[i] * 32, offsets[i + 1] - offsets[i]);
  return ALEO_MI355X_OK;
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------
// io: the chunk's fields, ciphertext in and plaintext out in place (a lane reads every field of its record before it writes one, and writes row j after its last
// read of it); offsets: the caller's own entries for the chunk's n + 1 boundaries, `base` the first of them.
__global__ void __launch_bounds__(DECRYPT_BLOCK) k_records_decrypt(char* __restrict__ io, uint8_t* __restrict__ flags, const char* __restrict__ rvk, const uint32_t* __restrict__ offsets,
                                                                   uint32_t base, uint32_t n, const uint32_t* __restrict__ K) {
  const uint32_t i = blockIdx.x * DECRYPT_BLOCK + threadIdx.x;
  if (i >= n) return;                                        // no barrier below
  const uint32_t first = offsets[i], m = offsets[i + 1] - first;
  char* mine = io + (size_t)(first - base) * 32;
  const Fr rv = load_fp<Fr>(rvk + (size_t)i * 32);
  const uint32_t flag = records_decrypt_lane(rv.v, m, K,
    [&](uint32_t j, uint32_t (&w)[8]) { const Fr f = load_fp<Fr>(mine + (size_t)j * 32);
#pragma unroll
      for (int q = 0; q < 8; ++q) w[q] = f.v[q]; },
    [&](uint32_t j, const F29& v) { store_fp<Fr>(mine + (size_t)j * 32, f29_to_fr(v)); });
  flags[i] = (uint8_t)flag;
}

// the cut of records into launches, and the launch itself: for decrypt_on_device and for records_found.hip, whose records are on the device
size_t decrypt_cut(const uint32_t* offsets, size_t at, size_t n, size_t record_cap, size_t field_cap) {
  size_t e = at + 1; while (e < n && e - at < record_cap && (size_t)offsets[e + 1] - offsets[at] <= field_cap) ++e; return e;
}
void launch_records_decrypt(hipStream_t s, char* io, uint8_t* dflags, const char* drvk, const uint32_t* doffsets, uint32_t base, size_t n, const uint32_t* dK) {
  hipLaunchKernelGGL(k_records_decrypt, dim3((uint32_t)((n + DECRYPT_BLOCK - 1) / DECRYPT_BLOCK)), dim3(DECRYPT_BLOCK), 0, s, io, dflags, drvk, doffsets, base, (uint32_t)n, dK);
}

// Copies, launch and synchronisation per chunk as scan_many_on_device (records_many.hip).  A chunk: as many whole records as stay within DECRYPT_CHUNK_RECORDS and the field
// cap, and one at least.  ALEO_MI355X_DECRYPT_CHUNK_FIELDS (read per call) lowers the field cap; the bytes do not depend on it.
static int32_t decrypt_on_device(uint8_t* plain, uint8_t* flags, const uint8_t* rvk, const uint32_t* offsets, const uint8_t* fields, size_t n) {
  const size_t cap = env_cap("ALEO_MI355X_DECRYPT_CHUNK_FIELDS", DECRYPT_CHUNK_FIELDS);
  std::vector<size_t> cut{0};                                 // chunk k: records cut[k] .. cut[k + 1]
  size_t max_records = 0, max_fields = 0;
  for (size_t at = 0; at < n;) {
    const size_t e = decrypt_cut(offsets, at, n, DECRYPT_CHUNK_RECORDS, cap);
    if (e - at > max_records) max_records = e - at;
    if ((size_t)offsets[e] - offsets[at] > max_fields) max_fields = offsets[e] - offsets[at];
    cut.push_back(e); at = e;
  }
  return on_slot([&](Ctx* c) -> int32_t {
    hipStream_t s = c->stream;
    int32_t rc;
    const uint32_t* dK; if ((rc = records_constants(c, &dK))) return rc;
    Carve cv;
    const size_t o_io = cv.part(max_fields * 32), o_rvk = cv.part(max_records * 32), o_off = cv.part((max_records + 1) * 4), o_fl = cv.part(max_records);
    if ((rc = c->scalars_stage.reserve(cv.total))) return rc;
    char* base = c->scalars_stage.as<char>();
    char* dio = base + o_io; char* drvk = base + o_rvk; uint32_t* doff = (uint32_t*)(base + o_off); uint8_t* dfl = (uint8_t*)(base + o_fl);
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
      const size_t at = cut[k], m = cut[k + 1] - at, first = offsets[at], nf = offsets[at + m] - first;
      if (nf) HIPCHK(hipMemcpyAsync(dio, fields + first * 32, nf * 32, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(drvk, rvk + at * 32, m * 32, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(doff, offsets + at, (m + 1) * 4, hipMemcpyHostToDevice, s));
      launch_records_decrypt(s, dio, dfl, drvk, doff, (uint32_t)first, m, dK);
      HIPCHK(hipGetLastError());
      if (nf) HIPCHK(hipMemcpyAsync(plain + first * 32, dio, nf * 32, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(flags + at, dfl, m, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));                         // the next chunk reuses the buffers
    }
    return ALEO_MI355X_OK;
  });
}

// ---- one record, entirely on the host ---------------------------------------------------------------------------------------------------------------------
static int32_t record_decrypt_on_host(const char* record1, const void* view_key32, const void* address_x32, char* out, size_t* out_len) {
  if (!record1 || !address_x32 || !out_len) return bad_arg("record_decrypt: null argument");
  plaintext::Record r; if (int32_t rc = plaintext::parse(r, record1, "record_decrypt")) return rc;
  const uint8_t* owner = r.payload.data() + r.owner_at;
  if (r.owner_kind == 0 && std::memcmp(owner, address_x32, 32)) { g_last_error = "record_decrypt: the record's owner is not the given address"; return ALEO_MI355X_ERR_NOT_OWNER; }
  std::vector<uint8_t> fields(32 * r.n_private), plain(32 * r.n_private);
  if (r.n_private) {                                           // a record with no private field needs neither the key nor a hash
    if (!view_key32) return bad_arg("record_decrypt: null argument");
    ScanArgs a; HFr addr; if (const char* why = scan_args(a, addr, view_key32, address_x32)) return bad_arg(why);
    uint8_t rvk[32];
    const uint8_t flag = scan_one_host(rvk, owner, r.payload.data() + r.nonce_at, a, addr, records_consts());
    if (flag == 2) return bad_arg("record_decrypt: the nonce is not the x of a point on the curve");
    if (r.owner_kind == 1 && flag != 1) { g_last_error = "record_decrypt: the view key does not decrypt the owner to the given address"; return ALEO_MI355X_ERR_NOT_OWNER; }
    plaintext::gather_fields(r, fields.data());
    if (decrypt_one_host(plain.data(), rvk, fields.data(), r.n_private)) return bad_arg("record_decrypt: a field is not canonical");
  }
  std::string s; if (int32_t rc = plaintext::render(s, r, plain.data(), (const uint8_t*)address_x32, "record_decrypt")) return rc;
  return put_string(s, out, out_len, "record_decrypt");
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The number of permutations from which records_decrypt_fields takes the GPU: the measured crossover against the host path on one thread (profiles/records_decrypt.txt:
// records of two fields, 0.99x at 2^5, 2.68x at 2^6), which is the scan's as well — a small call of either is one wave running one dependent chain.
size_t aleo_mi355x_min_decrypt(void) { return env_size("ALEO_MI355X_MIN_DECRYPT", (size_t)1 << 6); }

int32_t aleo_mi355x_records_decrypt_fields_host(void* plain_out, uint8_t* flags, const void* rvk, const uint32_t* offsets, const void* fields, size_t n) {
  return guarded([&] {
    size_t perms; if (int32_t rc = decrypt_args_ok(plain_out, flags, rvk, offsets, fields, n, &perms)) return rc;
    return decrypt_on_host((uint8_t*)plain_out, flags, (const uint8_t*)rvk, offsets, (const uint8_t*)fields, n);
  });
}

int32_t aleo_mi355x_records_decrypt_fields(void* plain_out, uint8_t* flags, const void* rvk, const uint32_t* offsets, const void* fields, size_t n) {
  return guarded([&] {
    size_t perms; if (int32_t rc = decrypt_args_ok(plain_out, flags, rvk, offsets, fields, n, &perms)) return rc;
    if (perms < aleo_mi355x_min_decrypt() || n == 0) return decrypt_on_host((uint8_t*)plain_out, flags, (const uint8_t*)rvk, offsets, (const uint8_t*)fields, n);
    return decrypt_on_device((uint8_t*)plain_out, flags, (const uint8_t*)rvk, offsets, (const uint8_t*)fields, n);
  });
}

int32_t aleo_mi355x_record_fields(const char* record1, void* fields_out, size_t cap, size_t* n_fields_out) {
  return guarded([&] {
    if (!record1 || !n_fields_out) return bad_arg("record_fields: null argument");
    plaintext::Record r; if (int32_t rc = plaintext::parse(r, record1, "record_fields")) return rc;
    *n_fields_out = r.n_private;
    if (!fields_out) return (int32_t)ALEO_MI355X_OK;
    if (cap < r.n_private) return bad_arg("record_fields: the output buffer is too short (n_fields_out holds the count)");
    plaintext::gather_fields(r, (uint8_t*)fields_out);
    return (int32_t)ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_record_plaintext(const char* record1, const void* plain_fields, size_t n_fields, const void* address_x32, char* out, size_t* out_len) {
  return guarded([&] {
    if (!record1 || !out_len || (!plain_fields && n_fields)) return bad_arg("record_plaintext: null argument");
    plaintext::Record r; if (int32_t rc = plaintext::parse(r, record1, "record_plaintext")) return rc;
    if (n_fields != r.n_private) return bad_arg("record_plaintext: n_fields is not the record's number of private fields");
    std::string s; if (int32_t rc = plaintext::render(s, r, (const uint8_t*)plain_fields, (const uint8_t*)address_x32, "record_plaintext")) return rc;
    return put_string(s, out, out_len, "record_plaintext");
  });
}

int32_t aleo_mi355x_record_decrypt(const char* record1, const void* view_key32, const void* address_x32, char* out, size_t* out_len) {
  return guarded([&] { return record_decrypt_on_host(record1, view_key32, address_x32, out, out_len); });
}

}  // extern "C"
