// records_serial.hip — the serial numbers of the records an account has found: the last step of the reference's get_unspent_records before it can ask the chain
// whether a record is spent (rust/src/api/blocking.rs:277, `Record::<N, Ciphertext<N>>::serial_number(*private_key, commitment)`; RecordPlaintext's
// serialNumberString, wasm/src/record/record_plaintext.rs:64-82) — snarkVM 0.14.5 console/program/src/data/record/serial_number.rs [UPSTREAM-RECALL], pinned by the
// reference's own vectors stage by stage (serial_host.hpp, tests/serial_ref.py).
//
// The kernel (one commitment per lane: records_serial_lane.h; one kernel for this call's one key and for the key segments of records_unspent.hip, which launches
// it through launch_records_serial), the same bytes on the host (serial_host.hpp — what small batches take, and the checker), the
// routing threshold, and the host-only calls around them: a record's commitment and checksum (records_bits.hpp) and the account of a private key.
// The lane's tables (181 KB: serial_host.hpp serial_tables) are built on the host at first use and stay resident per device for the life of the process.
#include "records_found.h"
#include "records_bits.hpp"
#include <cstdlib>

namespace aleo_mi355x {

using serial::SerialTables;

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t SERIAL_BLOCK = 256;
static constexpr size_t SERIAL_CHUNK = (size_t)1 << 20;     // commitments per launch: 65 bytes of slot scratch each

// The one serial-number kernel, over the waves wave_lo .. wave_hi of the padded grid of `seg` (records_found.h): a wave finds its key among the n_keys + 1
// boundaries (kernel arguments; with one segment the search runs zero times), reads that key's digits from the table in device memory through uniform loads, and
// the ladder's digit tests stay uniform branches.  cm: the commitment rows in rank order; sn / flags: per rank.
__global__ void __launch_bounds__(SERIAL_BLOCK) k_records_serial(char* __restrict__ sn, uint8_t* __restrict__ flags, const char* __restrict__ cm, const uint32_t* __restrict__ K,
                                                                 const SerialArgs* __restrict__ keys, UnspentSegs seg, uint32_t wave_lo, uint32_t wave_hi) {
  const uint32_t w = __builtin_amdgcn_readfirstlane(wave_lo + blockIdx.x * (SERIAL_BLOCK / 64) + (threadIdx.x >> 6));
  if (w >= wave_hi) return;                                    // uniform; no barrier below
  uint32_t key = 0;
  for (uint32_t k = 1; k < seg.n_keys; ++k) if (seg.wave0[k] <= w) key = k;      // the last key that starts at or before this wave: keys without rows have no wave
  key = __builtin_amdgcn_readfirstlane(key);
  const uint32_t rank = seg.rank0[key] + (w - seg.wave0[key]) * 64u + (threadIdx.x & 63u);
  if (rank >= seg.rank0[key + 1]) return;                      // the padding of the key's last wave
  const Fr c = load_fp<Fr>(cm + (size_t)rank * 32);
  char* out = sn + (size_t)rank * 32;
  const uint32_t flag = records_serial_lane(c.v, K, keys[key], [&](const F29& v) { store_fp<Fr>(out, f29_to_fr(v)); });
  flags[rank] = (uint8_t)flag;
}

int32_t serial_tables_on_device(int device, const uint32_t** out) {
  return resident_table(device, ResidentTable::SERIAL, []() -> const std::vector<uint32_t>& { return serial::serial_tables().words; }, out);
}

int32_t launch_records_serial(hipStream_t s, char* dsn, uint8_t* dflags, const char* dcm, const uint32_t* dK, const SerialArgs* dkeys, const UnspentSegs& seg) {
  const size_t cap = env_cap("ALEO_MI355X_SERIAL_CHUNK", SERIAL_CHUNK);
  const uint32_t waves = seg.wave0[seg.n_keys], per = cap < 64 ? 1 : (uint32_t)(cap / 64);
  for (uint32_t lo = 0; lo < waves; lo += per) {
    const uint32_t hi = waves - lo < per ? waves : lo + per;
    hipLaunchKernelGGL(k_records_serial, dim3((hi - lo + SERIAL_BLOCK / 64 - 1) / (SERIAL_BLOCK / 64)), dim3(SERIAL_BLOCK), 0, s, dsn, dflags, dcm, dK, dkeys, seg, lo, hi);
    HIPCHK(hipGetLastError());
  }
  return ALEO_MI355X_OK;
}

// One key: a table of one row and, per chunk, one segment over the chunk.  The row is declared outside the slot: it outlives the copy that reads it.
static int32_t serials_on_device(void* sn_out, uint8_t* flags, const void* commitments32, size_t n, const ScanArgs& key) {
  const SerialArgs a = serial_args_of(key);
  const size_t cap = env_cap("ALEO_MI355X_SERIAL_CHUNK", SERIAL_CHUNK), chunk = n < cap ? n : cap;
  return on_slot([&](Ctx* c) -> int32_t {
    const uint32_t* dK; if (int32_t rc = serial_tables_on_device(c->device, &dK)) return rc;
    hipStream_t s = c->stream;
    Carve cv;
    const size_t o_key = cv.part(sizeof(SerialArgs)), o_cm = cv.part(chunk * 32), o_sn = cv.part(chunk * 32), o_fl = cv.part(chunk);
    if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
    char* base = c->scalars_stage.as<char>();
    char* dcm = base + o_cm; char* dsn = base + o_sn; uint8_t* dfl = (uint8_t*)(base + o_fl);
    HIPCHK(hipMemcpyAsync(base + o_key, &a, sizeof a, hipMemcpyHostToDevice, s));
    for (size_t at = 0; at < n; at += chunk) {
      const size_t m = n - at < chunk ? n - at : chunk;
      UnspentSegs seg{}; seg.n_keys = 1; seg.rank0[1] = (uint32_t)m; seg.wave0[1] = (uint32_t)((m + 63) / 64);
      HIPCHK(hipMemcpyAsync(dcm, (const char*)commitments32 + at * 32, m * 32, hipMemcpyHostToDevice, s));
      if (int32_t rc = launch_records_serial(s, dsn, dfl, dcm, dK, (const SerialArgs*)(base + o_key), seg)) return rc;
      HIPCHK(hipMemcpyAsync((char*)sn_out + at * 32, dsn, m * 32, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(flags + at, dfl, m, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));                         // the next chunk reuses the buffers
    }
    return ALEO_MI355X_OK;
  });
}

static int32_t serial_numbers(void* sn_out, uint8_t* flags, const void* commitments32, size_t n, const void* sk_sig32, bool may_route) {
  if (!sk_sig32 || ((!sn_out || !flags || !commitments32) && n)) return bad_arg("records_serial_numbers: null buffer");
  ScanArgs key; if (!serial::serial_key(key, sk_sig32)) return bad_arg("records_serial_numbers: sk_sig is not a canonical scalar below the subgroup order");
  if (may_route && n && n >= aleo_mi355x_min_serials()) return serials_on_device(sn_out, flags, commitments32, n, key);
  const SerialTables& T = serial::serial_tables();
  for (size_t i = 0; i < n; ++i) flags[i] = serial::serial_one_host((uint8_t*)sn_out + 32 * i, (const uint8_t*)commitments32 + 32 * i, key, T);
  return ALEO_MI355X_OK;
}

static int32_t record_hash(void* out32, const char* record1, const void* plain_fields, size_t n_fields, const char* program_id, const char* record_name, const char* who) {
  if (!out32 || !record1) return bad_arg("record_commitment: null buffer");
  std::vector<uint8_t> bits;
  if (program_id) {                                          // the commitment: (program id || record name || record)
    size_t dot;
    if (!serial::program_id_ok(program_id, &dot)) return bad_arg("Invalid ProgramID specified");
    if (!record_name || !serial::identifier_ok(record_name, std::strlen(record_name))) return bad_arg("Invalid Identifier specified for record");
    serial::push_bytes(bits, (const uint8_t*)program_id, dot); serial::push_bytes(bits, (const uint8_t*)program_id + dot + 1, std::strlen(program_id + dot + 1));
    serial::push_bytes(bits, (const uint8_t*)record_name, std::strlen(record_name));
  }
  plaintext::Record r;
  if (int32_t rc = plaintext::parse(r, record1, who)) return rc;
  if (program_id && n_fields != r.n_private) { g_last_error = std::string(who) + ": the record has " + std::to_string(r.n_private) + " private fields"; return ALEO_MI355X_ERR_BAD_ARG; }
  if (program_id && r.n_private && !plain_fields) return bad_arg("record_commitment: null buffer");
  if (int32_t rc = serial::record_bits(bits, r, program_id ? (const uint8_t*)plain_fields : nullptr, who)) return rc;
  serial::store_canonical(out32, serial::bhp1024().hash(bits));
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The batch size from which the serial numbers take the GPU: the measured crossover against the host path on one thread, which is what a call below it runs
// (profiles/records_serial.txt: the GPU call takes 3.7-4.5 ms for any batch up to 2^14; the host path 4.4 ms for 2^5 commitments and 8.8 ms for 2^6)
size_t aleo_mi355x_min_serials(void) { return env_size("ALEO_MI355X_MIN_SERIALS", (size_t)1 << 6); }

int32_t aleo_mi355x_records_serial_numbers_host(void* sn_out, uint8_t* flags, const void* commitments32, size_t n, const void* sk_sig32) {
  return guarded([&] { return serial_numbers(sn_out, flags, commitments32, n, sk_sig32, false); });
}

int32_t aleo_mi355x_records_serial_numbers(void* sn_out, uint8_t* flags, const void* commitments32, size_t n, const void* sk_sig32) {
  return guarded([&] { return serial_numbers(sn_out, flags, commitments32, n, sk_sig32, true); });
}

int32_t aleo_mi355x_found_serial_numbers(const aleo_mi355x_found* found, const void* commitments32, size_t n, const void* sk_sig32, void* sn_out, uint8_t* flags) {
  return guarded([&] {
    if (!found) return bad_arg("found_serial_numbers: null result");
    const size_t c = aleo_mi355x_found_count(found); const uint32_t* index = aleo_mi355x_found_index(found);
    if (c && !commitments32) return bad_arg("found_serial_numbers: null buffer");
    std::vector<uint8_t> rows(32 * c);
    for (size_t k = 0; k < c; ++k) {
      if (index[k] >= n) return bad_arg("found_serial_numbers: the result was made from more strings than there are commitments");
      std::memcpy(rows.data() + 32 * k, (const uint8_t*)commitments32 + 32 * (size_t)index[k], 32);
    }
    return aleo_mi355x_records_serial_numbers(sn_out, flags, rows.data(), c, sk_sig32);
  });
}

int32_t aleo_mi355x_record_commitment(void* out32, const char* record1, const void* plain_fields, size_t n_fields, const char* program_id, const char* record_name) {
  return guarded([&] {
    if (!program_id) return bad_arg("Invalid ProgramID specified");
    return record_hash(out32, record1, plain_fields, n_fields, program_id, record_name, "record_commitment");
  });
}

int32_t aleo_mi355x_record_checksum(void* out32, const char* record1) {
  return guarded([&] { return record_hash(out32, record1, nullptr, 0, nullptr, nullptr, "record_checksum"); });
}

int32_t aleo_mi355x_account_from_private_key(const char* private_key, void* sk_sig32, void* view_key32, void* address_x32) {
  return guarded([&] { return serial::account_from_private_key(private_key, sk_sig32, view_key32, address_x32); });
}

}  // extern "C"
