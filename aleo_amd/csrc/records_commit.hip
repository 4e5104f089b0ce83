// records_commit.hip — the commitments of the records an account has found, from their strings and their decrypted fields alone: what the wasm SDK's
// findUnspentRecords derives per owned record before it can ask for a serial number (sdk/src/aleo_network_client.ts:365-373, `serialNumberString(privateKey,
// "credits.aleo", "credits")`; wasm/src/record/record_plaintext.rs:64-82: to_commitment(program_id, record_name), then serial_number) — a caller that has no
// (commitment, record) pairs, as the Rust client's block.into_records() hands out, had to bring every owned record down and call the host-only
// aleo_mi355x_record_commitment once per record.
//
// The kernel (one owned record per lane: records_commit_lane.h), its table (commit_host.hpp: 217 KB with the scan's constants, built on the host at first use and
// resident per device for the life of the process), the same bytes on the host (records_bits.hpp's record_bits and serial_host.hpp's BHP1024, as
// aleo_mi355x_record_commitment runs them — what small batches take, what a record with a constant or public entry takes, and the checker), the routing
// threshold, the stand-alone call over an existing result, and the rows of a chunk inside the flow of records_unspent_named[_many] (records_unspent.hip).
#include "records_found.h"
#include "records_bits.hpp"
#include "commit_host.hpp"
#include <cstdlib>

namespace aleo_mi355x {

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t COMMIT_BLOCK = 256;
static constexpr size_t COMMIT_CHUNK = (size_t)1 << 20;     // records per launch

// The records lo .. hi of a chunk's compacted arrays (records_found.h FoundChunk), one per lane.  index null: record j's string is string j.  A record whose status
// is not 0 gets its status as its flag; a row that is not computed is zeros.  route: counts the records the lane routes to the host (flag COMMIT_ROUTED).
__global__ void __launch_bounds__(COMMIT_BLOCK) k_records_commit(char* __restrict__ cm, uint8_t* __restrict__ flags, uint32_t* __restrict__ route, const char* __restrict__ fields,
                                                                 const uint32_t* __restrict__ off, const uint32_t* __restrict__ index, const int8_t* __restrict__ kind,
                                                                 const uint8_t* __restrict__ status, const char* __restrict__ text, const uint32_t* __restrict__ soff,
                                                                 const uint32_t* __restrict__ K, CommitArgs A, uint32_t lo, uint32_t hi) {
  const uint32_t j = lo + blockIdx.x * COMMIT_BLOCK + threadIdx.x;
  if (j >= hi) return;                                         // no barrier below
  uint4* out = (uint4*)(cm + (size_t)j * 32);
  uint32_t flag = status[j];
  if (flag == FOUND_OK) {
    const uint32_t i = index ? index[j] : j, first = soff[i], len = soff[i + 1] - first, f0 = off[j];
    const uint8_t* __restrict__ mine = (const uint8_t*)text + first;
    const char* __restrict__ my_fields = fields + (size_t)f0 * 32;
    flag = records_commit_lane([&](uint32_t q) { return mine[q]; }, len, kind[j], off[j + 1] - f0,
                               [&](uint32_t k, uint32_t (&w)[8]) { load_words8(w, my_fields + (size_t)k * 32); },
                               K, A, [&](const F29& v) { store_fp<Fr>(out, f29_to_fr(v)); });
    if (flag == COMMIT_ROUTED) atomicAdd(route, 1u);
  }
  if (flag) { out[0] = make_uint4(0, 0, 0, 0); out[1] = make_uint4(0, 0, 0, 0); }
  flags[j] = (uint8_t)flag;
}

int32_t commit_tables_on_device(int device, const uint32_t** out) {
  return resident_table(device, ResidentTable::COMMIT, []() -> const std::vector<uint32_t>& { return serial::commit_tables().words; }, out);
}

// k_records_commit over n records in launches of at most ALEO_MI355X_COMMIT_CHUNK lanes (read per call); *droute is zeroed first
static int32_t launch_records_commit(hipStream_t s, char* dcm, uint8_t* dflags, uint32_t* droute, const char* fields, const uint32_t* off, const uint32_t* index, const int8_t* kind,
                                     const uint8_t* status, const char* text, const uint32_t* soff, const uint32_t* dK, const CommitArgs& A, size_t n) {
  const size_t cap = env_cap("ALEO_MI355X_COMMIT_CHUNK", COMMIT_CHUNK);
  HIPCHK(hipMemsetAsync(droute, 0, 4, s));
  for (size_t lo = 0; lo < n; lo += cap) {
    const size_t hi = n - lo < cap ? n : lo + cap;
    hipLaunchKernelGGL(k_records_commit, dim3((uint32_t)((hi - lo + COMMIT_BLOCK - 1) / COMMIT_BLOCK)), dim3(COMMIT_BLOCK), 0, s, dcm, dflags, droute, fields, off, index, kind, status, text, soff,
                       dK, A, (uint32_t)lo, (uint32_t)hi);
    HIPCHK(hipGetLastError());
  }
  return ALEO_MI355X_OK;
}

// ---- the host path ------------------------------------------------------------------------------------------------------------------------------------
int32_t commit_call(CommitCall& cc, const char* program_id, const char* record_name) {
  size_t dot;
  if (!program_id || !serial::program_id_ok(program_id, &dot)) return bad_arg("Invalid ProgramID specified");
  if (!record_name || !serial::identifier_ok(record_name, std::strlen(record_name))) return bad_arg("Invalid Identifier specified for record");
  cc.name_bits = serial::commit_name_bits(program_id, dot, record_name);
  cc.args = serial::commit_args(cc.name_bits);
  return ALEO_MI355X_OK;
}

uint8_t commit_one_host(uint8_t* out32, const char* record1, size_t chars, const uint8_t* plain, size_t n_fields, const CommitCall& cc) {
  static const uint8_t none[32] = {0};                         // a record without private fields is still a plaintext: record_bits takes a null pointer for a ciphertext
  std::memset(out32, 0, 32);
  const std::string s(record1, chars);
  plaintext::Record r;
  if (plaintext::parse(r, s.c_str(), "record_commitment") || r.n_private != n_fields) return (uint8_t)COMMIT_REFUSED;
  std::vector<uint8_t> bits = cc.name_bits;
  if (serial::record_bits(bits, r, n_fields ? plain : none, "record_commitment")) return (uint8_t)COMMIT_REFUSED;
  serial::store_canonical(out32, serial::bhp1024().hash(bits));
  return (uint8_t)COMMIT_OK;
}

// row k of a result's records: the status where it is not 0, else the record's own flag
static void commit_rows_on_host(uint8_t* cm, uint8_t* flags, const uint32_t* index, const uint32_t* off, const uint8_t* status, const uint8_t* plain, size_t count, const char* text,
                                const uint64_t* offsets, size_t base, const CommitCall& cc, bool routed_only) {
  for (size_t k = 0; k < count; ++k) {
    if (routed_only && flags[k] != COMMIT_ROUTED) continue;
    const size_t i = base + index[k];
    if (status[k] != FOUND_OK) { std::memset(cm + 32 * k, 0, 32); flags[k] = status[k]; continue; }
    flags[k] = commit_one_host(cm + 32 * k, text + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), plain + 32 * (size_t)off[k], off[k + 1] - off[k], cc);
  }
}

// ---- inside the flow ----------------------------------------------------------------------------------------------------------------------------------
int32_t commit_rows_of_chunk(Ctx* c, hipStream_t s, const FoundChunk& ch, const CommitCall& cc, const char* text, const uint64_t* offsets, char* dcm, uint8_t* dflags, uint32_t* droute,
                             CommitScratch& H, bool want_host) {
  const size_t owned = ch.owned;
  const bool on_device = owned >= aleo_mi355x_min_commitments();
  uint32_t routed = 0;
  if (on_device) {
    const uint32_t* dK; if (int32_t rc = commit_tables_on_device(c->device, &dK)) return rc;
    if (int32_t rc = launch_records_commit(s, dcm, dflags, droute, ch.fields, ch.off, ch.index, ch.kind, ch.status, ch.text, ch.soff, dK, cc.args, owned)) return rc;
    uint32_t* h_route = &ch.pin->routed;
    HIPCHK(hipMemcpyAsync(h_route, droute, 4, hipMemcpyDeviceToHost, s));
    if (want_host) { H.cm.resize(owned * 32); HIPCHK(hipMemcpyAsync(H.cm.data(), dcm, owned * 32, hipMemcpyDeviceToHost, s)); }
    HIPCHK(hipStreamSynchronize(s));
    routed = *h_route;
    if (!routed) return ALEO_MI355X_OK;
  }
  // the calling thread: every row of a small chunk, or the routed ones.  The chunk's arrays come down for it.
  H.index.resize(owned); H.off.resize(owned + 1); H.status.resize(owned); H.fields.resize(ch.nf * 32); H.cm.resize(owned * 32); H.flags.resize(owned);
  HIPCHK(hipMemcpyAsync(H.index.data(), ch.index, owned * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(H.off.data(), ch.off, (owned + 1) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(H.status.data(), ch.status, owned, hipMemcpyDeviceToHost, s));
  if (ch.nf) HIPCHK(hipMemcpyAsync(H.fields.data(), ch.fields, ch.nf * 32, hipMemcpyDeviceToHost, s));
  if (on_device) {
    HIPCHK(hipMemcpyAsync(H.cm.data(), dcm, owned * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(H.flags.data(), dflags, owned, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  commit_rows_on_host(H.cm.data(), H.flags.data(), H.index.data(), H.off.data(), H.status.data(), H.fields.data(), owned, text, offsets, ch.at, cc, on_device);
  HIPCHK(hipMemcpyAsync(dcm, H.cm.data(), owned * 32, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dflags, H.flags.data(), owned, hipMemcpyHostToDevice, s));
  return ALEO_MI355X_OK;
}

// ---- the stand-alone call -------------------------------------------------------------------------------------------------------------------------------
// The owned strings' text and the result's arrays go up, one launch chain runs, rows and flags come down; the routed rows are the calling thread's.  The text and
// its offsets are declared outside the slot: they outlive the copies that read them.
static int32_t commitments_on_device(uint8_t* cm_out, uint8_t* flags, const Found& F, const char* text, const uint64_t* offsets, const CommitCall& cc) {
  const size_t count = F.index.size(), nf = F.offsets.back();
  std::vector<uint32_t> soff(count + 1, 0);
  size_t chars = 0;
  for (size_t k = 0; k < count; ++k) {
    const uint64_t span = offsets[F.index[k] + 1] - offsets[F.index[k]];
    if (span > RS_MAX_CHARS || chars + span > UINT32_MAX) return bad_arg("records_commitments_found: the strings are not those the result was made from");
    chars += span; soff[k + 1] = (uint32_t)chars;
  }
  std::vector<char> owned_text(chars);
  for (size_t k = 0; k < count; ++k) std::memcpy(owned_text.data() + soff[k], text + offsets[F.index[k]], soff[k + 1] - soff[k]);
  return on_slot([&](Ctx* c) -> int32_t {
    const uint32_t* dK; if (int32_t rc = commit_tables_on_device(c->device, &dK)) return rc;
    hipStream_t s = c->stream;
    Carve cv;
    const size_t o_text = cv.part(chars), o_soff = cv.part((count + 1) * 4), o_fields = cv.part(nf * 32), o_off = cv.part((count + 1) * 4), o_kind = cv.part(count), o_status = cv.part(count),
                 o_cm = cv.part(count * 32), o_fl = cv.part(count), o_route = cv.part(4);
    if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
    char* b = c->scalars_stage.as<char>();
    HIPCHK(hipMemcpyAsync(b + o_text, owned_text.data(), chars, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b + o_soff, soff.data(), (count + 1) * 4, hipMemcpyHostToDevice, s));
    if (nf) HIPCHK(hipMemcpyAsync(b + o_fields, F.plain.data(), nf * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b + o_off, F.offsets.data(), (count + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b + o_kind, F.kind.data(), count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b + o_status, F.status.data(), count, hipMemcpyHostToDevice, s));
    if (int32_t rc = launch_records_commit(s, b + o_cm, (uint8_t*)(b + o_fl), (uint32_t*)(b + o_route), b + o_fields, (const uint32_t*)(b + o_off), nullptr, (const int8_t*)(b + o_kind),
                                       (const uint8_t*)(b + o_status), b + o_text, (const uint32_t*)(b + o_soff), dK, cc.args, count)) return rc;
    HIPCHK(hipMemcpyAsync(cm_out, b + o_cm, count * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(flags, b + o_fl, count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    commit_rows_on_host(cm_out, flags, F.index.data(), F.offsets.data(), F.status.data(), F.plain.data(), count, text, offsets, 0, cc, true);
    return ALEO_MI355X_OK;
  });
}

static int32_t commitments_found(void* cm_out, uint8_t* flags, const Found* found, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name,
                                 bool may_route) {
  if (!found) return bad_arg("records_commitments_found: null result");
  CommitCall cc; if (int32_t rc = commit_call(cc, program_id, record_name)) return rc;
  const Found& F = *found;
  const size_t count = F.index.size();
  if (count && (!cm_out || !flags)) return bad_arg("records_commitments_found: null buffer");
  if (int32_t rc = strings_args_ok("records_commitments_found", text, offsets, n)) return rc;
  for (size_t k = 0; k < count; ++k) if (F.index[k] >= n) return bad_arg("records_commitments_found: the result was made from more strings than there are");
  if (!count) return ALEO_MI355X_OK;
  if (may_route && count >= aleo_mi355x_min_commitments()) return commitments_on_device((uint8_t*)cm_out, flags, F, text, offsets, cc);
  commit_rows_on_host((uint8_t*)cm_out, flags, F.index.data(), F.offsets.data(), F.status.data(), F.plain.data(), count, text, offsets, 0, cc, false);
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The number of owned records from which the commitments take the GPU: the measured crossover against the host path on one thread, which is what a call below it
// runs (profiles/records_commit.txt: the stand-alone GPU call takes 1.2-1.5 ms for any batch up to 2^10; the host path 0.83 ms for 2^4 records, 1.63 ms for 2^5)
size_t aleo_mi355x_min_commitments(void) { return env_size("ALEO_MI355X_MIN_COMMITMENTS", (size_t)1 << 5); }

int32_t aleo_mi355x_records_commitments_found(void* cm_out, uint8_t* flags, const aleo_mi355x_found* found, const char* text, const uint64_t* offsets, size_t n, const char* program_id,
                                              const char* record_name) {
  return guarded([&] { return commitments_found(cm_out, flags, found, text, offsets, n, program_id, record_name, true); });
}
int32_t aleo_mi355x_records_commitments_found_host(void* cm_out, uint8_t* flags, const aleo_mi355x_found* found, const char* text, const uint64_t* offsets, size_t n, const char* program_id,
                                                   const char* record_name) {
  return guarded([&] { return commitments_found(cm_out, flags, found, text, offsets, n, program_id, record_name, false); });
}

}  // extern "C"
