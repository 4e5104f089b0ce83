// plaintexts.hip — record PLAINTEXT strings: what every write call of the reference takes its records as (`fee_record`, `amount_record`:
// wasm/src/programs/manager/transfer.rs:66-68) and what a wallet stores — parsed, committed and serial-numbered.  RecordPlaintext.fromString, microcredits() and
// serialNumberString (wasm/src/record/record_plaintext.rs:45-82) for one string on the host, and for a batch "which of the plaintexts I hold are unspent?" in one
// call: commitments, serial numbers under one key, and the look-up in a set of spent serial numbers.
//
// The kernel (one string per lane: plaintexts_lane.h, over records_commit_lane.h's commit_hash and the commitment lane's resident table), the same bytes on the host
// (plaintext_parse.hpp's parse and record_bits, serial_host.hpp's BHP1024 — what small batches take, what the lane routes, and the checker), the routing
// threshold, and the flow of the batch calls on one slot and one stream:
//   text and offsets go up — k_plaintexts_commit — the rows the lane routed are computed by the calling thread and patched in — k_records_serial over the
//   commitments (records_serial.hip's, through launch_records_serial) — k_spent_insert over the spent set (records_unspent.hip's, through launch_spent_insert) —
//   k_plaintexts_flags: the look-up and the rows' final flags — rows and flags come down.
// Flags: 0 computed (and not in the set); 1 computed and in the spent set; 2 the serial number is refused (records_serial_numbers' own flag); 3 not a record
// plaintext.  A row that is not computed is zeros.
// The batch calls check canonical encoding only, as plaintext::render does; aleo_mi355x_record_plaintext_parse alone also asks that the owner, the nonce and
// every `group` value are x-coordinates of points of the prime-order subgroup (sig::point_from_x, the recovery the signature path has).
#include "records_found.h"
#include "records_spent_lane.h"
#include "plaintexts_lane.h"
#include "plaintext_parse.hpp"
#include "commit_host.hpp"
#include "signature_host.hpp"
#include <algorithm>
#include <array>

namespace aleo_mi355x {

static constexpr uint32_t PLAINTEXTS_BLOCK = 256;
static constexpr size_t PLAINTEXTS_CHUNK = (size_t)1 << 20;      // strings per launch
static constexpr uint8_t PT_FLAG_SPENT = 1, PT_FLAG_NOT_A_RECORD = 3;
static const char* const PT_INVALID = "The record plaintext string provided was invalid";      // RecordPlaintext.fromString's text (record_plaintext.rs:178)

static thread_local size_t g_plaintexts_routed = 0;

// ---- the kernels ----------------------------------------------------------------------------------------------------------------------------------------
// The strings lo .. hi, one per lane: string j is the characters soff[j] .. soff[j + 1] of text.  flags: 0, or COMMIT_ROUTED with a row of zeros; route counts the latter.
__global__ void __launch_bounds__(PLAINTEXTS_BLOCK) k_plaintexts_commit(char* __restrict__ cm, uint64_t* __restrict__ mc, uint8_t* __restrict__ flags, uint32_t* __restrict__ route,
                                                                        const char* __restrict__ text, const uint32_t* __restrict__ soff, const uint32_t* __restrict__ K, CommitArgs A,
                                                                        uint32_t lo, uint32_t hi) {
  const uint32_t j = lo + blockIdx.x * PLAINTEXTS_BLOCK + threadIdx.x;
  if (j >= hi) return;                                         // no barrier below
  uint4* out = (uint4*)(cm + (size_t)j * 32);
  uint64_t* my_mc = mc + j; uint8_t* my_flag = flags + j;
  asm volatile("" : "+v"(out), "+v"(my_mc), "+v"(my_flag), "+v"(route));      // what the lane writes through, in vector registers from here on: the four pointers' eight scalar ones are free
  const uint32_t first = soff[j], len = soff[j + 1] - first;
  const uint8_t* __restrict__ mine = (const uint8_t*)text + first;
  uint64_t microcredits = 0;
  const uint32_t flag = plaintexts_commit_lane([&](uint32_t q) { return mine[q]; }, len, K, A, microcredits, [&](const F29& v) { store_fp<Fr>(out, f29_to_fr(v)); });
  if (flag) { out[0] = make_uint4(0, 0, 0, 0); out[1] = make_uint4(0, 0, 0, 0); atomicAdd(route, 1u); }
  *my_mc = flag ? 0 : microcredits;
  *my_flag = (uint8_t)flag;
}

// The rows' final flags, one row per lane: the commitment's flag where it is not 0 (and the serial number zeroed), else the serial number's, else 1 where the
// serial number is in the set (cap 0: no set).
__global__ void __launch_bounds__(PLAINTEXTS_BLOCK) k_plaintexts_flags(uint8_t* __restrict__ flags, uint32_t* __restrict__ sn, const uint8_t* __restrict__ cm_flags, const uint32_t* __restrict__ table,
                                                                       uint32_t cap, const uint32_t* __restrict__ spent, uint32_t n) {
  const uint32_t j = blockIdx.x * PLAINTEXTS_BLOCK + threadIdx.x;
  if (j >= n) return;
  uint4* row = (uint4*)(sn + (size_t)j * 8);
  uint32_t flag = cm_flags[j];
  if (flag) { row[0] = make_uint4(0, 0, 0, 0); row[1] = make_uint4(0, 0, 0, 0); }
  else flag = flags[j];
  if (!flag && cap) {
    const uint4 l = row[0], h = row[1];
    const uint32_t mine[8] = {l.x, l.y, l.z, l.w, h.x, h.y, h.z, h.w};
    if (spent_probe(cap, mine, [&](uint32_t slot) { return table[slot]; }, [&](uint32_t r, uint32_t k) { return spent[(size_t)r * 8 + k]; })) flag = PT_FLAG_SPENT;
  }
  flags[j] = (uint8_t)flag;
}

// ---- the host path ------------------------------------------------------------------------------------------------------------------------------------
// one string on the host: the flag (0, or 3 with a row of zeros and no microcredits)
static uint8_t plaintext_one_host(uint8_t* cm32, uint64_t* microcredits, const char* s, size_t chars, const CommitCall& cc) {
  std::memset(cm32, 0, 32);
  if (microcredits) *microcredits = 0;
  ptext::Parsed r; std::string why;
  std::vector<uint8_t> bits = cc.name_bits;
  if (!ptext::parse(r, s, chars, why) || !ptext::record_bits(bits, r, why)) return PT_FLAG_NOT_A_RECORD;
  serial::store_canonical(cm32, serial::bhp1024().hash(bits));
  if (microcredits) *microcredits = ptext::microcredits(r);
  return 0;
}

using Row32 = std::array<uint8_t, 32>;
struct SerialCall { ScanArgs key; const uint8_t* spent; size_t n_spent; };      // null for the commitments alone

// the serial number and the final flag of a row whose commitment is there
static uint8_t serial_row_host(uint8_t* sn32, const uint8_t* cm32, const SerialCall& sc, const std::vector<Row32>& sorted_spent) {
  const uint8_t flag = serial::serial_one_host(sn32, cm32, sc.key, serial::serial_tables());
  if (flag) return flag;
  Row32 row; std::memcpy(row.data(), sn32, 32);
  return std::binary_search(sorted_spent.begin(), sorted_spent.end(), row) ? PT_FLAG_SPENT : 0;
}

static void plaintexts_on_host(uint8_t* sn, uint8_t* cm, uint64_t* mc, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const CommitCall& cc, const SerialCall* sc) {
  std::vector<Row32> sorted_spent(sc ? sc->n_spent : 0);
  if (!sorted_spent.empty()) std::memcpy(sorted_spent.data(), sc->spent, sc->n_spent * 32);
  std::sort(sorted_spent.begin(), sorted_spent.end());
  for (size_t i = 0; i < n; ++i) {
    uint8_t row[32];
    flags[i] = plaintext_one_host(row, mc ? mc + i : nullptr, text + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), cc);
    if (cm) std::memcpy(cm + 32 * i, row, 32);
    if (!sc) continue;
    if (flags[i]) std::memset(sn + 32 * i, 0, 32); else flags[i] = serial_row_host(sn + 32 * i, row, *sc, sorted_spent);
  }
  g_plaintexts_routed = n;
}

// ---- the device flow ----------------------------------------------------------------------------------------------------------------------------------
// k_plaintexts_commit over n strings in launches of at most ALEO_MI355X_PLAINTEXTS_CHUNK lanes (read per call); *droute is zeroed first
static int32_t launch_plaintexts_commit(hipStream_t s, char* dcm, uint64_t* dmc, uint8_t* dflags, uint32_t* droute, const char* text, const uint32_t* soff, const uint32_t* dK, const CommitArgs& A, size_t n) {
  const size_t cap = env_cap("ALEO_MI355X_PLAINTEXTS_CHUNK", PLAINTEXTS_CHUNK);
  HIPCHK(hipMemsetAsync(droute, 0, 4, s));
  for (size_t lo = 0; lo < n; lo += cap) {
    const size_t hi = n - lo < cap ? n : lo + cap;
    hipLaunchKernelGGL(k_plaintexts_commit, dim3((uint32_t)((hi - lo + PLAINTEXTS_BLOCK - 1) / PLAINTEXTS_BLOCK)), dim3(PLAINTEXTS_BLOCK), 0, s, dcm, dmc, dflags, droute, text, soff, dK, A,
                       (uint32_t)lo, (uint32_t)hi);
    HIPCHK(hipGetLastError());
  }
  return ALEO_MI355X_OK;
}

// The staging vectors are declared outside the slot: they outlive the copies that read and write them.
static int32_t plaintexts_on_device(uint8_t* sn, uint8_t* cm, uint64_t* mc, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const CommitCall& cc, const SerialCall* sc) {
  const uint64_t chars = offsets[n] - offsets[0];
  if (chars > UINT32_MAX) return bad_arg("plaintexts: more than 2^32 - 1 characters in one call");
  std::vector<uint32_t> soff(n + 1);
  for (size_t i = 0; i <= n; ++i) soff[i] = (uint32_t)(offsets[i] - offsets[0]);
  std::vector<uint8_t> h_cm(n * 32), h_flags(n); std::vector<uint64_t> h_mc(n);
  SerialArgs key{}; if (sc) key = serial_args_of(sc->key);
  const size_t n_spent = sc ? sc->n_spent : 0;
  const uint32_t cap = n_spent ? spent_capacity(n_spent) : 0;
  size_t routed = 0;
  const int32_t rc = on_slot([&](Ctx* c) -> int32_t {
    const uint32_t* dK; if (int32_t rc = commit_tables_on_device(c->device, &dK)) return rc;
    const uint32_t* dKs = nullptr; if (sc) if (int32_t rc = serial_tables_on_device(c->device, &dKs)) return rc;
    if (int32_t rc = ensure_host_pinned(c, 4)) return rc;
    uint32_t* h_route = (uint32_t*)c->h_pinned;
    hipStream_t s = c->stream;
    Carve cv;
    const size_t o_text = cv.part(chars), o_soff = cv.part((n + 1) * 4), o_cm = cv.part(n * 32), o_mc = cv.part(n * 8), o_cf = cv.part(n), o_route = cv.part(4), o_key = cv.part(sizeof(SerialArgs)),
                 o_sn = cv.part(sc ? n * 32 : 0), o_fl = cv.part(sc ? n : 0), o_rows = cv.part(n_spent * 32), o_table = cv.part((size_t)cap * 4);
    if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
    char* b = c->scalars_stage.as<char>();
    if (chars) HIPCHK(hipMemcpyAsync(b + o_text, text + offsets[0], chars, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b + o_soff, soff.data(), (n + 1) * 4, hipMemcpyHostToDevice, s));
    if (int32_t rc = launch_plaintexts_commit(s, b + o_cm, (uint64_t*)(b + o_mc), (uint8_t*)(b + o_cf), (uint32_t*)(b + o_route), b + o_text, (const uint32_t*)(b + o_soff), dK, cc.args, n)) return rc;
    HIPCHK(hipMemcpyAsync(h_route, b + o_route, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_cm.data(), b + o_cm, n * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_mc.data(), b + o_mc, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_flags.data(), b + o_cf, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    routed = *h_route;
    if (routed) {                                              // the calling thread: the rows the lane routed
      for (size_t i = 0; i < n; ++i)
        if (h_flags[i] == COMMIT_ROUTED) h_flags[i] = plaintext_one_host(h_cm.data() + 32 * i, &h_mc[i], text + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), cc);
      if (sc) {
        HIPCHK(hipMemcpyAsync(b + o_cm, h_cm.data(), n * 32, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b + o_cf, h_flags.data(), n, hipMemcpyHostToDevice, s));
      }
    }
    if (!sc) return ALEO_MI355X_OK;
    HIPCHK(hipMemcpyAsync(b + o_key, &key, sizeof key, hipMemcpyHostToDevice, s));
    UnspentSegs seg{}; seg.n_keys = 1; seg.rank0[1] = (uint32_t)n; seg.wave0[1] = (uint32_t)((n + 63) / 64);
    if (int32_t rc = launch_records_serial(s, b + o_sn, (uint8_t*)(b + o_fl), b + o_cm, dKs, (const SerialArgs*)(b + o_key), seg)) return rc;
    if (n_spent) {
      HIPCHK(hipMemcpyAsync(b + o_rows, sc->spent, n_spent * 32, hipMemcpyHostToDevice, s));
      if (int32_t rc = launch_spent_insert(s, (uint32_t*)(b + o_table), cap, (const uint32_t*)(b + o_rows), n_spent)) return rc;
    }
    hipLaunchKernelGGL(k_plaintexts_flags, dim3((uint32_t)((n + PLAINTEXTS_BLOCK - 1) / PLAINTEXTS_BLOCK)), dim3(PLAINTEXTS_BLOCK), 0, s, (uint8_t*)(b + o_fl), (uint32_t*)(b + o_sn),
                       (const uint8_t*)(b + o_cf), (const uint32_t*)(b + o_table), cap, (const uint32_t*)(b + o_rows), (uint32_t)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sn, b + o_sn, n * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(flags, b + o_fl, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ALEO_MI355X_OK;
  });
  if (rc) return rc;
  if (cm) std::memcpy(cm, h_cm.data(), n * 32);
  if (mc) std::memcpy(mc, h_mc.data(), n * 8);
  if (!sc) std::memcpy(flags, h_flags.data(), n);
  g_plaintexts_routed = routed;
  return ALEO_MI355X_OK;
}

static int32_t plaintexts(void* sn_out, void* cm_out, uint64_t* microcredits, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name,
                          const void* sk_sig32, const void* spent32, size_t n_spent, bool serials, bool may_route) {
  const char* who = serials ? "plaintexts_serial_numbers" : "plaintexts_commitments";
  g_plaintexts_routed = 0;
  CommitCall cc; if (int32_t rc = commit_call(cc, program_id, record_name)) return rc;
  if (n && (!flags || (serials ? !sn_out : !cm_out))) return bad_arg("plaintexts: null buffer");
  SerialCall sc{}; sc.spent = (const uint8_t*)spent32; sc.n_spent = n_spent;
  if (serials) {
    if (!sk_sig32 || !serial::serial_key(sc.key, sk_sig32)) return bad_arg("plaintexts_serial_numbers: sk_sig is not a canonical scalar below the subgroup order");
    if (n_spent && !spent32) return bad_arg("plaintexts_serial_numbers: null spent set with n_spent > 0");
    if (n_spent > SPENT_MAX_ROWS) return bad_arg("plaintexts_serial_numbers: more than 2^30 spent serial numbers");
  }
  if (int32_t rc = strings_args_ok(who, text, offsets, n)) return rc;
  if (n > UINT32_MAX) return bad_arg("plaintexts: more than 2^32 - 1 strings");
  if (!n) return ALEO_MI355X_OK;
  if (may_route && n >= aleo_mi355x_min_plaintexts()) return plaintexts_on_device((uint8_t*)sn_out, (uint8_t*)cm_out, microcredits, flags, text, offsets, n, cc, serials ? &sc : nullptr);
  plaintexts_on_host((uint8_t*)sn_out, (uint8_t*)cm_out, microcredits, flags, text, offsets, n, cc, serials ? &sc : nullptr);
  return ALEO_MI355X_OK;
}

// every x-coordinate a record holds — the owner, the nonce, `group` values — is that of a point of the prime-order subgroup
static bool points_ok(const ptext::Value& v) {
  if (v.is_struct) { for (const auto& m : v.members) if (!points_ok(m.second)) return false; return true; }
  if (v.type != 0 && v.type != 3) return true;
  HFr x; std::memcpy(x.l, v.v, 32); EdH p;
  return sig::point_from_x(p, x);
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The batch size from which the plaintext calls take the GPU: the measured crossover against the host twin on one thread of a call without a spent set
// (profiles/records_plaintexts.txt: serial numbers 5.86 ms against 3.04 at 2^4 and 5.89 against 6.09 at 2^5; commitments 1.37 against 0.80 and 1.38 against 1.58)
size_t aleo_mi355x_min_plaintexts(void) { return env_size("ALEO_MI355X_MIN_PLAINTEXTS", (size_t)1 << 5); }

size_t aleo_mi355x_plaintexts_last_routed(void) { return g_plaintexts_routed; }

int32_t aleo_mi355x_record_plaintext_parse(const char* plaintext, int32_t* owner_kind, void* owner_x32, void* nonce_x32, uint64_t* microcredits) {
  return guarded([&] {
    if (!plaintext) return bad_arg("record_plaintext_parse: null string");
    ptext::Parsed r; std::string why;
    if (!ptext::parse(r, plaintext, std::strlen(plaintext), why)) { g_last_error = std::string(PT_INVALID) + " (" + why + ")"; return ALEO_MI355X_ERR_BAD_ARG; }
    ptext::Value owner, nonce; std::memcpy(owner.v, r.owner, 32); nonce.type = 3; std::memcpy(nonce.v, r.nonce, 32);
    bool on_curve = points_ok(owner) && points_ok(nonce);
    for (const ptext::Entry& e : r.entries) on_curve = on_curve && points_ok(e.value);
    if (!on_curve) { g_last_error = std::string(PT_INVALID) + " (an x-coordinate is that of no point of the subgroup)"; return ALEO_MI355X_ERR_BAD_ARG; }
    if (owner_kind) *owner_kind = r.owner_kind;
    if (owner_x32) std::memcpy(owner_x32, r.owner, 32);
    if (nonce_x32) std::memcpy(nonce_x32, r.nonce, 32);
    if (microcredits) *microcredits = ptext::microcredits(r);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_plaintext_commitment(void* out32, const char* plaintext, const char* program_id, const char* record_name) {
  return guarded([&] {
    CommitCall cc; if (int32_t rc = commit_call(cc, program_id, record_name)) return rc;
    if (!out32 || !plaintext) return bad_arg("plaintext_commitment: null buffer");
    if (plaintext_one_host((uint8_t*)out32, nullptr, plaintext, std::strlen(plaintext), cc)) return bad_arg(PT_INVALID);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_plaintexts_commitments(void* cm_out, uint64_t* microcredits, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const char* program_id,
                                           const char* record_name) {
  return guarded([&] { return plaintexts(nullptr, cm_out, microcredits, flags, text, offsets, n, program_id, record_name, nullptr, nullptr, 0, false, true); });
}
int32_t aleo_mi355x_plaintexts_commitments_host(void* cm_out, uint64_t* microcredits, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const char* program_id,
                                                const char* record_name) {
  return guarded([&] { return plaintexts(nullptr, cm_out, microcredits, flags, text, offsets, n, program_id, record_name, nullptr, nullptr, 0, false, false); });
}
int32_t aleo_mi355x_plaintexts_serial_numbers(void* sn_out, void* cm_out, uint64_t* microcredits, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const char* program_id,
                                              const char* record_name, const void* sk_sig32, const void* spent32, size_t n_spent) {
  return guarded([&] { return plaintexts(sn_out, cm_out, microcredits, flags, text, offsets, n, program_id, record_name, sk_sig32, spent32, n_spent, true, true); });
}
int32_t aleo_mi355x_plaintexts_serial_numbers_host(void* sn_out, void* cm_out, uint64_t* microcredits, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const char* program_id,
                                                   const char* record_name, const void* sk_sig32, const void* spent32, size_t n_spent) {
  return guarded([&] { return plaintexts(sn_out, cm_out, microcredits, flags, text, offsets, n, program_id, record_name, sk_sig32, spent32, n_spent, true, false); });
}

}  // extern "C"
