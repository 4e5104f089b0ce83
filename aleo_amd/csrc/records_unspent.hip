// records_unspent.hip — unspent_strings and unspent_strings_many: the records each of K accounts owns among n "record1…" strings that decrypt, whose serial
// number computes and is not in a set S of spent serial numbers — the whole of the reference's get_unspent_records behind the fetch of the blocks
// (rust/src/api/blocking.rs:229-325: is_owner, decrypt, serial_number, the spent check) in one call.  The one-account call is K = 1.
//
// records.py's `unspent` takes that road in pieces: decrypt_strings brings every owned record down, the spent ones included, found_serial_numbers is a second
// call with one key per launch, and the spent check is a callback per record.  Here the flow of decrypt_strings_many (records_found.hip) runs as it stands and,
// per chunk, behind k_found_microcredits (records_found.h FoundStage):
//   — the compacted `index` comes down behind the gather, while the decryption's kernels are still to run; the host gathers the owned records' commitment rows
//   (owned x 32 B go up instead of the chunk's m x 32 B: a wallet owns a small part of what it scans) —
//   k_records_serial    records_serial.hip's, the kernel of the one-account serial numbers too: ONE launch over the owned pairs of ALL keys, one pair per lane,
//                       every key's segment of the compacted arrays padded to whole waves so that a wave has one key (launch_records_serial, records_found.h)
//                       Below aleo_mi355x_min_serials() owned pairs the host computes the serial numbers inside the call (the rows are there already) and
//                       uploads them: the kernel's chain costs the same for 1 pair as for 2^14.  The bytes are the same either way.
//   k_unspent_keep      one lane per owned pair: keep = status 0, flag 0 and not in S (records_spent_lane.h; no S: no probe); then the first level of the exclusive
//                       sums of the keep bits and of the kept records' field counts, in rank order, which is [key][record] order
//   k_found_offsets     records_found.hip's, over the block totals
//   k_unspent_scatter   index, kind, rvk, offsets, microcredits, serial numbers and fields of the kept pairs into a SECOND set of arrays (moving fields forward
//                       in place would race between blocks); the kept ranks and fields before each key's segment, K + 1 of each
//   — one read of the totals and boundaries; the kept arrays come down as decrypt_strings_many's would, and are split per key by the same code —
// S goes up once per call: its rows, and an open-addressing table over them built by k_spent_insert (one row per lane, atomicCAS).  n_spent = 0: neither.
// The host path is found_on_host per key, serial_one_host per owned record and a sorted vector of S's rows; it shares no code with the above.
// unspent_named[_many] are the same flow without commitments from outside: the stage computes them (records_commit.hip commit_rows_of_chunk: k_records_commit over the
// chunk's owned records, or the calling thread below aleo_mi355x_min_commitments() of them) where the other road gathers and uploads the caller's rows; there is then no
// index download and no wait behind the gather, k_unspent_keep reads the commitment flags too, and k_unspent_scatter compacts the rows, which come down with the rest.
#include "records_found.h"
#include "records_spent_lane.h"
#include "serial_host.hpp"
#include <algorithm>
#include <array>
#include <string>

namespace aleo_mi355x {

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------------------
// One row of S per lane.
__global__ void __launch_bounds__(FOUND_BLOCK) k_spent_insert(uint32_t* __restrict__ table, uint32_t cap, const uint32_t* __restrict__ rows, uint32_t n_spent) {
  const uint32_t i = blockIdx.x * FOUND_BLOCK + threadIdx.x;
  if (i >= n_spent) return;
  spent_insert(cap, i, rows[(size_t)i * 8], [&](uint32_t slot, uint32_t expected, uint32_t desired) { return atomicCAS(&table[slot], expected, desired); });
}

int32_t launch_spent_insert(hipStream_t s, uint32_t* table, uint32_t cap, const uint32_t* rows, size_t n_spent) {
  HIPCHK(hipMemsetAsync(table, 0, (size_t)cap * 4, s));
  hipLaunchKernelGGL(k_spent_insert, dim3((uint32_t)((n_spent + FOUND_BLOCK - 1) / FOUND_BLOCK)), dim3(FOUND_BLOCK), 0, s, table, cap, rows, (uint32_t)n_spent);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

// cnt / pos: the exclusive sums of the kept field counts and of the keep bits WITHIN the block; blk: [fields | kept][block], the block totals.  cap 0: no set.
// cm_flags (unspent_named; else null): the flags of the commitments the call computed itself.
__global__ void __launch_bounds__(FOUND_BLOCK) k_unspent_keep(uint32_t* __restrict__ cnt, uint32_t* __restrict__ pos, uint8_t* __restrict__ keep, uint32_t* __restrict__ blk,
                                                             const uint8_t* __restrict__ status, const uint8_t* __restrict__ flags, const uint8_t* __restrict__ cm_flags, const uint32_t* __restrict__ sn,
                                                             const uint32_t* __restrict__ off, const uint32_t* __restrict__ table, uint32_t cap,
                                                             const uint32_t* __restrict__ spent, uint32_t n_owned) {
  __shared__ uint32_t wave_tot[2][FOUND_BLOCK / 64];
  const uint32_t j = blockIdx.x * FOUND_BLOCK + threadIdx.x;
  const bool live = j < n_owned;
  bool kept = live && status[j] == FOUND_OK && flags[j] == 0 && (!cm_flags || cm_flags[j] == 0);
  if (kept && cap) {
    const uint4 l = *(const uint4*)(sn + (size_t)j * 8), h = *(const uint4*)(sn + (size_t)j * 8 + 4);
    const uint32_t mine[8] = {l.x, l.y, l.z, l.w, h.x, h.y, h.z, h.w};
    kept = !spent_probe(cap, mine, [&](uint32_t slot) { return table[slot]; }, [&](uint32_t row, uint32_t k) { return spent[(size_t)row * 8 + k]; });
  }
  uint32_t a = kept ? off[j + 1] - off[j] : 0u, b = kept ? 1u : 0u, ta, tb;
  block_exclusive2(a, b, wave_tot, &ta, &tb);
  if (live) { cnt[j] = a; pos[j] = b; keep[j] = kept ? 1 : 0; }
  if (threadIdx.x == 0) { blk[blockIdx.x] = ta; blk[gridDim.x + blockIdx.x] = tb; }
}

// Behind k_found_offsets over blk (stat[0]: the kept pairs, stat[1]: their fields).  A kept pair's rank among the kept is blk[kept row][block] + pos, its first
// field blk[fields row][block] + cnt.  stat[8 + j] / stat[8 + 65 + j], j <= n_keys: the kept pairs / fields before key j's segment (j = n_keys: all of them).
__global__ void __launch_bounds__(FOUND_BLOCK) k_unspent_scatter(char* __restrict__ o_fields, uint32_t* __restrict__ o_index, int8_t* __restrict__ o_kind, char* __restrict__ o_rvk,
                                                                uint32_t* __restrict__ o_off, uint64_t* __restrict__ o_mc, char* __restrict__ o_sn, char* __restrict__ o_cm, uint32_t* __restrict__ stat,
                                                                const char* __restrict__ fields, const uint32_t* __restrict__ index, const int8_t* __restrict__ kind,
                                                                const char* __restrict__ rvk, const uint32_t* __restrict__ off, const uint64_t* __restrict__ mc,
                                                                const char* __restrict__ sn, const char* __restrict__ cm, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ pos,
                                                                const uint8_t* __restrict__ keep, const uint32_t* __restrict__ blk, UnspentSegs seg, uint32_t n_owned) {
  const uint32_t nb = gridDim.x, j = blockIdx.x * FOUND_BLOCK + threadIdx.x;
  const uint32_t n_kept = stat[0], n_fields = stat[1];
  if (blockIdx.x == 0 && threadIdx.x <= seg.n_keys) {
    const uint32_t r = seg.rank0[threadIdx.x];
    stat[8 + threadIdx.x] = r >= n_owned ? n_kept : blk[nb + r / FOUND_BLOCK] + pos[r];
    stat[8 + SCAN_MANY_KEYS + 1 + threadIdx.x] = r >= n_owned ? n_fields : blk[r / FOUND_BLOCK] + cnt[r];
    if (threadIdx.x == 0) o_off[n_kept] = n_fields;
  }
  if (j >= n_owned || !keep[j]) return;
  const uint32_t q = blk[nb + blockIdx.x] + pos[j], f = blk[blockIdx.x] + cnt[j], first = off[j], m = off[j + 1] - first;
  if (q >= n_kept || f + m > n_fields) return;                 // cannot happen: the totals are these sums
  o_index[q] = index[j]; o_kind[q] = kind[j]; o_off[q] = f; o_mc[q] = mc[j];
  const uint4* r = (const uint4*)(rvk + (size_t)j * 32); uint4* ro = (uint4*)(o_rvk + (size_t)q * 32);
  ro[0] = r[0]; ro[1] = r[1];
  const uint4* s = (const uint4*)(sn + (size_t)j * 32); uint4* so = (uint4*)(o_sn + (size_t)q * 32);
  so[0] = s[0]; so[1] = s[1];
  if (o_cm) { const uint4* t = (const uint4*)(cm + (size_t)j * 32); uint4* to = (uint4*)(o_cm + (size_t)q * 32); to[0] = t[0]; to[1] = t[1]; }      // unspent_named
  for (uint32_t k = 0; k < m; ++k) {
    const uint4* p = (const uint4*)(fields + (size_t)(first + k) * 32); uint4* po = (uint4*)(o_fields + (size_t)(f + k) * 32);
    po[0] = p[0]; po[1] = p[1];
  }
}

// ---- the stage ----------------------------------------------------------------------------------------------------------------------------------------
struct UnspentKeys { ManyKeys scan; std::vector<ScanArgs> serial; };      // per account: the view key's and the address's arguments; sk_sig's digits

struct UnspentStage : FoundStage {
  const uint8_t* commitments; const UnspentKeys& keys; const uint8_t* spent; size_t n_spent;
  const uint32_t* dK = nullptr; const SerialArgs* dkeys = nullptr; const uint32_t* dspent = nullptr; const uint32_t* dtable = nullptr; uint32_t cap = 0;
  std::vector<SerialArgs> table;                               // outlives the call's last synchronisation
  std::vector<uint32_t> h_index; std::vector<uint8_t> h_cm, h_sn, h_fl;
  // unspent_named (named not null): no commitments come in; the stage computes them from the call's strings (records_commit.hip) in front of the serial numbers
  const CommitCall* named; const char* text; const uint64_t* offsets; CommitScratch H;
  UnspentStage(const uint8_t* cm, const UnspentKeys& k, const uint8_t* sp, size_t ns, const CommitCall* named_call, const char* strings, const uint64_t* string_offsets)
      : commitments(cm), keys(k), spent(sp), n_spent(ns), named(named_call), text(strings), offsets(string_offsets) {}

  // once per call: the lane's tables, the keys' digits, and S with its table
  int32_t begin(Ctx* c, hipStream_t s) override {
    if (int32_t rc = serial_tables_on_device(c->device, &dK)) return rc;
    const size_t K = keys.serial.size();
    table.resize(K);
    for (size_t j = 0; j < K; ++j) table[j] = serial_args_of(keys.serial[j]);
    cap = n_spent ? spent_capacity(n_spent) : 0;
    Carve cv;
    const size_t o_keys = cv.part(K * sizeof(SerialArgs)), o_rows = cv.part(n_spent * 32), o_table = cv.part((size_t)cap * 4);
    if (int32_t rc = c->unspent_set.reserve(cv.total)) return rc;
    char* base = c->unspent_set.as<char>();
    dkeys = (const SerialArgs*)(base + o_keys);
    HIPCHK(hipMemcpyAsync(base + o_keys, table.data(), K * sizeof(SerialArgs), hipMemcpyHostToDevice, s));
    if (!n_spent) return ALEO_MI355X_OK;
    dspent = (const uint32_t*)(base + o_rows); dtable = (const uint32_t*)(base + o_table);
    HIPCHK(hipMemcpyAsync(base + o_rows, spent, n_spent * 32, hipMemcpyHostToDevice, s));
    return launch_spent_insert(s, (uint32_t*)(base + o_table), cap, dspent, n_spent);
  }

  // the owned records' indices come down now: the host gathers their commitments while the decryption runs
  int32_t gathered(Ctx*, hipStream_t s, const FoundChunk& ch) override {
    if (named) return ALEO_MI355X_OK;                          // nothing to gather: no wait
    h_index.resize(ch.owned);
    HIPCHK(hipMemcpyAsync(h_index.data(), ch.index, ch.owned * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ALEO_MI355X_OK;
  }

  int32_t filter(Ctx* c, hipStream_t s, FoundChunk& ch) override {
    const size_t K = keys.serial.size(), owned = ch.owned, nf = ch.nf;
    const uint32_t nb = (uint32_t)((owned + FOUND_BLOCK - 1) / FOUND_BLOCK);
    const bool host_serials = owned < aleo_mi355x_min_serials();      // few pairs: the host's serial numbers, the same bytes
    if (!named) {
      h_cm.resize(owned * 32);
      for (size_t q = 0; q < owned; ++q) std::memcpy(h_cm.data() + 32 * q, commitments + 32 * (ch.at + h_index[q]), 32);
    }
    UnspentSegs seg{}; seg.n_keys = (uint32_t)K;
    for (size_t j = 0; j <= K; ++j) seg.rank0[j] = ch.first[j];
    for (size_t j = 0; j < K; ++j) seg.wave0[j + 1] = seg.wave0[j] + (ch.first[j + 1] - ch.first[j] + 63) / 64;
    const size_t stat_words = sizeof(FoundPinned::stage) / 4;
    Carve cv;
    const size_t o_cm = cv.part(owned * 32), o_cf = cv.part(owned), o_route = cv.part(4), k_cm = cv.part(owned * 32), o_sn = cv.part(owned * 32), o_fl = cv.part(owned), o_keep = cv.part(owned), o_cnt = cv.part(owned * 4), o_pos = cv.part(owned * 4), o_blk = cv.part((size_t)2 * nb * 4),
                 o_stat = cv.part(stat_words * 4), k_fields = cv.part(nf * 32), k_index = cv.part(owned * 4), k_off = cv.part((owned + 1) * 4), k_mc = cv.part(owned * 8), k_rvk = cv.part(owned * 32),
                 k_kind = cv.part(owned), k_sn = cv.part(owned * 32);
    if (int32_t rc = c->unspent_ws.reserve(cv.total)) return rc;
    char* b = c->unspent_ws.as<char>();
    char* dsn = b + o_sn; uint8_t* dfl = (uint8_t*)(b + o_fl); uint8_t* dkeep = (uint8_t*)(b + o_keep);
    uint32_t* dcnt = (uint32_t*)(b + o_cnt); uint32_t* dpos = (uint32_t*)(b + o_pos); uint32_t* dblk = (uint32_t*)(b + o_blk); uint32_t* dstat = (uint32_t*)(b + o_stat);
    const uint8_t* dcf = named ? (const uint8_t*)(b + o_cf) : nullptr;
    if (named) if (int32_t rc = commit_rows_of_chunk(c, s, ch, *named, text, offsets, b + o_cm, (uint8_t*)(b + o_cf), (uint32_t*)(b + o_route), H, host_serials)) return rc;
    const std::vector<uint8_t>& h_cm = named ? H.cm : this->h_cm;
    if (host_serials) {
      const serial::SerialTables& T = serial::serial_tables();
      h_sn.resize(owned * 32); h_fl.resize(owned);
      for (size_t j = 0; j < K; ++j)
        for (size_t q = ch.first[j]; q < ch.first[j + 1]; ++q) h_fl[q] = serial::serial_one_host(h_sn.data() + 32 * q, h_cm.data() + 32 * q, keys.serial[j], T);
      HIPCHK(hipMemcpyAsync(dsn, h_sn.data(), owned * 32, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(dfl, h_fl.data(), owned, hipMemcpyHostToDevice, s));
    } else {
      if (!named) HIPCHK(hipMemcpyAsync(b + o_cm, h_cm.data(), owned * 32, hipMemcpyHostToDevice, s));
      if (int32_t rc = launch_records_serial(s, dsn, dfl, b + o_cm, dK, dkeys, seg)) return rc;
    }
    hipLaunchKernelGGL(k_unspent_keep, dim3(nb), dim3(FOUND_BLOCK), 0, s, dcnt, dpos, dkeep, dblk, (const uint8_t*)ch.status, (const uint8_t*)dfl, dcf, (const uint32_t*)dsn, (const uint32_t*)ch.off,
                       dtable, cap, dspent, (uint32_t)owned);
    HIPCHK(hipGetLastError());
    launch_found_offsets(s, dblk, dstat, nb, nb);
    HIPCHK(hipGetLastError());
    FoundChunk kept = ch;
    kept.fields = b + k_fields; kept.index = (uint32_t*)(b + k_index); kept.off = (uint32_t*)(b + k_off); kept.mc = (uint64_t*)(b + k_mc); kept.rvk = b + k_rvk; kept.kind = (int8_t*)(b + k_kind);
    kept.serials = b + k_sn; kept.status = nullptr; kept.commitments = named ? b + k_cm : nullptr;
    hipLaunchKernelGGL(k_unspent_scatter, dim3(nb), dim3(FOUND_BLOCK), 0, s, kept.fields, kept.index, kept.kind, kept.rvk, kept.off, kept.mc, kept.serials, kept.commitments, dstat, (const char*)ch.fields,
                       (const uint32_t*)ch.index, (const int8_t*)ch.kind, (const char*)ch.rvk, (const uint32_t*)ch.off, (const uint64_t*)ch.mc, (const char*)dsn, (const char*)(b + o_cm), (const uint32_t*)dcnt,
                       (const uint32_t*)dpos, (const uint8_t*)dkeep, (const uint32_t*)dblk, seg, (uint32_t)owned);
    HIPCHK(hipGetLastError());
    uint32_t* stat = ch.pin->stage;
    HIPCHK(hipMemcpyAsync(stat, dstat, stat_words * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    kept.owned = stat[0]; kept.nf = stat[1];
    for (size_t j = 0; j <= K; ++j) { kept.first[j] = stat[8 + j]; kept.first_f[j] = stat[8 + SCAN_MANY_KEYS + 1 + j]; }
    ch = std::move(kept);
    return ALEO_MI355X_OK;
  }
};

// ---- the host path ------------------------------------------------------------------------------------------------------------------------------------
using Row32 = std::array<uint8_t, 32>;

// named (unspent_named; else null): the commitment of an owned record is computed here, and a record whose commitment is refused is dropped
static int32_t unspent_on_host(Found& R, const char* text, const uint64_t* offsets, size_t n, const uint8_t* commitments, const UnspentKeys& k, size_t j, const std::vector<Row32>& sorted_spent,
                               const CommitCall* named) {
  Found F;
  if (int32_t rc = found_on_host(F, text, offsets, n, k.scan.args[j], k.scan.addr[j])) return rc;
  const serial::SerialTables& T = serial::serial_tables();
  R.unparsed = F.unparsed; R.first_unparsed = F.first_unparsed; R.owned = F.index.size();
  for (size_t q = 0; q < F.index.size(); ++q) {
    Row32 sn, cm;
    if (named) {
      const size_t i = F.index[q];
      if (F.status[q] != FOUND_OK || commit_one_host(cm.data(), text + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), F.plain.data() + 32 * (size_t)F.offsets[q], F.offsets[q + 1] - F.offsets[q], *named)) continue;
    } else std::memcpy(cm.data(), commitments + 32 * (size_t)F.index[q], 32);
    const uint8_t flag = serial::serial_one_host(sn.data(), cm.data(), k.serial[j], T);
    if (F.status[q] != FOUND_OK || flag != 0 || std::binary_search(sorted_spent.begin(), sorted_spent.end(), sn)) continue;
    R.index.push_back(F.index[q]); R.kind.push_back(F.kind[q]); R.status.push_back(0); R.microcredits.push_back(F.microcredits[q]);
    R.rvk.insert(R.rvk.end(), F.rvk.begin() + 32 * q, F.rvk.begin() + 32 * (q + 1));
    R.plain.insert(R.plain.end(), F.plain.begin() + 32 * (size_t)F.offsets[q], F.plain.begin() + 32 * (size_t)F.offsets[q + 1]);
    R.offsets.push_back(R.offsets.back() + (F.offsets[q + 1] - F.offsets[q]));
    R.serials.insert(R.serials.end(), sn.begin(), sn.end());
    if (named) R.commitments.insert(R.commitments.end(), cm.begin(), cm.end());
  }
  return ALEO_MI355X_OK;
}

static int32_t unspent_strings_many(Found** out, const char* text, const uint64_t* offsets, size_t n, const void* commitments32, const void* sk_sigs32, const void* view_keys32,
                                    const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent, bool may_route, const CommitCall* named = nullptr) {
  if (!out) return bad_arg("records_unspent_strings: null result pointer");
  for (size_t j = 0; j < n_keys; ++j) out[j] = nullptr;
  UnspentKeys k; if (int32_t rc = many_keys(k.scan, view_keys32, address_xs32, n_keys)) return rc;
  if (!sk_sigs32 || (!commitments32 && !named)) return bad_arg("records_unspent_strings: null buffer");
  k.serial.resize(n_keys);
  for (size_t j = 0; j < n_keys; ++j)
    if (!serial::serial_key(k.serial[j], (const uint8_t*)sk_sigs32 + 32 * j)) {
      g_last_error = "records_unspent_strings: sk_sig is not a canonical scalar below the subgroup order (key " + std::to_string(j) + ")";
      return ALEO_MI355X_ERR_BAD_ARG;
    }
  if (int32_t rc = strings_args_ok("records_scan_strings", text, offsets, n)) return rc;
  if (n > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 records");
  if (n_spent && !spent32) return bad_arg("records_unspent_strings: null spent set with n_spent > 0");
  if (n_spent > SPENT_MAX_ROWS) return bad_arg("records_unspent_strings: more than 2^30 spent serial numbers");
  std::vector<std::unique_ptr<Found>> R(n_keys);
  for (auto& r : R) { r.reset(new Found); r->filtered = true; r->serials.reserve(32); r->named = named != nullptr; r->commitments.reserve(32); }      // serials.data() is not null, whatever is kept
  int32_t rc = ALEO_MI355X_OK;
  if (!may_route || n * n_keys < aleo_mi355x_min_records() || n == 0) {
    std::vector<Row32> sorted_spent(n_spent);
    if (n_spent) std::memcpy(sorted_spent.data(), spent32, n_spent * 32);
    std::sort(sorted_spent.begin(), sorted_spent.end());
    for (size_t j = 0; j < n_keys && !rc; ++j) rc = unspent_on_host(*R[j], text, offsets, n, (const uint8_t*)commitments32, k, j, sorted_spent, named);
  } else {
    UnspentStage stage((const uint8_t*)commitments32, k, (const uint8_t*)spent32, n_spent, named, text, offsets);      // its host buffers outlive the flow's slot
    rc = found_many_on_device(R, text, offsets, n, k.scan, &stage);
  }
  if (rc) return rc;
  for (size_t j = 0; j < n_keys; ++j) out[j] = R[j].release();
  return ALEO_MI355X_OK;
}

// unspent_named[_many]: the call above without commitments — every owned record's is computed from its string and its decrypted fields under (program id, record name)
static int32_t unspent_named_many(Found** out, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name, const void* sk_sigs32,
                                  const void* view_keys32, const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent, bool may_route) {
  if (!out) return bad_arg("records_unspent_named: null result pointer");
  for (size_t j = 0; j < n_keys; ++j) out[j] = nullptr;
  CommitCall cc; if (int32_t rc = commit_call(cc, program_id, record_name)) return rc;
  return unspent_strings_many(out, text, offsets, n, nullptr, sk_sigs32, view_keys32, address_xs32, n_keys, spent32, n_spent, may_route, &cc);
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

int32_t aleo_mi355x_records_unspent_strings_many(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* commitments32, const void* sk_sigs32,
                                                 const void* view_keys32, const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent) {
  return guarded([&] { return unspent_strings_many(out, text, offsets, n, commitments32, sk_sigs32, view_keys32, address_xs32, n_keys, spent32, n_spent, true); });
}
int32_t aleo_mi355x_records_unspent_strings_many_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* commitments32, const void* sk_sigs32,
                                                      const void* view_keys32, const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent) {
  return guarded([&] { return unspent_strings_many(out, text, offsets, n, commitments32, sk_sigs32, view_keys32, address_xs32, n_keys, spent32, n_spent, false); });
}
int32_t aleo_mi355x_records_unspent_strings(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* commitments32, const void* sk_sig32,
                                            const void* view_key32, const void* address_x32, const void* spent32, size_t n_spent) {
  return guarded([&] { return unspent_strings_many(out, text, offsets, n, commitments32, sk_sig32, view_key32, address_x32, 1, spent32, n_spent, true); });
}
int32_t aleo_mi355x_records_unspent_strings_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* commitments32, const void* sk_sig32,
                                                 const void* view_key32, const void* address_x32, const void* spent32, size_t n_spent) {
  return guarded([&] { return unspent_strings_many(out, text, offsets, n, commitments32, sk_sig32, view_key32, address_x32, 1, spent32, n_spent, false); });
}
int32_t aleo_mi355x_records_unspent_named_many(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name,
                                               const void* sk_sigs32, const void* view_keys32, const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent) {
  return guarded([&] { return unspent_named_many(out, text, offsets, n, program_id, record_name, sk_sigs32, view_keys32, address_xs32, n_keys, spent32, n_spent, true); });
}
int32_t aleo_mi355x_records_unspent_named_many_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name,
                                                    const void* sk_sigs32, const void* view_keys32, const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent) {
  return guarded([&] { return unspent_named_many(out, text, offsets, n, program_id, record_name, sk_sigs32, view_keys32, address_xs32, n_keys, spent32, n_spent, false); });
}
int32_t aleo_mi355x_records_unspent_named(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name, const void* sk_sig32,
                                          const void* view_key32, const void* address_x32, const void* spent32, size_t n_spent) {
  return guarded([&] { return unspent_named_many(out, text, offsets, n, program_id, record_name, sk_sig32, view_key32, address_x32, 1, spent32, n_spent, true); });
}
int32_t aleo_mi355x_records_unspent_named_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name, const void* sk_sig32,
                                               const void* view_key32, const void* address_x32, const void* spent32, size_t n_spent) {
  return guarded([&] { return unspent_named_many(out, text, offsets, n, program_id, record_name, sk_sig32, view_key32, address_x32, 1, spent32, n_spent, false); });
}
const uint8_t* aleo_mi355x_found_commitments(const aleo_mi355x_found* f) { return f && f->named ? f->commitments.data() : nullptr; }
const uint8_t* aleo_mi355x_found_serials(const aleo_mi355x_found* f) { return f && f->filtered ? f->serials.data() : nullptr; }
size_t aleo_mi355x_found_owned(const aleo_mi355x_found* f) { return !f ? 0 : f->filtered ? f->owned : f->index.size(); }

}  // extern "C"
