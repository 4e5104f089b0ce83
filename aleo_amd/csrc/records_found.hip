// records_found.hip — decrypt_strings: the records ONE account owns among n "record1…" strings, decrypted, in one call: their indices, record view keys,
// plain private fields and microcredits, and nothing of the records it does not own.
//
// The reference's unspent-record search does this record by record behind the ownership test (rust/src/api/blocking.rs:274-283: `if is_owner {
// record.decrypt(&view_key) … microcredits() }`).  scan_strings (records_strings.hip) stops at "which records"; from there a caller parsed every owned string
// again for its fields, sent them up for records_decrypt_fields and read the microcredits out of the rendered string.  Everything that tail needs is on the
// device when the scan kernel finishes — the symbols in the chunk's text, the record view keys, the flags — so per chunk of the StringSource:
//   fill / scan / resolve   records_strings.hip and records_many.hip, unchanged; the scan's own flags are kept aside (a public owner's flag is overwritten by
//                           the resolve, and whether its nonce was on the curve decides its status when it has private fields)
//   (the bodies of the four k_found_* kernels are records_found_blocks.h's, which records_found_many.hip runs over several accounts' rows)
//   k_found_count           one lane per record (records_found_lane.h): an owned record's number of private fields and whether record_fields would refuse it;
//                           the block's span staged in LDS as k_records_parse stages it (blocks without an owned record skip that); then the first level of the
//                           exclusive sums of the field counts and of the owned bits, within the block
//   k_found_offsets         the second level over the block totals (one block), and the two totals
//   — one 16-byte read: owned records, their fields, unparsed strings and the first of those; the host sizes the field buffer —
//   k_found_gather          the second walk: a lane writes its fields at its offset and its index, kind and key row at its rank among the owned
//   k_records_decrypt       records_decrypt.hip, unchanged, over the compacted records in place; several launches when the fields exceed the launch cap
//   k_found_microcredits    the status of every owned record, zero rows for a malformed one, and the microcredits entry from the plain fields
//   — the compacted arrays come down and are appended, the chunk's base added to indices and offsets —
// The host path puts the existing host calls together (the lane parse and host scan of scan_strings_host, records_plaintext.hpp's structure as record_fields
// reads it, the host decryption); it shares no code with the walk above, which is what the device tests compare it with.
#include "records_strings.h"
#include "records_found_blocks.h"
#include "records_found_host.hpp"

namespace aleo_mi355x {

static constexpr size_t FOUND_CHUNK_RECORDS = (size_t)1 << 20;      // FOUND_TOP lanes cover its 4096 blocks four each

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------------------
// Their bodies are records_found_blocks.h's, over the one row of flags there is here: a block's totals lie at its own index among gridDim.x.
// cnt / pos: the exclusive sums of the field counts and of the owned bits WITHIN the block; blk: [fields | owned][block], the block totals.
// stat: [2] the unparsed strings, [3] n - (the first of them), both through one atomic per wave that holds one; zeroed before the launch.
__global__ void __launch_bounds__(FOUND_BLOCK) k_found_count(uint32_t* __restrict__ cnt, uint32_t* __restrict__ pos, uint8_t* __restrict__ pre, uint32_t* __restrict__ blk, uint32_t* __restrict__ stat,
                                                            const uint8_t* __restrict__ flags, const uint8_t* __restrict__ scan_flags, const int8_t* __restrict__ kinds,
                                                            const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t n) {
  __shared__ uint4 stage[FOUND_LDS_BYTES / 16];
  __shared__ uint32_t wave_tot[2][FOUND_BLOCK / 64];
  found_count_block(stage, wave_tot, cnt, pos, pre, blk, blockIdx.x, gridDim.x, stat, true, flags, scan_flags, kinds, text, off, blockIdx.x * FOUND_BLOCK, n);
}

// One block: blk's two rows of nb block totals become their exclusive sums, the totals go to stat[0] (owned records) and stat[1] (fields).
__global__ void __launch_bounds__(FOUND_TOP) k_found_offsets(uint32_t* __restrict__ blk, uint32_t* __restrict__ stat, uint32_t nb) {
  __shared__ uint32_t wave_tot[2][FOUND_TOP / 64];
  found_offsets_block(wave_tot, blk, stat, nb, 0);
}

// An owned record's rank among the chunk's owned is j = blk[owned row][block] + pos[i], its first field f = blk[fields row][block] + cnt[i].  fields: room for
// n_fields rows; the c_* arrays: n_owned entries (c_off one more: the total).  c_mc: the value of a public microcredits entry, else 0; c_mc_at / c_mc_n: where a
// private one's fields lie among the chunk's fields (n 0: none).
__global__ void __launch_bounds__(FOUND_BLOCK) k_found_gather(char* __restrict__ fields, uint32_t* __restrict__ c_index, int8_t* __restrict__ c_kind, char* __restrict__ c_rvk, uint32_t* __restrict__ c_off,
                                                             uint8_t* __restrict__ c_pre, uint64_t* __restrict__ c_mc, uint32_t* __restrict__ c_mc_at, uint32_t* __restrict__ c_mc_n,
                                                             const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ pos, const uint8_t* __restrict__ pre, const uint32_t* __restrict__ blk,
                                                             const uint8_t* __restrict__ flags, const int8_t* __restrict__ kinds, const char* __restrict__ rvk,
                                                             const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t n, uint32_t n_owned, uint32_t n_fields) {
  __shared__ uint4 stage[FOUND_LDS_BYTES / 16];
  found_gather_block(stage, fields, c_index, c_kind, c_rvk, c_off, c_pre, c_mc, c_mc_at, c_mc_n, cnt, pos, pre, blk, blockIdx.x, gridDim.x, true, flags, kinds, rvk, text, off,
                     blockIdx.x * FOUND_BLOCK, n, n_owned, n_fields);
}

// Behind k_records_decrypt, one lane per owned record: status = what the walk found, else the decryption's flag; the rows of a record the walk marked malformed are
// zeroed (the decryption ran over them with a zero key); microcredits only of a record with status 0.
__global__ void __launch_bounds__(FOUND_BLOCK) k_found_microcredits(uint8_t* __restrict__ c_status, uint64_t* __restrict__ c_mc, char* __restrict__ fields, const uint8_t* __restrict__ c_pre,
                                                                   const uint8_t* __restrict__ c_dec, const uint32_t* __restrict__ c_off, const uint32_t* __restrict__ c_mc_at,
                                                                   const uint32_t* __restrict__ c_mc_n, uint32_t n_owned) {
  const uint32_t j = blockIdx.x * FOUND_BLOCK + threadIdx.x;
  if (j >= n_owned) return;
  found_microcredits_lane(j, c_status, c_mc, fields, c_pre, c_dec, c_off, c_mc_at, c_mc_n);
}

// ---- the device flow ----------------------------------------------------------------------------------------------------------------------------------
static int32_t found_on_device(Ctx* c, Found& R, const char* text, const uint64_t* offsets, size_t n, const ScanArgs& key) {
  const RecordsConsts& C = records_consts();
  StringSource src{text, offsets, nullptr};
  src.cut_chunks(n, FOUND_CHUNK_RECORDS);
  const size_t M = src.max_records, NB = (M + FOUND_BLOCK - 1) / FOUND_BLOCK;
  hipStream_t s = c->stream;
  int32_t rc;
  if (!c->records_k_ready) {                                   // records.hip's protocol: the flag is set only once the stream has completed the copy
    if ((rc = c->records_k.reserve(RK_WORDS * 4))) return rc;
    HIPCHK(hipMemcpyAsync(c->records_k.p, C.words.data(), RK_WORDS * 4, hipMemcpyHostToDevice, s));
  }
  if ((rc = ensure_host_pinned(c, 16))) return rc;
  size_t total = 0;
  auto part = [&](size_t bytes) { const size_t at = total; total += (bytes + 31) & ~(size_t)31; return at; };
  const size_t o_key = part(sizeof(ScanArgs)), o_c0 = part(M * 32), o_nx = part(M * 32), o_rvk = part(M * 32), o_fl = part(M), o_scan = part(M), o_pre = part(M), o_cnt = part(M * 4),
               o_pos = part(M * 4), o_blk = part(2 * NB * 4), o_stat = part(16), o_index = part(M * 4), o_off = part((M + 1) * 4), o_mc_at = part(M * 4), o_mc_n = part(M * 4), o_mc = part(M * 8),
               o_crvk = part(M * 32), o_kind = part(M), o_cpre = part(M), o_dec = part(M), o_status = part(M), o_str = part(src.scratch_bytes());
  if ((rc = c->scalars_stage.reserve(total))) return rc;
  char* base = c->scalars_stage.as<char>();
  const ScanArgs* dkey = (const ScanArgs*)(base + o_key);
  char* dc0 = base + o_c0; char* dnx = base + o_nx; char* drvk = base + o_rvk; char* dstr = base + o_str; char* dcrvk = base + o_crvk;
  uint8_t* dfl = (uint8_t*)(base + o_fl); uint8_t* dscan = (uint8_t*)(base + o_scan); uint8_t* dpre = (uint8_t*)(base + o_pre); uint8_t* dcpre = (uint8_t*)(base + o_cpre);
  uint8_t* ddec = (uint8_t*)(base + o_dec); uint8_t* dstatus = (uint8_t*)(base + o_status); int8_t* dkind = (int8_t*)(base + o_kind);
  uint32_t* dcnt = (uint32_t*)(base + o_cnt); uint32_t* dpos = (uint32_t*)(base + o_pos); uint32_t* dblk = (uint32_t*)(base + o_blk); uint32_t* dstat = (uint32_t*)(base + o_stat);
  uint32_t* dindex = (uint32_t*)(base + o_index); uint32_t* doff = (uint32_t*)(base + o_off); uint32_t* dmc_at = (uint32_t*)(base + o_mc_at); uint32_t* dmc_n = (uint32_t*)(base + o_mc_n);
  uint64_t* dmc = (uint64_t*)(base + o_mc);
  HIPCHK(hipMemcpyAsync(base + o_key, &key, sizeof(ScanArgs), hipMemcpyHostToDevice, s));      // `key` outlives the call's last synchronisation
  const uint32_t* dK = c->records_k.as<uint32_t>();
  const uint32_t* dsoff; const int8_t* dkinds; const char* dtext; src.parts(dstr, &dsoff, &dkinds, &dtext);
  const size_t cap = decrypt_chunk_fields();
  uint32_t* stat = (uint32_t*)c->h_pinned;
  std::vector<uint32_t> cut_off;
  R.first_unparsed = n;
  for (size_t ck = 0; ck + 1 < src.cut.size(); ++ck) {
    const size_t at = src.cut[ck], m = src.cut[ck + 1] - at;
    const uint32_t nb = (uint32_t)((m + FOUND_BLOCK - 1) / FOUND_BLOCK);
    if ((rc = src.fill(s, ck, dstr, dc0, dnx))) return rc;
    launch_scan_one_key(s, dfl, drvk, dc0, dnx, m, dK, dkey);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dscan, dfl, m, hipMemcpyDeviceToDevice, s));
    if ((rc = src.resolve(s, ck, dstr, dfl, drvk, dc0, dkey, 1))) return rc;
    HIPCHK(hipMemsetAsync(dstat, 0, 16, s));
    hipLaunchKernelGGL(k_found_count, dim3(nb), dim3(FOUND_BLOCK), 0, s, dcnt, dpos, dpre, dblk, dstat, (const uint8_t*)dfl, (const uint8_t*)dscan, dkinds, dtext, dsoff, (uint32_t)m);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_found_offsets, dim3(1), dim3(FOUND_TOP), 0, s, dblk, dstat, nb);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(stat, dstat, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                           // the one wait before the gather: the host sizes the field buffer
    c->records_k_ready = true;
    const size_t owned = stat[0], nf = stat[1];
    if (stat[2]) { if (!R.unparsed) R.first_unparsed = at + (m - stat[3]); R.unparsed += stat[2]; }
    if (!owned) continue;
    if (R.index.size() + owned > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 owned records");
    if ((size_t)R.offsets.back() + nf > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 private fields");
    if ((rc = c->out_stage.reserve(nf * 32 + 32))) return rc;
    char* dfields = c->out_stage.as<char>();
    hipLaunchKernelGGL(k_found_gather, dim3(nb), dim3(FOUND_BLOCK), 0, s, dfields, dindex, dkind, dcrvk, doff, dcpre, dmc, dmc_at, dmc_n, (const uint32_t*)dcnt, (const uint32_t*)dpos,
                       (const uint8_t*)dpre, (const uint32_t*)dblk, (const uint8_t*)dfl, dkinds, (const char*)drvk, dtext, dsoff, (uint32_t)m, (uint32_t)owned, (uint32_t)nf);
    HIPCHK(hipGetLastError());
    const size_t have = R.index.size(), have_f = R.offsets.back();
    R.index.resize(have + owned); R.offsets.resize(have + owned + 1); R.kind.resize(have + owned); R.rvk.resize((have + owned) * 32); R.status.resize(have + owned);
    R.microcredits.resize(have + owned); R.plain.resize((have_f + nf) * 32);
    HIPCHK(hipMemcpyAsync(R.offsets.data() + have, doff, (owned + 1) * 4, hipMemcpyDeviceToHost, s));      // chunk-relative until the base is added below
    if (nf <= cap) launch_records_decrypt(s, dfields, ddec, dcrvk, doff, 0, owned, dK);
    else {                                                     // launches of whole records within the cap, one record at least: the host needs the offsets to cut
      HIPCHK(hipStreamSynchronize(s));
      const uint32_t* off = R.offsets.data() + have;
      for (size_t a = 0; a < owned;) {
        size_t e = a + 1;
        while (e < owned && (size_t)off[e + 1] - off[a] <= cap) ++e;
        launch_records_decrypt(s, dfields, ddec + a, dcrvk + a * 32, doff + a, 0, e - a, dK);
        HIPCHK(hipGetLastError());
        a = e;
      }
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_found_microcredits, dim3((uint32_t)((owned + FOUND_BLOCK - 1) / FOUND_BLOCK)), dim3(FOUND_BLOCK), 0, s, dstatus, dmc, dfields, (const uint8_t*)dcpre, (const uint8_t*)ddec,
                       (const uint32_t*)doff, (const uint32_t*)dmc_at, (const uint32_t*)dmc_n, (uint32_t)owned);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(R.index.data() + have, dindex, owned * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(R.kind.data() + have, dkind, owned, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(R.rvk.data() + have * 32, dcrvk, owned * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(R.status.data() + have, dstatus, owned, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(R.microcredits.data() + have, dmc, owned * 8, hipMemcpyDeviceToHost, s));
    if (nf) HIPCHK(hipMemcpyAsync(R.plain.data() + have_f * 32, dfields, nf * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                           // the next chunk reuses the buffers
    for (size_t q = 0; q < owned; ++q) { R.index[have + q] += (uint32_t)at; R.offsets[have + q] += (uint32_t)have_f; }
    R.offsets[have + owned] += (uint32_t)have_f;
  }
  return ALEO_MI355X_OK;
}

static int32_t decrypt_strings(Found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_key32, const void* address_x32, bool may_route) {
  if (!out) return bad_arg("records_decrypt_strings: null result pointer");
  *out = nullptr;
  ManyKeys k; if (int32_t rc = many_keys(k, view_key32, address_x32, 1)) return rc;
  if (int32_t rc = strings_args_ok("records_scan_strings", text, offsets, n)) return rc;
  if (n > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 records");
  Found* R = new Found;
  int32_t rc;
  if (!may_route || n < aleo_mi355x_min_records() || n == 0) rc = found_on_host(*R, text, offsets, n, k.args[0], k.addr[0]);
  else { Slot sl; rc = sl.rc ? sl.rc : found_on_device(sl.c, *R, text, offsets, n, k.args[0]); }
  if (rc) { delete R; return rc; }
  *out = R;
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

int32_t aleo_mi355x_records_decrypt_strings(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_key32, const void* address_x32) {
  return guarded([&] { return decrypt_strings(out, text, offsets, n, view_key32, address_x32, true); });
}
int32_t aleo_mi355x_records_decrypt_strings_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_key32, const void* address_x32) {
  return guarded([&] { return decrypt_strings(out, text, offsets, n, view_key32, address_x32, false); });
}
void aleo_mi355x_found_free(aleo_mi355x_found* f) { delete f; }
size_t aleo_mi355x_found_count(const aleo_mi355x_found* f) { return f ? f->index.size() : 0; }
const uint32_t* aleo_mi355x_found_index(const aleo_mi355x_found* f) { return f ? f->index.data() : nullptr; }
const int8_t* aleo_mi355x_found_kind(const aleo_mi355x_found* f) { return f ? f->kind.data() : nullptr; }
const uint8_t* aleo_mi355x_found_rvk(const aleo_mi355x_found* f) { return f ? f->rvk.data() : nullptr; }
const uint32_t* aleo_mi355x_found_offsets(const aleo_mi355x_found* f) { return f ? f->offsets.data() : nullptr; }
size_t aleo_mi355x_found_fields(const aleo_mi355x_found* f) { return f ? f->offsets.back() : 0; }
const uint8_t* aleo_mi355x_found_plain(const aleo_mi355x_found* f) { return f ? f->plain.data() : nullptr; }
const uint8_t* aleo_mi355x_found_status(const aleo_mi355x_found* f) { return f ? f->status.data() : nullptr; }
const uint64_t* aleo_mi355x_found_microcredits(const aleo_mi355x_found* f) { return f ? f->microcredits.data() : nullptr; }
size_t aleo_mi355x_found_unparsed(const aleo_mi355x_found* f) { return f ? f->unparsed : 0; }
size_t aleo_mi355x_found_first_unparsed(const aleo_mi355x_found* f) { return f ? f->first_unparsed : 0; }

}  // extern "C"
