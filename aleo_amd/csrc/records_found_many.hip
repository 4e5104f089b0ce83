// records_found_many.hip — decrypt_strings for SEVERAL accounts in one call: the records each of K accounts owns among n "record1…" strings, decrypted: per
// account exactly the result of records_found.hip's one-account call (the same aleo_mi355x_found, byte for byte).
//
// The caller is the front end of records_many.hip: the reference's dev server runs find_one_record -> get_unspent_records on every deploy, execute and transfer
// request that brings no fee record (rust/develop/src/routes.rs:112, :143, :194-220; rust/src/api/blocking.rs:229-292), each walking the same blocks, and what
// it needs per account is decrypted records and balances, not flags.  K one-account calls upload and parse the text K times and scan at width 1; one K-key
// scan_strings brings K x n flags, kinds and key rows down and leaves the tail to the host.  Here, per chunk of whole records (cut as scan_many_on_device cuts
// them for K keys):
//   fill                    records_strings.hip, once: the text goes up and is parsed once for all keys
//   k_records_scan_many<W>  records_many.hip, unchanged, at the width it would pick itself; flags and key rows [key][record]; the scan's flags are kept aside
//   resolve                 records_strings.hip, with K keys
//   k_pairs_count           grid (record blocks, keys): records_found_blocks.h's counting block over row blockIdx.y of the flag matrix — the walk of a (key,
//                           record) pair that is owned; its block totals lie at [key][block], so the sums below run in [key][record] order.  Row 0 counts the
//                           strings that do not parse: they are the same for every key
//   k_pairs_offsets         one block: the second level over the K x nb block totals; the totals, and what lies before each key's row (its first rank, its
//                           first field): the per-key totals are their differences
//   — one read of 16 + 8 K bytes; the host sizes the compacted arrays from it, for the owned pairs there are and not for m x K —
//   k_pairs_gather          grid (record blocks, keys): the gathering block; a pair's rank and first field are global, so the compacted arrays hold key 0's
//                           records, then key 1's, each in record order; the key row comes from the scan's [key][record] rows
//   k_records_decrypt       records_decrypt.hip, unchanged, over ALL keys' compacted records in one pass (several launches above the launch cap)
//   k_pairs_microcredits    the status and microcredits lane of records_found_blocks.h
//   — the compacted arrays come down once; the host splits them at the per-key totals into the K results, the chunk's base added to the indices and each
//   result's own field count to its offsets —
// The lanes only call the unchanged walk (records_found_lane.h) through the blocks records_found.hip's kernels call too: what is new is the indexing of rows.
// The host path is K passes of records_found_host.hpp's found_on_host.
#include "records_strings.h"
#include "records_found_blocks.h"
#include "records_found_host.hpp"
#include <memory>

namespace aleo_mi355x {

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------------------
// cnt / pos / pre / flags / scan_flags: [key][record], n per row; blk: [fields | owned][key][block]; stat as k_found_count's, counted by row 0 alone.
__global__ void __launch_bounds__(FOUND_BLOCK) k_pairs_count(uint32_t* __restrict__ cnt, uint32_t* __restrict__ pos, uint8_t* __restrict__ pre, uint32_t* __restrict__ blk, uint32_t* __restrict__ stat,
                                                            const uint8_t* __restrict__ flags, const uint8_t* __restrict__ scan_flags, const int8_t* __restrict__ kinds,
                                                            const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t n) {
  __shared__ uint4 stage[FOUND_LDS_BYTES / 16];
  __shared__ uint32_t wave_tot[2][FOUND_BLOCK / 64];
  const size_t row = (size_t)blockIdx.y * n;
  found_count_block(stage, wave_tot, cnt + row, pos + row, pre + row, blk, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, stat, blockIdx.y == 0, flags + row, scan_flags + row,
                    kinds, text, off, blockIdx.x * FOUND_BLOCK, n);
}

// One block over the rows = n_keys x nb block totals; stat[0], stat[1]: the totals; stat[4 + key], stat[4 + n_keys + key]: the owned pairs and the fields before key's row.
__global__ void __launch_bounds__(FOUND_TOP) k_pairs_offsets(uint32_t* __restrict__ blk, uint32_t* __restrict__ stat, uint32_t rows, uint32_t nb) {
  __shared__ uint32_t wave_tot[2][FOUND_TOP / 64];
  found_offsets_block(wave_tot, blk, stat, rows, nb);
}

// rvk: the scan's rows [key][record]; everything else as k_found_gather's, a pair's rank and first field counted over all keys.
__global__ void __launch_bounds__(FOUND_BLOCK) k_pairs_gather(char* __restrict__ fields, uint32_t* __restrict__ c_index, int8_t* __restrict__ c_kind, char* __restrict__ c_rvk, uint32_t* __restrict__ c_off,
                                                             uint8_t* __restrict__ c_pre, uint64_t* __restrict__ c_mc, uint32_t* __restrict__ c_mc_at, uint32_t* __restrict__ c_mc_n,
                                                             const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ pos, const uint8_t* __restrict__ pre, const uint32_t* __restrict__ blk,
                                                             const uint8_t* __restrict__ flags, const int8_t* __restrict__ kinds, const char* __restrict__ rvk,
                                                             const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t n, uint32_t n_owned, uint32_t n_fields) {
  __shared__ uint4 stage[FOUND_LDS_BYTES / 16];
  const size_t row = (size_t)blockIdx.y * n;
  found_gather_block(stage, fields, c_index, c_kind, c_rvk, c_off, c_pre, c_mc, c_mc_at, c_mc_n, cnt + row, pos + row, pre + row, blk, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y,
                     blockIdx.y == 0, flags + row, kinds, rvk + row * 32, text, off, blockIdx.x * FOUND_BLOCK, n, n_owned, n_fields);
}

__global__ void __launch_bounds__(FOUND_BLOCK) k_pairs_microcredits(uint8_t* __restrict__ c_status, uint64_t* __restrict__ c_mc, char* __restrict__ fields, const uint8_t* __restrict__ c_pre,
                                                                   const uint8_t* __restrict__ c_dec, const uint32_t* __restrict__ c_off, const uint32_t* __restrict__ c_mc_at,
                                                                   const uint32_t* __restrict__ c_mc_n, uint32_t n_owned) {
  const uint32_t j = blockIdx.x * FOUND_BLOCK + threadIdx.x;
  if (j >= n_owned) return;
  found_microcredits_lane(j, c_status, c_mc, fields, c_pre, c_dec, c_off, c_mc_at, c_mc_n);
}

// ---- the device flow ----------------------------------------------------------------------------------------------------------------------------------
static int32_t found_many_on_device(Ctx* c, std::vector<std::unique_ptr<Found>>& R, const char* text, const uint64_t* offsets, size_t n, const ManyKeys& k) {
  const RecordsConsts& C = records_consts();
  const size_t K = k.args.size();
  uint32_t W;
  const size_t chunk = scan_many_plan(n, K, &W);
  StringSource src{text, offsets, nullptr};
  src.cut_chunks(n, chunk);
  std::vector<ScanArgs> table((K + W - 1) / W * W, ScanArgs{});      // the padding: no digits at all
  std::copy(k.args.begin(), k.args.end(), table.begin());
  const size_t M = src.max_records, NB = (M + FOUND_BLOCK - 1) / FOUND_BLOCK, P = M * K;
  hipStream_t s = c->stream;
  int32_t rc;
  if (!c->records_k_ready) {                                   // records.hip's protocol: the flag is set only once the stream has completed the copy
    if ((rc = c->records_k.reserve(RK_WORDS * 4))) return rc;
    HIPCHK(hipMemcpyAsync(c->records_k.p, C.words.data(), RK_WORDS * 4, hipMemcpyHostToDevice, s));
  }
  const size_t stat_words = 4 + 2 * K;
  if ((rc = ensure_host_pinned(c, stat_words * 4))) return rc;
  // the scan's own scratch (64 B per record, 33 B per pair) and 10 B per pair for the walk: the scan's flags, the pre-status, the two first-level sums
  size_t total = 0;
  auto part = [&](size_t bytes) { const size_t at = total; total += (bytes + 31) & ~(size_t)31; return at; };
  const size_t o_keys = part(table.size() * sizeof(ScanArgs)), o_c0 = part(M * 32), o_nx = part(M * 32), o_rvk = part(P * 32), o_fl = part(P), o_scan = part(P), o_pre = part(P), o_cnt = part(P * 4),
               o_pos = part(P * 4), o_blk = part(2 * K * NB * 4), o_stat = part(stat_words * 4), o_str = part(src.scratch_bytes());
  if ((rc = c->scalars_stage.reserve(total))) return rc;
  char* base = c->scalars_stage.as<char>();
  const ScanArgs* dkeys = (const ScanArgs*)(base + o_keys);
  char* dc0 = base + o_c0; char* dnx = base + o_nx; char* drvk = base + o_rvk; char* dstr = base + o_str;
  uint8_t* dfl = (uint8_t*)(base + o_fl); uint8_t* dscan = (uint8_t*)(base + o_scan); uint8_t* dpre = (uint8_t*)(base + o_pre);
  uint32_t* dcnt = (uint32_t*)(base + o_cnt); uint32_t* dpos = (uint32_t*)(base + o_pos); uint32_t* dblk = (uint32_t*)(base + o_blk); uint32_t* dstat = (uint32_t*)(base + o_stat);
  HIPCHK(hipMemcpyAsync(base + o_keys, table.data(), table.size() * sizeof(ScanArgs), hipMemcpyHostToDevice, s));      // `table` outlives the call's last synchronisation
  const uint32_t* dK = c->records_k.as<uint32_t>();
  const uint32_t* dsoff; const int8_t* dkinds; const char* dtext; src.parts(dstr, &dsoff, &dkinds, &dtext);
  const size_t cap = decrypt_chunk_fields();
  const uint32_t* stat = (const uint32_t*)c->h_pinned;
  // the compacted arrays of a chunk on the host, all keys' one after another
  std::vector<uint32_t> h_index, h_off; std::vector<int8_t> h_kind; std::vector<uint8_t> h_rvk, h_status, h_plain; std::vector<uint64_t> h_mc;
  for (auto& r : R) r->first_unparsed = n;
  for (size_t ck = 0; ck + 1 < src.cut.size(); ++ck) {
    const size_t at = src.cut[ck], m = src.cut[ck + 1] - at;
    const uint32_t nb = (uint32_t)((m + FOUND_BLOCK - 1) / FOUND_BLOCK);
    const dim3 pairs(nb, (uint32_t)K);
    if ((rc = src.fill(s, ck, dstr, dc0, dnx))) return rc;
    launch_scan_keys(s, W, dfl, drvk, dc0, dnx, m, dK, dkeys, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dscan, dfl, m * K, hipMemcpyDeviceToDevice, s));      // rows of m: a public owner's status depends on the flag the resolve overwrites
    if ((rc = src.resolve(s, ck, dstr, dfl, drvk, dc0, dkeys, K))) return rc;
    HIPCHK(hipMemsetAsync(dstat, 0, 16, s));
    hipLaunchKernelGGL(k_pairs_count, pairs, dim3(FOUND_BLOCK), 0, s, dcnt, dpos, dpre, dblk, dstat, (const uint8_t*)dfl, (const uint8_t*)dscan, dkinds, dtext, dsoff, (uint32_t)m);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pairs_offsets, dim3(1), dim3(FOUND_TOP), 0, s, dblk, dstat, nb * (uint32_t)K, nb);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_pinned, dstat, stat_words * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                           // the one wait before the gather: the host sizes the compacted arrays
    c->records_k_ready = true;
    const size_t owned = stat[0], nf = stat[1];
    if (stat[2]) for (auto& r : R) { if (!r->unparsed) r->first_unparsed = at + (m - stat[3]); r->unparsed += stat[2]; }
    if (!owned) continue;
    for (size_t j = 0; j < K; ++j) {
      const size_t mine = (j + 1 < K ? stat[4 + j + 1] : owned) - stat[4 + j], mine_f = (j + 1 < K ? stat[4 + K + j + 1] : nf) - stat[4 + K + j];
      if (R[j]->index.size() + mine > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 owned records");
      if ((size_t)R[j]->offsets.back() + mine_f > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 private fields");
    }
    size_t ctotal = 0;
    auto cpart = [&](size_t bytes) { const size_t a = ctotal; ctotal += (bytes + 31) & ~(size_t)31; return a; };
    const size_t o_fields = cpart(nf * 32), o_index = cpart(owned * 4), o_off = cpart((owned + 1) * 4), o_mc_at = cpart(owned * 4), o_mc_n = cpart(owned * 4), o_mc = cpart(owned * 8),
                 o_crvk = cpart(owned * 32), o_kind = cpart(owned), o_cpre = cpart(owned), o_dec = cpart(owned), o_status = cpart(owned);
    if ((rc = c->out_stage.reserve(ctotal))) return rc;
    char* cb = c->out_stage.as<char>();
    char* dfields = cb + o_fields; char* dcrvk = cb + o_crvk;
    uint32_t* dindex = (uint32_t*)(cb + o_index); uint32_t* doff = (uint32_t*)(cb + o_off); uint32_t* dmc_at = (uint32_t*)(cb + o_mc_at); uint32_t* dmc_n = (uint32_t*)(cb + o_mc_n);
    uint64_t* dmc = (uint64_t*)(cb + o_mc); int8_t* dkind = (int8_t*)(cb + o_kind);
    uint8_t* dcpre = (uint8_t*)(cb + o_cpre); uint8_t* ddec = (uint8_t*)(cb + o_dec); uint8_t* dstatus = (uint8_t*)(cb + o_status);
    hipLaunchKernelGGL(k_pairs_gather, pairs, dim3(FOUND_BLOCK), 0, s, dfields, dindex, dkind, dcrvk, doff, dcpre, dmc, dmc_at, dmc_n, (const uint32_t*)dcnt, (const uint32_t*)dpos,
                       (const uint8_t*)dpre, (const uint32_t*)dblk, (const uint8_t*)dfl, dkinds, (const char*)drvk, dtext, dsoff, (uint32_t)m, (uint32_t)owned, (uint32_t)nf);
    HIPCHK(hipGetLastError());
    h_index.resize(owned); h_off.resize(owned + 1); h_kind.resize(owned); h_rvk.resize(owned * 32); h_status.resize(owned); h_mc.resize(owned); h_plain.resize(nf * 32);
    HIPCHK(hipMemcpyAsync(h_off.data(), doff, (owned + 1) * 4, hipMemcpyDeviceToHost, s));
    if (nf <= cap) launch_records_decrypt(s, dfields, ddec, dcrvk, doff, 0, owned, dK);
    else {                                                     // launches of whole records within the cap, one record at least, across key boundaries: the host needs the offsets to cut
      HIPCHK(hipStreamSynchronize(s));
      for (size_t a = 0; a < owned;) {
        size_t e = a + 1;
        while (e < owned && (size_t)h_off[e + 1] - h_off[a] <= cap) ++e;
        launch_records_decrypt(s, dfields, ddec + a, dcrvk + a * 32, doff + a, 0, e - a, dK);
        HIPCHK(hipGetLastError());
        a = e;
      }
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pairs_microcredits, dim3((uint32_t)((owned + FOUND_BLOCK - 1) / FOUND_BLOCK)), dim3(FOUND_BLOCK), 0, s, dstatus, dmc, dfields, (const uint8_t*)dcpre, (const uint8_t*)ddec,
                       (const uint32_t*)doff, (const uint32_t*)dmc_at, (const uint32_t*)dmc_n, (uint32_t)owned);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_index.data(), dindex, owned * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_kind.data(), dkind, owned, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_rvk.data(), dcrvk, owned * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_status.data(), dstatus, owned, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_mc.data(), dmc, owned * 8, hipMemcpyDeviceToHost, s));
    if (nf) HIPCHK(hipMemcpyAsync(h_plain.data(), dfields, nf * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                           // the next chunk reuses the buffers; h_pinned is read below and not written before the next chunk's copy
    for (size_t j = 0; j < K; ++j) {                           // key j's records: the ranks a .. e, the fields fa .. fe
      const size_t a = stat[4 + j], e = j + 1 < K ? stat[4 + j + 1] : owned, fa = stat[4 + K + j], fe = j + 1 < K ? stat[4 + K + j + 1] : nf;
      if (a == e) continue;
      Found& r = *R[j];
      const size_t have = r.index.size(), have_f = r.offsets.back();
      r.index.resize(have + (e - a)); r.offsets.resize(have + (e - a) + 1);
      for (size_t q = a; q < e; ++q) { r.index[have + (q - a)] = h_index[q] + (uint32_t)at; r.offsets[have + (q - a) + 1] = (uint32_t)(have_f + (h_off[q + 1] - fa)); }
      r.kind.insert(r.kind.end(), h_kind.begin() + a, h_kind.begin() + e);
      r.rvk.insert(r.rvk.end(), h_rvk.begin() + a * 32, h_rvk.begin() + e * 32);
      r.status.insert(r.status.end(), h_status.begin() + a, h_status.begin() + e);
      r.microcredits.insert(r.microcredits.end(), h_mc.begin() + a, h_mc.begin() + e);
      r.plain.insert(r.plain.end(), h_plain.begin() + fa * 32, h_plain.begin() + fe * 32);
    }
  }
  return ALEO_MI355X_OK;
}

static int32_t decrypt_strings_many(Found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_keys32, const void* address_xs32, size_t n_keys, bool may_route) {
  if (!out) return bad_arg("records_decrypt_strings_many: null result pointer");
  for (size_t j = 0; j < n_keys; ++j) out[j] = nullptr;
  ManyKeys k; if (int32_t rc = many_keys(k, view_keys32, address_xs32, n_keys)) return rc;
  if (int32_t rc = strings_args_ok("records_scan_strings", text, offsets, n)) return rc;
  if (n > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 records");
  std::vector<std::unique_ptr<Found>> R(n_keys);
  for (auto& r : R) r.reset(new Found);
  int32_t rc = ALEO_MI355X_OK;
  if (!may_route || n * n_keys < aleo_mi355x_min_records() || n == 0)      // in pairs, as records_scan_strings counts
    for (size_t j = 0; j < n_keys && !rc; ++j) rc = found_on_host(*R[j], text, offsets, n, k.args[j], k.addr[j]);
  else { Slot sl; rc = sl.rc ? sl.rc : found_many_on_device(sl.c, R, text, offsets, n, k); }
  if (rc) return rc;
  for (size_t j = 0; j < n_keys; ++j) out[j] = R[j].release();
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

int32_t aleo_mi355x_records_decrypt_strings_many(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_keys32, const void* address_xs32, size_t n_keys) {
  return guarded([&] { return decrypt_strings_many(out, text, offsets, n, view_keys32, address_xs32, n_keys, true); });
}
int32_t aleo_mi355x_records_decrypt_strings_many_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_keys32, const void* address_xs32, size_t n_keys) {
  return guarded([&] { return decrypt_strings_many(out, text, offsets, n, view_keys32, address_xs32, n_keys, false); });
}

}  // extern "C"
