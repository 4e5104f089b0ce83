// records_found.hip — decrypt_strings and decrypt_strings_many: the records each of K accounts owns among n "record1…" strings, decrypted, in one call: per
// account their indices, record view keys, plain private fields and microcredits, and nothing of the records it does not own.  The one-account call is K = 1.
//
// The reference's unspent-record search does this record by record behind the ownership test (rust/src/api/blocking.rs:274-283: `if is_owner {
// record.decrypt(&view_key) … microcredits() }`), and its dev server runs find_one_record -> get_unspent_records on every deploy, execute and transfer request
// that brings no fee record (rust/develop/src/routes.rs:112, :143, :194-220; rust/src/api/blocking.rs:229-292), each walking the same blocks.  scan_strings
// (records_strings.hip) stops at "which records"; from there a caller parsed every owned string again for its fields, sent them up for records_decrypt_fields
// and read the microcredits out of the rendered string, and K one-account calls upload and parse the text K times and scan at width 1.  Everything that tail
// needs is on the device when the scan kernel finishes — the symbols in the chunk's text, the record view keys, the flags — so per chunk of whole records (cut
// as scan_many_on_device cuts them for K keys):
//   fill                    records_strings.hip, once: the text goes up and is parsed once for all keys
//   k_records_scan_many<W>  records_many.hip, unchanged, at the width it would pick itself; flags and key rows [key][record]; the scan's own flags are kept aside
//                           (a public owner's flag is overwritten by the resolve, and whether its nonce was on the curve decides its status when it has
//                           private fields)
//   resolve                 records_strings.hip, with K keys
//   k_found_count           grid (record blocks, keys), one lane per (key, record) pair (records_found_lane.h): an owned pair's number of private fields and
//                           whether record_fields would refuse it; the block's span staged in LDS by the stage_span of k_records_parse (blocks without an owned pair
//                           skip that); then the first level of the exclusive sums of the field counts and of the owned bits, within the block.  Its block
//                           totals lie at [key][block], so the sums below run in [key][record] order.  Row 0 counts the strings that do not parse: they are
//                           the same for every key
//   k_found_offsets         one block: the second level over the K x nb block totals; the totals, and what lies before each key's row (its first rank, its
//                           first field): the per-key totals are their differences
//   — one read of 16 + 8 K bytes; the host sizes the compacted arrays from it, for the owned pairs there are and not for m x K —
//   k_found_gather          the same grid, the second walk: a lane writes its fields at its offset and its index, kind and key row at its rank among the
//                           owned; a pair's rank and first field are global, so the compacted arrays hold key 0's records, then key 1's, each in record order
//   k_records_decrypt       records_decrypt.hip, unchanged, over ALL keys' compacted records in place; several launches when the fields exceed the launch cap
//   k_found_microcredits    the status of every owned pair, zero rows for a malformed one, and the microcredits entry from the plain fields
//   — the compacted arrays come down once; the host splits them at the per-key totals into the K results, the chunk's base added to the indices and each
//   result's own field count to its offsets —
// The host path is K passes of records_found_host.hpp's found_on_host, which puts the existing host calls together (the lane parse and host scan of
// scan_strings_host, records_plaintext.hpp's structure as record_fields reads it, the host decryption); it shares no code with the walk above, which is what
// the device tests compare it with.
// records_unspent_strings[_many] (records_unspent.hip) is this flow with one more stage (records_found.h FoundStage) between k_found_microcredits and the
// downloads: what comes down is then what the stage kept.
#include "records_found.h"

namespace aleo_mi355x {

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------------------
// A block is (blockIdx.x, key blockIdx.y): the records b0 .. b0 + 256 of row `key` of the [key][record] matrices (n per row); its totals lie at bi among the
// gridDim.x x gridDim.y of all blocks.
//
// The counting walk.  cnt / pos: the exclusive sums of the field counts and of the owned bits WITHIN the block; blk: [fields | owned][key][block], the block
// totals.  stat: [2] the unparsed strings, [3] n - (the first of them), both through one atomic per wave that holds one, zeroed before the launch — counted by
// row 0 alone (the strings are the same for every row).
__global__ void __launch_bounds__(FOUND_BLOCK) k_found_count(uint32_t* __restrict__ cnt, uint32_t* __restrict__ pos, uint8_t* __restrict__ pre, uint32_t* __restrict__ blk, uint32_t* __restrict__ stat,
                                                            const uint8_t* __restrict__ flags, const uint8_t* __restrict__ scan_flags, const int8_t* __restrict__ kinds,
                                                            const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t n) {
  __shared__ uint4 stage[SPAN_LDS_BYTES / 16];
  __shared__ uint32_t wave_tot[2][FOUND_BLOCK / 64];
  const size_t row = (size_t)blockIdx.y * n;
  const uint32_t bi = blockIdx.y * gridDim.x + blockIdx.x, rows = gridDim.x * gridDim.y, b0 = blockIdx.x * FOUND_BLOCK;
  cnt += row; pos += row; pre += row; flags += row; scan_flags += row;
  const uint32_t i = b0 + threadIdx.x;
  const bool live = i < n;
  const int32_t kind = live ? kinds[i] : 0;
  const bool owned = live && flags[i] == 1;
  if (blockIdx.y == 0) {                                       // uniform
    const unsigned long long refused = __ballot(live && kind < 0);
    if (refused && (threadIdx.x & 63u) == 0) {
      atomicAdd(&stat[2], (uint32_t)__popcll(refused));
      atomicMax(&stat[3], n - (i + (uint32_t)__ffsll(refused) - 1u));
    }
  }
  uint32_t m = 0, status = FOUND_OK;
  if (__syncthreads_or(owned)) {                               // uniform
    uint32_t lo;
    const bool staged = stage_span(stage, text, off, b0, n, &lo);
    if (owned) {
      const uint32_t first = off[i], len = off[i + 1] - first;
      auto nothing = [](uint32_t, const uint32_t (&)[8]) {};
      FoundWalk w;
      if (staged) { const uint8_t* mine = (const uint8_t*)stage + (first - lo); w = records_found_walk([&](uint32_t j) { return mine[j]; }, len, kind, nothing); }
      else { const uint8_t* __restrict__ mine = (const uint8_t*)text + first; w = records_found_walk([&](uint32_t j) { return mine[j]; }, len, kind, nothing); }
      m = w.fields; status = w.status;
      if (kind == 0 && m && scan_flags[i] == 2) status = FOUND_MALFORMED;
    }
  }
  if (live) pre[i] = (uint8_t)status;
  uint32_t a = m, b = owned ? 1u : 0u, ta, tb;
  block_exclusive2(a, b, wave_tot, &ta, &tb);
  if (live) { cnt[i] = a; pos[i] = b; }
  if (threadIdx.x == 0) { blk[bi] = ta; blk[rows + bi] = tb; }
}

// One block of FOUND_TOP lanes over the rows = n_keys x nb block totals: blk's two rows of them become their exclusive sums, the totals go to stat[0] (owned
// pairs) and stat[1] (fields), and what lies before each key's row — its two sums at its first block — to stat[4 + key] (owned) and stat[4 + n_keys + key] (fields).
__global__ void __launch_bounds__(FOUND_TOP) k_found_offsets(uint32_t* __restrict__ blk, uint32_t* __restrict__ stat, uint32_t rows, uint32_t nb) {
  __shared__ uint32_t wave_tot[2][FOUND_TOP / 64];
  const uint32_t per = (rows + FOUND_TOP - 1) / FOUND_TOP, first = threadIdx.x * per, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t* f = blk; uint32_t* o = blk + rows;
  uint32_t sf = 0, so = 0;
  for (uint32_t k = first; k < first + per && k < rows; ++k) { sf += f[k]; so += o[k]; }
  uint32_t af = sf, ao = so;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t uf = __shfl_up(af, d, 64), uo = __shfl_up(ao, d, 64);
    if (lane >= (uint32_t)d) { af += uf; ao += uo; }
  }
  if (lane == 63) { wave_tot[0][wave] = af; wave_tot[1][wave] = ao; }
  __syncthreads();
  uint32_t bf = 0, bo = 0, tf = 0, to = 0;
  for (uint32_t w = 0; w < FOUND_TOP / 64; ++w) { if (w < wave) { bf += wave_tot[0][w]; bo += wave_tot[1][w]; } tf += wave_tot[0][w]; to += wave_tot[1][w]; }
  uint32_t rf = bf + af - sf, ro = bo + ao - so;
  for (uint32_t k = first; k < first + per && k < rows; ++k) {
    const uint32_t vf = f[k], vo = o[k]; f[k] = rf; o[k] = ro;
    if (k % nb == 0) { stat[4 + k / nb] = ro; stat[4 + rows / nb + k / nb] = rf; }
    rf += vf; ro += vo;
  }
  if (threadIdx.x == 0) { stat[0] = to; stat[1] = tf; }
}

// The gathering walk.  An owned pair's rank among ALL rows' owned is j = blk[owned row][bi] + pos[i], its first field f = blk[fields row][bi] + cnt[i].  fields:
// room for n_fields rows; the c_* arrays: n_owned entries (c_off one more: the total, written by row 0).  rvk: the scan's rows [key][record].  c_mc: the value of
// a public microcredits entry, else 0; c_mc_at / c_mc_n: where a private one's fields lie among the gathered fields (n 0: none).
__global__ void __launch_bounds__(FOUND_BLOCK) k_found_gather(char* __restrict__ fields, uint32_t* __restrict__ c_index, int8_t* __restrict__ c_kind, char* __restrict__ c_rvk, uint32_t* __restrict__ c_off,
                                                             uint8_t* __restrict__ c_pre, uint64_t* __restrict__ c_mc, uint32_t* __restrict__ c_mc_at, uint32_t* __restrict__ c_mc_n,
                                                             const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ pos, const uint8_t* __restrict__ pre, const uint32_t* __restrict__ blk,
                                                             const uint8_t* __restrict__ flags, const int8_t* __restrict__ kinds, const char* __restrict__ rvk,
                                                             const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t n, uint32_t n_owned, uint32_t n_fields) {
  __shared__ uint4 stage[SPAN_LDS_BYTES / 16];
  const size_t row = (size_t)blockIdx.y * n;
  const uint32_t bi = blockIdx.y * gridDim.x + blockIdx.x, rows = gridDim.x * gridDim.y, b0 = blockIdx.x * FOUND_BLOCK;
  cnt += row; pos += row; pre += row; flags += row; rvk += row * 32;
  const uint32_t i = b0 + threadIdx.x;
  if (blockIdx.y == 0 && i == 0) c_off[n_owned] = n_fields;
  const bool owned = i < n && flags[i] == 1;
  if (!__syncthreads_or(owned)) return;                        // uniform
  uint32_t lo;
  const bool staged = stage_span(stage, text, off, b0, n, &lo);
  if (!owned) return;                                          // no barrier below
  const uint32_t j = blk[rows + bi] + pos[i], f = blk[bi] + cnt[i];
  if (j >= n_owned) return;                                    // cannot happen: the totals are these sums
  const int32_t kind = kinds[i];
  const uint32_t status = pre[i];
  c_index[j] = i; c_kind[j] = (int8_t)kind; c_off[j] = f; c_pre[j] = (uint8_t)status;
  const uint4* r = (const uint4*)(rvk + (size_t)i * 32); uint4* ro = (uint4*)(c_rvk + (size_t)j * 32);
  ro[0] = r[0]; ro[1] = r[1];
  FoundWalk w{0, status, FOUND_MC_NONE, 0, 0, 0};
  if (status != FOUND_REFUSED) {
    const uint32_t first_char = off[i], len = off[i + 1] - first_char;
    auto store = [&](uint32_t k, const uint32_t (&v)[8]) {
      if (f + k >= n_fields) return;                           // cannot happen: the count walk counted them
      uint4* o = (uint4*)(fields + (size_t)(f + k) * 32);
      o[0] = make_uint4(v[0], v[1], v[2], v[3]); o[1] = make_uint4(v[4], v[5], v[6], v[7]);
    };
    if (staged) { const uint8_t* mine = (const uint8_t*)stage + (first_char - lo); w = records_found_walk([&](uint32_t q) { return mine[q]; }, len, kind, store); }
    else { const uint8_t* __restrict__ mine = (const uint8_t*)text + first_char; w = records_found_walk([&](uint32_t q) { return mine[q]; }, len, kind, store); }
  }
  c_mc[j] = w.mc_kind == FOUND_MC_PUBLIC ? w.mc_value : 0;
  c_mc_at[j] = w.mc_kind == FOUND_MC_PRIVATE ? f + w.mc_at : 0;
  c_mc_n[j] = w.mc_kind == FOUND_MC_PRIVATE ? w.mc_n : 0;
}

// Behind k_records_decrypt, one lane per owned record: status = what the walk found, else the decryption's flag; the rows of a record the walk marked malformed are
// zeroed (the decryption ran over them with a zero key); microcredits only of a record with status 0.
__global__ void __launch_bounds__(FOUND_BLOCK) k_found_microcredits(uint8_t* __restrict__ c_status, uint64_t* __restrict__ c_mc, char* __restrict__ fields, const uint8_t* __restrict__ c_pre,
                                                                   const uint8_t* __restrict__ c_dec, const uint32_t* __restrict__ c_off, const uint32_t* __restrict__ c_mc_at,
                                                                   const uint32_t* __restrict__ c_mc_n, uint32_t n_owned) {
  const uint32_t j = blockIdx.x * FOUND_BLOCK + threadIdx.x;
  if (j >= n_owned) return;
  const uint32_t pre = c_pre[j], status = pre ? pre : c_dec[j];
  c_status[j] = (uint8_t)status;
  if (pre == FOUND_MALFORMED)
    for (uint32_t k = c_off[j]; k < c_off[j + 1]; ++k) { uint4* o = (uint4*)(fields + (size_t)k * 32); o[0] = make_uint4(0, 0, 0, 0); o[1] = make_uint4(0, 0, 0, 0); }
  if (status != FOUND_OK) { c_mc[j] = 0; return; }
  const uint32_t mn = c_mc_n[j];
  if (!mn) return;                                             // a public entry's value, or 0, stands
  const char* at = fields + (size_t)c_mc_at[j] * 32;
  c_mc[j] = found_microcredits_private(mn, [&](uint32_t k, uint32_t (&w)[8]) { load_words8(w, at + (size_t)k * 32); });
}

void launch_found_offsets(hipStream_t s, uint32_t* blk, uint32_t* stat, uint32_t rows, uint32_t nb) {
  hipLaunchKernelGGL(k_found_offsets, dim3(1), dim3(FOUND_TOP), 0, s, blk, stat, rows, nb);
}

// ---- the device flow ----------------------------------------------------------------------------------------------------------------------------------
// What one call holds on the device, in the slot's scalars_stage: the scan's own scratch (64 B per record, 33 B per pair), 10 B per pair for the walk (the scan's
// flags, the pre-status, the two first-level sums), the block totals, the statistics (read through pin->flow) and the source's scratch.
struct FoundCall {
  Ctx* c; hipStream_t s; FoundPinned* pin; FoundStage* stage; size_t K, cap, stat_words; uint32_t W;      // cap: the fields of one decryption launch
  const uint32_t* dK; const ScanArgs* dkeys;
  char* dc0; char* dnx; char* drvk; char* dstr; uint8_t* dfl; uint8_t* dscan; uint8_t* dpre; uint32_t* dcnt; uint32_t* dpos; uint32_t* dblk; uint32_t* dstat;
  uint32_t* dsoff; int8_t* dkinds; char* dtext;
};

// `to` sized for records / fields in all, what it held before included
static void found_size(Found& to, size_t records, size_t fields, bool serials, bool commitments = false) {
  to.index.resize(records); to.offsets.resize(records + 1); to.kind.resize(records); to.rvk.resize(records * 32); to.status.resize(records);
  to.microcredits.resize(records); to.plain.resize(fields * 32);
  if (serials) to.serials.resize(records * 32);
  if (commitments) to.commitments.resize(records * 32);
}

// Chunk ck up to the one wait before the gather: parse, scan, resolve, the counting walk and its sums; the unparsed strings into every result; into `ch` the totals
// and the keys' boundaries (key j: the ranks first[j] .. first[j + 1], the fields first_f[j] .. first_f[j + 1]), from which the host sizes what follows.  ch.owned 0: done.
static int32_t found_count(const FoundCall& f, StringSource& src, size_t ck, std::vector<std::unique_ptr<Found>>& R, FoundChunk& ch) {
  const size_t K = f.K, at = src.cut[ck], m = src.cut[ck + 1] - at;
  const uint32_t nb = (uint32_t)((m + FOUND_BLOCK - 1) / FOUND_BLOCK);
  hipStream_t s = f.s;
  if (int32_t rc = src.fill(s, ck, f.dstr, f.dc0, f.dnx)) return rc;
  launch_scan_keys(s, f.W, f.dfl, f.drvk, f.dc0, f.dnx, m, f.dK, f.dkeys, K);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(f.dscan, f.dfl, m * K, hipMemcpyDeviceToDevice, s));      // rows of m: a public owner's status depends on the flag the resolve overwrites
  if (int32_t rc = src.resolve(s, ck, f.dstr, f.dfl, f.drvk, f.dc0, f.dkeys, K)) return rc;
  HIPCHK(hipMemsetAsync(f.dstat, 0, 16, s));
  hipLaunchKernelGGL(k_found_count, dim3(nb, (uint32_t)K), dim3(FOUND_BLOCK), 0, s, f.dcnt, f.dpos, f.dpre, f.dblk, f.dstat, (const uint8_t*)f.dfl, (const uint8_t*)f.dscan, (const int8_t*)f.dkinds,
                     (const char*)f.dtext, (const uint32_t*)f.dsoff, (uint32_t)m);
  HIPCHK(hipGetLastError());
  launch_found_offsets(s, f.dblk, f.dstat, nb * (uint32_t)K, nb);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(f.pin->flow, f.dstat, f.stat_words * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));                           // the one wait before the gather: the host sizes the compacted arrays
  const uint32_t* stat = f.pin->flow;
  const size_t owned = stat[0], nf = stat[1];
  if (stat[2]) for (auto& r : R) { if (!r->unparsed) r->first_unparsed = at + (m - stat[3]); r->unparsed += stat[2]; }
  ch.pin = f.pin; ch.at = at; ch.owned = owned; ch.nf = nf; ch.first.assign(K + 1, 0); ch.first_f.assign(K + 1, 0);
  if (!owned) return ALEO_MI355X_OK;
  for (size_t j = 0; j < K; ++j) { ch.first[j] = stat[4 + j]; ch.first_f[j] = stat[4 + K + j]; }      // a stage moves these boundaries
  ch.first[K] = (uint32_t)owned; ch.first_f[K] = (uint32_t)nf;
  for (size_t j = 0; j < K; ++j) {
    const size_t mine = ch.first[j + 1] - ch.first[j], mine_f = ch.first_f[j + 1] - ch.first_f[j];
    R[j]->owned += mine;
    if (R[j]->index.size() + mine > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 owned records");
    if ((size_t)R[j]->offsets.back() + mine_f > UINT32_MAX) return bad_arg("records_decrypt_strings: more than 2^32 - 1 private fields");
  }
  return ALEO_MI355X_OK;
}

// The chunk's m records behind the count: the compacted arrays in the slot's out_stage (`ch` gets their pointers), the gathering walk, the decryption over all keys'
// records in place and k_found_microcredits.  Without a stage everything owned comes down, so `to` is sized here, behind put records and put_f fields, and the offsets
// come down first; with one the result is sized later, for what it keeps, and the unfiltered offsets, which only the cut of the decryption's launches reads, go aside.
static int32_t found_gather_decrypt(const FoundCall& f, size_t m, FoundChunk& ch, Found& to, size_t put, size_t put_f) {
  const size_t owned = ch.owned, nf = ch.nf;
  hipStream_t s = f.s;
  Carve cv;
  const size_t o_fields = cv.part(nf * 32), o_index = cv.part(owned * 4), o_off = cv.part((owned + 1) * 4), o_mc_at = cv.part(owned * 4), o_mc_n = cv.part(owned * 4), o_mc = cv.part(owned * 8),
               o_crvk = cv.part(owned * 32), o_kind = cv.part(owned), o_cpre = cv.part(owned), o_dec = cv.part(owned), o_status = cv.part(owned);
  if (int32_t rc = f.c->out_stage.reserve(cv.total)) return rc;
  char* cb = f.c->out_stage.as<char>();
  uint32_t* dmc_at = (uint32_t*)(cb + o_mc_at); uint32_t* dmc_n = (uint32_t*)(cb + o_mc_n); uint8_t* dcpre = (uint8_t*)(cb + o_cpre); uint8_t* ddec = (uint8_t*)(cb + o_dec);
  ch.fields = cb + o_fields; ch.index = (uint32_t*)(cb + o_index); ch.kind = (int8_t*)(cb + o_kind); ch.rvk = cb + o_crvk; ch.off = (uint32_t*)(cb + o_off); ch.mc = (uint64_t*)(cb + o_mc);
  ch.status = (uint8_t*)(cb + o_status); ch.text = f.dtext; ch.soff = f.dsoff;
  hipLaunchKernelGGL(k_found_gather, dim3((uint32_t)((m + FOUND_BLOCK - 1) / FOUND_BLOCK), (uint32_t)f.K), dim3(FOUND_BLOCK), 0, s, ch.fields, ch.index, ch.kind, ch.rvk, ch.off, dcpre, ch.mc, dmc_at,
                     dmc_n, (const uint32_t*)f.dcnt, (const uint32_t*)f.dpos, (const uint8_t*)f.dpre, (const uint32_t*)f.dblk, (const uint8_t*)f.dfl, (const int8_t*)f.dkinds, (const char*)f.drvk, (const char*)f.dtext, (const uint32_t*)f.dsoff,
                     (uint32_t)m, (uint32_t)owned, (uint32_t)nf);
  HIPCHK(hipGetLastError());
  if (f.stage) { if (int32_t rc = f.stage->gathered(f.c, s, ch)) return rc; }
  std::vector<uint32_t> off_aside;
  if (f.stage) off_aside.resize(nf > f.cap ? owned + 1 : 0); else found_size(to, put + owned, put_f + nf, false);
  uint32_t* h_off = f.stage ? off_aside.data() : to.offsets.data() + put;      // chunk-relative until found_download adds a base
  if (!f.stage || nf > f.cap) HIPCHK(hipMemcpyAsync(h_off, ch.off, (owned + 1) * 4, hipMemcpyDeviceToHost, s));
  if (nf <= f.cap) launch_records_decrypt(s, ch.fields, ddec, ch.rvk, ch.off, 0, owned, f.dK);
  else {                                                     // launches of whole records within the cap, across key boundaries: the host needs the offsets to cut
    HIPCHK(hipStreamSynchronize(s));
    for (size_t a = 0, e; a < owned; a = e) {
      e = decrypt_cut(h_off, a, owned, owned, f.cap);
      launch_records_decrypt(s, ch.fields, ddec + a, ch.rvk + a * 32, ch.off + a, 0, e - a, f.dK);
    }
  }
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_found_microcredits, dim3((uint32_t)((owned + FOUND_BLOCK - 1) / FOUND_BLOCK)), dim3(FOUND_BLOCK), 0, s, ch.status, ch.mc, ch.fields, (const uint8_t*)dcpre, (const uint8_t*)ddec,
                     (const uint32_t*)ch.off, (const uint32_t*)dmc_at, (const uint32_t*)dmc_n, (uint32_t)owned);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

// What `ch` holds — everything owned, or what the stage kept — comes down into `to` behind put records and put_f fields, and is split: with one key it lies in
// its result's tail already and the split is the two bases; with several, `to` is the staging of this chunk and key j's part is appended to R[j].
static int32_t found_download(const FoundCall& f, const FoundChunk& ch, Found& to, size_t put, size_t put_f, std::vector<std::unique_ptr<Found>>& R) {
  const size_t K = f.K, at = ch.at, got = ch.owned, got_f = ch.nf;
  hipStream_t s = f.s;
  if (f.stage) found_size(to, put + got, put_f + got_f, true, ch.commitments != nullptr);
  uint32_t* h_off = to.offsets.data() + put;                 // chunk-relative until a base is added below
  if (f.stage) HIPCHK(hipMemcpyAsync(h_off, ch.off, (got + 1) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(to.index.data() + put, ch.index, got * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(to.kind.data() + put, ch.kind, got, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(to.rvk.data() + put * 32, ch.rvk, got * 32, hipMemcpyDeviceToHost, s));
  if (ch.status) HIPCHK(hipMemcpyAsync(to.status.data() + put, ch.status, got, hipMemcpyDeviceToHost, s));      // else zeros, as the resize left them
  HIPCHK(hipMemcpyAsync(to.microcredits.data() + put, ch.mc, got * 8, hipMemcpyDeviceToHost, s));
  if (ch.serials) HIPCHK(hipMemcpyAsync(to.serials.data() + put * 32, ch.serials, got * 32, hipMemcpyDeviceToHost, s));
  if (ch.commitments) HIPCHK(hipMemcpyAsync(to.commitments.data() + put * 32, ch.commitments, got * 32, hipMemcpyDeviceToHost, s));
  if (got_f) HIPCHK(hipMemcpyAsync(to.plain.data() + put_f * 32, ch.fields, got_f * 32, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));                           // the next chunk reuses the buffers
  if (K == 1) {
    for (size_t q = 0; q < got; ++q) { to.index[put + q] += (uint32_t)at; h_off[q] += (uint32_t)put_f; }
    h_off[got] += (uint32_t)put_f;
  } else for (size_t j = 0; j < K; ++j) {                    // key j's records: the ranks a .. e, the fields fa .. fe
    const size_t a = ch.first[j], e = ch.first[j + 1], fa = ch.first_f[j], fe = ch.first_f[j + 1];
    if (a == e) continue;
    Found& r = *R[j];
    const size_t have = r.index.size(), have_f = r.offsets.back();
    r.index.resize(have + (e - a)); r.offsets.resize(have + (e - a) + 1);
    for (size_t q = a; q < e; ++q) { r.index[have + (q - a)] = to.index[q] + (uint32_t)at; r.offsets[have + (q - a) + 1] = (uint32_t)(have_f + (h_off[q + 1] - fa)); }
    r.kind.insert(r.kind.end(), to.kind.begin() + a, to.kind.begin() + e);
    r.rvk.insert(r.rvk.end(), to.rvk.begin() + a * 32, to.rvk.begin() + e * 32);
    r.status.insert(r.status.end(), to.status.begin() + a, to.status.begin() + e);
    r.microcredits.insert(r.microcredits.end(), to.microcredits.begin() + a, to.microcredits.begin() + e);
    r.plain.insert(r.plain.end(), to.plain.begin() + fa * 32, to.plain.begin() + fe * 32);
    if (f.stage) r.serials.insert(r.serials.end(), to.serials.begin() + a * 32, to.serials.begin() + e * 32);
    if (ch.commitments) r.commitments.insert(r.commitments.end(), to.commitments.begin() + a * 32, to.commitments.begin() + e * 32);
  }
  return ALEO_MI355X_OK;
}

int32_t found_many_on_device(std::vector<std::unique_ptr<Found>>& R, const char* text, const uint64_t* offsets, size_t n, const ManyKeys& k, FoundStage* stage) {
  FoundCall f{}; f.stage = stage; f.K = k.args.size(); f.cap = env_cap("ALEO_MI355X_DECRYPT_CHUNK_FIELDS", DECRYPT_CHUNK_FIELDS); f.stat_words = 4 + 2 * f.K;
  // The host ends of the flow's copies are declared outside the slot, as R and the stage are: the key table, the source's offsets, and where a chunk's compacted
  // arrays come down, all keys' one after another: staging arrays that are split into the K results — or, when there is one key and everything is its own, the
  // tail of its result, which saves a host copy of everything owned (120 MB at 2^20 records all owned).
  std::vector<ScanArgs> table; StringSource src{text, offsets, nullptr}; Found staged;
  Found& to = f.K == 1 ? *R[0] : staged;
  return on_slot([&](Ctx* c) -> int32_t {
    f.c = c; f.s = c->stream;
    int32_t rc;
    if (stage && (rc = stage->begin(c, f.s))) return rc;      // its uploads run while the host cuts the chunks
    const size_t K = f.K, chunk = scan_many_plan(n, k, &f.W, &table);
    src.cut_chunks(n, chunk);
    const size_t M = src.max_records, NB = (M + FOUND_BLOCK - 1) / FOUND_BLOCK, P = M * K;
    if ((rc = records_constants(c, &f.dK))) return rc;
    if ((rc = found_pinned(c, &f.pin))) return rc;
    Carve cv;
    const size_t o_keys = cv.part(table.size() * sizeof(ScanArgs)), o_c0 = cv.part(M * 32), o_nx = cv.part(M * 32), o_rvk = cv.part(P * 32), o_fl = cv.part(P), o_scan = cv.part(P), o_pre = cv.part(P),
                 o_cnt = cv.part(P * 4), o_pos = cv.part(P * 4), o_blk = cv.part(2 * K * NB * 4), o_stat = cv.part(f.stat_words * 4), o_str = cv.part(src.scratch_bytes());
    if ((rc = c->scalars_stage.reserve(cv.total))) return rc;
    char* base = c->scalars_stage.as<char>();
    f.dkeys = (const ScanArgs*)(base + o_keys); f.dc0 = base + o_c0; f.dnx = base + o_nx; f.drvk = base + o_rvk; f.dstr = base + o_str;
    f.dfl = (uint8_t*)(base + o_fl); f.dscan = (uint8_t*)(base + o_scan); f.dpre = (uint8_t*)(base + o_pre);
    f.dcnt = (uint32_t*)(base + o_cnt); f.dpos = (uint32_t*)(base + o_pos); f.dblk = (uint32_t*)(base + o_blk); f.dstat = (uint32_t*)(base + o_stat);
    HIPCHK(hipMemcpyAsync(base + o_keys, table.data(), table.size() * sizeof(ScanArgs), hipMemcpyHostToDevice, f.s));
    src.parts(f.dstr, &f.dsoff, &f.dkinds, &f.dtext);
    for (auto& r : R) r->first_unparsed = n;
    for (size_t ck = 0; ck + 1 < src.cut.size(); ++ck) {
      FoundChunk ch;
      if ((rc = found_count(f, src, ck, R, ch))) return rc;
      if (!ch.owned) continue;
      const size_t put = K == 1 ? to.index.size() : 0, put_f = K == 1 ? to.offsets.back() : 0;      // `staged` starts over with every chunk
      if ((rc = found_gather_decrypt(f, src.cut[ck + 1] - src.cut[ck], ch, to, put, put_f))) return rc;
      if (stage) {                                               // from here on `ch` is what the stage kept
        if ((rc = stage->filter(c, f.s, ch))) return rc;
        if (!ch.owned) continue;
      }
      if ((rc = found_download(f, ch, to, put, put_f, R))) return rc;
    }
    return ALEO_MI355X_OK;
  });
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
  else rc = found_many_on_device(R, text, offsets, n, k);
  if (rc) return rc;
  for (size_t j = 0; j < n_keys; ++j) out[j] = R[j].release();
  return ALEO_MI355X_OK;
}

// one account: the call above with one key; only the refusal of a null result pointer names the call
static int32_t decrypt_strings(Found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_key32, const void* address_x32, bool may_route) {
  if (!out) return bad_arg("records_decrypt_strings: null result pointer");
  return decrypt_strings_many(out, text, offsets, n, view_key32, address_x32, 1, may_route);
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
