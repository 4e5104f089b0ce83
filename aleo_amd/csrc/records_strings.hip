// records_strings.hip — the record search straight from "record1…" strings: parse_many (owner variant, owner field and nonce x of n strings) and scan_strings
// (which of these strings' records does each of these accounts own), with the strings handed over in one blob and decoded on the device.
//
// What a caller holds is what the chain hands out: the reference reads record ciphertexts out of block JSON as strings (rust/src/api/blocking.rs:209-218, :264-276;
// RecordCiphertext.fromString of its wasm) and parses them one by one before it asks is_owner.  aleo_mi355x_record_parse (wire.hip) is that step here, one call,
// one string copy and three grown vectors per record on one thread — several times the cost of the scan it feeds.  These calls take the text of all strings and
// n + 1 offsets instead:
//   k_records_parse     one string per lane (records_strings_lane.h): bech32m decode, checksum, layout walk; writes the owner variant and the two 32-byte rows
//                       where k_records_scan_many<W> reads them (records_many.hip), zeros for a refused string.  A block's strings are one contiguous span
//                       of the blob: it is staged in LDS where it fits, and read from global memory lane by lane where it does not.
//   k_records_resolve   behind the scan kernel, per (key, record): a refused string gets flag 3 and a zero key row; a public owner is compared with the key's
//                       address x (RecordCiphertext.isOwner for a public owner: the nonce plays no part) and keeps the row the scan computed from its nonce; a
//                       private owner keeps the scan's answer untouched.
// The scan between them is records_many.hip's, unchanged: scan_many_on_device takes a StringSource (records_strings.h) in place of the caller's rows.
// The host path is the same lane function on the calling thread, with no allocation per string — the fallback, what small batches take, and the checker.
#include "records_strings.h"
#include "records_strings_lane.h"
#include <cstdlib>

namespace aleo_mi355x {

static constexpr uint32_t PARSE_BLOCK = SPAN_BLOCK;
static constexpr size_t PARSE_CHUNK_RECORDS = (size_t)1 << 20;
static constexpr size_t STRINGS_CHUNK_CHARS = (size_t)256 << 20;

// ---- the host path ----------------------------------------------------------------------------------------------------------------------------------
static int32_t parse_one_host(uint8_t* owner32, uint8_t* nonce32, const char* text, const uint64_t* offsets, size_t i) {
  const uint64_t span = offsets[i + 1] - offsets[i];
  const uint8_t* mine = (const uint8_t*)text + offsets[i];
  uint32_t ow[8], nw[8];
  const int32_t kind = records_parse_lane([&](uint32_t j) { return mine[j]; }, span > RS_MAX_CHARS ? RS_MAX_CHARS + 1 : (uint32_t)span, ow, nw);
  std::memcpy(owner32, ow, 32); std::memcpy(nonce32, nw, 32);
  return kind;
}

static int32_t parse_many_on_host(int8_t* kinds, void* owner32, void* nonce32, const char* text, const uint64_t* offsets, size_t n) {
  for (size_t i = 0; i < n; ++i) kinds[i] = (int8_t)parse_one_host((uint8_t*)owner32 + 32 * i, (uint8_t*)nonce32 + 32 * i, text, offsets, i);
  return ALEO_MI355X_OK;
}

// every string is parsed once; the rule of k_records_resolve per (key, record)
static int32_t scan_strings_on_host(uint8_t* flags, int8_t* kinds, void* rvk_out, const char* text, const uint64_t* offsets, size_t n, const ManyKeys& k) {
  const RecordsConsts& C = records_consts();
  for (size_t i = 0; i < n; ++i) {
    uint8_t c0[32], nx[32], addr[32];
    const int32_t kind = parse_one_host(c0, nx, text, offsets, i);
    if (kinds) kinds[i] = (int8_t)kind;
    for (size_t j = 0; j < k.args.size(); ++j) {
      uint8_t* rvk = rvk_out ? (uint8_t*)rvk_out + 32 * (j * n + i) : nullptr;
      if (kind < 0) { flags[j * n + i] = 3; if (rvk) std::memset(rvk, 0, 32); continue; }
      const uint8_t flag = scan_one_host(rvk, c0, nx, k.args[j], k.addr[j], C);      // zeros into rvk where the nonce is malformed
      if (kind == 1) { flags[j * n + i] = flag; continue; }
      const HFr a = HFr::from_mont(k.addr[j]); std::memcpy(addr, a.l, 32);
      flags[j * n + i] = std::memcmp(c0, addr, 32) ? 0 : 1;
    }
  }
  return ALEO_MI355X_OK;
}

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------------------
// text: the chunk's characters, readable up to the next multiple of 16 past the last of them; off: n + 1 chunk-relative offsets.  c0 / nx: 32-byte aligned rows.
__global__ void __launch_bounds__(PARSE_BLOCK) k_records_parse(int8_t* __restrict__ kinds, char* __restrict__ c0, char* __restrict__ nx, const char* __restrict__ text,
                                                               const uint32_t* __restrict__ off, uint32_t n) {
  __shared__ uint4 stage[SPAN_LDS_BYTES / 16];
  const uint32_t b0 = blockIdx.x * PARSE_BLOCK;
  uint32_t lo;
  const bool staged = stage_span(stage, text, off, b0, n, &lo);
  const uint32_t i = b0 + threadIdx.x;
  if (i >= n) return;                                        // no barrier below
  const uint32_t first = off[i], len = off[i + 1] - first;
  uint32_t ow[8], nw[8];
  int32_t kind;
  if (staged) { const uint8_t* mine = (const uint8_t*)stage + (first - lo); kind = records_parse_lane([&](uint32_t j) { return mine[j]; }, len, ow, nw); }
  else { const uint8_t* __restrict__ mine = (const uint8_t*)text + first; kind = records_parse_lane([&](uint32_t j) { return mine[j]; }, len, ow, nw); }
  kinds[i] = (int8_t)kind;
  uint4* o = (uint4*)(c0 + (size_t)i * 32); uint4* x = (uint4*)(nx + (size_t)i * 32);
  o[0] = make_uint4(ow[0], ow[1], ow[2], ow[3]); o[1] = make_uint4(ow[4], ow[5], ow[6], ow[7]);
  x[0] = make_uint4(nw[0], nw[1], nw[2], nw[3]); x[1] = make_uint4(nw[4], nw[5], nw[6], nw[7]);
}

// grid = (record blocks, keys); flags / rvk: [key][record], n records per row
__global__ void __launch_bounds__(PARSE_BLOCK) k_records_resolve(uint8_t* __restrict__ flags, char* __restrict__ rvk, const int8_t* __restrict__ kinds, const char* __restrict__ c0,
                                                                 uint32_t n, const ScanArgs* __restrict__ keys) {
  const uint32_t i = blockIdx.x * PARSE_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t kind = kinds[i];
  if (kind == 1) return;                                     // a private owner: the scan's flag and row stand
  const size_t at = (size_t)blockIdx.y * n + i;
  if (kind < 0) {
    flags[at] = 3;
    uint4* r = (uint4*)(rvk + at * 32); r[0] = make_uint4(0, 0, 0, 0); r[1] = make_uint4(0, 0, 0, 0);
    return;
  }
  const uint4* o = (const uint4*)(c0 + (size_t)i * 32);
  const uint4 lo = o[0], hi = o[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const F29 owner = f29_from_words(w);                       // canonical (the parse refused anything else), as the key's address limbs are
  bool same = true;
#pragma unroll
  for (int l = 0; l < 9; ++l) same = same && owner.v[l] == keys[blockIdx.y].addr[l];
  flags[at] = same ? 1 : 0;
}

// ---- the source of strings of the scan's device flow (records_strings.h) -------------------------------------------------------------------------------
static inline size_t uploaded(const uint64_t* offsets, size_t i) { const uint64_t span = offsets[i + 1] - offsets[i]; return span > RS_MAX_CHARS ? 0 : (size_t)span; }

void StringSource::cut_chunks(size_t n, size_t record_cap) {
  const size_t cap = env_cap("ALEO_MI355X_SCAN_CHUNK_CHARS", STRINGS_CHUNK_CHARS);
  cut.assign(1, 0); max_records = max_chars = 0;
  for (size_t at = 0; at < n;) {
    size_t e = at + 1, chars = uploaded(offsets, at);
    while (e < n && e - at < record_cap && chars + uploaded(offsets, e) <= cap) chars += uploaded(offsets, e++);
    if (e - at > max_records) max_records = e - at;
    if (chars > max_chars) max_chars = chars;
    cut.push_back(e); at = e;
  }
}

// scratch: [offsets (max_records + 1) x 4 B][kinds max_records B][text max_chars B], each part 32-byte aligned (k_records_parse reads the text in 16-byte pieces)
size_t StringSource::scratch_bytes() const { Carve cv; cv.part((max_records + 1) * 4); cv.part(max_records); cv.part(max_chars); return cv.total; }

int32_t StringSource::fill(hipStream_t s, size_t k, char* scratch, char* dc0, char* dnx) {
  const size_t at = cut[k], m = cut[k + 1] - at;
  uint32_t* doff; int8_t* dkinds; char* dtext; parts(scratch, &doff, &dkinds, &dtext);
  rel.resize(m + 1);
  size_t pos = 0, run_dev = 0; uint64_t run_host = offsets[at];      // a run: strings that go up in one copy; an over-long string ends it
  auto flush = [&](uint64_t host_end) -> int32_t {
    if (host_end > run_host) HIPCHK(hipMemcpyAsync(dtext + run_dev, text + run_host, (size_t)(host_end - run_host), hipMemcpyHostToDevice, s));
    return ALEO_MI355X_OK;
  };
  rel[0] = 0;
  for (size_t i = 0; i < m; ++i) {
    const uint64_t span = offsets[at + i + 1] - offsets[at + i];
    if (span > RS_MAX_CHARS) { if (int32_t rc = flush(offsets[at + i])) return rc; run_host = offsets[at + i + 1]; run_dev = pos; }
    else pos += (size_t)span;
    rel[i + 1] = (uint32_t)pos;
  }
  if (int32_t rc = flush(offsets[at + m])) return rc;
  HIPCHK(hipMemcpyAsync(doff, rel.data(), (m + 1) * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_records_parse, dim3((uint32_t)((m + PARSE_BLOCK - 1) / PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, s, dkinds, dc0, dnx, (const char*)dtext, (const uint32_t*)doff, (uint32_t)m);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

int32_t StringSource::resolve(hipStream_t s, size_t k, char* scratch, uint8_t* dflags, char* drvk, const char* dc0, const ScanArgs* dkeys, size_t n_keys) {
  const size_t at = cut[k], m = cut[k + 1] - at;
  uint32_t* doff; int8_t* dkinds; char* dtext; parts(scratch, &doff, &dkinds, &dtext);
  hipLaunchKernelGGL(k_records_resolve, dim3((uint32_t)((m + PARSE_BLOCK - 1) / PARSE_BLOCK), (uint32_t)n_keys), dim3(PARSE_BLOCK), 0, s, dflags, drvk, (const int8_t*)dkinds, dc0, (uint32_t)m, dkeys);
  HIPCHK(hipGetLastError());
  if (kinds) HIPCHK(hipMemcpyAsync(kinds + at, dkinds, m, hipMemcpyDeviceToHost, s));
  return ALEO_MI355X_OK;
}

void StringSource::parts(char* scratch, uint32_t** off, int8_t** kinds_, char** text_) const {
  Carve cv;
  *off = (uint32_t*)(scratch + cv.part((max_records + 1) * 4)); *kinds_ = (int8_t*)(scratch + cv.part(max_records)); *text_ = scratch + cv.part(max_chars);
}

// parse_many on the device: the chunks of a scan over strings, the parse kernel alone, the rows copied back
static int32_t parse_many_on_device(int8_t* kinds, void* owner32, void* nonce32, const char* text, const uint64_t* offsets, size_t n) {
  StringSource src{text, offsets, kinds};                     // outside the slot: its offsets outlive the copies that read them
  src.cut_chunks(n, PARSE_CHUNK_RECORDS);
  return on_slot([&](Ctx* c) -> int32_t {
    hipStream_t s = c->stream;
    Carve cv;
    const size_t o_c0 = cv.part(src.max_records * 32), o_nx = cv.part(src.max_records * 32), o_str = cv.part(src.scratch_bytes());
    if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
    char* base = c->scalars_stage.as<char>(); char* dc0 = base + o_c0; char* dnx = base + o_nx; char* dstr = base + o_str;
    uint32_t* doff; int8_t* dkinds; char* dtext; src.parts(dstr, &doff, &dkinds, &dtext);
    for (size_t k = 0; k + 1 < src.cut.size(); ++k) {
      const size_t at = src.cut[k], m = src.cut[k + 1] - at;
      if (int32_t rc = src.fill(s, k, dstr, dc0, dnx)) return rc;
      HIPCHK(hipMemcpyAsync(kinds + at, dkinds, m, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync((char*)owner32 + at * 32, dc0, m * 32, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync((char*)nonce32 + at * 32, dnx, m * 32, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));                         // the next chunk reuses the buffers
    }
    return ALEO_MI355X_OK;
  });
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

int32_t aleo_mi355x_records_parse_many_host(int8_t* kinds, void* owner32, void* nonce32, const char* text, const uint64_t* offsets, size_t n) {
  return guarded([&] {
    if ((!kinds || !owner32 || !nonce32) && n) return bad_arg("records_parse_many: null buffer");
    if (int32_t rc = strings_args_ok("records_parse_many", text, offsets, n)) return rc;
    return parse_many_on_host(kinds, owner32, nonce32, text, offsets, n);
  });
}

int32_t aleo_mi355x_records_parse_many(int8_t* kinds, void* owner32, void* nonce32, const char* text, const uint64_t* offsets, size_t n) {
  return guarded([&] {
    if ((!kinds || !owner32 || !nonce32) && n) return bad_arg("records_parse_many: null buffer");
    if (int32_t rc = strings_args_ok("records_parse_many", text, offsets, n)) return rc;
    if (n < aleo_mi355x_min_records() || n == 0) return parse_many_on_host(kinds, owner32, nonce32, text, offsets, n);
    return parse_many_on_device(kinds, owner32, nonce32, text, offsets, n);
  });
}

int32_t aleo_mi355x_records_scan_strings_host(uint8_t* flags, int8_t* kinds, void* rvk_out, const char* text, const uint64_t* offsets, size_t n,
                                              const void* view_keys32, const void* address_xs32, size_t n_keys) {
  return guarded([&] {
    ManyKeys k; if (int32_t rc = many_keys(k, view_keys32, address_xs32, n_keys)) return rc;
    if (!flags && n) return bad_arg("records_scan_strings: null buffer");
    if (int32_t rc = strings_args_ok("records_scan_strings", text, offsets, n)) return rc;
    return scan_strings_on_host(flags, kinds, rvk_out, text, offsets, n, k);
  });
}

int32_t aleo_mi355x_records_scan_strings(uint8_t* flags, int8_t* kinds, void* rvk_out, const char* text, const uint64_t* offsets, size_t n,
                                         const void* view_keys32, const void* address_xs32, size_t n_keys) {
  return guarded([&] {
    ManyKeys k; if (int32_t rc = many_keys(k, view_keys32, address_xs32, n_keys)) return rc;
    if (!flags && n) return bad_arg("records_scan_strings: null buffer");
    if (int32_t rc = strings_args_ok("records_scan_strings", text, offsets, n)) return rc;
    if (n * n_keys < aleo_mi355x_min_records() || n == 0) return scan_strings_on_host(flags, kinds, rvk_out, text, offsets, n, k);      // in pairs, as records_scan_many counts
    StringSource src{text, offsets, kinds};
    return scan_many_on_device(flags, rvk_out, nullptr, nullptr, n, k, &src);
  });
}

}  // extern "C"
