// records_many.hip — the ownership scan of records.hip for SEVERAL accounts in one call: which of these n records does each of these K accounts own.
//
// What a front end asks that serves several callers: the reference's dev server runs record_finder.find_one_record(&private_key, ...) on every deploy, execute
// and transfer request that brings no fee record (rust/develop/src/routes.rs:112, :143, :194-220 of the reference), each walking the same blocks through
// get_unspent_records -> is_owner_with_address_x_coordinate (rust/src/api/blocking.rs:229-292).  K calls of aleo_mi355x_records_scan upload the records K times
// and repeat K times what depends on the record alone; this call uploads them once per chunk and, from a launch size on, gives a GROUP of W keys to one lane
// (records_many_lane.h), which shares the root, the doublings and the inversion among them.
//
// k_records_scan_many<W>: grid = (record blocks, key groups); a block's group is blockIdx.y.  The key table (K x ScanArgs, padded with zero entries to a
// multiple of W) lies in device memory and is read through uniform loads.  W = 1 is records_scan_lane itself over the same grid, and the one-account scan's only
// kernel (records.hip calls scan_many_on_device with one key).  Results are written [key][record of the chunk] and copied to the caller's [key][record] rows.
// A launch covers at most SCAN_MANY_PAIRS = 2^22 pairs and 2^20 records: 64 B per record and 33 B per pair keep the slot's grow-only scratch near 200 MB.
#include "records_strings.h"
#include "records_many_lane.h"
#include <string>
#include <vector>

namespace aleo_mi355x {

static constexpr uint32_t SCAN_BLOCK = 256;
static constexpr size_t SCAN_MANY_PAIRS = (size_t)1 << 22, SCAN_MANY_RECORDS = (size_t)1 << 20;
static constexpr size_t SCAN_FULL_LANES = 65536;            // 256 CUs x 4 SIMDs x 64 lanes at one wave per SIMD: below it a call's time is one lane's chain, which a group makes ~W times longer

// the per-call arguments of every key; a refused key is named by its index
int32_t many_keys(ManyKeys& k, const void* view_keys32, const void* address_xs32, size_t n_keys) {
  if (n_keys < 1 || n_keys > SCAN_MANY_KEYS) return bad_arg("records_scan_many: n_keys must be 1..64");
  if (!view_keys32 || !address_xs32) return bad_arg("records_scan_many: null buffer");
  k.args.resize(n_keys); k.addr.resize(n_keys);
  for (size_t j = 0; j < n_keys; ++j)
    if (const char* why = scan_args(k.args[j], k.addr[j], (const uint8_t*)view_keys32 + 32 * j, (const uint8_t*)address_xs32 + 32 * j)) {
      g_last_error = std::string(why) + " (records_scan_many: key " + std::to_string(j) + ")";
      return ALEO_MI355X_ERR_BAD_ARG;
    }
  return ALEO_MI355X_OK;
}

static int32_t scan_many_on_host(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const ManyKeys& k) {
  if ((!flags || !owner_c0 || !nonce_x) && n) return bad_arg("records_scan_many: null buffer");
  const RecordsConsts& C = records_consts();
  for (size_t j = 0; j < k.args.size(); ++j)
    for (size_t i = 0; i < n; ++i)
      flags[j * n + i] = scan_one_host(rvk_out ? (uint8_t*)rvk_out + 32 * (j * n + i) : nullptr, (const uint8_t*)owner_c0 + 32 * i, (const uint8_t*)nonce_x + 32 * i, k.args[j], k.addr[j], C);
  return ALEO_MI355X_OK;
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------
// flags / rvk: [key][record], n records per row.  keys: ceil(n_keys / W) * W entries.
template <int W>
__global__ void __launch_bounds__(SCAN_BLOCK) k_records_scan_many(uint8_t* __restrict__ flags, char* __restrict__ rvk, const char* __restrict__ c0, const char* __restrict__ nx,
                                                                  uint32_t n, const uint32_t* __restrict__ K, const ScanArgs* __restrict__ keys, uint32_t n_keys) {
  const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  if (i >= n) return;                                        // no barrier below: a lane parks and fetches its own words only
  const uint32_t first = blockIdx.y * W;
  const Fr c = load_fp<Fr>(c0 + (size_t)i * 32), x = load_fp<Fr>(nx + (size_t)i * 32);
  if constexpr (W == 1) {
    const size_t at = (size_t)first * n + i;
    char* out = rvk + at * 32;
    flags[at] = (uint8_t)records_scan_lane(c.v, x.v, K, keys[first], [&](const F29& v) { store_fp<Fr>(out, f29_to_fr(v)); });
  } else {
    __shared__ uint32_t parked[W * 9 * SCAN_BLOCK];           // [key][limb][lane]: 9 KB per key
    const ScanArgs* __restrict__ A = keys + first;
    const uint32_t live = n_keys - first < (uint32_t)W ? n_keys - first : (uint32_t)W;
    uint32_t len = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) len = A[j].naf_len > len ? A[j].naf_len : len;
    uint32_t* mine = parked + threadIdx.x;
    records_scan_lane_many<W>(c.v, x.v, K, A, live, len,
      [&](int j, const F29& v) {
#pragma unroll
        for (int l = 0; l < 9; ++l) mine[(j * 9 + l) * SCAN_BLOCK] = v.v[l]; },
      [&](uint32_t j) { F29 v;
#pragma unroll
        for (int l = 0; l < 9; ++l) v.v[l] = mine[(j * 9 + l) * SCAN_BLOCK];
        return v; },
      [&](uint32_t j, const F29& v) { store_fp<Fr>(rvk + ((size_t)(first + j) * n + i) * 32, f29_to_fr(v)); },
      [&](uint32_t j, uint32_t flag) { flags[(size_t)(first + j) * n + i] = (uint8_t)flag; });
  }
}

template <int W> static void launch_many(hipStream_t s, uint8_t* dfl, char* drvk, const char* dc0, const char* dnx, size_t m, const uint32_t* dK, const ScanArgs* dkeys, size_t n_keys) {
  hipLaunchKernelGGL(k_records_scan_many<W>, dim3((uint32_t)((m + SCAN_BLOCK - 1) / SCAN_BLOCK), (uint32_t)((n_keys + W - 1) / W)), dim3(SCAN_BLOCK), 0, s,
                     dfl, drvk, dc0, dnx, (uint32_t)m, dK, dkeys, (uint32_t)n_keys);
}

// The keys one lane takes.  ALEO_MI355X_SCAN_KEYS_PER_LANE (1, 2, 4, 8; read per call) forces it, for one key as well (padded; same bytes); otherwise the widest group that still leaves the launch
// SCAN_FULL_LANES lanes, among the widths that a call of n_keys keys can fill more than half of.
static uint32_t scan_many_width(size_t records_per_launch, size_t n_keys) {
  const size_t forced = env_size("ALEO_MI355X_SCAN_KEYS_PER_LANE", 0);
  if (forced == 1 || forced == 2 || forced == 4 || forced == 8) return (uint32_t)forced;
  for (uint32_t w = 8; w > 1; w >>= 1)
    if (w / 2 < n_keys && records_per_launch * ((n_keys + w - 1) / w) >= SCAN_FULL_LANES) return w;
  return 1;
}

// The plan of a scan of k's keys over n records — the records of one launch (the pair cap, the record cap, n), *W, the keys one lane takes, and the key table of
// that width (padded to a multiple of W with zero entries, which have no digits at all) — and that launch over m records already on the device: scan_many_on_device
// below and records_found.hip, which runs the scan between a parse and a walk of its own, both go through these two.
size_t scan_many_plan(size_t n, const ManyKeys& k, uint32_t* W, std::vector<ScanArgs>* table) {
  const size_t n_keys = k.args.size();
  size_t chunk = SCAN_MANY_PAIRS / n_keys; if (chunk > SCAN_MANY_RECORDS) chunk = SCAN_MANY_RECORDS; if (chunk > n) chunk = n;
  *W = scan_many_width(chunk, n_keys);
  table->assign((n_keys + *W - 1) / *W * *W, ScanArgs{});
  std::copy(k.args.begin(), k.args.end(), table->begin());
  return chunk;
}
void launch_scan_keys(hipStream_t s, uint32_t W, uint8_t* dflags, char* drvk, const char* dc0, const char* dnx, size_t m, const uint32_t* dK, const ScanArgs* dkeys, size_t n_keys) {
  switch (W) {
    case 8: launch_many<8>(s, dflags, drvk, dc0, dnx, m, dK, dkeys, n_keys); break;
    case 4: launch_many<4>(s, dflags, drvk, dc0, dnx, m, dK, dkeys, n_keys); break;
    case 2: launch_many<2>(s, dflags, drvk, dc0, dnx, m, dK, dkeys, n_keys); break;
    default: launch_many<1>(s, dflags, drvk, dc0, dnx, m, dK, dkeys, n_keys);
  }
}

// The records of a chunk reach dc0 / dnx either as the caller's rows, by two copies, or from `strings` (records_strings.h): its text goes up and k_records_parse
// writes the rows; its chunks are cut at the character cap as well, and k_records_resolve follows the scan kernel.
int32_t scan_many_on_device(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const ManyKeys& k, StringSource* strings) {
  const size_t n_keys = k.args.size();
  uint32_t W; std::vector<ScanArgs> table;                    // the table and the source's offsets are declared outside the slot: they outlive every copy that reads them
  const size_t chunk = scan_many_plan(n, k, &W, &table);
  if (strings) strings->cut_chunks(n, chunk);
  return on_slot([&](Ctx* c) -> int32_t {
    hipStream_t s = c->stream;
    int32_t rc;
    const uint32_t* dK; if ((rc = records_constants(c, &dK))) return rc;
    Carve cv;
    const size_t o_keys = cv.part(table.size() * sizeof(ScanArgs)), o_c0 = cv.part(chunk * 32), o_nx = cv.part(chunk * 32), o_rvk = cv.part(chunk * n_keys * 32), o_fl = cv.part(chunk * n_keys),
                 o_str = cv.part(strings ? strings->scratch_bytes() : 0);
    if ((rc = c->scalars_stage.reserve(cv.total))) return rc;
    char* base = c->scalars_stage.as<char>();
    char* dkeys = base + o_keys; char* dc0 = base + o_c0; char* dnx = base + o_nx; char* drvk = base + o_rvk; uint8_t* dfl = (uint8_t*)(base + o_fl); char* dstr = base + o_str;
    HIPCHK(hipMemcpyAsync(dkeys, table.data(), table.size() * sizeof(ScanArgs), hipMemcpyHostToDevice, s));
    for (size_t at = 0, ck = 0, m; at < n; at += m, ++ck) {
      m = strings ? strings->cut[ck + 1] - at : (n - at < chunk ? n - at : chunk);
      if (strings) { if ((rc = strings->fill(s, ck, dstr, dc0, dnx))) return rc; }
      else {
        HIPCHK(hipMemcpyAsync(dc0, (const char*)owner_c0 + at * 32, m * 32, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dnx, (const char*)nonce_x + at * 32, m * 32, hipMemcpyHostToDevice, s));
      }
      launch_scan_keys(s, W, dfl, drvk, dc0, dnx, m, dK, (const ScanArgs*)dkeys, n_keys);
      HIPCHK(hipGetLastError());
      if (strings && (rc = strings->resolve(s, ck, dstr, dfl, drvk, dc0, (const ScanArgs*)dkeys, n_keys))) return rc;
      // rows of m on the device, rows of n at the caller
      HIPCHK(hipMemcpy2DAsync(flags + at, n, dfl, m, m, n_keys, hipMemcpyDeviceToHost, s));
      if (rvk_out) HIPCHK(hipMemcpy2DAsync((char*)rvk_out + at * 32, n * 32, drvk, m * 32, m * 32, n_keys, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));                         // the next chunk reuses the buffers
    }
    return ALEO_MI355X_OK;
  });
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

int32_t aleo_mi355x_records_scan_many_host(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const void* view_keys32, const void* address_xs32, size_t n_keys) {
  return guarded([&] {
    ManyKeys k; if (int32_t rc = many_keys(k, view_keys32, address_xs32, n_keys)) return rc;
    return scan_many_on_host(flags, rvk_out, owner_c0, nonce_x, n, k);
  });
}

int32_t aleo_mi355x_records_scan_many(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const void* view_keys32, const void* address_xs32, size_t n_keys) {
  return guarded([&] {
    ManyKeys k; if (int32_t rc = many_keys(k, view_keys32, address_xs32, n_keys)) return rc;
    if (n * n_keys < aleo_mi355x_min_records() || n == 0) return scan_many_on_host(flags, rvk_out, owner_c0, nonce_x, n, k);      // in pairs: such a call runs at width 1, one lane's chain like a single scan
    if (!flags || !owner_c0 || !nonce_x) return bad_arg("records_scan_many: null buffer");
    return scan_many_on_device(flags, rvk_out, owner_c0, nonce_x, n, k);
  });
}

}  // extern "C"
