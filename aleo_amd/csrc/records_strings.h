// records_strings.h — what records_many.hip and records_strings.hip share: the keys of a multi-account scan, its device flow, and the source of strings that
// flow can be given in place of the caller's 32-byte rows (records_strings.hip: the chunk's text goes up, k_records_parse writes the rows where the scan kernels
// read them, k_records_resolve settles the refused strings and the public owners behind the scan).
#pragma once
#include "entry.h"
#include "records_host.hpp"
#include <vector>

namespace aleo_mi355x {

// *dK: the records constants (records_lane.h RK_*) resident on the slot's device: what the scan, the decryption and the walks between them read
inline int32_t records_constants(Ctx* c, const uint32_t** dK) {
  return resident_table(c->device, ResidentTable::RECORDS, []() -> const std::vector<uint32_t>& { return records_consts().words; }, dK);
}

static constexpr uint32_t SCAN_MANY_KEYS = 64;               // the accounts of one call: many_keys refuses more, and the per-key tables are sized by it
struct ManyKeys { std::vector<ScanArgs> args; std::vector<HFr> addr; };

static constexpr uint32_t SPAN_BLOCK = 256, SPAN_LDS_BYTES = 64 * 1024;      // the lanes, and strings, of a block that reads the text; the LDS it spends on its span

#ifdef __HIPCC__
// A block's strings (b0 .. b0 + SPAN_BLOCK of the chunk's n) are one contiguous span of the text: where it fits SPAN_LDS_BYTES the block copies it to LDS with
// 16-byte loads, every lane of a wave reading its neighbours' lines, and string i lies at stage + (off[i] - *lo_out); a lane's own byte loads from global memory
// touch 64 cache lines per instruction of a wave (measured: DESIGN §11).  A longer span — 256 strings of more than 255 characters on average — gets false and is
// read from global memory.  Every lane of the block calls it (a barrier follows the copy); text: readable up to the next multiple of 16 past its last character.
// BLOCK, LDS_BYTES: the same for a block of another size (key_ciphertexts.hip: one wave).
template <uint32_t BLOCK = SPAN_BLOCK, uint32_t LDS_BYTES = SPAN_LDS_BYTES>
__device__ __forceinline__ bool stage_span(uint4* stage, const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t b0, uint32_t n, uint32_t* lo_out) {
  const uint32_t b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
  const uint32_t lo = off[b0] & ~15u, hi = off[b1];            // uniform: the block's span, from a 16-byte boundary
  *lo_out = lo;
  if (hi - lo > LDS_BYTES) return false;
  for (uint32_t t = threadIdx.x; lo + 16 * t < hi; t += BLOCK) stage[t] = *(const uint4*)(text + lo + 16 * (size_t)t);
  __syncthreads();
  return true;
}
#endif

// n strings one after another in `text`, string i at text[offsets[i] .. offsets[i + 1]), cut into chunks of whole records: chunk k holds the records
// cut[k] .. cut[k + 1], at most `record_cap` of them and, unless it is one record, at most the character cap (ALEO_MI355X_SCAN_CHUNK_CHARS, read per call; 256 MiB)
// of uploaded characters.  A string longer than RS_MAX_CHARS is refused without being uploaded: it counts, and travels, as the empty string, which is refused too.
struct StringSource {
  const char* text; const uint64_t* offsets; int8_t* kinds;   // kinds: the caller's, or null
  std::vector<size_t> cut;
  size_t max_records = 0, max_chars = 0;                      // of one chunk
  std::vector<uint32_t> rel;                                  // the chunk-relative offsets on their way to the device: kept until the stream has taken them
  void cut_chunks(size_t n, size_t record_cap);
  size_t scratch_bytes() const;                               // of device memory behind the rows, 32-byte aligned
  // chunk k: uploads text and offsets into `scratch` and launches k_records_parse, which fills dc0 / dnx (32 B per record) and the kinds kept in scratch
  int32_t fill(hipStream_t s, size_t k, char* scratch, char* dc0, char* dnx);
  // behind the scan kernel: k_records_resolve over flags / rvk ([key][record of the chunk]), then the copy of the kinds to the caller
  int32_t resolve(hipStream_t s, size_t k, char* scratch, uint8_t* dflags, char* drvk, const char* dc0, const ScanArgs* dkeys, size_t n_keys);
  // where fill left the chunk's relative offsets, kinds and text inside `scratch` (records_found.hip walks the owned records from them)
  void parts(char* scratch, uint32_t** off, int8_t** kinds, char** text) const;
};

// records_many.hip
int32_t many_keys(ManyKeys& k, const void* view_keys32, const void* address_xs32, size_t n_keys);
// the records come as rows (owner_c0, nonce_x) or, when `strings` is given, from it; takes a slot for itself (entry.h on_slot)
int32_t scan_many_on_device(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const ManyKeys& k, StringSource* strings = nullptr);
// the plan of a scan of k's keys over n records — the records of one launch (the pair cap, the record cap, n), *W, the keys one lane takes, and the table of the
// keys padded with zero entries to a multiple of W — and that launch over m records already on the device (flags m x n_keys B, rvk m x n_keys x 32 B,
// [key][record]; dkeys: the table); the caller checks hipGetLastError
size_t scan_many_plan(size_t n, const ManyKeys& k, uint32_t* W, std::vector<ScanArgs>* table);
void launch_scan_keys(hipStream_t s, uint32_t W, uint8_t* dflags, char* drvk, const char* dc0, const char* dnx, size_t m, const uint32_t* dK, const ScanArgs* dkeys, size_t n_keys);

// records_decrypt.hip
static constexpr size_t DECRYPT_CHUNK_FIELDS = (size_t)1 << 22;      // the field cap of one k_records_decrypt launch; ALEO_MI355X_DECRYPT_CHUNK_FIELDS (read per call) lowers it
// the end of the launch that starts at record `at` of n (offsets: n + 1 field boundaries): whole records within the two caps, one at least
size_t decrypt_cut(const uint32_t* offsets, size_t at, size_t n, size_t record_cap, size_t field_cap);
// k_records_decrypt over n records already on the device: io the fields from offsets[0] on, in place; the caller checks hipGetLastError
void launch_records_decrypt(hipStream_t s, char* io, uint8_t* dflags, const char* drvk, const uint32_t* doffsets, uint32_t base, size_t n, const uint32_t* dK);

}  // namespace aleo_mi355x
