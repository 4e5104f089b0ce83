// records_found.h — what records_found.hip shares with records_unspent.hip: the device flow of decrypt_strings[_many] with an optional stage between
// k_found_microcredits and the downloads, the second level of its exclusive sums, the block-level sums both files' kernels run, and the layout of the words a call
// reads back through the slot's pinned buffer (FoundPinned).  From records_serial.hip:
// the resident tables of the serial-number lane and the one serial-number kernel's launches over key segments.
#pragma once
#include "records_strings.h"
#include "records_found_host.hpp"
#include "records_serial_lane.h"
#include "records_commit_lane.h"
#include <memory>

namespace aleo_mi355x {

static constexpr uint32_t FOUND_BLOCK = SPAN_BLOCK, FOUND_TOP = 1024;      // FOUND_BLOCK: the walks stage their block's span (records_strings.h stage_span)

#ifdef __HIPCC__
// The exclusive sums of two values over the block's 256 lanes (wave shuffles, then the four wave totals through LDS); *ta / *tb: the block's totals.
__device__ __forceinline__ void block_exclusive2(uint32_t& a, uint32_t& b, uint32_t (*wave_tot)[FOUND_BLOCK / 64], uint32_t* ta, uint32_t* tb) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t ia = a, ib = b;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t ua = __shfl_up(ia, d, 64), ub = __shfl_up(ib, d, 64);
    if (lane >= (uint32_t)d) { ia += ua; ib += ub; }
  }
  if (lane == 63) { wave_tot[0][wave] = ia; wave_tot[1][wave] = ib; }
  __syncthreads();
  uint32_t ba = 0, bb = 0, sa = 0, sb = 0;
#pragma unroll
  for (uint32_t w = 0; w < FOUND_BLOCK / 64; ++w) { if (w < wave) { ba += wave_tot[0][w]; bb += wave_tot[1][w]; } sa += wave_tot[0][w]; sb += wave_tot[1][w]; }
  a = ba + ia - a; b = bb + ib - b; *ta = sa; *tb = sb;
}
#endif

// One chunk's compacted arrays on the device, all keys' one after another (key 0's records, then key 1's, each in record order): `owned` records with `nf`
// fields; key j's are the ranks first[j] .. first[j + 1] and the fields first_f[j] .. first_f[j + 1] (K + 1 entries each).  index is chunk-relative, off has
// owned + 1 entries.  status null: every record's is 0.  serials, commitments null: there are none.  text / soff: the chunk's strings on the device, record i of the
// chunk the characters soff[i] .. soff[i + 1].  pin: the call's words in pinned memory (FoundPinned below).
struct FoundPinned;
struct FoundChunk {
  FoundPinned* pin = nullptr;
  char* fields = nullptr; uint32_t* index = nullptr; int8_t* kind = nullptr; char* rvk = nullptr; uint32_t* off = nullptr; uint64_t* mc = nullptr; uint8_t* status = nullptr; char* serials = nullptr;
  char* commitments = nullptr; const char* text = nullptr; const uint32_t* soff = nullptr;
  size_t at = 0, owned = 0, nf = 0;                                        // at: the chunk's first record among the call's strings
  std::vector<uint32_t> first, first_f;
};

// The optional stage of found_many_on_device.  begin: once per call, on the call's slot, in front of the first chunk.  gathered: behind k_found_gather, before
// the decryption is launched (ch.index is written; the stage may wait for
// it while the decryption's kernels are still to come).  filter: behind k_found_microcredits, on the same stream: it may replace every pointer, count and
// boundary of `ch` by those of the records it keeps, in buffers of its own; it returns with the stream idle.  What `ch` then holds is what comes down.
struct FoundStage {
  virtual int32_t begin(Ctx* c, hipStream_t s) = 0;
  virtual int32_t gathered(Ctx* c, hipStream_t s, const FoundChunk& ch) = 0;
  virtual int32_t filter(Ctx* c, hipStream_t s, FoundChunk& ch) = 0;
  virtual ~FoundStage() = default;
};

// records_found.hip: the flow of decrypt_strings_many over K = k.args.size() keys into R[0 .. K); R[j]->owned counts what key j owned before any stage.
// It takes a slot for itself (entry.h on_slot); R and the stage are the caller's and outlive it.
int32_t found_many_on_device(std::vector<std::unique_ptr<Found>>& R, const char* text, const uint64_t* offsets, size_t n, const ManyKeys& k, FoundStage* stage = nullptr);
// k_found_offsets over `rows` block totals of two kinds (blk: [fields | owned][rows]) in groups of nb: see the kernel; the caller checks hipGetLastError
void launch_found_offsets(hipStream_t s, uint32_t* blk, uint32_t* stat, uint32_t rows, uint32_t nb);

// records_serial.hip: the lane's tables on this device (entry.h resident_table)
int32_t serial_tables_on_device(int device, const uint32_t** out);

// Where the keys' segments lie among commitment rows in rank order: key j's rows are the ranks rank0[j] .. rank0[j + 1], and the waves wave0[j] .. wave0[j + 1]
// of the padded grid (ceil(rows / 64) waves each), so a wave has one key.
struct UnspentSegs { uint32_t n_keys, wave0[SCAN_MANY_KEYS + 1], rank0[SCAN_MANY_KEYS + 1]; };
// What a call of the flow reads back through the slot's pinned buffer, every reader its own member: found_count the flow's words (k_found_offsets: four totals,
// then per key the owned pairs and the fields before its row), UnspentStage::filter the stage's (k_unspent_scatter: eight words of totals, then the kept pairs
// and the kept fields before each key's segment, one more of each for the end), commit_rows_of_chunk the records its lane routed to the host.
struct FoundPinned { uint32_t flow[4 + 2 * SCAN_MANY_KEYS], stage[8 + 2 * (SCAN_MANY_KEYS + 1)], routed; };
static_assert(sizeof(UnspentSegs::rank0) / 4 == SCAN_MANY_KEYS + 1 && sizeof(FoundPinned::stage) / 4 == 8 + 2 * (sizeof(UnspentSegs::rank0) / 4) &&
              sizeof(FoundPinned::flow) / 4 == 4 + 2 * SCAN_MANY_KEYS, "the kernels write one pair of words per key (the stage: per segment boundary), many_keys admits SCAN_MANY_KEYS keys");
// room for it, once per call; the stage and the commitment rows reach it through FoundChunk::pin
inline int32_t found_pinned(Ctx* c, FoundPinned** out) { if (int32_t rc = ensure_host_pinned(c, sizeof(FoundPinned))) return rc; *out = (FoundPinned*)c->h_pinned; return ALEO_MI355X_OK; }
// the digits of a key made by serial::serial_key, as the kernel's key table holds them
inline SerialArgs serial_args_of(const ScanArgs& a) {
  SerialArgs r; std::memcpy(r.naf_pos, a.naf_pos, sizeof r.naf_pos); std::memcpy(r.naf_neg, a.naf_neg, sizeof r.naf_neg); r.naf_len = a.naf_len; return r;
}
// k_records_serial over every segment, key j's digits at dkeys[j] in device memory: launches of at most ALEO_MI355X_SERIAL_CHUNK lanes (read per call), which may span key boundaries
int32_t launch_records_serial(hipStream_t s, char* dsn, uint8_t* dflags, const char* dcm, const uint32_t* dK, const SerialArgs* dkeys, const UnspentSegs& seg);

// records_unspent.hip: the open-addressing table (records_spent_lane.h) over the n_spent rows of a spent set on the device: the table's `cap` slots are zeroed,
// then k_spent_insert runs, one row per lane
int32_t launch_spent_insert(hipStream_t s, uint32_t* table, uint32_t cap, const uint32_t* rows, size_t n_spent);

// records_commit.hip: the commitment lane's table on this device (entry.h resident_table)
int32_t commit_tables_on_device(int device, const uint32_t** out);
// records_commit.hip: what a call's (program id, record name) comes to — refused with the reference's two texts — and the commitments of owned records
struct CommitCall { std::vector<uint8_t> name_bits; CommitArgs args; };
int32_t commit_call(CommitCall& cc, const char* program_id, const char* record_name);
// one record on the host, as aleo_mi355x_record_commitment computes it: the flag (0, or 4 with a row of zeros); plain: its n_fields decrypted fields
uint8_t commit_one_host(uint8_t* out32, const char* record1, size_t chars, const uint8_t* plain, size_t n_fields, const CommitCall& cc);
// What commit_rows_of_chunk keeps on the host; the stage that owns it outlives the call's last synchronisation.
struct CommitScratch { std::vector<uint32_t> index, off; std::vector<int8_t> kind; std::vector<uint8_t> status, fields, cm, flags; };
// The rows (dcm: owned x 32 B) and flags (dflags: owned) of the chunk's records behind k_found_microcredits, on the device when the stream has run: from
// k_records_commit, or from the calling thread below aleo_mi355x_min_commitments() records and for the records the lane routes (text / offsets: the call's strings).
// want_host: H.cm holds the rows on return.  droute: one word of device scratch.
int32_t commit_rows_of_chunk(Ctx* c, hipStream_t s, const FoundChunk& ch, const CommitCall& cc, const char* text, const uint64_t* offsets, char* dcm, uint8_t* dflags, uint32_t* droute,
                             CommitScratch& H, bool want_host);

}  // namespace aleo_mi355x
