// records_found_blocks.h — what ONE BLOCK does in the kernels behind the scan that count, rank, gather and finish the owned records' private fields: the bodies
// of records_found.hip's four kernels (one account: a row of n flags) and of records_found_many.hip's (several accounts: a [key][record] matrix, a block's row
// being blockIdx.y).  A kernel hands its block the pointers of ITS row and the place of its totals among all blocks' (`bi` of `rows`); nothing here reads a
// block index except for the record index inside the row, so the two files differ only in how they lay the rows out.  The walk itself is records_found_lane.h's.
#pragma once
#include "records_found_lane.h"

namespace aleo_mi355x {

static constexpr uint32_t FOUND_BLOCK = 256, FOUND_TOP = 1024;
static constexpr uint32_t FOUND_LDS_BYTES = 64 * 1024;              // k_records_parse's budget

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

// The block's span of the text into LDS where it fits, as k_records_parse stages it: text readable up to the next multiple of 16 past the chunk's last character.
__device__ __forceinline__ bool stage_span(uint4* stage, const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t b0, uint32_t n, uint32_t* lo_out) {
  const uint32_t b1 = b0 + FOUND_BLOCK < n ? b0 + FOUND_BLOCK : n;
  const uint32_t lo = off[b0] & ~15u, hi = off[b1];            // uniform
  *lo_out = lo;
  if (hi - lo > FOUND_LDS_BYTES) return false;
  for (uint32_t t = threadIdx.x; lo + 16 * t < hi; t += FOUND_BLOCK) stage[t] = *(const uint4*)(text + lo + 16 * (size_t)t);
  __syncthreads();
  return true;
}

// The counting walk of the records b0 .. b0 + 256 of a row.  cnt / pos: the exclusive sums of the field counts and of the owned bits WITHIN the block;
// blk: [fields | owned][rows], this block's totals at bi.  stat: [2] the unparsed strings, [3] n - (the first of them), both through one atomic per wave that holds
// one, zeroed before the launch — only where count_refused (the strings are the same for every row: one row counts them).
__device__ __forceinline__ void found_count_block(uint4* stage, uint32_t (*wave_tot)[FOUND_BLOCK / 64], uint32_t* __restrict__ cnt, uint32_t* __restrict__ pos, uint8_t* __restrict__ pre,
                                                  uint32_t* __restrict__ blk, uint32_t bi, uint32_t rows, uint32_t* __restrict__ stat, bool count_refused,
                                                  const uint8_t* __restrict__ flags, const uint8_t* __restrict__ scan_flags, const int8_t* __restrict__ kinds,
                                                  const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t b0, uint32_t n) {
  const uint32_t i = b0 + threadIdx.x;
  const bool live = i < n;
  const int32_t kind = live ? kinds[i] : 0;
  const bool owned = live && flags[i] == 1;
  if (count_refused) {                                         // uniform
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

// One block of FOUND_TOP lanes: blk's two rows of `rows` block totals become their exclusive sums, the totals go to stat[0] (owned records) and stat[1] (fields).
// per_row != 0: every per_row totals are one row of the flag matrix, and row r's two sums at its first block — what lies before the row — go to
// stat[4 + r] (owned) and stat[4 + rows / per_row + r] (fields).
__device__ __forceinline__ void found_offsets_block(uint32_t (*wave_tot)[FOUND_TOP / 64], uint32_t* __restrict__ blk, uint32_t* __restrict__ stat, uint32_t rows, uint32_t per_row) {
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
    if (per_row && k % per_row == 0) { stat[4 + k / per_row] = ro; stat[4 + rows / per_row + k / per_row] = rf; }
    rf += vf; ro += vo;
  }
  if (threadIdx.x == 0) { stat[0] = to; stat[1] = tf; }
}

// The gathering walk of the records b0 .. b0 + 256 of a row.  An owned record's rank among ALL rows' owned is j = blk[owned row][bi] + pos[i], its first field
// f = blk[fields row][bi] + cnt[i].  fields: room for n_fields rows; the c_* arrays: n_owned entries (c_off one more: the total, written where `first`).
// c_mc: the value of a public microcredits entry, else 0; c_mc_at / c_mc_n: where a private one's fields lie among the gathered fields (n 0: none).
__device__ __forceinline__ void found_gather_block(uint4* stage, char* __restrict__ fields, uint32_t* __restrict__ c_index, int8_t* __restrict__ c_kind, char* __restrict__ c_rvk, uint32_t* __restrict__ c_off,
                                                   uint8_t* __restrict__ c_pre, uint64_t* __restrict__ c_mc, uint32_t* __restrict__ c_mc_at, uint32_t* __restrict__ c_mc_n,
                                                   const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ pos, const uint8_t* __restrict__ pre, const uint32_t* __restrict__ blk,
                                                   uint32_t bi, uint32_t rows, bool first, const uint8_t* __restrict__ flags, const int8_t* __restrict__ kinds, const char* __restrict__ rvk,
                                                   const char* __restrict__ text, const uint32_t* __restrict__ off, uint32_t b0, uint32_t n, uint32_t n_owned, uint32_t n_fields) {
  const uint32_t i = b0 + threadIdx.x;
  if (first && i == 0) c_off[n_owned] = n_fields;
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

// Behind k_records_decrypt, the lane of owned record j: status = what the walk found, else the decryption's flag; the rows of a record the walk marked malformed
// are zeroed (the decryption ran over them with a zero key); microcredits only of a record with status 0.
__device__ __forceinline__ void found_microcredits_lane(uint32_t j, uint8_t* __restrict__ c_status, uint64_t* __restrict__ c_mc, char* __restrict__ fields, const uint8_t* __restrict__ c_pre,
                                                        const uint8_t* __restrict__ c_dec, const uint32_t* __restrict__ c_off, const uint32_t* __restrict__ c_mc_at,
                                                        const uint32_t* __restrict__ c_mc_n) {
  const uint32_t pre = c_pre[j], status = pre ? pre : c_dec[j];
  c_status[j] = (uint8_t)status;
  if (pre == FOUND_MALFORMED)
    for (uint32_t k = c_off[j]; k < c_off[j + 1]; ++k) { uint4* o = (uint4*)(fields + (size_t)k * 32); o[0] = make_uint4(0, 0, 0, 0); o[1] = make_uint4(0, 0, 0, 0); }
  if (status != FOUND_OK) { c_mc[j] = 0; return; }
  const uint32_t mn = c_mc_n[j];
  if (!mn) return;                                             // a public entry's value, or 0, stands
  const char* at = fields + (size_t)c_mc_at[j] * 32;
  c_mc[j] = found_microcredits_private(mn, [&](uint32_t k, uint32_t (&w)[8]) {
    const uint4* p = (const uint4*)(at + (size_t)k * 32); const uint4 l = p[0], h = p[1];
    w[0] = l.x; w[1] = l.y; w[2] = l.z; w[3] = l.w; w[4] = h.x; w[5] = h.y; w[6] = h.z; w[7] = h.w; });
}

}  // namespace aleo_mi355x
