// ntt_plan.h — the host-side decisions of a transform (ntt.hip): which kernel configuration serves a call, and how 2^lg_n splits into passes.
// Plain C++, no HIP: tests/cpp/ntt_plan_test.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace aleo_mi355x {

static constexpr uint32_t INNER_MAX_LG = 11;        // longest in-LDS transform (the inner twiddle table holds w_2048^t)

// One pass of a transform over a tile of 2^lgTE elements: all length-2^lgL DFTs of one axis, 2^lgT adjacent ones per block.
// A pass before the last sees the data as [A][L][Bn] (k_ntt_strided: lgBn, tw_scale); the last sees rows of L and scatters output k of row
// k1 * n2 + k2 to k1 + n1 * (k2 + n2 * k) (k_ntt_final: lgN1, lgN2).
struct NttPass {
  uint32_t lgL = 0, lgT = 0, grid_x = 0;
  uint32_t lgBn = 0, tw_scale = 0;        // before the last pass
  uint32_t lgN1 = 0, lgN2 = 0;            // the last pass
  bool src_tmp = false, dst_tmp = false;  // which of the caller's buffer and the scratch buffer the pass reads and writes
};
struct NttPlan { uint32_t npass = 0; NttPass pass[3]; };      // npass == 0: 2^lg_n does not fit three axes of this tile

inline NttPlan plan_passes(uint32_t lg_n, uint32_t lgTE) {
  NttPlan p;
  const uint32_t maxL = lgTE < INNER_MAX_LG ? lgTE : INNER_MAX_LG;            // longest in-LDS transform with this tile
  if (lg_n > 3 * maxL) return p;
  p.npass = lg_n <= maxL ? 1 : (lg_n <= 2 * maxL ? 2 : 3);
  uint32_t s1 = 0, s2 = 0;                                                      // the axes: s1 (first pass), s2, s3 (last pass)
  if (p.npass == 2) s1 = (lg_n + 1) / 2;
  else if (p.npass == 3) { s1 = (lg_n + 2) / 3; s2 = (lg_n - s1 + 1) / 2; }
  const uint32_t s3 = lg_n - s1 - s2;
  auto lgT_for = [lgTE](uint32_t lgL, uint32_t lg_limit) { const uint32_t lgT = lgTE - lgL; return lgT < lg_limit ? lgT : lg_limit; };
  uint32_t i = 0;
  if (p.npass >= 2) {                     // in place when a third pass follows, into the scratch buffer otherwise
    NttPass& a = p.pass[i++];
    a.lgL = s1; a.lgBn = s2 + s3; a.lgT = lgT_for(a.lgL, a.lgBn); a.grid_x = 1u << (a.lgBn - a.lgT); a.tw_scale = 1u; a.dst_tmp = p.npass == 2;
  }
  if (p.npass == 3) {
    NttPass& b = p.pass[i++];
    b.lgL = s2; b.lgBn = s3; b.lgT = lgT_for(b.lgL, b.lgBn); b.grid_x = (1u << s1) << (b.lgBn - b.lgT); b.tw_scale = 1u << s1; b.dst_tmp = true;
  }
  NttPass& f = p.pass[i];
  f.lgL = s3; f.lgN1 = s1; f.lgN2 = s2; f.lgT = lgT_for(f.lgL, f.lgN1); f.grid_x = (1u << s2) << (s1 - f.lgT); f.src_tmp = p.npass >= 2;
  return p;
}

// Which configuration serves `batch` transforms of 2^lg_n elements.
// Small transforms are latency-bound on the few blocks a 2048-element tile leaves them (2^16: 32 blocks on 256 CUs); 512-element tiles spread them
// over the chip.  Calls of at most 2^19 elements in all (transforms of 2^10 … 2^18 points) take the one-butterfly-per-lane tiles of the 32-bit limbs:
// 2^12 52 -> 22 us, 2^15 64 -> 27 us, 3 x 2^15 67 -> 30 us, 8 x 2^16 85 -> 72 us; from 2^20 elements on the three-stage register groups win again
// (8 x 2^17: 138 against 142 us) (tools/ntt_small_probe.py, profiles/r02_ntt_small_probe.jsonl).
// Everything else runs on 29-bit limbs.  128 KiB-class tiles for 2^20..2^22 (at 2^19 they are only 128 blocks for 256 CUs: 242 against
// 343 GB/s with 64 KiB tiles); beyond 2^22 three passes are needed either way and two 64 KiB-class blocks per CU overlap their HBM phases better
// (2^24: 3.5 vs 4.0 ms).
enum class NttForm { Latency512, Tile4096, Tile2048 };
inline NttForm choose_form(uint32_t lg_n, uint64_t batch) {
  if (lg_n >= 10 && lg_n <= 18 && (batch << lg_n) <= ((uint64_t)1 << 19)) return NttForm::Latency512;
  if (lg_n >= 20 && lg_n <= 22) return NttForm::Tile4096;
  return NttForm::Tile2048;
}

}  // namespace aleo_mi355x
