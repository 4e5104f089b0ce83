// msm_reduce.h — what follows the accumulation on the plain path (c <= 16, every window its own buckets), for any group: the slice-tree, segment-tree and
// gather kernels as templates over the point format of the partial sums, and the host back end (chunk sums, a pairwise tree per window, the window sums
// to the host, Horner over the windows, normalisation) as a template over the group.  msm.hip instantiates them for G1, g2.hip for G2.
#pragma once
#include "ec.h"
#include "fp28.h"
#include "host_field.hpp"
#include "msm_chain.h"
#include <type_traits>

namespace aleo_mi355x {

// Point formats of the partial sums: a size and the cooperative addition out = pa + pb on LANES adjacent lanes (all of them call it together; any operand may
// be the identity, they may be equal or opposite, out may alias either).  32-bit XYZZ (192 B, ec.h) on G1's plain path; 28-bit XYZZ (224 B, fp28.h) on the
// table path, where everything after the accumulation kernel stays in the representation that kernel computes in (its products are ~14 % cheaper and nothing
// is converted on the device) and a launch that leaves the chip latency-bound takes FOUR lanes per addition (xyzz28_add_quad: four product levels instead of
// seven; msm.hip grp_lanes); G2's pair form (448 B) is g2.hip's PtG2.
constexpr uint32_t lg_lanes(uint32_t lanes) { return lanes == 4 ? 2u : 1u; }
struct Pt32 {
  static constexpr uint32_t BYTES = 192, WORDS = BYTES / 4; static constexpr bool TE = false;
  template <uint32_t LANES> static __device__ __forceinline__ void add(const char* pa, const char* pb, char* out) { static_assert(LANES == 2, "quad additions work on 28-bit points"); xyzz_add_pair(pa, pb, out); }
};
struct Pt28 {
  static constexpr uint32_t BYTES = 224, WORDS = BYTES / 4; static constexpr bool TE = false;
  template <uint32_t LANES> static __device__ __forceinline__ void add(const char* pa, const char* pb, char* out) { if constexpr (LANES == 4) xyzz28_add_quad(pa, pb, out); else xyzz28_add_pair(pa, pb, out); }
};
// A format whose addition reports Z3 == 0 (the extended Edwards points of msm_table.h: operands that differ by a point of even order) says so with TE = true;
// the report goes into word TE_FLAG_WORD of the sort's metadata block, zeroed with it for every chain.
static constexpr uint32_t TE_FLAG_WORD = 12;
template <class PT, class = void> struct pt_reports : std::false_type {};
template <class PT> struct pt_reports<PT, std::void_t<decltype(PT::TE)>> : std::bool_constant<PT::TE> {};

// partial[ft + i] += partial[ft + i + half] inside every multi-slice bucket: one launch per level serves both lists of the scan —
// the common one (buckets of <= 16 slices, `pairs_a` lane pairs each) and the super-heavy one (`pairs_b` each; skewed scalars).
template <class PT, uint32_t LANES = 2>
__global__ void __launch_bounds__(256) k_tree_pass(char* __restrict__ partial, const uint32_t* __restrict__ list_a, uint32_t len_a, uint32_t pairs_a,
                                                   const uint32_t* __restrict__ list_b, uint32_t len_b, uint32_t pairs_b, const uint2* __restrict__ scan_local,
                                                   const uint2* __restrict__ scan_blk, uint32_t M, const uint32_t* __restrict__ meta, uint32_t pass, uint32_t skip_b) {
  constexpr uint32_t PB = PT::BYTES;
  uint32_t op = (blockIdx.x * 256 + threadIdx.x) >> lg_lanes(LANES);
  const uint32_t ops_a = len_a * pairs_a;
  const uint32_t* list = list_a; uint32_t max_pairs = pairs_a, list_len = len_a, skip = 0;
  if (op >= ops_a) { op -= ops_a; list = list_b; max_pairs = pairs_b; list_len = len_b; skip = skip_b; }
  if (max_pairs == 0) return;
  uint32_t h = op / max_pairs, i = op % max_pairs;
  if (h >= list_len) return;
  uint32_t g = list[h];
  uint32_t ft = scan_at(scan_local, scan_blk, g).y + skip;      // skip_b = 1: the tree of slices 1.. of a super-heavy bucket (slice 0 stays the bucket's sum for the reduction; msm_run "aside")
  uint32_t fn = (g + 1 < M) ? scan_at(scan_local, scan_blk, g + 1).y : meta[0];
  uint32_t L = fn - ft;
  for (uint32_t p = 0; p < pass; ++p) L = (L + 1) >> 1;
  if (L <= 1) return;
  uint32_t half = (L + 1) >> 1;
  if (i >= L - half) return;
  char* pa = partial + (size_t)(ft + i) * PB;
  if constexpr (pt_reports<PT>::value) { if (PT::template add<LANES>(pa, pa + (size_t)half * PB, pa)) ((uint32_t*)meta)[TE_FLAG_WORD] = 1u; }
  else PT::template add<LANES>(pa, pa + (size_t)half * PB, pa);
}
// V[seg*seg_len + i] += V[seg*seg_len + i + half] for i < L - half, L = current length of every segment
template <class PT>
__global__ void __launch_bounds__(256) k_seg_tree_pass(char* __restrict__ V, uint32_t seg_len, uint32_t nseg, uint32_t L) {
  const uint32_t half = (L + 1) >> 1, pairs = L - half;
  const uint32_t op = (blockIdx.x * 256 + threadIdx.x) >> 1;
  if (op >= pairs * nseg) return;
  const uint32_t seg = op / pairs, i = op % pairs;
  char* pa = V + ((size_t)seg * seg_len + i) * PT::BYTES;
  PT::template add<2>(pa, pa + (size_t)half * PT::BYTES, pa);
}
// gathers V[w*seg_len] (the window sums) into a dense array for one D2H copy
template <class PT>
__global__ void k_gather_windows(const char* __restrict__ V, uint32_t seg_len, uint32_t W, char* __restrict__ out) {
  constexpr uint32_t Q = PT::BYTES / 16;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W * Q) return;
  uint32_t w = t / Q, q = t % Q;
  ((uint4*)out)[t] = ((const uint4*)(V + (size_t)w * seg_len * PT::BYTES))[q];
}

// The plain back end behind msm_front_finish (bucket b's sum is then the first slice of b): chunk sums, a pairwise tree per window, the W window sums to the
// host for the 2^c Horner chain, normalisation.  G, the group: PT (the format of its partial sums), HF (its host field), read (a window sum as the host's
// point), launch_chunks (its chunk kernel: V[chunk] = sum_{b in chunk} (b + 1) * S_b; `work` is the space behind the window sums), TIMED (publish phase times).
template <class G> int32_t msm_back_plain(Ctx* c, uint64_t* out_jac, Front& f, hipStream_t s) {
  using PT = typename G::PT; constexpr uint32_t PB = PT::BYTES;
  const MsmPlan& P = f.P; const uint32_t cpw = f.cpw, nchunks = f.nchunks;
  char* V = c->vbuf.as<char>(); char* Vout = V + (size_t)nchunks * PB; char* h_win = (char*)c->h_pinned + 64;
  G::launch_chunks(c, f, s, V, Vout + (size_t)P.W * PB);
  for (uint32_t L = cpw; L > 1; L = (L + 1) >> 1) {
    uint32_t pairs = (L - ((L + 1) >> 1)) * P.W;
    hipLaunchKernelGGL(k_seg_tree_pass<PT>, dim3((2 * pairs + 255) / 256), dim3(256), 0, s, V, cpw, P.W, L);
  }
  hipLaunchKernelGGL(k_gather_windows<PT>, dim3((P.W * (PB / 16) + 255) / 256), dim3(256), 0, s, V, cpw, P.W, Vout);
  HIPCHK(hipMemcpyAsync(h_win, Vout, (size_t)P.W * PB, hipMemcpyDeviceToHost, s));
  if (G::TIMED) HIPCHK(hipEventRecord(c->ev[3], s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  const auto t_host0 = std::chrono::steady_clock::now();
  // host tail: total = sum_w 2^(c*w) * S_w  (Horner from the top window), then affine normalisation
  auto total = XYZZOf<typename G::HF>::infinity();
  for (int w = (int)P.W - 1; w >= 0; --w) {
    for (int d = 0; d < win_width((int)P.c, w); ++d) total = law_double(total);          // window w spans win_width bits (balanced windows)
    total = law_add(total, G::read(h_win + (size_t)w * PB));
  }
  law_store_jacobian_normalized(out_jac, total);
  return G::TIMED ? phase_times(c, f, t_host0) : ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
