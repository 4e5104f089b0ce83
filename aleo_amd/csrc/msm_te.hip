// msm_te.hip — the whole-set tier of a pinned G1 set in twisted Edwards form (te28.h): the bucket accumulation with 7 products per mixed addition against
// 192-byte rows (y - x | y + x | 2d x y), and the table path's reduction (msm_table.h) on extended Edwards points, 9 products per addition against 14.
// Selected by PinnedBases::PreTable::te; the launch chain, its grids and its workspaces are msm.hip's.
#include "msm_table.h"
#include "msm_te.h"

namespace aleo_mi355x {

// One lane per slice, as k_accum28 (msm.hip).  The lane holds ONE row: each entry is consumed by exactly one product of the addition's first half, the next row's
// gather is issued right behind those three products and the four products of the second half hide it.  Seeds and slice sums are stored Edwards points and load /
// store as they are; the first point of an unseeded slice costs two products (te28_first).  No refusals and no slow path: the law is unified, and a Z3 == 0
// (bases outside G1) is recorded in the chain's flag word for the host to rerun the request without the table.
template <bool SEED>
__global__ void __launch_bounds__(256) k_accum28_te(const char* __restrict__ bases, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ hist,
                                                    const uint2* __restrict__ scan_local, const uint2* __restrict__ scan_blk, const uint32_t* __restrict__ total_pairs, uint32_t M,
                                                    const uint32_t* __restrict__ meta, const uint32_t* __restrict__ order, const uint32_t* __restrict__ task_g,
                                                    char* __restrict__ partial, FrontChain seed) {
  uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= meta[0]) return;
  const uint32_t sid = order[t], g = task_g[sid];
  uint2 st = scan_at(scan_local, scan_blk, g);
  uint32_t cnt = hist[g], m = slices_of(cnt, pick_rule(total_pairs, M)), k = sid - st.y;
  uint32_t j0 = (uint32_t)(((uint64_t)k * cnt) / m), j1 = (uint32_t)(((uint64_t)(k + 1) * cnt) / m);
  const uint32_t* run = sorted + st.x;
  uint32_t e = run[j0];
  const char* row = bases + (size_t)(e & 0x7fffffffu) * TE_ROW;
  F28 r0 = load_te28_entry(row), r1 = load_te28_entry(row + 64), r2 = load_te28_entry(row + 128);
  TE28 acc; bool z = false, seeded = false;
  uint32_t j = j0;
  if constexpr (SEED) {      // first slice of the bucket: continue from what the earlier chunks of this request summed into the same bucket
    const char* sp = k == 0 ? chain_sum(seed, g) : nullptr;
    if (sp) { acc.X = load_f28(sp); acc.Y = load_f28(sp + 56); acc.Z = load_f28(sp + 112); acc.T = load_f28(sp + 168); seeded = true; }
  }
  if (!seeded) {
    te28_row_negate_if(e >> 31, r0, r1, r2);
    te28_first(acc, r0, r1, r2);
    if (++j < j1) { e = run[j]; row = bases + (size_t)(e & 0x7fffffffu) * TE_ROW; r0 = load_te28_entry(row); r1 = load_te28_entry(row + 64); r2 = load_te28_entry(row + 128); }
  }
  for (; j < j1; ++j) {
    te28_row_negate_if(e >> 31, r0, r1, r2);
    const TE28Half h = te28_madd_rows(acc, r0, r1, r2);
    if (j + 1 < j1) { e = run[j + 1]; row = bases + (size_t)(e & 0x7fffffffu) * TE_ROW; r0 = load_te28_entry(row); r1 = load_te28_entry(row + 64); r2 = load_te28_entry(row + 128); }
    z |= te28_madd_finish(acc, h);
  }
  if (z) *te_flag_of(meta) = 1u;
  char* out = partial + (size_t)sid * 224;
  store_f28(out, acc.X); store_f28(out + 56, acc.Y); store_f28(out + 112, acc.Z); store_f28(out + 168, acc.T);      // every coordinate exact < 2q: the stored invariant of te28.h
}

template <uint32_t LANES>
__global__ void __launch_bounds__(256) k_tree_rest_te(char* __restrict__ partial, const uint32_t* __restrict__ list, uint32_t list_len, const uint2* __restrict__ scan_local,
                                                      const uint2* __restrict__ scan_blk, uint32_t M, const uint32_t* __restrict__ meta) {
  tree_rest_body<PtTE, LANES>(partial, list, list_len, scan_local, scan_blk, M, meta);
}
__global__ void k_gather_super_te(const char* __restrict__ partial, const uint32_t* __restrict__ list, uint32_t len, const uint2* __restrict__ scan_local,
                                  const uint2* __restrict__ scan_blk, uint32_t* __restrict__ dst, const uint32_t* __restrict__ flag) {
  gather_super_body(partial, list, len, scan_local, scan_blk, dst, flag);
}
template <uint32_t LANES>
__global__ void __launch_bounds__(256) k_bucket_chunks_te(const char* __restrict__ partial, const uint32_t* __restrict__ hist, const uint2* __restrict__ scan_local,
                                                          const uint2* __restrict__ scan_blk, uint32_t B, uint32_t S, uint32_t nchunks_total, char* __restrict__ V,
                                                          uint32_t v_set_stride, char* __restrict__ Vrun, FrontChain older, uint32_t flag_off) {
  bucket_chunks_body<PtTE, LANES>(partial, hist, scan_local, scan_blk, B, S, nchunks_total, V, v_set_stride, Vrun, older, flag_off);
}
template <uint32_t LANES>
__global__ void __launch_bounds__(256) k_prog_pass_te(const char* __restrict__ node, uint32_t node_set_stride, const char* __restrict__ A, uint32_t a_set_stride,
                                                      const char* __restrict__ T, uint32_t t_set_stride, uint32_t nT, uint32_t L, uint32_t nsets,
                                                      char* __restrict__ out, uint32_t out_set_stride, uint32_t* __restrict__ flag) {
  prog_pass_body<PtTE, LANES>(node, node_set_stride, A, a_set_stride, T, t_set_stride, nT, L, nsets, out, out_set_stride, flag);
}
__global__ void __launch_bounds__(256) k_prog_pass2_te(const char* __restrict__ node, uint32_t node_set_stride, const char* __restrict__ A, uint32_t a_set_stride,
                                                       const char* __restrict__ T, uint32_t t_set_stride, uint32_t nT, uint32_t L, uint32_t nsets,
                                                       char* __restrict__ out, uint32_t out_set_stride, uint32_t* __restrict__ flag) {
  prog_pass2_body<PtTE>(node, node_set_stride, A, a_set_stride, T, t_set_stride, nT, L, nsets, out, out_set_stride, flag);
}
template <uint32_t LANES>
__global__ void __launch_bounds__(128 * LANES) k_prog_final_te(const char* __restrict__ in, uint32_t in_set_stride, uint32_t L, uint32_t nT, uint32_t lgL, uint32_t nsets,
                                                               char* __restrict__ out, const uint32_t* __restrict__ flag, uint32_t* __restrict__ host_flags) {
  prog_final_body<PtTE, LANES>(in, in_set_stride, L, nT, lgL, nsets, out, flag, host_flags);
}

void te_accum(bool seeded, hipStream_t s, const char* bases, const SortPhase& sp, char* partial, const FrontChain& seed) {
  hipLaunchKernelGGL(seeded ? k_accum28_te<true> : k_accum28_te<false>, dim3(sp.slice_blocks), dim3(256), 0, s, bases, sp.sorted, sp.hist, sp.scan_local, sp.scan_blk, sp.total_pairs, sp.M,
                     sp.meta, sp.order, sp.task_g, partial, seeded ? seed : FrontChain{});
}
void te_tree_pass(uint32_t lanes, uint64_t ops, hipStream_t s, char* partial, const uint32_t* list_a, uint32_t len_a, uint32_t pairs_a, const uint32_t* list_b, uint32_t len_b,
                  uint32_t pairs_b, const SortPhase& sp, uint32_t pass, uint32_t skip_b) {
  launch_grp(lanes, k_tree_pass<PtTE, 4>, k_tree_pass<PtTE, 2>, ops, s, partial, list_a, len_a, pairs_a, list_b, len_b, pairs_b, sp.scan_local, sp.scan_blk, sp.M, sp.meta, pass, skip_b);
}
void te_tree_rest(hipStream_t s, char* partial, const uint32_t* list, uint32_t list_len, const SortPhase& sp) {
  hipLaunchKernelGGL(k_tree_rest_te<4>, dim3((uint32_t)((4ull * list_len + 255) / 256)), dim3(256), 0, s, partial, list, list_len, sp.scan_local, sp.scan_blk, sp.M, sp.meta);
}
void te_gather_super(hipStream_t s, const char* partial, uint32_t len, const SortPhase& sp, uint32_t* dst) {
  hipLaunchKernelGGL(k_gather_super_te, dim3((len * 57 + 255) / 256), dim3(256), 0, s, partial, sp.super_list, len, sp.scan_local, sp.scan_blk, dst, te_flag_of(sp.meta));
}
void te_bucket_chunks(uint32_t lanes, hipStream_t s, const char* partial, const SortPhase& sp, uint32_t B, uint32_t S, uint32_t nchunks, char* V, uint32_t v_set_stride, char* Vrun,
                      const FrontChain& older) {
  const uint32_t per_block = lanes == 4 ? 32u : 64u, flag_off = (uint32_t)(sp.meta - sp.hist) + TE_FLAG_WORD;      // (the same offset in every chunk of a request: one M, one layout)
  hipLaunchKernelGGL(lanes == 4 ? k_bucket_chunks_te<4> : k_bucket_chunks_te<2>, dim3((nchunks + per_block - 1) / per_block), dim3(256), 0, s, partial, sp.hist, sp.scan_local, sp.scan_blk,
                     B, S, nchunks, V, v_set_stride, Vrun, older, flag_off);
}
void te_prog_pass(uint32_t lanes, uint64_t ops, hipStream_t s, const char* node, uint32_t node_ss, const char* A, uint32_t a_ss, const char* T, uint32_t t_ss, uint32_t nT, uint32_t L,
                  uint32_t nsets, char* out, uint32_t out_ss, const SortPhase& sp) {
  launch_grp(lanes, k_prog_pass_te<4>, k_prog_pass_te<2>, ops, s, node, node_ss, A, a_ss, T, t_ss, nT, L, nsets, out, out_ss, te_flag_of(sp.meta));
}
void te_prog_pass2(uint64_t octs, hipStream_t s, const char* node, uint32_t node_ss, const char* A, uint32_t a_ss, const char* T, uint32_t t_ss, uint32_t nT, uint32_t L, uint32_t nsets,
                   char* out, uint32_t out_ss, const SortPhase& sp) {
  hipLaunchKernelGGL(k_prog_pass2_te, dim3((uint32_t)((octs + 31) / 32)), dim3(256), 0, s, node, node_ss, A, a_ss, T, t_ss, nT, L, nsets, out, out_ss, te_flag_of(sp.meta));
}
void te_prog_final(uint32_t blocks, hipStream_t s, const char* in, uint32_t in_ss, uint32_t L, uint32_t nT, uint32_t lgL, uint32_t nsets, char* out, const SortPhase& sp,
                   uint32_t* host_flags) {
  hipLaunchKernelGGL(k_prog_final_te<4>, dim3(blocks), dim3(512), 0, s, in, in_ss, L, nT, lgL, nsets, out, (const uint32_t*)te_flag_of(sp.meta), host_flags);
}

}  // namespace aleo_mi355x
