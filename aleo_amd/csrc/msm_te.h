// msm_te.h — the kernels of the whole-set tier in twisted Edwards form (msm_te.hip: te28.h's accumulation, msm_table.h's bodies for PtTE), as msm.hip
// launches them where the chain's tier is Edwards.  Same grids, same order, same workspaces as the XYZZ kernels they stand in for.
#pragma once
#include "msm_chain.h"

namespace aleo_mi355x {
#pragma GCC visibility push(hidden)
void te_accum(bool seeded, hipStream_t s, const char* bases, const SortPhase& sp, char* partial, const FrontChain& seed);
void te_tree_pass(uint32_t lanes, uint64_t ops, hipStream_t s, char* partial, const uint32_t* list_a, uint32_t len_a, uint32_t pairs_a, const uint32_t* list_b, uint32_t len_b,
                  uint32_t pairs_b, const SortPhase& sp, uint32_t pass, uint32_t skip_b);
void te_tree_rest(hipStream_t s, char* partial, const uint32_t* list, uint32_t list_len, const SortPhase& sp);
void te_gather_super(hipStream_t s, const char* partial, uint32_t len, const SortPhase& sp, uint32_t* dst);      // dst[len * 57]: the side stream's Z3 == 0 word
void te_bucket_chunks(uint32_t lanes, hipStream_t s, const char* partial, const SortPhase& sp, uint32_t B, uint32_t S, uint32_t nchunks, char* V, uint32_t v_set_stride, char* Vrun,
                      const FrontChain& older);
void te_prog_pass(uint32_t lanes, uint64_t ops, hipStream_t s, const char* node, uint32_t node_ss, const char* A, uint32_t a_ss, const char* T, uint32_t t_ss, uint32_t nT, uint32_t L,
                  uint32_t nsets, char* out, uint32_t out_ss, const SortPhase& sp);
void te_prog_pass2(uint64_t octs, hipStream_t s, const char* node, uint32_t node_ss, const char* A, uint32_t a_ss, const char* T, uint32_t t_ss, uint32_t nT, uint32_t L, uint32_t nsets,
                   char* out, uint32_t out_ss, const SortPhase& sp);
void te_prog_final(uint32_t blocks, hipStream_t s, const char* in, uint32_t in_ss, uint32_t L, uint32_t nT, uint32_t lgL, uint32_t nsets, char* out, const SortPhase& sp,
                   uint32_t* host_flags);      // host_flags[block]: every Z3 == 0 report of the chain up to and including that block
#pragma GCC visibility pop
}  // namespace aleo_mi355x
