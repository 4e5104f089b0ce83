// frops.h — the hosts of the Fr kernels, as api.hip and the prover (varuna*.hip) call them.  Every function queues its kernels on `s` and returns without
// synchronising; pointers named d_* are device memory, constants are 32-byte Montgomery values on the host.
#pragma once
#include "ctx.h"

namespace aleo_mi355x {

// frops.hip: element-wise operations, batch inversion, geometric sequences, gathers, the random stream, single elements
int32_t fr_vec_op(Ctx* c, void* d_dst, const void* d_a, const void* d_b, size_t n, int32_t op, hipStream_t s);
int32_t fr_lin(Ctx* c, void* d_dst, size_t n, const void* c0, const void* c1, const void* d_a, const void* c2, const void* d_b, hipStream_t s);
int32_t fr_lincomb(Ctx* c, void* d_dst, size_t n, const void* c0, const void* const* d_terms, const size_t* lens, const void* coeffs, size_t k, hipStream_t s);
int32_t fr_add_tiled(Ctx* c, void* d_dst, size_t n, const void* d_src, size_t n_src, hipStream_t s);
int32_t fr_sub_mul(Ctx* c, void* d_dst, const void* d_a, const void* d_b, const void* d_m, size_t n, hipStream_t s);
int32_t fr_scale_rows(Ctx* c, void* d_dst, const void* d_src, size_t n, size_t rows, const void* consts_mont, hipStream_t s);
int32_t fr_batch_inverse(Ctx* c, void* d_inout, size_t n, hipStream_t s);
int32_t fr_powers(Ctx* c, void* d_dst, size_t n, const void* first, const void* ratio, hipStream_t s);
int32_t fr_gather_mul(Ctx* c, void* d_dst, size_t n, const void* d_scale, const void* d_t1, const void* d_idx1, const void* d_t2, const void* d_idx2, hipStream_t s);
int32_t fr_gather_mul3(Ctx* c, void* const* d_dst, const size_t* n, const void* const* d_scale, const void* d_t1, const void* const* d_idx1, const void* d_t2, const void* const* d_idx2, uint32_t count, hipStream_t s);      // the same for up to three ranges (scale and both tables present) in one launch
int32_t fr_random(Ctx* c, void* d_dst, size_t n, const uint8_t* seed32, uint64_t first, int32_t mont, hipStream_t s);
int32_t fr_scatter_to_mont(Ctx* c, void* d_dst, const void* d_src, const void* d_pos, size_t n, void* d_flag, hipStream_t s);
int32_t fr_pick(Ctx* c, void* dst_devptr, const void* const* d_src, size_t count, hipStream_t s);
int32_t launch_fq_mul(Ctx* c, void* r, const void* a, const void* b, size_t n);      // test only: host buffers, blocking
int32_t launch_fr_mul(Ctx* c, void* r, const void* a, const void* b, size_t n);
// fr_spmv.hip
int32_t fr_spmv(Ctx* c, void* d_y, const void* d_row_ptr, const void* d_col, const void* d_vals, const void* d_x, size_t rows, hipStream_t s, size_t max_row = 0);      // max_row: bound of the longest row (0 = unknown): skips the long / huge-row launches that cannot have work
// fr_divide.hip
int32_t fr_divide_by_linear(Ctx* c, void* d_q, void* d_eval, const void* d_p, size_t n, const void* z_mont32, hipStream_t s);
int32_t fr_divide_by_linear_many(Ctx* c, void* const* d_q, void* const* d_eval, const void* const* d_p, const size_t* n, const void* const* z_mont32, size_t count, hipStream_t s);      // <= 4 divisions in three launches
int32_t fr_eval_batch(Ctx* c, void* d_out, const void* const* d_polys, const size_t* lens, const void* z_mont, size_t k, hipStream_t s);
// ahp_kernels.hip
int32_t ahp_first_sumcheck(Ctx* c, void* d_dst, size_t n, const void* d_r, const void* d_a, const void* d_b, const void* d_t, const void* d_z, const void* eta_b, const void* eta_c, hipStream_t s);
int32_t ahp_matrix_sumcheck(Ctx* c, void* d_dst, size_t n, const void* const* d_index, size_t index_stride_elems, const void* const* d_f, const void* consts, hipStream_t s);
int32_t fr_blind_rows(Ctx* c, void* d_dst, const void* d_src, size_t n, size_t rows, const void* rho_mont, hipStream_t s);
int32_t ahp_sumcheck_operands(Ctx* c, void* d_dst, const void* d_wit, const void* d_xp, size_t n, size_t n_x, size_t instances, hipStream_t s);
int32_t fr_split_quotient(Ctx* c, void* d_hq, void* d_rq, const void* d_q, const void* d_mask, size_t n, void* host_sum_devptr, hipStream_t s);

}  // namespace aleo_mi355x
