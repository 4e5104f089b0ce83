// g2.h — the G2 multi-scalar multiplication (g2.hip) as api.hip and bases.hip call it.
#pragma once
#include "ctx.h"

namespace aleo_mi355x {
// d_rows28: the set's resident 28-bit rows (a pinned G2 set), else built per call
int32_t msm_g2_run(Ctx* c, uint64_t* out_jac36, const void* d_xy, const uint8_t* d_inf, const void* d_scalars, size_t n, hipStream_t s, const void* d_rows28 = nullptr);
int32_t g2_rows_to28(const void* d_xy192, void* d_dst224, size_t n, hipStream_t s);
int32_t g2_sum_host(uint64_t* out36, const uint64_t* pts36, size_t count);
int32_t selftest_g2pair(Ctx* c, const void* aff192_host, uint32_t n, uint32_t npairs, uint32_t* failures2);      // [0] pairs that disagreed, [1] OR of the failing steps
int32_t g2_unpack200(const void* d_rows200, void* d_xy192, void* d_flags, uint32_t* d_count, size_t n, hipStream_t s);      // 200-byte G2Affine rows -> 192-byte rows + flag bytes + their count
}  // namespace aleo_mi355x
