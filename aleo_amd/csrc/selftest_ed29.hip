// selftest_ed29.hip — test hook: the 29-bit-limb field product and the helpers of edwards29.h on rows the caller built, raw limbs in and raw limbs out
// (aleo_mi355x_selftest_ed29_rows).
//
// Every account-side lane (records, serial numbers, commitments, signatures, accounts, key ciphertexts, plaintexts) reaches this arithmetic with canonical
// inputs and whatever its own formulas produce.  Here the HOST chooses every limb — multiplicands with limbs of 5 * 2^29 - 1 next to 2^261, multipliers at the
// 3 r edge, coordinates lifted to the largest representative their contract allows, the identity, the points of order 2 and 4 — and checks what comes back against
// integers (tests/test_gpu_ed29_extremes.py); the device converts nothing.  One lane per row.  A unit of its own, so that the code objects of the units that ship
// kernels stay what they were.
#include "ctx.h"
#include "edwards29.h"
#include <cstring>

namespace aleo_mi355x {

static constexpr uint32_t EL29 = 9, PT29 = 36;               // words of an element, of a point X | Y | Z | T

__device__ __forceinline__ F29 row_load(const uint32_t* __restrict__ p) { return f29_limbs(p); }
__device__ __forceinline__ void row_store(uint32_t* __restrict__ p, const F29& a) {
#pragma unroll
  for (int i = 0; i < 9; ++i) p[i] = a.v[i];
}
__device__ __forceinline__ Ed29 point_load(const uint32_t* __restrict__ p) { Ed29 e; e.X = row_load(p); e.Y = row_load(p + 9); e.Z = row_load(p + 18); e.T = row_load(p + 27); return e; }
__device__ __forceinline__ void point_store(uint32_t* __restrict__ p, const Ed29& e) { row_store(p, e.X); row_store(p + 9, e.Y); row_store(p + 18, e.Z); row_store(p + 27, e.T); }

__global__ void __launch_bounds__(256) k_ed29_rows_mul(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  row_store(out + (size_t)t * EL29, f29_mul(row_load(a + (size_t)t * EL29), row_load(b + (size_t)t * EL29)));
}
__global__ void __launch_bounds__(256) k_ed29_rows_tidy(const uint32_t* __restrict__ a, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  F29 v = row_load(a + (size_t)t * EL29); f29_tidy(v);
  row_store(out + (size_t)t * EL29, v);
}
__global__ void __launch_bounds__(256) k_ed29_rows_canonical(const uint32_t* __restrict__ a, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  row_store(out + (size_t)t * EL29, f29_canonical(row_load(a + (size_t)t * EL29)));
}
// p + q or p - q: q goes through ed29_cache with the 2d the caller gave
__global__ void __launch_bounds__(256) k_ed29_rows_add(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q, const uint8_t* __restrict__ neg, F29Arg d2, uint32_t n,
                                                       uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  Ed29 acc = point_load(p + (size_t)t * PT29);
  ed29_add(acc, ed29_cache(point_load(q + (size_t)t * PT29), f29_limbs(d2.v)), neg[t] != 0);
  point_store(out + (size_t)t * PT29, acc);
}
// 2 p, with T or without: the T that was not asked for is the one that came in
__global__ void __launch_bounds__(256) k_ed29_rows_dbl(const uint32_t* __restrict__ p, const uint8_t* __restrict__ want_t, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  Ed29 acc = point_load(p + (size_t)t * PT29);
  ed29_dbl(acc, want_t[t] != 0);
  point_store(out + (size_t)t * PT29, acc);
}

// `words` words per row: rows up, output filled with 0xA5 (a limb nobody stored shows), and after the launch the output down
struct Rows {
  DevTmp in[2], flags, out; size_t bytes = 0; uint32_t n = 0;
  int32_t up(Ctx* c, uint32_t n_, uint32_t words, const void* a, const void* b, const uint8_t* f) {
    int32_t rc; n = n_; bytes = (size_t)n * words * 4;
    if ((rc = in[0].alloc(bytes)) || (rc = out.alloc(bytes)) || (b && (rc = in[1].alloc(bytes))) || (f && (rc = flags.alloc(n)))) return rc;
    HIPCHK(hipMemcpyAsync(in[0].p, a, bytes, hipMemcpyHostToDevice, c->stream));
    if (b) HIPCHK(hipMemcpyAsync(in[1].p, b, bytes, hipMemcpyHostToDevice, c->stream));
    if (f) HIPCHK(hipMemcpyAsync(flags.p, f, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(out.p, 0xA5, bytes, c->stream));
    return ALEO_MI355X_OK;
  }
  int32_t down(Ctx* c, void* host) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host, out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ALEO_MI355X_OK;
  }
  dim3 grid() const { return dim3((n + 255) / 256); }
};

int32_t selftest_ed29_rows(Ctx* c, const void* mul_a36, const void* mul_b36, uint32_t n_mul, void* out_mul36, const void* tidy36, uint32_t n_tidy, void* out_tidy36,
                           const void* canon36, uint32_t n_canon, void* out_canon36, const void* p144, const void* q144, const uint8_t* neg_u8, const void* d2_36,
                           uint32_t n_add, void* out_add144, const void* dbl144, const uint8_t* want_t_u8, uint32_t n_dbl, void* out_dbl144) {
  int32_t rc;
  if (n_mul) {
    Rows r; if ((rc = r.up(c, n_mul, EL29, mul_a36, mul_b36, nullptr))) return rc;
    hipLaunchKernelGGL(k_ed29_rows_mul, r.grid(), dim3(256), 0, c->stream, (const uint32_t*)r.in[0].p, (const uint32_t*)r.in[1].p, n_mul, (uint32_t*)r.out.p);
    if ((rc = r.down(c, out_mul36))) return rc;
  }
  if (n_tidy) {
    Rows r; if ((rc = r.up(c, n_tidy, EL29, tidy36, nullptr, nullptr))) return rc;
    hipLaunchKernelGGL(k_ed29_rows_tidy, r.grid(), dim3(256), 0, c->stream, (const uint32_t*)r.in[0].p, n_tidy, (uint32_t*)r.out.p);
    if ((rc = r.down(c, out_tidy36))) return rc;
  }
  if (n_canon) {
    Rows r; if ((rc = r.up(c, n_canon, EL29, canon36, nullptr, nullptr))) return rc;
    hipLaunchKernelGGL(k_ed29_rows_canonical, r.grid(), dim3(256), 0, c->stream, (const uint32_t*)r.in[0].p, n_canon, (uint32_t*)r.out.p);
    if ((rc = r.down(c, out_canon36))) return rc;
  }
  if (n_add) {
    F29Arg d2; std::memcpy(d2.v, d2_36, sizeof d2.v);
    Rows r; if ((rc = r.up(c, n_add, PT29, p144, q144, neg_u8))) return rc;
    hipLaunchKernelGGL(k_ed29_rows_add, r.grid(), dim3(256), 0, c->stream, (const uint32_t*)r.in[0].p, (const uint32_t*)r.in[1].p, (const uint8_t*)r.flags.p, d2, n_add, (uint32_t*)r.out.p);
    if ((rc = r.down(c, out_add144))) return rc;
  }
  if (n_dbl) {
    Rows r; if ((rc = r.up(c, n_dbl, PT29, dbl144, nullptr, want_t_u8))) return rc;
    hipLaunchKernelGGL(k_ed29_rows_dbl, r.grid(), dim3(256), 0, c->stream, (const uint32_t*)r.in[0].p, (const uint8_t*)r.flags.p, n_dbl, (uint32_t*)r.out.p);
    if ((rc = r.down(c, out_dbl144))) return rc;
  }
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
