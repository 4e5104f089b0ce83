// selftest_g2p.hip — test hook: the G2 lane-pair formulas of g2p28.h on rows the caller built, raw limbs in and raw limbs out (aleo_mi355x_selftest_g2p_rows).
//
// aleo_mi355x_selftest_g2pair (g2.hip) compares the pair form with the one-lane 32-bit device code on canonical points of the prime-order subgroup: no
// component is ever 0, no y is 0, no representative is lifted.  Here the HOST chooses every limb — each component lifted on its own up to 12q / 6q / 2q,
// 2-torsion points, x = (0, 0), identities, operands whose ZZ3 has exactly one zero component, P == +-acc, the negated entry of y = 0 — and checks what
// comes back against the group law in integers (tests/test_gpu_g2p_extremes.py); the device converts nothing.  A unit of its own, so that g2.hip's code
// object stays what it was: this unit compiles its own copy of the same header source.
#include "ctx.h"
#include "g2p28.h"

namespace aleo_mi355x {

// one lane pair per row, 64 rows per block
__global__ void __launch_bounds__(128) k_g2p_rows_add(const char* __restrict__ a, const char* __restrict__ b, uint32_t n, char* __restrict__ out) {
  const uint32_t t = (blockIdx.x * 128 + threadIdx.x) >> 1;
  if (t >= n) return;                                        // pair-uniform
  const size_t o = (size_t)t * P2B;
  g2p_add_any(a + o, b + o, out + o);
}
__global__ void __launch_bounds__(128) k_g2p_rows_double(const char* __restrict__ a, uint32_t n, char* __restrict__ out) {
  const uint32_t t = (blockIdx.x * 128 + threadIdx.x) >> 1;
  if (t >= n) return;
  const size_t o = (size_t)t * P2B;
  g2p_double_any(a + o, out + o);
}
// acc (448-byte row) + the 224-byte entry x.a | y.a | x.b | y.b, negated first where neg[t]; both lanes write what the formula returned to them
__global__ void __launch_bounds__(128) k_g2p_rows_madd(const char* __restrict__ acc448, const char* __restrict__ ent224, const uint8_t* __restrict__ neg, uint32_t n,
                                                       char* __restrict__ out448, uint8_t* __restrict__ ok2) {
  const uint32_t t = (blockIdx.x * 128 + threadIdx.x) >> 1; const bool odd = threadIdx.x & 1;
  if (t >= n) return;
  XYZZ2P acc = g2p_load(acc448 + (size_t)t * P2B, odd);
  F28 x, y; load_affine28(ent224 + (size_t)t * ROW2 + (odd ? 112 : 0), x, y);
  if (neg[t]) y = g2p_negate_entry(y);
  const bool r = g2p_madd_fast(acc, x, y, odd);
  g2p_store(out448 + (size_t)t * P2B, odd, acc);
  ok2[2 * t + (odd ? 1 : 0)] = r ? 1 : 0;
}

int32_t selftest_g2p_rows(Ctx* c, const void* a448, const void* b448, uint32_t n_add, void* out_add448, const void* d448, uint32_t n_dbl, void* out_dbl448,
                          const void* acc448, const void* ent224, const uint8_t* neg_u8, uint32_t n_madd, void* out_acc448, uint8_t* ok2_u8) {
  int32_t rc;
  if (n_add) {
    const size_t bytes = (size_t)n_add * P2B; DevTmp a, b, o;
    if ((rc = a.alloc(bytes)) || (rc = b.alloc(bytes)) || (rc = o.alloc(bytes))) return rc;
    HIPCHK(hipMemcpyAsync(a.p, a448, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.p, b448, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(o.p, 0xA5, bytes, c->stream));       // a coordinate nobody stored shows
    hipLaunchKernelGGL(k_g2p_rows_add, dim3((n_add + 63) / 64), dim3(128), 0, c->stream, (const char*)a.p, (const char*)b.p, n_add, (char*)o.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_add448, o.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (n_dbl) {
    const size_t bytes = (size_t)n_dbl * P2B; DevTmp a, o;
    if ((rc = a.alloc(bytes)) || (rc = o.alloc(bytes))) return rc;
    HIPCHK(hipMemcpyAsync(a.p, d448, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(o.p, 0xA5, bytes, c->stream));
    hipLaunchKernelGGL(k_g2p_rows_double, dim3((n_dbl + 63) / 64), dim3(128), 0, c->stream, (const char*)a.p, n_dbl, (char*)o.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_dbl448, o.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (n_madd) {
    DevTmp acc, ent, neg, out, ok;
    if ((rc = acc.alloc((size_t)n_madd * P2B)) || (rc = ent.alloc((size_t)n_madd * ROW2)) || (rc = neg.alloc(n_madd)) || (rc = out.alloc((size_t)n_madd * P2B)) || (rc = ok.alloc(2 * (size_t)n_madd))) return rc;
    HIPCHK(hipMemcpyAsync(acc.p, acc448, (size_t)n_madd * P2B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(ent.p, ent224, (size_t)n_madd * ROW2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(neg.p, neg_u8, n_madd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(out.p, 0xA5, (size_t)n_madd * P2B, c->stream));
    HIPCHK(hipMemsetAsync(ok.p, 0xA5, 2 * (size_t)n_madd, c->stream));
    hipLaunchKernelGGL(k_g2p_rows_madd, dim3((n_madd + 63) / 64), dim3(128), 0, c->stream, (const char*)acc.p, (const char*)ent.p, (const uint8_t*)neg.p, n_madd, (char*)out.p, (uint8_t*)ok.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_acc448, out.p, (size_t)n_madd * P2B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ok2_u8, ok.p, 2 * (size_t)n_madd, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
