// selftest_f28.hip — test hook: the point formulas of fp28.h on rows the caller built, raw limbs in and raw limbs out (aleo_mi355x_selftest_f28_rows).
//
// The other self-tests of the 28-bit form (msm.hip) draw pseudo-random canonical operands on the device and compare one hand-written form with another.
// Here the HOST chooses every limb — representatives near 2q / 6q / 12q, limbs near 3 * 2^28, 2-torsion points, identities — and checks what comes back
// against the group law in integers (tests/test_gpu_fp28_extremes.py); the device converts nothing.  A unit of its own, so that the code objects of the
// units that ship kernels stay what they were.
#include "ctx.h"
#include "fp28.h"

namespace aleo_mi355x {

static constexpr uint32_t PB28 = 224;

// one quad per addition: all four lanes run the quad form, its lanes 0 and 1 the pair form as well, into separate outputs
__global__ void __launch_bounds__(256) k_f28_rows_add(const char* __restrict__ a, const char* __restrict__ b, uint32_t n, char* __restrict__ out_pair, char* __restrict__ out_quad) {
  const uint32_t op = (blockIdx.x * 256 + threadIdx.x) >> 2, q = threadIdx.x & 3u;
  if (op >= n) return;                                       // quad-uniform
  const size_t o = (size_t)op * PB28;
  xyzz28_add_quad(a + o, b + o, out_quad + o);
  if (q < 2) xyzz28_add_pair(a + o, b + o, out_pair + o);
}
// one lane per mixed addition: acc (224-byte row) + the 112-byte entry x | y
__global__ void __launch_bounds__(256) k_f28_rows_madd(const char* __restrict__ acc224, const char* __restrict__ pt112, uint32_t n, char* __restrict__ out224, uint8_t* __restrict__ ok) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const char* p = acc224 + (size_t)t * PB28;
  XYZZ28 acc; acc.X = load_f28(p); acc.Y = load_f28(p + 56); acc.ZZ = load_f28(p + 112); acc.ZZZ = load_f28(p + 168);
  F28 x, y; load_affine28(pt112 + (size_t)t * 112, x, y);
  const bool r = xyzz28_madd_fast(acc, x, y);
  store_xyzz28(out224 + (size_t)t * PB28, acc);
  ok[t] = r ? 1 : 0;
}

int32_t selftest_f28_rows(Ctx* c, const void* a224, const void* b224, uint32_t n_add, void* out_pair224, void* out_quad224,
                          const void* acc224, const void* pt112, uint32_t n_madd, void* out_acc224, uint8_t* ok_u8) {
  int32_t rc;
  if (n_add) {
    const size_t bytes = (size_t)n_add * PB28; DevTmp a, b, op, oq;
    if ((rc = a.alloc(bytes)) || (rc = b.alloc(bytes)) || (rc = op.alloc(bytes)) || (rc = oq.alloc(bytes))) return rc;
    HIPCHK(hipMemcpyAsync(a.p, a224, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.p, b224, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(op.p, 0xA5, bytes, c->stream));      // a coordinate nobody stored shows
    HIPCHK(hipMemsetAsync(oq.p, 0xA5, bytes, c->stream));
    hipLaunchKernelGGL(k_f28_rows_add, dim3((n_add + 63) / 64), dim3(256), 0, c->stream, (const char*)a.p, (const char*)b.p, n_add, (char*)op.p, (char*)oq.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_pair224, op.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_quad224, oq.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (n_madd) {
    DevTmp acc, pt, out, ok;
    if ((rc = acc.alloc((size_t)n_madd * PB28)) || (rc = pt.alloc((size_t)n_madd * 112)) || (rc = out.alloc((size_t)n_madd * PB28)) || (rc = ok.alloc(n_madd))) return rc;
    HIPCHK(hipMemcpyAsync(acc.p, acc224, (size_t)n_madd * PB28, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(pt.p, pt112, (size_t)n_madd * 112, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(out.p, 0xA5, (size_t)n_madd * PB28, c->stream));
    HIPCHK(hipMemsetAsync(ok.p, 0xA5, n_madd, c->stream));
    hipLaunchKernelGGL(k_f28_rows_madd, dim3((n_madd + 255) / 256), dim3(256), 0, c->stream, (const char*)acc.p, (const char*)pt.p, n_madd, (char*)out.p, (uint8_t*)ok.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_acc224, out.p, (size_t)n_madd * PB28, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ok_u8, ok.p, n_madd, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
