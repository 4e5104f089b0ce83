// selftest_te28.hip — test hook: the Edwards-form formulas of te28.h on rows the caller built, raw limbs in and raw limbs out (aleo_mi355x_selftest_te28_rows).
// The counterpart of selftest_f28.hip: the HOST chooses every limb — representatives next to 2q, the identity, P = +-acc, negated rows, the first and the last
// quad (lane) of a wave — and checks what comes back against the group law in integers (tests/test_gpu_te28_extremes.py); the device converts nothing.
#include "ctx.h"
#include "te28.h"

namespace aleo_mi355x {

static constexpr uint32_t PB28 = 224;

// one quad per addition: all four lanes run the quad form, its lanes 0 and 1 the pair form as well, into separate outputs; z[i]: bit 0 pair, bit 1 quad reported Z3 == 0
__global__ void __launch_bounds__(256) k_te28_rows_add(const char* __restrict__ a, const char* __restrict__ b, uint32_t n, char* __restrict__ out_pair, char* __restrict__ out_quad, uint32_t* __restrict__ z) {
  const uint32_t op = (blockIdx.x * 256 + threadIdx.x) >> 2, q = threadIdx.x & 3u;
  if (op >= n) return;                                       // quad-uniform
  const size_t o = (size_t)op * PB28;
  if (te28_add_quad(a + o, b + o, out_quad + o)) atomicOr(z + op, 2u);
  if (q < 2) { if (te28_add_pair(a + o, b + o, out_pair + o)) atomicOr(z + op, 1u); }
}
// one lane per mixed addition: acc (224-byte row) + the entry r0 | r1 | r2 (168 bytes), negated on the device when how[i] & 1; how[i] & 2: the entry starts a slice
// (te28_first, acc ignored).  z[i] = what te28_madd returned.
__global__ void __launch_bounds__(256) k_te28_rows_madd(const char* __restrict__ acc224, const char* __restrict__ row168, const uint8_t* __restrict__ how, uint32_t n, char* __restrict__ out224,
                                                        uint8_t* __restrict__ z) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const char* p = acc224 + (size_t)t * PB28; const char* e = row168 + (size_t)t * 168;
  TE28 acc; acc.X = load_f28(p); acc.Y = load_f28(p + 56); acc.Z = load_f28(p + 112); acc.T = load_f28(p + 168);
  F28 r0 = load_f28(e), r1 = load_f28(e + 56), r2 = load_f28(e + 112);
  te28_row_negate_if(how[t] & 1u, r0, r1, r2);
  bool r = false;
  if (how[t] & 2u) te28_first(acc, r0, r1, r2); else r = te28_madd(acc, r0, r1, r2);
  char* o = out224 + (size_t)t * PB28;
  store_f28(o, acc.X); store_f28(o + 56, acc.Y); store_f28(o + 112, acc.Z); store_f28(o + 168, acc.T);
  z[t] = r ? 1 : 0;
}

int32_t selftest_te28_rows(Ctx* c, const void* a224, const void* b224, uint32_t n_add, void* out_pair224, void* out_quad224, uint32_t* z_add_u32,
                           const void* acc224, const void* row168, const uint8_t* how_u8, uint32_t n_madd, void* out_acc224, uint8_t* z_madd_u8) {
  int32_t rc;
  if (n_add) {
    const size_t bytes = (size_t)n_add * PB28; DevTmp a, b, op, oq, z;
    if ((rc = a.alloc(bytes)) || (rc = b.alloc(bytes)) || (rc = op.alloc(bytes)) || (rc = oq.alloc(bytes)) || (rc = z.alloc((size_t)n_add * 4))) return rc;
    HIPCHK(hipMemcpyAsync(a.p, a224, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.p, b224, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(op.p, 0xA5, bytes, c->stream));      // a coordinate nobody stored shows
    HIPCHK(hipMemsetAsync(oq.p, 0xA5, bytes, c->stream));
    HIPCHK(hipMemsetAsync(z.p, 0, (size_t)n_add * 4, c->stream));
    hipLaunchKernelGGL(k_te28_rows_add, dim3((n_add + 63) / 64), dim3(256), 0, c->stream, (const char*)a.p, (const char*)b.p, n_add, (char*)op.p, (char*)oq.p, (uint32_t*)z.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_pair224, op.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_quad224, oq.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(z_add_u32, z.p, (size_t)n_add * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (n_madd) {
    DevTmp acc, row, how, out, z;
    if ((rc = acc.alloc((size_t)n_madd * PB28)) || (rc = row.alloc((size_t)n_madd * 168)) || (rc = how.alloc(n_madd)) || (rc = out.alloc((size_t)n_madd * PB28)) || (rc = z.alloc(n_madd))) return rc;
    HIPCHK(hipMemcpyAsync(acc.p, acc224, (size_t)n_madd * PB28, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(row.p, row168, (size_t)n_madd * 168, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(how.p, how_u8, n_madd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(out.p, 0xA5, (size_t)n_madd * PB28, c->stream));
    HIPCHK(hipMemsetAsync(z.p, 0xA5, n_madd, c->stream));
    hipLaunchKernelGGL(k_te28_rows_madd, dim3((n_madd + 255) / 256), dim3(256), 0, c->stream, (const char*)acc.p, (const char*)row.p, (const uint8_t*)how.p, n_madd, (char*)out.p, (uint8_t*)z.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_acc224, out.p, (size_t)n_madd * PB28, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(z_madd_u8, z.p, n_madd, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
