// fr_kernels.h — what the units of Fr kernels share (frops.hip, fr_spmv.hip, fr_divide.hip, ahp_kernels.hip): a field constant passed to a kernel by
// value, the lazy-reduction step of their sums, the out-of-line power, and how their hosts size a grid and end in one launch.  (Their hosts' declarations: frops.h.)
#pragma once
#include "ctx.h"
#include "fp.h"
#include <cstring>

namespace aleo_mi355x {

// A host-side constant (Montgomery form, 32 bytes) as a kernel argument.
struct FrK { uint32_t v[8]; };
__device__ __forceinline__ Fr fr_arg(const FrK& k) { Fr r; for (int i = 0; i < 8; ++i) r.v[i] = k.v[i]; return r; }
inline FrK load_k(const void* mont32) { FrK k; std::memcpy(k.v, mont32, 32); return k; }

// a + b with a + b < 4r, back below 2r: the step that keeps a running sum lazily reduced (fp.h)
__device__ __forceinline__ Fr add_lt2r(const Fr& a, const Fr& b) { return Fr::cond_sub<2>(Fr::add(a, b)); }

// io^e, io < 2r.  Out of line (a call, not ~64 unrolled products, in the kernels that need one power per lane); static: every unit that includes this gets its own.
static __device__ __noinline__ void fr_pow_u64_ni(Fr* io, uint64_t e) {
  Fr b = *io, acc = Fr::one();
  for (; e; e >>= 1) { if (e & 1) acc = Fr::mul(acc, b); b = Fr::sqr(b); }
  *io = acc;
}

// Blocks of 256 lanes for n grid-stride items, at most `cap` of them (every kernel keeps the cap it was tuned with).
inline dim3 grid_for(size_t n, uint32_t cap) { const size_t want = (n + 255) / 256; return dim3((uint32_t)(want < cap ? want : cap)); }

// The last statement of a host function: the kernel queued on s, the status of the launch.
template <class... P, class... A> int32_t launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, const A&... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
