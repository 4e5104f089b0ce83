// g2.hip — BLS12-377 G2 multi-scalar multiplication for MI355X (gfx950): y^2 = x^3 + b' over Fq2 = Fq[u] / (u^2 + 5).
//
// Replaces snarkvm-algorithms 0.14.5 `VariableBase::msm::<G2Affine>` -> `standard::msm` [UPSTREAM-RECALL: variable_base/mod.rs sends
// every curve but BLS12-377 G1 to the standard Pippenger] over snarkvm-curves bls12_377/{fq2,g2}.rs (pin: /root/reference/Cargo.lock:2637).
// The prover never runs a G2 MSM (G2 appears in the verifying key and in SRS setup), so this path is built for
// parity and reach, not for the last percent: it shares the whole scalar side with G1 — signed-digit windows, the two-level
// counting sort, slice sizing and ordering (msm_sort.hip msm_sort_phase: none of it depends on the group) — and, behind its own accumulation, the plain
// path's slice trees, reduction kernels and host back end (msm_reduce.h, msm_front_finish), instantiated for its point format — and swaps the group law:
// extended Jacobian (XYZZ) over Fq2 on the 32-bit-limb Montgomery blocks of fp.h, one lane per addition, out-of-line field
// calls (a 2 x 12-limb product inlined ten times per addition would not fit the register file).
//
// Layouts at the boundary (snarkVM in-memory): G2Affine {x: Fq2 (c0, c1), y: Fq2, infinity: bool} = 4 x 48 bytes Montgomery +
// flag byte at 192, stride 200 (or 192 without the flag); result G2Projective (Jacobian) {x, y, z: Fq2} = 288 bytes,
// returned affine-normalised (x, y, 1) or (1, 1, 0) for the identity.  HBM: bases n x 192 B (+ 224 B 28-bit rows); partial sums 448 B per slice.
#include "g2.h"
#include "msm_reduce.h"

namespace aleo_mi355x {

// ---- Fq2 on the device: components stay below 2q between operations, so the one XYZZ law of xyzz_law.h runs over it as it does over the host's fields ---
struct Fq2;
__device__ void fq2_mul_ni(Fq2* r, const Fq2* px, const Fq2* py);
__device__ void fq2_sqr_ni(Fq2* r, const Fq2* px);
__device__ __forceinline__ Fq lt2q(const Fq& x) { return Fq::cond_sub<2>(x); }                       // < 4q -> < 2q
struct Fq2 {                                   // a + b u,  u^2 = -5
  Fq a, b;
  static __device__ __forceinline__ Fq2 zero() { Fq2 r; r.a = Fq::zero(); r.b = Fq::zero(); return r; }
  static __device__ __forceinline__ Fq2 one() { Fq2 r; r.a = Fq::one(); r.b = Fq::zero(); return r; }
  static __device__ __forceinline__ Fq2 add(const Fq2& x, const Fq2& y) { Fq2 r; r.a = lt2q(Fq::add(x.a, y.a)); r.b = lt2q(Fq::add(x.b, y.b)); return r; }
  static __device__ __forceinline__ Fq2 sub(const Fq2& x, const Fq2& y) { Fq2 r; r.a = lt2q(Fq::sub<2>(x.a, y.a)); r.b = lt2q(Fq::sub<2>(x.b, y.b)); return r; }
  static __device__ __forceinline__ Fq2 dbl(const Fq2& x) { return add(x, x); }
  static __device__ __forceinline__ Fq2 mul(const Fq2& x, const Fq2& y) { Fq2 r; fq2_mul_ni(&r, &x, &y); return r; }      // out of line: a 2 x 12-limb product inlined ten times per addition would not fit the register file
  static __device__ __forceinline__ Fq2 sqr(const Fq2& x) { Fq2 r; fq2_sqr_ni(&r, &x); return r; }
  __device__ __forceinline__ bool is_zero() const { return a.is_zero_mod_lt2p() && b.is_zero_mod_lt2p(); }
  __device__ __forceinline__ bool is_zero_raw() const { return a.is_zero_raw() && b.is_zero_raw(); }
};
struct G2Affine { Fq2 x, y; };                 // 192 bytes
using XYZZ2 = XYZZOf<Fq2>;                     // 384 bytes; infinity <=> ZZ stored as raw zero

__device__ __forceinline__ Fq fq_times5_canonical(const Fq& v) {      // 5 v mod q, v < 2q
  Fq d2 = Fq::dbl(v), d4 = Fq::dbl(d2);                               // < 4q, < 8q
  return Fq::reduce(Fq::add(d4, v));                                  // < 10q -> canonical
}
// (x.a + x.b u)(y.a + y.b u) = (x.a y.a - 5 x.b y.b) + (x.a y.b + x.b y.a) u   (Karatsuba: three base-field products)
__device__ __noinline__ void fq2_mul_ni(Fq2* r, const Fq2* px, const Fq2* py) {
  const Fq2 x = *px, y = *py;
  Fq v0 = Fq::mul(x.a, y.a), v1 = Fq::mul(x.b, y.b);                  // < 2q
  Fq s = Fq::mul(Fq::add(x.a, x.b), Fq::add(y.a, y.b));               // (< 4q)(< 4q): 16/152 + 1 -> < 2q
  Fq2 o;
  o.b = lt2q(Fq::sub<2>(lt2q(Fq::sub<2>(s, v0)), v1));
  o.a = lt2q(Fq::sub<1>(v0, fq_times5_canonical(v1)));                // v0 + q - 5 v1 < 3q
  *r = o;
}
// (a + b u)^2 = (a + b)(a - 5b) + 4ab  +  2ab u   (two base-field products)
__device__ __noinline__ void fq2_sqr_ni(Fq2* r, const Fq2* px) {
  const Fq2 x = *px;
  Fq m = Fq::mul(x.a, x.b);                                           // < 2q
  Fq w = Fq::mul(Fq::add(x.a, x.b), Fq::sub<1>(x.a, fq_times5_canonical(x.b)));      // (< 4q)(< 3q) -> < 2q
  Fq2 o;
  o.b = lt2q(Fq::dbl(m));
  o.a = Fq::reduce(Fq::add(w, Fq::dbl(Fq::dbl(m))));                  // < 10q -> canonical
  *r = o;
}
__device__ __forceinline__ Fq2 load_fq2(const void* p) { Fq2 r; r.a = load_fp<Fq>(p); r.b = load_fp<Fq>((const char*)p + 48); return r; }

// 2P and acc += b: the law of xyzz_law.h, out of line (the identity, doubling and cancellation included)
__device__ __noinline__ void g2_double_ni(XYZZ2* io) { *io = law_double(*io); }
__device__ __noinline__ void g2_add_ni(XYZZ2* pa, const XYZZ2* pb) { const XYZZ2 a = *pa, b = *pb; *pa = law_add(a, b); }
// acc += (x, y) affine (EFD madd-2008-s): the repeated-base path's own formula (an addition with ZZ = ZZZ = 1 would spend four products on the ones)
__device__ __noinline__ void g2_madd_ni(XYZZ2* pa, const G2Affine* pp) {
  const XYZZ2 a = *pa; const G2Affine q = *pp;
  if (a.is_inf()) { XYZZ2 r; r.X = q.x; r.Y = q.y; r.ZZ = Fq2::one(); r.ZZZ = Fq2::one(); *pa = r; return; }
  Fq2 U2 = Fq2::mul(q.x, a.ZZ), S2 = Fq2::mul(q.y, a.ZZZ);
  Fq2 P = Fq2::sub(U2, a.X), R = Fq2::sub(S2, a.Y);
  if (P.is_zero()) {
    if (R.is_zero()) { XYZZ2 d; d.X = q.x; d.Y = q.y; d.ZZ = Fq2::one(); d.ZZZ = Fq2::one(); g2_double_ni(&d); *pa = d; } else *pa = XYZZ2::infinity();
    return;
  }
  Fq2 PP = Fq2::sqr(P), PPP = Fq2::mul(P, PP), Q = Fq2::mul(a.X, PP);
  XYZZ2 r;
  r.X = Fq2::sub(Fq2::sub(Fq2::sqr(R), PPP), Fq2::dbl(Q));
  r.Y = Fq2::sub(Fq2::mul(R, Fq2::sub(Q, r.X)), Fq2::mul(a.Y, PPP));
  r.ZZ = Fq2::mul(a.ZZ, PP);
  r.ZZZ = Fq2::mul(a.ZZZ, PPP);
  *pa = r;
}

// ---- the accumulation on 28-bit limbs, one LANE PAIR per slice (round 4) -------------------------------------------------------------------------------
// The Fq2 lane-pair formulas (fq2p_mul, g2p_madd_fast, g2p_double, g2p_add, the stored 448-byte pair form and g2p_add_any / g2p_double_any) live in
// g2p28.h, written over the names of fp28.h's guarded block alone, so that the host bounds checker and the row hook compile the same source.
// Included HERE, not at the top: its two out-of-line functions keep their place among this unit's device functions.
}  // namespace aleo_mi355x
#include "g2p28.h"
namespace aleo_mi355x {

// conversions between the pair form and the 32-bit XYZZ2 the slow path of the accumulation works in (one lane does the whole point)
__device__ __noinline__ void g2_p2_to_xyzz2(const char* p, XYZZ2* out) {
  XYZZ2 r;
  if (f28_is_zero_raw(load_f28(p + 224)) && f28_is_zero_raw(load_f28(p + 280))) { *out = XYZZ2::infinity(); return; }
  r.X.a = f28_to_fq(load_f28(p)); r.X.b = f28_to_fq(load_f28(p + 56)); r.Y.a = f28_to_fq(load_f28(p + 112)); r.Y.b = f28_to_fq(load_f28(p + 168));
  r.ZZ.a = f28_to_fq(load_f28(p + 224)); r.ZZ.b = f28_to_fq(load_f28(p + 280)); r.ZZZ.a = f28_to_fq(load_f28(p + 336)); r.ZZZ.b = f28_to_fq(load_f28(p + 392));
  *out = r;
}
__device__ __noinline__ void g2_xyzz2_to_p2(const XYZZ2* in, char* p) {
  const XYZZ2 a = *in;
  if (a.is_inf() || a.ZZ.is_zero()) { for (int i = 0; i < 8; ++i) store_f28(p + 56 * i, f28_const(Limbs14{})); return; }
  store_f28(p, f28_from_fq(a.X.a)); store_f28(p + 56, f28_from_fq(a.X.b)); store_f28(p + 112, f28_from_fq(a.Y.a)); store_f28(p + 168, f28_from_fq(a.Y.b));
  store_f28(p + 224, f28_from_fq(a.ZZ.a)); store_f28(p + 280, f28_from_fq(a.ZZ.b)); store_f28(p + 336, f28_from_fq(a.ZZZ.a)); store_f28(p + 392, f28_from_fq(a.ZZZ.b));
}

// 192-byte rows (x.a | x.b | y.a | y.b, 32-bit Montgomery) -> 224-byte rows [x.a | y.a | x.b | y.b] in the 28-bit form: each lane of a pair reads 112 contiguous bytes
__global__ void __launch_bounds__(256) k_g2_rows_to28(const char* __restrict__ src192, char* __restrict__ dst224, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  const char* r = src192 + (size_t)i * 192; char* o = dst224 + (size_t)i * ROW2;
  store_affine28(o, f28_from_fq(load_fp<Fq>(r)), f28_from_fq(load_fp<Fq>(r + 96)));
  store_affine28(o + 112, f28_from_fq(load_fp<Fq>(r + 48)), f28_from_fq(load_fp<Fq>(r + 144)));
}
// snarkVM G2Affine rows (200 bytes: x.c0 | x.c1 | y.c0 | y.c1 | infinity byte + padding) -> 192-byte rows + one flag byte per point; *n_inf counts the
// flagged points (the host drops the flag array when it is zero).  200 = 8 * 25: rows are 8-byte aligned, so a lane moves its row as 25 eight-byte words.
__global__ void __launch_bounds__(256) k_g2_unpack200(const char* __restrict__ rows200, char* __restrict__ xy192, uint8_t* __restrict__ flags, uint32_t* __restrict__ n_inf, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  const uint2* s = (const uint2*)(rows200 + (size_t)i * 200); uint2* d = (uint2*)(xy192 + (size_t)i * 192);
#pragma unroll
  for (int k = 0; k < 24; ++k) d[k] = s[k];
  const uint8_t f = (uint8_t)(s[24].x & 0xffu) ? 1 : 0;
  flags[i] = f;
  if (f) atomicAdd(n_inf, 1u);
}
int32_t g2_unpack200(const void* d_rows200, void* d_xy192, void* d_flags, uint32_t* d_count, size_t n, hipStream_t s) {
  HIPCHK(hipMemsetAsync(d_count, 0, 4, s));
  if (n) hipLaunchKernelGGL(k_g2_unpack200, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (const char*)d_rows200, (char*)d_xy192, (uint8_t*)d_flags, d_count, (uint32_t)n);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

// the rest of a slice whose fast loop met P == +-acc: the general 32-bit code, continuing from the sum the pair stored in the slice's slot
__device__ __noinline__ void g2_slice_slow_path(const char* bases192, const uint32_t* run, uint32_t j, uint32_t j1, char* slot) {
  XYZZ2 acc; g2_p2_to_xyzz2(slot, &acc);
  for (; j < j1; ++j) {
    const uint32_t e = run[j];
    G2Affine p; const char* row = bases192 + (size_t)(e & 0x7fffffffu) * 192;
    p.x = load_fq2(row); p.y = load_fq2(row + 96);
    if (e >> 31) { p.y.a = Fq::sub<1>(Fq::zero(), p.y.a); p.y.b = Fq::sub<1>(Fq::zero(), p.y.b); }
    g2_madd_ni(&acc, &p);
  }
  g2_xyzz2_to_p2(&acc, slot);
}
// One lane pair per slice on the 28-bit form (rows28: k_g2_rows_to28); the slice sum leaves as a 448-byte pair-form point: the slice trees and the bucket
// reduction below (k_g2p_*) continue in that form.
__global__ void __launch_bounds__(256, 2) k_g2_accum28(const char* __restrict__ rows28, const char* __restrict__ bases192, const uint32_t* __restrict__ sorted,
                                                    const uint32_t* __restrict__ hist, const uint2* __restrict__ scan_local, const uint2* __restrict__ scan_blk,
                                                    const uint32_t* __restrict__ total_pairs, uint32_t M, const uint32_t* __restrict__ meta, const uint32_t* __restrict__ order,
                                                    const uint32_t* __restrict__ task_g, char* __restrict__ partial) {
  const uint32_t t = (blockIdx.x * 256 + threadIdx.x) >> 1; const bool odd = threadIdx.x & 1;
  if (t >= meta[0]) return;
  const uint32_t sid = order[t], g = task_g[sid];
  const uint2 st = scan_at(scan_local, scan_blk, g);
  const uint32_t cnt = hist[g], m = slices_of(cnt, pick_rule(total_pairs, M)), k = sid - st.y;
  const uint32_t j0 = (uint32_t)(((uint64_t)k * cnt) / m), j1 = (uint32_t)(((uint64_t)(k + 1) * cnt) / m);
  const uint32_t* run = sorted + st.x;
  char* slot = partial + (size_t)sid * P2B;
  auto fetch = [&](uint32_t e, F28& x, F28& y) {
    load_affine28(rows28 + (size_t)(e & 0x7fffffffu) * ROW2 + (odd ? 112 : 0), x, y);
    if (e >> 31) y = g2p_negate_entry(y);                     // 2q - y (canonical rows): exact digits, <= 2q
  };
  XYZZ2P acc; uint32_t j = j0; bool ok = true;
  {
    F28 x, y; fetch(run[j], x, y);
    acc.X = x; acc.Y = y; acc.ZZ = odd ? f28_const(Limbs14{}) : f28_const(ONE28); acc.ZZZ = acc.ZZ;      // (x, +-y, 1, 1): the one of Fq2 is (1, 0)
    ++j;
  }
  // Pin the accumulator to registers here.  Without it hipcc (ROCm 7.2) drops the initial value of two limbs of acc.Y on the path that skips the loop
  // (a one-point slice): the store below then reads a register no instruction of the kernel writes — seen in the ISA and as 0x5a5a5a5a in the slice sums.
#ifndef ALEO_G2_NO_PIN      // (probe build: tools/isa_undef_check.py shows the unwritten registers without it)
#pragma unroll
  for (int i = 0; i < 14; ++i) asm volatile("" : "+v"(acc.X.v[i]), "+v"(acc.Y.v[i]), "+v"(acc.ZZ.v[i]), "+v"(acc.ZZZ.v[i]));
#endif
  for (; j < j1; ++j) {
    F28 x, y; fetch(run[j], x, y);
    if (!g2p_madd_fast(acc, x, y, odd)) { ok = false; break; }
  }
  g2p_store(slot, odd, acc);                               // the stored invariant is the loop's own
  if (!ok) {                                               // rare: repeated or opposite bases in one bucket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // both lanes' halves of the slot are in memory (one wave: its accesses to an address stay in order)
    if (!odd) g2_slice_slow_path(bases192, run, j, j1, slot);
  }
}
// ---- the reduction in the pair form: the plain path's kernels and back end (msm_reduce.h) over this point format, one lane pair per addition ------
struct PtG2 {
  static constexpr uint32_t BYTES = P2B;
  template <uint32_t LANES> static __device__ __forceinline__ void add(const char* pa, const char* pb, char* out) { static_assert(LANES == 2, "the pair form"); g2p_add_any(pa, pb, out); }
};
// one lane pair per chunk of S consecutive buckets: run / acc / the double-and-add register live in a per-pair work area between the cooperative operations
__global__ void __launch_bounds__(128) k_g2p_bucket_chunks(const char* __restrict__ partial, const uint32_t* __restrict__ hist, const uint2* __restrict__ scan_local,
                                                           const uint2* __restrict__ scan_blk, uint32_t B, uint32_t S, uint32_t nchunks_total, char* __restrict__ V,
                                                           char* __restrict__ work) {
  const uint32_t pr = threadIdx.x >> 1, t = blockIdx.x * 64 + pr; const bool odd = threadIdx.x & 1;
  if (t >= nchunks_total) return;
  char* run = work + (size_t)t * 3 * P2B; char* acc = run + P2B; char* r = acc + P2B;      // the pair's three working points (global memory: L2-resident)
  g2p_store_inf(run, odd); g2p_store_inf(acc, odd); g2p_store_inf(r, odd);
  const uint32_t cpw = B / S, w = t / cpw, j = t % cpw, g0 = w * B + j * S;
  for (uint32_t k = 0; k < S; ++k) {
    const uint32_t g = g0 + (S - 1 - k);
    if (hist[g]) g2p_add_any(run, partial + (size_t)scan_at(scan_local, scan_blk, g).y * P2B, run);
    g2p_add_any(acc, run, acc);
  }
  const uint32_t base = j * S;
  if (base) {
    for (int bit = 31 - __clz(base); bit >= 0; --bit) { g2p_double_any(r, r); if ((base >> bit) & 1) g2p_add_any(r, run, r); }
    g2p_add_any(acc, r, acc);
  }
  const XYZZ2P v = g2p_load(acc, odd); g2p_store(V + (size_t)t * P2B, odd, v);
}

// Test hook: the pair-form addition / doubling against the one-lane 32-bit code on chains of real curve points (aleo_mi355x_selftest_g2pair).
// Pair t takes the affine points i = t, t + 1, t + 2 (mod n): s = (P_i + P_j) + P_k, u = s + (P_i + P_j), d = 2u, e = u + u (the same-point case),
// z = u + (-u) (the opposite case), w = z + s (identity operand) — every result compared with the 32-bit code's by subtracting and asking for the identity.
__global__ void __launch_bounds__(128) k_g2p_selftest(const char* __restrict__ aff192, uint32_t n, uint32_t npairs, char* __restrict__ scratch, uint32_t* __restrict__ failures) {
  const uint32_t t = (blockIdx.x * 128 + threadIdx.x) >> 1; const bool odd = threadIdx.x & 1;
  if (t >= npairs) return;
  char* sl = scratch + (size_t)t * 9 * P2B;                  // nine pair-form slots per pair
  auto aff = [&](uint32_t i) { XYZZ2 r; const char* row = aff192 + (size_t)(i % n) * 192; r.X = load_fq2(row); r.Y = load_fq2(row + 96); r.ZZ = Fq2::one(); r.ZZZ = r.ZZ; return r; };
  XYZZ2 Pi = aff(t), Pj = aff(t + 1), Pk = aff(t + 2);
  if (!odd) { g2_xyzz2_to_p2(&Pi, sl); g2_xyzz2_to_p2(&Pj, sl + P2B); g2_xyzz2_to_p2(&Pk, sl + 2 * P2B); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  bool okm;
  { XYZZ2P m = g2p_load(sl, odd); const XYZZ2P pj = g2p_load(sl + P2B, odd); okm = g2p_madd_fast(m, pj.X, pj.Y, odd); g2p_store(sl + 8 * P2B, odd, m); }      // the mixed addition of the accumulation loop on the same operands
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  g2p_add_any(sl, sl + P2B, sl + 3 * P2B);                   // a = Pi + Pj
  if (!okm) { const XYZZ2P v = g2p_load(sl + 3 * P2B, odd); g2p_store(sl + 8 * P2B, odd, v); }      // P_i = +-P_j: the fast form refuses (the accumulation kernel leaves its loop there); the general sum stands in
  g2p_add_any(sl + 3 * P2B, sl + 2 * P2B, sl + 4 * P2B);     // s = a + Pk
  g2p_add_any(sl + 4 * P2B, sl + 3 * P2B, sl + 5 * P2B);     // u = s + a
  g2p_double_any(sl + 5 * P2B, sl + 6 * P2B);                // d = 2u
  g2p_add_any(sl + 5 * P2B, sl + 5 * P2B, sl + 7 * P2B);     // e = u + u
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (odd) return;
  XYZZ2 a = Pi; g2_add_ni(&a, &Pj); XYZZ2 sref = a; g2_add_ni(&sref, &Pk); XYZZ2 u = sref; g2_add_ni(&u, &a); XYZZ2 d = u; g2_double_ni(&d);
  auto differs = [&](const char* slot, const XYZZ2& want) {
    XYZZ2 got; g2_p2_to_xyzz2(slot, &got);
    XYZZ2 neg = want; neg.Y.a = lt2q(Fq::sub<2>(Fq::zero(), neg.Y.a)); neg.Y.b = lt2q(Fq::sub<2>(Fq::zero(), neg.Y.b));
    g2_add_ni(&got, &neg);
    return !(got.is_inf() || got.ZZ.is_zero());
  };
  uint32_t bad = 0;
  if (differs(sl + 8 * P2B, a)) bad |= 64;                  // g2p_madd_fast
  if (differs(sl, Pi)) bad |= 32;                           // the conversions alone
  if (differs(sl + 3 * P2B, a)) bad |= 1;
  if (differs(sl + 4 * P2B, sref)) bad |= 2;
  if (differs(sl + 5 * P2B, u)) bad |= 4;
  if (differs(sl + 6 * P2B, d)) bad |= 8;
  if (differs(sl + 7 * P2B, d)) bad |= 16;
  if (bad) { atomicAdd(failures, 1u); atomicOr(failures + 1, bad); }
}
int32_t selftest_g2pair(Ctx* c, const void* aff192_host, uint32_t n, uint32_t npairs, uint32_t* failures2) {
  DevTmp pts, scr, fl; int32_t rc;
  if ((rc = pts.alloc((size_t)n * 192)) || (rc = scr.alloc((size_t)npairs * 9 * P2B)) || (rc = fl.alloc(8))) return rc;
  HIPCHK(hipMemcpyAsync(pts.p, aff192_host, (size_t)n * 192, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(fl.p, 0, 8, c->stream));
  hipLaunchKernelGGL(k_g2p_selftest, dim3((2 * npairs + 127) / 128), dim3(128), 0, c->stream, (const char*)pts.p, n, npairs, (char*)scr.p, (uint32_t*)fl.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(failures2, fl.p, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return ALEO_MI355X_OK;
}

// the 28-bit rows of n affine points (192-byte x | y rows on the device) into dst224: what a pinned G2 set keeps beside its rows
int32_t g2_rows_to28(const void* d_xy192, void* d_dst224, size_t n, hipStream_t s) {
  if (n == 0) return ALEO_MI355X_OK;
  hipLaunchKernelGGL(k_g2_rows_to28, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (const char*)d_xy192, (char*)d_dst224, (uint32_t)n);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}
// G2 on the plain back end (msm_reduce.h): pair-form partial sums, a lane pair per chunk; no phase times (a G2 call leaves g_last_msm alone)
struct G2Plain {
  using PT = PtG2; using HF = host::HFq2; static constexpr bool TIMED = false;
  static host::HXYZZ2 read(const char* p) { return law_point28<HF>(p); }
  static void launch_chunks(Ctx* c, const Front& f, hipStream_t s, char* V, char* work) {      // work: three points per chunk
    hipLaunchKernelGGL(k_g2p_bucket_chunks, dim3((f.nchunks + 63) / 64), dim3(128), 0, s, c->partial.as<char>(), f.sp.hist, f.sp.scan_local, f.sp.scan_blk, f.P.B, f.P.S, f.nchunks, V, work);
  }
};
// One G2 MSM: bases d_xy (n x 192 B, device) with optional infinity flags, scalars on the device.  Plain schedule (no table): the scalar side of
// msm_sort.hip, this unit's accumulation, then the slice trees and the back end G1's plain path runs (msm_front_finish, msm_back_plain).
int32_t msm_g2_run(Ctx* c, uint64_t* out_jac36, const void* d_xy, const uint8_t* d_inf, const void* d_scalars, size_t n, hipStream_t s, const void* d_rows28) {
  if (n == 0) { law_store_jacobian_normalized(out_jac36, host::HXYZZ2::infinity()); return ALEO_MI355X_OK; }
  if (n >= (1ull << 31)) { g_last_error = "msm_g2: n exceeds 2^31"; return ALEO_MI355X_ERR_BAD_ARG; }
  Front f; f.lean = true; f.plain_tree = k_tree_pass<PtG2, 2>;      // lean: no phase-timing events behind the sort's
  MsmPlan& P = f.P; P = make_plan(n, 0);
  SegArgs segs{}; segs.nseg = 1; segs.ptr[0] = (const char*)d_scalars; segs.n[0] = (uint32_t)n;
  int32_t rc;
  if ((rc = ensure_host_pinned(c, 64 + (size_t)P.W * P2B))) return rc;
  SortPhase& sp = f.sp;
  if ((rc = msm_sort_phase(c, segs, n, false, d_inf, (uint32_t)n, P, false, s, &sp))) return rc;
  f.cpw = P.B / P.S; f.nchunks = f.cpw * P.W;
  if ((rc = c->partial.reserve(sp.slices_max * P2B))) return rc;
  if ((rc = c->vbuf.reserve(((size_t)f.nchunks * 4 + P.W) * P2B))) return rc;      // chunk sums | window sums | three working points per chunk (pair form)
  const bool resident = d_rows28 != nullptr;                // a pinned set (aleo_mi355x_bases_g2_pin) keeps its 28-bit rows
  if ((rc = c->out_stage.reserve((resident ? 0 : n * ROW2) + 256))) return rc;      // the bases in the 28-bit form (per call for the one-shot entry point)
  if (!resident && (rc = g2_rows_to28(d_xy, c->out_stage.p, n, s))) return rc;
  hipLaunchKernelGGL(k_g2_accum28, dim3(2 * sp.slice_blocks), dim3(256), 0, s, resident ? (const char*)d_rows28 : c->out_stage.as<const char>(), (const char*)d_xy, sp.sorted, sp.hist, sp.scan_local, sp.scan_blk,
                     sp.total_pairs, sp.M, sp.meta, sp.order, sp.task_g, c->partial.as<char>());
  HIPCHK(hipGetLastError());
  if ((rc = msm_front_finish(c, s, f, false))) return rc;
  return msm_back_plain<G2Plain>(c, out_jac36, f, s);
}
// Slot acquisition lives in device.hip; the entry points are defined in api.hip around msm_g2_run and this sum of Jacobian points on the host:
int32_t g2_sum_host(uint64_t* out36, const uint64_t* pts36, size_t count) {
  host::HXYZZ2 t = host::HXYZZ2::infinity();
  for (size_t i = 0; i < count; ++i) t = law_add(t, law_from_jacobian<host::HFq2>(pts36 + 36 * i));
  law_store_jacobian_normalized(out36, t);
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
