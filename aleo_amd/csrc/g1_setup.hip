// g1_setup.hip — G1 set-up, off the hot path: synthetic base sets generated in HBM, the fixed-base tables of a pinned set (msm_precompute,
// msm_precompute_range) and the row formats (104-byte Affine rows, 96-byte rows, the 28-bit rows the accumulation kernel of msm.hip gathers).
#include "ec.h"
#include "fp28.h"
#include "te28.h"
#include "msm_common.h"

namespace aleo_mi355x {

// ---- synthetic base sets generated in HBM: P_i = (first + i) * G --------------------------------------
// Off the hot path (setup): every group operation is an out-of-line call, code size over speed.
static constexpr uint32_t GEN_K = 64;      // consecutive points per lane
__device__ __constant__ uint32_t FQ_P_MINUS_2[12] = {0xffffffffu, 0x8508bfffu, 0x30000000u, 0x170b5d44u, 0xba094800u, 0x1ef3622fu,
                                                     0x00f5138fu, 0x1a22d9f3u, 0x6ca1493bu, 0xc63b05c0u, 0x17c510eau, 0x01ae3a46u};
__device__ __noinline__ void fq_mul_ni(Fq* r, const Fq* a, const Fq* b) { *r = Fq::mul(*a, *b); }
__device__ __noinline__ void fq_inverse_ni(Fq* io) {   // a^(q-2), a < 2q
  Fq a = *io, acc = Fq::one();
  for (int bit = 376; bit >= 0; --bit) {
    fq_mul_ni(&acc, &acc, &acc);
    if ((FQ_P_MINUS_2[bit >> 5] >> (bit & 31)) & 1u) fq_mul_ni(&acc, &acc, &a);
  }
  *io = acc;
}

__global__ void __launch_bounds__(256) k_gen_xyzz(const char* __restrict__ g_affine, uint64_t first, uint32_t n, char* __restrict__ tmp) {
  uint32_t t = blockIdx.x * 256 + threadIdx.x;
  uint64_t i0 = (uint64_t)t * GEN_K; if (i0 >= n) return;
  AffinePt g = load_affine(g_affine);
  XYZZ G; G.X = g.x; G.Y = g.y; G.ZZ = Fq::one(); G.ZZZ = Fq::one();
  uint64_t k = first + i0;
  XYZZ acc = xyzz_infinity();
  for (int bit = 63 - __clzll(k); bit >= 0; --bit) {
    xyzz_double_ni(&acc);
    if ((k >> bit) & 1ull) xyzz_add_ni(&acc, &G);
  }
  for (uint32_t j = 0; j < GEN_K && i0 + j < n; ++j) {
    store_xyzz(tmp + (i0 + j) * 192, acc);
    xyzz_add_ni(&acc, &G);
  }
}
// XYZZ -> affine with one shared inversion per lane (Montgomery's trick over the lane's GEN_K points)
__global__ void __launch_bounds__(256) k_gen_normalize(char* __restrict__ tmp, uint32_t n, char* __restrict__ prefix, char* __restrict__ out_xy) {
  uint32_t t = blockIdx.x * 256 + threadIdx.x;
  uint64_t i0 = (uint64_t)t * GEN_K; if (i0 >= n) return;
  uint32_t cnt = (uint32_t)((n - i0) < GEN_K ? (n - i0) : GEN_K);
  Fq prod = Fq::one();
  for (uint32_t j = 0; j < cnt; ++j) {
    store_fp<Fq>(prefix + (i0 + j) * 48, prod);
    Fq zzz = load_fp<Fq>(tmp + (i0 + j) * 192 + 144);
    if (zzz.is_zero_mod_lt2p()) zzz = Fq::one();      // the identity: keep it out of the shared inversion
    fq_mul_ni(&prod, &prod, &zzz);
  }
  fq_inverse_ni(&prod);
  for (uint32_t jj = cnt; jj-- > 0;) {
    const char* src = tmp + (i0 + jj) * 192;
    Fq pre = load_fp<Fq>(prefix + (i0 + jj) * 48), zzz = load_fp<Fq>(src + 144), zz = load_fp<Fq>(src + 96);
    Fq zi3, zi, zi2, x, y;
    if (zzz.is_zero_mod_lt2p()) {                       // identity -> (0, 0): never on the curve, callers skip it
      store_fp<Fq>(out_xy + (i0 + jj) * 96, Fq::zero()); store_fp<Fq>(out_xy + (i0 + jj) * 96 + 48, Fq::zero());
      continue;
    }
    fq_mul_ni(&zi3, &prod, &pre);            // 1/ZZZ_j
    fq_mul_ni(&prod, &prod, &zzz);
    fq_mul_ni(&zi, &zz, &zi3);               // 1/Z
    fq_mul_ni(&zi2, &zi, &zi);               // 1/ZZ
    Fq X = load_fp<Fq>(src), Y = load_fp<Fq>(src + 48);
    fq_mul_ni(&x, &X, &zi2); fq_mul_ni(&y, &Y, &zi3);
    store_fp<Fq>(out_xy + (i0 + jj) * 96, Fq::reduce(x));
    store_fp<Fq>(out_xy + (i0 + jj) * 96 + 48, Fq::reduce(y));
  }
}

int32_t generate_multiples(Ctx* c, const void* base104, uint64_t first, size_t n, PinnedBases* out) {
  if (n == 0 || n >= (1ull << 31) || first == 0) { g_last_error = "bases_generate: bad range"; return ALEO_MI355X_ERR_BAD_ARG; }
  DevTmp xy, g, tmp, pre; int32_t rc;           // freed on every return path; xy is handed to the caller at the end
  if ((rc = xy.alloc(n * 96)) || (rc = g.alloc(96)) || (rc = tmp.alloc(n * 192)) || (rc = pre.alloc(n * 48))) return rc;
  HIPCHK(hipMemcpyAsync(g.p, base104, 96, hipMemcpyHostToDevice, c->stream));
  uint32_t lanes = (uint32_t)((n + GEN_K - 1) / GEN_K), grid = (lanes + 255) / 256;
  hipLaunchKernelGGL(k_gen_xyzz, dim3(grid), dim3(256), 0, c->stream, (const char*)g.p, first, (uint32_t)n, (char*)tmp.p);
  hipLaunchKernelGGL(k_gen_normalize, dim3(grid), dim3(256), 0, c->stream, (char*)tmp.p, (uint32_t)n, (char*)pre.p, (char*)xy.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  PinnedBases pb; pb.n = n; pb.d_xy = xy.p;
  if ((rc = make_rows28(c, &pb))) return rc;    // xy still owned here: freed on failure
  xy.release();
  *out = pb; return ALEO_MI355X_OK;
}

// P_i = s_i * G for caller-supplied canonical scalars (SRS-shaped bases P_i = beta^i * G, whose commitment to p
// is p(beta) * G — what the opening equation of KZG10 needs).  One lane per point, plain double-and-add (setup, not timed).
__global__ void __launch_bounds__(256) k_gen_scalar_mul(const char* __restrict__ g_affine, const uint32_t* __restrict__ scalars, uint32_t n, char* __restrict__ tmp,
                                                        uint8_t* __restrict__ inf, uint32_t* __restrict__ n_inf) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  AffinePt g = load_affine(g_affine);
  XYZZ G; G.X = g.x; G.Y = g.y; G.ZZ = Fq::one(); G.ZZZ = Fq::one();
  uint32_t k[8];
  for (int l = 0; l < 8; ++l) k[l] = scalars[(size_t)i * 8 + l];
  XYZZ acc = xyzz_infinity();
  for (int bit = 255; bit >= 0; --bit) {
    xyzz_double_ni(&acc);
    if ((k[bit >> 5] >> (bit & 31)) & 1u) xyzz_add_ni(&acc, &G);
  }
  store_xyzz(tmp + (size_t)i * 192, acc);
  const bool is_inf = acc.ZZZ.is_zero_mod();                 // s_i = 0 mod r: flagged like an uploaded Affine with infinity = true
  inf[i] = is_inf ? 1 : 0;
  if (is_inf) atomicAdd(n_inf, 1u);
}

int32_t generate_from_scalars(Ctx* c, const void* base104, const void* scalars32, size_t n, PinnedBases* out) {
  if (n == 0 || n >= (1ull << 31) || !scalars32) { g_last_error = "bases_from_scalars: bad range"; return ALEO_MI355X_ERR_BAD_ARG; }
  DevTmp xy, g, tmp, pre, sc, inf, cnt; int32_t rc;
  if ((rc = xy.alloc(n * 96)) || (rc = g.alloc(96)) || (rc = tmp.alloc(n * 192)) || (rc = pre.alloc(n * 48)) || (rc = sc.alloc(n * 32)) ||
      (rc = inf.alloc(n)) || (rc = cnt.alloc(4))) return rc;
  HIPCHK(hipMemcpyAsync(g.p, base104, 96, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(sc.p, scalars32, n * 32, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(cnt.p, 0, 4, c->stream));
  hipLaunchKernelGGL(k_gen_scalar_mul, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, (const char*)g.p, (const uint32_t*)sc.p, (uint32_t)n, (char*)tmp.p,
                     (uint8_t*)inf.p, (uint32_t*)cnt.p);
  uint32_t lanes = (uint32_t)((n + GEN_K - 1) / GEN_K), grid = (lanes + 255) / 256;
  hipLaunchKernelGGL(k_gen_normalize, dim3(grid), dim3(256), 0, c->stream, (char*)tmp.p, (uint32_t)n, (char*)pre.p, (char*)xy.p);
  HIPCHK(hipGetLastError());
  uint32_t n_inf = 0;
  HIPCHK(hipMemcpyAsync(&n_inf, cnt.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  PinnedBases pb; pb.n = n; pb.d_xy = xy.p;
  if ((rc = make_rows28(c, &pb))) return rc;
  xy.release();
  if (n_inf) pb.d_inf = (uint8_t*)inf.release();             // only sets that hold the identity carry flags (as uploaded sets do)
  *out = pb; return ALEO_MI355X_OK;
}

// ---- fixed-base table: row w = 2^(c * w) * P_i  (setup, once per pinned base set) -------------------
// With the table every window of a scalar feeds the same 2^(c-1) buckets (c = 20 at 2^20: 13 instead of 16 additions
// per point), one bucket reduction instead of W, and no Horner tail.  Costs W x 96 bytes of HBM per point (there are
// 288 GB) and ~250 doublings per point once, at pin time — the SRS of a proving key never changes.
__global__ void __launch_bounds__(256) k_pre_init(const char* __restrict__ xy, uint32_t n, char* __restrict__ cur) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  AffinePt p = load_affine(xy + (size_t)i * 96);
  XYZZ a; a.X = p.x; a.Y = p.y; a.ZZ = Fq::one(); a.ZZZ = Fq::one();
  if (p.x.is_zero_raw() && p.y.is_zero_raw()) a = xyzz_infinity();
  store_xyzz(cur + (size_t)i * 192, a);
}
__global__ void __launch_bounds__(256) k_pre_double(char* __restrict__ cur, uint32_t n, int doublings) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  XYZZ a = load_xyzz(cur + (size_t)i * 192);
  for (int d = 0; d < doublings; ++d) xyzz_double_ni(&a);
  store_xyzz(cur + (size_t)i * 192, a);
}

// 104-byte Affine rows (x | y | infinity byte | padding) -> 96-byte rows, the flag bytes, and the number of flagged rows
__global__ void __launch_bounds__(256) k_unpack104(const char* __restrict__ src, char* __restrict__ dst, uint8_t* __restrict__ flags, uint32_t* __restrict__ count, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const uint2* s2 = (const uint2*)(src + i * 104); uint2* d2 = (uint2*)(dst + i * 96);
#pragma unroll
    for (int k = 0; k < 12; ++k) d2[k] = s2[k];
    const uint8_t f = (uint8_t)(s2[12].x & 0xffu) ? 1 : 0;
    flags[i] = f;
    if (f) atomicAdd(count, 1u);
  }
}
int32_t unpack_affine104(Ctx* c, const void* d_rows104, void* d_xy96, void* d_flags, size_t n, hipStream_t s) {
  (void)c;
  uint32_t* count = (uint32_t*)((char*)d_flags + ((n + 3) & ~(size_t)3));
  HIPCHK(hipMemsetAsync(count, 0, 4, s));
  const size_t want = (n + 255) / 256;
  hipLaunchKernelGGL(k_unpack104, dim3((uint32_t)(want < 16384 ? want : 16384)), dim3(256), 0, s, (const char*)d_rows104, (char*)d_xy96, (uint8_t*)d_flags, count, n);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

// 96-byte rows (x | y, 12 x 32-bit Montgomery) -> 112-byte rows of the 28-bit table; (0, 0) marks the identity and stays 0
__global__ void __launch_bounds__(256) k_rows_to28(const char* __restrict__ src96, char* __restrict__ dst112, uint32_t n) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  AffinePt p = load_affine(src96 + (size_t)i * 96);
  F28 x, y;
  if (p.x.is_zero_raw() && p.y.is_zero_raw()) { x = f28_const(Limbs14{}); y = x; }
  else { x = f28_from_fq(p.x); y = f28_from_fq(p.y); }
  store_affine28(dst112 + (size_t)i * ROW28, x, y);
}
// the same conversion into a buffer the caller provides (the cold one-shot call's slot buffers), queued on s
int32_t rows_to28_into(const void* d_xy96, void* d_dst, size_t n, hipStream_t s) {
  if (n == 0) return ALEO_MI355X_OK;
  hipLaunchKernelGGL(k_rows_to28, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (const char*)d_xy96, (char*)d_dst, (uint32_t)n);
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}
int32_t make_rows28(Ctx* c, PinnedBases* pb) {
  if (pb->d_xy28 || pb->n == 0) return ALEO_MI355X_OK;
  DevTmp rows; int32_t rc;
  if ((rc = rows.alloc(pb->n * ROW28))) return rc;
  if ((rc = rows_to28_into(pb->d_xy, rows.p, pb->n, c->stream))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  pb->d_xy28 = rows.release();
  return ALEO_MI355X_OK;
}

// Affine rows (x | y, 32-bit Montgomery; (0, 0) marks the identity) -> the Edwards rows of te28.h: (y' - x' | y' + x' | 2d x' y') of the image
// x' = f (x + 1) / y, y' = (u - 1) / (u + 1), u = s (x + 1)  (tools/te28_model.py).  The two divisions of a row share ONE inverse, of y (u + 1), and the rows
// of a lane share one inversion by the prefix-product scheme of k_gen_normalize.  The identity becomes the row (1, 1, 0).  A point without a finite image
// (y = 0 or u = -1: neither is in G1) raises *no_image and gets the identity's row; the caller then drops the table.
__device__ __forceinline__ Fq fq_of(const uint32_t (&k)[12]) { Fq r; for (int i = 0; i < 12; ++i) r.v[i] = k[i]; return r; }
__device__ __noinline__ void te_denominator(const AffinePt* p, Fq* up1, Fq* den, bool* plain) {      // plain: an ordinary point (not the identity's marker, with an image)
  const Fq one = Fq::one(), s = fq_of(TE_S_32);
  Fq x1 = Fq::add(p->x, one), u;
  fq_mul_ni(&u, &s, &x1);
  *up1 = Fq::add(u, one);
  fq_mul_ni(den, &p->y, up1);
  *plain = !(p->x.is_zero_raw() && p->y.is_zero_raw()) && !den->is_zero_mod();
}
__global__ void __launch_bounds__(256) k_rows_te(const char* __restrict__ src96, uint32_t n, char* __restrict__ prefix, char* __restrict__ dst, uint32_t* __restrict__ no_image) {
  uint32_t t = blockIdx.x * 256 + threadIdx.x;
  uint64_t i0 = (uint64_t)t * GEN_K; if (i0 >= n) return;
  uint32_t cnt = (uint32_t)((n - i0) < GEN_K ? (n - i0) : GEN_K);
  const Fq one = Fq::one();
  Fq prod = one;
  for (uint32_t j = 0; j < cnt; ++j) {
    store_fp<Fq>(prefix + (i0 + j) * 48, prod);
    const AffinePt p = load_affine(src96 + (i0 + j) * 96);
    Fq up1, den; bool plain;
    te_denominator(&p, &up1, &den, &plain);
    if (plain) fq_mul_ni(&prod, &prod, &den);
  }
  fq_inverse_ni(&prod);
  const F28 one28 = te28_const(TE_ONE_28), zero28 = f28_const(Limbs14{});
  for (uint32_t jj = cnt; jj-- > 0;) {
    const AffinePt p = load_affine(src96 + (i0 + jj) * 96);
    Fq up1, den; bool plain;
    te_denominator(&p, &up1, &den, &plain);
    char* out = dst + (i0 + jj) * TE_ROW;
    if (!plain) {
      if (!(p.x.is_zero_raw() && p.y.is_zero_raw())) atomicOr(no_image, 1u);
      store_te28_row(out, one28, one28, zero28);
      continue;
    }
    const Fq pre = load_fp<Fq>(prefix + (i0 + jj) * 48), f = fq_of(TE_F_32), k = fq_of(TE_K_32);
    Fq inv, iy, iu, xe, ye, r2;
    fq_mul_ni(&inv, &prod, &pre);            // 1 / (y (u + 1))
    fq_mul_ni(&prod, &prod, &den);
    fq_mul_ni(&iy, &inv, &up1);              // 1 / y
    fq_mul_ni(&iu, &inv, &p.y);              // 1 / (u + 1)
    const Fq x1 = Fq::add(p.x, one), um1 = Fq::sub<2>(up1, Fq::dbl(one));      // x + 1; u - 1 = (u + 1) + 2q - 2
    fq_mul_ni(&xe, &f, &x1); fq_mul_ni(&xe, &xe, &iy);
    fq_mul_ni(&ye, &um1, &iu);
    fq_mul_ni(&r2, &xe, &ye); fq_mul_ni(&r2, &r2, &k);
    store_te28_row(out, f28_from_fq(Fq::sub<2>(ye, xe)), f28_from_fq(Fq::add(ye, xe)), f28_from_fq(r2));      // products are < 2q: sums and differences < 4q
  }
}

// A table row 2^k * P that is the identity although P is not: P has even order, so it is no point of G1.  The rows are affine and cannot hold the identity (the
// sort drops identity BASES by their flags, not rows), so a table over such a set would add the marker (0, 0) as if it were a point: the set gets no tables.
__global__ void __launch_bounds__(256) k_rows_vanished(const char* __restrict__ row96, const uint8_t* __restrict__ inf, uint32_t n, uint32_t* __restrict__ vanished) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  const AffinePt p = load_affine(row96 + (size_t)i * 96);
  if (p.x.is_zero_raw() && p.y.is_zero_raw() && !(inf && inf[i])) atomicOr(vanished, 1u);
}

// te: the rows in twisted Edwards form (k_rows_te).  A set with a base that has no Edwards image gets the XYZZ rows after all — and, like any set with a base of
// even order whose multiples reach the identity inside the table, no table (out->d stays null, the status is OK: the set multiplies on the plain path).
static int32_t build_table(Ctx* c, const PinnedBases* pb, int pre_c, size_t n, PinnedBases::PreTable* out, size_t off = 0, bool te = false) {
  const uint32_t W = (SCALAR_BITS + pre_c - 1) / pre_c;
  if (n * (size_t)W >= (1ull << 31)) { g_last_error = "bases_precompute: table index would exceed 31 bits"; return ALEO_MI355X_ERR_BAD_ARG; }
  const size_t stride = te ? TE_ROW : ROW28;
  DevTmp tab, cur, prefix, row, flag; int32_t rc;     // freed on every return path; tab is handed over at the end
  if ((rc = tab.alloc(n * stride * W))) return rc;                             // rows in the accumulation kernel's 28-bit formats (fp28.h, te28.h)
  if ((rc = cur.alloc(n * 192)) || (rc = prefix.alloc(n * 48)) || (rc = row.alloc(n * 96)) || (rc = flag.alloc(8))) return rc;
  hipStream_t s = c->stream;
  const uint32_t g = (uint32_t)((n + 255) / 256), lanes = (uint32_t)((n + GEN_K - 1) / GEN_K), gl = (lanes + 255) / 256;
  const char* xy = (const char*)pb->d_xy + off * 96;      // the table covers points [off, off + n) of the set
  HIPCHK(hipMemsetAsync(flag.p, 0, 8, s));
  const uint8_t* inf = pb->d_inf ? pb->d_inf + off : nullptr;
  if (te) hipLaunchKernelGGL(k_rows_te, dim3(gl), dim3(256), 0, s, xy, (uint32_t)n, (char*)prefix.p, (char*)tab.p, (uint32_t*)flag.p);
  else if (pb->d_xy28) HIPCHK(hipMemcpyAsync(tab.p, (const char*)pb->d_xy28 + off * ROW28, n * ROW28, hipMemcpyDeviceToDevice, s));
  else hipLaunchKernelGGL(k_rows_to28, dim3(g), dim3(256), 0, s, xy, (char*)tab.p, (uint32_t)n);
  hipLaunchKernelGGL(k_pre_init, dim3(g), dim3(256), 0, s, xy, (uint32_t)n, (char*)cur.p);
  for (uint32_t w = 1; w < W; ++w) {
    hipLaunchKernelGGL(k_pre_double, dim3(g), dim3(256), 0, s, (char*)cur.p, (uint32_t)n, win_width(pre_c, (int)w - 1));      // row w = 2^win_offset(w) * P
    hipLaunchKernelGGL(k_gen_normalize, dim3(gl), dim3(256), 0, s, (char*)cur.p, (uint32_t)n, (char*)prefix.p, (char*)row.p);
    hipLaunchKernelGGL(k_rows_vanished, dim3(g), dim3(256), 0, s, (const char*)row.p, inf, (uint32_t)n, (uint32_t*)flag.p + 1);
    if (te) hipLaunchKernelGGL(k_rows_te, dim3(gl), dim3(256), 0, s, (const char*)row.p, (uint32_t)n, (char*)prefix.p, (char*)tab.p + (size_t)w * n * stride, (uint32_t*)flag.p);
    else hipLaunchKernelGGL(k_rows_to28, dim3(g), dim3(256), 0, s, (const char*)row.p, (char*)tab.p + (size_t)w * n * stride, (uint32_t)n);
  }
  HIPCHK(hipGetLastError());
  uint32_t flags[2] = {0, 0};      // [0] a base without an Edwards image, [1] a row that vanished
  HIPCHK(hipMemcpyAsync(flags, flag.p, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (flags[1]) { *out = PinnedBases::PreTable(); return ALEO_MI355X_OK; }
  if (te && flags[0]) { (void)hipFree(tab.release()); return build_table(c, pb, pre_c, n, out, off, false); }
  out->d = tab.release(); out->c = pre_c; out->cover = n; out->te = te; out->row = stride;
  return ALEO_MI355X_OK;
}

// Tiers (measured, tools/small_probe.py): c = 20 needs >= 2^17 points per call to fill its 2^19 buckets, c = 16 wins from 2^15,
// c = 13 from 2^10 (0.5 ms against 1.1-1.4 ms on the plain path); KZG10::commit multiplies polynomials of every degree against
// prefixes of ONE SRS, so a pinned set carries a table for each range it can serve.  The two small tiers cost < 20 % extra HBM
// and build time of a 2^20-point set.
int32_t msm_precompute(Ctx* c, PinnedBases* pb) {
  if (pb->tabled || pb->n == 0) return ALEO_MI355X_OK;
  const size_t N = pb->n; int32_t rc = ALEO_MI355X_OK; int k = 0;
  auto lim = [&](size_t cap) { return N < cap ? N : cap; };
  auto tier = [&](int cbits, size_t cover, size_t min_n, bool te = false) {
    if (rc) return;
    if ((rc = build_table(c, pb, cbits, cover, &pb->tab[k], 0, te)) == ALEO_MI355X_OK && pb->tab[k].d) pb->tab[k++].min_n = min_n;      // (no table: a base of even order — see k_rows_vanished)
  };
  // Prefix tiers reach TIER_SLACK points past their power of two: a committer key is a power of two of powers FOLLOWED by a few hiding
  // powers, and commitments that touch those (every hiding one) would otherwise fall through to the next wider window (2x the buckets per
  // result: with 25 results in a chain, as many as a batch of 8 instances commits in its first round, most of the reduction time).
  constexpr size_t TIER_SLACK = 64;
  const size_t cover16 = lim(((size_t)1 << 17) + TIER_SLACK), cover13 = lim(((size_t)1 << 15) + TIER_SLACK);
  if (N > cover16) tier(N >= (1u << 19) ? 20 : 17, N, cover16 + 1, true);      // up to cover16 points the c = 16 tier is faster (2^17: 0.90 vs 1.18 ms); the whole-set tier alone is in Edwards form
  if (N >= (1u << 15)) tier(16, cover16, (size_t)1 << 15);
  if (N >= (1u << 10)) tier(13, cover13, (size_t)1 << 10);
  if (rc) {                                     // a later tier failed (out of memory): give back the ones already built
    for (auto& t : pb->tab) { if (t.d) (void)hipFree(t.d); t = PinnedBases::PreTable(); }
    return rc;
  }
  pb->tabled = true;
  return ALEO_MI355X_OK;
}

int32_t msm_precompute_range(Ctx* c, PinnedBases* pb, size_t off, size_t n, int window_bits) {
  if (pb->range.d) { g_last_error = "bases_precompute_range: this set already has a range table"; return ALEO_MI355X_ERR_BAD_ARG; }
  if (!n || off + n > pb->n || (window_bits != 13 && window_bits != 16)) { g_last_error = "bases_precompute_range: bad range or window (13 or 16 bits)"; return ALEO_MI355X_ERR_BAD_ARG; }
  int32_t rc = build_table(c, pb, window_bits, n, &pb->range, off);
  if (rc || !pb->range.d) return rc;      // (no table: a base of even order in the range — the calls take the other paths)
  pb->range.min_n = 0; pb->range_off = off;
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
