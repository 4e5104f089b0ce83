// The four point formulas of aleo_amd/csrc/fp28.h (xyzz28_madd_fast, xyzz28_double_both, xyzz28_add_pair, xyzz28_add_quad) run on the HOST, over
// values and bounds together, against the affine group law in host_field.hpp's HFq.
//
// fp28.h keeps everything that touches F28::v or a device builtin behind ALEO_F28_PROVIDED.  This file defines the macro and supplies that part
// itself: an F28 that carries, next to its 14 concrete limbs, an upper bound per limb, an upper bound of the value as a multiple of q (32.32 fixed
// point, strict: value < vb q) and whether the digits are exact.  Every primitive computes the concrete result the way the device does (products
// column by column with R' = 2^392, differences with the spread constant of spread_kq), propagates the bounds from the operation alone — never
// from a comment — and checks its preconditions against the BOUNDS, so one run speaks for every input inside the stated invariants:
//   limb     no 32-bit limb wraps in add / sub / normalise / the doubled operand of a squaring; no limb 0..12 of a difference can go negative
//   column   every product column, carry-in included, stays below 2^64 (and what is left for the top limb below 2^32)
//   value    the subtrahend's top limb fits the constant's (b < K q as a value); normalise sees < 2^392; the == 0 (mod q) tests see exact digits
//            below 2q / 4q
//   closure  what a formula stores satisfies the stored invariant of that field (X exact < 12q; Y class L3 < 6q; ZZ, ZZZ exact < 2q), and what
//            xyzz28_madd_fast leaves in acc the accumulator's (Y exact < 2q): outputs are legal inputs again
//   sound    every concrete limb and value is within its tracked bound (the bookkeeping of this file itself)
// A broken rule prints itself with the fp28.h line (the primitives take __builtin_LINE() as a default argument) and is counted.  The lane pair /
// quad are 2 / 4 host threads with a barrier inside each exchange helper; stores are held back until all lanes have returned, which is what
// lockstep execution gives the device where `out` aliases `pa`.
//   hipcc -x c++ -std=c++17 -O2 -mbmi2 -madx -pthread -I aleo_amd/csrc tests/cpp/fp28_bounds_emul.cpp   (tests/test_fp28_bounds.py builds and runs it;
//   -DFP28_HEADER='"path"' points it at a patched copy of the header: the negative controls).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host_field.hpp"      // the reference: independent of fp28.h and ec.h

#define __device__
#define __forceinline__ inline
#ifndef FP28_HEADER
#define FP28_HEADER "fp28.h"
#endif

typedef unsigned __int128 u128;
using aleo_mi355x::host::HFq;

// ---- plain multi-precision helpers (512 bits) ------------------------------------------------------------------------------------------------
struct Big { uint64_t w[8]; Big() { std::memset(w, 0, sizeof w); } };
static void big_add_shifted(Big& r, uint64_t x, int bit) {      // r += x << bit
  const int j = bit >> 6, sh = bit & 63; const u128 t = (u128)x << sh;
  uint64_t add[2] = {(uint64_t)t, (uint64_t)(t >> 64)}, c = 0;
  for (int q = j; q < 8; ++q) { const u128 s = (u128)r.w[q] + (q - j < 2 ? add[q - j] : 0) + c; r.w[q] = (uint64_t)s; c = (uint64_t)(s >> 64); }
}
static Big big_of_limbs(const uint64_t* l14) { Big r; for (int i = 0; i < 14; ++i) big_add_shifted(r, l14[i], 28 * i); return r; }
static Big big_of_limbs(const uint32_t* l14) { uint64_t t[14]; for (int i = 0; i < 14; ++i) t[i] = l14[i]; return big_of_limbs(t); }
static int big_cmp(const Big& a, const Big& b) { for (int i = 7; i >= 0; --i) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1; return 0; }
static Big big_mul64(const Big& a, uint64_t m) { Big r; uint64_t c = 0; for (int i = 0; i < 8; ++i) { const u128 t = (u128)a.w[i] * m + c; r.w[i] = (uint64_t)t; c = (uint64_t)(t >> 64); } return r; }
static Big big_add(const Big& a, const Big& b) { Big r; uint64_t c = 0; for (int i = 0; i < 8; ++i) { const u128 t = (u128)a.w[i] + b.w[i] + c; r.w[i] = (uint64_t)t; c = (uint64_t)(t >> 64); } return r; }
static Big big_shr(const Big& a, int n) {
  Big r; const int j = n >> 6, sh = n & 63;
  for (int i = 0; i + j < 8; ++i) { r.w[i] = a.w[i + j] >> sh; if (sh && i + j + 1 < 8) r.w[i] |= a.w[i + j + 1] << (64 - sh); }
  return r;
}
static void big_digits(const Big& a, uint32_t* v14) {            // base-2^28 digits, the top limb takes what is left (must fit 32 bits)
  for (int i = 0; i < 13; ++i) v14[i] = (uint32_t)(big_shr(a, 28 * i).w[0]) & 0x0fffffffu;
  const Big top = big_shr(a, 364); if (top.w[0] >> 32 || top.w[1]) { std::fprintf(stderr, "big_digits: value does not fit 14 limbs\n"); std::exit(2); }
  v14[13] = (uint32_t)top.w[0];
}
static Big big_q() { Big r; for (int i = 0; i < 6; ++i) r.w[i] = aleo_mi355x::host::HParams<6>::P[i]; return r; }
static const Big QB = big_q();
static constexpr uint64_t UNIT = 1ull << 32;                     // value bounds are multiples of q in units of 2^-32
static Big q_times(uint64_t vb) { return big_shr(big_mul64(QB, vb), 32); }
static uint64_t top_limb_below(uint64_t vb) { return big_shr(q_times(vb), 364).w[0]; }      // the top limb of any value < vb q
static const uint64_t QR48 = big_shr(QB, 344).w[0] + 1;          // q / 2^392, rounded up, in units of 2^-48

// ---- the books: violations by kind, slack by formula -------------------------------------------------------------------------------------------
enum Kind { LIMB, COLUMN, VALUE, CLOSURE, SOUND, NKINDS };
static const char* const KIND_NAME[NKINDS] = {"limb", "column", "value", "closure", "sound"};
static std::mutex g_mu;
static unsigned long g_viol[NKINDS], g_mismatches;
struct Slack {
  double col = 0; int col_line = 0;                              // largest product column as a fraction of 2^64
  double margin = 1e30; int margin_line = 0;                     // smallest c_i - bound(b_i) over the limbs 0..12 of a difference, in limb units
  double top_margin = 1e30; int top_margin_line = 0;             // the same for the top limb, in units of q's top limb (~ multiples of q)
  double wrap = 0; int wrap_line = 0;                            // largest limb bound of a sum / difference / carry step as a fraction of 2^32
  double norm = 0; int norm_line = 0;                            // largest value bound handed to normalise as a fraction of 2^392
  double stored[4] = {0, 0, 0, 0};                               // largest value bound stored per field, in multiples of q
  double stored_ylimb = 0;                                       // largest limb bound of a stored Y, in units of 2^28
};
static std::map<std::string, Slack> g_slack;
static void rule(bool ok, Kind k, const char* what, int line, const char* fn) {
  if (ok) return;
  std::lock_guard<std::mutex> l(g_mu);
  if (g_viol[k]++ < 4) std::fprintf(stderr, "%s rule broken: %s (fp28.h line %d, %s)\n", KIND_NAME[k], what, line, fn);
}

// ---- the guarded block of fp28.h, restated with bounds -------------------------------------------------------------------------------------------
namespace aleo_mi355x {

struct Limbs14 { uint32_t v[14]; };
struct F28 {
  static constexpr int N = 14;
  static constexpr uint32_t MASK = 0x0fffffffu;
  uint32_t v[N];
  uint64_t b[N];              // v[i] <= b[i]
  uint64_t vb;                // value < vb q / 2^32
  bool exact;                 // limbs 0..12 are base-2^28 digits
};
struct XYZZ28 { F28 X, Y, ZZ, ZZZ; };

static const Limbs14 Q28 = [] { Limbs14 r; big_digits(QB, r.v); return r; }();
static Limbs14 kq_digits(uint32_t K) { Limbs14 r; big_digits(big_mul64(QB, K), r.v); return r; }
static Limbs14 spread_kq(uint32_t K, uint32_t S) {               // as fp28.h: c_0 = d_0 + S 2^28, c_i = d_i + S 2^28 - S, c_13 = d_13 - S
  const Limbs14 d = kq_digits(K); Limbs14 c;
  for (int i = 0; i < 14; ++i) c.v[i] = d.v[i] + (i < 13 ? S << 28 : 0u) - (i > 0 ? S : 0u);
  return c;
}

static Big value_of(const F28& a) { return big_of_limbs(a.v); }
static Big value_bound(const F28& a) {                           // the smaller of what the limb bounds and the value bound allow (inclusive)
  const Big byl = big_of_limbs(a.b), byv = q_times(a.vb);
  return big_cmp(byl, byv) < 0 ? byl : byv;
}
static void sound(const F28& r, int line, const char* fn) {
  bool ok = true;
  for (int i = 0; i < 14; ++i) ok = ok && r.v[i] <= r.b[i];
  if (r.exact) for (int i = 0; i < 13; ++i) ok = ok && r.b[i] <= F28::MASK;
  ok = ok && big_cmp(value_of(r), q_times(r.vb)) <= 0;
  rule(ok, SOUND, "a concrete limb or value exceeds its tracked bound", line, fn);
}
static void note_wrap(uint64_t bound, int line, const char* fn) {
  std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[fn]; const double f = (double)bound / 4294967296.0;
  if (f > s.wrap) { s.wrap = f; s.wrap_line = line; }
}
static F28 exact_below(const uint32_t* limbs, uint64_t vb) {      // tags: exact digits, value < vb q
  F28 r; for (int i = 0; i < 14; ++i) { r.v[i] = limbs[i]; r.b[i] = F28::MASK; }
  r.b[13] = top_limb_below(vb); r.vb = vb; r.exact = true; return r;
}

inline F28 f28_const(const Limbs14& k, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  F28 r; bool zero = true;
  for (int i = 0; i < 14; ++i) { r.v[i] = k.v[i]; r.b[i] = k.v[i]; zero = zero && !k.v[i]; }
  r.exact = true; for (int i = 0; i < 13; ++i) r.exact = r.exact && k.v[i] <= F28::MASK;
  uint64_t vb = 1; if (!zero) { vb = UNIT; while (big_cmp(value_of(r), q_times(vb)) >= 0) vb += UNIT; }
  r.vb = vb; sound(r, line, fn); return r;
}

// (a b [+ c d]) 2^-392 mod q, exact digits out; sqr: a a with the doubled cross terms of the generated block
static F28 mont(const F28& a, const F28& b, const F28* c, const F28* d, bool sqr, int line, const char* fn) {
  if (sqr) for (int j = 1; j < 14; ++j) { rule(2 * a.b[j] < (1ull << 32), LIMB, "the doubled operand of a squaring wraps 32 bits", line, fn); note_wrap(2 * a.b[j], line, fn); }
  uint32_t m[14]; F28 r; u128 acc = 0, bnd = 0; double worst = 0;
  for (int col = 0; col < 27; ++col) {
    for (int i = 0; i < 14; ++i) {
      const int j = col - i; if (j < 0 || j > 13) continue;
      acc += (u128)a.v[i] * b.v[j]; bnd += (u128)a.b[i] * b.b[j];
      if (c) { acc += (u128)c->v[i] * d->v[j]; bnd += (u128)c->b[i] * d->b[j]; }
      if (j >= 1) { acc += (u128)m[i] * Q28.v[j]; bnd += (u128)F28::MASK * Q28.v[j]; }
    }
    if (col < 14) { m[col] = (uint32_t)(0 - (uint64_t)acc) & F28::MASK; acc += m[col]; bnd += F28::MASK; }
    rule(bnd < ((u128)1 << 64), COLUMN, "a product column can exceed 2^64", line, fn);
    const double f = (double)bnd / 18446744073709551616.0; if (f > worst) worst = f;
    if (col < 14) { if ((uint64_t)acc & F28::MASK) { std::fprintf(stderr, "mont: column %d does not clear\n", col); std::exit(2); } }
    else r.v[col - 14] = (uint32_t)acc & F28::MASK;
    acc >>= 28; bnd >>= 28;
  }
  rule(bnd < ((u128)1 << 32), COLUMN, "what is left for a product's top limb can exceed 2^32", line, fn);
  r.v[13] = (uint32_t)acc;
  u128 ab = (u128)a.vb * b.vb; if (c) ab += (u128)c->vb * d->vb;                 // units of 2^-64
  const u128 ab32 = (ab + (UNIT - 1)) >> 32;
  r.vb = (uint64_t)((ab32 * QR48 + (((u128)1 << 48) - 1)) >> 48) + UNIT;          // (A B q / 2^392 + 1) q
  for (int i = 0; i < 13; ++i) r.b[i] = F28::MASK;
  const uint64_t tv = top_limb_below(r.vb); r.b[13] = (uint64_t)bnd < tv ? (uint64_t)bnd : tv;
  r.exact = true;
  { std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[fn]; if (worst > s.col) { s.col = worst; s.col_line = line; } }
  sound(r, line, fn); return r;
}
inline F28 f28_mul(const F28& a, const F28& b, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) { return mont(a, b, nullptr, nullptr, false, line, fn); }
inline F28 f28_sqr(const F28& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) { return mont(a, a, nullptr, nullptr, true, line, fn); }
inline F28 f28_muladd(const F28& a, const F28& b, const F28& c, const F28& d, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) { return mont(a, b, &c, &d, false, line, fn); }

inline F28 f28_add(const F28& a, const F28& b, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  F28 r;
  for (int i = 0; i < 14; ++i) {
    r.b[i] = a.b[i] + b.b[i]; rule(r.b[i] < (1ull << 32), LIMB, "a limb of a sum wraps 32 bits", line, fn); note_wrap(r.b[i], line, fn);
    r.v[i] = a.v[i] + b.v[i];
  }
  r.vb = a.vb + b.vb; r.exact = false; sound(r, line, fn); return r;
}
template <uint32_t K, uint32_t S> inline F28 f28_sub(const F28& a, const F28& b, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  const Limbs14 c = spread_kq(K, S);
  rule(c.v[13] < 0x80000000u, VALUE, "K too small for this spread", line, fn);
  F28 r; double margin = 1e30;
  for (int i = 0; i < 14; ++i) {
    // the minuend taken as 0: b's limb must fit the constant's
    rule(b.b[i] <= c.v[i], i < 13 ? LIMB : VALUE, i < 13 ? "a limb of a difference can go negative" : "the top limb of a difference can go negative (subtrahend not below K q)", line, fn);
    if (i < 13) { const double mg = (double)c.v[i] - (double)b.b[i]; if (mg < margin) margin = mg; }
    r.b[i] = a.b[i] + c.v[i]; rule(r.b[i] < (1ull << 32), LIMB, "a limb of a difference wraps 32 bits", line, fn); note_wrap(r.b[i], line, fn);
    r.v[i] = a.v[i] + c.v[i] - b.v[i];
  }
  r.vb = a.vb + (uint64_t)K * UNIT; r.exact = false;
  {
    std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[fn];
    if (margin < s.margin) { s.margin = margin; s.margin_line = line; }
    const double tm = ((double)c.v[13] - (double)b.b[13]) / (double)Q28.v[13];
    if (tm < s.top_margin) { s.top_margin = tm; s.top_margin_line = line; }
  }
  sound(r, line, fn); return r;
}
inline F28 f28_normalise(const F28& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  Big two392; two392.w[6] = 1ull << 8;
  const Big vbnd = value_bound(a);
  rule(big_cmp(vbnd, two392) < 0, VALUE, "normalise can see a value of 2^392 or more", line, fn);
  { std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[fn]; const double f = (double)big_shr(vbnd, 340).w[0] / 4503599627370496.0; if (f > s.norm) { s.norm = f; s.norm_line = line; } }
  F28 r = a; uint64_t carry = 0;
  for (int i = 0; i < 13; ++i) {
    const uint64_t in = a.b[i] + carry; rule(in < (1ull << 32), LIMB, "a carry step of normalise wraps 32 bits", line, fn); note_wrap(in, line, fn);
    carry = in >> 28;
    r.v[i + 1] += r.v[i] >> 28; r.v[i] &= F28::MASK; r.b[i] = F28::MASK;
  }
  const uint64_t top = a.b[13] + carry; rule(top < (1ull << 32), LIMB, "the top limb of normalise wraps 32 bits", line, fn);
  const uint64_t tv = big_shr(vbnd, 364).w[0];
  r.b[13] = top < tv ? top : tv; r.exact = true; sound(r, line, fn); return r;
}
inline bool f28_is_zero_mod_lt2q(const F28& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  rule(a.exact && a.vb <= 2 * UNIT, VALUE, "the == 0 (mod q) test needs exact digits below 2q", line, fn);
  uint32_t z = 0, e = 0;
  for (int i = 0; i < 14; ++i) { z |= a.v[i]; e |= a.v[i] ^ Q28.v[i]; }
  return z == 0 || e == 0;
}
inline bool f28_is_small_multiple_of_q(const F28& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  rule(a.exact && a.vb <= 4 * UNIT, VALUE, "the q / 2q / 3q test needs exact digits below 4q", line, fn);
  const Limbs14 q1 = kq_digits(1), q2 = kq_digits(2), q3 = kq_digits(3);
  uint32_t e1 = 0, e2 = 0, e3 = 0;
  for (int i = 0; i < 14; ++i) { e1 |= a.v[i] ^ q1.v[i]; e2 |= a.v[i] ^ q2.v[i]; e3 |= a.v[i] ^ q3.v[i]; }
  return e1 == 0 || e2 == 0 || e3 == 0;
}
inline bool f28_is_zero_raw(const F28& a) { uint32_t z = 0; for (int i = 0; i < 14; ++i) z |= a.v[i]; return z == 0; }
inline F28 f28_sel(bool take_b, const F28& a, const F28& b) {
  F28 r = take_b ? b : a;
  for (int i = 0; i < 14; ++i) r.b[i] = a.b[i] > b.b[i] ? a.b[i] : b.b[i];
  r.vb = a.vb > b.vb ? a.vb : b.vb; r.exact = a.exact && b.exact; return r;
}

// ---- memory: an arena of 224-byte points; a load takes the stored invariant of its field as its bounds, a store checks it ---------------------------
static constexpr int ARENA_ROWS = 8;
alignas(16) static uint32_t g_arena[ARENA_ROWS][56];
static const uint64_t STORED_VB[4] = {12 * UNIT, 6 * UNIT, 2 * UNIT, 2 * UNIT};
static constexpr uint64_t L3_MAX = 3ull * (1u << 28) - 1;
static int field_of(const void* p, int line, const char* fn) {
  const ptrdiff_t off = (const char*)p - (const char*)g_arena;
  if (off < 0 || off + 56 > (ptrdiff_t)sizeof g_arena || off % 56) { std::fprintf(stderr, "access outside the arena or not at a coordinate (fp28.h line %d, %s)\n", line, fn); std::exit(2); }
  return (int)(off / 56) % 4;
}
inline F28 load_f28(const void* p, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  const int f = field_of(p, line, fn); F28 r; std::memcpy(r.v, p, 56);
  r.vb = STORED_VB[f]; r.exact = f != 1;
  for (int i = 0; i < 13; ++i) r.b[i] = f == 1 ? L3_MAX : F28::MASK;
  r.b[13] = top_limb_below(r.vb);
  sound(r, line, fn); return r;
}
struct Pending { char* p; uint32_t w[28]; int bytes; };
static std::vector<Pending> g_pending;                           // committed when every lane has returned
static void hold(char* p, const uint32_t* w, int bytes) { Pending s; s.p = p; s.bytes = bytes; std::memcpy(s.w, w, bytes); std::lock_guard<std::mutex> l(g_mu); g_pending.push_back(s); }
inline void store_f28(void* p, const F28& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  const int f = field_of(p, line, fn);
  bool ok = a.vb <= STORED_VB[f];
  if (f == 1) for (int i = 0; i < 14; ++i) ok = ok && a.b[i] <= L3_MAX; else ok = ok && a.exact;
  static const char* const what[4] = {"a stored X is not exact digits below 12q", "a stored Y is not class L3 below 6q", "a stored ZZ is not exact digits below 2q", "a stored ZZZ is not exact digits below 2q"};
  rule(ok, CLOSURE, what[f], line, fn);
  {
    std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[fn]; const double v = (double)a.vb / (double)UNIT;
    if (v > s.stored[f]) s.stored[f] = v;
    if (f == 1) for (int i = 0; i < 13; ++i) { const double lb = (double)a.b[i] / 268435456.0; if (lb > s.stored_ylimb) s.stored_ylimb = lb; }
  }
  hold((char*)p, a.v, 56);
}

// ---- lanes: 2 or 4 host threads in lockstep at every exchange ---------------------------------------------------------------------------------------
struct Barrier {
  std::mutex m; std::condition_variable cv; int n, count = 0; unsigned gen = 0;
  explicit Barrier(int n_) : n(n_) {}
  void wait() { std::unique_lock<std::mutex> l(m); const unsigned g = gen; if (++count == n) { count = 0; ++gen; cv.notify_all(); } else cv.wait(l, [&] { return gen != g; }); }
};
struct Group { Barrier quad{4}, pair0{2}, pair1{2}; F28 slot[4]; int flag[4]; int lanes; };
static thread_local Group* t_grp; static thread_local uint32_t t_lane;
static unsigned long g_calls_double, g_calls_pair, g_calls_quad, g_quad_to_pair, g_two_torsion, g_identity, g_copy_half, g_copy_quarter;
inline uint32_t f28_lane(int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {      // called once at the top of each lane-group formula
  if (t_lane == 0) {
    std::lock_guard<std::mutex> l(g_mu);
    if (!std::strcmp(fn, "xyzz28_double_both")) ++g_calls_double;
    else if (!std::strcmp(fn, "xyzz28_add_quad")) ++g_calls_quad;
    else if (!std::strcmp(fn, "xyzz28_add_pair")) { ++g_calls_pair; if (t_grp->lanes == 4) ++g_quad_to_pair; }
  }
  return t_lane;
}
static Barrier& pair_barrier() { return t_lane < 2 ? t_grp->pair0 : t_grp->pair1; }
inline F28 f28_xchg(const F28& a) { Barrier& b = pair_barrier(); t_grp->slot[t_lane] = a; b.wait(); const F28 r = t_grp->slot[t_lane ^ 1]; b.wait(); return r; }
template <int S0, int S1, int S2, int S3> inline F28 f28_qperm(const F28& a) {
  const int src[4] = {S0, S1, S2, S3};
  t_grp->slot[t_lane] = a; t_grp->quad.wait(); const F28 r = t_grp->slot[src[t_lane]]; t_grp->quad.wait(); return r;
}
inline int f28_pair_flag_of_even(int z) { Barrier& b = pair_barrier(); t_grp->flag[t_lane] = z; b.wait(); const int r = t_grp->flag[t_lane & ~1u]; b.wait(); return r; }
inline int f28_quad_flag_of_lane1(int z) { t_grp->flag[t_lane] = z; t_grp->quad.wait(); const int r = t_grp->flag[1]; t_grp->quad.wait(); return r; }
inline void f28_zero_half(char* d, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  field_of(d, line, fn); const uint32_t z[28] = {}; hold(d, z, 112);
  if (t_lane == 0) { std::lock_guard<std::mutex> l(g_mu); if (!std::strcmp(fn, "xyzz28_double_both")) ++g_two_torsion; else ++g_identity; }
}
inline void f28_copy_half(char* out, const char* src, uint32_t off, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  field_of(out + off, line, fn); field_of(src + off, line, fn); hold(out + off, (const uint32_t*)(src + off), 112);
  if (t_lane == 0) { std::lock_guard<std::mutex> l(g_mu); ++g_copy_half; }
}
inline void f28_copy_quarter(char* out, const char* src, uint32_t off, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  field_of(out + off, line, fn); field_of(src + off, line, fn); hold(out + off, (const uint32_t*)(src + off), 56);
  if (t_lane == 0) { std::lock_guard<std::mutex> l(g_mu); ++g_copy_quarter; }
}

}  // namespace aleo_mi355x

#define ALEO_F28_PROVIDED
#include FP28_HEADER

using namespace aleo_mi355x;

// ---- the reference: the affine group law on y^2 = x^3 + 1 over HFq -----------------------------------------------------------------------------
struct Aff { bool inf; HFq x, y; };
static Aff aff_inf() { Aff r; r.inf = true; r.x = HFq::zero(); r.y = HFq::zero(); return r; }
static Aff aff_neg(const Aff& p) { Aff r = p; r.y = HFq::neg(p.y); return r; }
static Aff aff_add(const Aff& p, const Aff& q) {
  if (p.inf) return q;
  if (q.inf) return p;
  HFq lam;
  if (p.x == q.x) {
    if (!(p.y == q.y) || p.y.is_zero()) return aff_inf();                       // opposite points, the 2-torsion point (-1, 0) twice
    const HFq xx = HFq::sqr(p.x); lam = HFq::mul(HFq::add(HFq::dbl(xx), xx), HFq::inv(HFq::dbl(p.y)));
  } else lam = HFq::mul(HFq::sub(q.y, p.y), HFq::inv(HFq::sub(q.x, p.x)));
  Aff r; r.inf = false;
  r.x = HFq::sub(HFq::sub(HFq::sqr(lam), p.x), q.x);
  r.y = HFq::sub(HFq::mul(lam, HFq::sub(p.x, r.x)), p.y);
  return r;
}
static bool on_curve(const Aff& p) { return p.inf || HFq::sqr(p.y) == HFq::add(HFq::mul(HFq::sqr(p.x), p.x), HFq::one()); }

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static HFq rnd_fq() { HFq r = HFq::from_u64(rnd()); for (int i = 0; i < 6; ++i) r = HFq::add(HFq::mul(r, HFq::from_u64(rnd())), HFq::from_u64(rnd())); return r; }
// Tonelli-Shanks: q - 1 = 2^46 t
static bool fq_sqrt(HFq& r, const HFq& a) {
  static uint64_t t[6], th[6], half[6]; static HFq c; static bool init = false;
  if (!init) {
    Big qm1 = QB; qm1.w[0] -= 1;
    const Big tb = big_shr(qm1, 46), thb = big_shr(tb, 1), hb = big_shr(qm1, 1);
    for (int i = 0; i < 6; ++i) { t[i] = tb.w[i]; th[i] = thb.w[i]; half[i] = hb.w[i]; }
    for (uint64_t z = 2;; ++z) { const HFq zz = HFq::from_u64(z); if (!(HFq::pow(zz, half, 6) == HFq::one())) { c = HFq::pow(zz, t, 6); break; } }
    init = true;
  }
  if (a.is_zero()) { r = a; return true; }
  if (!(HFq::pow(a, half, 6) == HFq::one())) return false;
  const HFq w = HFq::pow(a, th, 6);                          // a^((t - 1) / 2)
  HFq x = HFq::mul(a, w), b = HFq::mul(x, w), z = c; int m = 46;
  while (!(b == HFq::one())) {
    int k = 0; HFq b2 = b; while (!(b2 == HFq::one())) { b2 = HFq::sqr(b2); ++k; }
    HFq g = z; for (int i = 0; i < m - k - 1; ++i) g = HFq::sqr(g);
    x = HFq::mul(x, g); z = HFq::sqr(g); b = HFq::mul(b, z); m = k;
  }
  r = x; return true;
}
static Aff rnd_point() { for (;;) { Aff p; p.inf = false; p.x = rnd_fq(); if (fq_sqrt(p.y, HFq::add(HFq::mul(HFq::sqr(p.x), p.x), HFq::one()))) return p; } }

// ---- representatives --------------------------------------------------------------------------------------------------------------------------
// canonical 28-bit Montgomery digits of a residue (HFq keeps v 2^384; times 2^8 under its own product gives v 2^392), plus k q
static Big mont28_value(const HFq& v, uint32_t k) {
  const HFq c = HFq::mul(v, HFq::from_u64(256)); Big r; for (int i = 0; i < 6; ++i) r.w[i] = c.l[i];
  return big_add(r, big_mul64(QB, k));
}
static void relimb_up(uint32_t* v) {                             // same value, limbs raised towards 3 2^28 - 1: every limb lends two units to the one below
  for (int i = 12; i >= 0; --i) { const uint32_t k = v[i + 1] < 2 ? v[i + 1] : 2; v[i + 1] -= k; v[i] += k << 28; }
}
struct Rep { uint32_t kx, ky, kzz, kzzz; bool relimb_y; };
static const Rep REPS[4] = {{0, 0, 0, 0, false}, {11, 5, 1, 1, false}, {11, 5, 1, 1, true}, {0, 0, 1, 0, true}};
static void make_row(uint32_t* row, const Aff& p, const HFq& z, const Rep& r) {
  if (p.inf) { std::memset(row, 0, 224); return; }
  const HFq zz = HFq::sqr(z), zzz = HFq::mul(zz, z);
  big_digits(mont28_value(HFq::mul(p.x, zz), r.kx), row);
  big_digits(mont28_value(HFq::mul(p.y, zzz), r.ky), row + 14); if (r.relimb_y) relimb_up(row + 14);
  big_digits(mont28_value(zz, r.kzz), row + 28);
  big_digits(mont28_value(zzz, r.kzzz), row + 42);
}
// residues of a point in the 28-bit form; compares with an affine point after dividing by ZZ and ZZZ
static bool point_is(const uint32_t* row, const Aff& want, const char** why) {
  uint32_t z = 0; for (int i = 0; i < 14; ++i) z |= row[28 + i];
  const HFq X = aleo_mi355x::host::hfq_from28(row), Y = aleo_mi355x::host::hfq_from28(row + 14), ZZ = aleo_mi355x::host::hfq_from28(row + 28), ZZZ = aleo_mi355x::host::hfq_from28(row + 42);
  if (want.inf) { *why = "expected the identity (ZZ all zero)"; return z == 0; }
  if (z == 0 || ZZ.is_zero()) { *why = "ZZ is zero for a finite point"; return false; }
  if (!(HFq::mul(HFq::sqr(ZZ), ZZ) == HFq::sqr(ZZZ))) { *why = "ZZ^3 != ZZZ^2"; return false; }
  if (!(HFq::mul(X, HFq::inv(ZZ)) == want.x)) { *why = "x differs"; return false; }
  if (!(HFq::mul(Y, HFq::inv(ZZZ)) == want.y)) { *why = "y differs"; return false; }
  return true;
}
static void mismatch(const char* what, const char* why, int id) { if (g_mismatches++ < 10) std::fprintf(stderr, "mismatch: %s, case %d: %s\n", what, id, why); }

// ---- running the lane-group formulas --------------------------------------------------------------------------------------------------------------
static unsigned long g_adds[2], g_inf_cases, g_alias_cases;
static void run_add(int lanes, const uint32_t* rowA, const uint32_t* rowB, bool alias, const Aff& A, const Aff& B, int id) {
  std::memcpy(g_arena[0], rowA, 224); std::memcpy(g_arena[1], rowB, 224); std::memset(g_arena[2], 0xff, 224);
  const char* pa = (const char*)g_arena[0]; const char* pb = (const char*)g_arena[1]; char* out = alias ? (char*)g_arena[0] : (char*)g_arena[2];
  Group g; g.lanes = lanes; g_pending.clear();
  std::thread th[4];
  for (int l = 0; l < lanes; ++l) th[l] = std::thread([&, l] { t_grp = &g; t_lane = (uint32_t)l; if (lanes == 4) xyzz28_add_quad(pa, pb, out); else xyzz28_add_pair(pa, pb, out); });
  for (int l = 0; l < lanes; ++l) th[l].join();
  // commit: no byte written twice, and a result that is not one of the operands left in place written whole
  uint8_t seen[224] = {}; bool twice = false;
  for (const Pending& s : g_pending) {
    const ptrdiff_t o = s.p - out; if (o < 0 || o + s.bytes > 224) { mismatch("a store lands outside `out`", "", id); continue; }
    for (int i = 0; i < s.bytes; ++i) { twice = twice || seen[o + i]; seen[o + i] = 1; }
    std::memcpy(s.p, s.w, s.bytes);
  }
  size_t written = 0; for (int i = 0; i < 224; ++i) written += seen[i];
  const bool kept = alias && (B.inf);                            // A + O with out == pa: nothing to write
  if (twice || (written != 224 && !(kept && written == 0))) mismatch(lanes == 4 ? "quad" : "pair", "the lanes do not write `out` exactly once", id);
  const char* why = ""; if (!point_is((const uint32_t*)out, aff_add(A, B), &why)) mismatch(lanes == 4 ? "quad" : "pair", why, id);
  ++g_adds[lanes == 4]; g_inf_cases += A.inf || B.inf; g_alias_cases += alias;
}
static int g_case = 0;
static void add_case(const Aff& A, const HFq& za, const Rep& ra, const Aff& B, const HFq& zb, const Rep& rb) {
  uint32_t rowA[56], rowB[56]; make_row(rowA, A, za, ra); make_row(rowB, B, zb, rb);
  ++g_case;
  for (int lanes = 2; lanes <= 4; lanes += 2) for (int alias = 0; alias < 2; ++alias) run_add(lanes, rowA, rowB, alias, A, B, g_case);
}

// ---- the mixed addition --------------------------------------------------------------------------------------------------------------------------
static unsigned long g_madds, g_madd_refused;
static F28 tagged(const HFq& v, uint32_t k, uint64_t vb) { uint32_t d[14]; big_digits(mont28_value(v, k), d); return exact_below(d, vb); }
static F28 l2_negation(const F28& y) { return f28_sub<2, 1>(f28_const(Limbs14{}), y); }      // as msm.hip builds it; y tagged canonical
static void acc_row(uint32_t* row, const XYZZ28& a) { std::memcpy(row, a.X.v, 56); std::memcpy(row + 14, a.Y.v, 56); std::memcpy(row + 28, a.ZZ.v, 56); std::memcpy(row + 42, a.ZZZ.v, 56); }
// acc: X exact < 12q, Y exact < 2q (or the L2 negation), ZZ / ZZZ exact < 2q — tagged with the invariant's bounds, whatever the concrete limbs are
static bool run_madd(XYZZ28& acc, const Aff& A, const Aff& P, bool neg_entry, int id) {
  F28 x2 = tagged(P.x, 0, UNIT), y2 = tagged(neg_entry ? HFq::neg(P.y) : P.y, 0, UNIT);
  if (neg_entry) y2 = l2_negation(y2);                            // the entry holds -P's y; the sign bit of the sorted index asks for 2q - y
  const XYZZ28 before = acc;
  const bool ok = xyzz28_madd_fast(acc, x2, y2);
  ++g_madds; g_madd_refused += !ok;
  const bool same_x = !A.inf && A.x == P.x;
  uint32_t r0[56], r1[56]; acc_row(r0, before); acc_row(r1, acc);
  if (ok == same_x) mismatch("madd", ok ? "accepted P == +-acc" : "refused a point that is not +-acc", id);
  if (!ok) { if (std::memcmp(r0, r1, 224)) mismatch("madd", "acc changed by a refused addition", id); return false; }
  const char* why = ""; if (!point_is(r1, aff_add(A, P), &why)) mismatch("madd", why, id);
  const char* fn = "xyzz28_madd_fast";
  rule(acc.X.exact && acc.X.vb <= 12 * UNIT, CLOSURE, "acc.X is not exact digits below 12q after the addition", 0, fn);
  rule(acc.Y.exact && acc.Y.vb <= 2 * UNIT, CLOSURE, "acc.Y is not exact digits below 2q after the addition", 0, fn);
  rule(acc.ZZ.exact && acc.ZZ.vb <= 2 * UNIT, CLOSURE, "acc.ZZ is not exact digits below 2q after the addition", 0, fn);
  rule(acc.ZZZ.exact && acc.ZZZ.vb <= 2 * UNIT, CLOSURE, "acc.ZZZ is not exact digits below 2q after the addition", 0, fn);
  {
    std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[fn]; const F28* f[4] = {&acc.X, &acc.Y, &acc.ZZ, &acc.ZZZ};
    for (int i = 0; i < 4; ++i) { const double v = (double)f[i]->vb / (double)UNIT; if (v > s.stored[i]) s.stored[i] = v; }
  }
  return true;
}
static XYZZ28 make_acc(const Aff& A, const HFq& z, uint32_t kx, uint32_t ky, uint32_t kz) {
  const HFq zz = HFq::sqr(z), zzz = HFq::mul(zz, z); XYZZ28 a;
  a.X = tagged(HFq::mul(A.x, zz), kx, 12 * UNIT); a.Y = tagged(HFq::mul(A.y, zzz), ky, 2 * UNIT);
  a.ZZ = tagged(zz, kz, 2 * UNIT); a.ZZZ = tagged(zzz, kz, 2 * UNIT); return a;
}
static XYZZ28 first_point(const Aff& A, bool neg) {               // acc = (x, +-y, 1, 1) as the accumulation kernel starts a slice: A = +-(entry)
  XYZZ28 a; const HFq ey = neg ? HFq::neg(A.y) : A.y;
  a.X = tagged(A.x, 0, UNIT); a.Y = tagged(ey, 0, UNIT); if (neg) a.Y = l2_negation(a.Y);
  Limbs14 one28; big_digits(mont28_value(HFq::one(), 0), one28.v);      // 2^392 mod q: fp28.h's ONE28
  a.ZZ = f28_const(one28); a.ZZZ = a.ZZ; return a;
}

int main() {
  t_grp = nullptr; t_lane = 0;
  const HFq one = HFq::one();
  std::vector<Aff> P; for (int i = 0; i < 4; ++i) P.push_back(rnd_point());
  const HFq z1 = rnd_fq(), z2 = rnd_fq();
  Aff T; T.inf = false; T.x = HFq::neg(one); T.y = HFq::zero();                // (-1, 0): 2-torsion
  Aff W; W.inf = false; W.x = HFq::zero(); W.y = one;                           // (0, 1): X has all limbs zero while ZZ does not
  const Aff O = aff_inf();
  for (const Aff& p : P) if (!on_curve(p)) { std::fprintf(stderr, "a test point is not on the curve\n"); return 2; }
  if (!on_curve(T) || !on_curve(W)) return 2;
  const HFq zs[3] = {one, z1, z2};

  // ---- pair and quad: every case in both forms, with `out` apart and with `out` aliasing `pa` (msm.hip's in-place folds)
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) {
    const Rep &ra = REPS[a], &rb = REPS[b]; const HFq &za = zs[(a + b) % 3], &zb = zs[(a + 2 * b + 1) % 3];
    add_case(P[a], za, ra, P[(a + 1 + b % 3) % 4], zb, rb);                   // distinct points
    add_case(P[a], za, ra, P[a], zb, rb);                                     // the same point: other representatives, other Z -> doubling
    add_case(P[b], za, ra, aff_neg(P[b]), zb, rb);                            // opposite points -> the identity
    add_case(T, za, ra, T, zb, rb);                                           // (-1, 0) + (-1, 0): the Y == 0 branch of the doubling
    add_case(T, za, ra, P[b], zb, rb); add_case(P[a], za, ra, T, zb, rb);
    add_case(W, za, ra, W, zb, rb); add_case(W, za, ra, aff_neg(W), zb, rb);  // (0, 1) doubled, (0, 1) + (0, -1)
    add_case(W, za, ra, P[b], zb, rb); add_case(P[a], za, ra, aff_neg(W), zb, rb);
    add_case(W, za, ra, T, zb, rb);                                           // (0, 1) + (-1, 0) = (2, -3)
    add_case(P[a], one, ra, P[(a + 1) % 4], one, rb);                         // Z = 1 on both sides
  }
  for (int a = 0; a < 4; ++a) {
    add_case(O, one, REPS[0], P[a], zs[a % 3], REPS[a]); add_case(P[a], zs[a % 3], REPS[a], O, one, REPS[0]);
    add_case(O, one, REPS[0], T, zs[a % 3], REPS[a]); add_case(W, zs[a % 3], REPS[a], O, one, REPS[0]);
  }
  add_case(O, one, REPS[0], O, one, REPS[0]);
  const int add_cases = g_case;

  // ---- the mixed addition of the accumulation loop
  int id = 0;
  for (int a = 0; a < 4; ++a) for (uint32_t lift = 0; lift < 2; ++lift) for (int neg = 0; neg < 2; ++neg) {
    const uint32_t kx = lift ? 11 : 0, ky = lift, kz = lift ^ (uint32_t)(a & 1); const HFq& z = zs[(a + lift) % 3];
    const Aff& A = P[a]; const Aff& B = P[(a + 1) % 4]; const Aff Bn = neg ? aff_neg(B) : B;
    { XYZZ28 acc = make_acc(A, z, kx, ky, kz); run_madd(acc, A, Bn, neg, ++id); }                       // distinct
    { XYZZ28 acc = make_acc(A, z, kx, ky, kz); run_madd(acc, A, A, neg, ++id); }                        // P == acc: refused
    { XYZZ28 acc = make_acc(A, z, kx, ky, kz); run_madd(acc, A, aff_neg(A), neg, ++id); }               // P == -acc: refused
    { XYZZ28 acc = first_point(A, neg); run_madd(acc, A, Bn, !neg, ++id); }                             // the first point (+-y, Z = 1), then another
    { XYZZ28 acc = first_point(A, neg); run_madd(acc, A, A, neg, ++id); }
    { XYZZ28 acc = first_point(A, neg); run_madd(acc, A, aff_neg(A), !neg, ++id); }
    { XYZZ28 acc = make_acc(T, z, kx, ky, kz); run_madd(acc, T, Bn, neg, ++id); }                       // acc = (-1, 0): Y is 0 or q
    { XYZZ28 acc = make_acc(T, z, kx, ky, kz); run_madd(acc, T, T, neg, ++id); }                        // (-1, 0) twice: refused
    { XYZZ28 acc = make_acc(W, z, kx, ky, kz); run_madd(acc, W, Bn, neg, ++id); }                       // acc = (0, 1): X is 0 or 11q
    { XYZZ28 acc = make_acc(W, z, kx, ky, kz); run_madd(acc, W, neg ? W : aff_neg(W), neg, ++id); }     // refused
    { XYZZ28 acc = make_acc(A, z, kx, ky, kz); run_madd(acc, A, W, neg, ++id); }                        // the entry is (0, 1): x2 all zero
    { XYZZ28 acc = first_point(W, neg); run_madd(acc, W, T, neg, ++id); }                               // y2 = 0 and its negation 2q
    // a chain: what an addition leaves is the next one's acc, re-tagged with the invariant alone
    XYZZ28 acc = first_point(A, neg); Aff sum = A;
    for (int s = 1; s <= 6; ++s) {
      const Aff& Q = P[(a + s) % 4]; const bool ng = (s + neg) & 1; const Aff Qs = ng ? aff_neg(Q) : Q;
      if (!run_madd(acc, sum, Qs, ng, ++id)) break;
      sum = aff_add(sum, Qs);
      acc.X = exact_below(acc.X.v, 12 * UNIT); acc.Y = exact_below(acc.Y.v, 2 * UNIT); acc.ZZ = exact_below(acc.ZZ.v, 2 * UNIT); acc.ZZZ = exact_below(acc.ZZZ.v, 2 * UNIT);
    }
  }

  unsigned long viol = 0; for (int k = 0; k < NKINDS; ++k) viol += g_viol[k];
  for (const char* fn : {"xyzz28_madd_fast", "xyzz28_double_both", "xyzz28_add_pair", "xyzz28_add_quad"}) {
    const Slack& s = g_slack[fn];
    std::printf("slack %s: largest column %.4f of 2^64 (line %d); smallest subtrahend-limb margin %.0f units (line %d), top limb %.2f q (line %d); largest limb %.4f of 2^32 (line %d); "
                "largest value into normalise %.6f of 2^392 (line %d); largest kept/stored X %.4f q, Y %.4f q (limbs %.4f x 2^28), ZZ %.4f q, ZZZ %.4f q\n",
                fn, s.col, s.col_line, s.margin, s.margin_line, s.top_margin, s.top_margin_line, s.wrap, s.wrap_line, s.norm, s.norm_line, s.stored[0], s.stored[1], s.stored_ylimb, s.stored[2], s.stored[3]);
  }
  std::printf("calls: madd %lu, double %lu, pair %lu, quad %lu (%d add cases; %lu additions with out == pa, %lu with an identity operand)\n", g_madds, g_calls_double, g_calls_pair, g_calls_quad, add_cases, g_alias_cases, g_inf_cases);
  std::printf("branches: madd_refused %lu, identity_copy_half %lu, identity_copy_quarter %lu, opposite_to_identity %lu, doubling %lu, two_torsion %lu, quad_to_pair %lu\n",
              g_madd_refused, g_copy_half, g_copy_quarter, g_identity, g_calls_double, g_two_torsion, g_quad_to_pair);
  std::printf("violations: limb %lu, column %lu, value %lu, closure %lu, sound %lu\n", g_viol[LIMB], g_viol[COLUMN], g_viol[VALUE], g_viol[CLOSURE], g_viol[SOUND]);
  std::printf("fp28_bounds_emul: %lu additions, %lu mixed additions, %lu mismatches, %lu limb-rule violations\n", g_adds[0] + g_adds[1], g_madds, g_mismatches, viol);
  return g_mismatches || viol ? 1 : 0;
}
