// The 28-bit-limb field of the MSM point formulas (the guarded block of aleo_amd/csrc/fp28.h) for the programs that run those formulas on the HOST over
// values and bounds together: tests/cpp/fp28_bounds_emul.cpp (fp28.h), te28_bounds_emul.cpp (te28.h), g2p28_bounds_emul.cpp (g2p28.h).
//
// An F28 here carries, next to its 14 concrete limbs, an upper bound per limb, an upper bound of the value as a multiple of q (32.32 fixed point, strict:
// value < vb q) and whether the digits are exact.  Every primitive computes the concrete result the way the device does (products column by column with
// R' = 2^392, differences with the spread constant of spread_kq), propagates the bounds from the operation alone — never from a comment — and checks its
// preconditions against the BOUNDS, so one run speaks for every input inside the stated invariants.  The kinds of rule (limb, column, value, closure,
// sound) are described where the programs use them; a broken rule prints itself with the line of the header under test (the primitives take
// __builtin_LINE() as a default argument) and is counted.  A lane pair / quad is 2 / 4 host threads with a barrier inside each exchange helper; stores
// are held back until all lanes have returned, which is what lockstep execution gives the device where `out` aliases an operand.
// With it: the qualifiers of device code defined away, the books (violations by kind, slack by formula), the arena the formulas load from and store to,
// the programs' generator and the 28-bit Montgomery representatives of a residue.  It ends by defining ALEO_F28_PROVIDED and including FP28_HEADER
// (fp28.h, or a patched copy of it).  One program includes it once; no program includes another.
#pragma once
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
#define __noinline__
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
// the formula a lane is running, where its primitives are called from helpers (g2p28.h: every product sits in fq2p_mul); null: the calling function's own name
static thread_local const char* t_formula = nullptr;
static const char* book(const char* fn) { return t_formula ? t_formula : fn; }
static const char* g_formula_header = "fp28.h";                  // what the line numbers of a broken rule refer to (a program that checks another header says so)
static void rule(bool ok, Kind k, const char* what, int line, const char* fn) {
  if (ok) return;
  std::lock_guard<std::mutex> l(g_mu);
  if (g_viol[k]++ < 4) std::fprintf(stderr, "%s rule broken: %s (%s line %d, %s)\n", KIND_NAME[k], what, g_formula_header, line, fn);
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
static const Limbs14 ONE28 = [] {                                // 2^392 mod q: HFq keeps v 2^384, times 2^8 under its own product
  const HFq c = HFq::mul(HFq::one(), HFq::from_u64(256)); Big v; for (int i = 0; i < 6; ++i) v.w[i] = c.l[i];
  Limbs14 r; big_digits(v, r.v); return r;
}();
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
  std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[book(fn)]; const double f = (double)bound / 4294967296.0;
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
  { std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[book(fn)]; if (worst > s.col) { s.col = worst; s.col_line = line; } }
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
// 5 v limb-wise (g2p28.h's f28_neg5 then takes K q - 5 v with a spread of 6: f28_sub<K, 6> below checks the limbs and the value against that constant)
inline F28 f28_times5(const F28& v, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  F28 r;
  for (int i = 0; i < 14; ++i) {
    r.b[i] = 5 * v.b[i]; rule(r.b[i] < (1ull << 32), LIMB, "a limb of 5 v wraps 32 bits", line, fn); note_wrap(r.b[i], line, fn);
    r.v[i] = 5u * v.v[i];
  }
  r.vb = 5 * v.vb; r.exact = false; sound(r, line, fn); return r;
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
    std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[book(fn)];
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
  { std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[book(fn)]; const double f = (double)big_shr(vbnd, 340).w[0] / 4503599627370496.0; if (f > s.norm) { s.norm = f; s.norm_line = line; } }
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
static constexpr int ARENA_ROWS = 16;
alignas(16) static uint32_t g_arena[ARENA_ROWS][56];
static const uint64_t STORED_VB[4] = {12 * UNIT, 6 * UNIT, 2 * UNIT, 2 * UNIT};
static constexpr uint64_t L3_MAX = 3ull * (1u << 28) - 1;
// the stored point: X | Y | ZZ | ZZZ with g_components residues per coordinate (1: fp28.h's 224-byte points; 2: g2p28.h's 448-byte pair form, a-component
// then b-component), and whether a stored Y is exact digits (g2p28.h) or class L3 (fp28.h)
static int g_components = 1;
static bool g_stored_y_exact = false;
static int field_of(const void* p, int line, const char* fn) {
  const ptrdiff_t off = (const char*)p - (const char*)g_arena;
  if (off < 0 || off + 56 > (ptrdiff_t)sizeof g_arena || off % 56) { std::fprintf(stderr, "access outside the arena or not at a coordinate (%s line %d, %s)\n", g_formula_header, line, fn); std::exit(2); }
  return (int)(off / (56 * g_components)) % 4;
}
inline F28 load_f28(const void* p, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  const int f = field_of(p, line, fn); F28 r; std::memcpy(r.v, p, 56);
  const bool loose = f == 1 && !g_stored_y_exact;
  r.vb = STORED_VB[f]; r.exact = !loose;
  for (int i = 0; i < 13; ++i) r.b[i] = loose ? L3_MAX : F28::MASK;
  r.b[13] = top_limb_below(r.vb);
  sound(r, line, fn); return r;
}
struct Pending { char* p; uint32_t w[28]; int bytes; };
static std::vector<Pending> g_pending;                           // committed when every lane has returned
static void hold(char* p, const uint32_t* w, int bytes) { Pending s; s.p = p; s.bytes = bytes; std::memcpy(s.w, w, bytes); std::lock_guard<std::mutex> l(g_mu); g_pending.push_back(s); }
inline void store_f28(void* p, const F28& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  const int f = field_of(p, line, fn);
  bool ok = a.vb <= STORED_VB[f];
  if (f == 1 && !g_stored_y_exact) for (int i = 0; i < 14; ++i) ok = ok && a.b[i] <= L3_MAX; else ok = ok && a.exact;
  static const char* const what[4] = {"a stored X is not exact digits below 12q", "a stored Y is not class L3 below 6q", "a stored ZZ is not exact digits below 2q", "a stored ZZZ is not exact digits below 2q"};
  rule(ok, CLOSURE, f == 1 && g_stored_y_exact ? "a stored Y is not exact digits below 6q" : what[f], line, fn);
  {
    std::lock_guard<std::mutex> l(g_mu); Slack& s = g_slack[book(fn)]; const double v = (double)a.vb / (double)UNIT;
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
static std::map<std::string, unsigned long> g_lane_calls;        // by the name of the lane-group formula that asked for its lane
inline uint32_t f28_lane(int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {      // called once at the top of each lane-group formula
  if (t_lane == 0) {
    std::lock_guard<std::mutex> l(g_mu);
    ++g_lane_calls[fn];
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
  Barrier& b = t_grp->lanes == 2 ? t_grp->pair0 : t_grp->quad;      // a lane pair on its own may only read inside itself: lanes 0, 1 of the pattern
  if (t_grp->lanes == 2 && src[t_lane] > 1) { std::fprintf(stderr, "f28_qperm: a lone lane pair reads outside itself\n"); std::exit(2); }
  t_grp->slot[t_lane] = a; b.wait(); const F28 r = t_grp->slot[src[t_lane]]; b.wait(); return r;
}
// v in both lanes of the pair (an exchange: both lanes must arrive, whatever their own v)
inline bool f28_pair_and(bool v) { Barrier& b = pair_barrier(); t_grp->flag[t_lane] = v; b.wait(); const bool o = t_grp->flag[t_lane ^ 1] != 0; b.wait(); return v && o; }
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

// ---- what the programs share beyond the field ----------------------------------------------------------------------------------------------------
// the generator: the same elements in every run
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static HFq rnd_fq() { HFq r = HFq::from_u64(rnd()); for (int i = 0; i < 6; ++i) r = HFq::add(HFq::mul(r, HFq::from_u64(rnd())), HFq::from_u64(rnd())); return r; }
// canonical 28-bit Montgomery digits of a residue (HFq keeps v 2^384; times 2^8 under its own product gives v 2^392), plus k q
static Big mont28_value(const HFq& v, uint32_t k) {
  const HFq c = HFq::mul(v, HFq::from_u64(256)); Big r; for (int i = 0; i < 6; ++i) r.w[i] = c.l[i];
  return big_add(r, big_mul64(QB, k));
}
// that representative as an F28 tagged exact digits, value < vb q — the bounds of an invariant, whatever the concrete limbs are
static F28 tagged(const HFq& v, uint32_t k, uint64_t vb) { uint32_t d[14]; big_digits(mont28_value(v, k), d); return exact_below(d, vb); }
static void mismatch(const char* what, const char* why, int id) { if (g_mismatches++ < 10) std::fprintf(stderr, "mismatch: %s, case %d: %s\n", what, id, why); }
