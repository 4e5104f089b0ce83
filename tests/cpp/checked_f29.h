// The 29-bit-limb field of the device lanes (aleo_amd/csrc/fr29.h and the guarded block of edwards29.h) for the programs that run a lane on the HOST
// (tests/cpp/*_lane_emul.cpp, tests/cpp/ed29_bounds_emul.cpp), over values and bounds together.
//
// An F29 here carries, next to its 9 concrete limbs, an upper bound per limb, an upper bound of the value as a multiple of r (32.32 fixed point, strict:
// value < vb r) and whether limbs 0..7 are exact digits.  Every primitive computes the concrete result the way the device does (products column by column with
// R = 2^261, differences with FR29_PAD), propagates the bounds from the operation alone — never from a comment — and checks its preconditions against the
// BOUNDS, so one run speaks for every input inside the bounds its operands carry, not for the pseudo-random values alone.  The kinds of rule:
//   limb     the operand class of a product (multiplicand limbs below 2^31.4, multiplier limbs 0..7 digits) or of a padded difference (minuend limbs <= 2^30,
//            subtrahend limbs 0..7 <= 2^30 - 2); no 32-bit wrap of a sum, a difference or a carry step
//   column   every product column, carry-in included, below 2^64, and what is left for the top limb below 2^32
//   value    a multiplicand below 2^261 into a product; a subtrahend's top limb covered by FR29_PAD[8] (any value below 18 r is); reduce_partial's precondition
//            (exact digits below 445 r) and its claim (below 3 r); the conditional subtraction of f29_canonical sees at most r; to_words sees below 2^256
//   closure  what a formula returns is again what it accepts (asked by the programs that drive formulas directly: f29_closure)
//   sound    every concrete limb and value is within its tracked bound (the bookkeeping of this file itself)
// A broken rule prints itself with the line of the source that called the primitive (__builtin_LINE() as a default argument) and is counted, by kind and in
// g_violations.  The slack of every rule is kept per calling function (or per t_formula, where a program names the formula it drives) and printed when the
// program ends.  With it: the qualifiers of device code defined away, the library's host path (records_host.hpp, which takes this F29 for the lanes it
// includes; F29_HEADER names a copy of it to include in its place, beside patched copies of the headers it includes), the programs' generator of field elements, and the opening of a program's case file.
// One program includes it once; it builds under g++ and under hipcc -x c++.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__

typedef unsigned __int128 u128;

// ---- the books: violations by kind, slack by formula -------------------------------------------------------------------------------------------------
enum Kind { LIMB, COLUMN, VALUE, CLOSURE, SOUND, NKINDS };
static const char* const KIND_NAME[NKINDS] = {"limb", "column", "value", "closure", "sound"};
static unsigned long g_violations = 0, g_viol[NKINDS];
struct Slack {
  unsigned long calls = 0;
  double col = 0; int col_line = 0;                              // largest product column as a fraction of 2^64
  double margin = 1e30; int margin_line = 0;                     // smallest FR29_PAD[i] - bound(b_i) over the limbs 0..7 of a difference, in limb units
  double top_margin = 1e30; int top_margin_line = 0;             // the same for the top limb, in units of r's top limb (~ multiples of r)
  double wrap = 0; int wrap_line = 0;                            // largest limb bound of a sum / difference / carry step / multiplicand as a fraction of 2^32
  double norm = 0; int norm_line = 0;                            // largest value bound into a product or normalise as a fraction of 2^261
  double stored[4] = {0, 0, 0, 0};                               // largest value bound returned per coordinate, in multiples of r (f29_closure)
};
static std::map<std::string, Slack> g_slack;
static const char* t_formula = nullptr;                          // the formula a program is driving; null: the name of the function that called the primitive
static Slack& book(const char* fn) {
  static const char* last_key = nullptr; static Slack* last = nullptr;
  const char* key = t_formula ? t_formula : fn;
  if (key != last_key) { last = &g_slack[key]; last_key = key; }
  return *last;
}
static void rule(bool ok, Kind k, const char* what, int line, const char* fn) {
  if (ok) return;
  ++g_violations;
  if (g_viol[k]++ < 4) std::fprintf(stderr, "%s rule broken: %s (line %d, %s)\n", KIND_NAME[k], what, line, t_formula ? t_formula : fn);
}
static void print_books() {
  for (const auto& kv : g_slack) {
    const Slack& s = kv.second;
    std::printf("slack %s: largest column %.4f of 2^64 (line %d); smallest subtrahend-limb margin %.0f units (line %d), top limb %.2f r (line %d); largest limb %.4f of 2^32 (line %d); "
                "largest value into a product or normalise %.6f of 2^261 (line %d)", kv.first.c_str(), s.col, s.col_line, s.margin > 1e29 ? -1.0 : s.margin, s.margin_line,
                s.top_margin > 1e29 ? -1.0 : s.top_margin, s.top_margin_line, s.wrap, s.wrap_line, s.norm, s.norm_line);
    if (s.stored[0] > 0 || s.stored[1] > 0 || s.stored[2] > 0 || s.stored[3] > 0) std::printf("; largest returned X %.4f r, Y %.4f r, Z %.4f r, T %.4f r", s.stored[0], s.stored[1], s.stored[2], s.stored[3]);
    std::printf("\n");
  }
  std::printf("violations: limb %lu, column %lu, value %lu, closure %lu, sound %lu\n", g_viol[LIMB], g_viol[COLUMN], g_viol[VALUE], g_viol[CLOSURE], g_viol[SOUND]);
  std::fflush(stdout);
}
static const int g_books_at_exit = std::atexit(print_books);     // every program prints its books as it ends, after its own last line

// ---- plain multi-precision helpers (320 bits: limb bounds reach 2^265, vb r reaches 2^300) --------------------------------------------------------------
struct Big { uint64_t w[5]; Big() { std::memset(w, 0, sizeof w); } };
static void big_add_shifted(Big& r, uint64_t x, int bit) {      // r += x << bit
  const int j = bit >> 6, sh = bit & 63; const u128 t = (u128)x << sh;
  const uint64_t add[2] = {(uint64_t)t, (uint64_t)(t >> 64)}; uint64_t c = 0;
  for (int q = j; q < 5; ++q) { const u128 s = (u128)r.w[q] + (q - j < 2 ? add[q - j] : 0) + c; r.w[q] = (uint64_t)s; c = (uint64_t)(s >> 64); }
}
static Big big_of_limbs(const uint64_t* l9) { Big r; for (int i = 0; i < 9; ++i) big_add_shifted(r, l9[i], 29 * i); return r; }
static Big big_of_limbs(const uint32_t* l9) { Big r; for (int i = 0; i < 9; ++i) big_add_shifted(r, l9[i], 29 * i); return r; }
static int big_cmp(const Big& a, const Big& b) { for (int i = 4; i >= 0; --i) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1; return 0; }
static Big big_mul64(const Big& a, uint64_t m) { Big r; uint64_t c = 0; for (int i = 0; i < 5; ++i) { const u128 t = (u128)a.w[i] * m + c; r.w[i] = (uint64_t)t; c = (uint64_t)(t >> 64); } return r; }
static Big big_shr(const Big& a, int n) {
  Big r; const int j = n >> 6, sh = n & 63;
  for (int i = 0; i + j < 5; ++i) { r.w[i] = a.w[i + j] >> sh; if (sh && i + j + 1 < 5) r.w[i] |= a.w[i + j + 1] << (64 - sh); }
  return r;
}
static Big big_pow2(int n) { Big r; r.w[n >> 6] = 1ull << (n & 63); return r; }

namespace aleo_mi355x {
static constexpr uint32_t M29 = 0x1fffffffu;
// r, and 19 r with its limbs raised by 2 * 2^29 (tools/gen_fr29_asm.py)
static constexpr uint32_t FR29_P[9] = {0x1u, 0x108c0000u, 0x42u, 0x14edfda0u, 0x1b00159au, 0x68f2e1bu, 0x155982d1u, 0xbd34594u, 0x12ab65u};
static constexpr uint32_t FR29_PAD[9] = {0x40000013u, 0x5a63fffeu, 0x400004edu, 0x4da9d2deu, 0x41019a78u, 0x5ca06c0fu, 0x55a4b584u, 0x40ae2a06u, 0x162b884u};
static constexpr uint32_t FR29_QMAGIC = 0xdb6u;
static constexpr uint32_t LAZY_MAX = 2833000000u;          // 2^31.4
}  // namespace aleo_mi355x

static const Big RB = big_of_limbs(aleo_mi355x::FR29_P);
static constexpr uint64_t UNIT = 1ull << 32;                     // value bounds are multiples of r in units of 2^-32
static Big r_times(uint64_t vb) { return big_shr(big_mul64(RB, vb), 32); }
static uint64_t top_limb_below(uint64_t vb) { const Big t = big_shr(r_times(vb), 232); return t.w[1] ? ~0ull : t.w[0]; }      // the top limb of any value < vb r
static const uint64_t RR48 = big_shr(RB, 213).w[0] + 1;          // r / 2^261, rounded up, in units of 2^-48
static uint64_t vb_covering(const Big& v) {                      // the smallest vb with v < vb r / 2^32
  uint64_t lo = 1, hi = 1ull << 43;
  while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (big_cmp(v, r_times(mid)) < 0) hi = mid; else lo = mid + 1; }
  return lo;
}
static const uint64_t VB_2_256 = vb_covering(big_pow2(256));     // 2^256 / r = 2.2085...
static const Big TWO261 = big_pow2(261), TWO256 = big_pow2(256);

// ---- fr29.h and the guarded block of edwards29.h, restated with bounds ------------------------------------------------------------------------------------
namespace aleo_mi355x {

struct F29 {
  uint32_t v[9];
  uint64_t b[9];              // v[i] <= b[i]
  uint64_t vb;                // value < vb r / 2^32
  bool exact;                 // limbs 0..7 are base-2^29 digits
};

static Big value_bound(const F29& a) {                           // the smaller of what the limb bounds and the value bound allow
  const Big byl = big_of_limbs(a.b), byv = r_times(a.vb);
  return big_cmp(byl, byv) < 0 ? byl : byv;
}
static void sound(const F29& r, int line, const char* fn) {
  bool ok = true;
  for (int i = 0; i < 9; ++i) ok = ok && r.v[i] <= r.b[i];
  if (r.exact) for (int i = 0; i < 8; ++i) ok = ok && r.b[i] <= M29;
  ok = ok && big_cmp(big_of_limbs(r.v), r_times(r.vb)) <= 0;
  rule(ok, SOUND, "a concrete limb or value exceeds its tracked bound", line, fn);
}
static void note_wrap(uint64_t bound, int line, const char* fn) { Slack& s = book(fn); const double f = (double)bound / 4294967296.0; if (f > s.wrap) { s.wrap = f; s.wrap_line = line; } }
static void note_norm(const Big& vbnd, int line, const char* fn) {
  Slack& s = book(fn); const double f = (double)big_shr(vbnd, 209).w[0] / 4503599627370496.0;      // / 2^52 after / 2^209
  if (f > s.norm) { s.norm = f; s.norm_line = line; }
}
// tags: exact digits, value < vb r — the bounds of a contract, whatever the concrete limbs are
static F29 exact_below(const uint32_t* limbs, uint64_t vb) {
  F29 r; for (int i = 0; i < 9; ++i) { r.v[i] = limbs[i]; r.b[i] = M29; }
  r.b[8] = top_limb_below(vb); r.vb = vb; r.exact = true; return r;
}

inline F29 f29_from_words(const uint32_t (&w)[8], int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  F29 r; r.v[0] = w[0] & M29;
  for (int i = 1; i < 8; ++i) r.v[i] = (uint32_t)((((uint64_t)w[i] << 32) | w[i - 1]) >> (32 - 3 * i)) & M29;
  r.v[8] = w[7] >> 8;
  for (int i = 0; i < 8; ++i) r.b[i] = M29;
  r.b[8] = 0xffffffu; r.vb = VB_2_256; r.exact = true; sound(r, line, fn); return r;
}
inline void f29_to_words(const F29& a, uint32_t (&w)[8], int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  rule(a.exact && big_cmp(value_bound(a), TWO256) <= 0, VALUE, "to_words can see loose limbs or a value of 2^256 or more", line, fn);
  for (int i = 0; i < 8; ++i) w[i] = (a.v[i] >> (3 * i)) | (a.v[i + 1] << (29 - 3 * i));
}
// nine limbs as they lie in a table or an argument block: bounded by their own value
inline F29 f29_limbs(const uint32_t* p, uint32_t at = 0, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  F29 r; r.exact = true; p += at;
  for (int i = 0; i < 9; ++i) { r.v[i] = p[i]; r.b[i] = p[i]; if (i < 8) r.exact = r.exact && p[i] <= M29; }
  // value < (v8 + 1) 2^232 <= (v8 + 1) / P8 r for exact digits; the search otherwise
  r.vb = r.exact ? (((uint64_t)p[8] + 1) << 32) / FR29_P[8] + 1 : vb_covering(big_of_limbs(r.v));
  sound(r, line, fn); return r;
}
inline F29 f29_small(uint32_t k, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {      // the plain number k
  F29 r; for (int i = 0; i < 9; ++i) { r.v[i] = 0; r.b[i] = 0; }
  r.v[0] = k; r.b[0] = k; r.vb = 1; r.exact = k <= M29; sound(r, line, fn); return r;
}
inline F29 f29_zero_if(bool c, const F29& a) { F29 r = a; for (int i = 0; i < 9; ++i) r.v[i] = c ? 0u : a.v[i]; return r; }      // the bounds of a cover zero
inline F29 f29_select(bool c, const F29& a, const F29& b) {
  F29 r = c ? a : b;
  for (int i = 0; i < 9; ++i) r.b[i] = a.b[i] > b.b[i] ? a.b[i] : b.b[i];
  r.vb = a.vb > b.vb ? a.vb : b.vb; r.exact = a.exact && b.exact; return r;
}

inline F29 f29_add(const F29& a, const F29& b, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  F29 r;
  for (int i = 0; i < 9; ++i) {
    r.b[i] = a.b[i] + b.b[i]; rule(r.b[i] < (1ull << 32), LIMB, "a limb of a sum wraps 32 bits", line, fn); note_wrap(r.b[i], line, fn);
    r.v[i] = a.v[i] + b.v[i];
  }
  r.vb = a.vb + b.vb; r.exact = false; sound(r, line, fn); return r;
}
inline F29 f29_sub_pad(const F29& a, const F29& b, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  F29 r; double margin = 1e30;
  for (int i = 0; i < 9; ++i) {
    rule(a.b[i] <= (1u << 30), LIMB, "the minuend of a padded difference has a limb above 2^30", line, fn);
    if (i < 8) {
      rule(b.b[i] <= (1u << 30) - 2, LIMB, "the subtrahend of a padded difference has a limb above 2^30 - 2", line, fn);
      const double mg = (double)FR29_PAD[i] - (double)b.b[i]; if (mg < margin) margin = mg;
    } else rule(b.b[8] <= FR29_PAD[8], VALUE, "the top limb of a padded difference can go negative (subtrahend not below 18 r)", line, fn);
    r.b[i] = a.b[i] + FR29_PAD[i]; rule(r.b[i] < (1ull << 32), LIMB, "a limb of a padded difference wraps 32 bits", line, fn); note_wrap(r.b[i], line, fn);
    r.v[i] = a.v[i] + FR29_PAD[i] - b.v[i];
  }
  r.vb = a.vb + 19 * UNIT; r.exact = false;
  {
    Slack& s = book(fn);
    if (margin < s.margin) { s.margin = margin; s.margin_line = line; }
    const double tm = ((double)FR29_PAD[8] - (double)b.b[8]) / (double)FR29_P[8];
    if (tm < s.top_margin) { s.top_margin = tm; s.top_margin_line = line; }
  }
  sound(r, line, fn); return r;
}
inline void f29_normalise(F29& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  const Big vbnd = value_bound(a);
  note_norm(vbnd, line, fn);                                      // normalise itself is bounded by its top limb alone (the carry steps below): f29_tidy takes up to 445 r
  uint64_t carry = 0; uint32_t c = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t in = a.b[i] + carry; rule(in < (1ull << 32), LIMB, "a carry step of normalise wraps 32 bits", line, fn); note_wrap(in, line, fn);
    carry = in >> 29;
    const uint32_t t = a.v[i] + c; c = t >> 29; a.v[i] = t & M29; a.b[i] = in < M29 ? in : M29;
  }
  const uint64_t top = a.b[8] + carry; rule(top < (1ull << 32), LIMB, "the top limb of normalise wraps 32 bits", line, fn);
  a.v[8] += c;
  const uint64_t tv = big_shr(vbnd, 232).w[0];
  a.b[8] = top < tv ? top : tv; a.exact = true; sound(a, line, fn);
}
// exact digits below 445 r -> exact digits below 3 r: the claim is not the operation's alone (it rests on how FR29_QMAGIC was chosen), so it is asserted
// on every concrete value
inline void f29_reduce_partial(F29& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  rule(a.exact && a.vb <= 445 * UNIT, VALUE, "reduce_partial can see loose limbs or a value of 445 r or more", line, fn);
  const uint32_t q = (uint32_t)(((uint64_t)a.v[8] * FR29_QMAGIC) >> 32);
  int64_t acc = 0;
  for (int i = 0; i < 8; ++i) { acc += (int64_t)a.v[i] - (int64_t)((uint64_t)q * FR29_P[i]); a.v[i] = (uint32_t)acc & M29; acc >>= 29; a.b[i] = M29; }
  const int64_t top = acc + (int64_t)a.v[8] - (int64_t)((uint64_t)q * FR29_P[8]);
  a.v[8] = (uint32_t)top;
  if (a.vb > 3 * UNIT) a.vb = 3 * UNIT;                            // q >= 0: never more than before
  a.b[8] = top_limb_below(a.vb);
  rule(top >= 0 && big_cmp(big_of_limbs(a.v), r_times(a.vb)) < 0, VALUE, "reduce_partial leaves a negative value or 3 r or more", line, fn);
  sound(a, line, fn);
}
// a * b * 2^-261 mod r with exact digits out, column by column as the generated device code does it
inline F29 f29_mul(const F29& a, const F29& b, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  for (int i = 0; i < 9; ++i) {
    rule(a.b[i] < LAZY_MAX, LIMB, "a product's multiplicand has a limb of 2^31.4 or more", line, fn); note_wrap(a.b[i], line, fn);
    if (i < 8) rule(b.b[i] <= M29, LIMB, "a product's multiplier is not normalised", line, fn);
  }
  const Big vbnd = value_bound(a);
  rule(big_cmp(vbnd, TWO261) <= 0, VALUE, "a product's multiplicand can exceed 2^261", line, fn); note_norm(vbnd, line, fn);
  uint32_t m[9]; F29 r; u128 acc = 0, bnd = 0; double worst = 0;
  for (int col = 0; col < 17; ++col) {
    for (int j = 0; j < 9; ++j) { const int k = col - j; if (k >= 0 && k < 9) { acc += (u128)a.v[j] * b.v[k]; bnd += (u128)a.b[j] * b.b[k]; } }
    for (int j = 0; j < 9 && j < col; ++j) { const int k = col - j; if (k >= 1 && k < 9) { acc += (u128)m[j] * FR29_P[k]; bnd += (u128)M29 * FR29_P[k]; } }
    if (col < 9) {
      m[col] = (uint32_t)(0 - (uint64_t)acc) & M29; acc += m[col]; bnd += M29;
      if ((uint64_t)acc & M29) { std::fprintf(stderr, "f29_mul: column %d does not clear\n", col); std::exit(2); }
    } else r.v[col - 9] = (uint32_t)acc & M29;
    rule(bnd < ((u128)1 << 64), COLUMN, "a product column can exceed 2^64", line, fn);
    const double f = (double)bnd / 18446744073709551616.0; if (f > worst) worst = f;
    acc >>= 29; bnd >>= 29;
  }
  rule(bnd < ((u128)1 << 32), COLUMN, "what is left for a product's top limb can exceed 2^32", line, fn);
  r.v[8] = (uint32_t)acc;
  const u128 ab32 = ((u128)a.vb * b.vb + (UNIT - 1)) >> 32;
  r.vb = (uint64_t)((ab32 * RR48 + (((u128)1 << 48) - 1)) >> 48) + UNIT;          // (A B r / 2^261 + 1) r
  for (int i = 0; i < 8; ++i) r.b[i] = M29;
  const uint64_t tv = top_limb_below(r.vb); r.b[8] = (uint64_t)bnd < tv ? (uint64_t)bnd : tv;
  r.exact = true;
  { Slack& s = book(fn); ++s.calls; if (worst > s.col) { s.col = worst; s.col_line = line; } }
  sound(r, line, fn); return r;
}
// r - (r >= the modulus ? the modulus : 0) for f29_canonical: what its product by the plain 1 leaves is at most r, a fact the bounds alone give only as
// "below (1 + 2^-32) r" — asserted on every concrete value
inline F29 f29_sub_r_if_ge(const F29& a, int line = __builtin_LINE(), const char* fn = __builtin_FUNCTION()) {
  rule(a.exact && a.vb <= 2 * UNIT, VALUE, "the conditional subtraction of f29_canonical can see loose limbs or 2 r or more", line, fn);
  rule(big_cmp(big_of_limbs(a.v), RB) <= 0, VALUE, "the product by the plain 1 left more than r", line, fn);
  F29 r = a; bool ge = true;
  for (int i = 0; i < 9; ++i) ge = r.v[i] > FR29_P[i] || (r.v[i] == FR29_P[i] && ge);
  int32_t br = 0;
  for (int i = 0; i < 9; ++i) { const int32_t t = (int32_t)r.v[i] - (ge ? (int32_t)FR29_P[i] : 0) + br; r.v[i] = (uint32_t)t & M29; br = t >> 29; }
  for (int i = 0; i < 8; ++i) r.b[i] = M29;
  r.b[8] = FR29_P[8]; r.vb = UNIT; r.exact = true; sound(r, line, fn); return r;
}
// for the programs that drive a formula directly: coordinate `which` of what it returned is exact digits below vmax r
inline void f29_closure(const F29& a, uint64_t vmax, int which, const char* what, const char* fn) {
  rule(a.exact && a.vb <= vmax, CLOSURE, what, 0, fn);
  Slack& s = book(fn); const double v = (double)a.vb / (double)UNIT; if (v > s.stored[which]) s.stored[which] = v;
}
}  // namespace aleo_mi355x

#define ALEO_F29_PROVIDED
#define ALEO_F29_LIMB_WRITES_PROVIDED
#ifndef F29_HEADER
#define F29_HEADER "records_host.hpp"
#endif
#include F29_HEADER

using namespace aleo_mi355x;

// the programs' generator: the same elements in every run
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static inline uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static inline void rnd_fr(uint8_t* out) { uint64_t v[4]; do { for (auto& x : v) x = rnd(); v[3] &= 0x1fffffffffffffffull; } while (HFr::geq_p(v)); std::memcpy(out, v, 32); }

// ---- a program's case file: its one argument, written by the test that runs it ---------------------------------------------------------------------------
static inline bool get(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
// The file, open, with the u32 it begins with in *count where one is asked for; null (the program returns 2) after the usage line, the system's error or a short file.
static inline std::FILE* open_cases(int argc, char** argv, uint32_t* count = nullptr) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return nullptr; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return nullptr; }
  if (count && !get(f, count, 4)) { std::fclose(f); return nullptr; }
  return f;
}
