// records_host.hpp — the host side of the record ownership scan (records.hip): the constants of a scan, the builder of the word tables the lanes read
// (WordTable: the scan's own, and those of the serial-number, commitment and signature lanes on top of it), the recoding of the scalar, and the whole test
// on the CPU from host_field.hpp and poseidon.hpp.  Plain C++ (no HIP): records.hip builds the library's entry points on it, and
// tests/cpp/records_lane_emul.cpp runs the device lane's code (records_lane.h) against it on the host (tests/cpp/checked_f29.h includes it over the checked field).
#pragma once
#include "records_lane.h"
#include "poseidon.hpp"
#include <cstring>
#include <vector>

namespace aleo_mi355x {

using host::HFr;

static constexpr uint64_t ED_ORDER[4] = {0xb95aee9ac33fd9ffULL, 0x5293a3afc43c8afeULL, 0x982d1347970dec00ULL, 0x04aad957a68b2955ULL};      // l: 251 bits, odd
static constexpr uint64_t ED_D = 3021;

// ---- what a scan needs besides its records: built once per process ----------------------------------------------------------------------------
struct HostSqrt { uint64_t t[4], e[4]; HFr c; };             // r - 1 = 2^47 t; e = (t - 1) / 2; c = 22^t generates the 2^47-th roots of unity
struct RecordsConsts {
  HFr s0[9], d, d2;                                          // the sponge after its first block (+ the encryption domain), 3021, 6042
  HostSqrt sq;
  std::vector<uint32_t> words;                               // the same for the device: records_lane.h RK_*
};

static void put_plain29(uint32_t* dst, const uint64_t* v) {  // a number of four words -> its 29-bit limbs
  for (int i = 0; i < 9; ++i) {
    const int pos = 29 * i, j = pos >> 6, sh = pos & 63;
    uint64_t w = v[j] >> sh; if (sh > 35 && j + 1 < 4) w |= v[j + 1] << (64 - sh);
    dst[i] = (uint32_t)w & 0x1fffffffu;
  }
}
static void put29(uint32_t* dst, const HFr& mont) {         // Montgomery R = 2^256 -> the limbs of value * 2^261 mod r
  static const HFr k32 = HFr::from_u64(32);
  put_plain29(dst, HFr::mul(mont, k32).l);
}

struct EdH { HFr X, Y, Z, T; };

// The words of a lane's table as the device reads them, for every host that builds one (records_consts below; serial_host.hpp, commit_host.hpp,
// signature_host.hpp): `total` words, zero but for the RK_* prefix when there is one, then entries of nine limbs each at entry index idx.
struct WordTable {
  std::vector<uint32_t> words; HFr d2;
  explicit WordTable(size_t total) : words(total, 0) {}                                          // the records constants themselves
  WordTable(size_t total, const RecordsConsts& C) : words(total, 0), d2(C.d2) { std::memcpy(words.data(), C.words.data(), RK_WORDS * 4); }
  void put(uint32_t idx, const HFr& v) { put29(words.data() + 9 * idx, v); }
  void put_plain(uint32_t idx, const uint64_t* v) { put_plain29(words.data() + 9 * idx, v); }   // a number as it stands, not in Montgomery form
  void put_cached(uint32_t idx, const EdH& p) { put(idx, HFr::sub(p.Y, p.X)); put(idx + 1, HFr::add(p.Y, p.X)); put(idx + 2, HFr::mul(p.T, d2)); }      // Z = 1: (Y - X, Y + X, T 2d)
  void put_exponent(uint32_t word, const uint64_t* e) { for (int i = 0; i < 4; ++i) { words[word + 2 * i] = (uint32_t)e[i]; words[word + 2 * i + 1] = (uint32_t)(e[i] >> 32); } }      // at a word index
};

static const RecordsConsts& records_consts() {
  static const RecordsConsts C = [] {
    RecordsConsts c;
    const auto& P = host::PoseidonParams<4, 8>::get();
    c.d = HFr::from_u64(ED_D); c.d2 = HFr::dbl(c.d);
    // r - 1 = 2^47 t
    uint64_t rm1[4]; std::memcpy(rm1, host::HParams<4>::P, 32); rm1[0] -= 1;
    auto shr = [](uint64_t* o, const uint64_t* a, int s) { for (int i = 0; i < 4; ++i) o[i] = (a[i] >> s) | (i + 1 < 4 ? a[i + 1] << (64 - s) : 0); };
    shr(c.sq.t, rm1, host::FR_TWO_ADICITY);
    uint64_t tm1[4]; std::memcpy(tm1, c.sq.t, 32); tm1[0] -= 1;      // t is odd
    shr(c.sq.e, tm1, 1);
    c.sq.c = HFr::pow(HFr::from_u64(host::FR_GENERATOR), c.sq.t, 4);
    // the sponge after [AleoPoseidon8, 2, 0 x 6]
    HFr s[9]; for (auto& v : s) v = HFr::zero();
    s[1] = host::fr_domain_separator("AleoPoseidon8"); s[2] = HFr::from_u64(2);
    host::poseidon_permute<4, 8>(s);
    s[1] = HFr::add(s[1], host::fr_domain_separator("AleoSymmetricEncryption0"));
    for (int i = 0; i < 9; ++i) c.s0[i] = s[i];
    // the device's copy
    WordTable w(RK_WORDS);
    w.put(RK_R2, HFr::pow_u64(HFr::from_u64(2), 261)); w.put(RK_ONE, HFr::one()); w.put(RK_D, c.d); w.put(RK_D2, c.d2);
    for (int i = 0; i < 9; ++i) w.put(RK_S0 + i, c.s0[i]);
    constexpr int H = host::POSEIDON_FULL / 2, RP = host::POSEIDON_PARTIAL;
    for (int r = 0; r < H; ++r) for (int i = 0; i < 9; ++i) w.put(RK_ARK_HEAD + 9 * r + i, P.ark[r][i]);
    for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) { w.put(RK_MDS + 9 * i + j, P.mds[i][j]); w.put(RK_PRE + 9 * i + j, P.pre[i][j]); }
    for (int j = 0; j < RP; ++j) {
      const uint32_t base = RK_PART + 18 * j;
      w.put(base, P.sp_c[j]); w.put(base + 1, P.sp_m00[j]);
      for (int i = 0; i < 8; ++i) { w.put(base + 2 + i, P.sp_v[j][i]); w.put(base + 10 + i, P.sp_w[j][i]); }
    }
    for (int i = 0; i < 9; ++i) w.put(RK_ARK_AFTER + i, P.ark_after[i]);
    for (int r = 0; r < 3; ++r) for (int i = 0; i < 9; ++i) w.put(RK_ARK_TAIL + 9 * r + i, P.ark[H + RP + 1 + r][i]);
    HFr g = c.sq.c;
    for (int j = 0; j < RK_TWO_ADICITY; ++j) { w.put(RK_ROOTS + j, g); g = HFr::sqr(g); }
    uint64_t rm2[4]; std::memcpy(rm2, host::HParams<4>::P, 32); rm2[0] -= 2;
    w.put_exponent(RK_EXP_SQRT, c.sq.e); w.put_exponent(RK_EXP_INV, rm2);
    c.words = std::move(w.words);
    return c;
  }();
  return C;
}

// The non-adjacent form of the odd one of {v, v + l}: digit i is +1 where bit i of pos is set, -1 where bit i of neg is set.  At most 253 digits; the top one is +1.
static void recode_scalar(ScanArgs& a, const uint64_t* v4) {
  uint64_t k[5] = {v4[0], v4[1], v4[2], v4[3], 0};
  if (!(k[0] & 1)) { unsigned __int128 cy = 0; for (int i = 0; i < 4; ++i) { cy += (unsigned __int128)k[i] + ED_ORDER[i]; k[i] = (uint64_t)cy; cy >>= 64; } }
  std::memset(a.naf_pos, 0, sizeof a.naf_pos); std::memset(a.naf_neg, 0, sizeof a.naf_neg);
  uint32_t i = 0;
  while (k[0] | k[1] | k[2] | k[3] | k[4]) {
    if (k[0] & 1) {
      if ((k[0] & 3) == 1) { a.naf_pos[i >> 5] |= 1u << (i & 31); k[0] &= ~1ull; }
      else { a.naf_neg[i >> 5] |= 1u << (i & 31); for (int q = 0; q < 5 && ++k[q] == 0; ++q) {} }
    }
    for (int q = 0; q < 4; ++q) k[q] = (k[q] >> 1) | (k[q + 1] << 63);
    k[4] >>= 1; ++i;
  }
  a.naf_len = i;
}

// ---- the host path --------------------------------------------------------------------------------------------------------------------------------
static inline void edh_dbl(EdH& p) {                         // dbl-2008-hwcd, a = -1
  const HFr A = HFr::sqr(p.X), B = HFr::sqr(p.Y), C = HFr::dbl(HFr::sqr(p.Z)), E = HFr::sub(HFr::sub(HFr::sqr(HFr::add(p.X, p.Y)), A), B);
  const HFr G = HFr::sub(B, A), F = HFr::sub(G, C), Hh = HFr::neg(HFr::add(A, B));
  p.X = HFr::mul(E, F); p.Y = HFr::mul(G, Hh); p.T = HFr::mul(E, Hh); p.Z = HFr::mul(F, G);
}
static inline void edh_add(EdH& p, const EdH& q, bool neg, const HFr& d2) {      // add-2008-hwcd-3; -q = (-X, Y, Z, -T)
  const HFr qx = neg ? HFr::neg(q.X) : q.X, qt = neg ? HFr::neg(q.T) : q.T;
  const HFr A = HFr::mul(HFr::sub(p.Y, p.X), HFr::sub(q.Y, qx)), B = HFr::mul(HFr::add(p.Y, p.X), HFr::add(q.Y, qx));
  const HFr C = HFr::mul(HFr::mul(p.T, d2), qt), D = HFr::dbl(HFr::mul(p.Z, q.Z));
  const HFr E = HFr::sub(B, A), F = HFr::sub(D, C), G = HFr::add(D, C), Hh = HFr::add(B, A);
  p.X = HFr::mul(E, F); p.Y = HFr::mul(G, Hh); p.T = HFr::mul(E, Hh); p.Z = HFr::mul(F, G);
}
static bool hfr_sqrt(HFr& r, const HFr& a, const HostSqrt& S) {      // Tonelli-Shanks (as wire.hip's for Fq); either root
  if (a.is_zero()) { r = a; return true; }
  const HFr y = HFr::pow(a, S.e, 4);
  HFr x = HFr::mul(y, a), b = HFr::mul(x, y), c = S.c; int m = host::FR_TWO_ADICITY;
  const HFr one = HFr::one();
  while (!(b == one)) {
    int i = 0; HFr b2 = b;
    while (!(b2 == one)) { b2 = HFr::sqr(b2); if (++i >= m) return false; }
    HFr e = c; for (int k = 0; k < m - i - 1; ++k) e = HFr::sqr(e);
    x = HFr::mul(x, e); c = HFr::sqr(e); b = HFr::mul(b, c); m = i;
  }
  r = x; return true;
}

// one record on the host: the flag, and the canonical record view key x (zeros with flag 2) into rvk32 when given
static uint8_t scan_one_host(uint8_t* rvk32, const uint8_t* c0_32, const uint8_t* nx_32, const ScanArgs& a, const HFr& addr_mont, const RecordsConsts& C) {
  if (rvk32) std::memset(rvk32, 0, 32);
  HFr c0, nx; std::memcpy(c0.l, c0_32, 32); std::memcpy(nx.l, nx_32, 32);
  if (HFr::geq_p(c0.l) || HFr::geq_p(nx.l)) return 2;
  const HFr x = HFr::to_mont(nx), xx = HFr::sqr(x), one = HFr::one();
  const HFr w = HFr::sub(one, HFr::mul(C.d, xx)), u = HFr::add(one, xx);
  HFr s; if (w.is_zero() || !hfr_sqrt(s, HFr::mul(u, w), C.sq)) return 2;      // not on the curve
  EdH p; p.X = HFr::mul(x, w); p.Y = s; p.Z = w; p.T = HFr::mul(x, s);
  const EdH base = p;
  for (int i = (int)a.naf_len - 2; i >= 0; --i) {
    edh_dbl(p);
    if ((a.naf_pos[i >> 5] >> (i & 31)) & 1u) edh_add(p, base, false, C.d2);
    else if ((a.naf_neg[i >> 5] >> (i & 31)) & 1u) edh_add(p, base, true, C.d2);
  }
  const HFr rvk = HFr::mul(p.X, HFr::inv(p.Z));
  if (rvk32) { const HFr o = HFr::from_mont(rvk); std::memcpy(rvk32, o.l, 32); }
  HFr st[9]; for (int i = 0; i < 9; ++i) st[i] = C.s0[i];
  st[2] = HFr::add(st[2], rvk);
  host::poseidon_permute<4, 8>(st);
  return HFr::sub(HFr::to_mont(c0), st[1]) == addr_mont ? 1 : 0;
}

// the per-call arguments from the caller's key and address; returns what is wrong with them, or nullptr
static const char* scan_args(ScanArgs& a, HFr& addr_mont, const void* view_key32, const void* address_x32) {
  uint64_t v[4]; std::memcpy(v, view_key32, 32);
  bool below = false;
  for (int i = 3; i >= 0; --i) { if (v[i] < ED_ORDER[i]) { below = true; break; } if (v[i] > ED_ORDER[i]) break; }
  if (!below) return "records_scan: the view key is not a canonical scalar below the subgroup order";
  HFr ax; std::memcpy(ax.l, address_x32, 32);
  if (HFr::geq_p(ax.l)) return "records_scan: the address x-coordinate is not a canonical field element";
  recode_scalar(a, v);
  addr_mont = HFr::to_mont(ax);
  put_plain29(a.addr, ax.l);
  return nullptr;
}

// ---- the decryption of one record's private fields (records_decrypt.hip, records_found_host.hpp) ------------------------------------------------------------
// one record on the host: the flag, and its m plain rows (zeros with flag 2)
static uint8_t decrypt_one_host(uint8_t* plain, const uint8_t* rvk32, const uint8_t* fields, size_t m) {
  HFr rv; std::memcpy(rv.l, rvk32, 32);
  bool bad = HFr::geq_p(rv.l);
  std::vector<HFr> c(m), rnd(m);
  for (size_t j = 0; j < m; ++j) { std::memcpy(c[j].l, fields + 32 * j, 32); bad = bad || HFr::geq_p(c[j].l); }
  if (bad) { std::memset(plain, 0, 32 * m); return 2; }
  if (!m) return 0;
  static const HFr dom = host::fr_domain_separator("AleoSymmetricEncryption0");
  const HFr in[2] = {dom, HFr::to_mont(rv)};
  host::poseidon_hash_many_fr<8>(in, 2, rnd.data(), m);
  for (size_t j = 0; j < m; ++j) { const HFr o = HFr::from_mont(HFr::sub(HFr::to_mont(c[j]), rnd[j])); std::memcpy(plain + 32 * j, o.l, 32); }
  return 0;
}

}  // namespace aleo_mi355x
