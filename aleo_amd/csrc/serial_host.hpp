// serial_host.hpp — the host side of a record's serial number (records_serial.hip): Blake2s and Blake2Xs, hash-to-curve, the account generator, BHP (bases,
// randomizer bases, lookup tables; hash and commit), Poseidon hash-to-group with Elligator2, the serial number itself, and the tables the device lane reads
// (records_serial_lane.h).  Plain C++ (no HIP, touches no device); everything built once per process behind function-local statics (thread-safe).
//
// snarkVM 0.14.5 [UPSTREAM-RECALL], restated first in tests/serial_ref.py and pinned there, stage by stage, by data the reference holds:
//   console/algorithms/src/blake2xs/{mod,hash_to_curve}.rs   message "{s} in {k}", 32-byte Blake2Xs digest, personalisation "AleoHtC0", from_random_bytes
//                                                           (bit 7 of the last byte: the greater y; spare bits masked; x >= r refused), times the cofactor,
//                                                           the first non-zero result — pinned: the account generator reproduces all reference accounts
//   console/algorithms/src/bhp/                              BHP<windows, size>, 3-bit chunks, bases "Aleo.BHP.{windows}.{size}.{domain}.{w}", randomizer base
//                                                           "Aleo.BHP.{windows}.{size}.{domain}.Randomizer" (capital R: what the serial-number vector decides) —
//                                                           BHP1024 pinned by a transaction's record checksum and id, BHP512's commit by the serial number
//   console/algorithms/src/{poseidon/hash_to_group,elligator2/encode}.rs, console/program/src/data/record/serial_number.rs — pinned by the reference's
//                                                           serial-number test (wasm/src/record/record_plaintext.rs:131-140).  Of Elligator2's square root the
//                                                           vector fixes the sign for two inputs, for which "not above (r - 1) / 2" (taken here), "even" and
//                                                           Tonelli-Shanks' own output coincide; the opposite sign is ruled out.
#pragma once
#include "records_host.hpp"
#include "records_serial_lane.h"
#include <string>

namespace aleo_mi355x { namespace serial {

using host::HFr;

// ---- Blake2s (RFC 7693) with its whole parameter block, and Blake2Xs --------------------------------------------------------------------------------------
struct Blake2sParams { uint8_t digest_length = 32, fanout = 1, depth = 1; uint32_t leaf_length = 0; uint64_t node_offset = 0; uint8_t node_depth = 0, inner_length = 0; uint8_t personal[8] = {0, 0, 0, 0, 0, 0, 0, 0}; };
static inline uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static void blake2s_compress(uint32_t (&h)[8], const uint8_t* block, uint64_t t, bool last) {
  static const uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  static const uint8_t SIGMA[10][16] = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}, {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},
    {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8}, {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10}, {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  uint32_t m[16], v[16];
  for (int i = 0; i < 16; ++i) std::memcpy(&m[i], block + 4 * i, 4);
  for (int i = 0; i < 8; ++i) { v[i] = h[i]; v[8 + i] = IV[i]; }
  v[12] ^= (uint32_t)t; v[13] ^= (uint32_t)(t >> 32);
  if (last) v[14] = ~v[14];
  auto g = [&](int a, int b, int c, int d, uint32_t x, uint32_t y) {
    v[a] += v[b] + x; v[d] = rotr32(v[d] ^ v[a], 16); v[c] += v[d]; v[b] = rotr32(v[b] ^ v[c], 12);
    v[a] += v[b] + y; v[d] = rotr32(v[d] ^ v[a], 8); v[c] += v[d]; v[b] = rotr32(v[b] ^ v[c], 7);
  };
  for (int r = 0; r < 10; ++r) {
    const uint8_t* s = SIGMA[r];
    g(0, 4, 8, 12, m[s[0]], m[s[1]]); g(1, 5, 9, 13, m[s[2]], m[s[3]]); g(2, 6, 10, 14, m[s[4]], m[s[5]]); g(3, 7, 11, 15, m[s[6]], m[s[7]]);
    g(0, 5, 10, 15, m[s[8]], m[s[9]]); g(1, 6, 11, 12, m[s[10]], m[s[11]]); g(2, 7, 8, 13, m[s[12]], m[s[13]]); g(3, 4, 9, 14, m[s[14]], m[s[15]]);
  }
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[8 + i];
}
// unkeyed; out: P.digest_length bytes
static void blake2s(uint8_t* out, const uint8_t* data, size_t n, const Blake2sParams& P) {
  static const uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  uint8_t block[32] = {P.digest_length, 0, P.fanout, P.depth};
  std::memcpy(block + 4, &P.leaf_length, 4);
  for (int i = 0; i < 6; ++i) block[8 + i] = (uint8_t)(P.node_offset >> (8 * i));
  block[14] = P.node_depth; block[15] = P.inner_length;
  std::memcpy(block + 24, P.personal, 8);
  uint32_t h[8];
  for (int i = 0; i < 8; ++i) { uint32_t w; std::memcpy(&w, block + 4 * i, 4); h[i] = IV[i] ^ w; }
  size_t t = 0;
  while (n - t > 64) { blake2s_compress(h, data + t, t + 64, false); t += 64; }
  uint8_t last[64] = {0};
  if (n - t) std::memcpy(last, data + t, n - t);
  blake2s_compress(h, last, n, true);
  uint8_t full[32]; std::memcpy(full, h, 32);
  std::memcpy(out, full, P.digest_length);
}
// Blake2Xs::evaluate: H0 with the output length in the upper 16 bits of the 48-bit node offset, then one expansion node per 32 bytes of output
static std::vector<uint8_t> blake2xs(const uint8_t* data, size_t n, uint16_t xof_length, const char* personal) {
  Blake2sParams P; std::memcpy(P.personal, personal, std::strlen(personal) < 8 ? std::strlen(personal) : 8);
  P.node_offset = (uint64_t)xof_length << 32;
  uint8_t h0[32]; blake2s(h0, data, n, P);
  std::vector<uint8_t> out(xof_length);
  for (uint32_t node = 0; 32 * node < xof_length; ++node) {
    Blake2sParams Q = P;
    Q.digest_length = (uint8_t)(xof_length - 32 * node < 32 ? xof_length - 32 * node : 32);
    Q.fanout = 0; Q.depth = 0; Q.leaf_length = 32; Q.node_offset = ((uint64_t)xof_length << 32) | node; Q.inner_length = 32;
    blake2s(out.data() + 32 * node, h0, 32, Q);
  }
  return out;
}

// ---- Edwards-BLS12 on the host: the extended coordinates of records_host.hpp (EdH, edh_dbl, edh_add: complete, any pair of points) ------------------------------
struct EdA { HFr x, y; };                                    // affine, Montgomery form
static inline const HFr& ed_d2() { static const HFr v = HFr::dbl(HFr::from_u64(ED_D)); return v; }
static inline EdH edh_of(const EdA& a) { EdH p; p.X = a.x; p.Y = a.y; p.Z = HFr::one(); p.T = HFr::mul(a.x, a.y); return p; }
static inline EdH edh_identity() { EdH p; p.X = HFr::zero(); p.Y = HFr::one(); p.Z = HFr::one(); p.T = HFr::zero(); return p; }
static inline EdA edh_affine(const EdH& p) { const HFr zi = HFr::inv(p.Z); return {HFr::mul(p.X, zi), HFr::mul(p.Y, zi)}; }
static inline EdH edh_normalised(const EdH& p) { return edh_of(edh_affine(p)); }      // Z = 1: a table entry
static inline bool edh_is_identity(const EdH& p) { return p.X.is_zero() && p.Y == p.Z; }
static inline bool canon_less(const HFr& a_mont, const HFr& b_mont) {      // a < b as numbers
  const HFr a = HFr::from_mont(a_mont), b = HFr::from_mont(b_mont);
  for (int i = 3; i >= 0; --i) { if (a.l[i] < b.l[i]) return true; if (a.l[i] > b.l[i]) return false; }
  return false;
}
// k p for a scalar below l and a point of the prime-order subgroup: the digits of the odd one of {k, k + l} (recode_scalar), whose top digit is +1
static EdH edh_mul_naf(const EdH& base, const ScanArgs& a) {
  EdH p = base;
  for (int i = (int)a.naf_len - 2; i >= 0; --i) {
    edh_dbl(p);
    if ((a.naf_pos[i >> 5] >> (i & 31)) & 1u) edh_add(p, base, false, ed_d2());
    else if ((a.naf_neg[i >> 5] >> (i & 31)) & 1u) edh_add(p, base, true, ed_d2());
  }
  return p;
}
static inline bool scalar_below_order(const uint64_t* v) { for (int i = 3; i >= 0; --i) { if (v[i] < ED_ORDER[i]) return true; if (v[i] > ED_ORDER[i]) return false; } return false; }

// Blake2Xs::hash_to_curve
static EdA hash_to_curve(const std::string& s) {
  const RecordsConsts& C = records_consts();
  const HFr one = HFr::one();
  for (int k = 0; k < 128; ++k) {
    const std::string msg = s + " in " + std::to_string(k);
    std::vector<uint8_t> dg = blake2xs((const uint8_t*)msg.data(), msg.size(), 32, "AleoHtC0");
    const bool greatest = dg[31] & 0x80; dg[31] &= 0x1f;
    HFr xc; std::memcpy(xc.l, dg.data(), 32);
    if (HFr::geq_p(xc.l) || xc.is_zero()) continue;          // x = 0 is the identity, which the cofactor leaves zero
    const HFr x = HFr::to_mont(xc), xx = HFr::sqr(x), den = HFr::sub(HFr::mul(C.d, xx), one);
    HFr y;
    if (den.is_zero() || !hfr_sqrt(y, HFr::mul(HFr::neg(HFr::add(xx, one)), HFr::inv(den)), C.sq)) continue;
    const HFr ny = HFr::neg(y);
    EdH p = edh_of({x, canon_less(y, ny) != greatest ? y : ny});
    edh_dbl(p); edh_dbl(p);
    if (!edh_is_identity(p)) return edh_affine(p);
  }
  return {HFr::zero(), HFr::one()};                          // upstream panics; 2^-128
}
static const EdA& account_generator() { static const EdA g = hash_to_curve("AleoAccountEncryptionAndSignatureScheme0"); return g; }

// ---- BHP ------------------------------------------------------------------------------------------------------------------------------------------------------
static constexpr int BHP_DATA_BITS = 252, BHP_SCALAR_BITS = 251;
struct Bhp {
  int windows, size;
  std::vector<EdH> lookup;                                   // [(w * size + j) * 4 + k - 1] = k 2^(4 j) base_w, k = 1 .. 4, Z = 1
  std::vector<EdH> random_base;                              // 2^i R, Z = 1
  std::vector<uint8_t> domain;                               // the domain's bits, zero-padded to 252 - 64, reversed
  Bhp(int windows_, int size_, const char* name) : windows(windows_), size(size_) {
    const std::string tag = "Aleo.BHP." + std::to_string(windows) + "." + std::to_string(size) + "." + name + ".";
    for (int w = 0; w < windows; ++w) {
      EdH base = edh_of(hash_to_curve(tag + std::to_string(w)));
      for (int j = 0; j < size; ++j) {
        EdH two = base; edh_dbl(two);
        EdH three = two; edh_add(three, base, false, ed_d2());
        EdH four = two; edh_dbl(four);
        lookup.push_back(edh_normalised(base)); lookup.push_back(edh_normalised(two)); lookup.push_back(edh_normalised(three)); lookup.push_back(edh_normalised(four));
        base = four; edh_dbl(base); edh_dbl(base);
      }
    }
    EdH g = edh_of(hash_to_curve(tag + "Randomizer"));
    for (int i = 0; i < BHP_SCALAR_BITS; ++i) { random_base.push_back(edh_normalised(g)); edh_dbl(g); }
    domain.assign(BHP_DATA_BITS - 64, 0);
    const size_t n = std::strlen(name);
    for (size_t i = 0; i < 8 * n && i < domain.size(); ++i) domain[domain.size() - 1 - i] = (name[i >> 3] >> (i & 7)) & 1;
  }
  // the hasher over at most windows * size * 3 bits, padded to whole chunks, from chunk `first` on (bits[0] is that chunk's first bit)
  void add_chunks(EdH& acc, const uint8_t* bits, size_t n, size_t first = 0) const {
    for (size_t c = 0; 3 * c < n; ++c) {
      auto bit = [&](size_t i) -> unsigned { return i < n ? bits[i] : 0u; };
      edh_add(acc, lookup[4 * (first + c) + (bit(3 * c) | bit(3 * c + 1) << 1)], bit(3 * c + 2) != 0, ed_d2());
    }
  }
  EdH hash_uncompressed(const std::vector<uint8_t>& bits) const {
    const size_t per = (size_t)windows * size * 3 - BHP_DATA_BITS;
    EdH digest = edh_identity();
    std::vector<uint8_t> pre;
    for (size_t at = 0; at == 0 || at < bits.size(); at += per) {
      pre.clear();
      if (at == 0) { pre = domain; for (int i = 0; i < 64; ++i) pre.push_back(((uint64_t)bits.size() >> i) & 1); }
      else { const HFr x = HFr::from_mont(edh_affine(digest).x); for (int i = 0; i < BHP_DATA_BITS; ++i) pre.push_back((x.l[i >> 6] >> (i & 63)) & 1); }
      const size_t m = bits.size() - at < per ? bits.size() - at : per;
      pre.insert(pre.end(), bits.begin() + at, bits.begin() + at + m);
      digest = edh_identity();
      add_chunks(digest, pre.data(), pre.size());
    }
    return digest;
  }
  HFr hash(const std::vector<uint8_t>& bits) const { return edh_affine(hash_uncompressed(bits)).x; }      // Montgomery form
  // randomizer: a canonical scalar (251 bits)
  HFr commit(const std::vector<uint8_t>& bits, const uint64_t* randomizer) const {
    EdH acc = hash_uncompressed(bits);
    for (int i = 0; i < BHP_SCALAR_BITS; ++i) if ((randomizer[i >> 6] >> (i & 63)) & 1) edh_add(acc, random_base[i], false, ed_d2());
    return edh_affine(acc).x;
  }
};
static const Bhp& bhp512() { static const Bhp b(6, 43, "AleoBHP512"); return b; }
static const Bhp& bhp1024() { static const Bhp b(8, 54, "AleoBHP1024"); return b; }
static inline void push_field_bits(std::vector<uint8_t>& bits, const uint64_t* canonical, int n = 253) { for (int i = 0; i < n; ++i) bits.push_back((canonical[i >> 6] >> (i & 63)) & 1); }

// ---- Elligator2, hash-to-group, the serial number -----------------------------------------------------------------------------------------------------------
struct SerialTables {
  HFr a, b, neg_a, a2, mb, dom;                              // y^2 = x^3 + a x^2 + b x; the Montgomery B; the domain separator "AleoSerialNumber0"
  HFr s0[3];                                                 // the sponge after [AleoPoseidon2, 2], dom added to its first rate element
  EdH start;                                                 // BHP512's chunks 0 .. 167 of a serial number's preimage
  std::vector<EdH> rnd;                                      // 63 x 16: v 2^(4 w) R (entry 0 the identity)
  std::vector<uint32_t> words;                               // records_lane.h RK_* and records_serial_lane.h SK_*
};

// Elligator2::encode without the cofactor: false where upstream returns Err.  r in Montgomery form.
static bool elligator2(EdH& out, const HFr& r, const SerialTables& T) {
  const RecordsConsts& C = records_consts();
  const HFr one = HFr::one();
  if (r.is_zero()) return false;
  const HFr ur2 = HFr::mul(C.d, HFr::sqr(r)), q = HFr::add(one, ur2);
  if (HFr::mul(T.a2, ur2) == HFr::mul(T.b, HFr::sqr(q))) return false;
  auto curve = [&](const HFr& x) { return HFr::mul(x, HFr::add(HFr::add(HFr::sqr(x), HFr::mul(T.a, x)), T.b)); };
  const HFr v = HFr::mul(T.neg_a, HFr::inv(q)), gv = curve(v);
  if (gv.is_zero()) return false;                            // v = 0, or the symbol is 0 and y with it
  HFr s;
  const bool qr = hfr_sqrt(s, gv, C.sq);
  const HFr x = qr ? v : HFr::sub(T.neg_a, v), g = curve(x);
  if (x.is_zero() || g.is_zero() || !hfr_sqrt(s, g, C.sq)) return false;
  const HFr ns = HFr::neg(s), small = canon_less(s, ns) ? s : ns;
  const HFr y = qr ? HFr::neg(small) : small;                // -e * the root not above (r - 1) / 2
  const HFr u = HFr::mul(x, T.mb), w = HFr::mul(y, T.mb), up = HFr::add(u, one), um = HFr::sub(u, one);
  if (up.is_zero()) return false;
  out.X = HFr::mul(u, up); out.Y = HFr::mul(um, w); out.Z = HFr::mul(w, up); out.T = HFr::mul(u, um);      // (u / w, (u - 1) / (u + 1))
  return true;
}

static const SerialTables& serial_tables() {
  static const SerialTables T = [] {
    SerialTables t;
    const RecordsConsts& C = records_consts();
    const HFr one = HFr::one(), amd = HFr::neg(HFr::add(one, C.d)), amd_inv = HFr::inv(amd);      // a - d of the Edwards form, a = -1
    const HFr ma = HFr::mul(HFr::dbl(HFr::sub(C.d, one)), amd_inv), mb = HFr::mul(HFr::from_u64(4), amd_inv), mb_inv = HFr::inv(mb);
    t.a = HFr::mul(ma, mb_inv); t.b = HFr::sqr(mb_inv); t.neg_a = HFr::neg(t.a); t.a2 = HFr::sqr(t.a); t.mb = mb;
    t.dom = host::fr_domain_separator("AleoSerialNumber0");
    t.s0[0] = HFr::zero(); t.s0[1] = host::fr_domain_separator("AleoPoseidon2"); t.s0[2] = HFr::from_u64(2);
    host::poseidon_permute<4, 2>(t.s0);
    t.s0[1] = HFr::add(t.s0[1], t.dom);
    const Bhp& B = bhp512();
    std::vector<uint8_t> pre = B.domain;
    for (int i = 0; i < 64; ++i) pre.push_back(((uint64_t)506 >> i) & 1);
    const HFr domc = HFr::from_mont(t.dom);
    push_field_bits(pre, domc.l, 252);                       // 504 bits = 168 chunks; the separator's bit 252 is 0 and opens chunk 168
    t.start = edh_identity(); B.add_chunks(t.start, pre.data(), pre.size()); t.start = edh_normalised(t.start);
    EdH g = B.random_base[0];
    for (int w = 0; w < SK_RND_WINDOWS; ++w) {
      EdH pw[4];
      for (int k = 0; k < 4; ++k) { pw[k] = g; edh_dbl(g); g = edh_normalised(g); }
      for (int v = 0; v < 16; ++v) {
        EdH e = edh_identity();
        for (int k = 0; k < 4; ++k) if ((v >> k) & 1) edh_add(e, pw[k], false, ed_d2());
        t.rnd.push_back(edh_normalised(e));
      }
    }
    // the device's copy
    WordTable wt(SK_WORDS, C);
    auto put = [&](uint32_t idx, const HFr& v) { wt.put(idx, v); };
    const auto& P = host::PoseidonParams<4, 2>::get();
    for (int i = 0; i < 3; ++i) put(SK_S0 + i, t.s0[i]);
    for (int r = 0; r < host::POSEIDON_ROUNDS; ++r) for (int i = 0; i < 3; ++i) put(SK_ARK + 3 * r + i, P.ark[r][i]);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) put(SK_MDS + 3 * i + j, P.mds[i][j]);
    put(SK_A, t.a); put(SK_B, t.b); put(SK_NEGA, t.neg_a); put(SK_A2, t.a2); put(SK_MB, t.mb); put(SK_TWO, HFr::from_u64(2));
    put(SK_START, t.start.X); put(SK_START + 1, t.start.Y); put(SK_START + 2, t.start.Z); put(SK_START + 3, t.start.T);
    uint64_t half[4]; std::memcpy(half, host::HParams<4>::P, 32);
    for (int i = 0; i < 4; ++i) half[i] = (half[i] >> 1) | (i + 1 < 4 ? half[i + 1] << 63 : 0);      // (r - 1) / 2: r is odd
    wt.put_plain(SK_HALF, half);
    for (int c = 0; c < SK_CHUNKS; ++c) for (int k = 0; k < 4; ++k) wt.put_cached(SK_CHUNK + 3 * (4 * c + k), B.lookup[4 * (SK_FIRST_CHUNK + c) + k]);
    for (size_t i = 0; i < t.rnd.size(); ++i) wt.put_cached(SK_RND + 3 * (uint32_t)i, t.rnd[i]);
    wt.put_exponent(SK_EXP_LEG, half);
    t.words = std::move(wt.words);
    return t;
  }();
  return T;
}

// the per-call key: false when sk_sig is not a canonical scalar below the subgroup order
static bool serial_key(ScanArgs& key, const void* sk_sig32) {
  uint64_t v[4]; std::memcpy(v, sk_sig32, 32);
  if (!scalar_below_order(v)) return false;
  std::memset(&key, 0, sizeof key);
  recode_scalar(key, v);
  return true;
}

// one commitment on the host: the flag (0 computed, 2 refused), and the canonical serial number (zeros with flag 2) into out32
static uint8_t serial_one_host(uint8_t* out32, const uint8_t* cm32, const ScanArgs& key, const SerialTables& T) {
  std::memset(out32, 0, 32);
  HFr cmc; std::memcpy(cmc.l, cm32, 32);
  if (HFr::geq_p(cmc.l)) return 2;
  // H = hash_to_group_psd2([D, cm])
  HFr st[3] = {T.s0[0], T.s0[1], T.s0[2]};
  st[2] = HFr::add(st[2], HFr::to_mont(cmc));
  host::poseidon_permute<4, 2>(st);
  EdH h, h1;
  if (!elligator2(h, st[1], T) || !elligator2(h1, st[2], T)) return 2;
  edh_add(h, h1, false, ed_d2()); edh_dbl(h); edh_dbl(h);
  // gamma = sk_sig H; the nonce = the low 250 bits of hash_psd2([D, x(4 gamma)])
  EdH gamma = edh_mul_naf(h, key);
  edh_dbl(gamma); edh_dbl(gamma);
  st[0] = T.s0[0]; st[1] = T.s0[1]; st[2] = HFr::add(T.s0[2], edh_affine(gamma).x);
  host::poseidon_permute<4, 2>(st);
  HFr nonce = HFr::from_mont(st[1]);
  nonce.l[3] &= (1ull << (SK_NONCE_BITS - 192)) - 1;
  // commit_bhp512((D, cm) bits, nonce)
  const Bhp& B = bhp512();
  uint8_t bits[3 * SK_CHUNKS];
  for (int i = 0; i < 3 * SK_CHUNKS; ++i) { const int j = 3 * SK_FIRST_CHUNK + i - SK_CM_AT; bits[i] = j >= 0 && j < 253 ? (cmc.l[j >> 6] >> (j & 63)) & 1 : 0; }
  EdH acc = T.start;
  B.add_chunks(acc, bits, sizeof bits, SK_FIRST_CHUNK);
  for (int w = 0; w < SK_RND_WINDOWS; ++w) { const unsigned v = (nonce.l[(4 * w) >> 6] >> ((4 * w) & 63)) & 15; if (v) edh_add(acc, T.rnd[16 * w + v], false, ed_d2()); }
  const HFr sn = HFr::from_mont(edh_affine(acc).x);
  std::memcpy(out32, sn.l, 32);
  return 0;
}

// the same from the definitions, without the tables: what the tables are checked against (tests/cpp/records_serial_lane_emul.cpp)
static uint8_t serial_one_plain(uint8_t* out32, const uint8_t* cm32, const ScanArgs& key, const SerialTables& T) {
  std::memset(out32, 0, 32);
  HFr cmc; std::memcpy(cmc.l, cm32, 32);
  if (HFr::geq_p(cmc.l)) return 2;
  const HFr in[2] = {T.dom, HFr::to_mont(cmc)}; HFr hh[2];
  host::poseidon_hash_many_fr<2>(in, 2, hh, 2);
  EdH e0, e1;
  if (!elligator2(e0, hh[0], T) || !elligator2(e1, hh[1], T)) return 2;
  edh_dbl(e0); edh_dbl(e0); edh_dbl(e1); edh_dbl(e1); edh_add(e0, e1, false, ed_d2());
  EdH gamma = edh_mul_naf(e0, key);
  edh_dbl(gamma); edh_dbl(gamma);
  const HFr in2[2] = {T.dom, edh_affine(gamma).x}; HFr nm;
  host::poseidon_hash_many_fr<2>(in2, 2, &nm, 1);
  HFr nonce = HFr::from_mont(nm);
  nonce.l[3] &= (1ull << (SK_NONCE_BITS - 192)) - 1;
  std::vector<uint8_t> bits;
  const HFr domc = HFr::from_mont(T.dom);
  push_field_bits(bits, domc.l); push_field_bits(bits, cmc.l);
  const HFr sn = HFr::from_mont(bhp512().commit(bits, nonce.l));
  std::memcpy(out32, sn.l, 32);
  return 0;
}

}}  // namespace aleo_mi355x::serial
