// signature_host.hpp — account signatures on the host: Signature<N>::sign / verify / sign_bytes / verify_bytes of snarkVM 0.14.5, console/account/src/signature
// [UPSTREAM-RECALL] — the reference's wasm/src/account/signature.rs:37-48, wasm/src/account/address.rs:69-71, wasm/src/account/private_key.rs:244-248 and
// sdk/src/account.ts:195,211-213.  Plain C++ (no HIP, touches no device) over serial_host.hpp (the curve, the account generator) and poseidon.hpp; the tables
// are a function-local static (thread-safe).  verify_one_host is the DEFINITION of a signature's flag; the device lane (signature_lane.h) returns the same.
//
//   sign     g_r = k G;  challenge = hash_to_scalar_psd8([g_r.x, pk_sig.x, pr_sig.x, address.x, m ...]);  response = k - challenge sk_sig  (mod l)
//   verify   g_r = response G + challenge pk_sig, the challenge again from the same preimage; sk_prf = hash_to_scalar_psd4([pk_sig.x, pr_sig.x]);
//            accepted iff the challenges are equal and x(pk_sig + pr_sig + sk_prf G) is the address
//   bytes    challenge | response | pk_sig.x | pr_sig.x, 32 bytes each, canonical little-endian
// Pinned by data the reference holds (tests/golden/reference_account.json: three accounts): the generator, hash_to_scalar's 250 bits, rate 4 for sk_prf, the
// sum that makes the address.  UNPINNED — the reference holds no signature, its own tests are round trips (wasm/src/account/signature.rs:98-115) —:
//   UNPINNED  the order of the challenge's preimage
//   UNPINNED  the packing of message bytes into fields: bits little-endian within a byte, 252 to a field, the last one short, none for no bytes
//   UNPINNED  the 128-byte layout
//   UNPINNED  the cap of SIG_MAX_FIELDS message fields
// A point from its x: of (x, +-y) the one in the prime-order subgroup, decided here from the definition, l P = O (the lane decides it with one exponentiation).
#pragma once
#include "serial_host.hpp"
#include "signature_lane.h"
#include "chacha.h"

namespace aleo_mi355x { namespace sig {

using host::HFr;
using serial::EdA;
using serial::ed_d2;
using serial::edh_affine;
using serial::edh_identity;
using serial::edh_is_identity;
using serial::edh_normalised;
using serial::edh_of;
using serial::scalar_below_order;

// ---- the scalar field: numbers below l as four words --------------------------------------------------------------------------------------------------------------
static inline bool geq_l(const uint64_t* v) { return !scalar_below_order(v); }
static inline void sub_l(uint64_t* v) { unsigned __int128 br = 0; for (int i = 0; i < 4; ++i) { const unsigned __int128 d = (unsigned __int128)v[i] - ED_ORDER[i] - (uint64_t)br; v[i] = (uint64_t)d; br = (d >> 64) & 1; } }
// a b mod l: the 512-bit product, reduced bit by bit from the top
static void scalar_mul(uint64_t* out4, const uint64_t* a, const uint64_t* b) {
  uint64_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) { unsigned __int128 cy = 0; for (int j = 0; j < 4; ++j) { cy += (unsigned __int128)a[i] * b[j] + p[i + j]; p[i + j] = (uint64_t)cy; cy >>= 64; } p[i + 4] = (uint64_t)cy; }
  uint64_t r[4] = {0, 0, 0, 0};
  for (int bit = 511; bit >= 0; --bit) {                     // r < l < 2^251, so 2 r + 1 fits
    for (int i = 3; i > 0; --i) r[i] = (r[i] << 1) | (r[i - 1] >> 63);
    r[0] = (r[0] << 1) | ((p[bit >> 6] >> (bit & 63)) & 1);
    if (geq_l(r)) sub_l(r);
  }
  std::memcpy(out4, r, 32);
}
// a - b mod l; a, b below l
static void scalar_sub(uint64_t* out4, const uint64_t* a, const uint64_t* b) {
  uint64_t r[4]; unsigned __int128 br = 0;
  for (int i = 0; i < 4; ++i) { const unsigned __int128 d = (unsigned __int128)a[i] - b[i] - (uint64_t)br; r[i] = (uint64_t)d; br = (d >> 64) & 1; }
  if (br) { unsigned __int128 cy = 0; for (int i = 0; i < 4; ++i) { cy += (unsigned __int128)r[i] + ED_ORDER[i]; r[i] = (uint64_t)cy; cy >>= 64; } }
  std::memcpy(out4, r, 32);
}

// ---- the tables ---------------------------------------------------------------------------------------------------------------------------------------------------
struct SigTables {
  std::vector<EdH> g;                                        // 63 x 16: v 2^(4 w) G (entry 0 the identity), Z = 1
  HFr s4[5];                                                 // the rate-4 sponge after [AleoPoseidon4, 2, 0, 0]
  std::vector<uint32_t> words;                               // records_lane.h RK_* and signature_lane.h SG_*
};

// k p for any point and any number of four words
static EdH edh_mul_words(const EdH& base, const uint64_t* k) {
  EdH p = edh_identity();
  for (int i = 255; i >= 0; --i) { edh_dbl(p); if ((k[i >> 6] >> (i & 63)) & 1) edh_add(p, base, false, ed_d2()); }
  return p;
}

static const SigTables& sig_tables() {
  static const SigTables T = [] {
    SigTables t;
    const RecordsConsts& C = records_consts();
    const HFr one = HFr::one();
    EdH g = edh_of(serial::account_generator());
    for (uint32_t w = 0; w < SIG_WINDOWS; ++w) {
      EdH pw[4];
      for (int k = 0; k < 4; ++k) { pw[k] = g; edh_dbl(g); g = edh_normalised(g); }
      for (int v = 0; v < 16; ++v) {
        EdH e = edh_identity();
        for (int k = 0; k < 4; ++k) if ((v >> k) & 1) edh_add(e, pw[k], false, ed_d2());
        t.g.push_back(edh_normalised(e));
      }
    }
    for (auto& v : t.s4) v = HFr::zero();
    t.s4[1] = host::fr_domain_separator("AleoPoseidon4"); t.s4[2] = HFr::from_u64(2);
    host::poseidon_permute<4, 4>(t.s4);
    // the tangent at T4 = (1, v4) of B v^2 = u^3 + A u^2 + u: B v4^2 = 2 + A, with A = 2 (a + d) / (a - d), B = 4 / (a - d), a = -1
    const HFr amd_inv = HFr::inv(HFr::neg(HFr::add(one, C.d)));
    const HFr ma = HFr::mul(HFr::dbl(HFr::sub(C.d, one)), amd_inv), mb = HFr::mul(HFr::from_u64(4), amd_inv);
    HFr v4; (void)hfr_sqrt(v4, HFr::mul(HFr::add(HFr::from_u64(2), ma), HFr::inv(mb)), C.sq);      // a square on this curve (the emulation checks the choice it leads to)
    uint64_t quart[4]; std::memcpy(quart, host::HParams<4>::P, 32);
    for (int i = 0; i < 4; ++i) quart[i] = (quart[i] >> 2) | (i + 1 < 4 ? quart[i + 1] << 62 : 0);      // (r - 1) / 4: r = 1 mod 4
    // kappa = psi(G), with w = 1 and s = y
    const EdA& G = serial::account_generator();
    const HFr nu = HFr::add(one, G.y), du = HFr::sub(one, G.y), dl = HFr::mul(G.x, du), xs = HFr::mul(G.x, G.y);
    const HFr nl = HFr::sub(nu, HFr::add(HFr::mul(dl, v4), HFr::mul(xs, HFr::dbl(v4))));
    const HFr arg = HFr::mul(HFr::mul(HFr::sqr(HFr::mul(nl, dl)), du), HFr::mul(HFr::sqr(nu), nu));
    const HFr kappa = HFr::pow(arg, quart, 4);
    // the device's copy
    WordTable wt(SG_WORDS, C);
    auto put = [&](uint32_t idx, const HFr& v) { wt.put(idx, v); };
    put(SG_TWO, HFr::from_u64(2)); put(SG_V4, v4); put(SG_V4X2, HFr::dbl(v4));
    const HFr kin = HFr::from_mont(kappa), kout = HFr::from_mont(HFr::neg(kappa));
    wt.put_plain(SG_KIN, kin.l); wt.put_plain(SG_KOUT, kout.l);
    put(SG_DOM8, host::fr_domain_separator("AleoPoseidon8"));
    const auto& P = host::PoseidonParams<4, 4>::get();
    for (int i = 0; i < 5; ++i) put(SG_S4 + i, t.s4[i]);
    for (int r = 0; r < host::POSEIDON_ROUNDS; ++r) for (int i = 0; i < 5; ++i) put(SG_ARK4 + 5 * r + i, P.ark[r][i]);
    for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) put(SG_MDS4 + 5 * i + j, P.mds[i][j]);
    for (size_t i = 0; i < t.g.size(); ++i) wt.put_cached(SG_G + 3 * (uint32_t)i, t.g[i]);
    wt.put_exponent(SG_EXP_QUART, quart);
    t.words = std::move(wt.words);
    return t;
  }();
  return T;
}

// p += k G for a number below 2^252
static void add_mul_g(EdH& p, const uint64_t* k, const SigTables& T) {
  for (uint32_t w = 0; w < SIG_WINDOWS; ++w) { const unsigned v = (k[(4 * w) >> 6] >> ((4 * w) & 63)) & 15; if (v) edh_add(p, T.g[16 * w + v], false, ed_d2()); }
}

// ---- points, messages, hashes ---------------------------------------------------------------------------------------------------------------------------------------
// The point of the prime-order subgroup with the canonical x-coordinate xc (below r); false: there is none
static bool point_from_x(EdH& out, const HFr& xc) {
  const RecordsConsts& C = records_consts();
  const HFr x = HFr::to_mont(xc), xx = HFr::sqr(x), one = HFr::one();
  const HFr w = HFr::sub(one, HFr::mul(C.d, xx)), u = HFr::add(one, xx);
  HFr s; if (w.is_zero() || !hfr_sqrt(s, HFr::mul(u, w), C.sq)) return false;
  EdH p; p.X = HFr::mul(x, w); p.Y = s; p.Z = w; p.T = HFr::mul(x, s);
  const EdH q = edh_mul_words(p, ED_ORDER);
  if (!q.X.is_zero()) return false;                          // of order 4 l or 4
  if (!(q.Y == q.Z)) { p.Y = HFr::neg(p.Y); p.T = HFr::neg(p.T); }      // l P = T2: (x, -y) = T2 - P is the one
  out = p; return true;
}

// the fields of a message, Montgomery form
static std::vector<HFr> message_fields(const uint8_t* msg, size_t len) {
  const size_t bits = 8 * len, m = (bits + SIG_FIELD_BITS - 1) / SIG_FIELD_BITS;
  std::vector<HFr> out(m);
  for (size_t j = 0; j < m; ++j) {
    HFr v = HFr::zero();
    for (size_t b = 0; b < SIG_FIELD_BITS && SIG_FIELD_BITS * j + b < bits; ++b) {
      const size_t src = SIG_FIELD_BITS * j + b;
      v.l[b >> 6] |= (uint64_t)((msg[src >> 3] >> (src & 7)) & 1) << (b & 63);
    }
    out[j] = HFr::to_mont(v);
  }
  return out;
}

template <int RATE> static void hash_to_scalar(uint64_t* out4, const HFr* in, size_t n) {      // the low 250 bits of the hash
  HFr h; host::poseidon_hash_many_fr<RATE>(in, n, &h, 1);
  h = HFr::from_mont(h); h.l[3] &= (1ull << (SIG_SCALAR_BITS - 192)) - 1;
  std::memcpy(out4, h.l, 32);
}
// the challenge of (g_r.x, pk_sig.x, pr_sig.x, address.x: Montgomery form) and a message
static void challenge_of(uint64_t* out4, const HFr& grx, const HFr& pkx, const HFr& prx, const HFr& ax, const uint8_t* msg, size_t len) {
  std::vector<HFr> pre = {grx, pkx, prx, ax};
  const std::vector<HFr> m = message_fields(msg, len);
  pre.insert(pre.end(), m.begin(), m.end());
  hash_to_scalar<8>(out4, pre.data(), pre.size());
}

// ---- verify and sign ------------------------------------------------------------------------------------------------------------------------------------------------
static uint8_t verify_one_host(const uint8_t* sig128, const uint8_t* address_x32, const uint8_t* msg, size_t len) {
  uint64_t ch[4], rs[4]; HFr pkx, prx, ax;
  std::memcpy(ch, sig128, 32); std::memcpy(rs, sig128 + 32, 32); std::memcpy(pkx.l, sig128 + 64, 32); std::memcpy(prx.l, sig128 + 96, 32); std::memcpy(ax.l, address_x32, 32);
  if (geq_l(ch) || geq_l(rs) || HFr::geq_p(pkx.l) || HFr::geq_p(prx.l) || HFr::geq_p(ax.l) || len > SIG_MAX_BYTES) return (uint8_t)SIG_MALFORMED;
  EdH pk, pr;
  if (!point_from_x(pk, pkx) || !point_from_x(pr, prx)) return (uint8_t)SIG_MALFORMED;
  const SigTables& T = sig_tables();
  EdH gr = edh_mul_words(pk, ch);
  add_mul_g(gr, rs, T);
  const HFr pkm = HFr::to_mont(pkx), prm = HFr::to_mont(prx), am = HFr::to_mont(ax);
  uint64_t again[4], prf[4];
  challenge_of(again, edh_affine(gr).x, pkm, prm, am, msg, len);
  const HFr in[2] = {pkm, prm};
  hash_to_scalar<4>(prf, in, 2);
  EdH a = pk; edh_add(a, pr, false, ed_d2()); add_mul_g(a, prf, T);
  const bool ok = std::memcmp(again, ch, 32) == 0 && edh_affine(a).x == am;
  return (uint8_t)(ok ? SIG_OK : SIG_INVALID);
}

// what signing needs of an account: sk_sig, and the x-coordinates (canonical bytes) of pk_sig = sk_sig G, pr_sig = r_sig G and the address
struct SignerKeys { uint64_t sk_sig[4]; uint8_t pk_x[32], pr_x[32], address_x[32]; };
static void x_of_mul_g(uint8_t* out32, const uint64_t* k) { EdH p = edh_identity(); add_mul_g(p, k, sig_tables()); const HFr c = HFr::from_mont(edh_affine(p).x); std::memcpy(out32, c.l, 32); }

// the signature of a message under a nonce below l
static void sign_with_nonce(uint8_t* out128, const SignerKeys& a, const uint64_t* nonce, const uint8_t* msg, size_t len) {
  uint8_t grx[32]; x_of_mul_g(grx, nonce);
  auto mont = [](const uint8_t* p) { HFr v; std::memcpy(v.l, p, 32); return HFr::to_mont(v); };
  uint64_t ch[4], t[4], rs[4];
  challenge_of(ch, mont(grx), mont(a.pk_x), mont(a.pr_x), mont(a.address_x), msg, len);
  scalar_mul(t, ch, a.sk_sig); scalar_sub(rs, nonce, t);
  std::memcpy(out128, ch, 32); std::memcpy(out128 + 32, rs, 32); std::memcpy(out128 + 64, a.pk_x, 32); std::memcpy(out128 + 96, a.pr_x, 32);
}
// The nonce of a seed: signature_lane.h sg_nonce_of_seed, the one definition the signing lane runs too
static void nonce_of_seed(uint64_t* out4, const uint8_t* seed32) {
  uint32_t key[8], w[8]; std::memcpy(key, seed32, 32);
  sg_nonce_of_seed(w, key);
  std::memcpy(out4, w, 32);
}

}}  // namespace aleo_mi355x::sig
