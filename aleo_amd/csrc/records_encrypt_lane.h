// records_encrypt_lane.h — what ONE lane of the two record-encryption kernels computes (records_encrypt.hip launches them, one RecordPlaintext string per lane): the
// "record1…" string of Record<N, Plaintext<N>>::encrypt(randomizer), byte for byte record_encrypt_host.hpp's encrypt_one_host, which is the definition.
//
// The lane COMPUTES OR ROUTES, as plaintexts_lane.h's does and for the same strings: it computes a record of at most PT_MAX_CHARS characters and PT_MAX_ENTRIES
// entries whose entries are numeric, boolean or address literals in render's spelling, in any visibility; everything else is RE_ROUTED (which never leaves the
// library), and the calling thread encrypts or refuses that row with the host code.
//
// Two lanes, because the two together do not fit one: the point arithmetic (two points, a cached one, the scalar, the square root's temporaries) takes 173 vector
// registers and the text walk — the sponge's nine elements through a permutation, a parsed field, the writer — all 256 and 136 more by itself.  So the plain fields
// never live across the point arithmetic: they do not exist before the second lane.
//   records_encrypt_keys_lane   the measure walk (plaintexts_lane.h pt_measure, with a visitor): the owner, the nonce the string says, the payload's bytes, the
//                               number of private fields.  r G from the resident table (sg_add_mul_g) and one inversion: the nonce, compared (mode 0) or kept
//                               (mode 1).  The owner's point from its x with the subgroup decided (sg_point_from_x), r Owner by the signature lane's double-and-add
//                               — scalar and point are the lane's own, the sum is always computed and selected — over the 251 bits of r, one more inversion: rvk.
//                               A routed or refused lane goes through all of it on zeros.
//   records_encrypt_text_lane   the second walk, field by field through the same pt_field: the payload's bytes in order — a private field is built from the
//                               literal's bits (00 | u8 type | u16 size | value | terminus 1, 252 to a field: one field, or two for a value over 225 bits), added to
//                               the next of the sponge's randomizers (a permutation every eight) and made canonical — each byte through a 5-bit symbol writer with a
//                               running polymod, then the padding symbol and the six checksum symbols.  Nothing is buffered: a character goes where put() says.
//                               Lanes of a wave permute when their own count of fields passes a multiple of eight; records of one shape stay in step.
// Plain C++: no thread index, characters come through a callable and leave through one, so tests/cpp/records_encrypt_lane_emul.cpp runs both on the host.
#pragma once
#include "plaintexts_lane.h"
#include "signature_lane.h"

namespace aleo_mi355x {

static constexpr uint32_t RE_OK = 0, RE_NONCE_MISMATCH = 1, RE_BAD_KEY = 2, RE_NOT_A_RECORD = 3, RE_ROUTED = 8;
static constexpr uint32_t RE_SCALAR_BITS = 251;                                       // l has 251 bits
static constexpr uint32_t RE_PLAIN_HEADER_BITS = 26, RE_FIELD_BITS = 252;             // 00 | u8 type | u16 size; the data bits of a field

// What the first walk leaves: info = entries | private fields << 8 | (owner private) << 16, the words of the owner's x and of the nonce the string says, the
// characters of the record1… string
struct ReMeasure { uint32_t info, chars, owner[8], nonce[8]; };
__host__ __device__ __forceinline__ uint32_t re_private_fields(uint32_t type) { return RE_PLAIN_HEADER_BITS + pt_literal_bits(type) + 1u > RE_FIELD_BITS ? 2u : 1u; }
__host__ __device__ __forceinline__ uint32_t re_chars_of(uint32_t payload_bytes) { return RS_PREFIX_CHARS + (8u * payload_bytes + 4u) / 5u + RS_CHECKSUM_SYMBOLS; }

template <class Ch>
__host__ __device__ __forceinline__ bool re_measure(Ch&& c, uint32_t len, ReMeasure& R) {
  PtMeasure M;
  uint32_t bytes = 1u + 32u + 1u + 32u, m = 0, owner_private = 0;      // owner variant and x, the entry count, the nonce
#pragma unroll
  for (int q = 0; q < 8; ++q) R.owner[q] = R.nonce[q] = 0;
  const bool ok = pt_measure(c, len, M, [&](const PtField& F, uint32_t which) {
    if (which == PT_OWNER) {
      owner_private = F.vis == 2 ? 1u : 0u;
      bytes += 2u * owner_private; m += owner_private;                 // u16 field count
#pragma unroll
      for (int q = 0; q < 8; ++q) R.owner[q] = F.v[q];
    } else if (which == PT_NONCE) {
#pragma unroll
      for (int q = 0; q < 8; ++q) R.nonce[q] = F.v[q];
    } else {
      const uint32_t nf = re_private_fields(F.type);
      bytes += 1u + F.name_len + 2u + (F.vis == 2 ? 3u + 32u * nf : 4u + (pt_literal_bits(F.type) + 7u) / 8u);
      if (F.vis == 2) m += nf;
    }
  });
  R.info = M.entries | (m << 8) | (owner_private << 16);
  R.chars = re_chars_of(bytes);
  return ok;
}

// ---- the keys ------------------------------------------------------------------------------------------------------------------------------------------------------
// One string and its randomizer rw (canonical words as they came).  Returns the flag — RE_OK, RE_NONCE_MISMATCH, RE_BAD_KEY or RE_ROUTED — with R (info and chars;
// chars 0 with a flag), the nonce to write and the record view key's x as canonical words (zeros with a flag).  phase(): signature_lane.h's, between the phases.
template <class Ch, class Phase>
__device__ __forceinline__ uint32_t records_encrypt_keys_lane(Ch&& c, uint32_t len, const uint32_t (&rw)[8], uint32_t mode, const uint32_t* K, ReMeasure& R, uint32_t (&nonce)[8],
                                                              uint32_t (&rvk)[8], Phase&& phase) {
  const bool routed = !re_measure(c, len, R);
  uint32_t bad = routed || !sg_below_order(rw);                   // a word of the lane's own (sg_point_from_x)
  const F29 one = rk_const(K, RK_ONE);
  // r G, and its x
  Ed29 p; p.X = f29_zero(); p.Y = one; p.Z = one; p.T = p.X;
  {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = bad ? 0u : rw[i];
    phase();
    sg_add_mul_g(p, k, K);
  }
  phase();
  f29_to_words(f29_canonical(f29_mul(p.X, f29_pow(p.Z, K + RK_EXP_INV, RK_INV_BITS))), nonce);      // Z is never 0 (the law is complete)
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= nonce[i] ^ R.nonce[i];
  const bool mismatch = mode == 0 && diff != 0;
  // r Owner, and its x
  phase();
  p = sg_point_from_x(f29_zero_if(bad != 0, f29_from_words(R.owner)), bad, K);
  phase();
  {
    const Ed29Cached owner = ed29_cache(p, rk_const(K, RK_D2));
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = bad ? 0u : rw[i];
#pragma unroll
    for (int i = 7; i > 0; --i) k[i] = (k[i] << 5) | (k[i - 1] >> 27);            // bit 250 to the top
    k[0] <<= 5;
    p.X = f29_zero(); p.Y = one; p.Z = one; p.T = p.X;
    for (uint32_t i = 0; i < RE_SCALAR_BITS; ++i) {
      const bool bit = k[7] >> 31;
#pragma unroll
      for (int q = 7; q > 0; --q) k[q] = (k[q] << 1) | (k[q - 1] >> 31);
      k[0] <<= 1;
      ed29_dbl(p, true);
      Ed29 t = p;
      ed29_add(t, owner, false);
      p.X = f29_select(bit, t.X, p.X); p.Y = f29_select(bit, t.Y, p.Y); p.Z = f29_select(bit, t.Z, p.Z); p.T = f29_select(bit, t.T, p.T);
    }
  }
  phase();
  f29_to_words(f29_canonical(f29_mul(p.X, f29_pow(p.Z, K + RK_EXP_INV, RK_INV_BITS))), rvk);
  const uint32_t flag = routed ? RE_ROUTED : (bad ? RE_BAD_KEY : (mismatch ? RE_NONCE_MISMATCH : RE_OK));
#pragma unroll
  for (int i = 0; i < 8; ++i) { rvk[i] = flag ? 0u : rvk[i]; nonce[i] = flag ? 0u : nonce[i]; }
  if (flag) R.chars = 0;
  return flag;
}

// ---- the text ------------------------------------------------------------------------------------------------------------------------------------------------------
// The symbol writer: bytes in, characters out, the checksum kept on the way
struct ReWriter { uint32_t acc = 0, nbits = 0, chk = RS_PREFIX_STATE; };
__host__ __device__ __forceinline__ uint32_t re_char_of(uint32_t symbol) {
  const char alphabet[33] = "qpzry9x8gf2tvdw0s3jn54khce6mua7l";
  return (uint32_t)(uint8_t)alphabet[symbol & 31u];
}
template <class Put> __host__ __device__ __forceinline__ void re_byte(ReWriter& Wr, uint32_t b, Put&& put) {
  Wr.acc = (Wr.acc << 8) | (b & 0xffu); Wr.nbits += 8;
  while (Wr.nbits >= 5) {
    Wr.nbits -= 5;
    const uint32_t s = (Wr.acc >> Wr.nbits) & 31u;
    Wr.chk = rs_polymod_step(Wr.chk, s);
    put(re_char_of(s));
  }
  Wr.acc &= (1u << Wr.nbits) - 1u;
}
// the low n bytes of NW words, least significant first; the words are used up (they move down: no lane indexes its registers)
template <int NW, class Put> __host__ __device__ __forceinline__ void re_push(ReWriter& Wr, uint32_t (&w)[NW], uint32_t n, Put&& put) {
#pragma unroll 1
  for (uint32_t i = 0; i < n; ++i) {
    re_byte(Wr, w[0], put);
#pragma unroll
    for (int q = 0; q + 1 < NW; ++q) w[q] = (w[q] >> 8) | (w[q + 1] << 24);
    w[NW - 1] >>= 8;
  }
}
template <class Put> __host__ __device__ __forceinline__ void re_finish(ReWriter& Wr, Put&& put) {
  if (Wr.nbits) { const uint32_t s = (Wr.acc << (5u - Wr.nbits)) & 31u; Wr.chk = rs_polymod_step(Wr.chk, s); put(re_char_of(s)); }
  uint32_t chk = Wr.chk;
  for (int i = 0; i < 6; ++i) chk = rs_polymod_step(chk, 0);
  chk ^= RS_BECH32M;
  for (int i = 0; i < 6; ++i) put(re_char_of(chk >> (5 * (5 - i))));
}

// One string that records_encrypt_keys_lane computed (flag RE_OK): info as it left it, the nonce to write and the record view key's x (canonical words).  put(ch):
// the characters behind "record1", in order — re_chars_of(..) - RS_PREFIX_CHARS of them.
template <class Ch, class Put>
__device__ __forceinline__ void records_encrypt_text_lane(Ch&& c, uint32_t info, const uint32_t (&nonce)[8], const uint32_t (&rvk)[8], const uint32_t* K, Put&& put) {
  const uint32_t entries = info & 0xffu;
  const F29 r2 = rk_const(K, RK_R2);
  F29 st[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) st[i] = rk_const(K, RK_S0 + i);
  st[2] = f29_add(st[2], f29_mul(f29_from_words(rvk), r2));
  ReWriter Wr;
  uint32_t at = 0, used = 0;
  (void)pt_punct(c, at, '{');
  for (uint32_t k = 0; k <= entries + 1u; ++k) {
    PtField F;
    (void)pt_field(c, at, F);                                    // the owner, an entry or the nonce
    if (k <= entries) (void)pt_punct(c, at, ',');
    const bool is_owner = k == 0, is_nonce = k == entries + 1u, is_private = F.vis == 2;
    const uint32_t bits = pt_literal_bits(F.type), nf = re_private_fields(F.type), plain_bytes = is_owner || is_nonce ? 32u : (bits + 7u) / 8u;
    // the bytes before the name: the owner's variant (and its count of one field); the entry count before the first field behind the owner; an entry's name length
    {
      uint32_t head[1] = {is_owner ? (is_private ? 0x000101u : 0u) : (k == 1 ? entries : 0u)}, n = is_owner ? (is_private ? 3u : 1u) : (k == 1 ? 1u : 0u);
      if (!is_owner && !is_nonce) { head[0] |= F.name_len << (8u * n); ++n; }
      re_push<1>(Wr, head, n, put);
    }
    if (!is_owner && !is_nonce) {
      for (uint32_t i = 0; i < F.name_len; ++i) re_byte(Wr, c(F.name_at + i), put);
      // u16 body length, then private: 02 | u16 fields;  constant, public: the visibility | 00 | u16 type
      const uint32_t body = is_private ? 3u + 32u * nf : 4u + plain_bytes;
      uint32_t mid[2] = {body | (is_private ? 0x02u << 16 | nf << 24 : F.vis << 16), is_private ? 0u : F.type};
      re_push<2>(Wr, mid, is_private ? 5u : 6u, put);
    }
    // the value: one chunk as it stands (a public owner, a constant or public value, the nonce), or the private fields
    uint32_t f0[8], f1 = 0;
    if (is_nonce) {
#pragma unroll
      for (int q = 0; q < 8; ++q) f0[q] = nonce[q];
    } else if (is_owner || !is_private) {
#pragma unroll
      for (int q = 0; q < 8; ++q) f0[q] = F.v[q];
    } else {                                                     // 00 | u8 type | u16 size | value | 1: at most 280 bits, as nine words
      uint32_t s[9];
      s[0] = (F.type << 2) | (bits << 10) | (F.v[0] << RE_PLAIN_HEADER_BITS);
#pragma unroll
      for (int q = 1; q < 8; ++q) s[q] = (F.v[q - 1] >> (32u - RE_PLAIN_HEADER_BITS)) | (F.v[q] << RE_PLAIN_HEADER_BITS);
      s[8] = F.v[7] >> (32u - RE_PLAIN_HEADER_BITS);
      const uint32_t terminus = RE_PLAIN_HEADER_BITS + bits;
#pragma unroll
      for (uint32_t q = 0; q < 9; ++q) s[q] |= q == (terminus >> 5) ? 1u << (terminus & 31u) : 0u;
#pragma unroll
      for (int q = 0; q < 8; ++q) f0[q] = s[q];
      f1 = (s[7] >> 28) | (s[8] << 4);                           // bits 252 .. 279
      f0[7] &= 0x0fffffffu;
    }
    const bool encrypted = is_private && !is_nonce;
    const uint32_t chunks = encrypted && !is_owner ? nf : 1u;
    for (uint32_t t = 0; t < chunks; ++t) {
      uint32_t w[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) w[q] = t ? (q == 0 ? f1 : 0u) : f0[q];
      if (encrypted) {
        const uint32_t j = used & 7u;
        if (j == 0) psd_permute(st, K);                          // every element tidied: a summand below and of the next permutation's first round
        F29 rnd = st[1];
#pragma unroll
        for (uint32_t q = 1; q < 8; ++q) rnd = f29_select(j == q, st[1 + q], rnd);
        f29_to_words(f29_canonical(f29_add(f29_mul(f29_from_words(w), r2), rnd)), w);
        ++used;
      }
      re_push<8>(Wr, w, encrypted ? 32u : plain_bytes, put);
    }
  }
  re_finish(Wr, put);
}

}  // namespace aleo_mi355x
