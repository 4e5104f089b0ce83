// records_commit_lane.h — what ONE lane of the commitment kernel computes (records_commit.hip launches it, one owned record per lane): the commitment of a
// decrypted record, Record<N, Plaintext<N>>::to_commitment(program_id, record_name) of snarkVM 0.14.5 [UPSTREAM-RECALL; pinned by the "id" of the record output
// in the reference's transaction: tests/golden/reference_serial.json] — what the wasm SDK's findUnspentRecords derives from the plaintext before it asks for the
// serial number (wasm/src/record/record_plaintext.rs:64-82).  Byte for byte serial::record_bits + bhp1024().hash (records_bits.hpp, serial_host.hpp):
//
//   message   program name | "aleo" | record name | is-private bit, 253 owner bits | u32 data bits | data | 253 bits of the nonce x
//   data      per entry: the name's bytes | 2 visibility bits | a private entry's PLAINTEXT BITS: the 252 data bits of each of its plain fields, the
//             trailing zeros and the terminus bit dropped (plaintext::fields_to_bits)
//   BHP1024   Bhp(8, 54): 432 chunks of 3 bits per iteration.  Iteration 0 hashes 188 domain bits | the 64-bit message length | 1044 message bits, every later
//             one the 252 low bits of the previous digest's affine x | the next 1044 message bits: 252 = 84 chunks and 1044 = 348, so message chunk k is
//             chunk 84 + k mod 348 of iteration k / 348, whatever the length, and an extra iteration costs one inversion.
//
// Two walks over the entries, as the u32 length precedes the data: commit_measure sums the lengths and refuses, commit_next hands out the message in order as
// items of at most 256 bits, which commit_hash feeds straight into 3-bit chunks — there is no bit buffer.  ONE place adds a chunk's table entry, so the
// eight products of an addition are in the code once (and once more where an iteration's digest is fed back): commit_hash takes its items from a source
// next(w, nbits), which is commit_next here and the walk over a plaintext string in plaintexts_lane.h.
// The start.  The domain (chunks 0 .. 61), the zero chunks 74 .. 83 of the length's upper bits and the whole chunks of the three names (from chunk 84 on) are
// the same for every record of a call: the host sums them (commit_host.hpp commit_args; 110 chunks for credits.aleo / credits) and passes the point and the
// names' leftover 0-2 bits by value.  The lane adds chunks 62 .. 73 — the domain's last two bits and the length's low 34 — and goes on behind the names.
// The table.  432 x 4 cached affine entries (k base_c, k = 1 .. 4: y - x, y + x, 2 d x y; 108 B each, 187 KB) behind the scan's constants (records_lane.h RK_*),
// resident per device.  At step c the lanes of a wave that are in step read one of the four entries of the same chunk: 432 B, served by L2.
// A record with a constant or public entry is not walked: its conversion (records_bits.hpp bytes_to_bits) is recursive and unpinned.  The lane reports it
// (COMMIT_ROUTED) and the calling thread computes its row with the host code.
// Flags: 0 computed; 4 refused where aleo_mi355x_record_commitment refuses — a private entry without a terminus bit or of no fields (and, on the host, a
// constant or public entry that does not parse) — with a row of zeros.
// The walk (commit_measure, commit_next) is plain C++; the hashing uses the device field (edwards29.h), which tests/cpp/records_commit_lane_emul.cpp supplies
// on the host with every limb rule checked.
#pragma once
#include "records_serial_lane.h"
#include "records_found_lane.h"

namespace aleo_mi355x {

static constexpr uint32_t COMMIT_OK = 0, COMMIT_REFUSED = 4, COMMIT_ROUTED = 8;      // ROUTED never leaves the library
static constexpr uint32_t CM_CHUNKS = 432, CM_PREFIX_CHUNKS = 84, CM_DOMAIN_CHUNKS = 62, CM_LENGTH_CHUNKS = 12, CM_DATA_BITS = 252, CM_NAMES_MAX = 31 + 4 + 31;

// The lane's constants: the scan's first, unchanged (K serves rk_const and f29_pow as it stands), then in units of one element
enum : uint32_t {
  CK_E0 = (RK_WORDS + 8) / 9,
  CK_TWO = CK_E0,                          // 2: the 2 Z of every table entry
  CK_TABLE = CK_TWO + 1,                   // 432 x 4 x 3
  CK_ELEMS = CK_TABLE + CM_CHUNKS * 4 * 3,
  CK_WORDS = CK_ELEMS * 9
};

// What is the same for every record of a call.  start: X, Y, T (Z = 1) of the pre-summed chunks, Montgomery limbs; first_chunk: where the stream goes on behind
// the length (84 + name_bits / 3); lead: the names' name_bits mod 3 last bits; head: bits 186 and 187 of the prefix (the domain's last two).
struct CommitArgs { uint32_t start[27], first_chunk, lead, lead_n, name_bits, head; };

// ---- the walks (plain C++) ---------------------------------------------------------------------------------------------------------------------------------
// The number of PLAINTEXT BITS of a private entry of nf fields (field i through load(i, w)): the position of the last set bit among the 252 data bits of its
// fields; false: there is none.
template <class LoadField>
__host__ __device__ __forceinline__ bool commit_value_bits(uint32_t nf, LoadField&& load, uint32_t& bits) {
  uint32_t w[8];
  for (uint32_t i = nf; i-- > 0;) {
    load(i, w);
    w[7] &= 0x0fffffffu;
#pragma unroll
    for (int q = 7; q >= 0; --q)
      if (w[q]) { bits = CM_DATA_BITS * i + 32u * (uint32_t)q + (31u - (uint32_t)__builtin_clz(w[q])); return true; }
  }
  return false;
}

// The first walk.  sym(k): symbol k of the string, which has passed records_parse_lane and records_found_walk (status 0) — the tests of the latter are repeated, so
// that no other string can lead the second walk astray; n_fields: the record's decrypted fields, field k through load(k, w).  data_bits: what the u32 says.
template <class Sym, class LoadField>
__host__ __device__ __forceinline__ uint32_t commit_measure(Sym&& sym, int32_t kind, uint32_t n_fields, LoadField&& load, uint32_t& data_bits) {
  auto byte_at = [&](uint32_t j) { return rs_byte_at(sym, j); };
  uint32_t at = (kind == 1 ? 3u : 1u) + 32u, field = kind == 1 ? 1u : 0u, bits = 0;
  const uint32_t entries = byte_at(at++);
  data_bits = 0;
  for (uint32_t e = 0; e < entries; ++e) {
    const uint32_t nl = byte_at(at++);
    if (!nl) return COMMIT_REFUSED;
    at += nl;
    const uint32_t el = byte_at(at) | (byte_at(at + 1) << 8); at += 2;
    if (el < 1) return COMMIT_REFUSED;
    const uint32_t vis = byte_at(at);
    if (vis > 2) return COMMIT_REFUSED;
    if (vis != 2) return COMMIT_ROUTED;
    if (el < 3) return COMMIT_REFUSED;
    const uint32_t nf = byte_at(at + 1) | (byte_at(at + 2) << 8);
    if (el != 3u + 32u * nf || field + nf > n_fields) return COMMIT_REFUSED;
    uint32_t value;
    if (!commit_value_bits(nf, [&](uint32_t i, uint32_t (&w)[8]) { load(field + i, w); }, value)) return COMMIT_REFUSED;
    bits += 8u * nl + 2u + value;
    field += nf; at += el;
  }
  if (field != n_fields) return COMMIT_REFUSED;                // cannot happen: the found walk counted them
  data_bits = bits;
  return COMMIT_OK;
}

// The second walk: the message behind the names, item by item.
struct CommitWalk { uint32_t stage, at, next_at, e, entries, field, nf, i, name_left, value_bits; };
static constexpr uint32_t CW_OWNER = 0, CW_LENGTH = 1, CW_ENTRY = 2, CW_NAME = 3, CW_VIS = 4, CW_FIELD = 5, CW_NONCE = 6, CW_DONE = 7;

// The next item of a record commit_measure accepted: its bits in w, little-endian (what lies above `nbits` is anything); false: the message has ended.
template <class Sym, class LoadField>
__host__ __device__ __forceinline__ bool commit_next(CommitWalk& W, Sym&& sym, int32_t kind, LoadField&& load, uint32_t data_bits, uint32_t (&w)[8], uint32_t& nbits) {
  auto byte_at = [&](uint32_t j) { return rs_byte_at(sym, j); };
  for (;;) {
    if (W.stage == CW_OWNER) {                                 // 1 | the decrypted field of a private owner, the payload's of a public one
      uint32_t f[8];
      if (kind == 1) load(0, f); else rs_field_at(sym, 1, f);
      w[0] = (kind == 1 ? 1u : 0u) | (f[0] << 1);
#pragma unroll
      for (int q = 1; q < 8; ++q) w[q] = (f[q - 1] >> 31) | (f[q] << 1);
      nbits = 254;
      W.at = (kind == 1 ? 3u : 1u) + 32u; W.entries = byte_at(W.at++); W.e = 0; W.field = kind == 1 ? 1u : 0u;
      W.stage = CW_LENGTH; return true;
    }
    if (W.stage == CW_LENGTH) { w[0] = data_bits; nbits = 32; W.stage = CW_ENTRY; return true; }
    if (W.stage == CW_ENTRY) {
      if (W.e == W.entries) { W.stage = CW_NONCE; continue; }
      W.name_left = byte_at(W.at++); W.stage = CW_NAME;
    }
    if (W.stage == CW_NAME) {                                  // at most 32 bytes of the name
      const uint32_t cnt = W.name_left < 32u ? W.name_left : 32u;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) if (4u * (uint32_t)q + b < cnt) v |= byte_at(W.at + 4u * (uint32_t)q + b) << (8 * b);
        w[q] = v;
      }
      nbits = 8 * cnt; W.at += cnt; W.name_left -= cnt;
      if (!W.name_left) W.stage = CW_VIS;
      return true;
    }
    if (W.stage == CW_VIS) {                                   // private: the bits 1, 0.  Then the entry's fields
      const uint32_t el = byte_at(W.at) | (byte_at(W.at + 1) << 8); W.at += 2;
      W.nf = byte_at(W.at + 1) | (byte_at(W.at + 2) << 8); W.next_at = W.at + el; W.i = 0; W.value_bits = 0;
      const uint32_t first = W.field;
      (void)commit_value_bits(W.nf, [&](uint32_t i, uint32_t (&v)[8]) { load(first + i, v); }, W.value_bits);
      w[0] = 1; nbits = 2; W.stage = CW_FIELD; return true;
    }
    if (W.stage == CW_FIELD) {
      if (CM_DATA_BITS * W.i >= W.value_bits) { W.field += W.nf; W.at = W.next_at; ++W.e; W.stage = CW_ENTRY; continue; }
      const uint32_t left = W.value_bits - CM_DATA_BITS * W.i;
      load(W.field + W.i, w); nbits = left < CM_DATA_BITS ? left : CM_DATA_BITS; ++W.i;
      return true;
    }
    if (W.stage == CW_NONCE) { rs_field_at(sym, W.at, w); nbits = 253; W.stage = CW_DONE; return true; }
    return false;
  }
}

// ---- the hash -------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Ed29Cached ck_entry(const uint32_t* __restrict__ K, uint32_t chunk, uint32_t k) {
  const uint32_t first = CK_TABLE + 3u * (4u * chunk + k);
  Ed29Cached c; c.ym = rk_const(K, first); c.yp = rk_const(K, first + 1); c.k = rk_const(K, first + 2); c.z2 = rk_const(K, CK_TWO);
  return c;
}

// The hash of a message of `message_bits` bits behind the call's names, whose items next(w, nbits) hands out in order (each at most 256 bits, little-endian in w,
// anything above nbits; false: the message has ended): the start point, chunks 62 .. 73, the 3-bit chunks, the feed-back of an iteration's digest.  Returns the
// canonical limbs of the digest's x.  The two item sources are commit_next above (a record string and its decrypted fields) and plaintexts_lane.h's (a plaintext string).
template <class Next>
__device__ __forceinline__ F29 commit_hash(Next&& next, uint32_t message_bits, const uint32_t* __restrict__ K, const CommitArgs& A) {
  Ed29 p;
  p.X = f29_limbs(A.start); p.Y = f29_limbs(A.start + 9); p.T = f29_limbs(A.start + 18);
  p.Z = rk_const(K, RK_ONE);
  uint32_t c = CM_DOMAIN_CHUNKS, nb = 0;                       // the chunk to come; the bits waiting for a whole one
  uint64_t acc = 0;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nbits;
  bool head = true, more = true;
  while (more) {
    if (head) { w[0] = A.head | (message_bits << 2); w[1] = message_bits >> 30; nbits = 3 * CM_LENGTH_CHUNKS; }      // chunks 62 .. 73
    else {
      more = next(w, nbits);
      if (!more) { w[0] = 0; nbits = nb ? 3u - nb : 0u; }      // the last chunk's padding
    }
    for (uint32_t left = nbits; left;) {                       // word by word from the bottom of w, which moves down: no lane indexes its registers
      const uint32_t n = left < 32u ? left : 32u, v = w[0];
#pragma unroll
      for (int q = 0; q < 7; ++q) w[q] = w[q + 1];
      left -= n;
      acc |= (uint64_t)(n < 32u ? v & ((1u << n) - 1u) : v) << nb; nb += n;
      while (nb >= 3) {
        if (c == CM_CHUNKS) {                                  // the next iteration opens with the 252 low bits of this digest's x
          const F29 x = f29_canonical(f29_mul(p.X, f29_pow(p.Z, K + RK_EXP_INV, RK_INV_BITS)));      // Z is never 0 (the law is complete)
          p.X = f29_zero(); p.Y = rk_const(K, RK_ONE); p.Z = p.Y; p.T = p.X;
          for (c = 0; c < CM_PREFIX_CHUNKS; ++c)
            ed29_add(p, ck_entry(K, c, (uint32_t)f29_bit(x, 3 * c) | (uint32_t)f29_bit(x, 3 * c + 1) << 1), f29_bit(x, 3 * c + 2));
        }
        ed29_add(p, ck_entry(K, c, (uint32_t)acc & 3u), ((uint32_t)acc & 4u) != 0);
        ++c; acc >>= 3; nb -= 3;
      }
    }
    if (head) { head = false; c = A.first_chunk; acc = A.lead; nb = A.lead_n; }      // behind the names
  }
  return f29_canonical(f29_mul(p.X, f29_pow(p.Z, K + RK_EXP_INV, RK_INV_BITS)));
}

// One owned record whose found status is 0.  ch(i): character i of its string, of `len`; kind: its owner variant; load(k, w): its decrypted field k of n_fields,
// canonical little-endian words, randomizer order.  Returns the flag; `emit` is handed the canonical limbs of the commitment when the flag is 0.
template <class LoadChar, class LoadField, class Emit>
__device__ __forceinline__ uint32_t records_commit_lane(LoadChar&& ch, uint32_t len, int32_t kind, uint32_t n_fields, LoadField&& load, const uint32_t* __restrict__ K,
                                                        const CommitArgs& A, Emit&& emit) {
  constexpr RsSymbols T = rs_symbols();
  auto sym = [&](uint32_t k) { return RS_PREFIX_CHARS + k < len ? (uint32_t)T.of[(uint8_t)ch(RS_PREFIX_CHARS + k) & 127u] & 31u : 0u; };      // never past the string
  auto field = [&](uint32_t k, uint32_t (&w)[8]) {
    if (k < n_fields) load(k, w);
    else { w[0] = w[1] = w[2] = w[3] = w[4] = w[5] = w[6] = w[7] = 0; }             // cannot happen: commit_measure counted them
  };
  uint32_t data_bits;
  const uint32_t flag = commit_measure(sym, kind, n_fields, field, data_bits);
  if (flag != COMMIT_OK) return flag;
  CommitWalk W{}; W.stage = CW_OWNER;
  emit(commit_hash([&](uint32_t (&w)[8], uint32_t& nbits) { return commit_next(W, sym, kind, field, data_bits, w, nbits); }, A.name_bits + 254u + 32u + data_bits + 253u, K, A));
  return COMMIT_OK;
}

}  // namespace aleo_mi355x
