// records_encrypt.hip — record plaintexts ENCRYPTED to the "record1…" strings a transition publishes: Record<N, Plaintext<N>>::encrypt(randomizer) and
// encrypt_symmetric_unchecked(record_view_key), which every execute, transfer, split and join of the reference runs for each output record
// (rust/src/program/execute.rs:74,177, rust/src/program/transfer.rs:99-106) — one string on the host, and n strings with n randomizers in one call on the GPU: what a
// service that prepares outputs for many recipients, a faucet, and this library's own soak and bench corpora need.  The other direction — parse, scan, decrypt,
// render — is records_strings.hip, records_found.hip and records_decrypt.hip.
//
// The host path (record_encrypt_host.hpp over plaintext_parse.hpp's parse tree) is the definition, what small batches take, what the lanes route, and the checker.
// The device flow per chunk of at most ALEO_MI355X_ENCRYPT_CHUNK strings, on one slot and one stream (records_encrypt_lane.h: why two lanes and not one):
//   text, offsets and randomizers go up
//   k_records_encrypt_keys   one string per lane, one wave per block: the measure walk, r G and the nonce, the owner's point, r Owner and the record view key; the
//                            flag, the row's number of characters (0 with a flag) and what the second walk needs
//   k_records_encrypt_sums   the first level of the exclusive sum of the characters (records_found.h block_exclusive2), k_found_offsets (records_found.hip) the second
//   — one read of 32 bytes: the characters in all, for which the output is sized, and how many rows the lane routed —
//   k_records_encrypt_text   one string per lane: the second walk, the squeeze, the symbol writer; every row's characters where the sums say
//   flags, record view keys, offsets and text come down; the rows the lane routed are encrypted or refused by the calling thread and spliced in.
// Flags: 0 encrypted; 1 mode 0 and x(r G) is not the string's nonce; 2 the randomizer is not below l or the owner's x has no point in the prime-order subgroup; 3 not
// a record plaintext.  A row with a flag has an empty string and a zero record view key.  Neither path is hardened against side channels.
#include "records_found.h"
#include "records_encrypt_lane.h"
#include "record_encrypt_host.hpp"

struct aleo_mi355x_encrypted { std::string text; std::vector<uint64_t> offsets; std::vector<uint8_t> flags, rvk; };

namespace aleo_mi355x {

using Encrypted = aleo_mi355x_encrypted;

static constexpr uint32_t ENC_BLOCK = 64;                          // one wave, as the signature kernels: a lane holds its points, and small batches spread over the CUs
static constexpr size_t ENC_CHUNK = (size_t)1 << 20;             // strings per launch
static const char* const ENC_INVALID = "The record plaintext string provided was invalid";

static thread_local size_t g_encrypt_routed = 0;

// A chunk's arrays lie in one device buffer at these byte offsets (signatures.hip: one base pointer and a few words in scalar registers); the output text in another.
struct EncChunk { uint32_t text, soff, rand, flags, info, lens, pos, blk, stat, nonce, rvk, goff, n, mode; };

// ---- the kernels ----------------------------------------------------------------------------------------------------------------------------------------------
// String i of the chunk: the characters soff[i] .. soff[i + 1] of text, its randomizer at rand + 32 i.  Writes flags[i], info[i], lens[i] (the row's characters),
// nonce and rvk rows; stat[2] counts the routed.
__global__ void __launch_bounds__(ENC_BLOCK) k_records_encrypt_keys(char* base, EncChunk C, const uint32_t* K) {
  const uint32_t i = blockIdx.x * ENC_BLOCK + threadIdx.x;
  if (i >= C.n) return;                                          // no barrier and no wave-level operation below
  const uint32_t first = *(const uint32_t*)(base + (C.soff + 4u * i)), len = *(const uint32_t*)(base + (C.soff + 4u * i + 4u)) - first;
  const uint32_t o_text = C.text + first, o_flag = C.flags + i;
  uint32_t rw[8]; load_words8(rw, base + (C.rand + 32u * i));
  ReMeasure R; uint32_t nonce[8], rvk[8];
  const uint32_t flag = records_encrypt_keys_lane([&](uint32_t q) { return q < len ? (uint32_t)(uint8_t)base[o_text + q] : 0u; }, len, rw, C.mode, K, R, nonce, rvk,
                                                  [&] { base[o_flag] = (char)RE_ROUTED; });      // provisional: signature_lane.h phase()
  base[o_flag] = (char)flag;
  *(uint32_t*)(base + (C.info + 4u * i)) = R.info;
  *(uint32_t*)(base + (C.lens + 4u * i)) = R.chars;
  uint4* n4 = (uint4*)(base + (C.nonce + 32u * i)); uint4* r4 = (uint4*)(base + (C.rvk + 32u * i));
  n4[0] = make_uint4(nonce[0], nonce[1], nonce[2], nonce[3]); n4[1] = make_uint4(nonce[4], nonce[5], nonce[6], nonce[7]);
  r4[0] = make_uint4(rvk[0], rvk[1], rvk[2], rvk[3]); r4[1] = make_uint4(rvk[4], rvk[5], rvk[6], rvk[7]);
  if (flag == RE_ROUTED) atomicAdd((uint32_t*)(base + C.stat) + 2, 1u);
}

// pos[i]: the characters of the block's rows before row i; blk: [characters | encrypted rows][block], the block totals k_found_offsets sums
__global__ void __launch_bounds__(FOUND_BLOCK) k_records_encrypt_sums(char* base, EncChunk C) {
  __shared__ uint32_t wave_tot[2][FOUND_BLOCK / 64];
  const uint32_t i = blockIdx.x * FOUND_BLOCK + threadIdx.x;
  const bool live = i < C.n;
  uint32_t a = live ? *(const uint32_t*)(base + (C.lens + 4u * i)) : 0u, b = live && base[C.flags + i] == 0 ? 1u : 0u, ta, tb;
  block_exclusive2(a, b, wave_tot, &ta, &tb);
  if (live) *(uint32_t*)(base + (C.pos + 4u * i)) = a;
  if (threadIdx.x == 0) { uint32_t* blk = (uint32_t*)(base + C.blk); blk[blockIdx.x] = ta; blk[gridDim.x + blockIdx.x] = tb; }
}

// Row i's characters at out + goff[i], goff[i] = blk[its block] + pos[i] (written for every row; goff[n] = total).  A row with a flag writes nothing.
__global__ void __launch_bounds__(ENC_BLOCK) k_records_encrypt_text(char* out, char* base, EncChunk C, uint32_t total, const uint32_t* K) {
  const uint32_t i = blockIdx.x * ENC_BLOCK + threadIdx.x;
  if (i >= C.n) return;                                          // no barrier and no wave-level operation below
  const uint32_t start = ((const uint32_t*)(base + C.blk))[i / FOUND_BLOCK] + *(const uint32_t*)(base + (C.pos + 4u * i));
  *(uint32_t*)(base + (C.goff + 4u * i)) = start;
  if (i == 0) *(uint32_t*)(base + (C.goff + 4u * C.n)) = total;
  // nothing wave-wide follows, so a row with a flag leaves here: a wave of computed rows does not walk for it
  if (base[C.flags + i] != 0) return;
  const uint32_t chars = *(const uint32_t*)(base + (C.lens + 4u * i));
  const uint32_t end = start + chars <= total ? start + chars : total;      // the sums are these rows': a guard, not a case
  const uint32_t first = *(const uint32_t*)(base + (C.soff + 4u * i)), len = *(const uint32_t*)(base + (C.soff + 4u * i + 4u)) - first;
  const uint32_t o_text = C.text + first;
  uint32_t nonce[8], rvk[8];
  load_words8(nonce, base + (C.nonce + 32u * i)); load_words8(rvk, base + (C.rvk + 32u * i));
  // Characters are gathered four to a word at their place in the output; a word that is all this row's is stored whole, the row's first and last few bytewise
  uint32_t at = start, word = 0;
  auto put = [&](uint32_t ch) {
    if (at >= end) return;
    word |= ch << (8u * (at & 3u));
    ++at;
    if ((at & 3u) == 0) {
      if (at - 4u >= start) *(uint32_t*)(out + (at - 4u)) = word;
      else for (uint32_t p = start; p < at; ++p) out[p] = (char)(word >> (8u * (p & 3u)));
      word = 0;
    }
  };
  const char prefix[RS_PREFIX_CHARS + 1] = "record1";
  for (uint32_t q = 0; q < RS_PREFIX_CHARS; ++q) put((uint32_t)(uint8_t)prefix[q]);
  records_encrypt_text_lane([&](uint32_t q) { return q < len ? (uint32_t)(uint8_t)base[o_text + q] : 0u; }, *(const uint32_t*)(base + (C.info + 4u * i)), nonce, rvk, K, put);
  const uint32_t tail = at & ~3u;
  for (uint32_t p = tail > start ? tail : start; p < at; ++p) out[p] = (char)(word >> (8u * (p & 3u)));
}

// ---- the host path ----------------------------------------------------------------------------------------------------------------------------------------------
static void append_row(Encrypted& E, size_t i, uint8_t flag, const std::string& s, const uint8_t* rvk32) {
  E.flags[i] = flag; std::memcpy(E.rvk.data() + 32 * i, rvk32, 32);
  E.text += s; E.offsets[i + 1] = E.text.size();
}

static void encrypt_on_host(Encrypted& E, const char* text, const uint64_t* offsets, size_t n, const uint8_t* randomizers, int mode) {
  std::string s; uint8_t rvk[32];
  for (size_t i = 0; i < n; ++i) {
    const uint8_t flag = renc::encrypt_one_host(s, rvk, text + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), randomizers + 32 * i, mode);
    append_row(E, i, flag, s, rvk);
  }
  g_encrypt_routed = n;
}

// ---- the device flow --------------------------------------------------------------------------------------------------------------------------------------------
// The staging vectors are declared outside the slot: they outlive the copies that read and write them.
static int32_t encrypt_on_device(Encrypted& E, const char* text, const uint64_t* offsets, size_t n, const uint8_t* randomizers, int mode) {
  const size_t cap = env_cap("ALEO_MI355X_ENCRYPT_CHUNK", ENC_CHUNK);
  std::vector<uint32_t> soff, goff; std::vector<uint8_t> flags; std::string dev_text, s;
  size_t routed = 0;
  const int32_t rc = on_slot([&](Ctx* c) -> int32_t {
    const uint32_t* dK;
    if (int32_t rc = resident_table(c->device, ResidentTable::SIGNATURE, []() -> const std::vector<uint32_t>& { return sig::sig_tables().words; }, &dK)) return rc;
    if (int32_t rc = ensure_host_pinned(c, 32)) return rc;
    const uint32_t* h_stat = (const uint32_t*)c->h_pinned;
    hipStream_t st = c->stream;
    for (size_t lo = 0; lo < n; lo += cap) {
      const size_t m = n - lo < cap ? n - lo : cap;
      const uint64_t chars = offsets[lo + m] - offsets[lo];
      if (chars > UINT32_MAX) return bad_arg("records_encrypt: more than 2^32 - 1 characters in one launch");
      soff.resize(m + 1);
      for (size_t i = 0; i <= m; ++i) soff[i] = (uint32_t)(offsets[lo + i] - offsets[lo]);
      const uint32_t nb = (uint32_t)((m + FOUND_BLOCK - 1) / FOUND_BLOCK);
      Carve cv;
      EncChunk C;
      C.text = (uint32_t)cv.part((size_t)chars); C.soff = (uint32_t)cv.part((m + 1) * 4); C.rand = (uint32_t)cv.part(m * 32); C.flags = (uint32_t)cv.part(m); C.info = (uint32_t)cv.part(m * 4);
      C.lens = (uint32_t)cv.part(m * 4); C.pos = (uint32_t)cv.part(m * 4); C.blk = (uint32_t)cv.part((size_t)nb * 8); C.stat = (uint32_t)cv.part(32); C.nonce = (uint32_t)cv.part(m * 32);
      C.rvk = (uint32_t)cv.part(m * 32); C.goff = (uint32_t)cv.part((m + 1) * 4); C.n = (uint32_t)m; C.mode = (uint32_t)mode;
      if (cv.total > 0xffffffffull) return bad_arg("records_encrypt: a launch's buffer passes 4 GiB");
      if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
      char* b = c->scalars_stage.as<char>();
      if (chars) HIPCHK(hipMemcpyAsync(b + C.text, text + offsets[lo], (size_t)chars, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(b + C.soff, soff.data(), (m + 1) * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(b + C.rand, randomizers + 32 * lo, m * 32, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(b + C.stat, 0, 32, st));
      hipLaunchKernelGGL(k_records_encrypt_keys, dim3((uint32_t)((m + ENC_BLOCK - 1) / ENC_BLOCK)), dim3(ENC_BLOCK), 0, st, b, C, dK);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(k_records_encrypt_sums, dim3(nb), dim3(FOUND_BLOCK), 0, st, b, C);
      HIPCHK(hipGetLastError());
      launch_found_offsets(st, (uint32_t*)(b + C.blk), (uint32_t*)(b + C.stat), nb, nb);      // stat[1]: the characters in all; stat[0]: the encrypted rows
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(c->h_pinned, b + C.stat, 32, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));                          // the one wait before the text: the host sizes the output
      const uint32_t total = h_stat[1], lane_routed = h_stat[2];
      if (int32_t rc = c->out_stage.reserve((size_t)total + 4)) return rc;
      char* dout = c->out_stage.as<char>();
      hipLaunchKernelGGL(k_records_encrypt_text, dim3((uint32_t)((m + ENC_BLOCK - 1) / ENC_BLOCK)), dim3(ENC_BLOCK), 0, st, dout, b, C, total, dK);
      HIPCHK(hipGetLastError());
      // no row was routed: the launch's text is the result's next characters as it stands; else it comes down aside and is spliced with the host's rows
      const size_t have = E.text.size();
      goff.resize(m + 1); flags.resize(m);
      char* h_text;
      if (lane_routed) { dev_text.resize(total); h_text = &dev_text[0]; } else { E.text.resize(have + total); h_text = &E.text[have]; }
      if (total) HIPCHK(hipMemcpyAsync(h_text, dout, total, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(goff.data(), b + C.goff, (m + 1) * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(flags.data(), b + C.flags, m, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(E.rvk.data() + 32 * lo, b + C.rvk, m * 32, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));                          // the next launch reuses the buffers and the staging vectors
      for (size_t i = 0; i < m; ++i) {
        if (flags[i] == RE_ROUTED) {                             // the calling thread: the rows the lane routed
          uint8_t rvk[32];
          const uint8_t flag = renc::encrypt_one_host(s, rvk, text + offsets[lo + i], (size_t)(offsets[lo + i + 1] - offsets[lo + i]), randomizers + 32 * (lo + i), mode);
          append_row(E, lo + i, flag, s, rvk);
        } else {
          E.flags[lo + i] = flags[i];
          if (lane_routed) E.text.append(dev_text, goff[i], goff[i + 1] - goff[i]);
          E.offsets[lo + i + 1] = lane_routed ? E.text.size() : have + goff[i + 1];
        }
      }
      routed += lane_routed;
    }
    return ALEO_MI355X_OK;
  });
  if (rc) return rc;
  g_encrypt_routed = routed;
  return ALEO_MI355X_OK;
}

static int32_t records_encrypt(Encrypted** out, const char* text, const uint64_t* offsets, size_t n, const void* randomizers32, int32_t mode, bool may_route) {
  g_encrypt_routed = 0;
  if (!out) return bad_arg("records_encrypt: null result pointer");
  *out = nullptr;
  if (mode != 0 && mode != ALEO_MI355X_ENCRYPT_SET_NONCE) return bad_arg("records_encrypt: unknown mode");
  if (n && !randomizers32) return bad_arg("records_encrypt: null randomizers");
  if (int32_t rc = strings_args_ok("records_encrypt", text, offsets, n)) return rc;
  if (n > UINT32_MAX) return bad_arg("records_encrypt: more than 2^32 - 1 strings");
  std::unique_ptr<Encrypted> E(new Encrypted);
  E->offsets.assign(n + 1, 0); E->flags.assign(n, 0); E->rvk.assign(n * 32, 0);
  if (may_route && n && n >= aleo_mi355x_min_encrypt()) { if (int32_t rc = encrypt_on_device(*E, text, offsets, n, (const uint8_t*)randomizers32, mode)) return rc; }
  else encrypt_on_host(*E, text, offsets, n, (const uint8_t*)randomizers32, mode);
  *out = E.release();
  return ALEO_MI355X_OK;
}

// what a one-record call says of a row's flag
static int32_t refuse_flag(const char* who, uint8_t flag) {
  if (flag == renc::ENC_NOT_A_RECORD) return bad_arg(ENC_INVALID);
  g_last_error = std::string(who) + (flag == renc::ENC_BAD_KEY ? ": the randomizer is not a scalar below the subgroup order, the key is not a field element, or the owner is no point of the subgroup"
                                                               : ": x(randomizer G) is not the string's nonce");
  return ALEO_MI355X_ERR_BAD_ARG;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The batch size from which records_encrypt takes the GPU: the measured crossover against the host twin on one thread (profiles/records_encrypt.txt: the GPU call takes
// 3.7-4.1 ms for any batch up to 2^12 strings and the host loop 0.15 ms a string: 2.41 ms for 2^4, 0.58x; 4.80 ms for 2^5, 1.16x)
size_t aleo_mi355x_min_encrypt(void) { return env_size("ALEO_MI355X_MIN_ENCRYPT", (size_t)1 << 5); }

size_t aleo_mi355x_records_encrypt_last_routed(void) { return g_encrypt_routed; }

int32_t aleo_mi355x_record_encrypt(const char* plaintext, const void* randomizer32, int32_t mode, char* out, size_t* out_len) {
  return guarded([&] {
    if (!plaintext || !randomizer32 || !out_len) return bad_arg("record_encrypt: null argument");
    if (mode != 0 && mode != ALEO_MI355X_ENCRYPT_SET_NONCE) return bad_arg("record_encrypt: unknown mode");
    std::string s; uint8_t rvk[32];
    if (const uint8_t flag = renc::encrypt_one_host(s, rvk, plaintext, std::strlen(plaintext), (const uint8_t*)randomizer32, mode)) return refuse_flag("record_encrypt", flag);
    return put_string(s, out, out_len, "record_encrypt");
  });
}

int32_t aleo_mi355x_record_encrypt_symmetric(const char* plaintext, const void* rvk32, char* out, size_t* out_len) {
  return guarded([&] {
    if (!plaintext || !rvk32 || !out_len) return bad_arg("record_encrypt_symmetric: null argument");
    std::string s;
    if (const uint8_t flag = renc::encrypt_symmetric_host(s, plaintext, std::strlen(plaintext), (const uint8_t*)rvk32)) return refuse_flag("record_encrypt_symmetric", flag);
    return put_string(s, out, out_len, "record_encrypt_symmetric");
  });
}

int32_t aleo_mi355x_record_nonce(void* out32, const void* randomizer32) {
  return guarded([&] {
    if (!out32 || !randomizer32) return bad_arg("record_nonce: null argument");
    uint64_t k[4]; std::memcpy(k, randomizer32, 32);
    if (sig::geq_l(k)) return bad_arg("record_nonce: the randomizer is not a scalar below the subgroup order");
    renc::nonce_of((uint8_t*)out32, k);
    return (int32_t)ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_records_encrypt(aleo_mi355x_encrypted** out, const char* text, const uint64_t* offsets, size_t n, const void* randomizers32, int32_t mode) {
  return guarded([&] { return records_encrypt(out, text, offsets, n, randomizers32, mode, true); });
}
int32_t aleo_mi355x_records_encrypt_host(aleo_mi355x_encrypted** out, const char* text, const uint64_t* offsets, size_t n, const void* randomizers32, int32_t mode) {
  return guarded([&] { return records_encrypt(out, text, offsets, n, randomizers32, mode, false); });
}
void aleo_mi355x_encrypted_free(aleo_mi355x_encrypted* e) { delete e; }
const char* aleo_mi355x_encrypted_text(const aleo_mi355x_encrypted* e) { return e ? e->text.data() : nullptr; }
const uint64_t* aleo_mi355x_encrypted_offsets(const aleo_mi355x_encrypted* e) { return e ? e->offsets.data() : nullptr; }
const uint8_t* aleo_mi355x_encrypted_flags(const aleo_mi355x_encrypted* e) { return e ? e->flags.data() : nullptr; }
const uint8_t* aleo_mi355x_encrypted_rvk(const aleo_mi355x_encrypted* e) { return e ? e->rvk.data() : nullptr; }

}  // extern "C"
