// key_ciphertexts.hip — private key ciphertexts: the encrypted form of a private key ("ciphertext1…", the reference's PrivateKeyCiphertext:
// wasm/src/account/private_key_ciphertext.rs:39-73, wasm/src/account/private_key.rs:102-130, rust/src/account/encryptor.rs:26-67), encrypted and decrypted one at a
// time on the host and OPENED in batches on the GPU: n (ciphertext, secret) pairs in, the seeds of their private keys and, where asked for, the accounts of those
// seeds out — what a front end holds per request (the development server decrypts its key ciphertext with the request's password on every deploy, execute and
// transfer: rust/develop/src/routes.rs:60-80) before it can call records_scan_many, records_unspent_* or signatures_verify.
//
//   k_key_ciphertexts_open   one pair per lane, one wave per block (key_ciphertext_lane.h): the string decoded from the block's span of the text, staged in LDS as
//                            the record strings are (records_strings.h stage_span), the secret packed, one width-9 and two width-3 permutations, the layout check,
//                            one inversion; writes the seed where k_accounts_derive reads it (32 x 0xff for a pair that does not open) and one flag byte.
//   k_accounts_derive        accounts.hip's, unchanged, behind it on the same stream over the same buffer when an account output is asked for: the seeds never come
//                            down unless the caller wants them.  The two lanes are not fused: account_lane alone takes every register a wave has.
// The host merges the flags (the open's wins where it is not 0) and zeroes the seed rows of flagged pairs.  The host path (key_ciphertext_host.hpp, account_host.hpp)
// is the definition, what small batches take, and the checker.
#include "accounts.h"
#include "records_strings.h"
#include "records_bits.hpp"
#include "key_ciphertext_host.hpp"
#include <algorithm>

namespace aleo_mi355x {

static constexpr uint32_t KC_BLOCK = ACC_BLOCK;                        // one wave, as the account kernels: the width-9 sponge and the string's walk leave no room for a second
static constexpr uint32_t KC_TEXT_LDS = 16 * 1024;                    // a block's span of text: 64 strings of 174 characters are 11 KB; a longer span is read from global memory
static constexpr uint32_t KC_SECRET_LDS = KC_BLOCK * KC_MAX_DEVICE_SECRET + 32;      // a block's secrets always fit

// The chunk's parts behind the AccChunk k_accounts_derive reads, at these byte offsets of the same buffer: the open's flags, the n + 1 chunk-relative offsets of the
// text and of the secrets, the text and the secrets (each readable up to the next multiple of 16 past its end)
struct KcChunk { AccChunk acc; uint32_t open_flags, text_off, secret_off, text, secrets, pad[3]; };

// Pair i of the chunk: its seed to acc.seeds + 32 i, its flag to open_flags + i.
__global__ void __launch_bounds__(KC_BLOCK) k_key_ciphertexts_open(char* base, uint32_t n, const uint32_t* K) {
  __shared__ uint4 stage_text[KC_TEXT_LDS / 16];
  __shared__ uint4 stage_secret[KC_SECRET_LDS / 16];
  const KcChunk* head = (const KcChunk*)base;
  const uint32_t b0 = blockIdx.x * KC_BLOCK;
  const char* text = base + head->text; const char* secrets = base + head->secrets;
  const uint32_t* toff = (const uint32_t*)(base + head->text_off); const uint32_t* soff = (const uint32_t*)(base + head->secret_off);
  uint32_t tlo, slo;
  const bool staged = stage_span<KC_BLOCK, KC_TEXT_LDS>(stage_text, text, toff, b0, n, &tlo);
  const bool sstaged = stage_span<KC_BLOCK, KC_SECRET_LDS>(stage_secret, secrets, soff, b0, n, &slo);
  const uint32_t i = b0 + threadIdx.x;
  if (i >= n) return;                                        // no barrier below
  const uint32_t o_flag = head->open_flags + i, o_seed = head->acc.seeds + 32u * i;
  const uint32_t first = toff[i], len = toff[i + 1] - first;
  // one walk for both sources: a pointer into LDS or into global memory, read with flat loads (two copies of the walk would be two sets of its masks)
  const uint8_t* mine = staged ? (const uint8_t*)stage_text + (first - tlo) : (const uint8_t*)text + first;
  uint32_t c[3][8];
  const uint32_t status = kc_decode([&](uint32_t j) { return mine[j]; }, len, c);
  const uint32_t sfirst = soff[i], slen = soff[i + 1] - sfirst;
  const uint8_t* secret = sstaged ? (const uint8_t*)stage_secret + (sfirst - slo) : (const uint8_t*)secrets + sfirst;
  uint32_t sw[8];
  kc_secret_words([&](uint32_t j) { return secret[j]; }, slen, sw);
  uint32_t seed[8];
  const uint32_t flag = key_ciphertext_lane(status, c, sw, K, seed, [&] { base[o_flag] = (char)KC_NO_CIPHERTEXT; });      // provisional: account_lane.h phase()
  store_words8(base + o_seed, seed);
  base[o_flag] = (char)flag;
}

static int32_t key_ciphertext_table(int device, const uint32_t** out) {
  return resident_table(device, ResidentTable::KEY_CIPHERTEXT, []() -> const std::vector<uint32_t>& { return kct::key_ciphertext_tables().words; }, out);
}

struct OpenOut { uint8_t* seeds; AccOut acc; uint8_t* flags; };

// ---- the host path --------------------------------------------------------------------------------------------------------------------------------------------------
static int32_t open_on_host(const char* text, const uint64_t* offsets, const uint8_t* secrets, const uint64_t* secret_offsets, size_t n, const OpenOut& o) {
  for (size_t i = 0; i < n; ++i) {
    uint8_t seed[32];
    const uint8_t flag = kct::open_one_host(seed, text + offsets[i], offsets[i + 1] - offsets[i], secrets + secret_offsets[i], (size_t)(secret_offsets[i + 1] - secret_offsets[i]));
    if (o.seeds) std::memcpy(o.seeds + 32 * i, seed, 32);
    if (o.flags) o.flags[i] = flag;
    if (o.acc.any()) (void)o.acc.row_on_host(i, seed, flag);      // a seed that was opened is below r: the flag stays the open's
  }
  return ALEO_MI355X_OK;
}

// ---- on the device --------------------------------------------------------------------------------------------------------------------------------------------------
// Chunk by chunk: text, secrets and offsets go up, the open kernel runs, the account kernel behind it where an account output is asked for, the rows asked for come
// down.  A chunk holds at most ALEO_MI355X_ACCOUNTS_CHUNK pairs and, unless it is one pair, at most the character cap of a record-string chunk.
static int32_t open_on_device(const char* text, const uint64_t* offsets, const uint8_t* secrets, const uint64_t* secret_offsets, size_t n, const OpenOut& o) {
  StringSource src{text, offsets, nullptr};                    // outside the slot: what the copies read outlives them
  src.cut_chunks(n, env_cap("ALEO_MI355X_ACCOUNTS_CHUNK", ACC_CHUNK));
  std::vector<uint32_t> trel, srel; std::vector<uint8_t> sblob, open_flags, derive_flags;
  KcChunk head;
  const bool accounts = o.acc.any();
  return on_slot([&](Ctx* c) -> int32_t {
    const uint32_t* dK;
    if (int32_t rc = key_ciphertext_table(c->device, &dK)) return rc;
    hipStream_t s = c->stream;
    for (size_t k = 0; k + 1 < src.cut.size(); ++k) {
      const size_t at = src.cut[k], m = src.cut[k + 1] - at;
      // the chunk's secrets as the kernel reads them, and the relative offsets of both blobs; a string over RS_MAX_CHARS travels as the empty one, refused alike
      trel.assign(m + 1, 0); srel.assign(m + 1, 0); sblob.clear();
      size_t pos = 0;
      for (size_t i = 0; i < m; ++i) {
        const uint64_t span = offsets[at + i + 1] - offsets[at + i];
        if (span <= RS_MAX_CHARS) pos += (size_t)span;
        trel[i + 1] = (uint32_t)pos;
        uint8_t sec[KC_MAX_DEVICE_SECRET];
        const uint32_t sl = kct::device_secret(sec, secrets + secret_offsets[at + i], (size_t)(secret_offsets[at + i + 1] - secret_offsets[at + i]));
        sblob.insert(sblob.end(), sec, sec + sl);
        srel[i + 1] = (uint32_t)sblob.size();
      }
      Carve cv;
      const size_t o_head = cv.part(sizeof(KcChunk)), o_seed = cv.part(m * 32), o_fl = cv.part(m), o_open = cv.part(m);
      head.acc = AccChunk{(uint32_t)o_seed, (uint32_t)o_fl, ACC_NONE, ACC_NONE, ACC_NONE, ACC_NONE, (uint32_t)m, 0u};
      o.acc.carve(cv, head.acc, m);
      const size_t o_toff = cv.part((m + 1) * 4), o_soff = cv.part((m + 1) * 4), o_text = cv.part(pos + 16), o_sec = cv.part(sblob.size() + 16);
      if (cv.total > 0xffffffffull) { g_last_error = "private_keys_open: a chunk's buffer passes 4 GiB"; return ALEO_MI355X_ERR_BAD_ARG; }
      if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
      char* b = c->scalars_stage.as<char>();
      // the text: runs of strings that go up in one copy; an over-long string ends a run
      {
        size_t run_dev = 0, dev = 0; uint64_t run_host = offsets[at];
        auto flush = [&](uint64_t host_end) -> int32_t {
          if (host_end > run_host) HIPCHK(hipMemcpyAsync(b + o_text + run_dev, text + run_host, (size_t)(host_end - run_host), hipMemcpyHostToDevice, s));
          return ALEO_MI355X_OK;
        };
        for (size_t i = 0; i < m; ++i) {
          const uint64_t span = offsets[at + i + 1] - offsets[at + i];
          if (span > RS_MAX_CHARS) { if (int32_t rc = flush(offsets[at + i])) return rc; run_host = offsets[at + i + 1]; run_dev = dev; }
          else dev += (size_t)span;
        }
        if (int32_t rc = flush(offsets[at + m])) return rc;
      }
      if (!sblob.empty()) HIPCHK(hipMemcpyAsync(b + o_sec, sblob.data(), sblob.size(), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(b + o_toff, trel.data(), (m + 1) * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(b + o_soff, srel.data(), (m + 1) * 4, hipMemcpyHostToDevice, s));
      head = KcChunk{head.acc, (uint32_t)o_open, (uint32_t)o_toff, (uint32_t)o_soff, (uint32_t)o_text, (uint32_t)o_sec, {0u, 0u, 0u}};
      HIPCHK(hipMemcpyAsync(b + o_head, &head, sizeof head, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_key_ciphertexts_open, dim3((uint32_t)((m + KC_BLOCK - 1) / KC_BLOCK)), dim3(KC_BLOCK), 0, s, b, (uint32_t)m, dK);
      HIPCHK(hipGetLastError());
      if (accounts) { launch_accounts_derive(s, b, m, dK); HIPCHK(hipGetLastError()); }
      open_flags.resize(m);
      HIPCHK(hipMemcpyAsync(open_flags.data(), b + o_open, m, hipMemcpyDeviceToHost, s));
      if (o.seeds) HIPCHK(hipMemcpyAsync(o.seeds + at * 32, b + o_seed, m * 32, hipMemcpyDeviceToHost, s));
      if (int32_t rc = o.acc.download(s, b, head.acc, at, m)) return rc;
      if (accounts) { derive_flags.resize(m); HIPCHK(hipMemcpyAsync(derive_flags.data(), b + o_fl, m, hipMemcpyDeviceToHost, s)); }
      HIPCHK(hipStreamSynchronize(s));                           // the next chunk reuses the buffer and the staging vectors
      for (size_t i = 0; i < m; ++i) {
        const uint8_t flag = open_flags[i];
        if (flag && o.seeds) std::memset(o.seeds + (at + i) * 32, 0, 32);
        if (o.flags) o.flags[at + i] = flag || !accounts ? flag : derive_flags[i];      // the open's flag wins where it is not 0; the account kernel's is 3 for every flagged pair
      }
    }
    return ALEO_MI355X_OK;
  });
}

static int32_t private_keys_open(const char* text, const uint64_t* offsets, const void* secrets, const uint64_t* secret_offsets, size_t n, void* seeds32, void* sk_sig32,
                                 void* view_key32, void* address_x32, char* address63, uint8_t* flags, bool may_route) {
  if (!n) return ALEO_MI355X_OK;
  if (int32_t rc = strings_args_ok("private_keys_open", text, offsets, n)) return rc;
  if (int32_t rc = strings_args_ok("private_keys_open", (const char*)secrets, secret_offsets, n)) return rc;
  const OpenOut o{(uint8_t*)seeds32, AccOut{(uint8_t*)sk_sig32, (uint8_t*)view_key32, (uint8_t*)address_x32, address63}, flags};
  if (may_route && n >= aleo_mi355x_min_key_ciphertexts()) return open_on_device(text, offsets, (const uint8_t*)secrets, secret_offsets, n, o);
  return open_on_host(text, offsets, (const uint8_t*)secrets, secret_offsets, n, o);
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The batch size from which private_keys_open takes the GPU: the measured crossover against the host path on one thread, the larger of the two ways to call it
// (profiles/key_ciphertexts.txt: with the seeds alone the GPU call takes 1.61-1.73 ms for any batch up to 2^12 and the host loop 46-48 us a pair: 0.73 ms for 2^4,
// 0.46x and 0.45x; 1.47 ms for 2^5, 0.91x and 0.91x; 3.00 ms for 2^6, 1.86x and 1.86x.  With every account output the call takes 3.8-4.4 ms and the host loop 221 us
// a pair: 3.55 ms for 2^4, 0.81x and 0.81x; 7.08 ms for 2^5, 1.62x and 1.61x: one step earlier)
size_t aleo_mi355x_min_key_ciphertexts(void) { return env_size("ALEO_MI355X_MIN_KEY_CIPHERTEXTS", (size_t)1 << 6); }

int32_t aleo_mi355x_private_keys_open(const char* text, const uint64_t* offsets, const void* secrets, const uint64_t* secret_offsets, size_t n, void* seeds32, void* sk_sig32,
                                      void* view_key32, void* address_x32, char* address63, uint8_t* flags) {
  return guarded([&] { return private_keys_open(text, offsets, secrets, secret_offsets, n, seeds32, sk_sig32, view_key32, address_x32, address63, flags, true); });
}
int32_t aleo_mi355x_private_keys_open_host(const char* text, const uint64_t* offsets, const void* secrets, const uint64_t* secret_offsets, size_t n, void* seeds32, void* sk_sig32,
                                           void* view_key32, void* address_x32, char* address63, uint8_t* flags) {
  return guarded([&] { return private_keys_open(text, offsets, secrets, secret_offsets, n, seeds32, sk_sig32, view_key32, address_x32, address63, flags, false); });
}

// No message of these two names a secret, a seed or a key.
int32_t aleo_mi355x_private_key_encrypt(char* out, size_t cap, const char* private_key, const void* secret, size_t secret_len, const void* nonce32) {
  return guarded([&] {
    if (!out || !private_key || !nonce32 || (!secret && secret_len)) return bad_arg("private_key_encrypt: null buffer");
    if (cap < KC_CHARS + 1) return bad_arg("private_key_encrypt: output buffer too small");
    uint8_t seed[32];
    if (serial::private_key_seed_or_why(seed, private_key)) return bad_arg("private_key_encrypt: not an Aleo private key");
    uint64_t nonce[4]; std::memcpy(nonce, nonce32, 32);
    if (host::HFr::geq_p(nonce)) return bad_arg("private_key_encrypt: the nonce is not a canonical field element");
    return string_out(out, cap, kct::encrypt_host(seed, (const uint8_t*)secret, secret_len, (const uint8_t*)nonce32), "private_key_encrypt: output buffer too small");
  });
}
int32_t aleo_mi355x_private_key_decrypt(char* out, size_t cap, const char* ciphertext, const void* secret, size_t secret_len) {
  return guarded([&] {
    if (!out || !ciphertext || (!secret && secret_len)) return bad_arg("private_key_decrypt: null buffer");
    uint8_t seed[32];
    const uint8_t flag = kct::open_one_host(seed, ciphertext, std::strlen(ciphertext), (const uint8_t*)secret, secret_len);
    if (flag == KC_NO_CIPHERTEXT) return bad_arg("private_key_decrypt: not a private key ciphertext string");
    if (flag) { g_last_error = "private_key_decrypt: the ciphertext does not decrypt under this secret"; return (int32_t)ALEO_MI355X_ERR_NOT_OWNER; }
    return string_out(out, cap, serial::private_key_string(seed), "private_key_decrypt: output buffer too small");
  });
}

}  // extern "C"
