// signatures_sign.hip — account signatures in batches: one key signing many messages, or many keys signing one message each, in one call — Signature::sign of
// the reference (wasm/src/account/signature.rs:37-44, wasm/src/account/private_key.rs:92-96, sdk/src/account.ts:195), the one account call that ran one message at
// a time on one host thread (signatures.hip signature_sign, which derives the account on every call).  snarkVM 0.14.5 console/account/src/signature
// [UPSTREAM-RECALL]; what is pinned by the reference's data and what is UNPINNED: signature_host.hpp, inherited unchanged.
//
// The kernels (one signature per lane: signature_sign_lane.h; one key row per lane: account_lane.h with its sink), their table (the account lane's, which begins
// with the signature lane's words), the same bytes on the host (signature_host.hpp sign_with_nonce under nonce_of_seed — what small batches take, and the
// definition), the check that no nonce seed comes twice, and the routing threshold.
#include "accounts.h"
#include "signatures.h"
#include "records_bits.hpp"
#include "signature_host.hpp"
#include "signature_sign_lane.h"
#include <cstdlib>
#include <string>

namespace aleo_mi355x {

static constexpr size_t SIGN_CHUNK = (size_t)1 << 20;        // signatures per launch

// ---- the signing kernels ---------------------------------------------------------------------------------------------------------------------------------
// A signing chunk's arrays, as SigChunk: the flags (up: 0, or 3 where the host refuses the row; down: the same), the rows of 128 bytes, the key rows (sk_sig |
// pk_sig.x | pr_sig.x | address.x) key_stride apart (0: one for all; 128), the nonce seeds, the messages and their offsets.
struct SignChunk { uint32_t flags, sigs, keys, key_stride, seeds, text, off, n; };
struct KeysChunk { uint32_t seeds, keys, n; };

// Key row i of the chunk from the private-key seed at seeds + 32 i: account_lane with its sink.  A seed that is no field element leaves a row nobody reads (the
// host has flagged it).  The row's first byte is the provisional store of account_lane's phase(): sk_sig overwrites it at the end.  The row's address waits in
// two of the lane's registers, not the buffer's in two scalar ones (k_accounts_search does the same): the lane's phases have no scalar register to spare.
__global__ void __launch_bounds__(SIG_BLOCK) k_signer_keys(char* base, KeysChunk C, const uint32_t* K) {
  const uint32_t i = blockIdx.x * SIG_BLOCK + threadIdx.x;
  if (i >= C.n) return;                                        // no barrier and no wave-level operation below
  uint32_t seed[8];
  load_words8(seed, base + (C.seeds + 32u * i));
  const uintptr_t at = (uintptr_t)(base + (C.keys + 128u * i));
  uint32_t row_lo = (uint32_t)at, row_hi = (uint32_t)(at >> 32);
  ac_lane_word(row_lo); ac_lane_word(row_hi);
  char* const row = (char*)(((uintptr_t)row_hi << 32) | row_lo);
  AccountWords a;
  (void)account_lane(seed, K, a, [&] { row[0] = (char)0; }, [&](const F29& pkx, const F29& prx) {
    uint32_t w[8];
    f29_to_words(f29_canonical(pkx), w); store_words8(row + 32, w);
    f29_to_words(f29_canonical(prx), w); store_words8(row + 64, w);
  });
  store_words8(row, a.sk_sig);
  store_words8(row + 96, a.address);
}

// Signature i of the chunk: its nonce seed at seeds + 32 i, its key row at keys + i * key_stride, its message the bytes off[i] .. off[i + 1] of text; the flag
// byte it finds says whether the host refused the row.
__global__ void __launch_bounds__(SIG_BLOCK) k_signatures_sign(char* base, SignChunk C, const uint32_t* K) {
  const uint32_t i = blockIdx.x * SIG_BLOCK + threadIdx.x;
  if (i >= C.n) return;                                        // no barrier and no wave-level operation below
  const uint32_t o_mine = C.sigs + i * 128u, o_key = C.keys + i * C.key_stride, o_flag = C.flags + i;
  const uint32_t first = *(const uint32_t*)(base + (C.off + 4u * i)), len = *(const uint32_t*)(base + (C.off + 4u * i + 4u)) - first;
  const uint32_t o_msg = C.text + first;
  const uint32_t refused = (uint8_t)base[o_flag];
  uint32_t seed[8];
  load_words8(seed, base + (C.seeds + 32u * i));
  base[o_flag] = (char)signature_sign_lane(
      seed, [&](uint32_t k, uint32_t (&w)[8]) { load_words8(w, base + (o_key + 32u * k)); }, refused,
      len, [&](uint32_t q) { return (uint8_t)base[o_msg + q]; }, K,
      [&](uint32_t k, const uint32_t (&w)[8]) { store_words8(base + (o_mine + 32u * k), w); }, [&] { base[o_flag] = (char)SIGN_REFUSED; });      // provisional: signature_lane.h phase()
}

// ---- signing in batches ------------------------------------------------------------------------------------------------------------------------------------
static bool key_seed_ok(const uint8_t* seed32) { uint64_t v[4]; std::memcpy(v, seed32, 32); return !host::HFr::geq_p(v); }

// Two equal rows among n nonce seeds: an open-addressed table of row numbers under a hash of all 32 bytes, a full comparison on every occupied slot met.  The
// first pair in the order of the later row.  A batch of one kind of seed only (all equal but for a counter, say) costs the same as a random one.
static bool equal_seed_rows(const uint8_t* seeds, size_t n, size_t* first, size_t* second) {
  if (n < 2) return false;
  size_t cap = 4; while (cap < 2 * n) cap <<= 1;
  std::vector<uint32_t> slot(cap, 0xffffffffu);                // n <= 2^32 - 1 rows of 32 bytes: the call's own arrays could not hold more
  auto mix = [](uint64_t h) { h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33; return h; };
  for (size_t i = 0; i < n; ++i) {
    uint64_t w[4]; std::memcpy(w, seeds + 32 * i, 32);
    size_t at = (size_t)mix(mix(mix(mix(w[0]) ^ w[1]) ^ w[2]) ^ w[3]) & (cap - 1);
    for (; slot[at] != 0xffffffffu; at = (at + 1) & (cap - 1))
      if (!std::memcmp(seeds + 32 * (size_t)slot[at], seeds + 32 * i, 32)) { *first = slot[at]; *second = i; return true; }
    slot[at] = (uint32_t)i;
  }
  return false;
}

static void key_row_of(uint8_t* row128, const sig::SignerKeys& a) { std::memcpy(row128, a.sk_sig, 32); std::memcpy(row128 + 32, a.pk_x, 32); std::memcpy(row128 + 64, a.pr_x, 32); std::memcpy(row128 + 96, a.address_x, 32); }

// Chunk by chunk: the flags the host set (3 for a row it refuses), the key seeds or the one key row, the nonce seeds, the offsets and the messages go up; with a
// key each, k_signer_keys fills the key rows; k_signatures_sign runs; the rows and the flags come down.  A message over the cap does not travel.
static int32_t sign_on_device(uint8_t* sigs, uint8_t* flags, const uint8_t* key_seeds, const uint8_t* one_row, size_t key_stride, const uint8_t* messages, const uint64_t* offsets, const uint8_t* nonce_seeds, size_t n) {
  const size_t cap = env_cap("ALEO_MI355X_SIGN_CHUNK", SIGN_CHUNK);
  std::vector<uint32_t> off; std::vector<uint8_t> text;
  return on_slot([&](Ctx* c) -> int32_t {
    const uint32_t* dK;
    if (int32_t rc = account_table(c->device, &dK)) return rc;
    hipStream_t s = c->stream;
    for (size_t lo = 0; lo < n;) {
      const size_t hi = cut_messages(text, off, messages, offsets, lo, n, cap, [&](size_t i) { return !flags[i]; });
      const size_t m = hi - lo;
      Carve cv;
      const size_t o_sig = cv.part(m * 128), o_keys = cv.part(key_stride ? m * 128 : 128), o_kseed = cv.part(key_stride ? m * 32 : 0), o_seed = cv.part(m * 32);
      const size_t o_text = cv.part(text.size()), o_off = cv.part((m + 1) * 4), o_fl = cv.part(m);
      if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
      char* b = c->scalars_stage.as<char>();
      const uint32_t blocks = (uint32_t)((m + SIG_BLOCK - 1) / SIG_BLOCK);
      if (key_stride) {
        HIPCHK(hipMemcpyAsync(b + o_kseed, key_seeds + lo * 32, m * 32, hipMemcpyHostToDevice, s));
        const KeysChunk KC{(uint32_t)o_kseed, (uint32_t)o_keys, (uint32_t)m};
        hipLaunchKernelGGL(k_signer_keys, dim3(blocks), dim3(SIG_BLOCK), 0, s, b, KC, dK);
        HIPCHK(hipGetLastError());
      } else HIPCHK(hipMemcpyAsync(b + o_keys, one_row, 128, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(b + o_seed, nonce_seeds + lo * 32, m * 32, hipMemcpyHostToDevice, s));
      if (!text.empty()) HIPCHK(hipMemcpyAsync(b + o_text, text.data(), text.size(), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(b + o_off, off.data(), (m + 1) * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(b + o_fl, flags + lo, m, hipMemcpyHostToDevice, s));
      const SignChunk C{(uint32_t)o_fl, (uint32_t)o_sig, (uint32_t)o_keys, key_stride ? 128u : 0u, (uint32_t)o_seed, (uint32_t)o_text, (uint32_t)o_off, (uint32_t)m};
      hipLaunchKernelGGL(k_signatures_sign, dim3(blocks), dim3(SIG_BLOCK), 0, s, b, C, dK);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(sigs + lo * 128, b + o_sig, m * 128, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(flags + lo, b + o_fl, m, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));                           // the next chunk reuses the buffers, and the host arrays above
      lo = hi;
    }
    return ALEO_MI355X_OK;
  });
}

static int32_t signatures_sign(void* sigs128, uint8_t* flags, const void* key_seeds32, size_t key_stride, const void* messages, const uint64_t* offsets, const void* nonce_seeds32, size_t n, bool may_route) {
  if (!n) return ALEO_MI355X_OK;
  if (!sigs128 || !flags || !key_seeds32 || !nonce_seeds32 || !offsets) return bad_arg("signatures_sign: null buffer");
  if (key_stride != 0 && key_stride != 32) return bad_arg("signatures_sign: the key stride is 0 (one key) or 32 (one per signature)");
  if (n > 0xfffffffeull) return bad_arg("signatures_sign: too many signatures for one call");
  if (int32_t rc = strings_args_ok("signatures_sign", (const char*)messages, offsets, n)) return rc;
  uint8_t* out = (uint8_t*)sigs128; const uint8_t* ks = (const uint8_t*)key_seeds32; const uint8_t* ms = (const uint8_t*)messages; const uint8_t* ns = (const uint8_t*)nonce_seeds32;
  size_t a = 0, b = 0;
  if (equal_seed_rows(ns, n, &a, &b)) {
    g_last_error = "signatures_sign: nonce seeds " + std::to_string(a) + " and " + std::to_string(b) + " are equal (two signatures under one nonce give the private key away)";
    return ALEO_MI355X_ERR_BAD_ARG;
  }
  // what no lane signs: a key seed that is no field element, a message over the cap
  const bool one_ok = key_stride || key_seed_ok(ks);
  for (size_t i = 0; i < n; ++i)
    flags[i] = (uint8_t)((key_stride ? key_seed_ok(ks + 32 * i) : one_ok) && offsets[i + 1] - offsets[i] <= SIG_MAX_BYTES ? SIGN_OK : SIGN_REFUSED);
  sig::SignerKeys one; std::memset(&one, 0, sizeof one);
  if (!key_stride && one_ok) one = acct::signer_keys_of_seed(ks);      // one key: derived once, on the host, for either path
  if (may_route && n >= aleo_mi355x_min_sign()) {
    uint8_t one_row[128]; key_row_of(one_row, one);              // declared outside the slot: it outlives the copies that read it
    return sign_on_device(out, flags, ks, one_row, key_stride, ms, offsets, ns, n);
  }
  for (size_t i = 0; i < n; ++i) {
    if (flags[i]) { std::memset(out + 128 * i, 0, 128); continue; }
    uint64_t nonce[4]; sig::nonce_of_seed(nonce, ns + 32 * i);
    sig::sign_with_nonce(out + 128 * i, key_stride ? acct::signer_keys_of_seed(ks + 32 * i) : one, nonce, ms + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
  }
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The batch size from which a signing call takes the GPU: the measured crossover against the host path on one thread, which is what a call below it runs, in the
// mode that crosses later (profiles/signatures_sign.txt.  One key: the GPU call takes 2.4-2.7 ms for any batch up to 2^12; the host path 1.61 ms for 2^5
// signatures, 0.65x and 0.65x; 2.93 ms for 2^6, 1.23x and 1.22x.  A key each: the call takes 4.3-4.8 ms; the host path 5.61 ms for 2^4, 1.16x and 1.16x.  The
// parent's road, a loop of signature_sign, is behind the call from 2^4 on in both modes: 5.05 ms and 5.63 ms, 1.88x and 1.16x)
size_t aleo_mi355x_min_sign(void) { return env_size("ALEO_MI355X_MIN_SIGN", (size_t)1 << 6); }

int32_t aleo_mi355x_signatures_sign(void* sigs128, uint8_t* flags, const void* key_seeds32, size_t key_stride, const void* messages, const uint64_t* offsets, const void* nonce_seeds32, size_t n) {
  return guarded([&] { return signatures_sign(sigs128, flags, key_seeds32, key_stride, messages, offsets, nonce_seeds32, n, true); });
}
int32_t aleo_mi355x_signatures_sign_host(void* sigs128, uint8_t* flags, const void* key_seeds32, size_t key_stride, const void* messages, const uint64_t* offsets, const void* nonce_seeds32, size_t n) {
  return guarded([&] { return signatures_sign(sigs128, flags, key_seeds32, key_stride, messages, offsets, nonce_seeds32, n, false); });
}

}  // extern "C"
