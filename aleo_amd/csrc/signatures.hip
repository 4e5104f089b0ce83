// signatures.hip — account signatures: sign, the sign1… string, and the verification of many signatures under many addresses in one call — the two account calls
// of the reference this library lacked (wasm/src/account/signature.rs:37-48 `Signature::sign` / `verify`, wasm/src/account/address.rs:69-71,
// wasm/src/account/private_key.rs:244-248, sdk/src/account.ts:195,211-213) — snarkVM 0.14.5 console/account/src/signature [UPSTREAM-RECALL]; what is pinned by the
// reference's data and what is UNPINNED: signature_host.hpp.
//
// The kernel (one signature per lane: signature_lane.h), its table (signature_host.hpp: 139 KB with the scan's constants, built on the host at first use and
// resident per device for the life of the process), the same flags on the host (signature_host.hpp verify_one_host — what small batches take, and the
// definition), the routing threshold, and the host-only calls: signing one message and the string.  (Signing in batches, on the device: signatures_sign.hip.)
#include "signatures.h"
#include "records_bits.hpp"
#include "signature_host.hpp"
#include <cstdlib>

namespace aleo_mi355x {

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------
static constexpr size_t SIG_CHUNK = (size_t)1 << 20;         // signatures per launch

// A chunk's arrays lie in one device buffer, at these byte offsets (each below 2^32: SIG_CHUNK signatures and SIG_CHUNK_BYTES of messages): one base pointer
// and five words in scalar registers instead of five pointers.
struct SigChunk { uint32_t flags, sigs, addr, addr_stride, text, off, n; };

// Signature i of the chunk: 128 bytes at sigs, its address at addr + i * addr_stride (0: one for all), its message the bytes off[i] .. off[i + 1] of text.
__global__ void __launch_bounds__(SIG_BLOCK) k_signatures_verify(char* base, SigChunk C, const uint32_t* K) {
  const uint32_t i = blockIdx.x * SIG_BLOCK + threadIdx.x;
  if (i >= C.n) return;                                        // no barrier and no wave-level operation below
  // every address is base + a 32-bit offset of the lane's own: the one pointer stays in scalar registers, the offsets in the lane's
  const uint32_t o_mine = C.sigs + i * 128u, o_addr = C.addr + i * C.addr_stride, o_flag = C.flags + i;
  const uint32_t first = *(const uint32_t*)(base + (C.off + 4u * i)), len = *(const uint32_t*)(base + (C.off + 4u * i + 4u)) - first;
  const uint32_t o_msg = C.text + first;
  base[o_flag] = (char)signature_verify_lane(
      [&](uint32_t k, uint32_t (&w)[8]) { load_words8(w, base + (k < 4 ? o_mine + 32u * k : o_addr)); },
      len, [&](uint32_t q) { return (uint8_t)base[o_msg + q]; }, K, [&] { base[o_flag] = (char)SIG_MALFORMED; });      // provisional: signature_lane.h phase()
}

// Chunk by chunk: the signatures, addresses and messages go up, one launch runs, the flags come down.  A message over the cap does not travel: its lane gets
// no bytes and the flag is set here.  The chunk's offsets and messages are declared outside the slot: they outlive the copies that read them.
static int32_t verify_on_device(uint8_t* flags, const uint8_t* sigs, const uint8_t* addresses, size_t address_stride, const uint8_t* messages, const uint64_t* offsets, size_t n) {
  const size_t cap = env_cap("ALEO_MI355X_SIGNATURES_CHUNK", SIG_CHUNK);
  std::vector<uint32_t> off; std::vector<uint8_t> text;
  return on_slot([&](Ctx* c) -> int32_t {
    const uint32_t* dK;
    if (int32_t rc = resident_table(c->device, ResidentTable::SIGNATURE, []() -> const std::vector<uint32_t>& { return sig::sig_tables().words; }, &dK)) return rc;
    hipStream_t s = c->stream;
    for (size_t lo = 0; lo < n;) {
      const size_t hi = cut_messages(text, off, messages, offsets, lo, n, cap, [&](size_t i) { return offsets[i + 1] - offsets[i] <= SIG_MAX_BYTES; });
      const size_t m = hi - lo, rows = address_stride ? m : 1;
      Carve cv;
      const size_t o_sig = cv.part(m * 128), o_addr = cv.part(rows * 32), o_text = cv.part(text.size()), o_off = cv.part((m + 1) * 4), o_fl = cv.part(m);
      if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
      char* b = c->scalars_stage.as<char>();
      HIPCHK(hipMemcpyAsync(b + o_sig, sigs + lo * 128, m * 128, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(b + o_addr, addresses + (address_stride ? lo * 32 : 0), rows * 32, hipMemcpyHostToDevice, s));
      if (!text.empty()) HIPCHK(hipMemcpyAsync(b + o_text, text.data(), text.size(), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(b + o_off, off.data(), (m + 1) * 4, hipMemcpyHostToDevice, s));
      const SigChunk C{(uint32_t)o_fl, (uint32_t)o_sig, (uint32_t)o_addr, address_stride ? 32u : 0u, (uint32_t)o_text, (uint32_t)o_off, (uint32_t)m};
      hipLaunchKernelGGL(k_signatures_verify, dim3((uint32_t)((m + SIG_BLOCK - 1) / SIG_BLOCK)), dim3(SIG_BLOCK), 0, s, b, C, dK);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(flags + lo, b + o_fl, m, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));                           // the next chunk reuses the buffers, and the host arrays above
      for (size_t i = lo; i < hi; ++i) if (offsets[i + 1] - offsets[i] > SIG_MAX_BYTES) flags[i] = (uint8_t)SIG_MALFORMED;
      lo = hi;
    }
    return ALEO_MI355X_OK;
  });
}

static int32_t signatures_verify(uint8_t* flags, const void* sigs128, const void* addresses_x32, size_t address_stride, const void* messages, const uint64_t* offsets, size_t n, bool may_route) {
  if (!n) return ALEO_MI355X_OK;
  if (!flags || !sigs128 || !addresses_x32) return bad_arg("signatures_verify: null buffer");
  if (address_stride != 0 && address_stride != 32) return bad_arg("signatures_verify: the address stride is 0 (one address) or 32 (one per signature)");
  if (int32_t rc = strings_args_ok("signatures_verify", (const char*)messages, offsets, n)) return rc;
  const uint8_t* sg = (const uint8_t*)sigs128; const uint8_t* ad = (const uint8_t*)addresses_x32; const uint8_t* ms = (const uint8_t*)messages;
  if (may_route && n >= aleo_mi355x_min_signatures()) return verify_on_device(flags, sg, ad, address_stride, ms, offsets, n);
  for (size_t i = 0; i < n; ++i) flags[i] = sig::verify_one_host(sg + 128 * i, ad + address_stride * i, ms + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
  return ALEO_MI355X_OK;
}

static int32_t signature_sign(void* out128, const char* private_key, const void* message, size_t len, const void* seed32) {
  if (!out128 || !seed32 || (len && !message)) return bad_arg("signature_sign: null buffer");
  if (len > SIG_MAX_BYTES) return bad_arg("signature_sign: the message exceeds the maximum of 4161 fields");
  uint8_t key_seed[32];
  if (int32_t rc = serial::private_key_seed(key_seed, private_key)) return rc;
  const sig::SignerKeys a = acct::signer_keys_of_seed(key_seed);
  uint64_t nonce[4]; sig::nonce_of_seed(nonce, (const uint8_t*)seed32);
  sig::sign_with_nonce((uint8_t*)out128, a, nonce, (const uint8_t*)message, len);
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The batch size from which a verification takes the GPU: the measured crossover against the host path on one thread, which is what a call below it runs
// (profiles/signatures_verify.txt: the GPU call takes 5.6-6.2 ms for any batch up to 2^10; the host path 3.75 ms for 2^4 signatures, 7.75 ms for 2^5)
size_t aleo_mi355x_min_signatures(void) { return env_size("ALEO_MI355X_MIN_SIGNATURES", (size_t)1 << 5); }

int32_t aleo_mi355x_signatures_verify(uint8_t* flags, const void* sigs128, const void* addresses_x32, size_t address_stride, const void* messages, const uint64_t* offsets, size_t n) {
  return guarded([&] { return signatures_verify(flags, sigs128, addresses_x32, address_stride, messages, offsets, n, true); });
}
int32_t aleo_mi355x_signatures_verify_host(uint8_t* flags, const void* sigs128, const void* addresses_x32, size_t address_stride, const void* messages, const uint64_t* offsets, size_t n) {
  return guarded([&] { return signatures_verify(flags, sigs128, addresses_x32, address_stride, messages, offsets, n, false); });
}

int32_t aleo_mi355x_signature_sign(void* out128, const char* private_key, const void* message, size_t len, const void* seed32) {
  return guarded([&] { return signature_sign(out128, private_key, message, len, seed32); });
}

int32_t aleo_mi355x_signature_to_string(char* out, size_t cap, const void* sig128) {
  return guarded([&] {
    if (!out || !sig128) return bad_arg("signature_to_string: null buffer");
    return aleo_mi355x_bech32m_encode(out, cap, "sign", sig128, 128);
  });
}
int32_t aleo_mi355x_signature_from_string(void* out128, const char* s) {
  return guarded([&] {
    if (!out128 || !s) return bad_arg("signature_from_string: null buffer");
    if (std::strlen(s) > 512) return bad_arg("signature_from_string: not a signature");
    uint8_t b[160]; size_t len = sizeof b; char hrp[8];
    if (int32_t rc = aleo_mi355x_bech32m_decode(b, &len, hrp, sizeof hrp, s)) return rc;
    if (std::strcmp(hrp, "sign") != 0) return bad_arg("signature_from_string: the prefix is not \"sign\"");
    if (len != 128) return bad_arg("signature_from_string: a signature has 128 bytes");
    std::memcpy(out128, b, 128);
    return ALEO_MI355X_OK;
  });
}

}  // extern "C"
