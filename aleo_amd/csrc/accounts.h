// accounts.h — what accounts.hip shares with key_ciphertexts.hip, which opens private key ciphertexts into seeds on the device and has the account kernel derive
// the accounts of those seeds where they lie, and with signatures_sign.hip, which derives its key rows with the account lane: the layout of a chunk's buffer, the
// launch of k_accounts_derive over one, the account outputs a caller may ask for (on the device and on the host), the resident table, and the string a call returns.
#pragma once
#include "entry.h"
#include "account_host.hpp"

namespace aleo_mi355x {

static constexpr uint32_t ACC_BLOCK = 64;                    // one wave: a lane holds its whole account in registers, and small batches spread over the CUs
static constexpr size_t ACC_CHUNK = (size_t)1 << 20;         // accounts or candidates per launch
static constexpr uint32_t ACC_NONE = 0xffffffffu;            // an output the caller did not ask for

// A chunk's arrays lie in one device buffer, at these byte offsets (each below 2^32: ACC_CHUNK rows of at most 63 bytes), and the offsets themselves at its start:
// one base pointer, and the words a lane needs only at its end are read there and then instead of being held in scalar registers through the lane's phases, which
// have none to spare.  sk, view, addr, str: ACC_NONE where the output is not wanted.
struct AccChunk { uint32_t seeds, flags, sk, view, addr, str, n, pad; };

__device__ __forceinline__ void store_words8(char* p, const uint32_t (&w)[8]) {      // 32 bytes at p (16-byte aligned), by two 16-byte stores
  uint4* q = (uint4*)p;
  q[0] = make_uint4(w[0], w[1], w[2], w[3]); q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// accounts.hip: k_accounts_derive over the m accounts of the chunk at `base` (its AccChunk first), on stream s; dK: a resident table that begins with the account
// lane's words (account_lane.h AC_*).  The caller checks hipGetLastError.
void launch_accounts_derive(hipStream_t s, char* base, size_t m, const uint32_t* dK);
// accounts.hip: the account lane's table (account_lane.h AC_*) resident on the device
int32_t account_table(int device, const uint32_t** out);

// The account outputs of a call, n rows each, null where the caller did not ask: sk_sig, view key and address x of 32 bytes, the address string of 63 characters.
struct AccOut {
  uint8_t* sk; uint8_t* view; uint8_t* addr; char* str;
  bool any() const { return sk || view || addr || str; }
  // room for m rows of every output asked for, behind what cv holds; the offsets into C (ACC_NONE where not asked for)
  void carve(Carve& cv, AccChunk& C, size_t m) const {
    C.sk = sk ? (uint32_t)cv.part(m * 32) : ACC_NONE; C.view = view ? (uint32_t)cv.part(m * 32) : ACC_NONE; C.addr = addr ? (uint32_t)cv.part(m * 32) : ACC_NONE;
    C.str = str ? (uint32_t)cv.part(m * ACC_ADDRESS_CHARS) : ACC_NONE;
  }
  // queues the copies of the chunk's m rows at b (carved as C says) to rows at .. at + m of the caller's
  int32_t download(hipStream_t s, const char* b, const AccChunk& C, size_t at, size_t m) const {
    if (sk) HIPCHK(hipMemcpyAsync(sk + at * 32, b + C.sk, m * 32, hipMemcpyDeviceToHost, s));
    if (view) HIPCHK(hipMemcpyAsync(view + at * 32, b + C.view, m * 32, hipMemcpyDeviceToHost, s));
    if (addr) HIPCHK(hipMemcpyAsync(addr + at * 32, b + C.addr, m * 32, hipMemcpyDeviceToHost, s));
    if (str) HIPCHK(hipMemcpyAsync(str + at * ACC_ADDRESS_CHARS, b + C.str, m * ACC_ADDRESS_CHARS, hipMemcpyDeviceToHost, s));
    return ALEO_MI355X_OK;
  }
  // the host path's row i: the account of the seed, or zero rows and a zero string where the row is flagged already or the seed is refused; returns the flag
  uint8_t row_on_host(size_t i, const uint8_t* seed32, uint8_t flag) const {
    uint8_t ax[32] = {0};
    uint8_t* const sk_i = sk ? sk + 32 * i : nullptr; uint8_t* const view_i = view ? view + 32 * i : nullptr;
    if (flag) { for (uint8_t* p : {sk_i, view_i}) if (p) std::memset(p, 0, 32); }
    else flag = acct::derive_one_host(seed32, sk_i, view_i, ax);
    if (addr) std::memcpy(addr + 32 * i, ax, 32);
    if (str) { if (flag) std::memset(str + ACC_ADDRESS_CHARS * i, 0, ACC_ADDRESS_CHARS); else acct::address_string(str + ACC_ADDRESS_CHARS * i, ax); }
    return flag;
  }
};

// a string result of the C ABI with its terminator, or the refusal of a buffer too small for it
inline int32_t string_out(char* out, size_t cap, const std::string& s, const char* too_small) {
  if (s.size() + 1 > cap) return bad_arg(too_small);
  std::memcpy(out, s.c_str(), s.size() + 1);
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
