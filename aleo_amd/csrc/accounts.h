// accounts.h — what accounts.hip shares with key_ciphertexts.hip, which opens private key ciphertexts into seeds on the device and has the account kernel derive
// the accounts of those seeds where they lie: the layout of a chunk's buffer and the launch of k_accounts_derive over one.
#pragma once
#include "entry.h"

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

}  // namespace aleo_mi355x
